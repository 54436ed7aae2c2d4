// The stand rule's column test (csrc/bisbm_stand_rule.hpp, the text the sweep kernel runs) against columns that are moved for
// real.  A stand-alone program: tests/test_stand_rule.py builds it with g++ and sanitizers and runs it.
//
// One case: a column of 3..32 blocks with entries 0..6, a draw x, a pass depth D in {4, 8}, and 1..D-1 earlier movers
// (r_i != s_i, 0 <= k_i <= the entry of row r_i at that moment) applied in order.  Step j's margins come from the column
// before the pass, packed the way the kernel packs them.  Whenever no mover shares a block with the target and column_clash
// keeps every pair, the target recomputed on the moved column must be the one the step read.  The two-steps rule
// (target_margin / target_moves) is exact for a single mover: it refuses iff the target really moves.
// A target's two margins add up to its entry - 1, so with entries <= 6 a pass of depth 8 (which needs 7 k <= margin) can keep no
// candidate at all: a second tier of columns with entries 0..48 runs the same check where depth 8 keeps some, also at the boundary.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bipartitesbm-mcmc_amd/csrc/bisbm_stand_rule.hpp"

using namespace bisbm;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*, uniform enough for a sampler
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545f4914f6cdd1dull) >> 33) % n);
}

// the first block whose running sum exceeds x, clamped to the last block (the kernel's inverse CDF)
static uint32_t target_of(const std::vector<uint32_t>& w, uint32_t x) {
    uint32_t S = 0;
    for (uint32_t b = 0; b < w.size(); ++b) {
        S += w[b];
        if (S > x) return b;
    }
    return (uint32_t)w.size() - 1u;
}

struct Mover {
    uint32_t r, s, k;
};

struct Tally {
    unsigned long long cases = 0, kept_cases = 0, kept_pairs = 0, refused_pairs = 0, kept_at_boundary = 0, refused_at_boundary = 0;
    unsigned long long wrong = 0, pair_cases = 0, pair_kept = 0, pair_refused = 0, pair_wrong = 0, packed_wrong = 0;
};

template <uint32_t D>
static void one_case(const std::vector<uint32_t>& w0, uint32_t x, Tally& t) {
    const uint32_t nb = (uint32_t)w0.size();
    std::vector<uint32_t> S(nb);
    uint32_t run = 0;
    for (uint32_t b = 0; b < nb; ++b) S[b] = (run += w0[b]);
    const uint32_t sp = target_of(w0, x);
    const uint32_t mup = margin_up(S[sp], w0[sp], x), mdn = margin_down(S[sp], x);
    const uint32_t margins = pack_margins(mup, mdn);
    if (packed_margin(margins, 0u) != mup || (x < run && packed_margin(margins, 1u) != mdn)) ++t.packed_wrong;
    if (x >= run && (int32_t)packed_margin(margins, 1u) >= 0) ++t.packed_wrong;  // a clamped target: mdn < 0 must stay negative

    // every other case is the rule's worst one: all D - 1 movers straddle the target in ONE direction, each with the largest k
    // the rule lets through (where its source row has that many edges left)
    const bool worst = rnd(2) != 0u && sp > 0u && sp + 1u < nb;
    const uint32_t worst_down = rnd(2);
    const uint32_t n_movers = worst ? D - 1u : 1u + rnd(D - 1u);
    std::vector<uint32_t> w = w0;
    bool all_kept = true;
    unsigned long long kept_here = 0, kept_at_boundary_here = 0;
    for (uint32_t i = 0; i < n_movers; ++i) {
        Mover m;
        if (worst) {
            const uint32_t below = rnd(sp), above = sp + 1u + rnd(nb - 1u - sp);
            m.r = worst_down ? below : above, m.s = worst_down ? above : below;
            const uint32_t most = (worst_down ? mdn : mup) / (D - 1u);
            m.k = w[m.r] < most ? w[m.r] : most;
            if (rnd(4) == 0u) m.k = rnd(w[m.r] + 1u);
        } else {
            m.r = rnd(nb);
            do m.s = rnd(nb); while (m.s == m.r);
            m.k = rnd(w[m.r] + 1u);
        }
        const bool shared = sp == m.r || sp == m.s;
        const uint32_t clash = column_clash<D>(m.r, m.s, sp, m.k, margins);
        const uint32_t candidate = column_clash_any(m.r, m.s, sp, m.k) & (shared ? 0u : 1u);
        if (candidate != 0u) {
            const uint32_t margin = m.r < m.s ? mdn : mup, need = (D - 1u) * m.k;
            if (clash != 0u) {
                ++t.refused_pairs;
                if (need == margin + 1u) ++t.refused_at_boundary;
            } else {
                ++kept_here;
                if (need == margin) ++kept_at_boundary_here;
            }
        }
        if (shared || clash != 0u) all_kept = false;
        w[m.r] -= m.k;  // the move itself, whatever the rule said: later movers see the column it leaves
        w[m.s] += m.k;
        if (i == 0u && !shared) {  // the two-steps rule on the first mover alone: exact
            ++t.pair_cases;
            const bool between = ((blocks_between(m.r, m.s) >> sp) & 1u) != 0u;
            const uint32_t down = m.r < m.s ? 1u : 0u;
            const uint32_t refuse = between ? target_moves(target_margin(down, down ? S[sp] : S[sp] - w0[sp], x), m.k) : 0u;
            const bool moved = target_of(w, x) != sp;
            refuse != 0u ? ++t.pair_refused : ++t.pair_kept;
            if ((refuse != 0u) != moved) ++t.pair_wrong;
        }
    }
    ++t.cases;
    if (all_kept) {
        ++t.kept_cases;
        t.kept_pairs += kept_here;  // (kept candidates count where the whole case was kept: those are the ones the target check covers)
        t.kept_at_boundary += kept_at_boundary_here;
        if (target_of(w, x) != sp) {
            if (t.wrong < 10)
                fprintf(stderr, "WRONG: D %u, %u blocks, x %u, target %u -> %u after %u movers\n", D, nb, x, sp, target_of(w, x), n_movers);
            ++t.wrong;
        }
    }
}

int main() {
    Tally t4, t8;
    for (uint32_t nb = 3; nb <= 32; ++nb) {
        for (uint32_t rep = 0; rep < 50u; ++rep) {
            std::vector<uint32_t> w(nb);
            uint32_t total = 0;
            const uint32_t top = rep < 40u ? 7u : 49u;  // entries 0..6, and the second tier
            // every third column sparse: many zero entries, i.e. equal neighbouring sums and small margins
            for (uint32_t b = 0; b < nb; ++b) total += (w[b] = rep % 3u == 0u ? (rnd(3) == 0u ? rnd(top) : 0u) : rnd(top));
            for (uint32_t x = 0; x <= total; ++x) {  // every draw; x == total: the clamped target
                one_case<4>(w, x, t4);
                one_case<8>(w, x, t8);
            }
        }
    }
    int rc = 0;
    const Tally* ts[2] = {&t4, &t8};
    for (int i = 0; i < 2; ++i) {
        const Tally& t = *ts[i];
        printf("D %d: cases %llu kept_cases %llu kept_pairs %llu refused_pairs %llu kept_at_boundary %llu refused_at_boundary %llu wrong %llu "
               "| two-steps rule: cases %llu kept %llu refused %llu wrong %llu | packing wrong %llu\n",
               i == 0 ? 4 : 8, t.cases, t.kept_cases, t.kept_pairs, t.refused_pairs, t.kept_at_boundary, t.refused_at_boundary, t.wrong,
               t.pair_cases, t.pair_kept, t.pair_refused, t.pair_wrong, t.packed_wrong);
        if (t.wrong != 0 || t.pair_wrong != 0 || t.packed_wrong != 0) rc = 1;
        if (t.kept_pairs == 0 || t.refused_pairs == 0 || t.kept_at_boundary == 0 || t.refused_at_boundary == 0 || t.pair_refused == 0) {
            fprintf(stderr, "NOT EXERCISED: D %d\n", i == 0 ? 4 : 8);
            rc = 2;
        }
    }
    return rc;
}
