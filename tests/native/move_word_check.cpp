// CPU check of step_quad32's one-stage update of the register copies of m_r / n_r (csrc/bisbm_move_word.hpp): the text the
// sweep kernel runs, on a 64-lane wave modelled as an array, against the per-mover loop it replaced.
//
// The kernel's lane layout: four steps per pass, one per row of 16 lanes, two blocks per lane column (c and c + 16), the
// register copies lane <-> block mod 32, with 17..32 blocks.  Steps are drawn at random (blocks, r == s included, degrees from
// {1, 127, 128, 255}); for every subset `moved` of the steps whose members have r != s and pairwise disjoint block sets -- what
// the stand rule guarantees of committed movers -- every lane's m_r / n_r after the combined update must equal the loop's.
#include <cstdint>
#include <cstdio>

#include "../../bipartitesbm-mcmc_amd/csrc/bisbm_move_word.hpp"

using namespace bisbm;

struct Wave {
    int32_t v[64];
    Wave operator|(const Wave& o) const {
        Wave r;
        for (int l = 0; l < 64; ++l) r.v[l] = v[l] | o.v[l];
        return r;
    }
};
struct ModelSwaps {
    void swap16(const Wave& a, const Wave& b, Wave& x, Wave& y) const {
        Wave xo, yo;
        for (int l = 0; l < 64; ++l) {
            const int row = l >> 4, c = l & 15;
            xo.v[l] = (row & 1) ? b.v[16 * (row - 1) + c] : a.v[l];  // [a.r0, b.r0, a.r2, b.r2]
            yo.v[l] = (row & 1) ? b.v[l] : a.v[16 * (row + 1) + c];  // [a.r1, b.r1, a.r3, b.r3]
        }
        x = xo, y = yo;
    }
    void swap32(const Wave& a, const Wave& b, Wave& x, Wave& y) const {
        Wave xo, yo;
        for (int l = 0; l < 64; ++l) {
            xo.v[l] = l < 32 ? a.v[l] : b.v[l - 32];  // [a.lower, b.lower]
            yo.v[l] = l < 32 ? a.v[l + 32] : b.v[l];  // [a.upper, b.upper]
        }
        x = xo, y = yo;
    }
};

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33) % n;
}

struct Counts {
    unsigned long long cases = 0, wrong = 0, by_movers[5] = {0, 0, 0, 0, 0}, big_deg = 0;
};

// `blocks` own blocks, copies of m_r / n_r every 32 lanes, two blocks per column of 16 lanes
static void run(const char* name, uint32_t blocks, int rounds) {
    const uint32_t W = 4u, period = 32u;
    static const uint32_t degs[4] = {1u, 127u, 128u, 255u};
    const uint32_t L = 64u / W;
    Counts c;
    for (int it = 0; it < rounds; ++it) {
        uint32_t r[4], s[4], deg[4];
        // (every other round: steps on distinct blocks as far as they go, so that passes in which all steps move occur)
        const bool spread = (it & 1) != 0;
        uint32_t perm[32];
        for (uint32_t i = 0; i < blocks; ++i) perm[i] = i;
        for (uint32_t i = blocks - 1; i > 0; --i) {
            const uint32_t j = rnd(i + 1), t = perm[i];
            perm[i] = perm[j], perm[j] = t;
        }
        for (uint32_t g = 0; g < W; ++g) {
            r[g] = spread && 2 * g + 1 < blocks ? perm[2 * g] : rnd(blocks);
            s[g] = spread && 2 * g + 1 < blocks ? perm[2 * g + 1] : rnd(blocks);
            deg[g] = degs[rnd(4)];
        }
        int32_t mr0[32], nr0[32];
        for (uint32_t b = 0; b < blocks; ++b) mr0[b] = 1000 + (int32_t)rnd(100000), nr0[b] = 2 + (int32_t)rnd(1000);
        for (uint32_t moved = 0; moved < (1u << W); ++moved) {
            uint32_t used = 0, n_movers = 0;
            bool ok = true;
            for (uint32_t g = 0; g < W && ok; ++g)
                if ((moved >> g) & 1u) {
                    const uint32_t set = (1u << r[g]) | (1u << s[g]);
                    ok = r[g] != s[g] && (used & set) == 0u;
                    used |= set;
                    ++n_movers;
                }
            if (!ok) continue;
            // the loop: one mover at a time
            int32_t mr_ref[32], nr_ref[32];
            for (uint32_t b = 0; b < blocks; ++b) mr_ref[b] = mr0[b], nr_ref[b] = nr0[b];
            for (uint32_t g = 0; g < W; ++g)
                if ((moved >> g) & 1u) {
                    mr_ref[r[g]] -= (int32_t)deg[g], nr_ref[r[g]] -= 1;
                    mr_ref[s[g]] += (int32_t)deg[g], nr_ref[s[g]] += 1;
                    c.big_deg += deg[g] > 127u;
                }
            // the kernel's stage: every lane forms its step's words, the movers' survive, one combine, two adds
            Wave z_lo, z_hi;
            for (uint32_t l = 0; l < 64; ++l) {
                const uint32_t g = l / L, on = (moved >> g) & 1u;
                const uint32_t b_lo = l & 15u, b_hi = (l & 15u) + 16u;
                z_lo.v[l] = on ? move_word(r[g], s[g], deg[g], b_lo) : 0;
                z_hi.v[l] = on ? move_word(r[g], s[g], deg[g], b_hi) : 0;
            }
            const Wave z = combine_move_words(z_lo, z_hi, ModelSwaps{});
            bool good = true;
            for (uint32_t l = 0; l < 64; ++l) {
                const uint32_t b = l % period;
                const int32_t mr = (b < blocks ? mr0[b] : 0) + move_word_dm(z.v[l]), nr = (b < blocks ? nr0[b] : 0) + move_word_dn(z.v[l]);
                good = good && mr == (b < blocks ? mr_ref[b] : 0) && nr == (b < blocks ? nr_ref[b] : 0);
            }
            c.cases += 1, c.wrong += good ? 0 : 1, c.by_movers[n_movers] += 1;
        }
    }
    std::printf("%s: cases %llu wrong %llu big_degree_movers %llu movers", name, c.cases, c.wrong, c.big_deg);
    for (int i = 0; i <= 4; ++i) std::printf(" %llu", c.by_movers[i]);
    std::printf("\n");
}

int main() {
    run("quad32", 32, 20000);
    run("quad27", 27, 20000);
    run("quad20", 20, 20000);
    run("quad17", 17, 20000);
    return 0;
}
