// The held word (csrc/bisbm_held_word.hpp, the text the production sweep kernel runs) against a literal loop over cn_allows, the
// generic kernel's look-up (csrc/bisbm_device.hpp, restated here: that header is HIP).  A stand-alone program:
// tests/test_held_word.py builds it with g++ and sanitizers and runs it.
//
// Every (ka, kb) in {1, 2, 31, 32, 33, 63, 64}^2, both types.  Classes of a table: 0 allows everything, then one class per
// block of the type that allows that block alone (local bit 0 and local bit k_own - 1 -- bit 63 at 64 blocks -- among them),
// then pseudo-random rows.  Every class is asked as an open node and as a clamped one, and without any table.  The bits of the
// row outside the type's window are set at random: the window must cut them off.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../bipartitesbm-mcmc_amd/csrc/bisbm_held_word.hpp"

using namespace bisbm;

static bool cn_allows(const uint32_t* bits, uint32_t cls, uint32_t s) { return ((bits[cls * kHeldRowWords + (s >> 5)] >> (s & 31u)) & 1u) != 0u; }

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

struct Tally {
    unsigned long long words = 0, targets = 0, wrong = 0, bit0 = 0, bit63 = 0, all_class = 0, one_block = 0, clamped_all = 0, barred = 0, allowed = 0,
                       third_word = 0;
};

static void check_word(Tally& t, uint64_t word, bool clamped, const uint32_t* bits, uint32_t cls, uint32_t own0, uint32_t k_own) {
    ++t.words;
    for (uint32_t s_loc = 0; s_loc < 64u; ++s_loc) {
        // the literal rule: a clamped node may go nowhere; a node under a table where its class allows; a free node anywhere
        // (targets past the type's blocks do not exist: the word may hold anything there only where no table cuts it)
        bool want_allowed;
        if (clamped)
            want_allowed = false;
        else if (bits != nullptr)
            want_allowed = s_loc < k_own && cn_allows(bits, cls, own0 + s_loc);
        else
            want_allowed = true;
        const uint32_t got = held_barred(word, s_loc);
        ++t.targets;
        if (got != (want_allowed ? 0u : 1u)) {
            if (t.wrong < 10) fprintf(stderr, "WRONG: own0 %u k_own %u class %u clamped %d target %u: barred %u\n", own0, k_own, cls, (int)clamped, s_loc, got);
            ++t.wrong;
        }
        if (s_loc < 32u && held_barred32((uint32_t)word, s_loc) != got) ++t.wrong;
        got ? ++t.barred : ++t.allowed;
        if (!clamped && bits != nullptr && want_allowed && s_loc == 0u) ++t.bit0;
        if (!clamped && bits != nullptr && want_allowed && s_loc == 63u) ++t.bit63;
    }
}

int main() {
    static const uint32_t ks[7] = {1u, 2u, 31u, 32u, 33u, 63u, 64u};
    Tally t;
    for (uint32_t ia = 0; ia < 7u; ++ia)
        for (uint32_t ib = 0; ib < 7u; ++ib) {
            const uint32_t ka = ks[ia], kb = ks[ib];
            for (uint32_t type = 0; type < 2u; ++type) {
                const uint32_t own0 = type ? ka : 0u, k_own = type ? kb : ka;
                const uint32_t n_random = 8u, n_classes = 1u + k_own + n_random;
                std::vector<uint32_t> bits((size_t)n_classes * kHeldRowWords);
                for (auto& w : bits) w = rnd();  // (every bit outside the window: noise)
                auto set_bit = [&](uint32_t cls, uint32_t s, bool on) {
                    uint32_t& w = bits[cls * kHeldRowWords + (s >> 5)];
                    w = on ? (w | (1u << (s & 31u))) : (w & ~(1u << (s & 31u)));
                };
                for (uint32_t i = 0; i < k_own; ++i) {
                    set_bit(0, own0 + i, true);                                               // class 0: everything
                    for (uint32_t j = 0; j < k_own; ++j) set_bit(1u + i, own0 + j, i == j);  // class 1 + i: block i alone
                }
                for (uint32_t cls = 0; cls < n_classes; ++cls)
                    for (int clamped = 0; clamped < 2; ++clamped) {
                        const uint64_t word = held_word(clamped != 0, bits.data() + (size_t)cls * kHeldRowWords, own0, k_own);
                        check_word(t, word, clamped != 0, bits.data(), cls, own0, k_own);
                        if (cls == 0u && !clamped) ++t.all_class;
                        if (cls == 0u && clamped) ++t.clamped_all;
                        if (cls >= 1u && cls <= k_own && !clamped) {
                            ++t.one_block;
                            if (word != 1ull << (cls - 1u)) ++t.wrong;
                        }
                        if ((own0 & 31u) != 0u && own0 + k_own > ((own0 >> 5) + 2u) * 32u) ++t.third_word;
                    }
                for (int clamped = 0; clamped < 2; ++clamped)  // no table at all
                    check_word(t, held_word(clamped != 0, nullptr, own0, k_own), clamped != 0, nullptr, 0u, own0, k_own);
            }
        }
    printf("words %llu targets %llu wrong %llu barred %llu allowed %llu bit0 %llu bit63 %llu all_class %llu one_block %llu clamped_all %llu third_word %llu\n",
           t.words, t.targets, t.wrong, t.barred, t.allowed, t.bit0, t.bit63, t.all_class, t.one_block, t.clamped_all, t.third_word);
    if (t.wrong != 0) return 1;
    if (t.bit0 == 0 || t.bit63 == 0 || t.all_class == 0 || t.one_block == 0 || t.clamped_all == 0 || t.barred == 0 || t.allowed == 0 || t.third_word == 0) {
        fprintf(stderr, "NOT EXERCISED\n");
        return 2;
    }
    return 0;
}
