// The held word: which blocks of its own type a step's node may move to, as the production sweep kernel's feeder wave hands
// it to the stepping wave -- one rule for clamped nodes and for block constraints.
//
// No HIP in here: the sweep kernel calls these functions and tests/native/held_word_check.cpp compiles the same text for
// the CPU and checks it against a literal loop over cn_allows (bisbm_device.hpp).
#pragma once

#include <cstdint>

#include "bisbm_stand_rule.hpp"

namespace bisbm {

// Bit i of the word stands for local block i of the node's type (own0 + i as a global label; both block counts are <= 64 on
// the production kernel, so own0 <= 64 and k_own <= 64).
//   a clamped node:             0 -- every target is barred, its own block included: the step is one that was not accepted
//   a node under constraints:   its class's row of the bit table (eight 32-bit words, bit s <-> global label s) cut to the
//                               window [own0, own0 + k_own).  Setting constraints validates the labels, so the bit of the
//                               node's own block is set and r == s stays an accepted step
//   neither:                    all ones
constexpr uint32_t kHeldRowWords = 8;  // (kCnWords of bisbm_device.hpp)

// bits [own0, own0 + k_own) of a class's row, moved down to bit 0.  Reads row[own0 / 32 .. own0 / 32 + 2]: with own0 <= 64
// that is inside the row's eight words.
BISBM_RULE_FN uint64_t held_window(const uint32_t* row, uint32_t own0, uint32_t k_own) {
    const uint32_t w = own0 >> 5, sh = own0 & 31u;
    const uint64_t lo = ((uint64_t)row[w + 1u] << 32) | row[w];
    // (sh == 0: the third word contributes nothing, and a shift by 64 is not one)
    const uint64_t top = sh != 0u ? (uint64_t)row[w + 2u] << (64u - sh) : 0ull;
    const uint64_t bits = (lo >> sh) | top;
    const uint64_t keep = k_own >= 64u ? ~0ull : (1ull << k_own) - 1ull;
    return bits & keep;
}

// row: the class's row, or nullptr without constraints
BISBM_RULE_FN uint64_t held_word(bool clamped, const uint32_t* row, uint32_t own0, uint32_t k_own) {
    if (clamped) return 0ull;
    return row != nullptr ? held_window(row, own0, k_own) : ~0ull;
}

// 0 / 1: the target s_loc (a local block of the node's type, < 64) is barred
BISBM_RULE_FN uint32_t held_barred(uint64_t word, uint32_t s_loc) { return ((uint32_t)(word >> s_loc) & 1u) ^ 1u; }
// ... on the low half alone (both block counts <= 32: s_loc < 32)
BISBM_RULE_FN uint32_t held_barred32(uint32_t word_lo, uint32_t s_loc) { return ((word_lo >> s_loc) & 1u) ^ 1u; }

}  // namespace bisbm
