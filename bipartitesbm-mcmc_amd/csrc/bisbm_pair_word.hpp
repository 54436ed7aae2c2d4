// The pair word: what a four-steps pass on verified predictions needs of an earlier step to test one pair, built once per
// chunk by the feeder wave.
//
// No HIP in here: the sweep kernel calls these functions and tests/native/pair_word_check.cpp compiles the same text for
// the CPU and checks it against shared | column_clash (bisbm_stand_rule.hpp) on every input.
#pragma once

#include <cstdint>

#include "bisbm_stand_rule.hpp"

namespace bisbm {

// A pass commits step j behind step i = j - d only if both rows' scans found the targets the feeder predicted, so every input
// of the pair test but the margins of step j is known when the chunk is prepared: the own blocks r_i, r_j, the predicted targets
// s_i, s_j and k = k_i[t_j], the edges step i would move in the column step j reads.  One field of 10 bits per distance:
//     bits 0..7   k
//     bits 8..9   which margin the test asks:  0 mup (s_j strictly between, r_i > s_i: the sums rise),
//                                              1 mdn (strictly between, r_i < s_i: they drop),
//                                              2 none, a clash whatever the margin ({r_i, s_i} meets {r_j, s_j}),
//                                              3 none, no clash whatever the margin (no shared block, s_j not between).
// The four are one lookup: the packed margins (bisbm_stand_rule.hpp: margin + 1 in 15 bits, mup low, mdn high) with two
// constant fields on top -- 0, the negative margin that refuses whatever it is asked, and kMarginCap + 1, the margin that
// passes whatever it is asked ((D - 1) k <= 7 * 255) -- shifted by 16 times the selector.
constexpr uint32_t kPairFieldBits = 10u;
constexpr uint32_t kPairMarginsTop = (kMarginCap + 1u) << 16;  // selector 2: 0, selector 3: the cap

BISBM_RULE_FN uint32_t pair_word_field(uint32_t r_i, uint32_t s_i, uint32_t r_j, uint32_t s_j, uint32_t k_i_tj) {
    // (bit arithmetic, no short-circuit and no compare: a lane-divergent `?:` costs a mask round trip on the GPU)
    const uint32_t common = ((1u << r_i) | (1u << s_i)) & ((1u << r_j) | (1u << s_j));
    const uint32_t shared = common < 1u ? common : 1u;
    const uint32_t outside = ((blocks_between(r_i, s_i) >> s_j) & 1u) ^ 1u;
    const uint32_t down = (r_i - s_i) >> 31;  // r_i < s_i
    // shared: 2; else strictly between: down; else: 3
    const uint32_t sel = ((shared | outside) << 1) | ((shared ^ 1u) & (down | outside));
    return (k_i_tj & 0xffu) | (sel << 8);
}

// 0 / 1: step j must be evaluated again if step i moves.  margins_j: pack_margins of step j's own scan.
template <uint32_t D>
BISBM_RULE_FN uint32_t pair_clash(uint32_t field, uint32_t margins_j) {
    static_assert(D == 4u || D == 8u, "depth of a deep pass");
    const uint64_t table = ((uint64_t)kPairMarginsTop << 32) | margins_j;
    const uint32_t margin = ((uint32_t)(table >> ((field >> 4) & 0x30u)) & 0xffffu) - 1u;
    return target_moves(margin, (D - 1u) * (field & 0xffu));
}

// the three fields of a step (distance d at bits 10 (d - 1)) in one word
BISBM_RULE_FN uint32_t pair_word(uint32_t f1, uint32_t f2, uint32_t f3) { return f1 | (f2 << kPairFieldBits) | (f3 << (2u * kPairFieldBits)); }
BISBM_RULE_FN uint32_t pair_word_at(uint32_t word, uint32_t d) { return (word >> (kPairFieldBits * (d - 1u))) & ((1u << kPairFieldBits) - 1u); }

}  // namespace bisbm
