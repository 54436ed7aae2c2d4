// The register copies of m_r / n_r after a four-steps pass with two blocks per lane column (step_quad32): one word per lane
// instead of one update per mover.
//
// No HIP in here: the sweep kernel calls these functions and tests/native/move_word_check.cpp compiles the same text for the
// CPU and checks it against the per-mover loop.
//
// A step that moves a node of degree deg from block r to block s adds +1 / +deg to n_r / m_r of s and -1 / -deg to those of r
// (apply_mcmc_moves, blockmodel.cc:461-503).  The steps of a pass that are committed AND move have pairwise disjoint block sets
// (the stand rule: a shared block is a clash), so at most one of them touches a given block and the pass's whole update of that
// block is that one step's contribution, or nothing.  Every row of lanes forms the contribution of ITS step to the lane's
// blocks before the verdicts are known (move_word); afterwards the words of the steps that do not move are zeroed and the rest
// is combined across the rows with a bitwise or (at most one is non-zero), and split into the two addends.
#pragma once

#include <cstdint>

#include "bisbm_stand_rule.hpp"

namespace bisbm {

// What the step (r -> s, degree deg in 1..255: a hot step's row fits the byte counters) adds to block b: the n_r addend in the
// low two bits (two's complement: 01, 11, 00), the m_r addend in the bits above.  (-4 deg + 3) >> 2 = -deg: the arithmetic shift
// rounds down.  Degrees above 127 are why the m_r addend is no signed byte.
BISBM_RULE_FN int32_t move_word(uint32_t r, uint32_t s, uint32_t deg, uint32_t b) {
    const int32_t at_s = (int32_t)((deg << 2) | 1u), at_r = (int32_t)((0u - (deg << 2)) | 3u);
    return b == s ? at_s : (b == r ? at_r : 0);
}
BISBM_RULE_FN int32_t move_word_dn(int32_t z) { return (int32_t)((uint32_t)z << 30) >> 30; }  // sign-extended bits 0..1
BISBM_RULE_FN int32_t move_word_dm(int32_t z) { return z >> 2; }

// The movers' words of a pass of four steps (one step per row of 16 lanes; the words of the other steps zeroed), combined so
// that every lane holds the word of the block its register copy of m_r / n_r stands for (lane <-> block mod 32).  V: one value
// per lane.  z_lo / z_hi: the words for the blocks that rows 0 / 2 and rows 1 / 3 of the wave hold in the lane's column: c, c + 16.
//   ops.swap16(a, b, x, y):   x = [a.r0, b.r0, a.r2, b.r2], y = [a.r1, b.r1, a.r3, b.r3]   (v_permlane16_swap)
//   ops.swap32(a, b, x, y):   x = [a.lower, b.lower], y = [a.upper, b.upper]               (v_permlane32_swap)
// After the first swap rows 0 / 2 hold z_lo of rows 0 | 1 and 2 | 3, rows 1 / 3 z_hi of the same; the second adds the other half.
template <class V, class Ops>
BISBM_RULE_FN V combine_move_words(V z_lo, V z_hi, const Ops& ops) {
    V x, y;
    ops.swap16(z_lo, z_hi, x, y);
    const V rows = x | y;
    ops.swap32(rows, rows, x, y);
    return x | y;
}

}  // namespace bisbm
