// The stand rule's column test: does an earlier step's move change a later step's inverse-CDF target?
//
// No HIP in here: the sweep kernel calls these functions and tests/native/stand_rule_check.cpp compiles the same text for
// the CPU and checks it against columns it moves for real.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BISBM_RULE_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define BISBM_RULE_FN inline
#endif

namespace bisbm {

// A later step's inverse-CDF target s' (the first block whose running sum S exceeds its draw x) lies strictly between the
// blocks r and s of an earlier step that moves k of the column's edges from row r to row s.  Both S_{s'-1} and S_{s'} then move
// by k: down when r < s (down = 1, edge = S_{s'}), up when r > s (down = 0, edge = S_{s'-1}).  The margin is how far they may
// move with s' still the target: S_{s'} - 1 - x = ~(x - S_{s'}), or x - S_{s'-1}; both >= 0, and the target holds iff k <= margin.
BISBM_RULE_FN uint32_t target_margin(uint32_t down, uint32_t edge, uint32_t x) { return (x - edge) ^ (0u - down); }
// k > margin as a 0 / 1 word (both < 2^31: column sums are edge counts)
BISBM_RULE_FN uint32_t target_moves(uint32_t margin, uint32_t k) { return (margin - k) >> 31; }

// ---- passes of depth D = 4 or 8: up to D - 1 earlier steps may move before step j is committed ----
// Step j read column t_j on the state before the pass: running sums S_b (S_{-1} = 0), entries w_b = S_b - S_{b-1}, draw x,
// target s' with S_{s'-1} <= x < S_{s'}.  Its two margins, from what the lane of block s' holds (S_{s'} and w_{s'}):
//     mup = x - S_{s'-1} = x - (S_{s'} - w_{s'})        how far the two sums may RISE with s' still the target,
//     mdn = S_{s'} - 1 - x                              how far they may DROP;
// both are >= 0.  (A clamped target -- no sum exceeds x, s' = the last block -- has mdn < 0; the last block is never strictly
// between two others, and a negative margin refuses whatever it is asked.)
BISBM_RULE_FN uint32_t margin_up(uint32_t S, uint32_t w, uint32_t x) { return x - (S - w); }
BISBM_RULE_FN uint32_t margin_down(uint32_t S, uint32_t x) { return S - 1u - x; }
// Both margins in one word, so that a pair lane fetches them in one read: each as margin + 1 clamped to [0, 0x7fff] (mup in the low
// half, mdn in the high half).  0 stands for every negative margin; the largest k a step can move is a byte-sized neighbour count,
// so (D - 1) k <= 7 * 255 = 1785 and a margin clamped at 0x7ffe still passes whatever it is asked.
constexpr uint32_t kMarginCap = 0x7ffeu;
BISBM_RULE_FN uint32_t margin_field(uint32_t margin) {
    const int32_t m = (int32_t)margin;
    return (uint32_t)(m < -1 ? -1 : (m > (int32_t)kMarginCap ? (int32_t)kMarginCap : m)) + 1u;
}
BISBM_RULE_FN uint32_t pack_margins(uint32_t mup, uint32_t mdn) { return margin_field(mup) | (margin_field(mdn) << 16); }
// the margin of one direction out of the packed word (down = 1: mdn), -1 for a negative one
BISBM_RULE_FN uint32_t packed_margin(uint32_t margins, uint32_t down) { return ((margins >> (down << 4)) & 0xffffu) - 1u; }

// blocks strictly between r and s, as a bit mask (blocks < 32)
BISBM_RULE_FN uint32_t blocks_between(uint32_t r, uint32_t s) {
    const uint32_t lo = r < s ? r : s, hi = r < s ? s : r;
    return ((1u << hi) - 1u) & ~((2u << lo) - 1u);
}

// An earlier step i that moves k = k_i[t_j] edges of the column from row r_i to row s_i changes the sums S_b for b in
// [min(r_i, s_i), max(r_i, s_i)) only: by -k if r_i < s_i, by +k otherwise.  So a target outside (min, max) keeps both of its
// sums (a target AT r_i or s_i is a shared block, which stays a clash as it is), and a target strictly between has both shifted
// by the same amount.  The pair (i, j) is no column clash iff
//     (D - 1) k <= mdn   for a downward shift (r_i < s_i),        (D - 1) k <= mup   for an upward one.
// Sufficient for ANY set of earlier movers that all pass: at most D - 1 of them move, each downward one contributes
// k <= mdn / (D - 1) and each upward one k <= mup / (D - 1), so the downward shifts sum to at most mdn and the upward ones to
// at most mup, whatever the order and the mix.  The shifted sums obey S'_{s'-1} <= S_{s'-1} + mup = x and
// S'_{s'} >= S_{s'} - mdn = x + 1 > x: s' is still the first block whose sum exceeds x.  The sums stay monotone (they are sums
// of entries >= 0 of a valid state) and the column total does not change, so neither does the last-block clamp.
// The test is pairwise -- it never looks at which other steps move -- so the commit chains that combine the pairs stay as they are.
// Returns 0 / 1: 1 = step j must be evaluated again if step i moves.  k = 0 moves nothing.
template <uint32_t D>
BISBM_RULE_FN uint32_t column_clash(uint32_t r_i, uint32_t s_i, uint32_t s_j, uint32_t k, uint32_t margins) {
    static_assert(D == 4u || D == 8u, "depth of a deep pass");
    const uint32_t down = (r_i - s_i) >> 31;  // r_i < s_i
    const uint32_t need = (D - 1u) * k;       // (k = 0: 0 <= margin)
    return (blocks_between(r_i, s_i) >> s_j) & target_moves(packed_margin(margins, down), need);
}
// the rule before the margins: every target strictly between r_i and s_i falls when k != 0 (kept for a pass that cannot hold
// the margins in registers)
BISBM_RULE_FN uint32_t column_clash_any(uint32_t r_i, uint32_t s_i, uint32_t s_j, uint32_t k) {
    return (blocks_between(r_i, s_i) >> s_j) & (k != 0u ? 1u : 0u);
}

}  // namespace bisbm
