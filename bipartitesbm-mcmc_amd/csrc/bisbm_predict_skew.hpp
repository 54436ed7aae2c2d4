// The predicted target of a step, where a test bends it.
//
// The feeder wave predicts each step's inverse-CDF target a chunk ahead (bisbm_sweep_fast.hip, prepare); the passes that start
// from it check it against their own scan before anything is written, so ANY prediction gives the same chain.  A product build
// cannot make a miss happen: BISBM_PREDICT_SKEW = n hands every n-th step of a chunk a wrong one.
//
// No HIP in here: the sweep kernel and the host call these functions and tests/native/predict_skew_check.cpp compiles the same
// text for the CPU.
#pragma once

#include <cstdint>
#include <cstdlib>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BISBM_SKEW_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define BISBM_SKEW_FN inline
#endif

namespace bisbm {

// BISBM_PREDICT_SKEW as SweepParams::predict_skew: unset, empty, 0 or no number -> 0 (nothing changes)
inline uint32_t predict_skew_from_env(const char* value) {
    if (value == nullptr) return 0u;
    const unsigned long long n = strtoull(value, nullptr, 10);
    return n > 0xffffffffull ? 0xffffffffu : (uint32_t)n;
}

// What the feeder hands step `step_in_chunk` (0..63) as its predicted target: the prediction, or -- skew = n > 0 and the step's
// index is n - 1 modulo n -- the next block, (prediction + 1) mod k_own: in range, and wrong unless the type has a single block.
BISBM_SKEW_FN uint32_t skewed_prediction(uint32_t prediction, uint32_t step_in_chunk, uint32_t skew, uint32_t k_own) {
    if (skew == 0u || step_in_chunk % skew != skew - 1u) return prediction;
    return prediction + 1u < k_own ? prediction + 1u : 0u;
}

}  // namespace bisbm
