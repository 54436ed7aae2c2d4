// BISBM_PREDICT_SKEW on the CPU: the text the host and the feeder wave run (csrc/bisbm_predict_skew.hpp).
//   * unset, empty, "0" and text without a number leave SweepParams::predict_skew at 0, and with 0 every step keeps its prediction;
//   * with n > 0 exactly the steps n - 1, 2 n - 1, ... of a chunk get another block, in range, the next one modulo k_own.
#include "../../bipartitesbm-mcmc_amd/csrc/bisbm_predict_skew.hpp"

#include <cstdio>
#include <initializer_list>

using namespace bisbm;

int main() {
    unsigned wrong = 0, cases = 0, skewed = 0;
    auto expect = [&](bool ok, const char* what) {
        ++cases;
        if (!ok) {
            ++wrong;
            std::printf("FAIL %s\n", what);
        }
    };
    expect(predict_skew_from_env(nullptr) == 0u, "unset");
    expect(predict_skew_from_env("") == 0u, "empty");
    expect(predict_skew_from_env("0") == 0u, "0");
    expect(predict_skew_from_env("x") == 0u, "no number");
    expect(predict_skew_from_env("1") == 1u, "1");
    expect(predict_skew_from_env("3") == 3u, "3");
    expect(predict_skew_from_env("64") == 64u, "64");
    expect(predict_skew_from_env("99999999999999") == 0xffffffffu, "clamped");
    for (uint32_t k_own = 1; k_own <= 64; ++k_own)
        for (uint32_t pred = 0; pred < k_own; ++pred)
            for (uint32_t step = 0; step < 64; ++step) {
                expect(skewed_prediction(pred, step, 0u, k_own) == pred, "skew 0 changes nothing");
                for (uint32_t n : {1u, 2u, 3u, 4u, 7u, 64u, 65u, 0xffffffffu}) {
                    const uint32_t got = skewed_prediction(pred, step, n, k_own);
                    const bool hit = step % n == n - 1u;
                    skewed += hit ? 1u : 0u;
                    expect(got < k_own, "in range");
                    expect(got == (hit ? (pred + 1u) % k_own : pred), "the next block on the n-th steps only");
                }
            }
    std::printf("predict_skew: cases %u wrong %u skewed %u\n", cases, wrong, skewed);
    return wrong == 0 ? 0 : 1;
}
