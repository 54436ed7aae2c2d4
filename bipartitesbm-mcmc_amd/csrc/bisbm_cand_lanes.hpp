// bisbm_cand_lanes.hpp -- how the accumulate kernels of the ranked queries lay candidates over lanes and workgroups:
// query_scores_kernel (bisbm_query_scores.hip), coassign_count_kernel (bisbm_coassign.hip) and foldin_rows_kernel
// (bisbm_foldin.hip).  The candidates of a launch are the nodes first .. first + n_cand - 1.  A workgroup owns a candidate tile of
// 256 label words x a tile of queries; lane t of candidate tile c holds the four nodes of label word
// w = first / 4 + 256 c + t, so a lane reads its labels in a chain as one word (coalesced) whatever `first` is, and keeps a
// running cell per (query of the tile, node) in registers from the start of the kernel to its end.  No two workgroups share a
// cell.  What a kernel adds to the cells, and in which order, is its own; so are its loops that load and store them (one
// definition of those gave two of the three kernels another register allocation).
#pragma once

#include <algorithm>

#include "bisbm_kernels.hpp"

namespace bisbm {

constexpr uint32_t kCandLanes = 256;  // lanes of a workgroup = label words of a candidate tile

// the lane's four nodes; the ones outside the candidates are never looked up or stored
struct CandLanes {
    uint32_t w;     // the lane's label word: nodes 4 w .. 4 w + 3
    bool any;       // the word lies before the end of the candidates: it is read
    bool valid[4];  // node 4 w + j is a candidate
    __device__ __forceinline__ uint64_t node(uint32_t j) const { return (uint64_t)w * 4 + j; }
};

// (__forceinline__: after inlining the members are what the kernels' own locals were)
__device__ __forceinline__ CandLanes cand_lanes(uint32_t first, uint32_t n_cand, uint32_t cand_tile) {
    CandLanes c;
    c.w = (first >> 2) + cand_tile * kCandLanes + threadIdx.x;
    c.any = (uint64_t)c.w * 4 < (uint64_t)first + n_cand;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) c.valid[j] = c.node(j) >= first && c.node(j) < (uint64_t)first + n_cand;
    return c;
}

// Host: launch(cand_tiles, q_tile0, grid) for grids of workgroup = candidate tile + cand_tiles * query tile -- neighbours in the
// grid walk neighbouring stretches of the same label rows for the same queries --, as many tiles of `q_tile` of the n_list
// queries per launch as a one-dimensional grid holds (n_cand >= 1)
template <class F>
hipError_t for_cand_grids(uint64_t first, uint64_t n_cand, uint32_t n_list, uint32_t q_tile, F launch) {
    const uint64_t words = ((first + n_cand - 1) >> 2) - (first >> 2) + 1;
    const uint32_t cand_tiles = (uint32_t)((words + kCandLanes - 1) / kCandLanes);
    const uint32_t q_tiles = (n_list + q_tile - 1) / q_tile, per_launch = std::max(1u, (1u << 30) / cand_tiles);
    for (uint32_t q_tile0 = 0; q_tile0 < q_tiles; q_tile0 += per_launch) {
        launch(cand_tiles, q_tile0, dim3(cand_tiles * std::min(per_launch, q_tiles - q_tile0)));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace bisbm
