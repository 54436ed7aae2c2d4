// bisbm_partition_device.hpp -- what the units that count contingency tables share on the device (bisbm_partition.hip: chains with
// chains, chains with references; bisbm_trace.hip: chains with their own snapshots): the description of a partition, the one
// count into a cell, the one order in which a table is reduced, and A = sum_r a_r ln a_r of a partition.  One definition each, so
// that the same integers give the same bits in both units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bisbm {
namespace {

struct ChainDesc {
    const uint8_t* row;  // n labels (readable up to the next multiple of 4)
    uint32_t ka, kb;
};

constexpr uint32_t kNone = 0xffffffffu;

// sum of x ln x over a table by one wave, in an order fixed by `cells`: lane l adds cells l, l + 64, ... in turn, then a
// butterfly over the lanes (every lane ends with the same bits)
__device__ double wave_xlnx(const uint32_t* t, uint32_t cells, uint32_t lane) {
    double s = 0.;
    for (uint32_t i = lane; i < cells; i += 64) {
        const uint32_t x = t[i];
        if (x > 1u) {
            const double d = (double)x;
            s += d * log(d);
        }
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// one count into cell idx (kNone: nothing) by every lane of a converged wave: the lanes that share the first lane's cell add
// once, together
__device__ __forceinline__ void count_cell(uint32_t* t, uint32_t idx, uint32_t lane) {
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
    const bool same = idx == first;
    const unsigned long long mask = __ballot(same);
    if (same) {
        if (first != kNone && lane == (uint32_t)__ffsll(mask) - 1u) atomicAdd(t + idx, (uint32_t)__popcll(mask));
    } else if (idx != kNone) {
        atomicAdd(t + idx, 1u);
    }
}

// A_c = sum_r a_r ln a_r of every described partition: one workgroup per partition counts the label bytes into a table per wave
// (256 cells, the global label is the index), adds the tables and reduces with wave_xlnx
__global__ __launch_bounds__(1024) void partition_sizes_kernel(const ChainDesc* chains, uint32_t n, double* A) {
    __shared__ uint32_t cnt[16 * 256];
    const ChainDesc c = chains[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < 16 * 256; i += 1024) cnt[i] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* mine = cnt + (threadIdx.x / 64u) * 256u;
    for (uint32_t w0 = 0; w0 < n; w0 += 4 * 1024) {
        const uint32_t w = w0 + 4 * threadIdx.x;
        const uint32_t L = w < n ? *(const uint32_t*)(c.row + w) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) count_cell(mine, w + j < n ? (L >> (8 * j)) & 0xffu : kNone, lane);
    }
    __syncthreads();
    uint32_t x = 0;
    if (threadIdx.x < 256)
        for (uint32_t k = 0; k < 16; ++k) x += cnt[k * 256 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < 256) cnt[threadIdx.x] = x;
    __syncthreads();
    if (threadIdx.x < 64) {
        const double s = wave_xlnx(cnt, 256, lane);
        if (lane == 0) A[blockIdx.x] = s;
    }
}

}  // namespace
}  // namespace bisbm
