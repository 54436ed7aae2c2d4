// bisbm_wave_chain.hpp -- what the "one wave owns one chain" move kernels share: heatbath_kernel (bisbm_heatbath.hip) and
// reshuffle_kernel (bisbm_reshuffle.hip); DESIGN.md, "The wave-chain state".  A kernel of this kind runs one wave per chain for
// a whole call.  The chain's block state lives in LDS, loaded at the start and stored at the end: the quadrant of m (row stride
// S = kb | 1, odd, so a walk down a column spreads over the banks), m_r, n_r, the k_v histogram, the list of the non-zero
// (t, k_t) of the node under way, and eta when it fits (template parameter EL); labels stay in HBM.  The nodes a kernel visits
// between two __threadfence_block() are of one type, hence an independent set: no step changes a label that another step reads,
// so a chunk of 64 nodes fetches the first 64 neighbour labels of all its rows at once (park_rows) and nothing of that is ever
// invalidated.  A step builds the node's list (neighbour_list), evaluates dS in its kernel's own way -- the f64 operation order
// is each kernel's specification and is not shared -- and applies the move (apply_move).
//
// Every member is __forceinline__ and takes the WaveChain by reference: after inlining its pointers are what the kernels' own
// locals were, wave-uniform values in SGPRs, LDS pointers known as such.
#pragma once

#include "bisbm_kernels.hpp"

namespace bisbm {

__device__ __forceinline__ void wave_fence() {  // (one wave: LDS operations execute in issue order; this only stops code motion)
    __builtin_amdgcn_wave_barrier();
    __asm__ volatile("" ::: "memory");
}

// log n from the host table, as the caller of log_q<true> hands it over
__device__ __forceinline__ double log_n_of(const Tables& tab, int n) { return (n > 0 && (uint64_t)n < tab.lg_size) ? tab.logtab[n] : 0.; }

// The type a phase or a pair works on (tb: type b): its nodes v0 .. v0 + n_cls - 1, its k_own blocks with global labels from
// own0, and the other type's k_oth blocks from oth0.
struct TypeView {
    uint32_t n_cls, v0, k_own, k_oth, own0, oth0;
};
__device__ __forceinline__ TypeView type_view(const WaveChainParams& p, bool tb) {
    return TypeView{tb ? p.nb : p.na, tb ? p.na : 0u, tb ? p.kb : p.ka, tb ? p.ka : p.kb, tb ? p.ka : 0u, tb ? 0u : p.ka};
}

template <bool EL>
struct WaveChain {
    int32_t *mq, *mr, *nr, *hist;  // LDS: ka rows of stride S; [K]; [K]; k_v over the other type's blocks
    uint32_t* s_t;                 // LDS: the non-zero t of the list, ascending
    int32_t* s_kt;                 // LDS: their k_t
    uint8_t* lab_lds;              // LDS: 64 rows x the labels of their first 64 neighbours
    uint32_t *eta_l, *eta_g;       // K * D in LDS when EL; the chain's eta in HBM
    int32_t *m_g, *mr_g, *nr_g;    // the chain's block state in HBM
    uint8_t* labels;
    const uint32_t* col;
    uint32_t lane, ka, kb, K, D, S;

    // Carves the arrays from `cur` on (wave_chain_lds_bytes counts them from the same constants) and loads chain `chain`; the
    // caller's __syncthreads() comes before the first use.
    __device__ __forceinline__ void load(unsigned char* cur, const WaveChainParams& p, uint32_t chain) {
        lane = (uint32_t)lane_id(), ka = p.ka, kb = p.kb, K = p.ka + p.kb, D = p.maxdeg + 1, S = wave_chain_stride(p.kb);
        const uint32_t kmax = p.ka > p.kb ? p.ka : p.kb;
        mq = (int32_t*)cur;
        cur += sizeof(int32_t) * p.ka * S;
        mr = (int32_t*)cur;
        cur += sizeof(int32_t) * K;
        nr = (int32_t*)cur;
        cur += sizeof(int32_t) * K;
        hist = (int32_t*)cur;
        cur += sizeof(int32_t) * kmax;
        s_t = (uint32_t*)cur;
        cur += sizeof(uint32_t) * kmax;
        s_kt = (int32_t*)cur;
        cur += sizeof(int32_t) * kmax;
        lab_lds = (uint8_t*)cur;
        cur += kParkedLabelBytes;
        eta_l = (uint32_t*)cur;
        eta_g = p.eta + (size_t)chain * K * D;
        labels = p.labels + (size_t)chain * p.label_stride, col = p.col;
        m_g = p.m + (size_t)chain * p.ka * p.kb;
        mr_g = p.m_r + (size_t)chain * K;
        nr_g = p.n_r + (size_t)chain * K;
        for (uint32_t i = lane; i < ka * kb; i += kWave) mq[(i / kb) * S + (i % kb)] = m_g[i];
        for (uint32_t i = lane; i < K; i += kWave) {
            mr[i] = mr_g[i];
            nr[i] = nr_g[i];
        }
        if (EL)
            for (uint32_t i = lane; i < K * D; i += kWave) eta_l[i] = eta_g[i];
    }

    // Stores the chain back.
    __device__ __forceinline__ void store() const {
        __syncthreads();
        for (uint32_t i = lane; i < ka * kb; i += kWave) m_g[i] = mq[(i / kb) * S + (i % kb)];
        for (uint32_t i = lane; i < K; i += kWave) {
            mr_g[i] = mr[i];
            nr_g[i] = nr[i];
        }
        if (EL)
            for (uint32_t i = lane; i < K * D; i += kWave) eta_g[i] = eta_l[i];
    }

    // m between block i_own of the type under way and block j_oth of the other type (both local)
    __device__ __forceinline__ int32_t& M(bool tb, uint32_t i_own, uint32_t j_oth) const { return tb ? mq[j_oth * S + i_own] : mq[i_own * S + j_oth]; }

    // (the split is at compile time: one generic pointer would make flat accesses, see eta_load in bisbm_kernels.hip)
    __device__ __forceinline__ uint32_t* eta_at(uint32_t idx) const {
        if constexpr (EL)
            return eta_l + idx;
        else
            return eta_g + idx;
    }

    // Chunk header, after lane q has taken the row extent (beg_l, deg_l; 0, 0 in the lanes past cnt) of the chunk's node q: parks
    // the first 64 neighbour labels of the chunk's rows in lab_lds, eight rows' id loads and eight rows' label gathers in flight
    // together (idle lanes read node 0; rows past cnt: deg 0).
    __device__ __forceinline__ void park_rows(uint32_t cnt, uint32_t beg_l, uint32_t deg_l) const {
        wave_fence();
        for (uint32_t q0 = 0; q0 < cnt; q0 += 8) {
            uint32_t id[8], lb[8];
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t b0 = readlane(beg_l, q0 + j), d0 = readlane(deg_l, q0 + j);
                id[j] = lane < d0 ? col[b0 + lane] : 0u;
            }
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) lb[j] = labels[id[j]];
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) lab_lds[(q0 + j) * kWave + lane] = (uint8_t)lb[j];
        }
        wave_fence();
    }

    // The list of the chunk's node q (row extent beg, deg): k_v, the histogram of its neighbours' labels (integer LDS atomics),
    // then the non-zero (t, k_t) in ascending t, compacted by ballots into s_t / s_kt.  on_entry(pos, t, kt) runs in the lane
    // of every entry, for what a kernel keeps beside it.  Returns the length of the list.
    template <class F>
    __device__ __forceinline__ uint32_t neighbour_list(uint32_t q, uint32_t beg, uint32_t deg, const TypeView& ty, F&& on_entry) const {
        for (uint32_t t = lane; t < ty.k_oth; t += kWave) hist[t] = 0;
        wave_fence();
        if (lane < deg) {
            const uint32_t t = (uint32_t)lab_lds[q * kWave + lane] - ty.oth0;
            if (t < ty.k_oth) atomicAdd(&hist[t], 1);
        }
        for (uint32_t j = kWave + lane; j < deg; j += kWave) {  // rows longer than one wave
            const uint32_t t = (uint32_t)labels[col[beg + j]] - ty.oth0;
            if (t < ty.k_oth) atomicAdd(&hist[t], 1);
        }
        wave_fence();
        uint32_t nnz = 0;
        for (uint32_t c0 = 0; c0 < ty.k_oth; c0 += kWave) {
            const uint32_t t = c0 + lane;
            const int kt = t < ty.k_oth ? hist[t] : 0;
            const unsigned long long bal = __ballot(kt != 0);
            if (kt != 0) {
                const uint32_t pos = nnz + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                s_t[pos] = t, s_kt[pos] = kt;
                on_entry(pos, t, kt);
            }
            nnz += (uint32_t)__popcll(bal);
        }
        wave_fence();
        return nnz;
    }

    // Moves node v (degree deg, list of nnz entries) from block `from` to block `to` (global labels; from_loc, to_loc: within
    // the type), as apply_mcmc_moves does.
    // eta in HBM (EL = false) and the label are written by lane 0 with a vector store and atomics that return nothing, and read
    // by all lanes of later steps with plain loads; wave_fence only stops code motion.  This rests on a property of the
    // hardware: the vector memory operations of ONE wave go through one L1 and reach the L2 in issue order, so a load issued
    // after a store or atomic of the same wave to the same address sees it (the generic sweep_kernel relies on the same for its
    // labels and its eta in HBM).  No other wave reads or writes a chain's arrays during the call.
    __device__ __forceinline__ void apply_move(uint32_t v, uint32_t deg, uint32_t from, uint32_t to, uint32_t from_loc, uint32_t to_loc, bool tb,
                                               uint32_t nnz) const {
        wave_fence();  // all lanes have read nr / mr / eta before lane 0 rewrites them
        if (lane == 0) {
            atomicSub(&nr[from], 1);
            atomicAdd(&nr[to], 1);
            atomicSub(eta_at(from * D + deg), 1u);
            atomicAdd(eta_at(to * D + deg), 1u);
            atomicSub(&mr[from], (int)deg);
            atomicAdd(&mr[to], (int)deg);
            labels[v] = (uint8_t)to;
        }
        for (uint32_t i = lane; i < nnz; i += kWave) {
            const uint32_t t = s_t[i];
            const int k = s_kt[i];
            atomicSub(&M(tb, from_loc, t), k);
            atomicAdd(&M(tb, to_loc, t), k);
        }
        wave_fence();
    }
};

// Sets the dynamic LDS of the two instantiations' one and launches it: n_chains blocks of one wave.
template <class P>
hipError_t launch_wave_chain(void (*in_lds)(P), void (*in_hbm)(P), const P& p, size_t lds_bytes, hipStream_t stream) {
    if (p.n_chains == 0 || p.rounds == 0) return hipSuccess;
    auto kern = p.eta_in_lds ? in_lds : in_hbm;
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(p.n_chains), dim3(kWave), lds_bytes, stream, p);
    return hipGetLastError();
}

}  // namespace bisbm
