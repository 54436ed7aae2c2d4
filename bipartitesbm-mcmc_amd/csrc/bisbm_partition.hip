// bisbm_partition.hip -- chain-by-chain partition distances (include/bisbm.h, "Partition distances and posterior modes"; no
// reference counterpart: the reference keeps one partition).  For every pair (c, d) of the selected chains the contingency table
// n_rs of their labels is counted and reduced to S_cd = sum_rs n_rs ln n_rs; per chain A_c = sum_r a_r ln a_r comes from the
// chain's block sizes.  The host finishes: VI(c, d) = (A_c + A_d - 2 S_cd) / n, H(c) = ln n - A_c / n.
//
// Counting kernel (partition_count_kernel): a workgroup owns a tile of T x T chain pairs -- T row chains, T column chains, so per
// chunk of nodes it loads 2 T label words for T * T pairs -- and keeps one table per pair in LDS, counted with integer LDS atomics
// (a wave whose lanes all hit the leader's cell adds once: chains that agree send whole waves to one diagonal cell).  A pair's
// table holds only the cells that can be non-zero: type a at 0 (r * ka_d + s), type b at ka_c * ka_d (r * kb_d + s), labels
// within the type.  Every pair slot of a launch has the same size, `stride` cells (the largest table of the selection).
//   many pairs (FUSED): a workgroup runs its tile over all nodes and reduces the tables to S_cd without leaving LDS;
//   few pairs: the nodes are split over workgroups, the tables are added into HBM and partition_reduce_kernel reduces them
//     (bisbm_partition_contingency copies one such table out instead); a table too large for LDS is counted straight in HBM.
// Both reduce with wave_xlnx: one wave per table, lane-strided, butterfly -- the same bits from the same integers.
// (ChainDesc, count_cell, wave_xlnx and partition_sizes_kernel: bisbm_partition_device.hpp, shared with bisbm_trace.hip.)
// Chains against reference partitions that are no chains (bisbm_partition_distances_to, and the anchored modes of
// bisbm_mode_marginals.hip through partition_distances_rows) run the same kernels in their RECT form: the tile is T selected
// chains (rows) x T references (columns, byte rows of their own shapes), every pair (row < m, column < mc) is live instead of
// i < j, and a slot's `stride` is kaM_chain * kaM_ref + kbM_chain * kbM_ref, the largest shape of either side taken separately.
// B_g = sum_s b_s ln b_s of a reference is partition_sizes_kernel over the reference rows.
// The chains' state is only read.
#include "bisbm_engine.hpp"
#include "bisbm_partition_device.hpp"

using namespace bisbm;

namespace {

struct CountParams {
    const ChainDesc* chains;  // [m] the row partitions
    const ChainDesc* cols;    // [mc] the column partitions: `chains` again, or (RECT) the references
    const uint2* tiles;       // [tiles of the launch] (row tile, column tile); square: row <= column
    uint32_t m, mc, n, na, stride, nodes_per_block, hbm_direct;
    uint32_t* tab;  // few pairs: [tile of the launch][T * T][stride]
    double* snn;    // [m][mc], entry (i, j) of every live pair
};

// is (row i, column j) a pair of the call?  Square: each unordered pair once; RECT: every chain with every reference
template <bool RECT>
__device__ __forceinline__ bool pair_live(const CountParams& p, uint32_t i, uint32_t j) {
    return RECT ? i < p.m && j < p.mc : i < j && j < p.m;
}

// the node loop of partition_count_kernel: counts the nodes [v0, v1) of the tile's pairs into tabs (LDS, or HBM for tables too
// large for it: a function, so that each call site keeps its pointer's address space and the LDS one gets LDS atomics)
template <int T, bool RECT>
__device__ __forceinline__ void count_tile(uint32_t* tabs, const ChainDesc* ch, const CountParams& p, uint32_t i0, uint32_t j0) {
    const uint8_t *rowr[T], *rowc[T];
    uint32_t kar[T], kbr[T], kac[T], kbc[T];
#pragma unroll
    for (int a = 0; a < T; ++a) {
        rowr[a] = ch[a].row, rowc[a] = ch[T + a].row;
        kar[a] = (uint32_t)__builtin_amdgcn_readfirstlane((int)ch[a].ka), kbr[a] = (uint32_t)__builtin_amdgcn_readfirstlane((int)ch[a].kb);
        kac[a] = (uint32_t)__builtin_amdgcn_readfirstlane((int)ch[T + a].ka), kbc[a] = (uint32_t)__builtin_amdgcn_readfirstlane((int)ch[T + a].kb);
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t v0 = blockIdx.y * p.nodes_per_block;  // (a multiple of 1024: the word loads below are aligned)
    const uint32_t v1 = min(p.n, v0 + p.nodes_per_block);
    // every lane of a wave makes every trip (count_cell needs the whole wave); a lane past the end counts nothing
    for (uint32_t w0 = v0; w0 < v1; w0 += 4 * blockDim.x) {
        const uint32_t w = w0 + 4 * threadIdx.x;
        const bool in = w < v1;
        uint32_t Lr[T], Lc[T];
#pragma unroll
        for (int a = 0; a < T; ++a) {
            // (w + 3 is readable: label rows are padded to a multiple of 256 labels)
            Lr[a] = in && rowr[a] ? *(const uint32_t*)(rowr[a] + w) : 0u;
            Lc[a] = in && rowc[a] ? *(const uint32_t*)(rowc[a] + w) : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t v = w + j;
            const bool live = in && v < v1;
            const bool tb = v >= p.na;
#pragma unroll
            for (int a = 0; a < T; ++a) {
#pragma unroll
                for (int b = 0; b < T; ++b) {
                    if (!pair_live<RECT>(p, i0 + a, j0 + b)) continue;  // (the same for every lane)
                    const uint32_t r = ((Lr[a] >> (8 * j)) & 0xffu) - (tb ? kar[a] : 0u), kr = tb ? kbr[a] : kar[a];
                    const uint32_t s = ((Lc[b] >> (8 * j)) & 0xffu) - (tb ? kac[b] : 0u), ks = tb ? kbc[b] : kac[b];
                    const uint32_t idx = live && r < kr && s < ks ? (uint32_t)(a * T + b) * p.stride + (tb ? kar[a] * kac[b] : 0u) + r * ks + s : kNone;
                    count_cell(tabs, idx, lane);
                }
            }
        }
    }
}

template <int T, bool FUSED, bool RECT>
__global__ __launch_bounds__(1024) void partition_count_kernel(CountParams p) {
    extern __shared__ __align__(16) uint32_t lds_tab[];  // [T * T][stride] unless hbm_direct
    __shared__ ChainDesc ch[2 * T];                      // the tile's row chains, then its column chains
    const uint2 tile = p.tiles[blockIdx.x];
    const uint32_t i0 = tile.x * T, j0 = tile.y * T;
    const bool direct = !FUSED && T == 1 && p.hbm_direct;
    if (threadIdx.x < 2 * T) {
        const bool is_row = threadIdx.x < T;
        const uint32_t idx = is_row ? i0 + threadIdx.x : j0 + threadIdx.x - T;
        const ChainDesc* from = is_row ? p.chains : p.cols;
        const bool have = idx < (is_row ? p.m : p.mc);  // (past the selection: a partition without a row, in no pair)
        ch[threadIdx.x].row = have ? from[idx].row : nullptr;
        ch[threadIdx.x].ka = have ? from[idx].ka : 0u;
        ch[threadIdx.x].kb = have ? from[idx].kb : 0u;
    }
    uint32_t* const out = FUSED ? nullptr : p.tab + (size_t)blockIdx.x * (T * T) * p.stride;
    if (!direct)
        for (uint32_t i = threadIdx.x; i < T * T * p.stride; i += blockDim.x) lds_tab[i] = 0;
    __syncthreads();
    if (direct)
        count_tile<T, RECT>(out, ch, p, i0, j0);
    else
        count_tile<T, RECT>(lds_tab, ch, p, i0, j0);
    if (direct) return;
    __syncthreads();
    if constexpr (FUSED) {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u, waves = blockDim.x / 64u;
        for (uint32_t q = wave; q < T * T; q += waves) {
            const uint32_t a = q / T, b = q % T, gi = i0 + a, gj = j0 + b;
            if (!pair_live<RECT>(p, gi, gj)) continue;
            const uint32_t cells = ch[a].ka * ch[T + b].ka + ch[a].kb * ch[T + b].kb;
            const double s = wave_xlnx(lds_tab + q * p.stride, cells, lane);
            if (lane == 0) p.snn[(size_t)gi * p.mc + gj] = s;
        }
    } else {
        for (uint32_t i = threadIdx.x; i < T * T * p.stride; i += blockDim.x) {
            const uint32_t x = lds_tab[i];
            if (x) atomicAdd(out + i, x);
        }
    }
}

// few pairs: one wave per pair slot of the launch's tiles reduces its HBM table
template <bool RECT>
__global__ __launch_bounds__(64) void partition_reduce_kernel(CountParams p, uint32_t T) {
    const uint2 tile = p.tiles[blockIdx.x];
    const uint32_t q = blockIdx.y, gi = tile.x * T + q / T, gj = tile.y * T + q % T;
    if (!pair_live<RECT>(p, gi, gj)) return;
    const ChainDesc c = p.chains[gi], d = p.cols[gj];
    const double s = wave_xlnx(p.tab + ((size_t)blockIdx.x * (T * T) + q) * p.stride, c.ka * d.ka + c.kb * d.kb, threadIdx.x);
    if (threadIdx.x == 0) p.snn[(size_t)gi * p.mc + gj] = s;
}

// ---- host side --------------------------------------------------------------------------------------------------------

constexpr size_t kLdsTables = kLdsPerCu - 1024;  // dynamic LDS a workgroup may take for its tables (ch[] is static)
constexpr size_t kTabScratch = 256u << 20;       // few pairs: HBM tables of one launch (at least one tile's)

template <int T, bool FUSED, bool RECT>
hipError_t launch_count_t(dim3 grid, uint32_t threads, size_t lds, hipStream_t stream, const CountParams& p) {
    hipError_t e = hipFuncSetAttribute((const void*)partition_count_kernel<T, FUSED, RECT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((partition_count_kernel<T, FUSED, RECT>), grid, dim3(threads), lds, stream, p);
    return hipGetLastError();
}

template <bool FUSED, bool RECT>
hipError_t launch_count(uint32_t T, dim3 grid, uint32_t threads, size_t lds, hipStream_t stream, const CountParams& p) {
    switch (T) {
        case 4: return launch_count_t<4, FUSED, RECT>(grid, threads, lds, stream, p);
        case 2: return launch_count_t<2, FUSED, RECT>(grid, threads, lds, stream, p);
        default: return launch_count_t<1, FUSED, RECT>(grid, threads, lds, stream, p);
    }
}

// the engine whose device computes and whose PartitionState holds the scratch
bisbm_engine* computing_engine(bisbm_engine* h) { return h->devs.empty() ? h : h->devs[0]; }

// checks the handle, waits for its chains' streams and describes the listed chains on the computing device (rows of chains
// on another device are copied into the staging buffer: peer copy, through the host where that is refused)
int describe(bisbm_engine* h, const char* call, const std::vector<uint32_t>& sel, std::vector<ChainDesc>& desc) {
    const std::vector<bisbm_engine*> all = leaves(h);
    for (bisbm_engine* e : all)
        if (e->wide)
            return fail(h, BISBM_ERR_UNSUPPORTED, "partition distances serve byte labels only (at most 256 blocks; this handle has %u + %u)", e->ka, e->kb);
    for (bisbm_engine* e : all)
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before %s", call);
    // (node indices are 32-bit in the kernels and run up to a workgroup's stride past n)
    if (h->n >= 0xFFFFFFFFull - 8192) return fail(h, BISBM_ERR_UNSUPPORTED, "more than 2^32 - 8193 nodes");
    for (bisbm_engine* e : all) {
        HIPCHK(h, hipSetDevice(e->device));
        HIPCHK(h, hipStreamSynchronize(e->stream));
    }
    bisbm_engine* ce = computing_engine(h);
    PartitionState& s = ce->partition;
    HIPCHK(h, hipSetDevice(ce->device));
    const size_t srow = ((size_t)h->n + 255) & ~(size_t)255;
    size_t staged = 0;
    desc.resize(sel.size());
    std::vector<std::pair<size_t, const uint8_t*>> away;  // (position, row on its own device)
    std::vector<int> away_dev;
    for (size_t i = 0; i < sel.size(); ++i) {
        uint32_t local = 0;
        bisbm_engine* e = leaf_of_chain(h, sel[i], &local);
        desc[i].ka = e->ka, desc[i].kb = e->kb;
        const uint8_t* row = e->d_labels + (size_t)local * e->label_stride;
        if (e->device == ce->device) {
            desc[i].row = row;
        } else {
            away.push_back({i, row});
            away_dev.push_back(e->device);
            ++staged;
        }
    }
    if (staged) {
        RESERVE(h, s.d_stage, staged * srow);
        std::vector<uint8_t> bounce;
        for (size_t k = 0; k < away.size(); ++k) {
            uint8_t* dst = s.d_stage.get() + k * srow;
            // (on the computing stream: the kernels that read the staging buffer are ordered behind the copy)
            if (hipMemcpyPeerAsync(dst, ce->device, away[k].second, away_dev[k], srow, ce->stream) != hipSuccess) {
                bounce.resize(srow);
                HIPCHK(h, hipSetDevice(away_dev[k]));
                HIPCHK(h, hipMemcpy(bounce.data(), away[k].second, srow, hipMemcpyDeviceToHost));
                HIPCHK(h, hipSetDevice(ce->device));
                HIPCHK(h, hipMemcpy(dst, bounce.data(), srow, hipMemcpyHostToDevice));
            }
            desc[away[k].first].row = dst;
        }
    }
    return BISBM_OK;
}

// the descriptors of a call onto the computing engine ce: the row partitions, then (distances_to) the references
int upload_desc(bisbm_engine* h, bisbm_engine* ce, const std::vector<ChainDesc>& rows, const std::vector<ChainDesc>* refs) {
    PartitionState& s = ce->partition;
    const size_t m = rows.size(), r = refs ? refs->size() : 0;
    RESERVE(h, s.d_desc, sizeof(ChainDesc) * (m + r));
    HIPCHK(h, hipMemcpyAsync(s.d_desc.get(), rows.data(), sizeof(ChainDesc) * m, hipMemcpyHostToDevice, ce->stream));
    if (r) HIPCHK(h, hipMemcpyAsync(s.d_desc.get() + sizeof(ChainDesc) * m, refs->data(), sizeof(ChainDesc) * r, hipMemcpyHostToDevice, ce->stream));
    return BISBM_OK;
}

hipError_t launch_count_any(bool fused, bool rect, uint32_t T, dim3 grid, uint32_t threads, size_t lds, hipStream_t stream, const CountParams& p) {
    if (fused) return rect ? launch_count<true, true>(T, grid, threads, lds, stream, p) : launch_count<true, false>(T, grid, threads, lds, stream, p);
    return rect ? launch_count<false, true>(T, grid, threads, lds, stream, p) : launch_count<false, false>(T, grid, threads, lds, stream, p);
}

enum Regime { kAuto = 0, kFused = 1, kSplit = 2 };

// S_cd of every pair i < j of the described chains into snn[m * m] (host), or -- table_out given, m = 2 -- the integer table
// of the pair (0, 1) in the kernel's layout; refs given (the descriptors behind the chains' on ce): S of every chain with every
// reference into snn[m * refs]
int run_pairs(bisbm_engine* h, bisbm_engine* ce, const std::vector<ChainDesc>& desc, const std::vector<ChainDesc>* refs, double* snn,
              std::vector<uint32_t>* table_out) {
    PartitionState& s = ce->partition;
    const bool rect = refs != nullptr;
    const uint32_t m = (uint32_t)desc.size(), mc = rect ? (uint32_t)refs->size() : m;
    // (a slot holds the largest table of the call: the largest row shape with the largest column shape, each on its own)
    uint32_t kaM = 0, kbM = 0, kaC = 0, kbC = 0;
    for (const ChainDesc& d : desc) kaM = std::max(kaM, d.ka), kbM = std::max(kbM, d.kb);
    for (const ChainDesc& d : rect ? *refs : desc) kaC = std::max(kaC, d.ka), kbC = std::max(kbC, d.kb);
    const uint32_t stride = kaM * kaC + kbM * kbC;
    const size_t pair_bytes = sizeof(uint32_t) * (size_t)stride;
    const bool direct = pair_bytes > kLdsTables;
    uint32_t T = 1;
    if (!table_out) {
        if (16 * pair_bytes <= kLdsTables) T = 4;
        else if (4 * pair_bytes <= kLdsTables) T = 2;
        // (no tile wider than the call: square tiles pair i < j, so T < m; rectangular ones only need T / 2 < max(m, refs))
        while (T > 1 && (rect ? T / 2 >= std::max(m, mc) : T >= m)) T /= 2;
    }
    std::vector<uint2> tiles;
    const uint32_t nT = (m + T - 1) / T, nTc = (mc + T - 1) / T;
    for (uint32_t ti = 0; ti < nT; ++ti)
        for (uint32_t tj = rect ? 0 : ti; tj < nTc; ++tj)
            if (rect || ti != tj || (T > 1 && m - ti * T >= 2)) tiles.push_back(make_uint2(ti, tj));
    if (tiles.empty() || !stride) {
        if (snn) std::fill(snn, snn + (size_t)m * mc, 0.);
        return BISBM_OK;
    }
    int regime = kAuto;
    if (const char* e = std::getenv("BISBM_PARTITION_REGIME")) regime = !strcmp(e, "fused") ? kFused : !strcmp(e, "split") ? kSplit : kAuto;
    int cus = 0;
    HIPCHK(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ce->device));
    // many pairs: a tile per workgroup fills the compute units; few pairs: the nodes are split as well
    const bool fused = !table_out && !direct && (regime == kFused || (regime == kAuto && tiles.size() >= (size_t)cus));
    RESERVE(h, s.d_tiles, tiles.size());
    RESERVE(h, s.d_snn, (size_t)m * mc);
    HIPCHK(h, hipMemcpyAsync(s.d_tiles.get(), tiles.data(), sizeof(uint2) * tiles.size(), hipMemcpyHostToDevice, ce->stream));
    CountParams p{};
    p.chains = (const ChainDesc*)s.d_desc.get();
    p.cols = rect ? p.chains + m : p.chains;
    p.m = m;
    p.mc = mc;
    p.n = (uint32_t)h->n;
    p.na = (uint32_t)h->na;
    p.stride = stride;
    p.hbm_direct = direct ? 1u : 0u;
    p.snn = s.d_snn.get();
    const size_t lds = direct ? 0 : (size_t)T * T * pair_bytes;
    const uint32_t threads = lds > 40 * 1024 ? 1024u : 256u;
    if (fused) {
        p.tiles = s.d_tiles.get();
        p.nodes_per_block = (p.n + 1023u) & ~1023u;
        HIPCHK(h, launch_count_any(true, rect, T, dim3((uint32_t)tiles.size(), 1), threads, lds, ce->stream, p));
    } else {
        const size_t tile_bytes = (size_t)T * T * pair_bytes;
        const size_t per = std::max<size_t>(1, std::min<size_t>(tiles.size(), kTabScratch / tile_bytes));
        RESERVE(h, s.d_tab, per * tile_bytes / sizeof(uint32_t));
        p.tab = s.d_tab.get();
        for (size_t t0 = 0; t0 < tiles.size(); t0 += per) {
            const uint32_t nb = (uint32_t)std::min(per, tiles.size() - t0);
            p.tiles = s.d_tiles.get() + t0;
            // about 8 workgroups per compute unit, at least 4096 nodes each (the LDS tables are zeroed and added to HBM once per
            // workgroup)
            const uint32_t max_chunks = (p.n + 4095u) / 4096u, want = 8u * (uint32_t)std::max(cus, 1);
            const uint32_t chunks = std::max(1u, std::min(max_chunks, (want + nb - 1) / nb));
            p.nodes_per_block = (((p.n + chunks - 1) / chunks) + 1023u) & ~1023u;
            HIPCHK(h, hipMemsetAsync(s.d_tab.get(), 0, (size_t)nb * tile_bytes, ce->stream));
            HIPCHK(h, launch_count_any(false, rect, T, dim3(nb, (p.n + p.nodes_per_block - 1) / p.nodes_per_block), threads, lds, ce->stream, p));
            if (table_out) {
                table_out->resize(stride);
                HIPCHK(h, hipMemcpyAsync(table_out->data(), s.d_tab.get(), pair_bytes, hipMemcpyDeviceToHost, ce->stream));
            } else {
                if (rect)
                    hipLaunchKernelGGL(partition_reduce_kernel<true>, dim3(nb, T * T), dim3(64), 0, ce->stream, p, T);
                else
                    hipLaunchKernelGGL(partition_reduce_kernel<false>, dim3(nb, T * T), dim3(64), 0, ce->stream, p, T);
                HIPCHK(h, hipGetLastError());
            }
        }
    }
    if (snn) HIPCHK(h, hipMemcpyAsync(snn, s.d_snn.get(), sizeof(double) * (size_t)m * mc, hipMemcpyDeviceToHost, ce->stream));
    HIPCHK(h, hipStreamSynchronize(ce->stream));
    return BISBM_OK;
}

// sum_r a_r ln a_r of the first m described partitions on ce (chains, then references)
int run_sizes(bisbm_engine* h, bisbm_engine* ce, uint32_t m, double* A) {
    PartitionState& s = ce->partition;
    RESERVE(h, s.d_A, m);
    hipLaunchKernelGGL(partition_sizes_kernel, dim3(m), dim3(1024), 0, ce->stream, (const ChainDesc*)s.d_desc.get(), (uint32_t)h->n, s.d_A.get());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(A, s.d_A.get(), sizeof(double) * m, hipMemcpyDeviceToHost, ce->stream));
    HIPCHK(h, hipStreamSynchronize(ce->stream));
    return BISBM_OK;
}

// the selection of a distances call: chains = NULL is every chain; no chain out of range or twice
int select_chains(bisbm_engine* h, uint32_t n_sel, const uint32_t* chains, std::vector<uint32_t>& sel) {
    if (!chains && n_sel != h->n_chains)
        return fail(h, BISBM_ERR_INVALID_ARG, "chains = NULL selects all %u chains of the handle, n_sel is %u", h->n_chains, n_sel);
    if (n_sel == 0) return fail(h, BISBM_ERR_INVALID_ARG, "no chain selected");
    sel.resize(n_sel);
    std::vector<int64_t> seen(h->n_chains, -1);
    for (uint32_t i = 0; i < n_sel; ++i) {
        const uint32_t c = chains ? chains[i] : i;
        if (c >= h->n_chains)
            return fail(h, BISBM_ERR_INVALID_ARG, "chain %u (position %u of the selection) is out of range: the handle has %u chains", c, i, h->n_chains);
        if (seen[c] >= 0)
            return fail(h, BISBM_ERR_INVALID_ARG, "chain %u is listed twice (positions %lld and %u of the selection)", c, (long long)seen[c], i);
        seen[c] = i, sel[i] = c;
    }
    return BISBM_OK;
}

// VI of every described chain with every described reference (rows on ce's device) into vi[m * refs], H of the references
int run_rect(bisbm_engine* h, bisbm_engine* ce, const std::vector<ChainDesc>& desc, const std::vector<ChainDesc>& refs, double* vi, double* h_ref) {
    const uint32_t m = (uint32_t)desc.size(), r = (uint32_t)refs.size();
    if (int rc = upload_desc(h, ce, desc, &refs)) return rc;
    std::vector<double> A(m + r), snn((size_t)m * r, 0.);
    if (int rc = run_sizes(h, ce, m + r, A.data())) return rc;
    if (int rc = run_pairs(h, ce, desc, &refs, snn.data(), nullptr)) return rc;
    const double n = (double)h->n;
    if (h_ref)
        for (uint32_t j = 0; j < r; ++j) h_ref[j] = std::log(n) - A[m + j] / n;
    if (vi)
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = 0; j < r; ++j) {
                const double v = ((A[i] + A[m + j]) - 2. * snn[(size_t)i * r + j]) / n;
                vi[(size_t)i * r + j] = v > 0. ? v : 0.;
            }
    return BISBM_OK;
}

}  // namespace

int bisbm::partition_distances_rows(bisbm_engine* e, const std::vector<uint32_t>& chains, const uint8_t* d_refs, size_t ref_stride, uint32_t n_refs, double* vi) {
    if (chains.empty() || !n_refs) return BISBM_OK;
    if (e->n >= 0xFFFFFFFFull - 8192) return fail(e, BISBM_ERR_UNSUPPORTED, "more than 2^32 - 8193 nodes");
    HIPCHK(e, hipSetDevice(e->device));
    try {
        std::vector<ChainDesc> desc(chains.size()), refs(n_refs);
        for (size_t i = 0; i < chains.size(); ++i) desc[i] = ChainDesc{e->d_labels + (size_t)chains[i] * e->label_stride, e->ka, e->kb};
        for (uint32_t g = 0; g < n_refs; ++g) refs[g] = ChainDesc{d_refs + (size_t)g * ref_stride, e->ka, e->kb};
        return run_rect(e, e, desc, refs, vi, nullptr);
    } catch (const std::bad_alloc&) {
        return fail(e, BISBM_ERR_STATE, "out of host memory");
    }
}

extern "C" {

int bisbm_partition_distances(bisbm_handle h, uint32_t n_sel, const uint32_t* chains, double* vi_out, double* h_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    try {
        std::vector<uint32_t> sel;
        if (int rc = select_chains(h, n_sel, chains, sel)) return rc;
        std::vector<ChainDesc> desc;
        if (int rc = describe(h, "bisbm_partition_distances", sel, desc)) return rc;
        bisbm_engine* ce = computing_engine(h);
        if (int rc = upload_desc(h, ce, desc, nullptr)) return rc;
        std::vector<double> A(n_sel), snn(vi_out ? (size_t)n_sel * n_sel : 0, 0.);
        if (int rc = run_sizes(h, ce, n_sel, A.data())) return rc;
        if (vi_out)
            if (int rc = run_pairs(h, ce, desc, nullptr, snn.data(), nullptr)) return rc;
        const double n = (double)h->n;
        if (h_out)
            for (uint32_t i = 0; i < n_sel; ++i) h_out[i] = std::log(n) - A[i] / n;
        if (vi_out)
            for (uint32_t i = 0; i < n_sel; ++i) {
                vi_out[(size_t)i * n_sel + i] = 0.;
                for (uint32_t j = i + 1; j < n_sel; ++j) {  // each pair once, mirrored
                    const double v = ((A[i] + A[j]) - 2. * snn[(size_t)i * n_sel + j]) / n;
                    vi_out[(size_t)i * n_sel + j] = vi_out[(size_t)j * n_sel + i] = v > 0. ? v : 0.;
                }
            }
    } catch (const std::bad_alloc&) {
        return fail(h, BISBM_ERR_STATE, "out of host memory");
    }
    return BISBM_OK;
}

int bisbm_partition_distances_to(bisbm_handle h, uint32_t n_sel, const uint32_t* chains, uint32_t n_refs, const uint32_t* ref_labels, const uint32_t* ref_ka,
                                 const uint32_t* ref_kb, double* vi_out, double* h_ref_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (n_refs == 0) return fail(h, BISBM_ERR_INVALID_ARG, "no reference partition (n_refs = 0)");
    if (!ref_labels || !ref_ka || !ref_kb || !vi_out) return fail(h, BISBM_ERR_INVALID_ARG, "ref_labels, ref_ka, ref_kb and vi_out must be non-NULL");
    try {
        std::vector<uint32_t> sel;
        if (int rc = select_chains(h, n_sel, chains, sel)) return rc;
        std::vector<ChainDesc> desc;
        if (int rc = describe(h, "bisbm_partition_distances_to", sel, desc)) return rc;
        bisbm_engine* ce = computing_engine(h);
        // the references as byte rows, padded with zeroes like a chain's label row (the kernels load words past n)
        const size_t srow = ((size_t)h->n + 255) & ~(size_t)255;
        std::vector<uint8_t> rows((size_t)n_refs * srow, 0);
        for (uint32_t g = 0; g < n_refs; ++g) {
            const uint32_t ka = ref_ka[g], kb = ref_kb[g];
            if ((uint64_t)ka + kb > 256)
                return fail(h, BISBM_ERR_INVALID_ARG, "reference %u has %u + %u blocks: partition distances serve at most 256", g, ka, kb);
            const uint32_t* lab = ref_labels + (size_t)g * h->n;
            for (uint64_t v = 0; v < h->n; ++v) {
                const bool tb = v >= h->na;
                if (lab[v] < (tb ? ka : 0u) || lab[v] >= (tb ? ka + kb : ka))
                    return fail(h, BISBM_ERR_INVALID_ARG, "reference %u: label %u of node %llu is outside its type's blocks [%u, %u)", g, lab[v],
                                (unsigned long long)v, tb ? ka : 0u, tb ? ka + kb : ka);
                rows[(size_t)g * srow + v] = (uint8_t)lab[v];
            }
        }
        PartitionState& s = ce->partition;
        RESERVE(h, s.d_refs, rows.size());
        HIPCHK(h, hipMemcpyAsync(s.d_refs.get(), rows.data(), rows.size(), hipMemcpyHostToDevice, ce->stream));
        HIPCHK(h, hipStreamSynchronize(ce->stream));
        std::vector<ChainDesc> refs(n_refs);
        for (uint32_t g = 0; g < n_refs; ++g) refs[g] = ChainDesc{s.d_refs.get() + (size_t)g * srow, ref_ka[g], ref_kb[g]};
        return run_rect(h, ce, desc, refs, vi_out, h_ref_out);
    } catch (const std::bad_alloc&) {
        return fail(h, BISBM_ERR_STATE, "out of host memory");
    }
}

int bisbm_partition_contingency(bisbm_handle h, uint32_t c, uint32_t d, uint32_t* table_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!table_out) return fail(h, BISBM_ERR_INVALID_ARG, "table_out is NULL");
    if (c >= h->n_chains || d >= h->n_chains)
        return fail(h, BISBM_ERR_INVALID_ARG, "chain %u out of range: the handle has %u chains", c >= h->n_chains ? c : d, h->n_chains);
    try {
        std::vector<ChainDesc> desc;
        if (int rc = describe(h, "bisbm_partition_contingency", {c, d}, desc)) return rc;
        bisbm_engine* ce = computing_engine(h);
        if (int rc = upload_desc(h, ce, desc, nullptr)) return rc;
        std::vector<uint32_t> tab;
        if (int rc = run_pairs(h, ce, desc, nullptr, nullptr, &tab)) return rc;
        const uint32_t kac = desc[0].ka, kbc = desc[0].kb, kad = desc[1].ka, kbd = desc[1].kb, Kd = kad + kbd;
        std::fill(table_out, table_out + (size_t)(kac + kbc) * Kd, 0u);
        for (uint32_t r = 0; r < kac; ++r)
            for (uint32_t q = 0; q < kad; ++q) table_out[(size_t)r * Kd + q] = tab[(size_t)r * kad + q];
        for (uint32_t r = 0; r < kbc; ++r)
            for (uint32_t q = 0; q < kbd; ++q) table_out[(size_t)(kac + r) * Kd + kad + q] = tab[(size_t)kac * kad + (size_t)r * kbd + q];
    } catch (const std::bad_alloc&) {
        return fail(h, BISBM_ERR_STATE, "out of host memory");
    }
    return BISBM_OK;
}

int bisbm_partition_modes(uint32_t m, const double* vi, double threshold, uint32_t* mode_out, uint32_t* medoid_out, uint32_t* n_modes_out) {
    if (m == 0 || !vi || !mode_out || !n_modes_out) return fail(nullptr, BISBM_ERR_INVALID_ARG, "m must be >= 1, vi, mode_out and n_modes_out non-NULL");
    if (!(threshold >= 0.)) return fail(nullptr, BISBM_ERR_INVALID_ARG, "the threshold must be a number >= 0, got %g", threshold);
    for (uint32_t i = 0; i < m; ++i)
        for (uint32_t j = 0; j < m; ++j) {
            const double x = vi[(size_t)i * m + j];
            if (std::isnan(x)) return fail(nullptr, BISBM_ERR_INVALID_ARG, "vi[%u][%u] is NaN", i, j);
            if (x != vi[(size_t)j * m + i])
                return fail(nullptr, BISBM_ERR_INVALID_ARG, "vi is not symmetric: vi[%u][%u] = %.17g, vi[%u][%u] = %.17g", i, j, x, j, i, vi[(size_t)j * m + i]);
        }
    try {
        // single linkage: union-find over the pairs within the threshold, the lowest index is the root
        std::vector<uint32_t> root(m);
        for (uint32_t i = 0; i < m; ++i) root[i] = i;
        auto find = [&](uint32_t x) {
            while (root[x] != x) x = root[x] = root[root[x]];
            return x;
        };
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = i + 1; j < m; ++j)
                if (vi[(size_t)i * m + j] <= threshold) {
                    const uint32_t a = find(i), b = find(j);
                    if (a != b) root[std::max(a, b)] = std::min(a, b);
                }
        std::vector<uint32_t> id(m, 0xffffffffu);
        uint32_t modes = 0;
        for (uint32_t i = 0; i < m; ++i) {  // numbered by their lowest member
            const uint32_t r = find(i);
            if (id[r] == 0xffffffffu) id[r] = modes++;
            mode_out[i] = id[r];
        }
        *n_modes_out = modes;
        if (medoid_out) {
            std::vector<std::vector<uint32_t>> members(modes);
            for (uint32_t i = 0; i < m; ++i) members[mode_out[i]].push_back(i);
            for (uint32_t k = 0; k < modes; ++k) {
                double best = 0.;
                uint32_t pick = members[k][0];
                for (size_t a = 0; a < members[k].size(); ++a) {
                    double sum = 0.;
                    for (uint32_t j : members[k]) sum += vi[(size_t)members[k][a] * m + j];
                    if (a == 0 || sum < best) best = sum, pick = members[k][a];
                }
                medoid_out[k] = pick;
            }
        }
    } catch (const std::bad_alloc&) {
        return fail(nullptr, BISBM_ERR_STATE, "out of host memory");
    }
    return BISBM_OK;
}

}  // extern "C"
