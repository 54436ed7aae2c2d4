// bisbm_trace.hip -- chain traces (include/bisbm.h, "Chain traces"; no reference counterpart: the reference keeps no history).
// Every device entry keeps a ring of `depth` snapshots of its own chains' label rows.  A record compares every chain's labels
// now with each held snapshot of the same chain (age a = 1 ... : taken a records ago): the contingency table of the pair in the
// layout of bisbm_partition.hip (type a at r * ka + s, type b at ka * ka + r * kb + s; both sides have the chain's shape), reduced
// to S_nn = sum n_rs ln n_rs by wave_xlnx and to agree = sum_r n_rr, the nodes whose label is unchanged.  The host finishes as
// bisbm_partition_distances_to does -- VI = ((A_now + A_then) - 2 S_nn) / n with A from partition_sizes_kernel, A_then cached
// when the snapshot was taken -- so the same integers give the same bits as that call with the snapshot as a reference.
//
// Counting kernel (trace_count_kernel): a workgroup owns one chain and a tile of up to TA = 4 ages, so per 4 nodes it loads one
// word of the current row and TA snapshot words, and keeps one table per age in LDS.  Consecutive snapshots of a chain mostly
// agree: most counts land on diagonal cells and whole waves hit one cell, which count_cell adds once.  The three regimes of
// bisbm_partition.hip, chosen by its criteria (BISBM_PARTITION_REGIME=fused|split forces the first two):
//   many (chain, age tile) workgroups (FUSED): a workgroup runs over all nodes and reduces its tables without leaving LDS;
//   few: the nodes are split over workgroups, the LDS tables are added into HBM and trace_reduce_kernel reduces them;
//   a table too large for the LDS is counted straight in HBM (a tile of one age), then reduced the same way.
// All integer adds; the only floating-point sums are wave_xlnx's, one wave per table.  The chains' state is only read.
#include "bisbm_engine.hpp"
#include "bisbm_partition_device.hpp"

using namespace bisbm;

namespace {

struct TraceParams {
    const ChainDesc* chains;  // [C] the current label rows and shapes of the entry's chains
    const uint8_t* ring;      // [depth][C][row_stride] snapshots
    size_t row_stride;
    uint32_t C, ages, depth, head;  // age index i (age i + 1) lives in slot (head + depth - 1 - i) % depth
    uint32_t n, na, stride, nodes_per_block, hbm_direct, age_tiles;
    uint32_t wg0;             // first (chain, age tile) of the launch: workgroup x is chain (wg0 + x) / age_tiles
    uint32_t* tab;            // few workgroups: [workgroup of the launch][TA][stride]
    double* snn;              // [C][ages]
    unsigned long long* agree;  // [C][ages]
};

__device__ __forceinline__ const uint8_t* snapshot_row(const TraceParams& p, uint32_t chain, uint32_t age_index) {
    const uint32_t slot = (p.head + p.depth - 1u - age_index) % p.depth;
    return p.ring + ((size_t)slot * p.C + chain) * p.row_stride;
}

// sum of the diagonal cells n_rr of one table by one wave (integers: any order)
__device__ uint32_t wave_agree(const uint32_t* t, uint32_t ka, uint32_t kb, uint32_t lane) {
    uint32_t s = 0;
    for (uint32_t i = lane; i < ka + kb; i += 64) s += i < ka ? t[i * ka + i] : t[ka * ka + (i - ka) * kb + (i - ka)];
    for (int off = 32; off > 0; off >>= 1) s += (uint32_t)__shfl_xor((int)s, off);
    return s;
}

// the node loop: counts the nodes [v0, v1) of chain `c` against the ages a0 .. a0 + TA - 1 into tabs (LDS or HBM: a function,
// so that each call site keeps its pointer's address space)
template <int TA>
__device__ __forceinline__ void trace_count_tile(uint32_t* tabs, const TraceParams& p, const ChainDesc& c, uint32_t chain, uint32_t a0) {
    const uint8_t* then[TA];
#pragma unroll
    for (int a = 0; a < TA; ++a) then[a] = a0 + a < p.ages ? snapshot_row(p, chain, a0 + a) : nullptr;
    const uint32_t ka = (uint32_t)__builtin_amdgcn_readfirstlane((int)c.ka), kb = (uint32_t)__builtin_amdgcn_readfirstlane((int)c.kb);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t v0 = blockIdx.y * p.nodes_per_block;  // (a multiple of 1024: the word loads below are aligned)
    const uint32_t v1 = min(p.n, v0 + p.nodes_per_block);
    // every lane of a wave makes every trip (count_cell needs the whole wave); a lane past the end counts nothing
    for (uint32_t w0 = v0; w0 < v1; w0 += 4 * blockDim.x) {
        const uint32_t w = w0 + 4 * threadIdx.x;
        const bool in = w < v1;
        // (w + 3 is readable: label rows and snapshot rows are padded to a multiple of 256 labels)
        const uint32_t Ln = in ? *(const uint32_t*)(c.row + w) : 0u;
        uint32_t Lt[TA];
#pragma unroll
        for (int a = 0; a < TA; ++a) Lt[a] = in && then[a] ? *(const uint32_t*)(then[a] + w) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t v = w + j;
            const bool live = in && v < v1;
            const bool tb = v >= p.na;
            const uint32_t k = tb ? kb : ka, base = tb ? ka * ka : 0u, off = tb ? ka : 0u;
            const uint32_t r = ((Ln >> (8 * j)) & 0xffu) - off;
#pragma unroll
            for (int a = 0; a < TA; ++a) {
                if (!then[a]) continue;  // (the same for every lane)
                const uint32_t s = ((Lt[a] >> (8 * j)) & 0xffu) - off;
                const uint32_t idx = live && r < k && s < k ? (uint32_t)a * p.stride + base + r * k + s : kNone;
                count_cell(tabs, idx, lane);
            }
        }
    }
}

template <int TA, bool FUSED>
__global__ __launch_bounds__(1024) void trace_count_kernel(TraceParams p) {
    extern __shared__ __align__(16) uint32_t lds_tab[];  // [TA][stride] unless hbm_direct
    const uint32_t wg = p.wg0 + blockIdx.x, chain = wg / p.age_tiles, a0 = (wg % p.age_tiles) * TA;
    const ChainDesc c = p.chains[chain];
    const bool direct = !FUSED && TA == 1 && p.hbm_direct;
    uint32_t* const out = FUSED ? nullptr : p.tab + (size_t)blockIdx.x * TA * p.stride;
    if (!direct)
        for (uint32_t i = threadIdx.x; i < TA * p.stride; i += blockDim.x) lds_tab[i] = 0;
    __syncthreads();
    if (direct)
        trace_count_tile<TA>(out, p, c, chain, a0);
    else
        trace_count_tile<TA>(lds_tab, p, c, chain, a0);
    if (direct) return;
    __syncthreads();
    if constexpr (FUSED) {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u, waves = blockDim.x / 64u;
        for (uint32_t q = wave; q < TA; q += waves) {
            if (a0 + q >= p.ages) continue;
            const double s = wave_xlnx(lds_tab + q * p.stride, c.ka * c.ka + c.kb * c.kb, lane);
            const uint32_t g = wave_agree(lds_tab + q * p.stride, c.ka, c.kb, lane);
            if (lane == 0) {
                p.snn[(size_t)chain * p.ages + a0 + q] = s;
                p.agree[(size_t)chain * p.ages + a0 + q] = g;
            }
        }
    } else {
        for (uint32_t i = threadIdx.x; i < TA * p.stride; i += blockDim.x) {
            const uint32_t x = lds_tab[i];
            if (x) atomicAdd(out + i, x);
        }
    }
}

// few workgroups: one wave per (workgroup of the launch, age of its tile) reduces its HBM table
__global__ __launch_bounds__(64) void trace_reduce_kernel(TraceParams p, uint32_t TA) {
    const uint32_t wg = p.wg0 + blockIdx.x, chain = wg / p.age_tiles, age = (wg % p.age_tiles) * TA + blockIdx.y;
    if (age >= p.ages) return;
    const ChainDesc c = p.chains[chain];
    const uint32_t* t = p.tab + ((size_t)blockIdx.x * TA + blockIdx.y) * p.stride;
    const double s = wave_xlnx(t, c.ka * c.ka + c.kb * c.kb, threadIdx.x);
    const uint32_t g = wave_agree(t, c.ka, c.kb, threadIdx.x);
    if (threadIdx.x == 0) {
        p.snn[(size_t)chain * p.ages + age] = s;
        p.agree[(size_t)chain * p.ages + age] = g;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------

constexpr size_t kLdsTables = kLdsPerCu - 1024;  // dynamic LDS a workgroup may take for its tables
constexpr size_t kTabScratch = 256u << 20;       // few workgroups: HBM tables of one launch (at least one workgroup's)

template <int TA, bool FUSED>
hipError_t launch_trace_t(dim3 grid, uint32_t threads, size_t lds, hipStream_t stream, const TraceParams& p) {
    hipError_t e = hipFuncSetAttribute((const void*)trace_count_kernel<TA, FUSED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((trace_count_kernel<TA, FUSED>), grid, dim3(threads), lds, stream, p);
    return hipGetLastError();
}

template <bool FUSED>
hipError_t launch_trace(uint32_t TA, dim3 grid, uint32_t threads, size_t lds, hipStream_t stream, const TraceParams& p) {
    switch (TA) {
        case 4: return launch_trace_t<4, FUSED>(grid, threads, lds, stream, p);
        case 2: return launch_trace_t<2, FUSED>(grid, threads, lds, stream, p);
        default: return launch_trace_t<1, FUSED>(grid, threads, lds, stream, p);
    }
}

enum Regime { kAuto = 0, kFused = 1, kSplit = 2 };

// what one device entry's part of a record brings back to the host
struct EntryResult {
    std::vector<ChainDesc> desc;            // [chains] (kept until the entry's stream has been waited for: the upload reads it)
    std::vector<double> A, snn;             // [chains], [chains][ages]
    std::vector<unsigned long long> agree;  // [chains][ages]
};

void drop(TraceState& t) {
    t.d_ring.reset(), t.d_desc.reset(), t.d_A.reset(), t.d_snn.reset(), t.d_agree.reset(), t.d_tab.reset();
}

void forget(bisbm_engine* h) {
    TraceState& t = h->trace;
    const size_t C = h->n_chains, D = t.depth;
    t.records = 0;
    t.A_ring.assign(D * C, 0.);
    t.snap_ka.assign(C, 0), t.snap_kb.assign(C, 0);
    t.vi_sum.assign(C * D, 0.);
    t.vi_last.assign(C * D, std::numeric_limits<double>::quiet_NaN());
    t.agree_sum.assign(C * D, 0);
    t.pairs.assign(D, 0);
    t.S.clear(), t.H.clear();
}

// one device entry's part of a record, enqueued on its stream (no sync): A of its chains now, S_nn and agree of every chain with
// every held age, and the current rows pushed into slot `head`
int enqueue_entry(bisbm_engine* h, bisbm_engine* d, uint32_t depth, uint32_t ages, uint32_t head, EntryResult& res) {
    TraceState& t = d->trace;
    const uint32_t C = d->n_chains;
    HIPCHK(h, hipSetDevice(d->device));
    for (bisbm_engine* e : leaves(d)) HIPCHK(h, hipStreamSynchronize(e->stream));
    std::vector<ChainDesc>& desc = res.desc;
    desc.resize(C);
    for (uint32_t c = 0; c < C; ++c) {
        uint32_t local = 0;
        bisbm_engine* e = leaf_of_chain(d, c, &local);
        desc[c] = ChainDesc{e->d_labels + (size_t)local * e->label_stride, e->ka, e->kb};
    }
    const size_t srow = d->label_stride;
    RESERVE(h, t.d_desc, sizeof(ChainDesc) * C);
    RESERVE(h, t.d_A, C);
    HIPCHK(h, hipMemcpyAsync(t.d_desc.get(), desc.data(), sizeof(ChainDesc) * C, hipMemcpyHostToDevice, d->stream));
    const ChainDesc* d_desc = (const ChainDesc*)t.d_desc.get();
    hipLaunchKernelGGL(partition_sizes_kernel, dim3(C), dim3(1024), 0, d->stream, d_desc, (uint32_t)h->n, t.d_A.get());
    HIPCHK(h, hipGetLastError());
    res.A.resize(C);
    HIPCHK(h, hipMemcpyAsync(res.A.data(), t.d_A.get(), sizeof(double) * C, hipMemcpyDeviceToHost, d->stream));
    if (ages) {
        // (a slot holds the largest table of the entry's chains)
        uint32_t stride = 0;
        for (const ChainDesc& c : desc) stride = std::max(stride, c.ka * c.ka + c.kb * c.kb);
        const size_t pair_bytes = sizeof(uint32_t) * (size_t)stride;
        const bool direct = pair_bytes > kLdsTables;
        uint32_t TA = 1;
        if (4 * pair_bytes <= kLdsTables) TA = 4;
        else if (2 * pair_bytes <= kLdsTables) TA = 2;
        while (TA > 1 && TA / 2 >= ages) TA /= 2;  // (no tile wider than the held ages need)
        const uint32_t age_tiles = (ages + TA - 1) / TA;
        const size_t wgs = (size_t)C * age_tiles;
        int regime = kAuto;
        if (const char* e = std::getenv("BISBM_PARTITION_REGIME")) regime = !strcmp(e, "fused") ? kFused : !strcmp(e, "split") ? kSplit : kAuto;
        int cus = 0;
        HIPCHK(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d->device));
        // many workgroups: one per (chain, age tile) fills the compute units; few: the nodes are split as well
        const bool fused = !direct && (regime == kFused || (regime == kAuto && wgs >= (size_t)cus));
        RESERVE(h, t.d_snn, (size_t)C * ages);
        RESERVE(h, t.d_agree, (size_t)C * ages);
        TraceParams p{};
        p.chains = d_desc;
        p.ring = t.d_ring.get();
        p.row_stride = srow;
        p.C = C, p.ages = ages, p.depth = depth, p.head = head;
        p.n = (uint32_t)h->n, p.na = (uint32_t)h->na;
        p.stride = stride;
        p.hbm_direct = direct ? 1u : 0u;
        p.age_tiles = age_tiles;
        p.snn = t.d_snn.get();
        p.agree = t.d_agree.get();
        const size_t lds = direct ? 0 : (size_t)TA * pair_bytes;
        const uint32_t threads = lds > 40 * 1024 ? 1024u : 256u;
        if (fused) {
            p.nodes_per_block = (p.n + 1023u) & ~1023u;
            HIPCHK(h, launch_trace<true>(TA, dim3((uint32_t)wgs, 1), threads, lds, d->stream, p));
        } else {
            const size_t tile_bytes = (size_t)TA * pair_bytes;
            const size_t per = std::max<size_t>(1, std::min<size_t>(wgs, kTabScratch / tile_bytes));
            RESERVE(h, t.d_tab, per * tile_bytes / sizeof(uint32_t));
            p.tab = t.d_tab.get();
            for (size_t w0 = 0; w0 < wgs; w0 += per) {
                const uint32_t nb = (uint32_t)std::min(per, wgs - w0);
                p.wg0 = (uint32_t)w0;
                // about 8 workgroups per compute unit, at least 4096 nodes each (as bisbm_partition.hip)
                const uint32_t max_chunks = (p.n + 4095u) / 4096u, want = 8u * (uint32_t)std::max(cus, 1);
                const uint32_t chunks = std::max(1u, std::min(max_chunks, (want + nb - 1) / nb));
                p.nodes_per_block = (((p.n + chunks - 1) / chunks) + 1023u) & ~1023u;
                HIPCHK(h, hipMemsetAsync(t.d_tab.get(), 0, (size_t)nb * tile_bytes, d->stream));
                HIPCHK(h, launch_trace<false>(TA, dim3(nb, (p.n + p.nodes_per_block - 1) / p.nodes_per_block), threads, lds, d->stream, p));
                hipLaunchKernelGGL(trace_reduce_kernel, dim3(nb, TA), dim3(64), 0, d->stream, p, TA);
                HIPCHK(h, hipGetLastError());
            }
        }
        res.snn.resize((size_t)C * ages), res.agree.resize((size_t)C * ages);
        HIPCHK(h, hipMemcpyAsync(res.snn.data(), t.d_snn.get(), sizeof(double) * C * ages, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(h, hipMemcpyAsync(res.agree.data(), t.d_agree.get(), sizeof(unsigned long long) * C * ages, hipMemcpyDeviceToHost, d->stream));
    }
    // the push: behind the counting kernels on the same stream, so the oldest slot is read before it is overwritten
    uint8_t* slot = t.d_ring.get() + (size_t)head * C * srow;
    if (d->groups.empty()) {
        HIPCHK(h, hipMemcpyAsync(slot, d->d_labels, (size_t)C * srow, hipMemcpyDeviceToDevice, d->stream));
    } else {
        for (uint32_t c = 0; c < C; ++c) HIPCHK(h, hipMemcpyAsync(slot + (size_t)c * srow, desc[c].row, srow, hipMemcpyDeviceToDevice, d->stream));
    }
    return BISBM_OK;
}

int trace_record(bisbm_engine* h) {
    TraceState& t = h->trace;
    for (bisbm_engine* e : leaves(h))
        if (e->wide)
            return fail(h, BISBM_ERR_UNSUPPORTED, "chain traces serve byte labels only (at most 256 blocks; this handle has %u + %u)", e->ka, e->kb);
    if (!t.depth) return fail(h, BISBM_ERR_STATE, "no snapshot ring: call bisbm_trace_set before bisbm_trace_record");
    for (bisbm_engine* e : leaves(h))
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_trace_record");
    const uint32_t C = h->n_chains, D = t.depth;
    std::vector<uint32_t> ka(C), kb(C);
    for (uint32_t c = 0; c < C; ++c) {
        uint32_t local = 0;
        const bisbm_engine* e = leaf_of_chain(h, c, &local);
        ka[c] = e->ka, kb[c] = e->kb;
        if (t.records && (ka[c] != t.snap_ka[c] || kb[c] != t.snap_kb[c]))
            return fail(h, BISBM_ERR_STATE, "chain %u has %u + %u blocks, its held snapshots were taken with %u + %u: bisbm_trace_reset first", c, ka[c], kb[c],
                        t.snap_ka[c], t.snap_kb[c]);
    }
    // step 1: the description lengths (the double bisbm_entropy returns)
    std::vector<double> S(C);
    if (int rc = bisbm_entropy(h, S.data())) return rc;
    // step 2 on every device entry, side by side on the entries' streams
    const uint32_t ages = (uint32_t)std::min<uint64_t>(D, t.records), head = (uint32_t)(t.records % D);
    const std::vector<bisbm_engine*> entries = device_entries(h);
    std::vector<EntryResult> res(entries.size());
    for (size_t i = 0; i < entries.size(); ++i)
        if (int rc = enqueue_entry(h, entries[i], D, ages, head, res[i])) return rc;
    for (bisbm_engine* d : entries) {
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
    }
    // steps 3 and 4 on the host, in the handle's chain order
    const double n = (double)h->n, nan = std::numeric_limits<double>::quiet_NaN();
    t.S.insert(t.S.end(), S.begin(), S.end());
    for (size_t i = 0; i < entries.size(); ++i) {
        const uint32_t first = h->devs.empty() ? 0u : h->dev_first[i];
        for (uint32_t l = 0; l < entries[i]->n_chains; ++l) {
            const uint32_t c = first + l;
            const double A_now = res[i].A[l];
            t.H.push_back(std::log(n) - A_now / n);
            for (uint32_t a = 0; a < D; ++a) {
                if (a >= ages) {
                    t.vi_last[(size_t)c * D + a] = nan;
                    continue;
                }
                const double A_then = t.A_ring[(size_t)((head + D - 1 - a) % D) * C + c];
                const double v = ((A_now + A_then) - 2. * res[i].snn[(size_t)l * ages + a]) / n;
                const double vi = v > 0. ? v : 0.;
                t.vi_last[(size_t)c * D + a] = vi;
                t.vi_sum[(size_t)c * D + a] += vi;
                t.agree_sum[(size_t)c * D + a] += res[i].agree[(size_t)l * ages + a];
            }
        }
    }
    for (uint32_t a = 0; a < ages; ++a) t.pairs[a] += 1;
    for (size_t i = 0; i < entries.size(); ++i) {
        const uint32_t first = h->devs.empty() ? 0u : h->dev_first[i];
        for (uint32_t l = 0; l < entries[i]->n_chains; ++l) t.A_ring[(size_t)head * C + first + l] = res[i].A[l];
    }
    if (!t.records) t.snap_ka = ka, t.snap_kb = kb;
    t.records += 1;
    return BISBM_OK;
}

}  // namespace

extern "C" {

int bisbm_trace_set(bisbm_handle h, uint32_t depth) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (depth > 1024) return fail(h, BISBM_ERR_INVALID_ARG, "depth %u: a chain trace holds at most 1024 snapshots", depth);
    if (depth && any_wide(h)) return fail(h, BISBM_ERR_UNSUPPORTED, "chain traces serve byte labels only (at most 256 blocks)");
    if (h->n >= 0xFFFFFFFFull - 8192) return fail(h, BISBM_ERR_UNSUPPORTED, "more than 2^32 - 8193 nodes");
    DeviceGuard guard;
    try {
        for (bisbm_engine* d : device_entries(h)) drop(d->trace);
        h->trace.depth = 0;
        forget(h);
        for (bisbm_engine* d : device_entries(h)) {
            if (!depth) break;
            HIPCHK(h, hipSetDevice(d->device));
            const size_t bytes = (size_t)depth * d->n_chains * d->label_stride;
            if (d->trace.d_ring.reserve(bytes) != hipSuccess) {
                for (bisbm_engine* x : device_entries(h)) drop(x->trace);
                return fail(h, BISBM_ERR_HIP, "bisbm_trace_set: %zu bytes of device memory for the snapshot ring (%u snapshots x %u chains x %zu) on device %d could not be allocated",
                            bytes, depth, d->n_chains, d->label_stride, d->device);
            }
        }
        h->trace.depth = depth;
        forget(h);
    } catch (const std::bad_alloc&) {
        return fail(h, BISBM_ERR_STATE, "out of host memory");
    }
    return BISBM_OK;
}

int bisbm_trace_reset(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    try {
        forget(h);
    } catch (const std::bad_alloc&) {
        return fail(h, BISBM_ERR_STATE, "out of host memory");
    }
    return BISBM_OK;
}

int bisbm_trace_record(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    DeviceGuard guard;
    try {
        return trace_record(h);
    } catch (const std::bad_alloc&) {
        return fail(h, BISBM_ERR_STATE, "out of host memory");
    }
}

int bisbm_trace_get_lags(bisbm_handle h, double* vi_sum, uint64_t* agree_sum, double* vi_last, uint64_t* pairs, uint64_t* records) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const TraceState& t = h->trace;
    if (!t.depth) return fail(h, BISBM_ERR_STATE, "no snapshot ring: call bisbm_trace_set first");
    if (vi_sum) std::copy(t.vi_sum.begin(), t.vi_sum.end(), vi_sum);
    if (agree_sum) std::copy(t.agree_sum.begin(), t.agree_sum.end(), agree_sum);
    if (vi_last) std::copy(t.vi_last.begin(), t.vi_last.end(), vi_last);
    if (pairs) std::copy(t.pairs.begin(), t.pairs.end(), pairs);
    if (records) *records = t.records;
    return BISBM_OK;
}

int bisbm_trace_get_series(bisbm_handle h, int what, double* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const TraceState& t = h->trace;
    if (!t.depth) return fail(h, BISBM_ERR_STATE, "no snapshot ring: call bisbm_trace_set first");
    if (what != BISBM_TRACE_S && what != BISBM_TRACE_H) return fail(h, BISBM_ERR_INVALID_ARG, "what must be BISBM_TRACE_S or BISBM_TRACE_H, got %d", what);
    if (!out) return fail(h, BISBM_ERR_INVALID_ARG, "out is NULL");
    const std::vector<double>& x = what == BISBM_TRACE_S ? t.S : t.H;
    std::copy(x.begin(), x.end(), out);
    return BISBM_OK;
}

int bisbm_trace_summary(uint64_t T, uint32_t C, const double* x, double window, double* tau_out, uint32_t* window_out, double* rhat_out) {
    if (T < 4 || C == 0 || !x) return fail(nullptr, BISBM_ERR_INVALID_ARG, "a series of at least 4 records of at least 1 chain is needed (T = %llu, C = %u)", (unsigned long long)T, C);
    if (!std::isfinite(window) || !(window > 0.)) return fail(nullptr, BISBM_ERR_INVALID_ARG, "the window factor must be finite and > 0, got %g", window);
    for (uint64_t t = 0; t < T; ++t)
        for (uint32_t c = 0; c < C; ++c)
            if (!std::isfinite(x[t * C + c])) return fail(nullptr, BISBM_ERR_INVALID_ARG, "x[%llu][%u] is not finite", (unsigned long long)t, c);
    try {
        const uint64_t half = T / 2;
        const double dT = (double)T;
        std::vector<double> d(T);
        for (uint32_t c = 0; c < C; ++c) {
            double sum = 0.;
            for (uint64_t t = 0; t < T; ++t) sum += x[t * C + c];
            const double mu = sum / dT;
            for (uint64_t t = 0; t < T; ++t) d[t] = x[t * C + c] - mu;
            auto gamma = [&](uint64_t k) {
                double g = 0.;
                for (uint64_t t = 0; t + k < T; ++t) g += d[t] * d[t + k];
                return g / dT;
            };
            const double g0 = gamma(0);
            double acc = std::numeric_limits<double>::infinity();
            uint64_t M = 0;
            if (g0 != 0.) {
                acc = 1.;
                for (uint64_t k = 1; k <= half; ++k) {
                    acc = acc + 2. * (gamma(k) / g0);
                    M = k;
                    if ((double)k >= window * acc) break;
                }
            }
            if (tau_out) tau_out[c] = acc;
            if (window_out) window_out[c] = (uint32_t)M;
        }
        if (rhat_out) {
            const double dh = (double)half, two_c = (double)(2 * (uint64_t)C);
            std::vector<double> m(2 * (size_t)C), v(2 * (size_t)C);
            for (size_t j = 0; j < 2 * (size_t)C; ++j) {
                const uint32_t c = (uint32_t)(j % C);
                const uint64_t t0 = j < C ? 0 : T - half;
                double sum = 0.;
                for (uint64_t t = 0; t < half; ++t) sum += x[(t0 + t) * C + c];
                m[j] = sum / dh;
                double sq = 0.;
                for (uint64_t t = 0; t < half; ++t) {
                    const double e = x[(t0 + t) * C + c] - m[j];
                    sq += e * e;
                }
                v[j] = sq / (double)(half - 1);
            }
            double sv = 0., sm = 0.;
            for (double y : v) sv += y;
            for (double y : m) sm += y;
            const double W = sv / two_c, mbar = sm / two_c;
            double sb = 0.;
            for (double y : m) {
                const double e = y - mbar;
                sb += e * e;
            }
            const double Bn = sb / (two_c - 1.);
            *rhat_out = W == 0. ? std::numeric_limits<double>::quiet_NaN() : std::sqrt((((double)(half - 1) / dh) * W + Bn) / W);
        }
    } catch (const std::bad_alloc&) {
        return fail(nullptr, BISBM_ERR_STATE, "out of host memory");
    }
    return BISBM_OK;
}

}  // extern "C"
