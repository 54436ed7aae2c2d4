// bisbm_align.hip -- aligned marginal samples (include/bisbm.h, "Label alignment before pooling" and "Mode-resolved
// marginals").  A block label means something only inside one chain, so before the chains' samples are pooled into a histogram
// every chain is renumbered to the histogram's reference partition.  A mode-resolved sample keeps one histogram per mode, each
// with its reference; the pooled aligned sample is the same thing with one mode that holds every chain.  One pipeline serves
// both, indexed by the position y in the engine's list of counted chains (sorted by (mode, chain)); per sample it
//   1. counts the overlap table C[r][s] of the labels of chain list[y] with the reference of its mode, per node type
//      (align_overlap_kernel),
//   2. finds the permutation of the chain's blocks that maximises the overlap, exactly (align_assign_kernel: one wavefront per
//      position and type runs the shortest-augmenting-path assignment of bisbm_align_assignment below),
//   3. counts the chain's labels through that permutation into its mode's histogram (marginals_aligned_kernel: a mode's list
//      positions are contiguous, so their permutation rows are staged in LDS in chunks).
// Integer adds only: nothing depends on an order.  The chains' own state is only read.  This unit also holds the pooled
// histogram's part of the C ABI; the per-mode calls are bisbm_mode_marginals.hip.
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr long long kInf = 0x3fffffffffffffffLL;

// ------------------------------------------------------------------------------------------
// 1. overlap tables: tab[y][ka*ka + kb*kb], type a at 0 (C[r][s] at r*ka + s), type b at ka*ka (r*kb + s), r = the chain's
// label, s = the reference's, both within the type.  Integer atomics: the tables do not depend on the order of the adds.
// ------------------------------------------------------------------------------------------
enum TableMode { kTablePerWave = 0, kTablePerBlock = 1, kTableInHbm = 2 };

// kTablePerWave: a table per wave in LDS (an aligned chain sends most nodes of a wave to the K diagonal cells: the four waves
// do not queue on each other's cells), summed into HBM at the end; kTablePerBlock: one table in LDS; kTableInHbm: the table is
// too large for a useful occupancy, count straight into HBM.
template <int MODE>
__global__ __launch_bounds__(256) void align_overlap_kernel(OverlapParams p) {
    extern __shared__ __align__(16) uint32_t lds_tab[];
    const uint32_t y = blockIdx.y;
    const uint32_t T = p.ka * p.ka + p.kb * p.kb;
    uint32_t* out = p.tab + (size_t)y * T;
    uint32_t* t = MODE == kTableInHbm ? out : lds_tab + (MODE == kTablePerWave ? (threadIdx.x / 64) * T : 0);
    if constexpr (MODE != kTableInHbm) {
        const uint32_t tot = MODE == kTablePerWave ? 4 * T : T;
        for (uint32_t i = threadIdx.x; i < tot; i += 256) lds_tab[i] = 0;
        __syncthreads();
    }
    const uint8_t* lab = p.labels + (size_t)p.list[y] * p.label_stride;
    const uint8_t* ref = p.ref + (size_t)p.ref_row[y] * p.label_stride;
    const uint32_t v0 = blockIdx.x * p.nodes_per_block;  // (a multiple of 1024: the word loads below are aligned)
    const uint32_t v1 = min(p.n, v0 + p.nodes_per_block);
    for (uint32_t w = v0 + 4 * threadIdx.x; w < v1; w += 4 * 256) {
        // (w + 3 < label_stride: label rows and reference rows are padded to a multiple of 256 labels)
        const uint32_t L = *(const uint32_t*)(lab + w);
        const uint32_t R = *(const uint32_t*)(ref + w);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t v = w + j;
            if (v >= v1) break;
            const bool tb = v >= p.na;
            const uint32_t base = tb ? p.ka : 0u, kt = tb ? p.kb : p.ka;
            const uint32_t r = ((L >> (8 * j)) & 0xffu) - base, s = ((R >> (8 * j)) & 0xffu) - base;
            if (r < kt && s < kt) atomicAdd(t + (tb ? p.ka * p.ka : 0u) + r * kt + s, 1u);
        }
    }
    if constexpr (MODE != kTableInHbm) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < T; i += 256) {
            uint32_t x = lds_tab[i];
            if (MODE == kTablePerWave) x += lds_tab[T + i] + lds_tab[2 * T + i] + lds_tab[3 * T + i];
            if (x) atomicAdd(out + i, x);
        }
    }
}

// ------------------------------------------------------------------------------------------
// 2. assignment: one wavefront per (chain, type).  The solver of bisbm_align_assignment, 1-based as there: column 0 is the
// virtual start column, p[j] the row (1..K) assigned to column j.  Lane l owns columns 1 + l + 64 q (q < 4: K <= 255), their
// dual v, least reduced distance minv and visited bit in registers; the row duals u, p and the path links `way` are in LDS.
// The argmin of a Dijkstra step (least minv, ties -> lowest column) is a wave reduction.
// ------------------------------------------------------------------------------------------
struct AssignParams {
    const uint32_t* tab;
    uint32_t ka, kb;
    uint8_t* perm;   // [chain][ka + kb]
    uint64_t* tot;   // [chain][2]
};

constexpr int kColsPerLane = 4;

__global__ __launch_bounds__(64) void align_assign_kernel(AssignParams p) {
    __shared__ long long u[256];
    __shared__ uint32_t pr[256], way[256];
    const uint32_t c = blockIdx.x, type = blockIdx.y, lane = threadIdx.x;
    const uint32_t K = type ? p.kb : p.ka;
    const uint32_t* C = p.tab + (size_t)c * (p.ka * p.ka + p.kb * p.kb) + (type ? p.ka * p.ka : 0u);
    uint32_t mx = 0;
    for (uint32_t i = lane; i < K * K; i += 64) mx = max(mx, C[i]);
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
    const long long cmax = mx;
    for (uint32_t i = lane; i <= K; i += 64) u[i] = 0, pr[i] = 0, way[i] = 0;
    long long v[kColsPerLane], minv[kColsPerLane];
#pragma unroll
    for (int q = 0; q < kColsPerLane; ++q) v[q] = 0;
    __syncthreads();
    for (uint32_t i = 1; i <= K; ++i) {
        if (lane == 0) pr[0] = i;
        uint32_t j0 = 0, used = 0;
#pragma unroll
        for (int q = 0; q < kColsPerLane; ++q) minv[q] = kInf;
        __syncthreads();
        while (true) {
#pragma unroll
            for (int q = 0; q < kColsPerLane; ++q)
                if (j0 == 1 + lane + 64 * q) used |= 1u << q;
            const uint32_t i0 = pr[j0];
            const long long ui0 = u[i0];
            const uint32_t* row = C + (size_t)(i0 - 1) * K;
            long long best = kInf;
            uint32_t bj = 0xffffffffu;
#pragma unroll
            for (int q = 0; q < kColsPerLane; ++q) {
                const uint32_t j = 1 + lane + 64 * q;
                if (j <= K && !((used >> q) & 1u)) {
                    const long long cur = cmax - (long long)row[j - 1] - ui0 - v[q];
                    if (cur < minv[q]) {
                        minv[q] = cur;
                        way[j] = j0;
                    }
                    if (minv[q] < best) best = minv[q], bj = j;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const long long ob = __shfl_xor(best, off);
                const uint32_t oj = (uint32_t)__shfl_xor((int)bj, off);
                if (ob < best || (ob == best && oj < bj)) best = ob, bj = oj;
            }
            __syncthreads();  // (every lane has read u[i0] before the duals move)
            if (lane == 0) u[pr[0]] += best;  // column 0 is visited from the start
#pragma unroll
            for (int q = 0; q < kColsPerLane; ++q) {
                const uint32_t j = 1 + lane + 64 * q;
                if (j <= K) {
                    if ((used >> q) & 1u) {
                        u[pr[j]] += best;
                        v[q] -= best;
                    } else {
                        minv[q] -= best;
                    }
                }
            }
            __syncthreads();
            j0 = bj;
            if (pr[j0] == 0) break;
        }
        if (lane == 0) {  // augment along the path
            do {
                const uint32_t j1 = way[j0];
                pr[j0] = pr[j1];
                j0 = j1;
            } while (j0);
        }
        __syncthreads();
    }
    const uint32_t base = type ? p.ka : 0u;
    uint8_t* perm = p.perm + (size_t)c * (p.ka + p.kb) + base;
    unsigned long long total = 0;
#pragma unroll
    for (int q = 0; q < kColsPerLane; ++q) {
        const uint32_t j = 1 + lane + 64 * q;
        if (j <= K) {
            const uint32_t r = pr[j] - 1;
            perm[r] = (uint8_t)(base + j - 1);
            total += C[(size_t)r * K + j - 1];
        }
    }
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
    if (lane == 0) p.tot[(size_t)c * 2 + type] = total;
}

// ------------------------------------------------------------------------------------------
// 3. counting.  Grid (ceil(n / 256), n_modes); thread = node: workgroup (x, g) counts its 256 nodes over the chains of mode g,
// list positions range[g] .. range[g + 1] - 1, through their permutations into slice g of the histogram.  IN_LDS: one row of
// (kmax | 1) counters per thread (the odd stride puts the 64 rows of a wave on 64 different banks), then the permutation rows of
// kPermChunk list positions; otherwise the thread owns row v of slice g and counts straight into it.  COLD_ONLY (replica exchange:
// the pooled sample only, whose list is the identity; AlignPlan::cold_only): position y is chain y, counted while it is on rung 0.  The test is a
// template flag because a branch in the loop over the chains keeps the compiler from batching the label loads of four chains,
// which is worth a third of the kernel's time where nothing is filtered.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kPermChunk = 64;

struct AlignedCountParams {
    uint32_t n, na, ka, kmax, K;
    const uint8_t* labels;
    size_t label_stride;
    const uint32_t* list;   // [position] chain
    const uint32_t* range;  // [n_modes + 1] positions of every mode
    const uint32_t* rung;   // [chain] COLD_ONLY: rung of every chain
    const uint8_t* perm;    // [position][K]
    uint32_t* counts;       // [n_modes][n][kmax]
};

template <bool IN_LDS, bool COLD_ONLY>
__global__ __launch_bounds__(256) void marginals_aligned_kernel(AlignedCountParams p) {
    extern __shared__ __align__(16) uint32_t hist[];
    const uint32_t stride = p.kmax | 1u;
    uint8_t* pm = (uint8_t*)(hist + (IN_LDS ? 256 * stride : 0u));
    const uint32_t g = blockIdx.y;
    const uint32_t y0 = p.range[g], y1 = p.range[g + 1];
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = v < p.n;
    const uint32_t base = v < p.na ? 0u : p.ka;
    uint32_t* out = p.counts + ((size_t)g * p.n + (live ? v : 0u)) * p.kmax;
    uint32_t* row = IN_LDS ? hist + threadIdx.x * stride : out;
    if (IN_LDS)
        for (uint32_t j = 0; j < p.kmax; ++j) row[j] = 0;
    for (uint32_t c0 = y0; c0 < y1; c0 += kPermChunk) {
        const uint32_t nc = min(kPermChunk, y1 - c0);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nc * p.K; i += 256) pm[i] = p.perm[(size_t)c0 * p.K + i];
        __syncthreads();
        if (live)
            for (uint32_t c = 0; c < nc; ++c) {
                const uint32_t chain = COLD_ONLY ? c0 + c : p.list[c0 + c];
                if (!COLD_ONLY || p.rung[chain] == 0u) row[(uint32_t)pm[c * p.K + p.labels[(size_t)chain * p.label_stride + v]] - base] += 1;
            }
    }
    if (IN_LDS && live)
        for (uint32_t j = 0; j < p.kmax; ++j)
            if (row[j]) out[j] += row[j];
}

}  // namespace

// Which overlap-table kernel serves a shape: the per-wave tables up to 64 KiB per workgroup (32 + 32 blocks: 32 KiB), one table
// per workgroup up to 64 KiB, HBM above.  BISBM_ALIGN_TABLE=wave|block|hbm forces a mode where it fits (tools/align_bench.py).
int bisbm::overlap_mode(uint32_t T) {
    const size_t limit = 64 * 1024;
    int mode = 4 * sizeof(uint32_t) * (size_t)T <= limit ? kTablePerWave : sizeof(uint32_t) * (size_t)T <= limit ? kTablePerBlock : kTableInHbm;
    if (const char* e = std::getenv("BISBM_ALIGN_TABLE")) {
        const int want = !strcmp(e, "wave") ? kTablePerWave : !strcmp(e, "block") ? kTablePerBlock : !strcmp(e, "hbm") ? kTableInHbm : -1;
        if (want >= mode) mode = want;
    }
    return mode;
}

hipError_t bisbm::launch_align_assign(const uint32_t* tab, uint32_t ka, uint32_t kb, uint8_t* perm, uint64_t* tot, uint32_t n_tables, hipStream_t stream) {
    AssignParams ap{};
    ap.tab = tab;
    ap.ka = ka;
    ap.kb = kb;
    ap.perm = perm;
    ap.tot = tot;
    hipLaunchKernelGGL(align_assign_kernel, dim3(n_tables, 2), dim3(64), 0, stream, ap);
    return hipGetLastError();
}

hipError_t bisbm::launch_overlap(const OverlapParams& p0, uint32_t n_pos, hipStream_t stream) {
    OverlapParams p = p0;
    const uint32_t T = p.ka * p.ka + p.kb * p.kb;
    // about 8192 workgroups over all tables, at least 4096 nodes each (the LDS tables are zeroed and summed once per workgroup)
    const uint32_t max_chunks = (p.n + 4095) / 4096;
    const uint32_t chunks = std::max(1u, std::min(max_chunks, (8192 + n_pos - 1) / n_pos));
    p.nodes_per_block = (((p.n + chunks - 1) / chunks) + 1023) & ~1023u;
    const dim3 grid((p.n + p.nodes_per_block - 1) / p.nodes_per_block, n_pos), block(256);
    switch (overlap_mode(T)) {
        case kTablePerWave:
            hipLaunchKernelGGL(align_overlap_kernel<kTablePerWave>, grid, block, 4 * sizeof(uint32_t) * T, stream, p);
            break;
        case kTablePerBlock:
            hipLaunchKernelGGL(align_overlap_kernel<kTablePerBlock>, grid, block, sizeof(uint32_t) * T, stream, p);
            break;
        default:
            hipLaunchKernelGGL(align_overlap_kernel<kTableInHbm>, grid, block, 0, stream, p);
    }
    return hipGetLastError();
}

namespace {

template <bool COLD_ONLY>
hipError_t launch_marginals_aligned(const AlignedCountParams& p, uint32_t n_modes, hipStream_t stream) {
    const size_t pm = (size_t)kPermChunk * p.K, hist = sizeof(uint32_t) * 256 * (p.kmax | 1u);
    const dim3 grid((p.n + 255) / 256, n_modes), block(256);
    if (hist + pm > kLdsPerCu) {
        hipLaunchKernelGGL((marginals_aligned_kernel<false, COLD_ONLY>), grid, block, pm, stream, p);
        return hipGetLastError();
    }
    hipError_t e = hipFuncSetAttribute((const void*)marginals_aligned_kernel<true, COLD_ONLY>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(hist + pm));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((marginals_aligned_kernel<true, COLD_ONLY>), grid, block, hist + pm, stream, p);
    return hipGetLastError();
}

// ---- host side --------------------------------------------------------------------------------------------------------

// the host solver (include/bisbm.h): the Jonker-Volgenant / Hungarian shortest-augmenting-path form, 1-based with column 0 as
// the virtual start; the device kernel above runs the same steps
void solve_assignment(uint32_t K, const uint32_t* C, uint32_t* perm, uint64_t* total) {
    long long cmax = 0;
    for (size_t i = 0; i < (size_t)K * K; ++i) cmax = std::max<long long>(cmax, C[i]);
    std::vector<long long> u(K + 1, 0), v(K + 1, 0), minv(K + 1);
    std::vector<uint32_t> p(K + 1, 0), way(K + 1, 0);
    std::vector<char> used(K + 1);
    for (uint32_t i = 1; i <= K; ++i) {
        p[0] = i;
        uint32_t j0 = 0;
        std::fill(minv.begin(), minv.end(), kInf);
        std::fill(used.begin(), used.end(), 0);
        do {
            used[j0] = 1;
            const uint32_t i0 = p[j0];
            long long delta = kInf;
            uint32_t j1 = 0;
            for (uint32_t j = 1; j <= K; ++j)
                if (!used[j]) {
                    const long long cur = cmax - (long long)C[(size_t)(i0 - 1) * K + j - 1] - u[i0] - v[j];
                    if (cur < minv[j]) minv[j] = cur, way[j] = j0;
                    if (minv[j] < delta) delta = minv[j], j1 = j;
                }
            for (uint32_t j = 0; j <= K; ++j)
                if (used[j])
                    u[p[j]] += delta, v[j] -= delta;
                else
                    minv[j] -= delta;
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const uint32_t j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0);
    }
    uint64_t tot = 0;
    for (uint32_t j = 1; j <= K; ++j) {
        perm[p[j] - 1] = j - 1;
        tot += C[(size_t)(p[j] - 1) * K + j - 1];
    }
    if (total) *total = tot;
}

}  // namespace

namespace bisbm {

int aligned_sample(bisbm_engine* e, AlignScratch& s, const AlignPlan& plan, uint32_t first, uint32_t* counts) {
    HIPCHK(e, hipSetDevice(e->device));
    const uint32_t ka = e->ka, kb = e->kb, K = ka + kb, M = plan.n_modes;
    const size_t T = (size_t)ka * ka + (size_t)kb * kb;
    // (pos is empty before a leaf's first sample; the pooled plan's list never moves, and shape groups are leaves of different sizes)
    if (s.list_uploaded != plan.list_serial || s.pos.size() != e->n_chains) {
        // the counted chains of this engine sorted by (mode, chain), the positions of every mode
        s.list.clear();
        s.pos.assign(e->n_chains, BISBM_MODE_NONE);
        std::vector<uint32_t> mode, range(M + 1, 0);
        for (uint32_t g = 0; g < M; ++g) {
            range[g] = (uint32_t)s.list.size();
            for (uint32_t c = 0; c < e->n_chains; ++c)
                if (plan.of_chain ? plan.of_chain[first + c] == g : g == 0) {
                    s.pos[c] = (uint32_t)s.list.size();
                    s.list.push_back(c);
                    mode.push_back(g);
                }
        }
        range[M] = (uint32_t)s.list.size();
        RESERVE(e, s.d_list, s.list.size());
        RESERVE(e, s.d_mode, s.list.size());
        RESERVE(e, s.d_range, M + 1);
        if (!s.list.empty()) {
            HIPCHK(e, hipMemcpyAsync(s.d_list.get(), s.list.data(), sizeof(uint32_t) * s.list.size(), hipMemcpyHostToDevice, e->stream));
            HIPCHK(e, hipMemcpyAsync(s.d_mode.get(), mode.data(), sizeof(uint32_t) * mode.size(), hipMemcpyHostToDevice, e->stream));
        }
        HIPCHK(e, hipMemcpyAsync(s.d_range.get(), range.data(), sizeof(uint32_t) * range.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));  // (the host vectors go)
        s.list_uploaded = plan.list_serial;
    }
    s.have_perm = false;
    const uint32_t Y = (uint32_t)s.list.size();
    if (!Y) return BISBM_OK;  // (no counted chain lives here: the histograms stay as they are)
    if (s.ref_uploaded != plan.ref_serial) {
        RESERVE(e, s.d_ref, (size_t)M * e->label_stride);
        std::vector<uint8_t> ref((size_t)M * e->label_stride, 0);
        for (uint32_t g = 0; g < M; ++g)
            for (uint64_t v = 0; v < e->n; ++v) ref[(size_t)g * e->label_stride + v] = (uint8_t)plan.refs[g].labels[v];
        HIPCHK(e, hipMemcpyAsync(s.d_ref.get(), ref.data(), ref.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        s.ref_uploaded = plan.ref_serial;
    }
    RESERVE(e, s.d_tab, Y * T);
    RESERVE(e, s.d_perm, (size_t)Y * K);
    RESERVE(e, s.d_tot, (size_t)Y * 2);
    HIPCHK(e, hipMemsetAsync(s.d_tab.get(), 0, sizeof(uint32_t) * Y * T, e->stream));
    OverlapParams op{};
    op.labels = e->d_labels;
    op.label_stride = e->label_stride;
    op.ref = s.d_ref.get();
    op.list = s.d_list.get();
    op.ref_row = s.d_mode.get();
    op.n = (uint32_t)e->n;
    op.na = (uint32_t)e->na;
    op.ka = ka;
    op.kb = kb;
    op.tab = s.d_tab.get();
    HIPCHK(e, launch_overlap(op, Y, e->stream));
    HIPCHK(e, launch_align_assign(s.d_tab.get(), ka, kb, s.d_perm.get(), s.d_tot.get(), Y, e->stream));
    AlignedCountParams cp{};
    cp.n = (uint32_t)e->n;
    cp.na = (uint32_t)e->na;
    cp.ka = ka;
    cp.kmax = std::max(ka, kb);
    cp.K = K;
    cp.labels = e->d_labels;
    cp.label_stride = e->label_stride;
    cp.list = s.d_list.get();
    cp.range = s.d_range.get();
    cp.perm = s.d_perm.get();
    cp.counts = counts;
    if (plan.cold_only) {  // replica exchange, pooled: the list is the identity, the kernel counts the cold chains only
        cp.rung = e->temper.d_rung.get();
        HIPCHK(e, launch_marginals_aligned<true>(cp, M, e->stream));
    } else {
        HIPCHK(e, launch_marginals_aligned<false>(cp, M, e->stream));
    }
    if (plan.block_what)  // block summaries: the chains' block states through the same list, ranges and permutations
        if (int rc = block_sums_sample(e, s, plan, Y)) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    s.have_perm = true, s.perm_ka = ka, s.perm_kb = kb;
    return BISBM_OK;
}

int refuse_wide_labels(bisbm_engine* h, uint32_t ka, uint32_t kb) {
    if (!any_wide(h)) return BISBM_OK;
    return fail(h, BISBM_ERR_UNSUPPORTED, "label alignment serves byte labels only (at most 256 blocks; this handle has %u + %u)", ka, kb);
}

int check_reference_labels(bisbm_engine* h, const uint32_t* labels, uint32_t ka, uint32_t kb) {
    for (uint64_t v = 0; v < h->n; ++v) {
        const bool tb = v >= h->na;
        if (labels[v] < (tb ? ka : 0u) || labels[v] >= (tb ? ka + kb : ka))
            return fail(h, BISBM_ERR_INVALID_ARG, "reference label %u of node %llu is outside its type's blocks [%u, %u)", labels[v],
                        (unsigned long long)v, tb ? ka : 0u, tb ? ka + kb : ka);
    }
    return BISBM_OK;
}

int read_alignment(bisbm_engine* h, bisbm_engine* e, const AlignScratch& s, uint32_t y, uint32_t* perm_out, uint64_t* overlap_out) {
    const uint32_t K = e->ka + e->kb;
    std::vector<uint8_t> perm(K);
    uint64_t tot[2];
    HIPCHK(h, hipSetDevice(e->device));
    HIPCHK(h, hipMemcpy(perm.data(), s.d_perm.get() + (size_t)y * K, K, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(tot, s.d_tot.get() + (size_t)y * 2, sizeof(tot), hipMemcpyDeviceToHost));
    if (perm_out)
        for (uint32_t r = 0; r < K; ++r) perm_out[r] = perm[r];
    if (overlap_out) *overlap_out = tot[0] + tot[1];
    return BISBM_OK;
}

int align_accumulate(bisbm_engine* h, uint32_t* device_counts) {
    if (!h->devs.empty() && device_counts)
        return fail(h, BISBM_ERR_UNSUPPORTED, "a handle over several devices accumulates into its own buffers (device_counts must be NULL); bisbm_marginals_map pools them");
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    if (int rc = refuse_wide_labels(h, ka, kb)) return rc;
    if (!device_counts) {
        // (as without the alignment: a histogram of other block counts is started afresh)
        bool stale = false;
        for (bisbm_engine* d : device_entries(h)) stale = stale || !d->counts_fit(ka, kb);
        if (stale)
            if (int rc = bisbm_marginals_reset(h)) return rc;
    }
    AlignState& a = h->align;
    if (a.ref.has && (a.ref.ka != ka || a.ref.kb != kb)) {
        if (a.ref.chain < 0)
            return fail(h, BISBM_ERR_STATE, "the reference partition was set for %u + %u blocks, the chains now have %u + %u: set it again", a.ref.ka,
                        a.ref.kb, ka, kb);
        a.ref.has = false;
    }
    if (!a.ref.has) {
        // the library's reference: the lowest description length (ties -> the lowest global chain id, which is the lowest chain
        // index of the handle); with replica exchange on, among the chains on rung 0 (there are n_chains / L >= 1)
        uint32_t n_chains = 0;
        if (int rc = bisbm_get_sizes(h, nullptr, nullptr, nullptr, &n_chains)) return rc;
        std::vector<double> S(n_chains);
        if (int rc = bisbm_entropy(h, S.data())) return rc;
        std::vector<uint32_t> rung(n_chains, 0);
        if (h->temper.L)
            if (int rc = bisbm_tempering_get(h, rung.data(), nullptr)) return rc;
        if (int rc = pick_reference(h, S, [&](uint32_t c) { return rung[c] == 0u; }, ka, kb, a.ref)) return rc;
        ++a.serial;
    }
    // one mode that holds every chain of the leaf; every leaf counts into the histogram of its device entry (a group's `root`),
    // or into the caller's
    AlignPlan plan;
    plan.refs = &a.ref;
    plan.ref_serial = a.serial;
    plan.cold_only = h->temper.L != 0;
    std::vector<uint32_t> mode_now;  // block summaries: the chains this sample counts (all; under replica exchange those on rung 0)
    if (h->blocks.what) {
        mode_now.assign(h->n_chains, 0u);
        if (h->temper.L) {
            std::vector<uint32_t> rung(h->n_chains, 0);
            if (int rc = bisbm_tempering_get(h, rung.data(), nullptr)) return rc;
            for (uint32_t c = 0; c < h->n_chains; ++c)
                if (rung[c] != 0u) mode_now[c] = BISBM_MODE_NONE;
        }
        if (int rc = block_sums_prepare(h, ka, kb, mode_now, plan)) return rc;
    }
    const int rc = each_leaf(h, [&](bisbm_engine* e) { return aligned_sample(e, e->align.scratch, plan, 0, device_counts ? device_counts : (e->root ? e->root : e)->d_counts); });
    if (rc == BISBM_OK) block_sums_commit(h, mode_now, plan);
    return rc;
}

}  // namespace bisbm

extern "C" {

int bisbm_marginals_set_alignment(bisbm_handle h, int mode) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (mode != BISBM_ALIGN_NONE && mode != BISBM_ALIGN_REFERENCE) return fail(h, BISBM_ERR_INVALID_ARG, "unknown alignment mode %d", mode);
    if (mode != h->align.mode && h->align.samples)
        return fail(h, BISBM_ERR_STATE, "the marginal histogram holds samples of the other alignment mode: bisbm_marginals_reset first");
    h->align.mode = mode;
    return BISBM_OK;
}

int bisbm_marginals_set_reference(bisbm_handle h, const uint32_t* labels) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = refuse_while_modes(h, "bisbm_marginals_set_reference", "bisbm_marginals_set_mode_reference")) return rc;
    AlignState& a = h->align;
    if (!labels) {
        a.ref.has = false;
        return BISBM_OK;
    }
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    if (int rc = check_reference_labels(h, labels, ka, kb)) return rc;
    a.ref.labels.assign(labels, labels + h->n);
    a.ref.has = true, a.ref.chain = -1, a.ref.ka = ka, a.ref.kb = kb;
    ++a.serial;
    return BISBM_OK;
}

int bisbm_marginals_get_reference(bisbm_handle h, uint32_t* labels_out, int64_t* chain_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = refuse_while_modes(h, "bisbm_marginals_get_reference", "bisbm_marginals_get_mode_reference")) return rc;
    const AlignRef& r = h->align.ref;
    if (!r.has) return fail(h, BISBM_ERR_STATE, "no reference partition (none set, and no aligned sample since the last reset)");
    if (labels_out) std::copy(r.labels.begin(), r.labels.end(), labels_out);
    if (chain_out) *chain_out = r.chain;
    return BISBM_OK;
}

int bisbm_marginals_get_alignment(bisbm_handle h, uint32_t chain, uint32_t* perm_out, uint64_t* overlap_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (chain >= h->n_chains) return fail(h, BISBM_ERR_INVALID_ARG, "chain %u out of range", chain);
    if (h->modes.n_modes) return mode_get_alignment(h, chain, perm_out, overlap_out);
    uint32_t local = 0;
    bisbm_engine* e = leaf_of_chain(h, chain, &local);
    const AlignScratch& s = e->align.scratch;
    if (!s.have_perm || s.perm_ka != e->ka || s.perm_kb != e->kb)
        return fail(h, BISBM_ERR_STATE, "chain %u has no aligned sample of its present block counts", chain);
    return read_alignment(h, e, s, s.pos[local], perm_out, overlap_out);
}

int bisbm_align_assignment(uint32_t k, const uint32_t* table, uint32_t* perm_out, uint64_t* total_out) {
    if (k == 0 || !table || !perm_out) return fail(nullptr, BISBM_ERR_INVALID_ARG, "k must be >= 1, table and perm_out non-NULL");
    try {
        solve_assignment(k, table, perm_out, total_out);
    } catch (...) {
        return fail(nullptr, BISBM_ERR_INVALID_ARG, "out of host memory");
    }
    return BISBM_OK;
}

}  // extern "C"
