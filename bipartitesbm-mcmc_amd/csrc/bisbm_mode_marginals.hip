// bisbm_mode_marginals.hip -- mode-resolved marginals (include/bisbm.h, "Mode-resolved marginals"): one aligned histogram per
// posterior mode, each mode aligned to a reference of its own.  The caller assigns chains to modes (bisbm_marginals_set_modes,
// e.g. from bisbm_partition_modes); a sample then runs the three steps of bisbm_align.hip over the counted chains only:
//   1. overlap tables, indexed by the position y in the engine's chain list (sorted by (mode, chain)): labels from row list[y],
//      the reference from row mode[y] of the [n_modes][label_stride] reference buffer (mode_overlap_kernel, the three table
//      placements of align_overlap_kernel),
//   2. the assignment, align_assign_kernel as it is over the positions,
//   3. counting: workgroup (x, g) counts its 256 nodes over the chains of mode g through their permutations into slice g of
//      the histogram (mode_count_kernel); a mode's list positions are contiguous, so its permutation rows are staged in LDS in
//      chunks exactly as marginals_aligned_kernel stages all chains'.
// Integer adds only: nothing depends on an order.  The chains' own state is only read.
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kNone = BISBM_MODE_NONE;

// ------------------------------------------------------------------------------------------
// 1. overlap tables tab[y][ka*ka + kb*kb] (layout as in bisbm_align.hip)
// ------------------------------------------------------------------------------------------
struct ModeOverlapParams {
    const uint8_t* labels;  // [chain][label_stride]
    size_t label_stride;
    const uint8_t* ref;     // [mode][label_stride] (n used)
    const uint32_t* list;   // [position] chain
    const uint32_t* mode;   // [position] mode
    uint32_t n, na, ka, kb, nodes_per_block;
    uint32_t* tab;
};

enum TableMode { kTablePerWave = 0, kTablePerBlock = 1, kTableInHbm = 2 };  // (the values of overlap_mode)

template <int MODE>
__global__ __launch_bounds__(256) void mode_overlap_kernel(ModeOverlapParams p) {
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
    const uint8_t* ref = p.ref + (size_t)p.mode[y] * p.label_stride;
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

hipError_t launch_mode_overlap(const ModeOverlapParams& p0, uint32_t n_pos, hipStream_t stream) {
    ModeOverlapParams p = p0;
    const uint32_t T = p.ka * p.ka + p.kb * p.kb;
    // the split of launch_overlap (bisbm_align.hip): about 8192 workgroups over all tables, at least 4096 nodes each
    const uint32_t max_chunks = (p.n + 4095) / 4096;
    const uint32_t chunks = std::max(1u, std::min(max_chunks, (8192 + n_pos - 1) / n_pos));
    p.nodes_per_block = (((p.n + chunks - 1) / chunks) + 1023) & ~1023u;
    const dim3 grid((p.n + p.nodes_per_block - 1) / p.nodes_per_block, n_pos), block(256);
    switch (overlap_mode(T)) {
        case kTablePerWave:
            hipLaunchKernelGGL(mode_overlap_kernel<kTablePerWave>, grid, block, 4 * sizeof(uint32_t) * T, stream, p);
            break;
        case kTablePerBlock:
            hipLaunchKernelGGL(mode_overlap_kernel<kTablePerBlock>, grid, block, sizeof(uint32_t) * T, stream, p);
            break;
        default:
            hipLaunchKernelGGL(mode_overlap_kernel<kTableInHbm>, grid, block, 0, stream, p);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// 3. counting.  Grid (ceil(n / 256), n_modes); thread = node.  IN_LDS: one row of (kmax | 1) counters per thread (the odd
// stride puts the 64 rows of a wave on 64 different banks), then the permutation rows of kPermChunk list positions; otherwise
// the thread owns row v of slice g and counts straight into it.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kPermChunk = 64;

struct ModeCountParams {
    uint32_t n, na, ka, kmax, K;
    const uint8_t* labels;
    size_t label_stride;
    const uint32_t* list;   // [position] chain
    const uint32_t* range;  // [n_modes + 1] positions of every mode
    const uint8_t* perm;    // [position][K]
    uint32_t* counts;       // [n_modes][n][kmax]
};

template <bool IN_LDS>
__global__ __launch_bounds__(256) void mode_count_kernel(ModeCountParams p) {
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
            for (uint32_t c = 0; c < nc; ++c) row[(uint32_t)pm[c * p.K + p.labels[(size_t)p.list[c0 + c] * p.label_stride + v]] - base] += 1;
    }
    if (IN_LDS && live)
        for (uint32_t j = 0; j < p.kmax; ++j)
            if (row[j]) out[j] += row[j];
}

hipError_t launch_mode_count(const ModeCountParams& p, uint32_t n_modes, hipStream_t stream) {
    const size_t pm = (size_t)kPermChunk * p.K, hist = sizeof(uint32_t) * 256 * (p.kmax | 1u);
    const dim3 grid((p.n + 255) / 256, n_modes), block(256);
    if (hist + pm > kLdsPerCu) {
        hipLaunchKernelGGL(mode_count_kernel<false>, grid, block, pm, stream, p);
        return hipGetLastError();
    }
    hipError_t e = hipFuncSetAttribute((const void*)mode_count_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(hist + pm));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mode_count_kernel<true>, grid, block, hist + pm, stream, p);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// MAP block and its count of every node from one slice: the most frequent block of the node's type, ties -> the lowest
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mode_map_kernel(const uint32_t* counts, uint32_t n, uint32_t kmax, uint32_t na, uint32_t ka,
                                                       uint16_t* labels_out, uint32_t* top_out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint32_t* row = counts + (size_t)v * kmax;
    uint32_t best = 0, arg = 0;
    for (uint32_t j = 0; j < kmax; ++j) {
        const uint32_t c = row[j];
        if (c > best) best = c, arg = j;
    }
    labels_out[v] = (uint16_t)(arg + (v < na ? 0u : ka));
    top_out[v] = best;
}

// ---- host side --------------------------------------------------------------------------------------------------------

// the calling thread's current device, put back when the call returns: the calls below that visit every device entry on the
// caller's thread must not move a torch caller's later allocations (as the pooling calls of bisbm_multi.hip)
struct CurrentDevice {
    int saved = -1;
    CurrentDevice() {
        if (hipGetDevice(&saved) != hipSuccess) saved = -1;
    }
    ~CurrentDevice() {
        if (saved >= 0) (void)hipSetDevice(saved);
    }
};

// the first chain of device entry i of the handle (a plain handle is its own only entry)
uint32_t entry_first(const bisbm_engine* h, size_t i) { return h->devs.empty() ? 0u : h->dev_first[i]; }

int check_mode(bisbm_engine* h, uint32_t mode) {
    if (!h->modes.n_modes) return fail(h, BISBM_ERR_STATE, "no modes are set: bisbm_marginals_set_modes first");
    if (mode >= h->modes.n_modes) return fail(h, BISBM_ERR_INVALID_ARG, "mode %u out of range: %u modes are set", mode, h->modes.n_modes);
    return BISBM_OK;
}

// one mode-resolved sample of the chains of device entry e (chains first .. of the handle) into its slices
int mode_leaf(bisbm_engine* e, const ModeState& top, uint32_t first) {
    ModeState& s = e->modes;
    HIPCHK(e, hipSetDevice(e->device));
    const uint32_t ka = e->ka, kb = e->kb, K = ka + kb, M = top.n_modes;
    const size_t T = (size_t)ka * ka + (size_t)kb * kb;
    if (s.list_uploaded != top.list_serial) {
        // the counted chains of this entry sorted by (mode, chain), the positions of every mode
        s.list.clear();
        s.pos.assign(e->n_chains, kNone);
        std::vector<uint32_t> mode, range(M + 1, 0);
        for (uint32_t g = 0; g < M; ++g) {
            range[g] = (uint32_t)s.list.size();
            for (uint32_t c = 0; c < e->n_chains; ++c)
                if (top.of_chain[first + c] == g) {
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
        s.list_uploaded = top.list_serial;
    }
    s.have_perm = false;
    const uint32_t Y = (uint32_t)s.list.size();
    if (!Y) return BISBM_OK;  // (no counted chain lives here: the slices stay as they are)
    if (s.ref_uploaded != top.ref_serial) {
        RESERVE(e, s.d_ref, (size_t)M * e->label_stride);
        std::vector<uint8_t> ref((size_t)M * e->label_stride, 0);
        for (uint32_t g = 0; g < M; ++g)
            for (uint64_t v = 0; v < e->n; ++v) ref[(size_t)g * e->label_stride + v] = (uint8_t)top.refs[g].labels[v];
        HIPCHK(e, hipMemcpyAsync(s.d_ref.get(), ref.data(), ref.size(), hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        s.ref_uploaded = top.ref_serial;
    }
    RESERVE(e, s.d_tab, Y * T);
    RESERVE(e, s.d_perm, (size_t)Y * K);
    RESERVE(e, s.d_tot, (size_t)Y * 2);
    HIPCHK(e, hipMemsetAsync(s.d_tab.get(), 0, sizeof(uint32_t) * Y * T, e->stream));
    ModeOverlapParams op{};
    op.labels = e->d_labels;
    op.label_stride = e->label_stride;
    op.ref = s.d_ref.get();
    op.list = s.d_list.get();
    op.mode = s.d_mode.get();
    op.n = (uint32_t)e->n;
    op.na = (uint32_t)e->na;
    op.ka = ka;
    op.kb = kb;
    op.tab = s.d_tab.get();
    HIPCHK(e, launch_mode_overlap(op, Y, e->stream));
    HIPCHK(e, launch_align_assign(s.d_tab.get(), ka, kb, s.d_perm.get(), s.d_tot.get(), Y, e->stream));
    ModeCountParams cp{};
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
    cp.counts = s.d_counts.get();
    HIPCHK(e, launch_mode_count(cp, M, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    s.have_perm = true, s.perm_ka = ka, s.perm_kb = kb;
    return BISBM_OK;
}

// the library's reference of mode g: the labels of its member chain of the lowest description length (ties -> the lowest chain)
int pick_mode_reference(bisbm_engine* h, uint32_t g, const std::vector<double>& S, uint32_t ka, uint32_t kb) {
    ModeState& m = h->modes;
    int64_t pick = -1;
    for (uint32_t c = 0; c < h->n_chains; ++c)
        if (m.of_chain[c] == g && (pick < 0 || S[c] < S[pick])) pick = c;
    ModeRef& r = m.refs[g];
    r.labels.resize((size_t)h->n);
    if (int rc = bisbm_get_memberships(h, (uint32_t)pick, r.labels.data())) return rc;  // (every mode has a member: set_modes)
    r.has = true, r.chain = pick, r.ka = ka, r.kb = kb;
    ++m.ref_serial;
    return BISBM_OK;
}

// does every device entry hold histograms of the present assignment and block counts?
bool histograms_fit(bisbm_engine* h, uint32_t ka, uint32_t kb) {
    for (bisbm_engine* d : device_entries(h))
        if (!d->modes.d_counts || d->modes.hist_ka != ka || d->modes.hist_kb != kb || d->modes.slices != h->modes.n_modes) return false;
    return true;
}

}  // namespace

namespace bisbm {

int refuse_while_modes(bisbm_engine* h, const char* call, const char* per_mode_call) {
    if (!h->modes.n_modes) return BISBM_OK;
    return fail(h, BISBM_ERR_STATE, "%s: mode-resolved marginals are set (%u modes, each in the numbering of its own reference): use %s", call,
                h->modes.n_modes, per_mode_call);
}

int mode_reset(bisbm_engine* h) {
    ModeState& m = h->modes;
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    const uint32_t kmax = std::max(ka, kb);
    const size_t cnt = (size_t)m.n_modes * (size_t)h->n * kmax;
    CurrentDevice keep;
    for (bisbm_engine* d : device_entries(h)) {
        ModeState& s = d->modes;
        HIPCHK(h, hipSetDevice(d->device));
        s.slices = 0;
        RESERVE(h, s.d_counts, cnt);
        HIPCHK(h, hipMemsetAsync(s.d_counts.get(), 0, sizeof(uint32_t) * cnt, d->stream));
        HIPCHK(h, hipStreamSynchronize(d->stream));
        s.slices = m.n_modes, s.hist_ka = ka, s.hist_kb = kb;
        s.have_perm = false;
    }
    std::fill(m.terms.begin(), m.terms.end(), 0);
    for (ModeRef& r : m.refs)
        if (r.has && r.chain >= 0) r.has = false;  // (a caller's reference stays)
    return BISBM_OK;
}

int mode_accumulate(bisbm_engine* h, uint32_t* device_counts) {
    ModeState& m = h->modes;
    if (device_counts)
        return fail(h, BISBM_ERR_UNSUPPORTED, "mode-resolved marginals accumulate into the library's histograms, one per mode (device_counts must be NULL); bisbm_marginals_get_mode reads them");
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "label alignment serves byte labels only (at most 256 blocks; this handle has %u + %u)", ka, kb);
    if (any_grouped(h))
        return fail(h, BISBM_ERR_STATE, "the chains of this handle are grouped by shape (after bisbm_agg_merge_total): no mode-resolved marginals");
    // (histograms of other block counts, after a merge or split, are started afresh, library-chosen references with them)
    if (!histograms_fit(h, ka, kb))
        if (int rc = bisbm_marginals_reset(h)) return rc;
    std::vector<double> S;
    for (uint32_t g = 0; g < m.n_modes; ++g) {
        ModeRef& r = m.refs[g];
        if (r.has && (r.ka != ka || r.kb != kb)) {
            if (r.chain < 0)
                return fail(h, BISBM_ERR_STATE, "the reference partition of mode %u was set for %u + %u blocks, the chains now have %u + %u: set it again", g,
                            r.ka, r.kb, ka, kb);
            r.has = false;
        }
        if (!r.has) {
            if (S.empty()) {
                S.resize(h->n_chains);
                if (int rc = bisbm_entropy(h, S.data())) return rc;
            }
            if (int rc = pick_mode_reference(h, g, S, ka, kb)) return rc;
        }
    }
    const int rc = h->devs.empty() ? mode_leaf(h, m, 0) : on_devices(h, [&](bisbm_engine* d, size_t i) { return mode_leaf(d, m, entry_first(h, i)); });
    if (rc) return rc;
    for (uint32_t c = 0; c < h->n_chains; ++c)
        if (m.of_chain[c] != kNone) m.terms[m.of_chain[c]] += 1;
    return BISBM_OK;
}

int mode_get_alignment(bisbm_engine* h, uint32_t chain, uint32_t* perm_out, uint64_t* overlap_out) {
    if (h->modes.of_chain[chain] == kNone) return fail(h, BISBM_ERR_STATE, "chain %u is in no mode (BISBM_MODE_NONE): it is not counted", chain);
    uint32_t local = chain;
    bisbm_engine* e = h->devs.empty() ? h : h->devs[dev_of_chain(h, chain, &local)];
    const ModeState& s = e->modes;
    if (!s.have_perm || s.perm_ka != e->ka || s.perm_kb != e->kb || s.list_uploaded != h->modes.list_serial || !e->groups.empty())
        return fail(h, BISBM_ERR_STATE, "chain %u has no aligned sample of its present block counts", chain);
    const uint32_t K = e->ka + e->kb, y = s.pos[local];
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

}  // namespace bisbm

extern "C" {

int bisbm_marginals_set_modes(bisbm_handle h, uint32_t n_modes, const uint32_t* mode_of_chain) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    ModeState& m = h->modes;
    if (n_modes && !mode_of_chain) return fail(h, BISBM_ERR_INVALID_ARG, "mode_of_chain is NULL");
    if (n_modes == BISBM_MODE_NONE) return fail(h, BISBM_ERR_INVALID_ARG, "n_modes = %u is the value of BISBM_MODE_NONE", n_modes);
    if (n_modes) {
        std::vector<uint32_t> members(n_modes, 0);
        for (uint32_t c = 0; c < h->n_chains; ++c) {
            if (mode_of_chain[c] == kNone) continue;
            if (mode_of_chain[c] >= n_modes)
                return fail(h, BISBM_ERR_INVALID_ARG, "chain %u is given mode %u: modes are 0 .. %u, or BISBM_MODE_NONE", c, mode_of_chain[c], n_modes - 1);
            members[mode_of_chain[c]] += 1;
        }
        for (uint32_t g = 0; g < n_modes; ++g)
            if (!members[g]) return fail(h, BISBM_ERR_INVALID_ARG, "mode %u has no chain", g);
    }
    if (!n_modes && !m.n_modes) return BISBM_OK;
    if (h->align.samples)
        return fail(h, BISBM_ERR_STATE, "the marginal histogram holds samples counted under the present assignment: bisbm_marginals_reset first");
    if (n_modes && h->temper.L)
        return fail(h, BISBM_ERR_STATE, "replica exchange is on: chains that trade temperatures have no mode of their own (bisbm_tempering_set with L = 0 first)");
    if (n_modes && any_grouped(h))
        return fail(h, BISBM_ERR_STATE, "the chains of this handle are grouped by shape (after bisbm_agg_merge_total): no mode-resolved marginals");
    m.n_modes = n_modes;
    m.of_chain.assign(mode_of_chain, mode_of_chain + (n_modes ? h->n_chains : 0));
    m.refs.assign(n_modes, ModeRef());
    m.terms.assign(n_modes, 0);
    ++m.list_serial, ++m.ref_serial;
    for (bisbm_engine* d : device_entries(h)) {  // (histograms of another assignment are gone; off: the memory goes back)
        d->modes.slices = 0;
        d->modes.have_perm = false;
        d->modes.d_counts.reset();
        if (!n_modes) d->modes = ModeState();
    }
    if (!n_modes) m = ModeState();
    return BISBM_OK;
}

int bisbm_marginals_get_modes(bisbm_handle h, uint32_t* n_modes, uint32_t* mode_of_chain, int64_t* ref_chain, uint64_t* terms) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const ModeState& m = h->modes;
    if (n_modes) *n_modes = m.n_modes;
    if (!m.n_modes) return BISBM_OK;
    if (mode_of_chain) std::copy(m.of_chain.begin(), m.of_chain.end(), mode_of_chain);
    for (uint32_t g = 0; g < m.n_modes; ++g) {
        if (ref_chain) ref_chain[g] = m.refs[g].has ? m.refs[g].chain : -2;
        if (terms) terms[g] = m.terms[g];
    }
    return BISBM_OK;
}

int bisbm_marginals_set_mode_reference(bisbm_handle h, uint32_t mode, const uint32_t* labels) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = check_mode(h, mode)) return rc;
    ModeRef& r = h->modes.refs[mode];
    if (!labels) {
        r.has = false;
        return BISBM_OK;
    }
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    for (uint64_t v = 0; v < h->n; ++v) {
        const bool tb = v >= h->na;
        if (labels[v] < (tb ? ka : 0u) || labels[v] >= (tb ? ka + kb : ka))
            return fail(h, BISBM_ERR_INVALID_ARG, "reference label %u of node %llu is outside its type's blocks [%u, %u)", labels[v],
                        (unsigned long long)v, tb ? ka : 0u, tb ? ka + kb : ka);
    }
    r.labels.assign(labels, labels + h->n);
    r.has = true, r.chain = -1, r.ka = ka, r.kb = kb;
    ++h->modes.ref_serial;
    return BISBM_OK;
}

int bisbm_marginals_get_mode_reference(bisbm_handle h, uint32_t mode, uint32_t* labels_out, int64_t* chain_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = check_mode(h, mode)) return rc;
    const ModeRef& r = h->modes.refs[mode];
    if (!r.has) return fail(h, BISBM_ERR_STATE, "mode %u has no reference partition (none set, and no sample since the last reset)", mode);
    if (labels_out) std::copy(r.labels.begin(), r.labels.end(), labels_out);
    if (chain_out) *chain_out = r.chain;
    return BISBM_OK;
}

int bisbm_marginals_get_mode(bisbm_handle h, uint32_t mode, uint32_t* counts_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!counts_out) return fail(h, BISBM_ERR_INVALID_ARG, "counts_out is NULL");
    if (int rc = check_mode(h, mode)) return rc;
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    const uint32_t kmax = std::max(ka, kb);
    if (!histograms_fit(h, ka, kb)) return fail(h, BISBM_ERR_STATE, "no mode-resolved histogram of the present block counts yet");
    const size_t cnt = (size_t)h->n * kmax;
    std::vector<uint32_t> part;
    bool first = true;
    CurrentDevice keep;
    for (bisbm_engine* d : device_entries(h)) {  // the devices' slices of the mode, added on the host
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
        if (first) {
            HIPCHK(h, hipMemcpy(counts_out, d->modes.d_counts.get() + mode * cnt, sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost));
        } else {
            part.resize(cnt);
            HIPCHK(h, hipMemcpy(part.data(), d->modes.d_counts.get() + mode * cnt, sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < cnt; ++i) counts_out[i] += part[i];
        }
        first = false;
    }
    return BISBM_OK;
}

int bisbm_marginals_map_mode(bisbm_handle h, uint32_t mode, uint32_t* labels_out, uint32_t* top_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!labels_out) return fail(h, BISBM_ERR_INVALID_ARG, "labels_out is NULL");
    if (int rc = check_mode(h, mode)) return rc;
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    const uint32_t kmax = std::max(ka, kb);
    if (!h->modes.terms[mode] || !histograms_fit(h, ka, kb))
        return fail(h, BISBM_ERR_STATE, "mode %u has no sample of the present block counts yet", mode);
    const std::vector<bisbm_engine*> entries = device_entries(h);
    bisbm_engine* e = entries[0];
    ModeState& s = e->modes;
    const size_t cnt = (size_t)h->n * kmax;
    CurrentDevice keep;
    HIPCHK(h, hipSetDevice(e->device));
    const uint32_t* counts = s.d_counts.get() + mode * cnt;
    if (entries.size() > 1) {
        // the other devices' slices of the mode are added onto a copy of the first device's
        RESERVE(h, s.d_sum, cnt);
        RESERVE(h, s.d_stage, cnt);
        HIPCHK(h, hipMemcpyAsync(s.d_sum.get(), counts, sizeof(uint32_t) * cnt, hipMemcpyDeviceToDevice, e->stream));
        for (size_t j = 1; j < entries.size(); ++j) {
            HIPCHK(h, hipMemcpyPeerAsync(s.d_stage.get(), e->device, entries[j]->modes.d_counts.get() + mode * cnt, entries[j]->device,
                                         sizeof(uint32_t) * cnt, e->stream));
            HIPCHK(h, launch_counts_add(s.d_sum.get(), s.d_stage.get(), cnt, e->stream));
        }
        counts = s.d_sum.get();
    }
    RESERVE(h, s.d_lab, (size_t)h->n);
    RESERVE(h, s.d_top, (size_t)h->n);
    hipLaunchKernelGGL(mode_map_kernel, dim3(((uint32_t)h->n + 255) / 256), dim3(256), 0, e->stream, counts, (uint32_t)h->n, kmax, (uint32_t)h->na, ka,
                       s.d_lab.get(), s.d_top.get());
    HIPCHK(h, hipGetLastError());
    std::vector<uint16_t> lab((size_t)h->n);
    HIPCHK(h, hipMemcpyAsync(lab.data(), s.d_lab.get(), sizeof(uint16_t) * h->n, hipMemcpyDeviceToHost, e->stream));
    if (top_out) HIPCHK(h, hipMemcpyAsync(top_out, s.d_top.get(), sizeof(uint32_t) * h->n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(h, hipStreamSynchronize(e->stream));
    for (uint64_t v = 0; v < h->n; ++v) labels_out[v] = lab[v];
    return BISBM_OK;
}

}  // extern "C"
