// bisbm_topk.hip -- the best k candidates of every query, selected on the device: what bisbm_query_scores_topk, bisbm_coassign_topk
// and bisbm_foldin_topk share from "the rows are accumulated" on ("Top-k: one selection").  A query's candidates are the
// cells of its row in id order; which node the first one is and which one cell is the query's own come from a table that the
// *_set calls build (TopkCand), so the kernels here know nothing of node types or row kinds.
//
// Mask kernel: one workgroup per query of a chunk, every entry of the query's list (its CSR row, a virtual node's neighbours)
// marks its cell, one byte per cell.
//
// Select kernel: one workgroup per query.  The cells are non-negative (counts, sums of non-negative terms), so their bit
// patterns order as unsigned integers of the cell's width (Key) -- an exact radix select (sizeof(Key) passes of 8 bits) of the
// k-th largest eligible key, an ordered compaction (ballots and wave offsets, no atomics order) of the larger keys and of the
// first ties in id order, and a rank sort of the k entries by (key descending, id ascending).
//
// Host: topk_select walks the queries in chunks, adds the other devices' rows onto a copy of the first device's in device order,
// masks, selects and copies back; read_row is the same device-order sum of one row on the host.
#include <type_traits>

#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kLanes = 256;

template <class P>
__global__ __launch_bounds__(256) void topk_mask_kernel(const P* ptr, const uint32_t* at, const uint32_t* col, uint32_t q0, const uint64_t* off,
                                                        const TopkCand* cand, uint8_t* mask) {
    const uint32_t qi = q0 + blockIdx.x, i = at ? at[qi] : qi;
    const uint32_t first = cand[qi].first, n_cand = (uint32_t)(off[qi + 1] - off[qi]);
    uint8_t* row = mask + (off[qi] - off[q0]);
    for (uint64_t e = (uint64_t)ptr[i] + threadIdx.x; e < ptr[i + 1]; e += blockDim.x) {  // (a repeated entry marks its cell again)
        const uint32_t x = col[e] - first;
        if (x < n_cand) row[x] = 1;
    }
}

// MASKED: p.mask is given (a kernel of its own: the loops over a row without a mask test nothing per cell but `self`)
// ASC: the smallest cells first -- every key is read complemented, which turns the order of the unsigned keys round and leaves the
// id order of the ties; val_out gets the cells themselves (bisbm_least_settled_topk by stay; the other instances hold none of it)
template <class Key, bool MASKED, bool ASC = false>
__global__ __launch_bounds__(256) void topk_select_kernel(TopkSelectParams<Key> p) {
    constexpr int kTop = (int)sizeof(Key) - 1;  // the highest byte of a key
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[2][2][kLanes / 64];
    __shared__ Key s_key[kQueryMaxK];
    __shared__ uint32_t s_id[kQueryMaxK];
    __shared__ Key s_prefix;
    __shared__ uint32_t s_remaining;
    const uint32_t qi = p.q0 + blockIdx.x;
    const uint32_t first = p.cand[qi].first, self = p.cand[qi].self, n_cand = (uint32_t)(p.off[qi + 1] - p.off[qi]);
    const uint64_t cell0 = p.off[qi] - p.off[p.q0];
    const Key* cells = p.rows + cell0;
    const auto key = [&](uint32_t i) -> Key { return ASC ? (Key)~cells[i] : cells[i]; };
    const uint8_t* mask = MASKED ? p.mask + cell0 : nullptr;
    const auto eligible = [&](uint32_t i) { return !(MASKED && mask[i]) && i != self; };
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t* node_out = p.node_out + (size_t)blockIdx.x * p.k;
    Key* val_out = p.val_out + (size_t)blockIdx.x * p.k;

    uint32_t n_eligible = n_cand - (self < n_cand ? 1u : 0u);
    if constexpr (MASKED) {  // the masked cells are counted
        uint32_t& s_eligible = wsum[0][0][0];  // (wsum is written next in the compaction, barriers away)
        if (tid == 0) s_eligible = 0;
        __syncthreads();
        uint32_t mine = 0;
        for (uint32_t i = tid; i < n_cand; i += kLanes) mine += eligible(i);
        if (mine) atomicAdd(&s_eligible, mine);
        __syncthreads();
        n_eligible = s_eligible;
    }
    const uint32_t kk = min(p.k, n_eligible);
    for (uint32_t e = kk + tid; e < p.k; e += kLanes) node_out[e] = 0xffffffffu, val_out[e] = 0;
    if (kk == 0) return;

    // the kk-th largest eligible key, byte by byte from the top: `prefix` holds the bytes found, `remaining` the rank within them
    if (tid == 0) s_prefix = 0, s_remaining = kk;
    for (int b = kTop; b >= 0; --b) {
        hist[tid] = 0;
        __syncthreads();
        const Key prefix = s_prefix;
        for (uint32_t i = tid; i < n_cand; i += kLanes) {
            if (!eligible(i)) continue;
            const Key x = key(i);
            if (b == kTop || (x >> (8 * (b + 1))) == (prefix >> (8 * (b + 1)))) atomicAdd(&hist[(x >> (8 * b)) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t rem = s_remaining, bin = 255;
            while (bin > 0 && hist[bin] < rem) rem -= hist[bin], --bin;  // (the bins hold at least `rem` keys in all)
            s_remaining = rem;
            s_prefix = prefix | ((Key)bin << (8 * b));
        }
        __syncthreads();
    }
    const Key kth = s_prefix;
    const uint32_t n_ties = s_remaining, n_greater = kk - n_ties;  // ties to take (>= 1), keys above the k-th

    // ordered compaction: the larger keys into [0, n_greater), the first n_ties ties in id order behind them
    uint32_t g_base = 0, t_base = 0, it = 0;
    for (uint32_t s = 0; s < n_cand && (g_base < n_greater || t_base < n_ties); s += kLanes, it ^= 1u) {
        const uint32_t i = s + tid;
        const bool in = i < n_cand && eligible(i);
        const Key x = in ? key(i) : 0;
        const bool isg = in && x > kth, ist = in && x == kth;
        const unsigned long long bg = __ballot(isg), bt = __ballot(ist), below = (1ull << lane) - 1ull;
        if (lane == 0) wsum[it][0][wave] = (uint32_t)__popcll(bg), wsum[it][1][wave] = (uint32_t)__popcll(bt);
        __syncthreads();  // (the other buffer is written next: one barrier per chunk)
        uint32_t g_off = 0, t_off = 0, g_all = 0, t_all = 0;
        for (uint32_t k = 0; k < kLanes / 64; ++k) {
            if (k < wave) g_off += wsum[it][0][k], t_off += wsum[it][1][k];
            g_all += wsum[it][0][k], t_all += wsum[it][1][k];
        }
        if (isg) {
            const uint32_t pos = g_base + g_off + (uint32_t)__popcll(bg & below);
            if (pos < n_greater) s_key[pos] = x, s_id[pos] = i;
        }
        if (ist) {
            const uint32_t pos = t_base + t_off + (uint32_t)__popcll(bt & below);
            if (pos < n_ties) s_key[n_greater + pos] = x, s_id[n_greater + pos] = i;
        }
        g_base += g_all, t_base += t_all;
    }
    __syncthreads();

    // rank of every entry among the kk: (key descending, id ascending); the ids differ, so the ranks are a permutation
    for (uint32_t e = tid; e < kk; e += kLanes) {
        const Key x = s_key[e];
        const uint32_t id = s_id[e];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < kk; ++j) rank += (s_key[j] > x) || (s_key[j] == x && s_id[j] < id);
        node_out[rank] = first + id;
        val_out[rank] = ASC ? (Key)~x : x;
    }
}

template <class T>
__global__ __launch_bounds__(256) void rows_add_kernel(T* a, const T* b, uint64_t count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) a[i] += b[i];
}

constexpr uint64_t kTopkChunkCells = 1ull << 24;  // cells of one chunk of queries in topk_select (at least one query)

// ... or what BISBM_TOPK_CHUNK_CELLS says (a positive integer; anything else is ignored): the tests' way to a second chunk
uint64_t chunk_cells() {
    const char* v = std::getenv("BISBM_TOPK_CHUNK_CELLS");
    if (v && *v >= '0' && *v <= '9') {
        char* end = nullptr;
        const unsigned long long x = std::strtoull(v, &end, 10);
        if (*end == 0 && x > 0) return x;
    }
    return kTopkChunkCells;
}

}  // namespace

namespace bisbm {

hipError_t launch_topk_mask(const TopkMaskLists& l, uint32_t q0, uint32_t n_q, const uint64_t* off, const TopkCand* cand, uint8_t* mask,
                            hipStream_t stream) {
    if (n_q == 0) return hipSuccess;
    if (l.ptr64)
        hipLaunchKernelGGL(topk_mask_kernel<uint64_t>, dim3(n_q), dim3(256), 0, stream, l.ptr64, l.at, l.col, q0, off, cand, mask);
    else
        hipLaunchKernelGGL(topk_mask_kernel<uint32_t>, dim3(n_q), dim3(256), 0, stream, l.ptr32, l.at, l.col, q0, off, cand, mask);
    return hipGetLastError();
}

template <class Key>
hipError_t launch_topk_select(const TopkSelectParams<Key>& p, hipStream_t stream, bool ascending) {
    if (p.n_q == 0) return hipSuccess;
    if (ascending) {  // (the f64 sums without a mask: the one caller)
        if constexpr (sizeof(Key) == 8) {
            if (p.mask) return hipErrorInvalidValue;
            hipLaunchKernelGGL((topk_select_kernel<Key, false, true>), dim3(p.n_q), dim3(kLanes), 0, stream, p);
        } else
            return hipErrorInvalidValue;
    } else if (p.mask)
        hipLaunchKernelGGL((topk_select_kernel<Key, true>), dim3(p.n_q), dim3(kLanes), 0, stream, p);
    else
        hipLaunchKernelGGL((topk_select_kernel<Key, false>), dim3(p.n_q), dim3(kLanes), 0, stream, p);
    return hipGetLastError();
}
template hipError_t launch_topk_select(const TopkSelectParams<uint32_t>&, hipStream_t, bool);
template hipError_t launch_topk_select(const TopkSelectParams<unsigned long long>&, hipStream_t, bool);

template <class T>
hipError_t launch_rows_add(T* a, const T* b, uint64_t count, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(rows_add_kernel<T>, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, stream, a, b, count);
    return hipGetLastError();
}
template hipError_t launch_rows_add(uint32_t*, const uint32_t*, uint64_t, hipStream_t);
template hipError_t launch_rows_add(double*, const double*, uint64_t, hipStream_t);

template <class T>
int read_row(bisbm_engine* h, const std::vector<const T*>& cells, uint64_t at, size_t len, T* out) {
    const std::vector<bisbm_engine*> entries = device_entries(h);
    DeviceGuard keep;
    std::vector<T> part(h->devs.empty() ? 0 : len);
    for (size_t j = 0; j < entries.size(); ++j) {  // (several devices: the device rows are added on the host in device order)
        HIPCHK(h, hipSetDevice(entries[j]->device));
        HIPCHK(h, hipStreamSynchronize(entries[j]->stream));
        T* dst = h->devs.empty() ? out : part.data();
        HIPCHK(h, hipMemcpy(dst, cells[j] + at, sizeof(T) * len, hipMemcpyDeviceToHost));
        if (!h->devs.empty())
            for (size_t i = 0; i < len; ++i) out[i] = j == 0 ? part[i] : out[i] + part[i];
    }
    return BISBM_OK;
}
template int read_row(bisbm_engine*, const std::vector<const uint32_t*>&, uint64_t, size_t, uint32_t*);
template int read_row(bisbm_engine*, const std::vector<const double*>&, uint64_t, size_t, double*);

template <class T>
int topk_select(bisbm_engine* h, const char* fn, const std::vector<const T*>& cells, const std::vector<uint64_t>& off, TopkScratch<T>& w,
                const uint64_t* d_off, const TopkCand* d_cand, const TopkMaskLists* lists, uint32_t k, uint32_t* node_out, T* val_out, bool ascending) {
    using Key = std::conditional_t<sizeof(T) == 8, unsigned long long, uint32_t>;
    const std::vector<bisbm_engine*> entries = device_entries(h);
    bisbm_engine* e = entries[0];  // the device that selects
    const uint32_t n = (uint32_t)off.size() - 1;
    const uint64_t cap = chunk_cells();
    DeviceGuard keep;
    for (bisbm_engine* d : entries) {  // (the rows of every device are complete)
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
    }
    HIPCHK(h, hipSetDevice(e->device));
    for (uint32_t q0 = 0; q0 < n;) {
        uint32_t q1 = q0 + 1;
        while (q1 < n && off[q1 + 1] - off[q0] <= cap) ++q1;
        const size_t n_cells = (size_t)(off[q1] - off[q0]), n_q = q1 - q0;
        const T* rows = cells[0] + off[q0];
        if (entries.size() > 1) {  // the other devices' rows are added onto a copy of the first device's, in device order
            RESERVE_AS(h, fn, w.d_rows, n_cells);
            RESERVE_AS(h, fn, w.d_stage, n_cells);
            HIPCHK(h, hipMemcpyAsync(w.d_rows.get(), rows, sizeof(T) * n_cells, hipMemcpyDeviceToDevice, e->stream));
            for (size_t j = 1; j < entries.size(); ++j) {
                HIPCHK(h, hipMemcpyPeerAsync(w.d_stage.get(), e->device, cells[j] + off[q0], entries[j]->device, sizeof(T) * n_cells, e->stream));
                HIPCHK(h, launch_rows_add(w.d_rows.get(), (const T*)w.d_stage.get(), n_cells, e->stream));
            }
            rows = w.d_rows.get();
        }
        if (lists) {
            RESERVE_AS(h, fn, w.d_mask, n_cells);
            HIPCHK(h, hipMemsetAsync(w.d_mask.get(), 0, n_cells, e->stream));
            HIPCHK(h, launch_topk_mask(*lists, q0, (uint32_t)n_q, d_off, d_cand, w.d_mask.get(), e->stream));
        }
        RESERVE_AS(h, fn, w.d_node, n_q * k);
        RESERVE_AS(h, fn, w.d_val, n_q * k);
        const TopkSelectParams<Key> p{q0, (uint32_t)n_q, k, d_off, d_cand, (const Key*)rows, lists ? w.d_mask.get() : nullptr,
                                      w.d_node.get(), (Key*)w.d_val.get()};
        HIPCHK(h, launch_topk_select(p, e->stream, ascending));
        HIPCHK(h, hipMemcpyAsync(node_out + (size_t)q0 * k, w.d_node.get(), sizeof(uint32_t) * n_q * k, hipMemcpyDeviceToHost, e->stream));
        if (val_out) HIPCHK(h, hipMemcpyAsync(val_out + (size_t)q0 * k, w.d_val.get(), sizeof(T) * n_q * k, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(h, hipStreamSynchronize(e->stream));  // (the scratch is reused by the next chunk)
        q0 = q1;
    }
    return BISBM_OK;
}
template int topk_select(bisbm_engine*, const char*, const std::vector<const uint32_t*>&, const std::vector<uint64_t>&, TopkScratch<uint32_t>&,
                         const uint64_t*, const TopkCand*, const TopkMaskLists*, uint32_t, uint32_t*, uint32_t*, bool);
template int topk_select(bisbm_engine*, const char*, const std::vector<const double*>&, const std::vector<uint64_t>&, TopkScratch<double>&,
                         const uint64_t*, const TopkCand*, const TopkMaskLists*, uint32_t, uint32_t*, double*, bool);

}  // namespace bisbm
