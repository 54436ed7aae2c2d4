// bisbm_coassign.hip -- co-assignment: how often every node of a query's own type sits in the query's block, and the k nodes that
// do so most often, selected on the device (no reference counterpart; include/bisbm.h, "Co-assignment").  A query is a node q of
// either type, its candidates are all nodes of its own type in id order (q included), and one counted chain adds 1 to
// count[q][v] iff label_c(v) == label_c(q).  Equality of labels does not depend on how a chain numbers its blocks and needs no
// block tables: chains of any shape, byte and two-byte labels are served, and every result is an integer.
//
// Gather kernel: qlab[chain][slot] = the label of every query in every chain of the engine, once per sample, so the counting
// kernel reads a query's label through a wave-uniform address (a scalar load), stages nothing in LDS and has no barrier.
//
// Count kernel: a workgroup owns kCoassignCandTile candidates (a lane reads its four labels as one word of the chain's label
// row, two words with two-byte labels: coalesced) x kCoassignTile queries of one type, keeps the 4 x 16 counters of a lane in
// registers and walks all chains of the engine.  With byte labels the four comparisons of a word against a query's label
// (replicated into the four bytes by the gather kernel) are one exact byte-equality on the whole word, and the four 0/1 results
// are added with one add into a packed partial of four byte-wide counters, flushed into the uint32 counters every 255 counted
// chains.  No two workgroups share a cell of `count`: no atomics.
//
// Top-k: the exact radix select, ordered compaction and rank sort of bisbm_query_scores.hip on uint32 keys (4 passes of 8
// bits), where the one candidate that is not eligible is the query's own node.
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kLanes = 256;
static_assert(kCoassignCandTile == kLanes * 4, "a lane of the count kernel holds four candidates");
constexpr uint32_t kFlushEvery = 255;  // counted chains a byte-wide partial holds

// 0x01 in every byte in which x and y agree, 0x00 in the others: exact (no carry leaves a byte: the sums stay below 0x100).
// Written with the three-input bit operation of gfx950 (v_bitop3_b32; truth tables with a = 0xf0, b = 0xcc, c = 0xaa), which the
// compiler does not form from the plain expression here: 5 VALU instructions, and the caller's add.
__device__ __forceinline__ uint32_t equal_bytes(uint32_t x, uint32_t y) {
    const uint32_t low = 0x7f7f7f7fu;
    const uint32_t t = __builtin_amdgcn_bitop3_b32(x, y, low, 0x28) + low;  // (x ^ y) & low, + low: bit 7 of a byte = some low bit differs
    const uint32_t e = __builtin_amdgcn_bitop3_b32(t, x, y, 0x09);          // ~(t | (x ^ y)): bit 7 of a byte = the bytes agree
    return (e >> 7) & 0x01010101u;
}

__global__ __launch_bounds__(256) void coassign_gather_kernel(CoassignGatherParams p, int wide) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)p.n_chains * p.q_slots) return;
    const uint32_t c = (uint32_t)(t / p.q_slots), s = (uint32_t)(t - (uint64_t)c * p.q_slots);
    const uint32_t qi = p.slot[s];
    if (qi == 0xffffffffu) {
        p.qlab[t] = 0u;
        return;
    }
    const size_t at = (size_t)c * p.label_stride + p.queries[qi];
    p.qlab[t] = wide ? (uint32_t)((const uint16_t*)p.labels)[at] : (uint32_t)p.labels[at] * 0x01010101u;
}

// WIDE: two-byte labels.  PLAIN (byte labels only): extract, compare and add every cell on its own.
template <bool WIDE, bool PLAIN>
__global__ __launch_bounds__(256) void coassign_count_kernel(CoassignParams p) {
    const uint32_t first = p.type ? p.na : 0u, n_own = p.type ? p.n - p.na : p.na;
    const uint32_t cand_tile = blockIdx.x % p.cand_tiles, q_tile = p.q_tile0 + blockIdx.x / p.cand_tiles, q0 = q_tile * kCoassignTile;
    const uint32_t nq = min(kCoassignTile, p.n_list - q0);

    // lane t holds the four nodes of label group w; the ones outside the candidates are never stored
    const uint32_t w = (first >> 2) + cand_tile * kLanes + threadIdx.x;
    const bool any = (uint64_t)w * 4 < (uint64_t)first + n_own;
    bool valid[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint64_t v = (uint64_t)w * 4 + j;
        valid[j] = v >= first && v < (uint64_t)first + n_own;
    }
    uint32_t cnt[kCoassignTile][4];
#pragma unroll
    for (uint32_t i = 0; i < kCoassignTile; ++i) {
        const uint32_t* row = i < nq ? p.count + p.off[p.list[q0 + i]] : nullptr;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) cnt[i][j] = (i < nq && valid[j]) ? row[(uint64_t)w * 4 + j - first] : 0u;
    }
    uint32_t part[kCoassignTile];  // (packed form) four byte-wide counters per query
#pragma unroll
    for (uint32_t i = 0; i < kCoassignTile; ++i) part[i] = 0u;
    uint32_t pending = 0;  // counted chains in `part`

    // (wave-uniform: scalar loads.  All kCoassignTile slots of the tile are read and counted, also past the last query of the
    // list -- the padding slots exist and hold 0 --, so the chain loop has no branch per query; those counters are never stored.)
    const uint32_t* __restrict__ ql = p.qlab + p.slot0 + q0;
    const size_t row_bytes = p.label_stride * (WIDE ? 2 : 1);
    for (uint32_t c = 0; c < p.n_chains; ++c, ql += p.q_slots) {
        if (p.rung && p.rung[c] != 0u) continue;  // (the same for every lane)
        const uint8_t* lab = p.labels + (size_t)c * row_bytes;
        if constexpr (WIDE) {
            const uint2 x = any ? *(const uint2*)(lab + (size_t)w * 8) : make_uint2(0u, 0u);
            const uint32_t l[4] = {x.x & 0xffffu, x.x >> 16, x.y & 0xffffu, x.y >> 16};
#pragma unroll
            for (uint32_t i = 0; i < kCoassignTile; ++i) {
                const uint32_t b = ql[i];
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) cnt[i][j] += l[j] == b;
            }
        } else {
            const uint32_t word = any ? *(const uint32_t*)(lab + (size_t)w * 4) : 0u;
            if constexpr (PLAIN) {
                const uint32_t l[4] = {word & 255u, (word >> 8) & 255u, (word >> 16) & 255u, word >> 24};
#pragma unroll
                for (uint32_t i = 0; i < kCoassignTile; ++i) {
                    const uint32_t b = ql[i] & 255u;
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) cnt[i][j] += l[j] == b;
                }
            } else {
#pragma unroll
                for (uint32_t i = 0; i < kCoassignTile; ++i) part[i] += equal_bytes(word, ql[i]);
                if (++pending == kFlushEvery) {  // (the same for every lane) a byte holds no more
#pragma unroll
                    for (uint32_t i = 0; i < kCoassignTile; ++i) {
#pragma unroll
                        for (uint32_t j = 0; j < 4; ++j) cnt[i][j] += (part[i] >> (8 * j)) & 255u;
                        part[i] = 0u;
                    }
                    pending = 0;
                }
            }
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kCoassignTile; ++i) {
        if (i < nq) {
            uint32_t* row = p.count + p.off[p.list[q0 + i]];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (valid[j]) row[(uint64_t)w * 4 + j - first] = cnt[i][j] + ((part[i] >> (8 * j)) & 255u);
        }
    }
}

// bisbm_query_scores.hip's query_select_kernel on uint32 keys: one workgroup per query of the chunk
__global__ __launch_bounds__(256) void coassign_select_kernel(CoassignSelectParams p) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[2][2][kLanes / 64];
    __shared__ uint32_t s_key[kQueryMaxK];
    __shared__ uint32_t s_id[kQueryMaxK];
    __shared__ uint32_t s_prefix, s_remaining;
    const uint32_t qi = p.q0 + blockIdx.x, q = p.queries[qi];
    const uint32_t first = q < p.na ? 0u : p.na, n_own = q < p.na ? p.na : p.n - p.na;
    const uint32_t self = q - first;  // the candidate that is not eligible
    const uint32_t* key = p.rows + (p.off[qi] - p.off[p.q0]);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t* node_out = p.node_out + (size_t)blockIdx.x * p.k;
    uint32_t* count_out = p.count_out + (size_t)blockIdx.x * p.k;

    const uint32_t kk = min(p.k, n_own - 1u);
    for (uint32_t e = kk + tid; e < p.k; e += kLanes) node_out[e] = 0xffffffffu, count_out[e] = 0u;
    if (kk == 0) return;

    // the kk-th largest eligible key, byte by byte from the top: `prefix` holds the bytes found, `remaining` the rank within them
    if (tid == 0) s_prefix = 0, s_remaining = kk;
    for (int b = 3; b >= 0; --b) {
        hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        for (uint32_t i = tid; i < n_own; i += kLanes) {
            if (i == self) continue;
            const uint32_t x = key[i];
            if (b == 3 || (x >> (8 * (b + 1))) == (prefix >> (8 * (b + 1)))) atomicAdd(&hist[(x >> (8 * b)) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t rem = s_remaining, bin = 255;
            while (bin > 0 && hist[bin] < rem) rem -= hist[bin], --bin;  // (the bins hold at least `rem` keys in all)
            s_remaining = rem;
            s_prefix = prefix | (bin << (8 * b));
        }
        __syncthreads();
    }
    const uint32_t kth = s_prefix;
    const uint32_t n_ties = s_remaining, n_greater = kk - n_ties;  // ties to take (>= 1), keys above the k-th

    // ordered compaction: the larger keys into [0, n_greater), the first n_ties ties in id order behind them
    uint32_t g_base = 0, t_base = 0, it = 0;
    for (uint32_t s = 0; s < n_own && (g_base < n_greater || t_base < n_ties); s += kLanes, it ^= 1u) {
        const uint32_t i = s + tid;
        const bool in = i < n_own && i != self;
        const uint32_t x = in ? key[i] : 0u;
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
        const uint32_t x = s_key[e], id = s_id[e];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < kk; ++j) rank += (s_key[j] > x) || (s_key[j] == x && s_id[j] < id);
        node_out[rank] = first + id;
        count_out[rank] = x;
    }
}

__global__ __launch_bounds__(256) void coassign_rows_add_kernel(uint32_t* a, const uint32_t* b, uint64_t count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) a[i] += b[i];
}

}  // namespace

namespace bisbm {

hipError_t launch_coassign_gather(const CoassignGatherParams& p, bool wide, hipStream_t stream) {
    const uint64_t cells = (uint64_t)p.n_chains * p.q_slots;
    if (cells == 0) return hipSuccess;
    hipLaunchKernelGGL(coassign_gather_kernel, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, stream, p, wide ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_coassign_count(const CoassignParams& p_in, bool wide, hipStream_t stream) {
    CoassignParams p = p_in;
    if (p.n_list == 0) return hipSuccess;
    const uint64_t first = p.type ? p.na : 0u, n_own = p.type ? p.n - p.na : p.na;  // (a query of the type exists: n_own >= 1)
    const uint64_t groups = ((first + n_own - 1) >> 2) - (first >> 2) + 1;
    p.cand_tiles = (uint32_t)((groups + kLanes - 1) / kLanes);
    // workgroup = candidate tile + cand_tiles * query tile, as launch_query_scores
    const uint32_t q_tiles = (p.n_list + kCoassignTile - 1) / kCoassignTile, per_launch = std::max(1u, (1u << 30) / p.cand_tiles);
    for (p.q_tile0 = 0; p.q_tile0 < q_tiles; p.q_tile0 += per_launch) {
        const dim3 grid(p.cand_tiles * std::min(per_launch, q_tiles - p.q_tile0));
        if (wide)
            hipLaunchKernelGGL((coassign_count_kernel<true, true>), grid, dim3(kLanes), 0, stream, p);
        else if (p.plain)
            hipLaunchKernelGGL((coassign_count_kernel<false, true>), grid, dim3(kLanes), 0, stream, p);
        else
            hipLaunchKernelGGL((coassign_count_kernel<false, false>), grid, dim3(kLanes), 0, stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_coassign_select(const CoassignSelectParams& p, hipStream_t stream) {
    if (p.n_q == 0) return hipSuccess;
    hipLaunchKernelGGL(coassign_select_kernel, dim3(p.n_q), dim3(kLanes), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_coassign_rows_add(uint32_t* a, const uint32_t* b, uint64_t count, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(coassign_rows_add_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, stream, a, b, count);
    return hipGetLastError();
}

}  // namespace bisbm

namespace {

constexpr uint64_t kTopkChunkCells = 1ull << 24;  // cells of one chunk of queries in bisbm_coassign_topk (at least one query)
constexpr uint64_t kMaxTerms = 0xffffffffull;     // what a uint32 cell holds

// the chains one sample of leaf `e` counts
uint64_t counted_chains(const bisbm_engine* e) { return e->temper.L ? e->n_chains / e->temper.L : e->n_chains; }  // (one chain of every ensemble is on rung 0)

// the byte-label form the count kernel runs: BISBM_COASSIGN_FORM=plain selects the extract-compare-add form (the A/B of
// tools/coassign_bench.py; the counts are the same)
int plain_form() {
    const char* v = std::getenv("BISBM_COASSIGN_FORM");
    return v && std::strcmp(v, "plain") == 0;
}

// one sample of the chains of `e` (the handle itself or one of its shape groups) into the counts of `h`, on h's stream
int add_sample(bisbm_engine* h, bisbm_engine* e) {
    CoassignState& s = h->coassign;
    RESERVE(h, s.d_qlab, (size_t)e->n_chains * s.q_slots);
    CoassignGatherParams g{};
    g.n_chains = e->n_chains, g.q_slots = s.q_slots;
    g.slot = s.d_slot.get();
    g.queries = s.d_q.get();
    g.labels = e->d_labels;
    g.label_stride = e->label_stride;
    g.qlab = s.d_qlab.get();
    HIPCHK(h, launch_coassign_gather(g, e->wide, h->stream));
    CoassignParams p{};
    p.n = (uint32_t)h->n;
    p.na = (uint32_t)h->na;
    p.n_chains = e->n_chains;
    p.q_slots = s.q_slots;
    p.plain = plain_form();
    p.off = s.d_off.get();
    p.labels = e->d_labels;
    p.label_stride = e->label_stride;
    p.rung = e->temper.L ? e->temper.d_rung.get() : nullptr;  // replica exchange: the cold chains only
    p.qlab = s.d_qlab.get();
    p.count = s.d_count.get();
    const uint32_t slots_a = (s.n_a + kCoassignTile - 1) / kCoassignTile * kCoassignTile;
    for (uint32_t type = 0; type < 2; ++type) {
        p.type = type;
        p.n_list = type ? s.n - s.n_a : s.n_a;
        p.list = s.d_list.get() + (type ? s.n_a : 0u);
        p.slot0 = type ? slots_a : 0u;
        HIPCHK(h, launch_coassign_count(p, e->wide, h->stream));
    }
    s.terms += counted_chains(e);
    return BISBM_OK;
}

uint64_t total_terms(bisbm_engine* h) {
    uint64_t t = 0;
    for (bisbm_engine* d : device_entries(h)) t += d->coassign.terms;
    return t;
}

}  // namespace

extern "C" {

int bisbm_coassign_set(bisbm_handle h, uint32_t n_queries, const uint32_t* queries) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (n_queries && !queries) return fail(h, BISBM_ERR_INVALID_ARG, "queries is NULL");
    for (uint32_t i = 0; i < n_queries; ++i)  // (before anything changes: a refused call leaves the earlier queries in place)
        if (queries[i] >= h->n)
            return fail(h, BISBM_ERR_INVALID_ARG, "query %u = %u: not a node [0, %llu)", i, queries[i], (unsigned long long)h->n);
    std::vector<uint32_t> q(queries, queries + n_queries), list;
    std::vector<uint64_t> off((size_t)n_queries + 1, 0);
    uint32_t n_a = 0;
    for (uint32_t i = 0; i < n_queries; ++i) {
        off[i + 1] = off[i] + (q[i] < h->na ? h->na : h->nb);
        if (q[i] < h->na) list.push_back(i), ++n_a;
    }
    for (uint32_t i = 0; i < n_queries; ++i)
        if (q[i] >= h->na) list.push_back(i);
    if (!h->devs.empty()) {
        const int rc = on_devices(h, [&](bisbm_engine* d, size_t) { return bisbm_coassign_set(d, n_queries, queries); });
        h->coassign = CoassignState();
        if (rc == BISBM_OK && n_queries) h->coassign.n = n_queries, h->coassign.n_a = n_a, h->coassign.q = q, h->coassign.off = off;
        return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->coassign = CoassignState();  // (the old queries, their counts and buffers go)
    if (n_queries == 0) return BISBM_OK;
    CoassignState& s = h->coassign;
    // the slots of the queries' labels: type-a queries in list order, padded to whole tiles, then the type-b queries likewise
    const uint32_t slots_a = (n_a + kCoassignTile - 1) / kCoassignTile * kCoassignTile;
    const uint32_t slots_b = (n_queries - n_a + kCoassignTile - 1) / kCoassignTile * kCoassignTile;
    std::vector<uint32_t> slot((size_t)slots_a + slots_b, 0xffffffffu);
    for (uint32_t i = 0; i < n_queries; ++i) slot[i < n_a ? i : slots_a + (i - n_a)] = list[i];
    const size_t cells = (size_t)off[n_queries];
    hipError_t e = s.d_count.reserve(cells);
    if (e != hipSuccess) {
        h->coassign = CoassignState();
        return fail(h, BISBM_ERR_HIP, "bisbm_coassign_set: %zu bytes of device memory for the counts of %u queries could not be allocated: %s",
                    cells * sizeof(uint32_t), n_queries, hipGetErrorString(e));
    }
    e = s.d_q.reserve(n_queries);
    if (e == hipSuccess) e = s.d_off.reserve((size_t)n_queries + 1);
    if (e == hipSuccess) e = s.d_list.reserve(n_queries);
    if (e == hipSuccess) e = s.d_slot.reserve(slot.size());
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_q.get(), q.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_off.get(), off.data(), sizeof(uint64_t) * ((size_t)n_queries + 1), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_list.get(), list.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_slot.get(), slot.data(), sizeof(uint32_t) * slot.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.d_count.get(), 0, sizeof(uint32_t) * cells, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        h->coassign = CoassignState();
        return fail(h, BISBM_ERR_HIP, "bisbm_coassign_set: %s", hipGetErrorString(e));
    }
    s.n = n_queries, s.n_a = n_a, s.q_slots = slots_a + slots_b;
    s.q.swap(q), s.off.swap(off);
    return BISBM_OK;
}

int bisbm_coassign_accumulate(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->coassign.n) return fail(h, BISBM_ERR_STATE, "no queries to count: call bisbm_coassign_set first");
    if (int rc = refuse_rungs_over_groups(h)) return rc;
    uint64_t adds = 0;
    for (bisbm_engine* e : leaves(h)) {
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_coassign_accumulate");
        adds += counted_chains(e);
    }
    // (several devices: the counts are added up when they are read, so the bound is on the terms of all devices together)
    if (const uint64_t terms = total_terms(h); terms + adds > kMaxTerms)
        return fail(h, BISBM_ERR_STATE, "bisbm_coassign_accumulate: %llu terms and %llu more chains would pass the 4294967295 a count holds: read the rows and call bisbm_coassign_reset",
                    (unsigned long long)terms, (unsigned long long)adds);
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_coassign_accumulate(d); });
    HIPCHK(h, hipSetDevice(h->device));
    for (bisbm_engine* e : leaves(h))  // (chains grouped by shape: every group adds its chains)
        if (int rc = add_sample(h, e)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_coassign_reset(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->devs.empty()) return on_devices(h, [](bisbm_engine* d, size_t) { return bisbm_coassign_reset(d); });
    h->coassign.terms = 0;
    if (!h->coassign.n) return BISBM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->coassign.d_count.get(), 0, sizeof(uint32_t) * h->coassign.off[h->coassign.n], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

int bisbm_coassign_get_row(bisbm_handle h, uint32_t query_index, uint32_t* count_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const CoassignState& s = h->coassign;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "no queries to count: call bisbm_coassign_set first");
    if (query_index >= s.n) return fail(h, BISBM_ERR_INVALID_ARG, "query index %u: %u queries are set", query_index, s.n);
    if (terms_out) *terms_out = total_terms(h);
    if (!count_out) return BISBM_OK;
    const size_t len = (size_t)(s.off[query_index + 1] - s.off[query_index]);
    DeviceGuard keep;
    std::vector<uint32_t> part(h->devs.empty() ? 0 : len);
    bool first = true;
    for (bisbm_engine* d : device_entries(h)) {  // (several devices: the device rows are added on the host)
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
        uint32_t* dst = h->devs.empty() ? count_out : part.data();
        HIPCHK(h, hipMemcpy(dst, d->coassign.d_count.get() + s.off[query_index], sizeof(uint32_t) * len, hipMemcpyDeviceToHost));
        if (!h->devs.empty())
            for (size_t i = 0; i < len; ++i) count_out[i] = first ? part[i] : count_out[i] + part[i];
        first = false;
    }
    return BISBM_OK;
}

int bisbm_coassign_topk(bisbm_handle h, uint32_t k, uint32_t* node_out, uint32_t* count_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const CoassignState& s = h->coassign;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "no queries to count: call bisbm_coassign_set first");
    if (k == 0) return fail(h, BISBM_ERR_INVALID_ARG, "k is 0");
    if (k > kQueryMaxK) return fail(h, BISBM_ERR_UNSUPPORTED, "k = %u: bisbm_coassign_topk selects at most %u nodes per query", k, kQueryMaxK);
    if (!node_out) return fail(h, BISBM_ERR_INVALID_ARG, "node_out is NULL");
    const uint64_t terms = total_terms(h);
    if (!terms) return fail(h, BISBM_ERR_STATE, "no sample yet: call bisbm_coassign_accumulate before bisbm_coassign_topk");
    if (terms_out) *terms_out = terms;
    const std::vector<bisbm_engine*> entries = device_entries(h);
    bisbm_engine* e = entries[0];  // the device that selects
    CoassignState& w = e->coassign;
    DeviceGuard keep;
    for (bisbm_engine* d : entries) {  // (the counts of every device are complete)
        HIPCHK(h, hipSetDevice(d->device));
        HIPCHK(h, hipStreamSynchronize(d->stream));
    }
    HIPCHK(h, hipSetDevice(e->device));
    for (uint32_t q0 = 0; q0 < s.n;) {
        uint32_t q1 = q0 + 1;
        while (q1 < s.n && s.off[q1 + 1] - s.off[q0] <= kTopkChunkCells) ++q1;
        const size_t cells = (size_t)(s.off[q1] - s.off[q0]), n_q = q1 - q0;
        CoassignSelectParams p{};
        p.n = (uint32_t)h->n, p.na = (uint32_t)h->na, p.q0 = q0, p.n_q = (uint32_t)n_q, p.k = k;
        p.queries = w.d_q.get();
        p.off = w.d_off.get();
        p.rows = w.d_count.get() + s.off[q0];
        if (entries.size() > 1) {  // the other devices' rows are added onto a copy of the first device's
            RESERVE(h, w.d_rows, cells);
            RESERVE(h, w.d_stage, cells);
            HIPCHK(h, hipMemcpyAsync(w.d_rows.get(), p.rows, sizeof(uint32_t) * cells, hipMemcpyDeviceToDevice, e->stream));
            for (size_t j = 1; j < entries.size(); ++j) {
                HIPCHK(h, hipMemcpyPeerAsync(w.d_stage.get(), e->device, entries[j]->coassign.d_count.get() + s.off[q0], entries[j]->device,
                                             sizeof(uint32_t) * cells, e->stream));
                HIPCHK(h, launch_coassign_rows_add(w.d_rows.get(), w.d_stage.get(), cells, e->stream));
            }
            p.rows = w.d_rows.get();
        }
        RESERVE(h, w.d_node, n_q * k);
        RESERVE(h, w.d_val, n_q * k);
        p.node_out = w.d_node.get();
        p.count_out = w.d_val.get();
        HIPCHK(h, launch_coassign_select(p, e->stream));
        HIPCHK(h, hipMemcpyAsync(node_out + (size_t)q0 * k, w.d_node.get(), sizeof(uint32_t) * n_q * k, hipMemcpyDeviceToHost, e->stream));
        if (count_out) HIPCHK(h, hipMemcpyAsync(count_out + (size_t)q0 * k, w.d_val.get(), sizeof(uint32_t) * n_q * k, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(h, hipStreamSynchronize(e->stream));  // (the scratch is reused by the next chunk)
        q0 = q1;
    }
    return BISBM_OK;
}

}  // extern "C"
