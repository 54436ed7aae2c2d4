// bisbm_coassign.hip -- co-assignment: how often every node of a query's own type sits in the query's block; the k nodes that do
// so most often are selected on the device by bisbm_topk.hip (no reference counterpart; include/bisbm.h, "Co-assignment").  A
// query is a node q of either type, its candidates are all nodes of its own type in id order (q included), and one counted chain
// adds 1 to count[q][v] iff label_c(v) == label_c(q).  Equality of labels does not depend on how a chain numbers its blocks and
// needs no block tables: chains of any shape, byte and two-byte labels are served, and every result is an integer.
//
// Gather kernel: qlab[chain][slot] = the label of every query in every chain of the engine, once per sample, so the counting
// kernel reads a query's label through a wave-uniform address (a scalar load), stages nothing in LDS and has no barrier.
//
// Count kernel: a workgroup owns kCoassignCandTile candidates x kCoassignTile queries of one type (bisbm_cand_lanes.hpp; with
// two-byte labels a lane's four labels are two words), keeps the 4 x 16 counters of a lane in registers and walks all chains of
// the engine.  With byte labels the four comparisons of a word against a query's label (replicated into the four bytes by the
// gather kernel) are one exact byte-equality on the whole word, and the four 0/1 results are added with one add into a packed
// partial of four byte-wide counters, flushed into the uint32 counters every 255 counted chains.  No two workgroups share a cell
// of `count`: no atomics.
//
// Top-k: the selection of bisbm_topk.hip on the counts, where the one candidate that is not eligible is the query's own node.
#include "bisbm_cand_lanes.hpp"
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

    const CandLanes cl = cand_lanes(first, n_own, cand_tile);
    uint32_t cnt[kCoassignTile][4];
#pragma unroll
    for (uint32_t i = 0; i < kCoassignTile; ++i) {
        const uint32_t* row = i < nq ? p.count + p.off[p.list[q0 + i]] : nullptr;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) cnt[i][j] = (i < nq && cl.valid[j]) ? row[cl.node(j) - first] : 0u;
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
            const uint2 x = cl.any ? *(const uint2*)(lab + (size_t)cl.w * 8) : make_uint2(0u, 0u);
            const uint32_t l[4] = {x.x & 0xffffu, x.x >> 16, x.y & 0xffffu, x.y >> 16};
#pragma unroll
            for (uint32_t i = 0; i < kCoassignTile; ++i) {
                const uint32_t b = ql[i];
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) cnt[i][j] += l[j] == b;
            }
        } else {
            const uint32_t word = cl.any ? *(const uint32_t*)(lab + (size_t)cl.w * 4) : 0u;
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
                if (cl.valid[j]) row[cl.node(j) - first] = cnt[i][j] + ((part[i] >> (8 * j)) & 255u);
        }
    }
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
    return for_cand_grids(first, n_own, p.n_list, kCoassignTile, [&](uint32_t cand_tiles, uint32_t q_tile0, dim3 grid) {
        p.cand_tiles = cand_tiles, p.q_tile0 = q_tile0;
        if (wide)
            hipLaunchKernelGGL((coassign_count_kernel<true, true>), grid, dim3(kLanes), 0, stream, p);
        else if (p.plain)
            hipLaunchKernelGGL((coassign_count_kernel<false, true>), grid, dim3(kLanes), 0, stream, p);
        else
            hipLaunchKernelGGL((coassign_count_kernel<false, false>), grid, dim3(kLanes), 0, stream, p);
    });
}

}  // namespace bisbm

namespace {

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

const uint32_t* counts_of(bisbm_engine* d) { return d->coassign.d_count.get(); }

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
    std::vector<TopkCand> cand(n_queries);  // the candidates: the own type's nodes, of which the query itself is not eligible
    const uint32_t n_a = partition_by_type(q, h->na, list);
    for (uint32_t i = 0; i < n_queries; ++i) {
        const uint32_t first = q[i] < h->na ? 0u : (uint32_t)h->na;
        off[i + 1] = off[i] + (q[i] < h->na ? h->na : h->nb);
        cand[i] = TopkCand{first, q[i] - first};
    }
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
    if (e == hipSuccess) e = s.d_cand.reserve(n_queries);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_q.get(), q.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_off.get(), off.data(), sizeof(uint64_t) * ((size_t)n_queries + 1), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_list.get(), list.data(), sizeof(uint32_t) * n_queries, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_slot.get(), slot.data(), sizeof(uint32_t) * slot.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_cand.get(), cand.data(), sizeof(TopkCand) * n_queries, hipMemcpyHostToDevice, h->stream);
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
    if (const uint64_t terms = total_terms(h, &bisbm_engine::coassign); terms + adds > kMaxTerms)
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
    if (terms_out) *terms_out = total_terms(h, &bisbm_engine::coassign);
    if (!count_out) return BISBM_OK;
    return read_row(h, per_device(h, counts_of), s.off[query_index], (size_t)(s.off[query_index + 1] - s.off[query_index]), count_out);
}

int bisbm_coassign_topk(bisbm_handle h, uint32_t k, uint32_t* node_out, uint32_t* count_out, uint64_t* terms_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const CoassignState& s = h->coassign;
    if (!s.n) return fail(h, BISBM_ERR_STATE, "no queries to count: call bisbm_coassign_set first");
    if (k == 0) return fail(h, BISBM_ERR_INVALID_ARG, "k is 0");
    if (k > kQueryMaxK) return fail(h, BISBM_ERR_UNSUPPORTED, "k = %u: bisbm_coassign_topk selects at most %u nodes per query", k, kQueryMaxK);
    if (!node_out) return fail(h, BISBM_ERR_INVALID_ARG, "node_out is NULL");
    const uint64_t terms = total_terms(h, &bisbm_engine::coassign);
    if (!terms) return fail(h, BISBM_ERR_STATE, "no sample yet: call bisbm_coassign_accumulate before bisbm_coassign_topk");
    if (terms_out) *terms_out = terms;
    CoassignState& w = device_entries(h)[0]->coassign;  // the device that selects
    return topk_select(h, __func__, per_device(h, counts_of), s.off, w.topk, w.d_off.get(), w.d_cand.get(), nullptr, k, node_out, count_out);
}

}  // extern "C"
