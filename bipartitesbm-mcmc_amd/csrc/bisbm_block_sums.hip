// bisbm_block_sums.hip -- block summaries (include/bisbm.h, "Block summaries"): at every aligned sample the block state of
// every counted chain -- the ka x kb quadrant of m, n_r and m_r -- is carried through the permutation the sample just computed
// for the chain onto its mode's reference and summed, cell by cell, into three 64-bit words (sum, and the low and high half of
// the sum of squares).  Integer adds only: the words depend on no order, on no split of the chains over workgroups and on no
// number of device entries.  The kernel runs inside aligned_sample (bisbm_align.hip) right after the counting kernel, on the
// same list of counted chains, mode ranges and permutations.  This unit also holds the feature's part of the C ABI.
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

constexpr uint32_t kNone = BISBM_MODE_NONE;
constexpr uint64_t kMaxTerms = 1ull << 32;  // chain samples per mode below which no accumulator overflows (x < 2^31)
constexpr uint32_t kChunk = 64;             // list positions whose inverse permutations are staged together (as marginals_aligned_kernel's kPermChunk)
constexpr uint32_t kInFlight = 4;           // chains whose loads a thread issues before it adds

struct BlockSumParams {
    uint32_t ka, kb, K, cells;  // cells = ka*kb + 2 K: E, then N, then D
    const int32_t* m;           // [chain][ka][kb]
    const int32_t* n_r;         // [chain][K]
    const int32_t* m_r;         // [chain][K]
    const uint32_t* list;       // [position] chain
    const uint32_t* range;      // [n_modes + 1] positions of every mode
    const uint32_t* rung;       // [chain] COLD_ONLY: rung of every chain
    const uint8_t* perm;        // [position][K]
    unsigned long long* sums;   // [n_modes][3][cells]
    int32_t* last;              // [position][cells], NULL: not kept
};

// Grid (ceil(cells / 256), n_modes, splits); thread = destination cell of mode g (the gather form: the cell's three accumulators
// stay in registers over all chains of the mode, and nothing is added to memory per chain).  Workgroup (x, g, z) takes the
// chunks z, z + splits, ... of kChunk list positions of the mode; per chunk the INVERSE permutations are built in LDS, then a
// thread reads, for kInFlight chains at a time, the source cell of its destination -- m_c[inv(R)][inv(ka + S) - ka], n_r_c[inv(r)]
// or m_r_c[inv(r)] -- and adds x, (x*x) & 0xffffffff and (x*x) >> 32.  COLD_ONLY (the pooled sample under replica exchange, whose
// list is the identity): a chain off rung 0 adds zeroes.  ATOMIC (splits > 1): several workgroups own a cell, they add their
// words with 64-bit integer atomics; otherwise the thread is the cell's only writer.  No floating point.
template <bool COLD_ONLY, bool ATOMIC>
__global__ __launch_bounds__(256) void block_sums_kernel(BlockSumParams p) {
    extern __shared__ __align__(16) uint8_t inv[];  // [kChunk][K]
    __shared__ uint32_t cid[kChunk], live[kChunk];
    const uint32_t g = blockIdx.y;
    const uint32_t y0 = p.range[g], y1 = p.range[g + 1];
    const uint32_t cell = blockIdx.x * 256 + threadIdx.x;
    const bool valid = cell < p.cells;
    const uint32_t nE = p.ka * p.kb;
    const bool isE = cell < nE;
    const uint32_t rest = isE || !valid ? 0u : cell - nE;  // N: [0, K), D: [K, 2 K)
    const int32_t* src = isE ? p.m : rest < p.K ? p.n_r : p.m_r;
    const size_t stride = isE ? (size_t)nE : (size_t)p.K;
    const uint32_t i0 = isE ? cell / p.kb : rest < p.K ? rest : rest - p.K;  // destination row / block
    const uint32_t i1 = isE ? p.ka + cell % p.kb : 0u;                        // destination column, as a global label
    unsigned long long sum = 0, lo = 0, hi = 0;
    for (uint32_t c0 = y0 + blockIdx.z * kChunk; c0 < y1; c0 += gridDim.z * kChunk) {
        const uint32_t nc = min(kChunk, y1 - c0);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nc * p.K; i += 256) {
            const uint32_t c = i / p.K, r = i - c * p.K;
            inv[c * p.K + p.perm[(size_t)c0 * p.K + i]] = (uint8_t)r;
        }
        if (threadIdx.x < nc) {
            const uint32_t chain = COLD_ONLY ? c0 + threadIdx.x : p.list[c0 + threadIdx.x];
            cid[threadIdx.x] = chain;
            live[threadIdx.x] = COLD_ONLY ? (p.rung[chain] == 0u ? 1u : 0u) : 1u;
        }
        __syncthreads();
        if (!valid) continue;
        for (uint32_t c = 0; c < nc; c += kInFlight) {
            uint32_t x[kInFlight];
#pragma unroll
            for (uint32_t j = 0; j < kInFlight; ++j) {
                const uint32_t cc = min(c + j, nc - 1);  // (past the chunk: the last chain again, masked below)
                const uint8_t* iv = inv + cc * p.K;
                const uint32_t row = iv[i0];
                const uint32_t at = isE ? row * p.kb + ((uint32_t)iv[i1] - p.ka) : row;
                x[j] = (uint32_t)src[(size_t)cid[cc] * stride + at];
            }
#pragma unroll
            for (uint32_t j = 0; j < kInFlight; ++j) {
                if (c + j >= nc) break;
                const uint32_t v = live[c + j] ? x[j] : 0u;
                if (p.last) p.last[(size_t)(c0 + c + j) * p.cells + cell] = (int32_t)v;
                const unsigned long long sq = (unsigned long long)v * v;
                sum += v;
                lo += sq & 0xffffffffull;
                hi += sq >> 32;
            }
        }
    }
    if (!valid) return;
    unsigned long long* out = p.sums + (size_t)g * 3 * p.cells + cell;
    if (ATOMIC) {
        if (sum) atomicAdd(out, sum);
        if (lo) atomicAdd(out + p.cells, lo);
        if (hi) atomicAdd(out + 2 * (size_t)p.cells, hi);
    } else {
        out[0] += sum;
        out[p.cells] += lo;
        out[2 * (size_t)p.cells] += hi;
    }
}

template <bool COLD_ONLY>
hipError_t launch_block_sums(const BlockSumParams& p, uint32_t n_modes, uint32_t n_pos, hipStream_t stream) {
    // One workgroup column per mode leaves the device idle when the modes are few: the chunks of a mode are then split over
    // workgroups (about 512 in all, no more than there are chunks) that add with atomics.  BISBM_BLOCK_SPLIT=<n> forces a
    // split (1: every cell has one owner); the words are the same either way.
    const uint32_t gx = (p.cells + 255) / 256, chunks = (n_pos + kChunk - 1) / kChunk;
    uint32_t splits = std::max(1u, std::min(chunks, 512u / std::max(1u, gx * n_modes)));
    if (const char* e = std::getenv("BISBM_BLOCK_SPLIT")) {
        const long want = std::atol(e);
        if (want >= 1) splits = (uint32_t)std::min<long>(want, 1024);
    }
    const dim3 grid(gx, n_modes, splits), block(256);
    const size_t lds = (size_t)kChunk * p.K;
    if (splits > 1)
        hipLaunchKernelGGL((block_sums_kernel<COLD_ONLY, true>), grid, block, lds, stream, p);
    else
        hipLaunchKernelGGL((block_sums_kernel<COLD_ONLY, false>), grid, block, lds, stream, p);
    return hipGetLastError();
}

uint32_t mode_count(const bisbm_engine* h) { return h->modes.n_modes ? h->modes.n_modes : 1u; }

int refuse_off(bisbm_engine* h, const char* call) {
    if (h->blocks.what) return BISBM_OK;
    return fail(h, BISBM_ERR_STATE, "%s: block sums are off: bisbm_block_sums_set first", call);
}

}  // namespace

namespace bisbm {

void block_sums_restart(bisbm_engine* h) {
    BlockSumState& b = h->blocks;
    ++b.serial;
    b.terms.clear();
    b.last_mode.clear();
}

int block_sums_prepare(bisbm_engine* h, uint32_t ka, uint32_t kb, const std::vector<uint32_t>& mode_now, AlignPlan& plan) {
    BlockSumState& b = h->blocks;
    if (!b.what) return BISBM_OK;
    const uint32_t M = plan.n_modes;
    // (sums of other block counts, after a merge or split, or of another number of modes start afresh)
    if (b.ka != ka || b.kb != kb || (!b.terms.empty() && b.terms.size() != M)) block_sums_restart(h);
    std::vector<uint64_t> add(M, 0);
    for (uint32_t g : mode_now)
        if (g != kNone) add[g] += 1;
    for (uint32_t g = 0; g < M; ++g) {
        const uint64_t have = b.terms.empty() ? 0 : b.terms[g];
        if (have + add[g] > kMaxTerms)
            return fail(h, BISBM_ERR_STATE, "the block sums of mode %u hold %llu chain samples and this sample adds %llu: past 2^32 the sums of squares could overflow (bisbm_marginals_reset starts them afresh)",
                        g, (unsigned long long)have, (unsigned long long)add[g]);
    }
    b.ka = ka, b.kb = kb;
    plan.block_what = b.what;
    plan.block_serial = b.serial;
    return BISBM_OK;
}

void block_sums_commit(bisbm_engine* h, const std::vector<uint32_t>& mode_now, const AlignPlan& plan) {
    BlockSumState& b = h->blocks;
    if (!plan.block_what) return;
    if (b.terms.empty()) b.terms.assign(plan.n_modes, 0);
    for (uint32_t g : mode_now)
        if (g != kNone) b.terms[g] += 1;
    b.last_mode = mode_now;
}

int block_sums_sample(bisbm_engine* e, AlignScratch& s, const AlignPlan& plan, uint32_t n_pos) {
    bisbm_engine* own = e->root ? e->root : e;  // (the groups of a device entry add into the entry's sums)
    BlockSumState& b = own->blocks;
    const uint32_t ka = e->ka, kb = e->kb, K = ka + kb, M = plan.n_modes;
    const size_t cells = (size_t)ka * kb + 2 * (size_t)K;
    if (b.zeroed != plan.block_serial || b.slices != M) {
        b.zeroed = 0;
        RESERVE(e, b.d_sums, (size_t)M * 3 * cells);
        HIPCHK(e, hipMemsetAsync(b.d_sums.get(), 0, sizeof(unsigned long long) * M * 3 * cells, e->stream));
        b.zeroed = plan.block_serial, b.slices = M;
    }
    BlockSumParams p{};
    p.ka = ka, p.kb = kb, p.K = K, p.cells = (uint32_t)cells;
    p.m = e->d_m, p.n_r = e->d_n_r, p.m_r = e->d_m_r;
    p.list = s.d_list.get(), p.range = s.d_range.get(), p.perm = s.d_perm.get();
    p.sums = b.d_sums.get();
    if (plan.block_what & BISBM_BLOCK_KEEP_LAST) {
        e->blocks.last_serial = 0;
        RESERVE(e, e->blocks.d_last, (size_t)n_pos * cells);
        p.last = e->blocks.d_last.get();
        e->blocks.last_serial = plan.block_serial;
    }
    if (plan.cold_only) {
        p.rung = e->temper.d_rung.get();
        HIPCHK(e, launch_block_sums<true>(p, M, n_pos, e->stream));
    } else {
        HIPCHK(e, launch_block_sums<false>(p, M, n_pos, e->stream));
    }
    return BISBM_OK;
}

}  // namespace bisbm

extern "C" {

int bisbm_block_sums_set(bisbm_handle h, uint32_t what) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if ((what & ~(BISBM_BLOCK_SUMS | BISBM_BLOCK_KEEP_LAST)) || what == BISBM_BLOCK_KEEP_LAST)
        return fail(h, BISBM_ERR_INVALID_ARG, "what = %u: 0, BISBM_BLOCK_SUMS or BISBM_BLOCK_SUMS | BISBM_BLOCK_KEEP_LAST", what);
    block_sums_restart(h);
    h->blocks.what = what;
    h->blocks.ka = h->blocks.kb = 0;
    for (bisbm_engine* d : device_entries(h)) {
        if (!what) d->blocks.d_sums.reset();
        d->blocks.zeroed = 0, d->blocks.slices = 0;
    }
    if (!(what & BISBM_BLOCK_KEEP_LAST))
        for (bisbm_engine* e : leaves(h)) {
            e->blocks.d_last.reset();
            e->blocks.last_serial = 0;
        }
    return BISBM_OK;
}

int bisbm_block_sums_get(bisbm_handle h, uint32_t mode, uint64_t* terms, uint64_t* e_out, uint64_t* n_out, uint64_t* d_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = refuse_off(h, "bisbm_block_sums_get")) return rc;
    const BlockSumState& b = h->blocks;
    const uint32_t M = mode_count(h);
    if (mode >= M) return fail(h, BISBM_ERR_INVALID_ARG, "mode %u out of range: the block sums have %u mode%s", mode, M, M == 1 ? " (the pooled histogram's)" : "s");
    uint32_t ka = 0, kb = 0;
    if (int rc = shared_shape(h, &ka, &kb)) return rc;
    const size_t nE = (size_t)ka * kb, K = (size_t)ka + kb, cells = nE + 2 * K;
    // (no sample since the sums started, or the block counts changed since: they are zero until the next sample)
    const bool any = !b.terms.empty() && b.terms.size() == M && b.ka == ka && b.kb == kb;
    if (terms) *terms = any ? b.terms[mode] : 0;
    std::vector<uint64_t> tot(3 * cells, 0), part(3 * cells);
    if (any) {
        DeviceGuard keep;
        for (bisbm_engine* d : device_entries(h)) {  // every entry's sums of its own chains, added on the host
            const BlockSumState& s = d->blocks;
            if (s.zeroed != b.serial || s.slices != M || !s.d_sums) continue;  // (no counted chain of the handle lives there)
            HIPCHK(h, hipSetDevice(d->device));
            HIPCHK(h, hipStreamSynchronize(d->stream));
            HIPCHK(h, hipMemcpy(part.data(), s.d_sums.get() + (size_t)mode * 3 * cells, sizeof(uint64_t) * 3 * cells, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < 3 * cells; ++i) tot[i] += part[i];
        }
    }
    for (size_t w = 0; w < 3; ++w) {
        const uint64_t* src = tot.data() + w * cells;
        if (e_out) std::copy(src, src + nE, e_out + w * nE);
        if (n_out) std::copy(src + nE, src + nE + K, n_out + w * K);
        if (d_out) std::copy(src + nE + K, src + nE + 2 * K, d_out + w * K);
    }
    return BISBM_OK;
}

int bisbm_block_sums_get_last(bisbm_handle h, uint32_t chain, uint32_t* mode_out, int32_t* e_out, int32_t* n_r_out, int32_t* m_r_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = refuse_off(h, "bisbm_block_sums_get_last")) return rc;
    const BlockSumState& b = h->blocks;
    if (!(b.what & BISBM_BLOCK_KEEP_LAST)) return fail(h, BISBM_ERR_STATE, "the last sample's tables are not kept: bisbm_block_sums_set with BISBM_BLOCK_KEEP_LAST");
    if (chain >= h->n_chains) return fail(h, BISBM_ERR_INVALID_ARG, "chain %u out of range", chain);
    if (b.last_mode.empty()) return fail(h, BISBM_ERR_STATE, "no aligned sample since the block sums started");
    if (b.last_mode[chain] == kNone) return fail(h, BISBM_ERR_STATE, "chain %u was not counted by the last sample", chain);
    uint32_t local = chain;
    bisbm_engine* e;
    const AlignScratch* s;
    if (h->modes.n_modes) {  // (a mode's list lives with the device entry: grouped chains are refused under modes)
        e = h->devs.empty() ? h : h->devs[dev_of_chain(h, chain, &local)];
        s = &e->modes.scratch;
    } else {
        e = leaf_of_chain(h, chain, &local);
        s = &e->align.scratch;
    }
    const size_t nE = (size_t)e->ka * e->kb, K = (size_t)e->ka + e->kb, cells = nE + 2 * K;
    if (e->blocks.last_serial != b.serial || !e->blocks.d_last || local >= s->pos.size() || s->pos[local] == kNone || e->ka != b.ka || e->kb != b.kb)
        return fail(h, BISBM_ERR_STATE, "chain %u has no kept tables of its present block counts", chain);
    std::vector<int32_t> row(cells);
    DeviceGuard keep;
    HIPCHK(h, hipSetDevice(e->device));
    HIPCHK(h, hipStreamSynchronize(e->stream));
    HIPCHK(h, hipMemcpy(row.data(), e->blocks.d_last.get() + (size_t)s->pos[local] * cells, sizeof(int32_t) * cells, hipMemcpyDeviceToHost));
    if (mode_out) *mode_out = b.last_mode[chain];
    if (e_out) std::copy(row.begin(), row.begin() + nE, e_out);
    if (n_r_out) std::copy(row.begin() + nE, row.begin() + nE + K, n_r_out);
    if (m_r_out) std::copy(row.begin() + nE + K, row.end(), m_r_out);
    return BISBM_OK;
}

}  // extern "C"
