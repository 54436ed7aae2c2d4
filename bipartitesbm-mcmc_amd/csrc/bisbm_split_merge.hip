// bisbm_split_merge.hip -- split and merge moves: one block divided in two, or two blocks of one type made one, in one accepted or
// rejected move, so that a chain samples (Ka, Kb) with its partition (no reference counterpart; include/bisbm.h, "Split and merge
// moves", states every draw, every order of operations and what a move updates).
//
// Kernel: one wave per chain, one move per launch, on the wave-chain state of bisbm_wave_chain.hpp.  A split needs room for one
// more block of the moving type, so the kernel does not run on the chain's own arrays: sm_pad_kernel copies every chain of a
// group into scratch with a SPARE EMPTY BLOCK PER TYPE -- shape (ka + 1, kb + 1); the spare of type a is label ka, every type-b
// label sits one higher, the spare of type b is the last label -- and split_merge_kernel is launched with that shape.  An empty
// block adds exactly 0 to every dS a restricted step evaluates, so the steps are those of the chain's own shape.  The chain's own
// arrays are never written: a rejection restores everything by construction; an accepted dS goes onto cum_dS in the gather below.
// After a launch in which some chain was accepted the host forms the groups again (regroup): every group that lost or gained a
// chain is made afresh -- sm_gather_kernel copies each of its chains from the scratch of the group it came from and takes the
// spare or emptied labels out on the way -- and its block state rebuilt; the other groups stay as they are.
//
// The restricted step -- the lane <-> non-zero (t, k_t) mapping, the four log_q side by side, the (mantissa, exponent) Q -- is
// reshuffle_kernel's (bisbm_reshuffle.hip), with (home, away) in the place of (r, s); merge_dS runs in the wave with the lanes
// over the other type's blocks and then over the degrees, added in ascending order one v_readlane at a time.
#include "bisbm_engine.hpp"
#include "bisbm_wave_chain.hpp"

#include <chrono>

using namespace bisbm;

namespace bisbm {

namespace {

constexpr uint32_t PHX_SPLIT_MERGE = 11;  // idx = (moves proposed << 32) | k, chain = the chain's global id
constexpr uint32_t kNoCut = 0xffffffffu;

enum : uint32_t { SM_TRANSIT = 0, SM_FREE = 1, SM_FORCED = 2 };

// ka, kb of the WaveChainParams: the shape WITH the spares
struct SplitMergeParams : WaveChainParams {
    uint32_t scans;
    uint32_t k_min[2], k_max[2];
    const uint32_t* proposed;  // [chain] j
    double shape_up[2];        // T(one more block of type t) - T(now)
    double shape_down[2];      // T(one block fewer of type t) - T(now)
    uint32_t* member;          // [chain][nmax]
    uint8_t* orig;             // [chain][nmax]
    uint8_t* launch;           // [chain][nmax]
    bisbm_split_merge_record* record;  // [chain]
};

struct PadParams {
    const uint8_t* labels;  // the group's own arrays
    const int32_t *m, *m_r, *n_r;
    const uint32_t* eta;
    uint8_t* labels_p;  // with the spares
    int32_t *m_p, *m_r_p, *n_r_p;
    uint32_t* eta_p;
    size_t label_stride;
    uint32_t n, ka, kb, D;
};

// a chain's state with a spare empty block per type: block x of the padded numbering is block real(x) of the chain, or a spare
__device__ __forceinline__ uint32_t real_block(uint32_t x, uint32_t ka, uint32_t K) { return x < ka ? x : (x == ka || x > K) ? kNoCut : x - 1u; }

__global__ __launch_bounds__(256) void sm_pad_kernel(PadParams q) {
    const uint32_t chain = blockIdx.x, K = q.ka + q.kb, KP = K + 2u, kbp = q.kb + 1u;
    const uint8_t* src = q.labels + (size_t)chain * q.label_stride;
    uint8_t* dst = q.labels_p + (size_t)chain * q.label_stride;
    for (uint32_t v = threadIdx.x; v < q.n; v += blockDim.x) {
        const uint32_t x = src[v];
        dst[v] = (uint8_t)(x + (x >= q.ka ? 1u : 0u));
    }
    for (uint32_t i = threadIdx.x; i < (q.ka + 1u) * kbp; i += blockDim.x) {
        const uint32_t a = i / kbp, b = i % kbp;
        q.m_p[(size_t)chain * (q.ka + 1u) * kbp + i] = (a < q.ka && b < q.kb) ? q.m[(size_t)chain * q.ka * q.kb + a * q.kb + b] : 0;
    }
    for (uint32_t x = threadIdx.x; x < KP; x += blockDim.x) {
        const uint32_t r = real_block(x, q.ka, K);
        q.m_r_p[(size_t)chain * KP + x] = r == kNoCut ? 0 : q.m_r[(size_t)chain * K + r];
        q.n_r_p[(size_t)chain * KP + x] = r == kNoCut ? 0 : q.n_r[(size_t)chain * K + r];
    }
    for (uint32_t i = threadIdx.x; i < KP * q.D; i += blockDim.x) {
        const uint32_t r = real_block(i / q.D, q.ka, K);
        q.eta_p[(size_t)chain * KP * q.D + i] = r == kNoCut ? 0u : q.eta[((size_t)chain * K + r) * q.D + i % q.D];
    }
}

// One chain of a group that is formed again: its label row in the scratch of the group it came from, the (at most two) labels
// that are taken out on the way -- new = x - (x > cut1) - (x > cut2) --, its scalars, and the dS of its accepted move (0.0 and
// not added otherwise): the running sum advances here, with one add, so a chain's sum and labels change together or not at all.
struct ChainCopy {
    const uint8_t* labels;
    const ChainScalars* scalars;
    uint32_t cut1, cut2;
    uint32_t moved, pad;
    double dS;
};

__global__ __launch_bounds__(256) void sm_gather_kernel(const ChainCopy* jobs, uint8_t* labels, size_t label_stride, uint32_t n, ChainScalars* scalars) {
    const ChainCopy job = jobs[blockIdx.x];
    uint8_t* dst = labels + (size_t)blockIdx.x * label_stride;
    for (uint32_t v = threadIdx.x; v < n; v += blockDim.x) {
        const uint32_t x = job.labels[v];
        dst[v] = (uint8_t)(x - (x > job.cut1 ? 1u : 0u) - (x > job.cut2 ? 1u : 0u));
    }
    if (threadIdx.x == 0) {
        ChainScalars sc = *job.scalars;
        if (job.moved) sc.cum_dS = sc.cum_dS + job.dS;
        scalars[blockIdx.x] = sc;
    }
}

// merge_dS of blocks hg and ag (labels of the launch's numbering, one type) without the shape term: step 5 of the definition
template <bool EL>
__device__ __forceinline__ double merge_dS_blocks(const WaveChain<EL>& wc, const Tables& tab, const TypeView& ty, bool tb, uint32_t hg, uint32_t ag) {
    const uint32_t lane = wc.lane, h_loc = hg - ty.own0, a_loc = ag - ty.own0, D = wc.D;
    double acc_m = 0., acc_e = 0.;
    for (uint32_t t0 = 0; t0 < ty.k_oth; t0 += kWave) {
        const uint32_t cn = ty.k_oth - t0 < (uint32_t)kWave ? ty.k_oth - t0 : (uint32_t)kWave;
        const uint32_t t = t0 + (lane < cn ? lane : cn - 1u);  // (idle lanes read the last entry again)
        const long long m_h = wc.M(tb, h_loc, t), m_a = wc.M(tb, a_loc, t);
        const double term = (lgamma_fast(tab, m_h + 1) + lgamma_fast(tab, m_a + 1)) - lgamma_fast(tab, m_h + m_a + 1);
        for (uint32_t j = 0; j < cn; ++j) acc_m = acc_m + readlane(term, j);
    }
    for (uint32_t k0 = 0; k0 < D; k0 += kWave) {
        const uint32_t cn = D - k0 < (uint32_t)kWave ? D - k0 : (uint32_t)kWave;
        const uint32_t k = k0 + (lane < cn ? lane : cn - 1u);
        const long long e_h = *wc.eta_at(hg * D + k), e_a = *wc.eta_at(ag * D + k);
        const double term = (lgamma_fast(tab, e_h + 1) + lgamma_fast(tab, e_a + 1)) - lgamma_fast(tab, e_h + e_a + 1);
        for (uint32_t j = 0; j < cn; ++j) acc_e = acc_e + readlane(term, j);
    }
    const int m0h = readlane(wc.mr[hg], 0u), m0a = readlane(wc.mr[ag], 0u), n0h = readlane(wc.nr[hg], 0u), n0a = readlane(wc.nr[ag], 0u);
    const double tail1 = lgamma_fast(tab, (long long)m0h + m0a + 1) - (lgamma_fast(tab, (long long)m0h + 1) + lgamma_fast(tab, (long long)m0a + 1));
    const double tail2 = log_q<false>(tab, m0h + m0a, n0h + n0a) - (log_q<false>(tab, m0h, n0h) + log_q<false>(tab, m0a, n0a));
    return ((acc_m + acc_e) + tail1) + tail2;
}

template <bool EL>
__global__ __launch_bounds__(kWave) void split_merge_kernel(SplitMergeParams p) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const uint32_t chain = blockIdx.x;
    if (chain >= p.n_chains) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t nmax = p.na > p.nb ? p.na : p.nb;

    WaveChain<EL> wc;
    wc.load(lds_raw, p, chain);
    int32_t *const mr = wc.mr, *const nr = wc.nr;
    const uint32_t D = wc.D;
    uint8_t* const labels = wc.labels;
    uint32_t* member = p.member + (size_t)chain * nmax;
    uint8_t* orig = p.orig + (size_t)chain * nmax;
    uint8_t* launch = p.launch + (size_t)chain * nmax;
    __syncthreads();

    const Tables tab{p.lgamma_tab, p.lgamma_size, p.q_tab, p.q_stride, p.log_tab};
    const uint32_t chain_gid = chain_gid_of(p, chain);
    const double beta = p.beta;
    const uint32_t ka = p.ka - 1u, kb = p.kb - 1u, K = ka + kb;  // the chain's own shape
    const uint32_t pairs_a = ka * (ka - 1u) / 2u, n_pairs = pairs_a + kb * (kb - 1u) / 2u;
    const uint64_t idx0 = (uint64_t)p.proposed[chain] << 32;

    bisbm_split_merge_record rec{};
    rec.ka_before = rec.ka_after = ka, rec.kb_before = rec.kb_after = kb;
    rec.lnA = -INFINITY;
    const U4 x0 = phx_draw(p.seed, chain_gid, PHX_SPLIT_MERGE, idx0);
    const U4 acc_draw = phx_draw(p.seed, chain_gid, PHX_SPLIT_MERGE, idx0 | 1u);
    rec.u_acc = u53(acc_draw.x, acc_draw.y);
    const bool merge = readlane(x0.x & 1u, 0u) != 0u;
    rec.kind = merge ? BISBM_SM_MERGE : BISBM_SM_SPLIT;

    // 2. the choice, in the chain's own numbering; hl / al: home and away in the launch's (a type-b label sits one higher there)
    bool tb = false;
    uint32_t r_loc = 0, s_loc = 0;
    if (!merge) {
        const uint32_t b = readlane((uint32_t)(((uint64_t)x0.y * K) >> 32), 0u);
        tb = b >= ka;
        r_loc = tb ? b - ka : b;
        s_loc = tb ? kb : ka;  // (the spare: the label away takes)
        rec.type = tb ? 1u : 0u, rec.r = b, rec.s = tb ? K : ka;
        if ((tb ? kb : ka) >= p.k_max[tb ? 1 : 0]) rec.refused = BISBM_SM_AT_K_MAX;
    } else if (n_pairs == 0) {
        rec.refused = BISBM_SM_NO_PAIR;
    } else {
        uint32_t pi = readlane((uint32_t)(((uint64_t)x0.y * n_pairs) >> 32), 0u);
        tb = pi >= pairs_a;
        if (tb) pi -= pairs_a;
        const uint32_t k_own = tb ? kb : ka;
        while (pi >= k_own - 1u - r_loc) {
            pi -= k_own - 1u - r_loc;
            ++r_loc;
        }
        s_loc = r_loc + 1u + pi;
        rec.type = tb ? 1u : 0u, rec.r = (tb ? ka : 0u) + r_loc, rec.s = (tb ? ka : 0u) + s_loc;
        if (k_own <= p.k_min[tb ? 1 : 0]) rec.refused = BISBM_SM_AT_K_MIN;
    }
    const TypeView ty = type_view(p, tb);
    const uint32_t n_cls = ty.n_cls, v0 = ty.v0, own0 = ty.own0;
    const uint32_t rg = own0 + r_loc, sg = own0 + s_loc;
    if (rec.refused == BISBM_SM_EVALUATED && !merge) {
        const uint32_t size = (uint32_t)readlane(nr[rg], 0u);
        if (size < 2u) rec.refused = BISBM_SM_SINGLETON, rec.M = size;
    }
    if (rec.refused != BISBM_SM_EVALUATED) {
        if (lane == 0) p.record[chain] = rec;
        return;
    }

    // 3. the members, ascending id, by ballot compaction; home is the block of the lowest one
    uint32_t M = 0, hl = rg;
    for (uint32_t i0 = 0; i0 < n_cls; i0 += kWave) {
        const uint32_t i = i0 + lane;
        const uint32_t lab = i < n_cls ? (uint32_t)labels[v0 + i] : 0xffffffffu;
        const bool is = lab == rg || (merge && lab == sg);
        const unsigned long long bal = __ballot(is);
        if (M == 0 && bal != 0) hl = readlane(lab, (uint32_t)__ffsll((long long)bal) - 1u);
        if (is) {
            const uint32_t pos = M + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            member[pos] = v0 + i;
            orig[pos] = (uint8_t)lab;
        }
        M += (uint32_t)__popcll(bal);
    }
    const uint32_t al = hl == rg ? sg : rg;
    rec.M = M;
    // 5. a merge's dS, at the present division, before anything moves
    double mdS = 0.;
    if (merge) mdS = merge_dS_blocks(wc, tab, ty, tb, hl, al) + p.shape_down[tb ? 1 : 0];
    // 4. the launch labels
    const uint32_t W = (M + 127u) >> 7;
    bool got_a = false;
    for (uint32_t i0 = 0; i0 < M; i0 += kWave) {
        const uint32_t i = i0 + lane;
        uint32_t bit = 0;
        if (i < M) {
            const U4 x = phx_draw(p.seed, chain_gid, PHX_SPLIT_MERGE, idx0 | (uint64_t)(2u + (i >> 7)));
            const uint32_t sel = (i >> 5) & 3u;
            const uint32_t word = sel == 0 ? x.x : sel == 1 ? x.y : sel == 2 ? x.z : x.w;
            bit = i == 0 ? 0u : (word >> (i & 31u)) & 1u;
            launch[i] = (uint8_t)(bit ? al : hl);
        }
        got_a = got_a || __ballot(i < M && bit != 0) != 0;
    }
    __threadfence_block();
    wave_fence();
    if (lane == 0 && !got_a) launch[M - 1u] = (uint8_t)al;
    __threadfence_block();  // the scratch this wave wrote is read by other lanes of it in the headers below
    wave_fence();

    // the passes: stage 0 transit to the launch labels; 1 .. scans the launch scans; scans + 1 the forward pass (split) or the
    // forced pass to the present division (merge); scans + 2 the decision and the transit it asks for
    double q_m = 0.5;
    int q_e = 1;
    bool dead = false, accepted = false;
    const uint64_t n_stages = (uint64_t)p.scans + 3u;
    for (uint64_t stage = 0; stage < n_stages; ++stage) {
        uint32_t kind = SM_TRANSIT;
        const uint8_t* tgt = launch;
        uint64_t draw0 = 0;  // k of member 0's slot in a free scan
        if (stage >= 1 && stage <= p.scans) {
            kind = SM_FREE;
            draw0 = 2u + (uint64_t)W + (stage - 1u) * (uint64_t)M;
        } else if (stage == (uint64_t)p.scans + 1u) {
            q_m = 0.5, q_e = 1;
            if (merge) {
                kind = SM_FORCED, tgt = orig;
            } else {
                kind = SM_FREE;
                draw0 = 2u + (uint64_t)W + (uint64_t)p.scans * (uint64_t)M;
            }
        } else if (stage == (uint64_t)p.scans + 2u) {
            // 6. - 8. accept
            rec.q_mant = q_m, rec.q_exp = q_e;
            const double ln_q = log(q_m) + (double)q_e * 0.6931471805599453;
            if (merge) {
                rec.dS = mdS;
                if (!dead) rec.lnA = ((0. - beta * rec.dS) + (log((double)n_pairs) - log((double)(K - 1u)))) + ln_q;
            } else {
                mdS = merge_dS_blocks(wc, tab, ty, tb, hl, al) + (0. - p.shape_up[tb ? 1 : 0]);
                rec.dS = 0. - mdS;
                const uint32_t ka2 = ka + (tb ? 0u : 1u), kb2 = kb + (tb ? 1u : 0u);
                const uint32_t pairs_after = ka2 * (ka2 - 1u) / 2u + kb2 * (kb2 - 1u) / 2u;
                rec.lnA = ((0. - beta * rec.dS) + (log((double)K) - log((double)pairs_after))) - ln_q;
            }
            rec.A = dead ? 0. : exp(rec.lnA);
            accepted = !dead && rec.u_acc < rec.A;
            if (accepted && !merge) break;   // (the proposal stays)
            if (!accepted && merge && !dead) break;  // (the forced pass has ended at the present division)
            if (accepted) {  // a merge: everything into r
                for (uint32_t i = lane; i < M; i += kWave) launch[i] = (uint8_t)rg;
                __threadfence_block();
                wave_fence();
            } else {
                tgt = orig;
            }
        }

        for (uint32_t i0 = 0; i0 < M; i0 += kWave) {
            // ---- chunk header: lane q holds the node, row extent, current label and target of member i0 + q ----
            const uint32_t cnt = M - i0 < (uint32_t)kWave ? M - i0 : (uint32_t)kWave;
            uint32_t v_l = 0, beg_l = 0, deg_l = 0, c_l = 0, want_l = 0;
            if (lane < cnt) {
                v_l = member[i0 + lane];
                beg_l = p.rowptr[v_l];
                deg_l = p.rowptr[v_l + 1] - beg_l;
                c_l = labels[v_l];
                want_l = tgt[i0 + lane];
            }
            wc.park_rows(cnt, beg_l, deg_l);

            for (uint32_t q = 0; q < cnt; ++q) {
                const uint32_t v = readlane(v_l, q), beg = readlane(beg_l, q), deg = readlane(deg_l, q);
                const uint32_t c = readlane(c_l, q), want = readlane(want_l, q);
                if (c != hl && c != al) continue;  // (a member's label: never)
                const bool evaluate = kind != SM_TRANSIT && !dead;
                if (evaluate && i0 + q == 0u) continue;  // (member 0 is pinned)
                const uint32_t o = c == hl ? al : hl, c_loc = c - own0, o_loc = o - own0;
                const int n0c = readlane(nr[c], 0u);
                uint32_t to = c;       // where the member goes
                bool tables = false;   // whether dS_o is evaluated
                if (!evaluate) {
                    to = want;
                } else if (n0c <= 1) {  // not free: the member stays with the factor 1.0, or a forced move kills the pass
                    if (kind == SM_FORCED && want != c) {
                        dead = true, q_m = 0., q_e = 0;
                        to = want;
                    }
                } else {
                    tables = true;
                }
                if (!tables && to == c) continue;
                const uint32_t nnz = wc.neighbour_list(q, beg, deg, ty, [](uint32_t, uint32_t, int) {});
                if (tables) {
                    // dS_o (step 1 of "Node conditionals" with r = c, s = o), as reshuffle_kernel evaluates it
                    const int ideg = (int)deg;
                    const int m0c = mr[c], m0o = mr[o], n0o = nr[o];
                    const long long eta_c = *wc.eta_at(c * D + deg), eta_o = *wc.eta_at(o * D + deg);
                    const double lg_c1 = lgamma_fast(tab, (long long)m0c - ideg + 1), lg_c0 = lgamma_fast(tab, (long long)m0c + 1);
                    const double lg_o1 = lgamma_fast(tab, (long long)m0o + ideg + 1), lg_o0 = lgamma_fast(tab, (long long)m0o + 1);
                    const double lg_ec1 = lgamma_fast(tab, eta_c + 1), lg_ec0 = lgamma_fast(tab, eta_c);
                    const double lg_eo1 = lgamma_fast(tab, eta_o + 1), lg_eo2 = lgamma_fast(tab, eta_o + 2);
                    const uint32_t sel = lane & 3u;
                    const int qn = sel == 0 ? m0c - ideg : sel == 1 ? m0c : sel == 2 ? m0o + ideg : m0o;
                    const int qk = sel == 0 ? n0c - 1 : sel == 1 ? n0c : sel == 2 ? n0o + 1 : n0o;
                    const double ln_qn = log_n_of(tab, qn);
                    double acc = 0.;
                    for (uint32_t l0 = 0; l0 < nnz; l0 += kWave) {
                        const uint32_t cn = nnz - l0 < (uint32_t)kWave ? nnz - l0 : (uint32_t)kWave;
                        const uint32_t li = l0 + (lane < cn ? lane : cn - 1u);  // (idle lanes read the last entry again)
                        const uint32_t t = wc.s_t[li];
                        const int kt = wc.s_kt[li];
                        const int32_t m_ct = wc.M(tb, c_loc, t), m_ot = wc.M(tb, o_loc, t);
                        const double a1 = lgamma_fast(tab, (long long)m_ct + 1), a2 = lgamma_fast(tab, (long long)m_ot + 1);
                        const double a3 = lgamma_fast(tab, (long long)m_ct - kt + 1), a4 = lgamma_fast(tab, (long long)m_ot + kt + 1);
                        const double term = (a1 + a2) - (a3 + a4);
                        for (uint32_t j = 0; j < cn; ++j) acc = acc + readlane(term, j);
                    }
                    const double lq = log_q<true>(tab, qn, qk, ln_qn);
                    const double tail1 = (lg_c1 - lg_c0) + (lg_o1 - lg_o0);
                    const double tail2 = (lg_ec1 - lg_ec0) + (lg_eo1 - lg_eo2);
                    const double tail3 = (readlane(lq, 0u) - readlane(lq, 1u)) + (readlane(lq, 2u) - readlane(lq, 3u));
                    const double dS_o = ((acc + tail1) + tail2) + tail3;
                    // the two weights, Z = w_home + w_away, the choice and its factor
                    const double mn = dS_o < 0. ? dS_o : 0.;
                    const double x_c = beta * (0. - mn), x_o = beta * (dS_o - mn);
                    const double w_c = x_c > 700. ? 0. : exp(-x_c), w_o = x_o > 700. ? 0. : exp(-x_o);
                    const double w_h = c == hl ? w_c : w_o, w_a = c == hl ? w_o : w_c;
                    const double Z = w_h + w_a;
                    const double P_h = w_h / Z, P_a = w_a / Z;
                    if (kind == SM_FREE) {
                        const U4 x = phx_draw(p.seed, chain_gid, PHX_SPLIT_MERGE, idx0 | (draw0 + i0 + q));
                        to = u53(x.x, x.y) < P_h ? hl : al;
                    } else {
                        to = want;
                    }
                    const double f = to == hl ? P_h : P_a;
                    int e2;
                    q_m = frexp(q_m * f, &e2);
                    q_e += e2;
                    if (readlane((uint32_t)(f == 0.), 0u) != 0u) dead = true, q_m = 0., q_e = 0;  // (a forced pass only)
                    to = readlane(to, 0u);  // (the same in every lane; this tells the compiler)
                    if (to == c) continue;
                }
                wc.apply_move(v, deg, c, o, c_loc, o_loc, tb, nnz);
            }
        }
        __threadfence_block();  // the labels this pass wrote are read by the next pass's headers
    }
    rec.accepted = accepted ? 1u : 0u;
    if (accepted) {
        if (merge)
            rec.ka_after = ka - (tb ? 0u : 1u), rec.kb_after = kb - (tb ? 1u : 0u);
        else
            rec.ka_after = ka + (tb ? 0u : 1u), rec.kb_after = kb + (tb ? 1u : 0u);
    }
    if (lane == 0) p.record[chain] = rec;  // (an accepted dS goes onto the running sum when the chain is moved to its group)
}

double shape_term(const bisbm_engine* e, uint32_t ka, uint32_t kb) {
    const HostTables& tab = *e->tab;
    return (h_lbinom_fast(tab, (uint64_t)ka * kb + e->num_edges - 1, e->num_edges) + h_lbinom_fast(tab, e->na - 1, ka - 1)) +
           h_lbinom_fast(tab, e->nb - 1, kb - 1);
}

// where group g's slice of the entry's scratch starts, in chains and in cells of every array
struct Slice {
    size_t chain0 = 0, m0 = 0, k0 = 0, eta0 = 0;
};

// the groups of a device entry as they run a launch: the entry itself while it is a plain engine
std::vector<bisbm_engine*> groups_of(bisbm_engine* d) { return d->groups.empty() ? std::vector<bisbm_engine*>{d} : d->groups; }
uint32_t entry_chain(const bisbm_engine* g, size_t c) { return g->ridx.empty() ? (uint32_t)c : g->ridx[c]; }

// One move of every chain of device entry d; *any_accepted: whether the groups must be formed again.
int launch_move(bisbm_engine* d, const std::vector<Slice>& slices, uint32_t scans, double beta, const uint32_t k_min[2], const uint32_t k_max[2],
                bool* any_accepted) {
    SplitMergeState& st = d->split_merge;
    const std::vector<bisbm_engine*> gs = groups_of(d);
    const size_t nmax = (size_t)std::max(d->na, d->nb), stride = d->label_stride, D = (size_t)d->maxdeg + 1;
    std::vector<uint32_t> prop(d->n_chains);
    for (size_t gi = 0; gi < gs.size(); ++gi)
        for (size_t c = 0; c < gs[gi]->n_chains; ++c) prop[slices[gi].chain0 + c] = st.proposed[entry_chain(gs[gi], c)];
    for (bisbm_engine* g : gs) {  // (before anything is launched)
        const size_t lds = wave_chain_lds_bytes(g->ka + 1u, g->kb + 1u, g->maxdeg, false);
        if (lds > kLdsPerCu) return fail(d, BISBM_ERR_UNSUPPORTED, "chain state needs %zu B of LDS (> 160 KiB)", lds);
    }
    HIPCHK(d, hipMemcpy(st.d_proposed.get(), prop.data(), sizeof(uint32_t) * prop.size(), hipMemcpyHostToDevice));
    for (size_t gi = 0; gi < gs.size(); ++gi) {
        bisbm_engine* g = gs[gi];
        const Slice& sl = slices[gi];
        PadParams q{};
        q.labels = g->d_labels, q.m = g->d_m, q.m_r = g->d_m_r, q.n_r = g->d_n_r, q.eta = g->d_eta;
        q.labels_p = st.d_labels.get() + sl.chain0 * stride;
        q.m_p = st.d_m.get() + sl.m0, q.m_r_p = st.d_m_r.get() + sl.k0, q.n_r_p = st.d_n_r.get() + sl.k0, q.eta_p = st.d_eta.get() + sl.eta0;
        q.label_stride = stride, q.n = (uint32_t)g->n, q.ka = g->ka, q.kb = g->kb, q.D = (uint32_t)D;
        hipLaunchKernelGGL(sm_pad_kernel, dim3(g->n_chains), dim3(256), 0, g->stream, q);
        HIPCHK(d, hipGetLastError());
        SplitMergeParams p{};
        wave_chain_fill(g, beta, false, p);
        p.ka = g->ka + 1u, p.kb = g->kb + 1u;
        p.labels = q.labels_p, p.m = q.m_p, p.m_r = q.m_r_p, p.n_r = q.n_r_p, p.eta = q.eta_p;
        p.rounds = 1, p.scans = scans;
        for (int t = 0; t < 2; ++t) p.k_min[t] = k_min[t], p.k_max[t] = k_max[t];
        p.proposed = st.d_proposed.get() + sl.chain0;
        const double T0 = shape_term(g, g->ka, g->kb);
        p.shape_up[0] = shape_term(g, g->ka + 1, g->kb) - T0, p.shape_up[1] = shape_term(g, g->ka, g->kb + 1) - T0;
        p.shape_down[0] = g->ka > 1 ? shape_term(g, g->ka - 1, g->kb) - T0 : 0.;
        p.shape_down[1] = g->kb > 1 ? shape_term(g, g->ka, g->kb - 1) - T0 : 0.;
        p.member = (uint32_t*)st.d_scratch.get() + sl.chain0 * nmax;
        p.orig = st.d_scratch.get() + 4 * nmax * d->n_chains + sl.chain0 * nmax;
        p.launch = st.d_scratch.get() + 5 * nmax * d->n_chains + sl.chain0 * nmax;
        p.record = st.d_record.get() + sl.chain0;
        p.eta_in_lds = wave_chain_lds_bytes(p.ka, p.kb, p.maxdeg, true) <= 40 * 1024 ? 1 : 0;
        const size_t lds = wave_chain_lds_bytes(p.ka, p.kb, p.maxdeg, p.eta_in_lds != 0);
        HIPCHK(d, launch_wave_chain(split_merge_kernel<true>, split_merge_kernel<false>, p, lds, g->stream));
    }
    for (bisbm_engine* g : gs) HIPCHK(d, hipStreamSynchronize(g->stream));
    std::vector<bisbm_split_merge_record> rec(d->n_chains);
    HIPCHK(d, hipMemcpy(rec.data(), st.d_record.get(), sizeof(bisbm_split_merge_record) * rec.size(), hipMemcpyDeviceToHost));
    *any_accepted = false;
    for (size_t gi = 0; gi < gs.size(); ++gi)
        for (size_t c = 0; c < gs[gi]->n_chains; ++c) {
            const uint32_t e = entry_chain(gs[gi], c);
            const bisbm_split_merge_record& r = rec[slices[gi].chain0 + c];
            st.last[e] = r;
            st.proposed[e] += 1u;
            st.totals[4 * (size_t)e + (r.kind == BISBM_SM_MERGE ? 2 : 0)] += 1;
            st.totals[4 * (size_t)e + (r.kind == BISBM_SM_MERGE ? 3 : 1)] += r.accepted;
            *any_accepted = *any_accepted || r.accepted != 0;
        }
    return BISBM_OK;
}

std::vector<Slice> plan_slices(bisbm_engine* d, size_t tot[3]) {
    const std::vector<bisbm_engine*> gs = groups_of(d);
    std::vector<Slice> out(gs.size());
    Slice at;
    const size_t D = (size_t)d->maxdeg + 1;
    for (size_t gi = 0; gi < gs.size(); ++gi) {
        out[gi] = at;
        const size_t C = gs[gi]->n_chains, KP = (size_t)gs[gi]->K + 2;
        at.chain0 += C, at.m0 += C * (gs[gi]->ka + 1) * (gs[gi]->kb + 1), at.k0 += C * KP, at.eta0 += C * KP * D;
    }
    tot[0] = at.m0, tot[1] = at.k0, tot[2] = at.eta0;
    return out;
}

// After a launch in which some chain of entry d was accepted: the chains by the shape they have now.  A group that neither lost
// nor gained a chain stays; every other shape gets a fresh group whose chains come out of the launch's scratch.
int regroup(bisbm_engine* d, const std::vector<Slice>& slices) {
    SplitMergeState& st = d->split_merge;
    const std::vector<bisbm_engine*> olds = groups_of(d);
    const bool plain = d->groups.empty();
    using Shape = std::pair<uint32_t, uint32_t>;
    struct From {
        size_t group, chain;
    };
    std::vector<Shape> shapes;                 // in order of first appearance in the entry's chain order
    std::map<Shape, std::vector<uint32_t>> members;  // entry chains of every shape, ascending
    std::vector<From> from(d->n_chains);
    for (size_t gi = 0; gi < olds.size(); ++gi)
        for (size_t c = 0; c < olds[gi]->n_chains; ++c) from[entry_chain(olds[gi], c)] = From{gi, c};
    for (uint32_t e = 0; e < d->n_chains; ++e) {
        const Shape s{st.last[e].ka_after, st.last[e].kb_after};
        if (!members.count(s)) shapes.push_back(s);
        members[s].push_back(e);
    }
    std::vector<bool> kept(olds.size(), false);
    std::vector<bisbm_engine*> next;
    std::vector<bisbm_engine*> fresh;
    auto drop_fresh = [&]() {
        for (bisbm_engine* f : fresh) {
            free_all(f);
            delete f;
        }
    };
    const size_t stride = d->label_stride;
    for (const Shape& s : shapes) {
        const std::vector<uint32_t>& mem = members[s];
        // an old group of this shape whose chains are exactly these, none of them moved: it stays
        bisbm_engine* same = nullptr;
        size_t same_i = 0;
        for (size_t gi = 0; gi < olds.size() && !plain; ++gi)
            if (olds[gi]->ka == s.first && olds[gi]->kb == s.second && olds[gi]->n_chains == mem.size()) same = olds[gi], same_i = gi;
        if (same) {
            for (size_t c = 0; c < mem.size() && same; ++c)
                if (from[mem[c]].group != same_i || st.last[mem[c]].accepted) same = nullptr;
        }
        if (same) {
            kept[same_i] = true;
            next.push_back(same);
            continue;
        }
        std::string err;
        bisbm_engine* g = new_group(d, s.first, s.second, (uint32_t)mem.size(), err);
        if (!g) {
            drop_fresh();
            return fail(d, BISBM_ERR_HIP, "%s", err.c_str());
        }
        fresh.push_back(g);
        next.push_back(g);
        std::vector<ChainCopy> jobs(mem.size());
        for (size_t j = 0; j < mem.size(); ++j) {
            const uint32_t e = mem[j];
            const From f = from[e];
            const bisbm_engine* o = olds[f.group];
            const bisbm_split_merge_record& r = st.last[e];
            g->gids.push_back(o->gid(f.chain));
            g->ridx.push_back(e);
            ChainCopy& job = jobs[j];
            job.labels = st.d_labels.get() + (slices[f.group].chain0 + f.chain) * stride;
            job.scalars = o->d_scalars + f.chain;
            job.moved = r.accepted, job.pad = 0, job.dS = r.dS;
            // the launch's numbering: the spare of type a is o->ka, a type-b label sits one higher than in the chain's own
            if (!r.accepted)
                job.cut1 = o->ka, job.cut2 = kNoCut;
            else if (r.kind == BISBM_SM_SPLIT)
                job.cut1 = r.type ? o->ka : kNoCut, job.cut2 = kNoCut;  // (type a: the spare has become block ka; type b: the last block)
            else if (r.type == 0)
                job.cut1 = r.s, job.cut2 = o->ka;  // (s is empty now)
            else
                job.cut1 = o->ka, job.cut2 = r.s + 1u;
        }
        hipError_t e = st.d_jobs.reserve(sizeof(ChainCopy) * jobs.size());
        if (e == hipSuccess) e = hipMemcpy(st.d_jobs.get(), jobs.data(), sizeof(ChainCopy) * jobs.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemsetAsync(g->d_labels, 0, (size_t)g->n_chains * stride, g->stream);  // (the padding, as bisbm_create leaves it)
        if (e == hipSuccess) {
            hipLaunchKernelGGL(sm_gather_kernel, dim3(g->n_chains), dim3(256), 0, g->stream, (const ChainCopy*)st.d_jobs.get(), g->d_labels, stride,
                               (uint32_t)g->n, g->d_scalars);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(g->d_gids, g->gids.data(), sizeof(uint32_t) * g->gids.size(), hipMemcpyHostToDevice, g->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g->stream);  // (d_jobs is written again for the next group)
        if (e != hipSuccess) {
            drop_fresh();
            return fail(d, BISBM_ERR_HIP, "moving chains to the group of %u + %u blocks: %s", s.first, s.second, hipGetErrorString(e));
        }
        if (const int rc = rebuild_state(g)) {
            const std::string msg = g->err;
            drop_fresh();
            return fail(d, rc, "%s", msg.c_str());
        }
    }
    if (plain) {
        free_chain_arrays(d);  // the chains live in the groups now
        d->state_ready = true;
    } else {
        for (size_t gi = 0; gi < olds.size(); ++gi)
            if (!kept[gi]) {
                free_all(olds[gi]);
                delete olds[gi];
            }
    }
    d->groups = next;
    remap_groups(d);
    (void)common_shape(d);
    return BISBM_OK;
}

int run_entry(bisbm_engine* d, uint64_t moves, uint32_t scans, double beta, const uint32_t k_min[2], const uint32_t k_max[2]) {
    HIPCHK(d, hipSetDevice(d->device));
    SplitMergeState& st = d->split_merge;
    const size_t C = d->n_chains, nmax = (size_t)std::max(d->na, d->nb);
    if (st.proposed.size() != C) st.proposed.assign(C, 0u), st.totals.assign(4 * C, 0);
    st.last.assign(C, bisbm_split_merge_record{});
    RESERVE(d, st.d_labels, C * d->label_stride);
    RESERVE(d, st.d_scratch, 6 * nmax * C);
    RESERVE(d, st.d_record, C);
    RESERVE(d, st.d_proposed, C);
    size_t tot[3];
    std::vector<Slice> slices = plan_slices(d, tot);
    using Clock = std::chrono::steady_clock;
    const Clock::time_point t_call = Clock::now();
    st.call_ms = st.regroup_ms = 0;
    struct Stamp {  // (on every way out)
        SplitMergeState& st;
        Clock::time_point t0;
        ~Stamp() { st.call_ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
    } stamp{st, t_call};
    for (uint64_t move = 0; move < moves; ++move) {
        RESERVE(d, st.d_m, tot[0]);
        RESERVE(d, st.d_m_r, tot[1]);
        RESERVE(d, st.d_n_r, tot[1]);
        RESERVE(d, st.d_eta, tot[2]);
        bool any = false;
        if (int rc = launch_move(d, slices, scans, beta, k_min, k_max, &any)) return rc;
        if (any) {
            const Clock::time_point t_re = Clock::now();
            const int rc_re = regroup(d, slices);
            st.regroup_ms += std::chrono::duration<double, std::milli>(Clock::now() - t_re).count();
            if (int rc = rc_re) {
                // nothing of the chains has changed (their own arrays and sums are only written when a group is formed): the
                // accepted moves of this launch did not happen -- proposed, as every draw was used, and rejected
                for (size_t c = 0; c < C; ++c)
                    if (st.last[c].accepted) {
                        st.totals[4 * c + (st.last[c].kind == BISBM_SM_MERGE ? 3 : 1)] -= 1;
                        st.last[c].accepted = 0, st.last[c].ka_after = st.last[c].ka_before, st.last[c].kb_after = st.last[c].kb_before;
                    }
                return rc;
            }
            slices = plan_slices(d, tot);
        }
    }
    return BISBM_OK;
}

}  // namespace

}  // namespace bisbm

extern "C" {

int bisbm_split_merge_run(bisbm_handle h, uint64_t moves, uint32_t scans, double beta, const uint32_t* k_min_in, const uint32_t* k_max_in,
                          uint64_t* accepted_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (h->rng_mode == BISBM_RNG_MT19937_COMPAT)
        return fail(h, BISBM_ERR_UNSUPPORTED, "split and merge moves are defined in the Philox-mode arithmetic: this handle runs BISBM_RNG_MT19937_COMPAT");
    if (!(beta > 0.) || std::isinf(beta)) return fail(h, BISBM_ERR_INVALID_ARG, "beta = %g: a finite value above 0 is needed", beta);
    if (h->temper.L)
        return fail(h, BISBM_ERR_STATE, "replica exchange is on: a rung's chains share one shape (bisbm_tempering_set(h, 0, NULL) turns it off)");
    if (!h->population.ancestor.empty() || h->population.rounds)
        return fail(h, BISBM_ERR_STATE, "a population is in progress: its resampling copies chains of one shape (bisbm_population_reset ends it)");
    if (h->constraints.n_classes)  // (a merge or split renumbers blocks: the table's columns would change their meaning)
        return fail(h, BISBM_ERR_STATE, "block constraints are set: a split or merge renumbers blocks, clear them first with bisbm_constraints_set(h, 0, NULL, NULL)");
    if (h->fields.n_classes)
        return fail(h, BISBM_ERR_STATE, "block fields are set: a split or merge renumbers blocks, clear them first with bisbm_fields_set(h, 0, NULL, NULL)");
    if (h->clamp.n_clamped)
        return fail(h, BISBM_ERR_STATE, "%llu node(s) are clamped: a split or merge renumbers blocks, clear the clamp first with bisbm_clamp_set(h, NULL)",
                    (unsigned long long)h->clamp.n_clamped);
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "split and merge moves serve byte labels only (at most 254 blocks): merge the blocks down first");
    const uint32_t k_min[2] = {k_min_in ? k_min_in[0] : 1u, k_min_in ? k_min_in[1] : 1u};
    const uint32_t k_max[2] = {k_max_in ? k_max_in[0] : (uint32_t)std::min<uint64_t>(h->na, 127), k_max_in ? k_max_in[1] : (uint32_t)std::min<uint64_t>(h->nb, 127)};
    for (int t = 0; t < 2; ++t)
        if (k_min[t] < 1 || k_min[t] > k_max[t])
            return fail(h, BISBM_ERR_INVALID_ARG, "type %c: k_min = %u, k_max = %u: 1 <= k_min <= k_max is needed", t ? 'b' : 'a', k_min[t], k_max[t]);
    if ((uint64_t)k_max[0] + k_max[1] > 254)
        return fail(h, BISBM_ERR_INVALID_ARG, "k_max = (%u, %u): a split keeps a spare block per type beside byte labels, k_max[0] + k_max[1] <= 254 is needed", k_max[0], k_max[1]);
    for (bisbm_engine* e : leaves(h)) {
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_split_merge_run");
        if (e->K > 254) return fail(h, BISBM_ERR_UNSUPPORTED, "a chain of this handle has %u + %u blocks: split and merge moves serve at most 254", e->ka, e->kb);
    }
    if (int rc = reshuffle_check_scans(h, scans)) return rc;
    if (moves == 0) {
        for (uint32_t c = 0; accepted_out && c < h->n_chains; ++c) accepted_out[c] = 0;
        return BISBM_OK;
    }
    DeviceGuard keep;
    const std::vector<bisbm_engine*> entries = device_entries(h);
    std::vector<std::vector<uint64_t>> before;
    for (bisbm_engine* d : entries) before.push_back(d->split_merge.totals);
    int rc;
    if (!h->devs.empty()) {
        rc = on_devices(h, [&](bisbm_engine* d, size_t) { return run_entry(d, moves, scans, beta, k_min, k_max); });
        (void)common_shape(h);
    } else {
        rc = run_entry(h, moves, scans, beta, k_min, k_max);
    }
    if (rc) return rc;
    uint32_t c = 0;
    for (size_t i = 0; i < entries.size(); ++i)
        for (uint32_t l = 0; l < entries[i]->n_chains; ++l, ++c) {
            const std::vector<uint64_t>& now = entries[i]->split_merge.totals;
            const uint64_t was = before[i].empty() ? 0 : before[i][4 * (size_t)l + 1] + before[i][4 * (size_t)l + 3];
            if (accepted_out) accepted_out[c] = now[4 * (size_t)l + 1] + now[4 * (size_t)l + 3] - was;
        }
    return BISBM_OK;
}

int bisbm_split_merge_get_last(bisbm_handle h, bisbm_split_merge_record* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!out) return fail(h, BISBM_ERR_INVALID_ARG, "out is NULL");
    for (bisbm_engine* d : device_entries(h))
        if (d->split_merge.last.size() != d->n_chains)
            return fail(h, BISBM_ERR_STATE, "no split or merge move on record: call bisbm_split_merge_run first");
    for (bisbm_engine* d : device_entries(h)) {
        std::copy(d->split_merge.last.begin(), d->split_merge.last.end(), out);
        out += d->n_chains;
    }
    return BISBM_OK;
}

int bisbm_split_merge_get_total(bisbm_handle h, uint64_t* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!out) return fail(h, BISBM_ERR_INVALID_ARG, "out is NULL");
    for (bisbm_engine* d : device_entries(h)) {
        if (d->split_merge.totals.size() == 4 * (size_t)d->n_chains)
            std::copy(d->split_merge.totals.begin(), d->split_merge.totals.end(), out);
        else
            std::fill(out, out + 4 * (size_t)d->n_chains, (uint64_t)0);
        out += 4 * (size_t)d->n_chains;
    }
    return BISBM_OK;
}

int bisbm_split_merge_get_groups(bisbm_handle h, uint32_t* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!out) return fail(h, BISBM_ERR_INVALID_ARG, "out is NULL");
    for (bisbm_engine* d : device_entries(h))
        for (uint32_t c = 0; c < d->n_chains; ++c) *out++ = d->groups.empty() ? 0u : d->where[c].first;
    return BISBM_OK;
}

int bisbm_split_merge_get_timing(bisbm_handle h, double* call_ms, double* regroup_ms) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    double c = 0, r = 0;
    for (bisbm_engine* d : device_entries(h))  // (the entries run side by side: the slowest one)
        if (d->split_merge.call_ms >= c) c = d->split_merge.call_ms, r = d->split_merge.regroup_ms;
    if (call_ms) *call_ms = c;
    if (regroup_ms) *regroup_ms = r;
    return BISBM_OK;
}

int bisbm_split_merge_shape_term(bisbm_handle h, uint32_t ka, uint32_t kb, double* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!out || ka < 1 || kb < 1) return fail(h, BISBM_ERR_INVALID_ARG, "ka, kb >= 1 and a non-NULL out are needed");
    *out = shape_term(leaves(h)[0], ka, kb);
    return BISBM_OK;
}

}  // extern "C"
