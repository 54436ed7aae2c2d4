// bisbm_reshuffle.hip -- pair reshuffles: the nodes of two blocks of one type divided afresh between the two in one accepted or
// rejected move (no reference counterpart; include/bisbm.h, "Pair reshuffles", states every draw, every order of operations and
// what a move updates).  The dS of a member's one other block is entry o of the row of "Node conditionals": the same f64
// operations in the same order as cond_rows_kernel of bisbm_conditionals.hip and heatbath_kernel of bisbm_heatbath.hip, restated
// here because this kernel evaluates ONE target per step.
//
// Kernel: one wave per chain, persistent over all moves of the call.  The chain state in LDS, its load and store-back, the
// chunk header's parked neighbour labels, the list of the non-zero (t, k_t) and the move are the WaveChain of
// bisbm_wave_chain.hpp, shared with heatbath_kernel; this file holds the pair, the passes and the one-target dS.  A move
// collects its members from the type's label row by ballot compaction into the
// chain's scratch (member id, original label, launch label), then runs its passes -- transit to the launch labels, the launch
// scans, the reverse pass, transit to L, the forward pass, transit back after a rejection -- through ONE copy of the pass loop,
// told apart by `kind`.  The members are one type, hence an independent set and their neighbours' labels never change during a
// move, which is what the shared chunk header asks for (lane q takes the node, row extent and label of member q).
//
// Step: a step has one non-trivial target, so the lanes are mapped to the non-zero (t, k_t) of the list instead of to targets:
// lane i reads m_ct and m_ot and issues its four table gathers, 64 list entries in flight together, then the terms are added
// in ascending t one v_readlane at a time, as the definition demands.  The four log_q evaluations of tail3 run side by side in
// lanes 0 .. 3 through one copy of log_q's code; the eight lgamma values of tail1 and tail2 are issued before the list is
// walked.  A transit step builds the list and applies the move, and reads no table.
#include "bisbm_engine.hpp"
#include "bisbm_wave_chain.hpp"

using namespace bisbm;

namespace bisbm {

namespace {

enum : uint32_t { RS_TRANSIT = 0, RS_FREE = 1, RS_FORCED = 2 };

// CN: the launch has block constraints (p.cn_bits is not NULL).  Without them the instance holds no look-up and is the code a
// handle ran before they existed.
// FL: the launch has block fields (p.fl_field is not NULL): the one instance per EL that adds the field to a member's dS_o.  It is
// compiled with CN and serves constraints beside the field by testing p.cn_bits at run time.
template <bool EL, bool CN, bool FL = false>
__global__ __launch_bounds__(kWave) void reshuffle_kernel(ReshuffleParams p) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const uint32_t chain = blockIdx.x;
    if (chain >= p.n_chains) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t nmax = p.na > p.nb ? p.na : p.nb;

    WaveChain<EL> wc;
    wc.load(lds_raw, p, chain);
    int32_t *const mr = wc.mr, *const nr = wc.nr;  // (the names the dS code below reads the state by)
    const uint32_t D = wc.D;
    uint8_t* const labels = wc.labels;
    uint32_t* member = p.member + (size_t)chain * nmax;
    uint8_t* orig = p.orig + (size_t)chain * nmax;
    uint8_t* launch = p.launch + (size_t)chain * nmax;
    ChainScalars* sc = p.scalars + chain;
    double cum_dS = sc->cum_dS;
    uint32_t total = sc->reshuffles_total;
    __syncthreads();

    const Tables tab{p.lgamma_tab, p.lgamma_size, p.q_tab, p.q_stride, p.log_tab};
    const uint32_t chain_gid = chain_gid_of(p, chain);
    const double beta = chain_beta_of(p, chain);  // (the launch's, or under replica exchange the chain's own)
    const uint32_t pairs_a = p.ka * (p.ka - 1u) / 2u, n_pairs = pairs_a + p.kb * (p.kb - 1u) / 2u;
    unsigned long long n_accepted = 0;
    bisbm_reshuffle_record rec{};
    rec.type = BISBM_RESHUFFLE_NONE;

    for (uint64_t move = 0; move < p.rounds; ++move, ++total) {
        const uint64_t idx0 = (uint64_t)total << 32;
        rec = bisbm_reshuffle_record{};
        rec.type = BISBM_RESHUFFLE_NONE;
        if (n_pairs == 0) continue;  // (a counted no-op)
        // 2. the pair
        uint32_t pi = readlane((uint32_t)(((uint64_t)phx_draw(p.seed, chain_gid, PHX_RESHUFFLE, idx0).x * n_pairs) >> 32), 0u);
        const bool tb = pi >= pairs_a;
        if (tb) pi -= pairs_a;
        const TypeView ty = type_view(p, tb);
        const uint32_t n_cls = ty.n_cls, v0 = ty.v0, k_own = ty.k_own, own0 = ty.own0;
        uint32_t r_loc = 0;
        while (pi >= k_own - 1u - r_loc) {
            pi -= k_own - 1u - r_loc;
            ++r_loc;
        }
        const uint32_t s_loc = r_loc + 1u + pi;
        const uint32_t rg = own0 + r_loc, sg = own0 + s_loc;  // global labels
        const U4 acc_draw = phx_draw(p.seed, chain_gid, PHX_RESHUFFLE, idx0 | 1u);
        const double u_acc = u53(acc_draw.x, acc_draw.y);

        // 3. the members, ascending id, by ballot compaction: the nodes of r and s that are not clamped and, under block
        //    constraints, may sit in both
        uint32_t M = 0;
        for (uint32_t i0 = 0; i0 < n_cls; i0 += kWave) {
            const uint32_t i = i0 + lane;
            const uint32_t lab = i < n_cls ? (uint32_t)labels[v0 + i] : 0xffffffffu;
            bool is = (lab == rg || lab == sg) && !(p.clamp && p.clamp[v0 + i] != 0);
            if (CN && (!FL || p.cn_bits) && is) {  // (block constraints: a member's class allows both blocks of the pair)
                const uint32_t cls = p.cn_class[v0 + i];
                is = cn_allows(p.cn_bits, cls, rg) && cn_allows(p.cn_bits, cls, sg);
            }
            const unsigned long long bal = __ballot(is);
            if (is) {
                const uint32_t pos = M + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                member[pos] = v0 + i;
                orig[pos] = (uint8_t)lab;
            }
            M += (uint32_t)__popcll(bal);
        }
        if (M < 2u) {  // (no block is ever empty: only under a clamp or block constraints) a counted no-op; the record keeps the pair and M
            rec.type = tb ? 1u : 0u, rec.r = rg, rec.s = sg, rec.M = M;
            continue;
        }
        // 4. the launch labels
        const uint32_t W = (M + 127u) >> 7;
        bool got_r = false, got_s = false;
        for (uint32_t i0 = 0; i0 < M; i0 += kWave) {
            const uint32_t i = i0 + lane;
            uint32_t bit = 0;
            if (i < M) {
                const U4 x = phx_draw(p.seed, chain_gid, PHX_RESHUFFLE, idx0 | (uint64_t)(2u + (i >> 7)));
                const uint32_t sel = (i >> 5) & 3u;
                const uint32_t word = sel == 0 ? x.x : sel == 1 ? x.y : sel == 2 ? x.z : x.w;
                bit = (word >> (i & 31u)) & 1u;
                launch[i] = (uint8_t)(bit ? sg : rg);
            }
            got_s = got_s || __ballot(i < M && bit != 0) != 0;
            got_r = got_r || __ballot(i < M && bit == 0) != 0;
        }
        __threadfence_block();
        wave_fence();
        if (lane == 0) {
            if (!got_r) launch[0] = (uint8_t)rg;
            if (!got_s) launch[M - 1u] = (uint8_t)sg;
        }
        __threadfence_block();  // the scratch this wave wrote is read by other lanes of it in the headers below
        wave_fence();

        // the passes: stage 0 transit to the launch labels; 1 .. scans the launch scans; scans + 1 the reverse pass; scans + 2
        // transit to L; scans + 3 the forward pass; scans + 4 transit back to the original labels after a rejection
        double q_m = 0.5, dsum = 0.;  // the running Q (mantissa, exponent) and sum of dS of the pass under way
        int q_e = 1;
        bool dead = false, accepted = false;
        const uint64_t n_stages = (uint64_t)p.scans + 5u;
        for (uint64_t stage = 0; stage < n_stages; ++stage) {
            uint32_t kind = RS_TRANSIT;
            const uint8_t* tgt = launch;
            uint64_t draw0 = 0;  // k of member 0's uniform in a free scan
            if (stage >= 1 && stage <= p.scans) {
                kind = RS_FREE;
                draw0 = 2u + (uint64_t)W + (stage - 1u) * (uint64_t)M;
            } else if (stage == (uint64_t)p.scans + 1u) {
                // L = the labels the launch scans ended at
                for (uint32_t i = lane; i < M; i += kWave) launch[i] = labels[member[i]];
                __threadfence_block();
                wave_fence();
                kind = RS_FORCED, tgt = orig;
                q_m = 0.5, q_e = 1, dsum = 0.;
            } else if (stage == (uint64_t)p.scans + 2u) {
                rec.q_rev_mant = q_m, rec.q_rev_exp = q_e, rec.dS_rev = dsum;
                if (dead) break;  // (the reverse pass has ended at the original state: a certain rejection)
            } else if (stage == (uint64_t)p.scans + 3u) {
                kind = RS_FREE;
                draw0 = 2u + (uint64_t)W + (uint64_t)p.scans * (uint64_t)M;
                q_m = 0.5, q_e = 1, dsum = 0.;
            } else if (stage == (uint64_t)p.scans + 4u) {
                // 8. accept
                rec.q_fwd_mant = q_m, rec.q_fwd_exp = q_e, rec.dS_fwd = dsum;
                const double dS = rec.dS_fwd - rec.dS_rev;
                const double lnA = (0. - beta * dS) + (log(rec.q_rev_mant / rec.q_fwd_mant) + (double)(rec.q_rev_exp - rec.q_fwd_exp) * 0.6931471805599453);
                rec.A = exp(lnA);
                accepted = u_acc < rec.A;
                if (accepted) {
                    cum_dS = cum_dS + dS;
                    break;
                }
                tgt = orig;
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
                    if (c != rg && c != sg) continue;  // (a member's label: never)
                    const uint32_t o = c == rg ? sg : rg, c_loc = c - own0, o_loc = o - own0;
                    const bool evaluate = kind != RS_TRANSIT && !dead;
                    const int n0c = readlane(nr[c], 0u);
                    uint32_t to = c;       // where the member goes
                    bool tables = false;   // whether dS_o is evaluated
                    if (!evaluate) {
                        to = want;
                    } else if (n0c <= 1) {  // not free: the member stays with the factor 1.0, or a forced move kills the pass
                        if (kind == RS_FORCED && want != c) {
                            dead = true, q_m = 0., q_e = 0;
                            to = want;
                        }
                    } else {
                        tables = true;
                    }
                    if (!tables && to == c) continue;
                    const uint32_t nnz = wc.neighbour_list(q, beg, deg, ty, [](uint32_t, uint32_t, int) {});
                    double dS_o = 0.;
                    if (tables) {
                        // dS_o (step 1 of "Node conditionals" with r = c, s = o)
                        const int ideg = (int)deg;
                        const int m0c = mr[c], m0o = mr[o], n0o = nr[o];
                        const long long eta_c = *wc.eta_at(c * D + deg), eta_o = *wc.eta_at(o * D + deg);
                        // every table gather of the tails is issued before the list is walked
                        const double lg_c1 = lgamma_fast(tab, (long long)m0c - ideg + 1), lg_c0 = lgamma_fast(tab, (long long)m0c + 1);
                        const double lg_o1 = lgamma_fast(tab, (long long)m0o + ideg + 1), lg_o0 = lgamma_fast(tab, (long long)m0o + 1);
                        const double lg_ec1 = lgamma_fast(tab, eta_c + 1), lg_ec0 = lgamma_fast(tab, eta_c);
                        const double lg_eo1 = lgamma_fast(tab, eta_o + 1), lg_eo2 = lgamma_fast(tab, eta_o + 2);
                        // lanes 0 .. 3: the four log_q of tail3 in the order they are subtracted
                        const uint32_t sel = lane & 3u;
                        const int qn = sel == 0 ? m0c - ideg : sel == 1 ? m0c : sel == 2 ? m0o + ideg : m0o;
                        const int qk = sel == 0 ? n0c - 1 : sel == 1 ? n0c : sel == 2 ? n0o + 1 : n0o;
                        const double ln_q = log_n_of(tab, qn);
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
                        const double lq = log_q<true>(tab, qn, qk, ln_q);
                        const double tail1 = (lg_c1 - lg_c0) + (lg_o1 - lg_o0);
                        const double tail2 = (lg_ec1 - lg_ec0) + (lg_eo1 - lg_eo2);
                        const double tail3 = (readlane(lq, 0u) - readlane(lq, 1u)) + (readlane(lq, 2u) - readlane(lq, 3u));
                        dS_o = ((acc + tail1) + tail2) + tail3;
                        if (FL) {  // (block fields: the move under E = S + Phi; v, c and o are wave-uniform)
                            const double* f = p.fl_field + (size_t)p.fl_class[v] * (p.ka + p.kb);
                            dS_o = dS_o + (f[o] - f[c]);
                        }
                        // the two weights, Z = w_r + w_s, the choice and its factor
                        const double mn = dS_o < 0. ? dS_o : 0.;
                        const double x_c = beta * (0. - mn), x_o = beta * (dS_o - mn);
                        const double w_c = x_c > 700. ? 0. : exp(-x_c), w_o = x_o > 700. ? 0. : exp(-x_o);
                        const double w_r = c == rg ? w_c : w_o, w_s = c == rg ? w_o : w_c;
                        const double Z = w_r + w_s;
                        const double P_r = w_r / Z, P_s = w_s / Z;
                        if (kind == RS_FREE) {
                            const U4 x = phx_draw(p.seed, chain_gid, PHX_RESHUFFLE, idx0 | (draw0 + i0 + q));
                            to = u53(x.x, x.y) < P_r ? rg : sg;
                        } else {
                            to = want;
                        }
                        const double f = to == rg ? P_r : P_s;
                        int e2;
                        q_m = frexp(q_m * f, &e2);
                        q_e += e2;
                        if (readlane((uint32_t)(f == 0.), 0u) != 0u) {  // (a forced pass only) a certain rejection: nothing more is evaluated or added
                            dead = true, q_m = 0., q_e = 0;
                        } else if (to != c) {
                            dsum = dsum + dS_o;
                        }
                        to = readlane(to, 0u);  // (the same in every lane; this tells the compiler)
                        if (to == c) continue;
                    }
                    wc.apply_move(v, deg, c, o, c_loc, o_loc, tb, nnz);
                }
            }
            __threadfence_block();  // the labels this pass wrote are read by the next pass's headers
        }
        rec.type = tb ? 1u : 0u, rec.r = rg, rec.s = sg, rec.M = M;
        rec.u_acc = u_acc;
        rec.accepted = accepted ? 1u : 0u;
        if (dead) rec.dS_fwd = 0., rec.q_fwd_mant = 0., rec.q_fwd_exp = 0, rec.A = 0.;
        n_accepted += accepted ? 1u : 0u;
    }

    wc.store();
    if (lane == 0) {
        sc->cum_dS = cum_dS;
        sc->reshuffles_total = total;
        p.record[chain] = rec;
        p.accepted[chain] = n_accepted;
    }
}

__global__ void exp_probe_kernel(const double* x, size_t count, double* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = exp(x[i]);
}

}  // namespace

hipError_t launch_exp_probe(const double* x, size_t count, double* out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(exp_probe_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, x, count, out);
    return hipGetLastError();
}

}  // namespace bisbm

int bisbm::reshuffle_engine(bisbm_engine* h, uint64_t moves, uint32_t scans, double beta, bool per_rung, bool read_back) {
    HIPCHK(h, hipSetDevice(h->device));
    ReshuffleState& st = h->reshuffle;
    const size_t nmax = (size_t)std::max(h->na, h->nb), C = h->n_chains;
    RESERVE(h, st.d_scratch, 6 * nmax * C);
    RESERVE(h, st.d_record, C);
    RESERVE(h, st.d_accepted, C);
    ReshuffleParams p{};
    wave_chain_fill(h, beta, per_rung, p);
    p.rounds = moves, p.scans = scans;
    p.member = (uint32_t*)st.d_scratch.get();
    p.orig = st.d_scratch.get() + 4 * nmax * C;
    p.launch = st.d_scratch.get() + 5 * nmax * C;
    p.record = st.d_record.get(), p.accepted = st.d_accepted.get();
    p.clamp = h->clamp.mask_or_null();
    p.cn_class = h->constraints.class_or_null(), p.cn_bits = h->constraints.bits_or_null();
    p.fl_class = h->fields.class_or_null(), p.fl_field = h->fields.field_or_null();
    size_t lds;
    if (int rc = wave_chain_plan(h, 0, p, lds)) return rc;
    h->ent_prev_valid = false;  // (the block state moves)
    st.last.clear();
    if (p.fl_field)
        HIPCHK(h, launch_wave_chain(reshuffle_kernel<true, true, true>, reshuffle_kernel<false, true, true>, p, lds, h->stream));
    else if (p.cn_bits)
        HIPCHK(h, launch_wave_chain(reshuffle_kernel<true, true>, reshuffle_kernel<false, true>, p, lds, h->stream));
    else
        HIPCHK(h, launch_wave_chain(reshuffle_kernel<true, false>, reshuffle_kernel<false, false>, p, lds, h->stream));
    return read_back ? reshuffle_read_back(h) : BISBM_OK;
}

int bisbm::reshuffle_read_back(bisbm_engine* h) {
    ReshuffleState& st = h->reshuffle;
    const size_t C = h->n_chains;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    st.last.resize(C);
    st.accepted.resize(C);
    HIPCHK(h, hipMemcpy(st.last.data(), st.d_record.get(), sizeof(bisbm_reshuffle_record) * C, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(st.accepted.data(), st.d_accepted.get(), sizeof(unsigned long long) * C, hipMemcpyDeviceToHost));
    return BISBM_OK;
}

int bisbm::reshuffle_check_scans(bisbm_engine* h, uint32_t scans) {
    const uint64_t nmax = std::max(h->na, h->nb);
    if (nmax >= (1ull << 32) || 2 + (nmax + 127) / 128 + ((uint64_t)scans + 1) * nmax >= (1ull << 32))
        return fail(h, BISBM_ERR_INVALID_ARG, "scans = %u: a move of up to %llu members could use 2^32 draws or more", scans, (unsigned long long)nmax);
    return BISBM_OK;
}

extern "C" {

int bisbm_reshuffle_run(bisbm_handle h, uint64_t moves, uint32_t scans, double beta, uint64_t* accepted_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (h->rng_mode == BISBM_RNG_MT19937_COMPAT)
        return fail(h, BISBM_ERR_UNSUPPORTED, "pair reshuffles are defined in the Philox-mode arithmetic: this handle runs BISBM_RNG_MT19937_COMPAT");
    if (!(beta > 0.) || std::isinf(beta)) return fail(h, BISBM_ERR_INVALID_ARG, "beta = %g: a finite value above 0 is needed", beta);
    if (h->temper.L)
        return fail(h, BISBM_ERR_STATE, "replica exchange is on: sweeps run through bisbm_tempering_run (bisbm_tempering_set(h, 0, NULL) turns it off)");
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "pair reshuffles serve byte labels only (at most 256 blocks): merge the blocks down first");
    for (bisbm_engine* e : leaves(h))
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_reshuffle_run");
    if (int rc = reshuffle_check_scans(h, scans)) return rc;
    if (moves == 0) {
        for (uint32_t c = 0; accepted_out && c < h->n_chains; ++c) accepted_out[c] = 0;
        return BISBM_OK;
    }
    DeviceGuard keep;
    if (int rc = each_leaf(h, [&](bisbm_engine* e) { return reshuffle_engine(e, moves, scans, beta, false, true); })) return rc;
    for (uint32_t c = 0; accepted_out && c < h->n_chains; ++c) {
        uint32_t local;
        bisbm_engine* e = leaf_of_chain(h, c, &local);
        accepted_out[c] = e->reshuffle.accepted[local];
    }
    return BISBM_OK;
}

int bisbm_reshuffle_get_last(bisbm_handle h, bisbm_reshuffle_record* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!out) return fail(h, BISBM_ERR_INVALID_ARG, "out is NULL");
    for (uint32_t c = 0; c < h->n_chains; ++c) {
        uint32_t local;
        bisbm_engine* e = leaf_of_chain(h, c, &local);
        if (local >= e->reshuffle.last.size())
            return fail(h, BISBM_ERR_STATE, "chain %u has no pair reshuffle on record: call bisbm_reshuffle_run first", c);
    }
    for (uint32_t c = 0; c < h->n_chains; ++c) {
        uint32_t local;
        bisbm_engine* e = leaf_of_chain(h, c, &local);
        out[c] = e->reshuffle.last[local];
    }
    return BISBM_OK;
}

int bisbm_reshuffle_get_total(bisbm_handle h, uint64_t* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->devs.empty() && out) return on_devices(h, [&](bisbm_engine* d, size_t i) { return bisbm_reshuffle_get_total(d, out + h->dev_first[i]); });
    if (!out) return fail(h, BISBM_ERR_INVALID_ARG, "out is NULL");
    if (!h->groups.empty()) return gather_groups<uint64_t>(h, out, [](bisbm_engine* g, uint64_t* o) { return bisbm_reshuffle_get_total(g, o); });
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<ChainScalars> sc(h->n_chains);
    HIPCHK(h, hipMemcpy(sc.data(), h->d_scalars, sizeof(ChainScalars) * h->n_chains, hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < h->n_chains; ++c) out[c] = sc[c].reshuffles_total;
    return BISBM_OK;
}

int bisbm_debug_exp(bisbm_handle h, const double* x, size_t count, double* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->devs.empty()) {
        const int rc = bisbm_debug_exp(h->devs[0], x, count, out);
        if (rc) h->err = h->devs[0]->err;
        return rc;
    }
    if (!x || !out) return fail(h, BISBM_ERR_INVALID_ARG, "NULL argument");
    if (count == 0) return BISBM_OK;
    DeviceGuard keep;
    HIPCHK(h, hipSetDevice(h->device));
    DeviceBuf<double> dx, dout;
    RESERVE(h, dx, count);
    RESERVE(h, dout, count);
    HIPCHK(h, hipMemcpy(dx.get(), x, sizeof(double) * count, hipMemcpyHostToDevice));
    HIPCHK(h, launch_exp_probe(dx.get(), count, dout.get(), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, dout.get(), sizeof(double) * count, hipMemcpyDeviceToHost));
    return BISBM_OK;
}

}  // extern "C"
