// bisbm_heatbath.hip -- moving nodes by their conditionals: heat-bath (Gibbs) sweeps at a finite beta and greedy polishing at
// beta = +inf (no reference counterpart; include/bisbm.h, "Heat-bath sweeps and greedy polishing", states the visit order, the
// choice and what a move updates).  The row of the visited node -- dS_s and P(s) over all blocks s of its type -- is the row of
// "Node conditionals": the same f64 operations in the same order as cond_rows_kernel of bisbm_conditionals.hip, restated here
// because this kernel reads the block state from LDS and keeps the list and the row in LDS arrays of its own.
//
// Kernel: one wave per chain, persistent over all sweeps of the call, like the generic sweep_kernel.  The chain state in LDS, its
// load and store-back, the chunk header's parked neighbour labels, the list of the non-zero (t, k_t) and the move are the
// WaveChain of bisbm_wave_chain.hpp, shared with reshuffle_kernel; this file holds the visit order, the row and the choice.  A
// sweep is two phases, type a then type b, each walked through TiledOrder in chunks of 64 positions that never straddle the
// two; the visited class is an independent set.  A step touches HBM only for rows longer than 64, the lgamma / log_q tables
// and the label it writes.
//
// Step: the list, with the r side's two table values per entry in LDS arrays of this kernel's own, then lane <-> target block s
// (a type with more than 64 blocks is walked in chunks of 64 lanes): per list entry
// two table gathers and one f64 add in list order, eight entries in flight together, then the three tails, whose gathers are
// issued before the list is walked.  min, Z and the running sum C_s are sequential in ascending s over k_own terms: the lane of
// block s holds its value and every lane adds them one v_readlane at a time.  A node that is not free (a one-
// block type, or alone in its block) is skipped before any of this: its conditional is the point mass on r.  A clamped node
// (include/bisbm.h, "Clamped nodes") is skipped in the chunk header already: the loop over a chunk walks its open positions.
// Under block constraints (include/bisbm.h, "Block constraints") a node with one allowed block is skipped the same way, and the
// row of every other node is restricted to its allowed blocks: they alone enter the minimum, and the others have weight 0.0.
#include "bisbm_engine.hpp"
#include "bisbm_wave_chain.hpp"

using namespace bisbm;

namespace bisbm {

namespace {

// CL: the launch has a clamp (p.clamp is not NULL).  Without one the instance reads no mask and counts through the chunk as it
// always did: an unclamped handle runs the code it ran before the clamp existed.
// CN: the launch has block constraints (p.cn_bits is not NULL; p.clamp may be set as well): the one instance that walks the
// chunk as a clamped launch does and restricts the rows.  The two instances without it hold none of its code.
// FL: the launch has block fields (p.fl_field is not NULL; include/bisbm.h, "Block fields"): the one instance per EL that adds the
// field to the row.  It is compiled with CL and CN and serves a clamp and constraints beside the field by testing their pointers
// at run time; the instances without it hold none of its code.
template <bool EL, bool CL, bool CN, bool FL = false>
__global__ __launch_bounds__(kWave) void heatbath_kernel(HeatbathParams p) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const uint32_t chain = blockIdx.x;
    if (chain >= p.n_chains) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t kmax = p.ka > p.kb ? p.ka : p.kb;

    // this kernel's own arrays, then the chain state
    unsigned char* cur = lds_raw;
    double* s_L1 = (double*)cur;  // lg(m_rt + 1) per list entry
    cur += sizeof(double) * kmax;
    double* s_L3 = (double*)cur;  // lg(m_rt - k_t + 1)
    cur += sizeof(double) * kmax;
    double* s_dS = (double*)cur;  // dS per target
    cur += sizeof(double) * kmax;
    double* s_x = (double*)cur;   // w, then P per target
    cur += sizeof(double) * kmax;
    WaveChain<EL> wc;
    wc.load(cur, p, chain);
    int32_t *const mr = wc.mr, *const nr = wc.nr;  // (the names the row's code below reads the state by)
    const uint32_t D = wc.D;
    ChainScalars* sc = p.scalars + chain;
    double cum_dS = sc->cum_dS;
    uint64_t sweeps_total = sc->sweeps_total;
    __syncthreads();

    const Tables tab{p.lgamma_tab, p.lgamma_size, p.q_tab, p.q_stride, p.log_tab};
    const uint32_t chain_gid = chain_gid_of(p, chain);
    const double beta = chain_beta_of(p, chain);  // (the launch's, or under replica exchange the chain's own)
    uint64_t moved = 0, sweeps_run = 0;
    for (uint64_t sweep = 0; sweep < p.rounds; ++sweep) {
        uint64_t moved_sweep = 0;
        for (uint32_t phase = 0; phase < 2; ++phase) {
            const bool tb = phase != 0;
            const TypeView ty = type_view(p, tb);
            const uint32_t n_cls = ty.n_cls, v0 = ty.v0, k_own = ty.k_own, own0 = ty.own0;
            if (k_own <= 1u) continue;  // (nobody of a one-block type is free)
            TiledOrder order;
            order.init(phx_draw(p.seed, chain_gid, PHX_SWEEP_KEY, 2 * sweeps_total + phase), n_cls);
            for (uint32_t vi0 = 0; vi0 < n_cls; vi0 += kWave) {
                // ---- chunk header: lane q holds the node, row extent and own label of position vi0 + q ----
                const uint32_t cnt = n_cls - vi0 < (uint32_t)kWave ? n_cls - vi0 : (uint32_t)kWave;
                uint32_t v_l = 0, beg_l = 0, deg_l = 0, r_l = 0, held_l = 0, cls_l = 0, fcls_l = 0;
                if (lane < cnt) {
                    v_l = v0 + order(vi0 + lane);
                    beg_l = p.rowptr[v_l];
                    deg_l = p.rowptr[v_l + 1] - beg_l;
                    r_l = wc.labels[v_l];
                    if (CL && !CN) held_l = p.clamp[v_l];
                    if (CN && !FL) {  // (held: clamped, or a class with one allowed block of the type)
                        cls_l = p.cn_class[v_l];
                        held_l = ((p.clamp && p.clamp[v_l] != 0) || cn_count(p.cn_bits, cls_l, own0, k_own) <= 1u) ? 1u : 0u;
                    }
                    if (FL) {  // (the same with the constraints' pointers tested; the field class of the node)
                        if (p.cn_bits) cls_l = p.cn_class[v_l];
                        held_l = ((p.clamp && p.clamp[v_l] != 0) || (p.cn_bits && cn_count(p.cn_bits, cls_l, own0, k_own) <= 1u)) ? 1u : 0u;
                        fcls_l = p.fl_class[v_l];
                    }
                }
                // under a clamp, the open positions of the chunk: a clamped node stays as a node that is not free does, its row
                // is not parked (extent 0), a chunk without an open position reads no row at all, and the loop walks the ballot
                unsigned long long open = CL ? __ballot(lane < cnt && held_l == 0u) : 0ull;
                if (CL && open == 0ull) continue;
                wc.park_rows(cnt, beg_l, CL && held_l ? 0u : deg_l);

                for (uint32_t qi = 0; CL ? open != 0ull : qi < cnt; ++qi) {
                    uint32_t q = qi;
                    if (CL) {
                        q = (uint32_t)__ffsll((long long)open) - 1u;
                        open &= open - 1ull;
                    }
                    const uint32_t v = readlane(v_l, q), beg = readlane(beg_l, q), deg = readlane(deg_l, q);
                    const uint32_t r = readlane(r_l, q), r_loc = r - own0;
                    if (r_loc >= k_own) continue;  // (a valid label: never)
                    const uint32_t cls = CN ? readlane(cls_l, q) : 0u;  // (wave-uniform: the table reads below are of one row)
                    // is block tid of the type in A_v (the node's own block always is)?
                    auto admits = [&](uint32_t tid) { return !CN || (FL && !p.cn_bits) || tid == r_loc || cn_allows(p.cn_bits, cls, own0 + tid); };
                    // block fields: the row of the node's class (wave-uniform), f[r] for every lane
                    const double* f_row = FL ? p.fl_field + (size_t)readlane(fcls_l, q) * (p.ka + p.kb) : nullptr;
                    const double f_r = FL ? f_row[r] : 0.;
                    const int n0r = nr[r];
                    if (n0r <= 1) continue;  // not free: the node stays, and no draw is used
                    // 1., 2. k_v and the non-zero (t, k_t) in ascending t, with the r side's two table values
                    const uint32_t nnz = wc.neighbour_list(q, beg, deg, ty, [&](uint32_t pos, uint32_t t, int kt) {
                        const int32_t m_rt = wc.M(tb, r_loc, t);
                        s_L1[pos] = lgamma_fast(tab, (long long)m_rt + 1);
                        s_L3[pos] = lgamma_fast(tab, (long long)m_rt - kt + 1);
                    });
                    // 3. dS of target s = tid (steps 1 of "Node conditionals")
                    const int ideg = (int)deg;
                    const int m0r = mr[r];
                    const long long eta_r = *wc.eta_at(r * D + deg);
                    // the r side of the tails is the same for every target
                    const double tail1_r = lgamma_fast(tab, (long long)m0r - ideg + 1) - lgamma_fast(tab, (long long)m0r + 1);
                    const double tail2_r = lgamma_fast(tab, eta_r + 1) - lgamma_fast(tab, eta_r);
                    for (uint32_t c0 = 0; c0 < k_own; c0 += kWave) {
                        const uint32_t tid = c0 + lane;
                        const uint32_t s = tid < k_own ? own0 + tid : r;  // (idle lanes evaluate r's own values)
                        const int m0s = mr[s], n0s = nr[s];
                        // every table gather of the tails is issued before the list is walked: the s side's four lgamma values
                        // and the log n of the three log_q evaluations below
                        const long long eta_s = *wc.eta_at(s * D + deg);
                        const double lg_s1 = lgamma_fast(tab, (long long)m0s + ideg + 1), lg_s0 = lgamma_fast(tab, (long long)m0s + 1);
                        const double lg_e1 = lgamma_fast(tab, eta_s + 1), lg_e2 = lgamma_fast(tab, eta_s + 2);
                        const int qn_r = (lane & 1u) ? m0r : m0r - ideg, qk_r = (lane & 1u) ? n0r : n0r - 1;
                        const double ln_s1 = log_n_of(tab, m0s + ideg), ln_s0 = log_n_of(tab, m0s), ln_r = log_n_of(tab, qn_r);
                        double acc = 0.;
                        // eight list entries at a time: their reads of m and the sixteen table gathers are in flight together;
                        // the adds keep the list order (past the end of the list the last entry is read again and not added)
                        for (uint32_t i = 0; i < nnz; i += 8) {
                            int32_t m_st[8];
                            double a[8], b[8];
#pragma unroll
                            for (uint32_t j = 0; j < 8; ++j) m_st[j] = wc.M(tb, tid < k_own ? tid : r_loc, wc.s_t[i + j < nnz ? i + j : nnz - 1u]);
#pragma unroll
                            for (uint32_t j = 0; j < 8; ++j) {
                                a[j] = lgamma_fast(tab, (long long)m_st[j] + 1);
                                b[j] = lgamma_fast(tab, (long long)m_st[j] + wc.s_kt[i + j < nnz ? i + j : nnz - 1u] + 1);
                            }
#pragma unroll
                            for (uint32_t j = 0; j < 8; ++j)
                                if (i + j < nnz) acc = acc + ((s_L1[i + j] + a[j]) - (s_L3[i + j] + b[j]));
                        }
                        // the four log_q values through one copy of its code: the target's two, then the r side's two in
                        // lanes 0 and 1
                        double lq_s1 = 0., lq_s0 = 0., lq_r = 0.;
#pragma nounroll
                        for (uint32_t it = 0; it < 3; ++it) {
                            const int qn = it == 0 ? m0s + ideg : it == 1 ? m0s : qn_r;
                            const int qk = it == 0 ? n0s + 1 : it == 1 ? n0s : qk_r;
                            const double val = log_q<true>(tab, qn, qk, it == 0 ? ln_s1 : it == 1 ? ln_s0 : ln_r);
                            if (it == 0)
                                lq_s1 = val;
                            else if (it == 1)
                                lq_s0 = val;
                            else
                                lq_r = val;
                        }
                        const double tail1 = tail1_r + (lg_s1 - lg_s0);
                        const double tail2 = tail2_r + (lg_e1 - lg_e2);
                        const double tail3 = (readlane(lq_r, 0u) - readlane(lq_r, 1u)) + (lq_s1 - lq_s0);
                        if (FL) {  // (one coalesced read of the row; idle lanes do not index the table: the last row ends the allocation)
                            if (tid < k_own) s_dS[tid] = tid == r_loc ? 0. : (((acc + tail1) + tail2) + tail3) + (f_row[own0 + tid] - f_r);
                        } else if (tid < k_own)
                            s_dS[tid] = tid == r_loc ? 0. : ((acc + tail1) + tail2) + tail3;
                    }
                    wave_fence();
                    // The passes that are sequential in ascending s by definition -- dS_min, Z, C_s -- run on registers: the lane of
                    // block s holds its value, and every lane adds the values one v_readlane at a time (64 blocks per trip).
                    // dS_min (the 0 at r included)
                    double mn = 0.;
                    for (uint32_t c0 = 0; c0 < k_own; c0 += kWave) {
                        const uint32_t tid = c0 + lane, cn = k_own - c0 < (uint32_t)kWave ? k_own - c0 : (uint32_t)kWave;
                        const double x = tid < k_own && admits(tid) ? s_dS[tid] : 0.;  // (the minimum is over A_v, the 0 at r included)
                        for (uint32_t s = 0; s < cn; ++s) {
                            const double y = readlane(x, s);
                            mn = y < mn ? y : mn;
                        }
                    }
                    uint32_t s_new = r_loc;
                    if (p.greedy) {
                        // 4. the lowest s that attains the minimum; a move only strictly downhill
                        if (!(mn < 0.)) continue;
                        for (uint32_t c0 = 0; c0 < k_own; c0 += kWave) {
                            const uint32_t tid = c0 + lane;
                            const unsigned long long hit = __ballot(tid < k_own && tid != r_loc && admits(tid) && s_dS[tid] == mn);
                            if (hit) {
                                s_new = c0 + (uint32_t)__ffsll((long long)hit) - 1u;
                                break;
                            }
                        }
                    } else {
                        // 3. weights and Z = w_0 + w_1 + ... (0.0 + w_0 is w_0) ...
                        double Z = 0.;
                        for (uint32_t c0 = 0; c0 < k_own; c0 += kWave) {
                            const uint32_t tid = c0 + lane, cn = k_own - c0 < (uint32_t)kWave ? k_own - c0 : (uint32_t)kWave;
                            double w = 0.;
                            if (tid < k_own) {
                                const double x = beta * (s_dS[tid] - mn);
                                w = x > 700. || !admits(tid) ? 0. : exp(-x);  // (exactly 0.0 outside A_v)
                                s_x[tid] = w;
                            }
                            for (uint32_t s = 0; s < cn; ++s) Z = Z + readlane(w, s);
                        }
                        wave_fence();
                        // ... then P = w / Z and C_s = P_0 + ... + P_s: the first s with u < C_s, else the largest s with P_s > 0
                        const uint64_t pos = (uint64_t)v0 + vi0 + q;  // position in the sweep
                        const U4 A = phx_draw(p.seed, chain_gid, PHX_HEATBATH, sweeps_total * (uint64_t)p.n + pos);
                        const double u = u53(A.x, A.y);
                        double C = 0.;
                        for (uint32_t c0 = 0; c0 < k_own; c0 += kWave) {
                            const uint32_t tid = c0 + lane, cn = k_own - c0 < (uint32_t)kWave ? k_own - c0 : (uint32_t)kWave;
                            const double P = tid < k_own ? s_x[tid] / Z : 0.;
                            double C_mine = 0.;
                            for (uint32_t s = 0; s < cn; ++s) {
                                C = C + readlane(P, s);
                                if (lane == s) C_mine = C;
                            }
                            const unsigned long long hit = __ballot(tid < k_own && u < C_mine);
                            if (hit) {
                                s_new = c0 + (uint32_t)__ffsll((long long)hit) - 1u;
                                break;
                            }
                            const unsigned long long some = __ballot(P > 0.);
                            if (some) s_new = c0 + 63u - (uint32_t)__clzll((long long)some);  // (P_r > 0: there is one)
                        }
                    }
                    s_new = readlane(s_new, 0u);  // (the same in every lane; this tells the compiler)
                    if (s_new == r_loc || s_new >= k_own) continue;
                    // 5. apply_mcmc_moves, as mh_step does
                    const double dS_new = s_dS[s_new];
                    const uint32_t s_glob = own0 + s_new;
                    wc.apply_move(v, deg, r, s_glob, r_loc, s_new, tb, nnz);
                    cum_dS = cum_dS + dS_new;
                    ++moved_sweep;
                }
            }
            __threadfence_block();  // the labels this phase wrote are read by the next phase's headers
        }
        ++sweeps_total;
        ++sweeps_run;
        moved += moved_sweep;
        if (p.stop_when_settled && moved_sweep == 0) break;
    }

    wc.store();
    if (lane == 0) {
        sc->cum_dS = cum_dS;
        sc->sweeps_total = sweeps_total;
        sc->last_accepted = moved;
        sc->last_sweeps = sweeps_run;
    }
}

}  // namespace

}  // namespace bisbm

void bisbm::wave_chain_fill(const bisbm_engine* h, double beta, bool per_rung, WaveChainParams& p) {
    p.rowptr = h->d_rowptr, p.col = h->d_col;
    p.n = (uint32_t)h->n, p.na = (uint32_t)h->na, p.nb = (uint32_t)h->nb;
    p.ka = h->ka, p.kb = h->kb, p.maxdeg = h->maxdeg;
    p.n_chains = h->n_chains, p.first_chain_id = h->first_chain_id, p.chain_gids = h->d_gids;
    p.labels = h->d_labels, p.label_stride = h->label_stride;
    p.m = h->d_m, p.m_r = h->d_m_r, p.n_r = h->d_n_r, p.eta = h->d_eta;
    p.scalars = h->d_scalars;
    p.lgamma_tab = h->d_lgamma, p.lgamma_size = h->tab->lg.size(), p.q_tab = h->d_q, p.q_stride = h->q_stride, p.log_tab = h->d_logtab;
    p.seed = h->seed;
    p.beta = beta;
    if (per_rung) p.beta_rung = h->temper.d_beta.get(), p.rung = h->temper.d_rung.get();
}

int bisbm::wave_chain_plan(bisbm_engine* h, size_t own_bytes, WaveChainParams& p, size_t& lds) {
    // eta goes to LDS when that still leaves room for four chains per CU, as in the generic sweep kernel's plan
    p.eta_in_lds = own_bytes + wave_chain_lds_bytes(h->ka, h->kb, h->maxdeg, true) <= 40 * 1024 ? 1 : 0;
    lds = own_bytes + wave_chain_lds_bytes(h->ka, h->kb, h->maxdeg, p.eta_in_lds != 0);
    if (lds > kLdsPerCu) return fail(h, BISBM_ERR_UNSUPPORTED, "chain state needs %zu B of LDS (> 160 KiB)", lds);
    return BISBM_OK;
}

int bisbm::heatbath_engine(bisbm_engine* h, uint64_t sweeps, double beta, int stop_when_settled, bool per_rung, bool sync) {
    HIPCHK(h, hipSetDevice(h->device));
    HeatbathParams p{};
    p.rounds = sweeps;
    p.greedy = !per_rung && std::isinf(beta) ? 1u : 0u;
    wave_chain_fill(h, p.greedy ? 0. : beta, per_rung, p);
    p.stop_when_settled = stop_when_settled ? 1u : 0u;
    p.clamp = h->clamp.mask_or_null();
    p.cn_class = h->constraints.class_or_null(), p.cn_bits = h->constraints.bits_or_null();
    p.fl_class = h->fields.class_or_null(), p.fl_field = h->fields.field_or_null();
    size_t lds;  // (the four double[kmax] arrays of the kernel's own: a multiple of 16 bytes, as the rounded chain state is)
    if (int rc = wave_chain_plan(h, 4 * sizeof(double) * std::max(h->ka, h->kb), p, lds)) return rc;
    h->ent_prev_valid = false;  // (the block state moves)
    if (p.fl_field)
        HIPCHK(h, launch_wave_chain(heatbath_kernel<true, true, true, true>, heatbath_kernel<false, true, true, true>, p, lds, h->stream));
    else if (p.cn_bits)
        HIPCHK(h, launch_wave_chain(heatbath_kernel<true, true, true>, heatbath_kernel<false, true, true>, p, lds, h->stream));
    else if (p.clamp)
        HIPCHK(h, launch_wave_chain(heatbath_kernel<true, true, false>, heatbath_kernel<false, true, false>, p, lds, h->stream));
    else
        HIPCHK(h, launch_wave_chain(heatbath_kernel<true, false, false>, heatbath_kernel<false, false, false>, p, lds, h->stream));
    if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
    return BISBM_OK;
}

extern "C" {

int bisbm_heatbath_run(bisbm_handle h, uint64_t sweeps, double beta, int stop_when_settled, uint64_t* moved_out, uint64_t* sweeps_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (h->rng_mode == BISBM_RNG_MT19937_COMPAT)
        return fail(h, BISBM_ERR_UNSUPPORTED, "heat-bath sweeps are defined in the Philox-mode arithmetic: this handle runs BISBM_RNG_MT19937_COMPAT");
    if (!(beta > 0.)) return fail(h, BISBM_ERR_INVALID_ARG, "beta = %g: a value above 0 is needed (+inf: greedy)", beta);
    if (h->temper.L)
        return fail(h, BISBM_ERR_STATE, "replica exchange is on: sweeps run through bisbm_tempering_run (bisbm_tempering_set(h, 0, NULL) turns it off)");
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "heat-bath sweeps serve byte labels only (at most 256 blocks): merge the blocks down first");
    for (bisbm_engine* e : leaves(h))
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_heatbath_run");
    if (sweeps == 0) {
        for (uint32_t c = 0; c < h->n_chains; ++c) {
            if (moved_out) moved_out[c] = 0;
            if (sweeps_out) sweeps_out[c] = 0;
        }
        return BISBM_OK;
    }
    DeviceGuard keep;
    if (int rc = each_leaf(h, [&](bisbm_engine* e) { return heatbath_engine(e, sweeps, beta, stop_when_settled, false, true); })) return rc;
    if (!moved_out && !sweeps_out) return BISBM_OK;
    return bisbm_get_last_counts(h, moved_out, sweeps_out);
}

}  // extern "C"
