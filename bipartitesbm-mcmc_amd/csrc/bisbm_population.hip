// bisbm_population.hip -- population annealing over the chains of a handle (no reference counterpart: the reference runs one
// chain).  All chains sit at one temperature; between temperature steps the population is resampled by description length:
// the offspring counts and the parent map are computed on the host from the chains' description lengths (the pure function
// bisbm_population_offspring), and the state of every dead slot is overwritten with its parent's by the copy kernel below --
// one launch per step and engine, plain vector loads and stores.  include/bisbm.h states the definition.
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

// What one launch of the copy kernel moves: for every job (dead slot d of the destination engine, parent s of the source
// engine -- the same engine, or another entry of the handle on the same device) the label row, m, m_r, n_r, eta and the running
// sum of dS.  A chain's state is addressed as `items`: first the 16-byte words of its label row (rows are 256-label aligned),
// then the 4-byte words of its m, m_r, n_r and eta slices one after the other (a slice starts at chain * ka * kb * 4 bytes and
// the like: not 16-byte aligned in general).
struct CopyParams {
    const uint2* jobs;
    uint32_t n_seg;      // segments of kCopySegment items per chain
    uint32_t lab_words;  // 16-byte words of a label row
    uint32_t nm, K, neta;  // 4-byte words of a chain's m, of its m_r (and n_r), of its eta
    const uint4* src_labels;
    const uint32_t *src_m, *src_m_r, *src_n_r, *src_eta;
    const ChainScalars* src_scalars;
    uint4* dst_labels;
    uint32_t *dst_m, *dst_m_r, *dst_n_r, *dst_eta;
    ChainScalars* dst_scalars;
};

// A workgroup streams one segment: every lane loads its kCopyPerLane items, then stores them, so a workgroup keeps up to 16 KiB
// of loads in flight and two resident workgroups per CU reach the ~32 KiB per CU at which HBM streams.
constexpr uint32_t kCopyThreads = 256, kCopyPerLane = 4, kCopySegment = kCopyThreads * kCopyPerLane;

template <class T>
__device__ __forceinline__ T* word_at(T* m, T* m_r, T* n_r, T* eta, const CopyParams& p, size_t chain, uint32_t w) {
    if (w < p.nm) return m + chain * p.nm + w;
    w -= p.nm;
    if (w < p.K) return m_r + chain * p.K + w;
    w -= p.K;
    if (w < p.K) return n_r + chain * p.K + w;
    w -= p.K;
    return eta + chain * p.neta + w;
}

// One workgroup per (job, segment).  Sources are survivors and destinations are dead slots, so no job reads what another
// writes; every word has one writer.
__global__ __launch_bounds__(kCopyThreads) void population_copy_kernel(CopyParams p) {
    const uint32_t job = blockIdx.x / p.n_seg, seg = blockIdx.x % p.n_seg;
    const uint2 j = p.jobs[job];
    const size_t d = j.x, s = j.y;
    const uint32_t items = p.lab_words + p.nm + 2u * p.K + p.neta;
    const uint32_t first = seg * kCopySegment + threadIdx.x;
    // (an item travels in a uint4: a 16-byte label word whole, a 4-byte word in .x)
    auto load = [&](uint32_t i) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i < p.lab_words)
            v = p.src_labels[s * p.lab_words + i];
        else if (i < items)
            v.x = *word_at(p.src_m, p.src_m_r, p.src_n_r, p.src_eta, p, s, i - p.lab_words);
        return v;
    };
    auto store = [&](uint32_t i, const uint4& v) {
        if (i < p.lab_words)
            p.dst_labels[d * p.lab_words + i] = v;
        else if (i < items)
            *word_at(p.dst_m, p.dst_m_r, p.dst_n_r, p.dst_eta, p, d, i - p.lab_words) = v.x;
    };
    static_assert(kCopyPerLane == 4, "the loads of a lane are written out");
    const uint4 v0 = load(first), v1 = load(first + kCopyThreads), v2 = load(first + 2 * kCopyThreads), v3 = load(first + 3 * kCopyThreads);
    store(first, v0), store(first + kCopyThreads, v1), store(first + 2 * kCopyThreads, v2), store(first + 3 * kCopyThreads, v3);
    if (seg == 0 && threadIdx.x == 0) p.dst_scalars[d].cum_dS = p.src_scalars[s].cum_dS;
}

constexpr uint64_t kNoStop = 1ull << 60;  // steps_await of the sweeps of a run: no early stop (as BlockModel.run_sweeps)

// the handles population annealing does not serve, in the order of the table in include/bisbm.h
int refuse(bisbm_engine* h) {
    if (h->rng_mode == BISBM_RNG_MT19937_COMPAT)
        return fail(h, BISBM_ERR_UNSUPPORTED, "population annealing runs in Philox mode only (mt19937-compat mode is the reference's verification path)");
    if (any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "population annealing needs byte labels: some chain of this handle has more than 256 blocks (wide mode)");
    if (any_grouped(h) || !common_shape(h))
        return fail(h, BISBM_ERR_STATE, "the chains of this handle are grouped by shape (a one-argument bisbm_agg_merge_total left different block counts): a chain's state cannot move into a slot of another shape");
    if (h->temper.L)
        return fail(h, BISBM_ERR_STATE, "replica exchange is on: a population sits at one temperature (bisbm_tempering_set(h, 0, NULL) turns it off)");
    if (h->modes.n_modes && !h->modes.anchored)  // (anchored modes assign every chain afresh at every sample)
        return fail(h, BISBM_ERR_STATE, "mode-resolved marginals are set (bisbm_marginals_set_modes): a slot that takes another chain's state has no mode of its own; turn the modes off first");
    return BISBM_OK;
}

// The copies of one step into device entry `dst` (chains first_dst .. of the handle): the jobs whose parent lives in an entry on
// the same device go through the kernel, one launch per source entry; the others go straight between the entries' buffers.
// Everything runs on dst's stream, which is idle again when the call returns; the caller has synchronised every entry before.
int copy_into(bisbm_engine* h, bisbm_engine* dst, uint32_t first_dst, const std::vector<uint32_t>& parent) {
    HIPCHK(dst, hipSetDevice(dst->device));
    const std::vector<bisbm_engine*> entries = device_entries(h);
    std::vector<std::vector<uint2>> jobs(entries.size());  // by source entry
    size_t total = 0;
    for (uint32_t c = 0; c < dst->n_chains; ++c) {
        const uint32_t p = parent[first_dst + c];
        if (p == first_dst + c) continue;
        uint32_t local = p;
        const uint32_t e = h->devs.empty() ? 0u : dev_of_chain(h, p, &local);
        jobs[e].push_back(make_uint2(c, local));
        ++total;
    }
    if (!total) return BISBM_OK;
    const size_t nm = (size_t)dst->ka * dst->kb, K = dst->K, neta = K * ((size_t)dst->maxdeg + 1), lab_words = dst->label_stride / 16;
    const size_t items = lab_words + nm + 2 * K + neta;
    const size_t n_seg = (items + kCopySegment - 1) / kCopySegment;
    // (a launch takes fewer than 2^32 lanes: 2^24 workgroups of kCopyThreads)
    if (items >= (1ull << 31) || total * n_seg >= (1ull << 32) / kCopyThreads)
        return fail(dst, BISBM_ERR_UNSUPPORTED, "a resampling step of %zu copies of %zu words each is more than one launch addresses", total, items);
    RESERVE(dst, dst->population.d_jobs, total);
    size_t at = 0;
    for (size_t e = 0; e < entries.size(); ++e) {
        if (jobs[e].empty()) continue;
        bisbm_engine* src = entries[e];
        if (src->device != dst->device) {  // sources are survivors: nothing is staged
            for (const uint2 j : jobs[e]) {
                const size_t d = j.x, s = j.y;
                auto peer = [&](void* to, const void* from, size_t bytes) {
                    return hipMemcpyPeerAsync(to, dst->device, from, src->device, bytes, dst->stream);
                };
                HIPCHK(dst, peer(dst->d_labels + d * dst->label_stride, src->d_labels + s * src->label_stride, dst->label_stride));
                HIPCHK(dst, peer(dst->d_m + d * nm, src->d_m + s * nm, sizeof(int32_t) * nm));
                HIPCHK(dst, peer(dst->d_m_r + d * K, src->d_m_r + s * K, sizeof(int32_t) * K));
                HIPCHK(dst, peer(dst->d_n_r + d * K, src->d_n_r + s * K, sizeof(int32_t) * K));
                HIPCHK(dst, peer(dst->d_eta + d * neta, src->d_eta + s * neta, sizeof(uint32_t) * neta));
                HIPCHK(dst, peer(&dst->d_scalars[d].cum_dS, &src->d_scalars[s].cum_dS, sizeof(double)));
            }
            continue;
        }
        uint2* d_jobs = dst->population.d_jobs.get() + at;
        at += jobs[e].size();
        HIPCHK(dst, hipMemcpyAsync(d_jobs, jobs[e].data(), sizeof(uint2) * jobs[e].size(), hipMemcpyHostToDevice, dst->stream));
        CopyParams p{};
        p.jobs = d_jobs;
        p.n_seg = (uint32_t)n_seg;
        p.lab_words = (uint32_t)lab_words;
        p.nm = (uint32_t)nm, p.K = (uint32_t)K, p.neta = (uint32_t)neta;
        p.src_labels = (const uint4*)src->d_labels;
        p.src_m = (const uint32_t*)src->d_m, p.src_m_r = (const uint32_t*)src->d_m_r, p.src_n_r = (const uint32_t*)src->d_n_r, p.src_eta = src->d_eta;
        p.src_scalars = src->d_scalars;
        p.dst_labels = (uint4*)dst->d_labels;
        p.dst_m = (uint32_t*)dst->d_m, p.dst_m_r = (uint32_t*)dst->d_m_r, p.dst_n_r = (uint32_t*)dst->d_n_r, p.dst_eta = dst->d_eta;
        p.dst_scalars = dst->d_scalars;
        hipLaunchKernelGGL(population_copy_kernel, dim3((uint32_t)(jobs[e].size() * n_seg)), dim3(kCopyThreads), 0, dst->stream, p);
        HIPCHK(dst, hipGetLastError());
    }
    // the block state of some slots changed under the baseline the running sum of dS is advanced from: the next anneal takes
    // a fresh one (the copied cum_dS belongs to the copied state, so the identity holds from there on)
    dst->ent_prev_valid = false;
    HIPCHK(dst, hipStreamSynchronize(dst->stream));  // (the job lists are read from this call's host memory)
    return BISBM_OK;
}

int copy_states(bisbm_engine* h, const std::vector<uint32_t>& parent) {
    DeviceGuard guard;
    const std::vector<bisbm_engine*> entries = device_entries(h);
    // (bisbm_entropy has synchronised every entry's stream: no source is still being written)
    uint32_t first = 0;
    int rc = BISBM_OK;
    for (bisbm_engine* e : entries) {
        if (!rc) {
            rc = copy_into(h, e, first, parent);
            if (rc && e != h) h->err = e->err;
        }
        first += e->n_chains;
    }
    if (rc)  // (nothing of a failed step stays in flight)
        for (bisbm_engine* e : entries)
            if (hipSetDevice(e->device) == hipSuccess) (void)hipStreamSynchronize(e->stream);
    return rc;
}

int check_temps(bisbm_engine* h, uint32_t n_temps, const float* temps) {
    if (n_temps < 2) return fail(h, BISBM_ERR_INVALID_ARG, "a population run needs at least 2 temperatures (n_temps = %u)", n_temps);
    if (!temps) return fail(h, BISBM_ERR_INVALID_ARG, "temps is NULL");
    for (uint32_t k = 0; k < n_temps; ++k) {
        if (!std::isfinite(temps[k]) || !(temps[k] > 0.f))
            return fail(h, BISBM_ERR_INVALID_ARG, "temps[%u] = %g: every temperature must be finite and > 0", k, (double)temps[k]);
        if (k && temps[k] > temps[k - 1])
            return fail(h, BISBM_ERR_INVALID_ARG, "temps[%u] = %g > temps[%u] = %g: the temperatures must be non-increasing", k, (double)temps[k], k - 1,
                        (double)temps[k - 1]);
    }
    return BISBM_OK;
}

}  // namespace

extern "C" {

int bisbm_population_offspring(uint32_t n, const double* S, double delta_beta, double u, uint32_t* offspring_out, uint32_t* parent_out,
                               double* log_ratio_out) {
    if (n == 0) return fail(nullptr, BISBM_ERR_INVALID_ARG, "a population needs at least one chain (n = 0)");
    if (!S) return fail(nullptr, BISBM_ERR_INVALID_ARG, "S is NULL");
    if (!std::isfinite(delta_beta) || delta_beta < 0.)
        return fail(nullptr, BISBM_ERR_INVALID_ARG, "delta_beta = %g: a resampling step goes to a lower or the same temperature (finite, >= 0)", delta_beta);
    if (!(u >= 0. && u < 1.)) return fail(nullptr, BISBM_ERR_INVALID_ARG, "u = %g is outside [0, 1)", u);
    double s_min = S[0];
    for (uint32_t c = 0; c < n; ++c) {
        if (!std::isfinite(S[c])) return fail(nullptr, BISBM_ERR_INVALID_ARG, "S[%u] = %g is not finite", c, S[c]);
        s_min = std::min(s_min, S[c]);
    }
    std::vector<double> cum(n);
    double W = 0.;
    for (uint32_t c = 0; c < n; ++c) {
        W += std::exp(-delta_beta * (S[c] - s_min));
        cum[c] = W;
    }
    if (log_ratio_out) *log_ratio_out = -delta_beta * s_min + std::log(W / (double)n);
    // systematic resampling: n_k = ceil(a_k - u) - ceil(a_{k-1} - u), a_{-1} = 0, a_k = min(n, (n * c_k) / W), a_{n-1} = n
    // exactly.  The min is part of the definition: where the trailing weights vanish beside W, c_k == W before the last slot,
    // and fl(fl(n * W) / W) can be n + 1 ulp, which a small u would round up to n + 1.  c_k does not fall and the f64 product
    // and quotient are monotone, so a_k does not fall either: 0 <= ceil(a_k - u) <= n, no n_k is negative, sum n_k = n.
    // ceil(a - u) is taken exactly, floor(a) + [a - floor(a) > u]: the subtraction a - u itself rounds (513 - (1 - 2^-53) is
    // 512 in f64)
    auto ceil_minus_u = [u](double a) {
        const double f = std::floor(a);
        return (uint64_t)f + (a - f > u ? 1u : 0u);
    };
    std::vector<uint32_t> off(n);
    uint64_t before = 0;  // (ceil(0 - u) = 0 for u in [0, 1))
    for (uint32_t k = 0; k < n; ++k) {
        const uint64_t here = ceil_minus_u(k + 1 < n ? std::min((double)n, (double)n * cum[k] / W) : (double)n);
        off[k] = (uint32_t)(here - before);
        before = here;
    }
    if (parent_out) {  // survivors keep their slot; the dead slots, ascending, take the surplus copies survivor by survivor
        uint32_t dead = 0;
        for (uint32_t k = 0; k < n; ++k) {
            if (off[k]) parent_out[k] = k;
            for (uint32_t copy = 1; copy < off[k]; ++copy) {
                while (off[dead]) ++dead;
                parent_out[dead++] = k;
            }
        }
    }
    if (offspring_out) std::copy(off.begin(), off.end(), offspring_out);
    return BISBM_OK;
}

int bisbm_population_reset(bisbm_handle h) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    h->population.ancestor.clear();
    h->population.rounds = 0;
    h->population.log_ratio_total = 0.;
    return BISBM_OK;
}

int bisbm_population_get(bisbm_handle h, uint32_t* ancestor_out, uint64_t* rounds_out, double* log_ratio_total_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    const PopulationState& s = h->population;
    if (ancestor_out)
        for (uint32_t c = 0; c < h->n_chains; ++c) ancestor_out[c] = s.ancestor.empty() ? c : s.ancestor[c];
    if (rounds_out) *rounds_out = s.rounds;
    if (log_ratio_total_out) *log_ratio_total_out = s.log_ratio_total;
    return BISBM_OK;
}

int bisbm_population_resample(bisbm_handle h, double beta_from, double beta_to, uint32_t* parent_out, double* log_ratio_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = refuse(h)) return rc;
    const double delta = beta_to - beta_from;
    if (!std::isfinite(beta_from) || !std::isfinite(beta_to) || delta < 0.)
        return fail(h, BISBM_ERR_INVALID_ARG, "beta_from = %g, beta_to = %g: a resampling step goes to a lower or the same temperature (finite, beta_to >= beta_from)",
                    beta_from, beta_to);
    PopulationState& s = h->population;
    const uint32_t C = h->n_chains;
    std::vector<double> S(C);
    if (int rc = bisbm_entropy(h, S.data())) return rc;
    if (h->fields.n_classes) {  // (block fields: the weights and the ln Z increment are those of E = S + Phi, the tilted target)
        std::vector<double> phi(C);
        if (int rc = bisbm_fields_energy(h, phi.data())) return rc;
        for (uint32_t c = 0; c < C; ++c) S[c] = S[c] + phi[c];
    }
    uint32_t U[4];
    philox_host(h->seed, h->first_chain_id, PHX_RESAMPLE, s.rounds, U);
    std::vector<uint32_t> parent(C);
    double log_ratio = 0.;
    if (int rc = bisbm_population_offspring(C, S.data(), delta, u53_host(U[0], U[1]), nullptr, parent.data(), &log_ratio))
        return fail(h, rc, "%s", g_create_error.c_str());
    if (int rc = copy_states(h, parent)) return rc;
    if (s.ancestor.empty()) {
        s.ancestor.resize(C);
        for (uint32_t c = 0; c < C; ++c) s.ancestor[c] = c;
    }
    for (uint32_t c = 0; c < C; ++c)
        if (parent[c] != c) s.ancestor[c] = s.ancestor[parent[c]];  // (a parent is a survivor: its own entry does not change)
    s.log_ratio_total += log_ratio;
    ++s.rounds;
    if (parent_out) std::copy(parent.begin(), parent.end(), parent_out);
    if (log_ratio_out) *log_ratio_out = log_ratio;
    return BISBM_OK;
}

int bisbm_population_run(bisbm_handle h, uint32_t n_temps, const float* temps, uint64_t sweeps_per_step, double* log_ratio_out,
                         uint32_t* distinct_out, double* acc_rate_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = refuse(h)) return rc;
    if (int rc = check_temps(h, n_temps, temps)) return rc;
    const uint32_t C = h->n_chains;
    std::vector<double> rate(C), acc(C, 0.);
    std::vector<uint8_t> seen(C);
    double ms = 0;
    uint64_t updates = 0;
    for (uint32_t k = 1; k < n_temps; ++k) {
        double log_ratio = 0.;
        if (int rc = bisbm_population_resample(h, 1. / (double)temps[k - 1], 1. / (double)temps[k], nullptr, &log_ratio)) return rc;
        if (log_ratio_out) log_ratio_out[k - 1] = log_ratio;
        if (distinct_out) {
            std::fill(seen.begin(), seen.end(), 0);
            uint32_t distinct = 0;
            for (uint32_t a : h->population.ancestor) distinct += !seen[a], seen[a] = 1;
            distinct_out[k - 1] = distinct;
        }
        if (!sweeps_per_step) continue;
        const float kw[2] = {temps[k], 0.f};
        if (int rc = bisbm_anneal(h, BISBM_SCHED_CONSTANT, kw, sweeps_per_step * h->n, kNoStop, rate.data())) return rc;
        for (uint32_t c = 0; c < C; ++c) acc[c] += rate[c];
        ms += h->last_kernel_ms;
        updates += h->last_updates;
    }
    if (sweeps_per_step) h->last_kernel_ms = ms, h->last_updates = updates;  // (the run's sweeps as one call)
    if (acc_rate_out)  // accepted steps / steps of the run: every step runs the same number of sweeps
        for (uint32_t c = 0; c < C; ++c) acc_rate_out[c] = sweeps_per_step ? acc[c] / (double)(n_temps - 1) : 0.;
    return BISBM_OK;
}

int bisbm_rounds_population_run(bisbm_handle h, uint32_t n_temps, const float* temps, uint64_t rounds_per_step, const bisbm_round_recipe* recipe,
                                double* log_ratio_out, uint32_t* distinct_out, double* acc_rate_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (int rc = refuse(h)) return rc;
    if (int rc = check_temps(h, n_temps, temps)) return rc;
    if (rounds_per_step) {
        if (!recipe) return fail(h, BISBM_ERR_INVALID_ARG, "recipe is NULL");
        if (!recipe->mh_sweeps && !recipe->heatbath_sweeps && !recipe->reshuffles)
            return fail(h, BISBM_ERR_INVALID_ARG, "the recipe runs nothing: mh_sweeps, heatbath_sweeps and reshuffles are all 0");
    }
    const bisbm_round_recipe r = rounds_per_step ? *recipe : bisbm_round_recipe{};
    const uint32_t C = h->n_chains;
    std::vector<double> rate(C), acc(C, 0.);
    std::vector<uint8_t> seen(C);
    double ms = 0;
    uint64_t updates = 0;
    for (uint32_t k = 1; k < n_temps; ++k) {
        double log_ratio = 0.;
        if (int rc = bisbm_population_resample(h, 1. / (double)temps[k - 1], 1. / (double)temps[k], nullptr, &log_ratio)) return rc;
        if (log_ratio_out) log_ratio_out[k - 1] = log_ratio;
        if (distinct_out) {
            std::fill(seen.begin(), seen.end(), 0);
            uint32_t distinct = 0;
            for (uint32_t a : h->population.ancestor) distinct += !seen[a], seen[a] = 1;
            distinct_out[k - 1] = distinct;
        }
        const float kw[2] = {temps[k], 0.f};
        const double beta = 1. / (double)temps[k];
        for (uint64_t round = 0; round < rounds_per_step; ++round) {
            if (r.mh_sweeps) {
                if (int rc = bisbm_anneal(h, BISBM_SCHED_CONSTANT, kw, (uint64_t)r.mh_sweeps * h->n, kNoStop, rate.data())) return rc;
                for (uint32_t c = 0; c < C; ++c) acc[c] += rate[c];
                ms += h->last_kernel_ms;
                updates += h->last_updates;
            }
            if (r.heatbath_sweeps)
                if (int rc = bisbm_heatbath_run(h, r.heatbath_sweeps, beta, 0, nullptr, nullptr)) return rc;
            if (r.reshuffles)
                if (int rc = bisbm_reshuffle_run(h, r.reshuffles, r.reshuffle_scans, beta, nullptr)) return rc;
        }
    }
    if (rounds_per_step && r.mh_sweeps) h->last_kernel_ms = ms, h->last_updates = updates;  // (the run's MH sweeps as one call)
    if (acc_rate_out)  // accepted MH steps / MH steps of the run: every round runs the same number of sweeps
        for (uint32_t c = 0; c < C; ++c)
            acc_rate_out[c] = rounds_per_step && r.mh_sweeps ? acc[c] / ((double)(n_temps - 1) * (double)rounds_per_step) : 0.;
    return BISBM_OK;
}

}  // extern "C"
