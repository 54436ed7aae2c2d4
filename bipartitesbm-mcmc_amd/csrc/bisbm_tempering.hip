// bisbm_tempering.hip -- replica exchange (parallel tempering) across the chains of a handle (no reference counterpart: the
// reference runs one chain).  The chains form ensembles of L consecutive global ids; every chain of an ensemble runs the
// constant-temperature chain at its rung's temperature (the sweep kernels read it per chain, SweepParams::T_chain), and every
// `exchange_every` sweeps neighbouring rungs of every ensemble propose to swap temperatures -- one lane per (ensemble, pair) of
// the exchange kernel below, on the device, with no host round trip per round.  include/bisbm.h states the definition.
#include "bisbm_engine.hpp"

using namespace bisbm;

namespace {

// What one exchange round of one engine reads and writes.  The description length of chain c is rebuilt from the block-state
// part the entropy kernel left in part[c] and the terms of entropy_terms, added in bisbm_entropy's order: the same double.
struct ExchangeParams {
    const double* part;  // [chain] block-state part of the description length
    double terms[8];     // entropy_terms
    uint32_t n_ens, L, pairs;
    uint32_t first_gid;  // global id of the engine's first chain (a multiple of L)
    uint64_t seed, round;
    const float* ladder;
    float* T;                    // [chain] temperature of the chain's rung
    uint32_t* rung;              // [chain] rung of the chain
    uint32_t* at;                // [ensemble][L] chain on every rung
    unsigned long long* stats;   // [2][L - 1] attempted, accepted
    const double* phi;           // [chain] block fields: Phi of every chain, the swap test is on E = S + Phi; NULL: no fields
};

__device__ __forceinline__ double description_length(const ExchangeParams& p, uint32_t c) {
    double s = p.terms[0];
    s += p.part[c];
    for (int i = 1; i < 8; ++i) s += p.terms[i];
    return s;
}

// E of chain c: the description length, under block fields plus Phi (one add; without fields the description length's own bits)
__device__ __forceinline__ double chain_energy(const ExchangeParams& p, uint32_t c) {
    const double s = description_length(p, c);
    return p.phi ? s + p.phi[c] : s;
}

// One lane per (ensemble, lower rung i of this round's parity).  The pairs of a round are disjoint, so every lane owns the
// entries it swaps.
__global__ __launch_bounds__(256) void tempering_exchange_kernel(ExchangeParams p) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.n_ens * p.pairs) return;
    const uint32_t g = t / p.pairs;
    const uint32_t i = (uint32_t)(p.round & 1u) + 2u * (t % p.pairs);  // i + 1 < L by the choice of `pairs`
    uint32_t* at = p.at + (size_t)g * p.L;
    const uint32_t a = at[i], b = at[i + 1];
    const double delta = (1.0 / (double)p.ladder[i] - 1.0 / (double)p.ladder[i + 1]) * (chain_energy(p, a) - chain_energy(p, b));
    const U4 U = phx_draw(p.seed, p.first_gid + g * p.L, PHX_EXCHANGE, p.round * p.L + i);
    const bool accept = delta >= 0. || u53(U.x, U.y) < exp(delta);
    atomicAdd(&p.stats[i], 1ull);
    if (accept) {
        atomicAdd(&p.stats[p.L - 1 + i], 1ull);
        at[i] = b, at[i + 1] = a;
        p.rung[a] = i + 1, p.rung[b] = i;
        p.T[a] = p.ladder[i + 1], p.T[b] = p.ladder[i];
    }
}

// The per-rung tally of a round (bisbm_tempering_rung_stats): what the kernel that has just run left per chain is added to the
// row of the rung the chain holds -- before the round's exchange moves it.  which = 0: the MH segment (ChainScalars::last_sweeps
// * n steps, last_accepted), 1: heat-bath sweeps (the same two scalars: visits, moves), 2: pair reshuffles (`moves` proposed,
// accepted[c]).  One lane per chain, integer atomics that return nothing.
__global__ __launch_bounds__(256) void tempering_tally_kernel(const ChainScalars* scalars, const unsigned long long* accepted, const uint32_t* rung,
                                                              uint32_t n_chains, uint32_t which, unsigned long long n, unsigned long long moves,
                                                              unsigned long long* stats) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chains) return;
    unsigned long long* row = stats + (size_t)rung[c] * 6u + 2u * which;
    if (which < 2u) {
        atomicAdd(&row[0], (unsigned long long)scalars[c].last_sweeps * n);
        atomicAdd(&row[1], (unsigned long long)scalars[c].last_accepted);
    } else {
        atomicAdd(&row[0], moves);
        atomicAdd(&row[1], accepted[c]);
    }
}

int tally(bisbm_engine* e, uint32_t which, uint64_t moves) {
    hipLaunchKernelGGL(tempering_tally_kernel, dim3((e->n_chains + 255) / 256), dim3(256), 0, e->stream, e->d_scalars, e->reshuffle.d_accepted.get(),
                       e->temper.d_rung.get(), e->n_chains, which, (unsigned long long)e->n, (unsigned long long)moves, e->temper.d_rung_stats.get());
    HIPCHK(e, hipGetLastError());
    return BISBM_OK;
}

constexpr uint64_t kNoStop = 1ull << 60;  // steps_await of every segment: no early stop (as BlockModel.run_sweeps)

int mixed_shapes(bisbm_engine* h) {
    if (any_grouped(h))
        return fail(h, BISBM_ERR_STATE, "the chains of this handle are grouped by shape (a one-argument bisbm_agg_merge_total left different block counts): replica exchange needs one common shape");
    return BISBM_OK;
}

// rungs, temperatures, statistics of a kernel-running engine: chain c on rung c mod L
int setup_leaf(bisbm_engine* e, uint32_t L, const float* ladder) {
    TemperState& t = e->temper;
    HIPCHK(e, hipSetDevice(e->device));
    const uint32_t C = e->n_chains;
    RESERVE(e, t.d_T, C);
    RESERVE(e, t.d_rung, C);
    RESERVE(e, t.d_at, C);
    RESERVE(e, t.d_ladder, L);
    RESERVE(e, t.d_stats, 2 * (size_t)L);
    RESERVE(e, t.d_beta, L);
    RESERVE(e, t.d_rung_stats, 6 * (size_t)L);
    std::vector<double> beta(L);
    for (uint32_t i = 0; i < L; ++i) beta[i] = 1.0 / (double)ladder[i];  // (the definition of a rung's beta: this host quotient)
    std::vector<float> T(C);
    std::vector<uint32_t> rung(C), at(C);
    for (uint32_t c = 0; c < C; ++c) T[c] = ladder[c % L], rung[c] = c % L, at[c] = c;
    HIPCHK(e, hipMemcpyAsync(t.d_T.get(), T.data(), sizeof(float) * C, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(t.d_rung.get(), rung.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(t.d_at.get(), at.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(t.d_ladder.get(), ladder, sizeof(float) * L, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemsetAsync(t.d_stats.get(), 0, sizeof(unsigned long long) * 2 * L, e->stream));
    HIPCHK(e, hipMemcpyAsync(t.d_beta.get(), beta.data(), sizeof(double) * L, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemsetAsync(t.d_rung_stats.get(), 0, sizeof(unsigned long long) * 6 * L, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    t.L = L;
    t.ladder.assign(ladder, ladder + L);
    t.round = 0;
    return BISBM_OK;
}

// one exchange round of a kernel-running engine, on its stream
int exchange_round(bisbm_engine* e) {
    TemperState& t = e->temper;
    // the block-state part of every chain's description length: the sweep call just before left it in d_ent_prev when it
    // advanced the running sum of dS that way (bisbm_anneal); otherwise the entropy kernel runs
    const double* part = e->d_ent_prev;
    if (!e->ent_prev_valid) {
        if (int rc = launch_block_entropy(e, e->d_tmp_f64)) return rc;
        part = e->d_tmp_f64;
    }
    ExchangeParams p{};
    p.part = part;
    entropy_terms(e, p.terms);
    p.L = t.L;
    p.n_ens = e->n_chains / t.L;
    p.pairs = (t.L - (uint32_t)(t.round & 1u)) / 2u;
    p.first_gid = e->first_chain_id;
    p.seed = e->seed;
    p.round = t.round;
    p.ladder = t.d_ladder.get();
    p.T = t.d_T.get();
    p.rung = t.d_rung.get();
    p.at = t.d_at.get();
    p.stats = t.d_stats.get();
    if (e->fields.n_classes) {  // (block fields: the swap test is on E = S + Phi)
        if (int rc = fields_energy_device(e)) return rc;
        p.phi = e->fields.d_phi.get();
    }
    const uint32_t lanes = p.n_ens * p.pairs;
    if (lanes) {
        hipLaunchKernelGGL(tempering_exchange_kernel, dim3((lanes + 255) / 256), dim3(256), 0, e->stream, p);
        HIPCHK(e, hipGetLastError());
    }
    ++t.round;
    return BISBM_OK;
}

int run_leaf(bisbm_engine* e, uint64_t sweeps, uint32_t every, double* acc_rate_out) {
    TemperState& t = e->temper;
    HIPCHK(e, hipSetDevice(e->device));
    const float kw[2] = {t.ladder[0], 0.f};  // (the host's view of the call; every chain's own T comes from T_chain)
    const uint64_t blocks = every ? sweeps / every : 0, rest = sweeps - blocks * every;
    std::vector<double> rate(e->n_chains), acc(e->n_chains, 0.);
    double ms = 0;
    uint64_t updates = 0;
    auto segment = [&](uint64_t k) -> int {
        if (int rc = anneal_engine(e, BISBM_SCHED_CONSTANT, kw, k * e->n, kNoStop, rate.data(), t.d_T.get())) return rc;
        for (uint32_t c = 0; c < e->n_chains; ++c) acc[c] += rate[c] * (double)k;  // (rate: accepted / steps of the segment)
        ms += e->last_kernel_ms;
        updates += e->last_updates;
        return tally(e, 0, 0);
    };
    for (uint64_t b = 0; b < blocks; ++b) {
        if (int rc = segment(every)) return rc;
        if (int rc = exchange_round(e)) return rc;
    }
    if (rest)
        if (int rc = segment(rest)) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->last_kernel_ms = ms;
    e->last_updates = updates;
    if (acc_rate_out)
        for (uint32_t c = 0; c < e->n_chains; ++c) acc_rate_out[c] = sweeps ? acc[c] / (double)sweeps : 0.;
    return BISBM_OK;
}

// `rounds` rounds of the recipe on a kernel-running engine: the MH segment of run_leaf, heat-bath sweeps and pair reshuffles at
// every chain's own beta, the tally, the exchange.  Nothing per chain travels to the host between the rounds beyond what the MH
// segment itself reads (bisbm_anneal's scalars); the reshuffle records of the last round are read back once, at the end.
int rounds_leaf(bisbm_engine* e, uint64_t rounds, const bisbm_round_recipe& r, bool exchange) {
    TemperState& t = e->temper;
    HIPCHK(e, hipSetDevice(e->device));
    const float kw[2] = {t.ladder[0], 0.f};
    double ms = 0;
    uint64_t updates = 0;
    for (uint64_t k = 0; k < rounds; ++k) {
        if (r.mh_sweeps) {
            if (int rc = anneal_engine(e, BISBM_SCHED_CONSTANT, kw, (uint64_t)r.mh_sweeps * e->n, kNoStop, nullptr, t.d_T.get())) return rc;
            ms += e->last_kernel_ms;
            updates += e->last_updates;
            if (int rc = tally(e, 0, 0)) return rc;
        }
        if (r.heatbath_sweeps) {
            if (int rc = heatbath_engine(e, r.heatbath_sweeps, 0., 0, true, false)) return rc;
            if (int rc = tally(e, 1, 0)) return rc;
        }
        if (r.reshuffles) {
            if (int rc = reshuffle_engine(e, r.reshuffles, r.reshuffle_scans, 0., true, false)) return rc;
            if (int rc = tally(e, 2, r.reshuffles)) return rc;
        }
        if (exchange)
            if (int rc = exchange_round(e)) return rc;
    }
    if (r.reshuffles && rounds) {
        if (int rc = reshuffle_read_back(e)) return rc;
    } else {
        HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    e->last_kernel_ms = ms;
    e->last_updates = updates;
    return BISBM_OK;
}

}  // namespace

extern "C" {

int bisbm_tempering_set(bisbm_handle h, uint32_t L, const float* ladder) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (L == 0) {  // off: every call behaves as without tempering again
        h->temper.L = 0;
        h->temper.ladder.clear();
        h->temper.round = 0;
        for (bisbm_engine* d : h->devs) d->temper.L = 0, d->temper.ladder.clear(), d->temper.round = 0;
        return BISBM_OK;
    }
    if (L < 2) return fail(h, BISBM_ERR_INVALID_ARG, "a temperature ladder needs at least 2 rungs (L = %u)", L);
    if (!ladder) return fail(h, BISBM_ERR_INVALID_ARG, "ladder is NULL");
    for (uint32_t i = 0; i < L; ++i) {
        if (!std::isfinite(ladder[i]) || !(ladder[i] > 0.f))
            return fail(h, BISBM_ERR_INVALID_ARG, "ladder[%u] = %g: every temperature must be finite and > 0", i, (double)ladder[i]);
        if (i && ladder[i] < ladder[i - 1])
            return fail(h, BISBM_ERR_INVALID_ARG, "ladder[%u] = %g < ladder[%u] = %g: the ladder must be non-decreasing", i, (double)ladder[i], i - 1,
                        (double)ladder[i - 1]);
    }
    if (h->rng_mode == BISBM_RNG_MT19937_COMPAT)
        return fail(h, BISBM_ERR_UNSUPPORTED, "replica exchange runs in Philox mode only (mt19937-compat mode is the reference's verification path)");
    if (int rc = mixed_shapes(h)) return rc;
    if (h->modes.n_modes && !h->modes.anchored)  // (anchored modes assign the cold chains afresh at every sample)
        return fail(h, BISBM_ERR_STATE, "mode-resolved marginals are set (bisbm_marginals_set_modes): chains that trade temperatures have no mode of their own; turn the modes off first");
    if (h->first_chain_id % L)
        return fail(h, BISBM_ERR_INVALID_ARG, "the first global chain id %u is not a multiple of L = %u: ensembles are global ids [g L, (g + 1) L)",
                    h->first_chain_id, L);
    for (bisbm_engine* e : device_entries(h))
        if (e->n_chains % L)
            return fail(h, BISBM_ERR_INVALID_ARG, "%s holds %u chains, not a multiple of L = %u: an ensemble may not straddle device entries",
                        h->devs.empty() ? "the handle" : ("the entry of device " + std::to_string(e->device)).c_str(), e->n_chains, L);
    h->temper.L = 0;
    for (bisbm_engine* e : device_entries(h)) {
        if (int rc = setup_leaf(e, L, ladder)) {
            if (e != h) h->err = e->err;
            for (bisbm_engine* d : h->devs) d->temper.L = 0;
            return rc;
        }
    }
    h->temper.L = L;
    h->temper.ladder.assign(ladder, ladder + L);
    h->temper.round = 0;
    return BISBM_OK;
}

int bisbm_tempering_run(bisbm_handle h, uint64_t sweeps, uint32_t exchange_every, double* acc_rate_out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->temper.L) return fail(h, BISBM_ERR_STATE, "replica exchange is off: call bisbm_tempering_set first");
    if (int rc = mixed_shapes(h)) return rc;
    if (h->devs.empty()) {
        const int rc = run_leaf(h, sweeps, exchange_every, acc_rate_out);
        return rc;
    }
    const int rc = on_devices(h, [&](bisbm_engine* d, size_t i) {
        return run_leaf(d, sweeps, exchange_every, acc_rate_out ? acc_rate_out + h->dev_first[i] : nullptr);
    });
    h->last_kernel_ms = 0;
    h->last_updates = 0;
    for (bisbm_engine* d : h->devs) {  // (as multi_anneal: the devices run side by side)
        h->last_kernel_ms = std::max(h->last_kernel_ms, d->last_kernel_ms);
        h->last_updates += d->last_updates;
        h->last_pass_steps = std::max(d == h->devs[0] ? 0u : h->last_pass_steps, d->last_pass_steps);
        if (d == h->devs[0]) std::copy(d->last_eta_plan, d->last_eta_plan + 4, h->last_eta_plan), h->last_route = d->last_route;
    }
    h->temper.round = h->devs[0]->temper.round;
    return rc;
}

int bisbm_tempering_run_rounds(bisbm_handle h, uint64_t rounds, const bisbm_round_recipe* recipe, int exchange) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->temper.L) return fail(h, BISBM_ERR_STATE, "replica exchange is off: call bisbm_tempering_set first");
    if (!recipe) return fail(h, BISBM_ERR_INVALID_ARG, "recipe is NULL");
    if (int rc = mixed_shapes(h)) return rc;
    const bisbm_round_recipe r = *recipe;
    if (!r.mh_sweeps && !r.heatbath_sweeps && !r.reshuffles)
        return fail(h, BISBM_ERR_INVALID_ARG, "the recipe runs nothing: mh_sweeps, heatbath_sweeps and reshuffles are all 0");
    if ((r.heatbath_sweeps || r.reshuffles) && any_wide(h))
        return fail(h, BISBM_ERR_UNSUPPORTED, "heat-bath sweeps and pair reshuffles serve byte labels only (at most 256 blocks): this recipe (heatbath_sweeps = %u, reshuffles = %u) needs them; merge the blocks down first",
                    r.heatbath_sweeps, r.reshuffles);
    for (bisbm_engine* e : leaves(h))
        if (!e->state_ready) return fail(h, BISBM_ERR_STATE, "call bisbm_init or bisbm_shuffle before bisbm_tempering_run_rounds");
    if (r.reshuffles)
        if (int rc = reshuffle_check_scans(h, r.reshuffle_scans)) return rc;
    DeviceGuard keep;
    if (h->devs.empty()) return rounds_leaf(h, rounds, r, exchange != 0);
    const int rc = on_devices(h, [&](bisbm_engine* d, size_t) { return rounds_leaf(d, rounds, r, exchange != 0); });
    h->last_kernel_ms = 0;
    h->last_updates = 0;
    for (bisbm_engine* d : h->devs) {  // (as bisbm_tempering_run)
        h->last_kernel_ms = std::max(h->last_kernel_ms, d->last_kernel_ms);
        h->last_updates += d->last_updates;
        h->last_pass_steps = std::max(d == h->devs[0] ? 0u : h->last_pass_steps, d->last_pass_steps);
        if (d == h->devs[0]) std::copy(d->last_eta_plan, d->last_eta_plan + 4, h->last_eta_plan), h->last_route = d->last_route;
    }
    h->temper.round = h->devs[0]->temper.round;
    return rc;
}

int bisbm_tempering_rung_stats(bisbm_handle h, uint64_t* out) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->temper.L) return fail(h, BISBM_ERR_STATE, "replica exchange is off");
    if (!out) return fail(h, BISBM_ERR_INVALID_ARG, "out is NULL");
    const size_t cells = 6 * (size_t)h->temper.L;
    std::vector<uint64_t> part(cells);
    std::fill(out, out + cells, 0);
    DeviceGuard keep;
    for (bisbm_engine* e : device_entries(h)) {
        HIPCHK(h, hipSetDevice(e->device));
        HIPCHK(h, hipStreamSynchronize(e->stream));
        HIPCHK(h, hipMemcpy(part.data(), e->temper.d_rung_stats.get(), sizeof(uint64_t) * cells, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cells; ++i) out[i] += part[i];
    }
    return BISBM_OK;
}

int bisbm_tempering_get(bisbm_handle h, uint32_t* rung_of_chain, float* T_of_chain) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->temper.L) return fail(h, BISBM_ERR_STATE, "replica exchange is off");
    uint32_t first = 0;
    for (bisbm_engine* e : device_entries(h)) {
        HIPCHK(h, hipSetDevice(e->device));
        HIPCHK(h, hipStreamSynchronize(e->stream));
        if (rung_of_chain)
            HIPCHK(h, hipMemcpy(rung_of_chain + first, e->temper.d_rung.get(), sizeof(uint32_t) * e->n_chains, hipMemcpyDeviceToHost));
        if (T_of_chain) HIPCHK(h, hipMemcpy(T_of_chain + first, e->temper.d_T.get(), sizeof(float) * e->n_chains, hipMemcpyDeviceToHost));
        first += e->n_chains;
    }
    return BISBM_OK;
}

int bisbm_tempering_stats(bisbm_handle h, uint64_t* attempted, uint64_t* accepted, uint64_t* rounds) {
    if (!h) return BISBM_ERR_INVALID_ARG;
    if (!h->temper.L) return fail(h, BISBM_ERR_STATE, "replica exchange is off");
    const uint32_t P = h->temper.L - 1;
    std::vector<uint64_t> sum(2 * (size_t)P, 0), part(2 * (size_t)P);
    for (bisbm_engine* e : device_entries(h)) {
        HIPCHK(h, hipSetDevice(e->device));
        HIPCHK(h, hipStreamSynchronize(e->stream));
        HIPCHK(h, hipMemcpy(part.data(), e->temper.d_stats.get(), sizeof(uint64_t) * 2 * P, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < part.size(); ++i) sum[i] += part[i];
    }
    for (uint32_t i = 0; i < P; ++i) {
        if (attempted) attempted[i] = sum[i];
        if (accepted) accepted[i] = sum[P + i];
    }
    if (rounds) *rounds = h->temper.round;
    return BISBM_OK;
}

}  // extern "C"
