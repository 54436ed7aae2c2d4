/*
 * bisbm.h -- C ABI of the MI355X-native Metropolis-Hastings sweep engine for the degree-corrected
 * bipartite SBM (libbisbm_hip.so).
 *
 * The reference (junipertcy/bipartiteSBM-MCMC) has no FFI; its CLI (src/mcmc_main.cc) drives the
 * hot path through two C++ classes.  Every entry point below stands behind one of those member
 * functions, cited as <file>:<line> relative to /root/reference/src.  Plain pointers and sizes only:
 * no C++ types, no torch types, no exceptions across the boundary.  Host buffers are caller-owned;
 * device memory is library-owned.  One host thread per handle.
 *
 * All functions return BISBM_OK (0) or a bisbm_status error code; bisbm_last_error() gives the text.
 * There is no CPU fallback: without a HIP device bisbm_create fails with BISBM_ERR_NO_DEVICE.
 */
#ifndef BISBM_H
#define BISBM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: bisbm_get_ka_kb_chain; KA + KB above 256 (wide mode); handles whose chains differ in shape.
 * 3: bisbm_check_shape; several devices behind one handle (bisbm_create_multi); bisbm_last_pass_steps; later additions: label
 *    alignment (bisbm_marginals_set_alignment ...), replica exchange (bisbm_tempering_*), pair scores (bisbm_pair_scores_*),
 *    partition distances and modes (bisbm_partition_*), mode-resolved marginals (bisbm_marginals_set_modes ...,
 *    bisbm_marginals_get_mode, bisbm_marginals_map_mode), distances to reference partitions (bisbm_partition_distances_to),
 *    anchored modes (bisbm_marginals_set_mode_anchors, bisbm_marginals_get_mode_assignment), query scores
 *    (bisbm_query_scores_*), co-assignment (bisbm_coassign_*), fold-in queries (bisbm_foldin_*), population annealing
 *    (bisbm_population_*), node conditionals (bisbm_conditionals_*), heat-bath sweeps and greedy polishing
 *    (bisbm_heatbath_run), pair reshuffles (bisbm_reshuffle_*, bisbm_debug_exp), chain traces (bisbm_trace_*), round recipes
 *    (bisbm_tempering_run_rounds, bisbm_tempering_rung_stats, bisbm_rounds_population_run), held conditionals and the least
 *    settled queries (bisbm_held_conditionals_*, bisbm_least_settled_topk, bisbm_debug_log), the eta plan of the last launch
 *    (bisbm_last_eta_plan), the route of the last launch (bisbm_last_sweep_route), edge probabilities
 *    (bisbm_edge_probs_*), edge queries (bisbm_edge_queries_*).  Additions only. */
#define BISBM_ABI_VERSION 3

typedef struct bisbm_engine *bisbm_handle;

typedef enum bisbm_status {
    BISBM_OK = 0,
    BISBM_ERR_INVALID_ARG = 1,   /* null pointer, size mismatch, label out of range ... */
    BISBM_ERR_NOT_BIPARTITE = 2, /* an edge joins two nodes of one type, or an id >= n */
    BISBM_ERR_UNSUPPORTED = 3,   /* more blocks than wide mode serves (bisbm_check_shape), more than 2^32-1 adjacency entries ... */
    BISBM_ERR_NO_DEVICE = 4,     /* no HIP device / bad ordinal: the engine has no CPU path */
    BISBM_ERR_HIP = 5,           /* a HIP runtime call failed */
    BISBM_ERR_STATE = 6          /* call order (e.g. anneal before init/shuffle) */
} bisbm_status;

/* Random-number definition of the chain.
 * BISBM_RNG_PHILOX         production: Philox4x32-10 counters keyed by (seed, global chain id),
 *                          Feistel visit order per sweep, integer inverse-CDF proposal draw,
 *                          butterfly FP64 sums (DESIGN.md "Philox-mode definition").
 * BISBM_RNG_MT19937_COMPAT the reference's own draw sequence: std::mt19937 `engine`
 *                          (mcmc_main.cc:242) + the hidden `gen` (blockmodel.hh:17-18),
 *                          libstdc++-11 shuffle / generate_canonical / discrete_distribution,
 *                          serial FP64 sums in source order.  Chain c uses engine seed `seed + c`
 *                          and gen seed `gen_seed + c` (c = global chain id).
 */
typedef enum bisbm_rng { BISBM_RNG_PHILOX = 0, BISBM_RNG_MT19937_COMPAT = 1 } bisbm_rng;

/* metropolis_hasting.cc:10-37 */
typedef enum bisbm_schedule {
    BISBM_SCHED_EXPONENTIAL = 0,
    BISBM_SCHED_LINEAR = 1,
    BISBM_SCHED_LOGARITHMIC = 2,
    BISBM_SCHED_CONSTANT = 3,
    BISBM_SCHED_ABRUPT_COOL = 4
} bisbm_schedule;

#define BISBM_ALL_CHAINS (-1)

/* Replaces blockmodel_t::blockmodel_t (blockmodel.hh:22-23, blockmodel.cc:15-75; call sites
 * mcmc_main.cc:352,420,453).  The graph is CSR of the reference's adj_list_t: row v holds the
 * neighbours of v in edge-file order, duplicates kept (graph_utilities.cc:36-49).  Nodes
 * [0,na) are type a, [na,na+nb) type b (mcmc_main.cc:121-130).  Blocks [0,ka) are type a,
 * [ka,ka+kb) type b.  `n_chains` independent chains are created on HIP device `device`; chain i
 * of this handle has global id first_chain_id + i (the id keys its random stream, so results do
 * not depend on how chains are sharded over GPUs).  Builds the lgamma / log_q tables
 * (support/cache.cc:64-91, support/int_part.cc:34-51) on the host and uploads them.
 * No more blocks than nodes of a type, and a shape bisbm_check_shape accepts.  With ka + kb > 256 (the reference's --merge driver starts from one
 * block per node, mcmc_main.cc:350-353) the handle runs in WIDE MODE: two-byte labels, the block matrix read and updated in
 * HBM, the generic kernel (slow per step; meant for the greedy sweeps between merge stages); bisbm_agg_merge switches it to
 * byte labels and the ordinary kernels as soon as it leaves ka + kb <= 256; a split (negative diff) that takes a handle past
 * 256 blocks switches it to wide mode, and splits are served while wide. */
int bisbm_create(bisbm_handle *out, uint64_t n, uint64_t na, uint64_t nb, const uint64_t *rowptr,
                 const uint32_t *col, uint32_t ka, uint32_t kb, double epsilon, uint32_t n_chains,
                 uint32_t first_chain_id, int device, int rng_mode, uint64_t seed,
                 uint64_t gen_seed);

/* The same for chains spread over several devices of one node (no reference counterpart: the reference is one chain in one
 * process; BASELINE north_star / SURVEY 8e: "chains shard trivially across the 8 GPUs of one node").  The n_chains chains are
 * split into contiguous ranges, one per entry of devices[] (the first n_chains % n_devices ranges one chain longer); graph
 * and tables are replicated per device; chain i keeps the global id first_chain_id + i, so every result equals what ONE
 * device with all the chains gives.  Every other call works on the returned handle as on a single-device one (all-chain calls
 * run the devices side by side, one host thread and one stream per device; there is no exchange during sweeps) except:
 * bisbm_set_stream (refused) and bisbm_marginals_accumulate with a caller-owned buffer (refused: each device accumulates into
 * its own; bisbm_marginals_map pools them on the devices, bisbm_marginals_get on the host).  A device may be listed more than
 * once (rehearsal on a one-GPU box). */
int bisbm_create_multi(bisbm_handle *out, uint64_t n, uint64_t na, uint64_t nb, const uint64_t *rowptr,
                       const uint32_t *col, uint32_t ka, uint32_t kb, double epsilon, uint32_t n_chains,
                       uint32_t first_chain_id, const int *devices, int n_devices, int rng_mode,
                       uint64_t seed, uint64_t gen_seed);

/* Devices behind a handle: their number, their ordinals and the first chain of each (arrays of *n_devices entries; any
 * pointer may be NULL).  1 / {device} / {0} for a bisbm_create handle. */
int bisbm_device_count(bisbm_handle h, int *n_devices, int *devices, uint32_t *first_chain);

int bisbm_destroy(bisbm_handle h);

/* Whether a handle of ka + kb blocks can be served, without creating one (no reference counterpart: blockmodel_t has no
 * block limit; the CLI's --merge driver asks before it starts from one block per node, mcmc_main.cc:350-353).
 * Up to 256 blocks: always.  Above (wide mode): labels are two bytes (ka + kb <= 65535) and a chain's m_r, n_r and k_v histogram
 * stay in LDS, which ends at about 14 000 blocks (even split: 14 700 in Philox mode, 13 700 in mt19937-compat mode; 10 bytes
 * per block plus 4 for the larger type, 160 KiB per CU).  BISBM_ERR_UNSUPPORTED with the numbers in bisbm_last_error(NULL). */
int bisbm_check_shape(uint32_t ka, uint32_t kb, int rng_mode);

/* Initial partition: the `memberships` constructor argument (blockmodel.cc:23), n labels in
 * [0, ka+kb).  chain = BISBM_ALL_CHAINS copies the vector to every chain. */
int bisbm_set_memberships(bisbm_handle h, int64_t chain, const uint32_t *labels);

/* blockmodel_t::init_bisbm (blockmodel.cc:682-688): rebuild n_r, m, m_r, eta from the labels. */
int bisbm_init(bisbm_handle h);

/* blockmodel_t::shuffle_bisbm (blockmodel.cc:672-680): shuffle the type-a labels, then the
 * type-b labels (block sizes preserved), then rebuild the block state. */
int bisbm_shuffle(bisbm_handle h);

/* metropolis_hasting::anneal (metropolis_hasting.hh:48-53, metropolis_hasting.cc:64-101) for
 * every chain (BISBM_ERR_STATE while replica exchange is on: bisbm_tempering_run): duration_steps / n sweeps of n node updates (step :42-62, transition_ratio
 * :103-192, single_vertex_change blockmodel.cc:613-637, apply_mcmc_moves blockmodel.cc:461-503),
 * early stop per chain when the count of T<1 steps since the last new minimum reaches steps_await.
 * kwargs are the two float cooling parameters (mcmc_main.cc:49).  acc_rate_out[n_chains] receives
 * anneal's return value per chain (may be NULL). */
int bisbm_anneal(bisbm_handle h, int schedule, const float kwargs[2], uint64_t duration_steps,
                 uint64_t steps_await, double *acc_rate_out);

/* blockmodel_t::get_memberships (blockmodel.cc:87) for one chain: n labels. */
int bisbm_get_memberships(bisbm_handle h, uint32_t chain, uint32_t *labels_out);

/* get_m / get_m_r / get_n_r / get_eta_rk_ (blockmodel.cc:93-99) for one chain.
 * m is the reference's full symmetric K*K matrix (row-major), eta is K*(max_degree+1).
 * Any output pointer may be NULL. */
int bisbm_get_block_state(bisbm_handle h, uint32_t chain, int32_t *m, int32_t *m_r, int32_t *n_r,
                          uint32_t *eta);

/* blockmodel_t::get_entropy (blockmodel.cc:91): running sum of accepted dS, per chain.  Launches that keep anneal()'s
 * early-stop bookkeeping (below T = 1 with steps_await in reach), the generic kernel and mt19937-compat mode add it up step by
 * step; a production launch that cannot stop early advances it per bisbm_anneal call by the change of the block-state part of
 * the description length instead -- the same quantity to <= 1e-12 of the description length (BISBM_KEEP_SUM=1: step by step
 * everywhere). */
int bisbm_get_cum_dS(bisbm_handle h, double *out);

/* blockmodel_t::entropy (blockmodel.cc:753-787): full description length, per chain.  The
 * reference's log(na*nb) table growth (cache.hh:47-57) that aborts on large graphs
 * is replaced by a direct log(). */
int bisbm_entropy(bisbm_handle h, double *out);

/* Bookkeeping of the last bisbm_anneal per chain: accepted steps and sweeps executed
 * (metropolis_hasting.cc:72,97,100).  Either pointer may be NULL. */
int bisbm_get_last_counts(bisbm_handle h, uint64_t *accepted, uint64_t *sweeps);

/* Marginal accumulation the README describes for "marginalize" (README.md:49-53; the code at
 * mcmc_main.cc:61-65 parses -b/-f and never uses them): add one sample of every chain's labels
 * to counts[n][kmax], kmax = max(ka,kb), column = block index within the node's type.
 * device_counts is a DEVICE pointer to n*kmax uint32 owned by the caller (e.g. a torch tensor
 * that RCCL then reduces across ranks); NULL uses an internal buffer read by bisbm_marginals_get.
 * Stream contract: the histogram kernel runs on the handle's own non-blocking stream and adds with
 * plain read-modify-writes, so everything the caller has in flight on device_counts (its zero fill,
 * its own kernels) must have COMPLETED before the call (synchronise the stream that wrote it); the
 * call returns after its kernel has finished, so the caller may read the buffer right away.
 * With the alignment on (bisbm_marginals_set_alignment) every chain's labels are counted through that chain's permutation onto
 * the reference partition, into the internal buffer and into a caller's device_counts alike; without it (the default) the raw
 * labels are counted.  A block label means something only inside one chain, so a histogram of more than one chain is a
 * marginal only when aligned.  bisbm_marginals_reset empties the histogram and drops a library-chosen reference (the
 * alignment mode and a caller's reference stay).
 * After a merge or split (bisbm_agg_merge, bisbm_split_merge_run) the caller resets.  Where it does not: while the chains have
 * different block counts accumulate, get and map are BISBM_ERR_STATE and nothing changes.  The internal histogram of a plain
 * handle is dropped when its chains are grouped by shape (bisbm_agg_merge_total, the first accepted split or merge).  Once the
 * chains share (ka, kb) again, get and map are BISBM_ERR_STATE while there is no histogram of these block counts -- none at
 * all, or one started for OTHER counts, either of them, also where max(ka, kb) and with it the row length is the same: 3 + 3
 * and 3 + 2 blocks share no numbering --, and the next accumulate into the internal buffer, raw or aligned, starts afresh and
 * holds that sample alone (the block sums start afresh with it, a library-chosen reference is taken afresh). */
int bisbm_marginals_accumulate(bisbm_handle h, uint32_t *device_counts);
int bisbm_marginals_reset(bisbm_handle h);
int bisbm_marginals_get(bisbm_handle h, uint32_t *counts_out /* n*kmax, host */);

/* Label alignment before pooling (no reference counterpart: one chain needs none).  Chains start from independent shuffles and
 * each settles on its own numbering of the blocks, so before a sample is added every chain's blocks are matched to a REFERENCE
 * partition, per node type: C[r][s] = nodes of the type with the chain's label r and reference label s (the overlap table);
 * the permutation pi maximises sum_r C[r][pi(r)], found exactly by a shortest-augmenting-path assignment in int64 with cost
 * max(C) - C[r][s], rows inserted in order 0..K-1, and in every Dijkstra step the unvisited column of least reduced
 * distance, ties -> the lowest column (bisbm_align_assignment is the same solver on the host: both give the same permutation
 * for the same table).  A fresh permutation is computed at every aligned sample; the chains' own state (labels, block state,
 * random streams, sum dS) is never touched.
 * The reference: the caller's (bisbm_marginals_set_reference), or else -- taken at the first aligned sample after a reset --
 * the labels of the chain of the lowest description length (bisbm_entropy; ties -> the lowest global chain id), over every
 * device of the handle.
 * Refused: byte labels only (a wide handle, more than 256 blocks: BISBM_ERR_UNSUPPORTED at the accumulate); chains of different
 * shapes (BISBM_ERR_STATE, as the histogram itself); a caller's reference made for other block counts than the chains have
 * now, after a merge or split (BISBM_ERR_STATE at the next accumulate; a library-chosen one is taken afresh). */
#define BISBM_ALIGN_NONE 0      /* raw labels are pooled (the default) */
#define BISBM_ALIGN_REFERENCE 1 /* labels are counted through each chain's permutation onto the reference */

/* Sets the mode; it holds across resets.  BISBM_ERR_STATE when it would change while the internal histogram holds samples. */
int bisbm_marginals_set_alignment(bisbm_handle h, int mode);
/* A reference partition of the caller: n labels of the present block counts (type-b offset by ka); a label outside its node's
 * type range is BISBM_ERR_INVALID_ARG.  It stays until it is replaced or cleared.  NULL clears any reference: the next aligned
 * sample takes the lowest-description-length chain's labels. */
int bisbm_marginals_set_reference(bisbm_handle h, const uint32_t *labels);
/* The reference (n labels) and the chain it came from (-1: set by the caller); either pointer may be NULL.  BISBM_ERR_STATE
 * while there is none. */
int bisbm_marginals_get_reference(bisbm_handle h, uint32_t *labels_out, int64_t *chain_out);
/* One chain's permutation of the last aligned sample, in global-label form (perm_out[r] = the reference block chain label r is
 * counted as, ka + kb entries) and its overlap sum_r C[r][pi(r)] over both types; either pointer may be NULL.
 * BISBM_ERR_STATE before the chain's first aligned sample or when its block counts changed since. */
int bisbm_marginals_get_alignment(bisbm_handle h, uint32_t chain, uint32_t *perm_out, uint64_t *overlap_out);
/* The assignment solver of the alignment on the host, without a device: table is k x k (row-major, C[r][s]), perm_out[k]
 * receives pi(r) in 0..k-1, total_out (may be NULL) sum_r C[r][pi(r)]. */
int bisbm_align_assignment(uint32_t k, const uint32_t *table, uint32_t *perm_out, uint64_t *total_out);

/* Replica exchange (parallel tempering; no reference counterpart: the reference runs one chain at one temperature).
 * Ladder: L >= 2 float temperatures, finite, > 0, non-decreasing (float, like the kwargs of bisbm_anneal: a chain at rung T runs
 * bit-for-bit as bisbm_anneal(BISBM_SCHED_CONSTANT, {T, .}) would run it).  Ensemble g is the chains of global ids
 * [g L, (g + 1) L); at the start chain g L + i sits on rung i.  The chain count of the handle and of every device entry, and the
 * first global chain id, must be multiples of L (an ensemble never straddles a device or a rank: no collective), and all chains
 * one shape.  Every chain runs the constant-temperature chain at its rung's temperature, its Philox streams keyed by its own
 * global id as always, so its path is that of a one-chain run with a piecewise-constant T; there is no early stop.
 * Exchange round r (r counts from 0 at bisbm_tempering_set): S = every chain's full description length (bisbm_entropy's value,
 * f64); for every ensemble and every lower rung i with i = r (mod 2) and i + 1 < L, with a = the chain on rung i, b = the chain
 * on rung i + 1: delta = (1/T_i - 1/T_{i+1}) (S_a - S_b); U = Philox(seed, counter (r L + i, global id of the ensemble's first
 * chain, purpose 7 = exchange)), u = the 53-bit uniform of U's first two words (DESIGN.md "Philox-mode definition"); the two
 * chains swap rungs iff delta >= 0 or u < exp(delta).  Chain states never move.  Attempted / accepted exchanges are counted per
 * rung pair (L - 1 counters each, summed over ensembles and devices).
 * While tempering is on, bisbm_anneal is refused (BISBM_ERR_STATE) and bisbm_marginals_accumulate counts only the chains on rung
 * 0, raw or aligned; the library-chosen alignment reference is the lowest-description-length chain on rung 0. */

/* On with the ladder (L temperatures), or off with L = 0 (ladder may be NULL then).  Resets the rungs, the round counter and the
 * statistics.  Refused: a bad ladder or L that does not divide the chain counts (BISBM_ERR_INVALID_ARG), mt19937-compat mode
 * (BISBM_ERR_UNSUPPORTED), chains grouped by shape after bisbm_agg_merge_total (BISBM_ERR_STATE). */
int bisbm_tempering_set(bisbm_handle h, uint32_t L, const float *ladder);
/* `sweeps` sweeps of every chain; after each complete block of exchange_every sweeps one exchange round (0: no exchange).
 * acc_rate_out[n_chains] (may be NULL): accepted steps / steps of the call, per chain. */
int bisbm_tempering_run(bisbm_handle h, uint64_t sweeps, uint32_t exchange_every, double *acc_rate_out);
/* Rung and temperature of every chain (n_chains entries each; either pointer may be NULL). */
int bisbm_tempering_get(bisbm_handle h, uint32_t *rung_of_chain, float *T_of_chain);
/* attempted[L - 1] / accepted[L - 1] exchanges of rung pair (i, i + 1) and the rounds run since bisbm_tempering_set; any pointer
 * may be NULL. */
int bisbm_tempering_stats(bisbm_handle h, uint64_t *attempted, uint64_t *accepted, uint64_t *rounds);

/* Heat-bath sweeps and pair reshuffles inside replica exchange.  Under a round recipe every chain runs the two moves (defined
 * under "Heat-bath sweeps and greedy polishing" and "Pair reshuffles" below, unchanged: the same counters sweeps_total and
 * reshuffles_total, purposes 9 and 10, every stated order) at its own beta_c = 1.0 / (double)T_c, the correctly rounded f64
 * quotient of its rung's float temperature as the host computes it at bisbm_tempering_set.  Each of the three moves leaves
 * exp(-S / T_c) invariant for the chain it runs on, so does their sequence, and the exchange leaves the joint distribution
 * invariant.  Greedy polishing (beta = +inf) is not available per chain. */
typedef struct bisbm_round_recipe {
    uint32_t mh_sweeps;        /* MH sweeps per round, each chain at T_c (the segment of bisbm_tempering_run) */
    uint32_t heatbath_sweeps;  /* then heat-bath sweeps at beta_c (no early stop) */
    uint32_t reshuffles;       /* then pair reshuffles per chain at beta_c */
    uint32_t reshuffle_scans;  /* launch scans of every reshuffle */
} bisbm_round_recipe;
/* `rounds` rounds; a round runs, in this order: the MH sweeps, the heat-bath sweeps, the reshuffles, the per-rung tally
 * (bisbm_tempering_rung_stats) and, if `exchange` is not 0, one exchange round as defined above (the same Philox index
 * round * L + i, the same round counter and statistics).  So bisbm_tempering_run_rounds(R, {k, 0, 0, .}, 1) is
 * bisbm_tempering_run(R * k, k) bit for bit, and chain c is the chain a one-chain handle of its global id runs through
 * bisbm_anneal, bisbm_heatbath_run and bisbm_reshuffle_run at the temperatures chain c held.  Refused: replica exchange off and
 * chains grouped by shape (BISBM_ERR_STATE), a NULL recipe or one of all zeros (BISBM_ERR_INVALID_ARG), a recipe with heat-bath
 * sweeps or reshuffles on a wide handle (BISBM_ERR_UNSUPPORTED).  bisbm_heatbath_run and bisbm_reshuffle_run themselves stay
 * refused while replica exchange is on.  bisbm_reshuffle_get_last reports the last round's last move afterwards. */
int bisbm_tempering_run_rounds(bisbm_handle h, uint64_t rounds, const bisbm_round_recipe *recipe, int exchange);
/* out[L * 6]: per rung i, out[6 i + ...] = MH steps, MH steps accepted, heat-bath steps (sweeps * n), heat-bath moves,
 * reshuffles proposed, reshuffles accepted since bisbm_tempering_set, summed over ensembles and device entries.  What a chain
 * does in a round (or in a segment of bisbm_tempering_run, which feeds the MH columns) is added to the rung it held during it,
 * before that round's exchange -- on the device, with integer adds. */
int bisbm_tempering_rung_stats(bisbm_handle h, uint64_t *out /* L * 6 */);

/* Population annealing (Hukushima & Iba 2003, Machta 2010; no reference counterpart: the reference runs one chain).  The
 * population is all C chains of the handle, over every device of it, all at one temperature; between temperature steps it is
 * resampled by description length, and sweeps at the new temperature then decorrelate the copies.  One resampling step from
 * beta_from to beta_to, D = beta_to - beta_from >= 0 (all f64, in exactly this order of operations):
 *  1. S_c = the description length of chain c: the double bisbm_entropy returns.
 *  2. S_min = min_c S_c; w_c = exp(-D * (S_c - S_min)) with the host's exp; c_k = w_0 + ... + w_k added in ascending c;
 *     W = c_{C-1}.
 *  3. log_ratio = -D * S_min + log(W / C): the step's estimate of ln Z(beta_to) / Z(beta_from).
 *  4. Offspring counts by systematic resampling with ONE uniform u in [0, 1): a_k = min(C, (C * c_k) / W) for k < C - 1,
 *     a_{C-1} = C exactly, a_{-1} = 0; n_k = ceil(a_k - u) - ceil(a_{k-1} - u), where ceil(a - u) is taken exactly as
 *     floor(a) + [a - floor(a) > u] (the f64 subtraction a - u itself would round: 513 - (1 - 2^-53) is 512).  The min is
 *     needed: where the trailing weights vanish beside W (a large D), c_k == W before the last slot and the rounded
 *     (C * W) / W can be C + 1 ulp, which u = 0 would round up to C + 1.  a_k does not fall with k and stays in [0, C], so
 *     every n_k >= 0 and sum n_k = C for every u in [0, 1); D = 0 gives n_k = 1 for every k.
 *  5. The parent map, in place: a survivor (n_k >= 1) keeps its slot, parent[k] = k; the dead slots (n_k = 0) in ascending
 *     order take the surplus copies, dealt out survivor by survivor in ascending k, n_k - 1 each (numpy: parent[dead] =
 *     repeat(arange(C), maximum(n - 1, 0))).  A source is never overwritten, so nothing is staged.
 *  6. Every dead slot d takes the state of chain parent[d]: the label row, m, m_r, n_r, eta and the running sum of dS
 *     (bisbm_get_cum_dS), bit for bit.  Slot d keeps what keys and counts ITS random streams and its acceptance bookkeeping
 *     (the sweep, shuffle, merge and split counters, accu_r, the last_* and stop_* values): the copies of one parent diverge
 *     at the next sweep, and no stream is ever replayed.
 *  7. u = the 53-bit uniform of the first two words of Philox(seed, counter (round, the handle's first global chain id, purpose
 *     8 = resample)); round = the resampling steps of this handle since the last bisbm_population_reset.
 *  8. ancestor[c] (c at the last reset) becomes ancestor[parent[c]]; log_ratio_total adds up the steps' log_ratio; rounds
 *     counts the steps.
 * Started from a population equilibrated at beta_0, log_ratio_total estimates ln Z(beta_L) - ln Z(beta_0), Z(beta) = sum over
 * partitions of exp(-beta S), and the share of the final population in a mode estimates that mode's posterior mass.
 * Refused, with a message and nothing changed: mt19937-compat mode and two-byte labels (a wide handle) BISBM_ERR_UNSUPPORTED;
 * chains grouped by shape, replica exchange on, static modes set (bisbm_marginals_set_modes; anchored modes are served)
 * BISBM_ERR_STATE; D < 0 or not finite, temperatures that rise BISBM_ERR_INVALID_ARG.  Not served: populations over several
 * processes, adaptive temperature steps, other resampling schemes, weighted (non-resampled) estimators. */

/* Steps 2-5 on the host, without a device: S[n] -> offspring_out[n], parent_out[n], *log_ratio_out (any of them may be NULL).
 * BISBM_ERR_INVALID_ARG (text: bisbm_last_error(NULL)): n = 0, S that is not finite, delta_beta < 0 or not finite, u outside
 * [0, 1). */
int bisbm_population_offspring(uint32_t n, const double *S, double delta_beta, double u,
                               uint32_t *offspring_out, uint32_t *parent_out, double *log_ratio_out);
/* One resampling step of the handle's chains (steps 1-8). */
int bisbm_population_resample(bisbm_handle h, double beta_from, double beta_to,
                              uint32_t *parent_out /* n_chains, may be NULL */, double *log_ratio_out);
/* temps: n_temps >= 2 float temperatures, finite, > 0, non-increasing; the caller has equilibrated the population at temps[0].
 * For k = 1 .. n_temps - 1: a resampling step from 1 / (double)temps[k - 1] to 1 / (double)temps[k], then sweeps_per_step
 * sweeps of every chain at temps[k] (bisbm_anneal with BISBM_SCHED_CONSTANT and no early stop; 0: none).  log_ratio_out[k - 1]:
 * the step's log_ratio; distinct_out[k - 1]: distinct values in `ancestor` after the step (C minus it: the family collapse);
 * acc_rate_out[c]: accepted steps / steps of the run's sweeps.  Any output may be NULL. */
int bisbm_population_run(bisbm_handle h, uint32_t n_temps, const float *temps, uint64_t sweeps_per_step,
                         double *log_ratio_out /* n_temps-1 */, uint32_t *distinct_out /* n_temps-1 */,
                         double *acc_rate_out /* n_chains, may be NULL */);
/* bisbm_population_run with, after every resampling step, rounds_per_step rounds of the recipe at the common temperature
 * temps[k]: mh_sweeps sweeps of bisbm_anneal (BISBM_SCHED_CONSTANT, no early stop), then bisbm_heatbath_run(heatbath_sweeps,
 * beta, 0), then bisbm_reshuffle_run(reshuffles, reshuffle_scans, beta) with beta = 1.0 / (double)temps[k].  There is no
 * exchange.  acc_rate_out[c]: accepted MH steps / MH steps of the run.  Refused as bisbm_population_run, and a NULL recipe or one
 * of all zeros with rounds_per_step > 0 (BISBM_ERR_INVALID_ARG). */
int bisbm_rounds_population_run(bisbm_handle h, uint32_t n_temps, const float *temps, uint64_t rounds_per_step,
                                const bisbm_round_recipe *recipe, double *log_ratio_out /* n_temps-1 */,
                                uint32_t *distinct_out /* n_temps-1 */, double *acc_rate_out /* n_chains, may be NULL */);
/* The genealogy and the totals since the last reset (ancestor_out: n_chains entries; any pointer may be NULL). */
int bisbm_population_get(bisbm_handle h, uint32_t *ancestor_out, uint64_t *rounds_out, double *log_ratio_total_out);
/* ancestor = the identity, rounds = 0, log_ratio_total = 0.  The chains are not touched. */
int bisbm_population_reset(bisbm_handle h);

/* The marginal estimate README.md:49-53 asks for: the most frequent block of every node over all samples of all chains (ties ->
 * the lowest block), n labels in the reference's numbering, from the internal histogram.  Over several devices this is the
 * exchange of SURVEY 8(e), on the devices: ncclReduceScatter of the per-device histograms by node range (RCCL over xGMI) ->
 * argmax on the owner of the range -> ncclAllGather of the labels; peer copies + an add kernel where RCCL cannot serve (a
 * device listed twice, librccl.so missing, BISBM_POOL=p2p). */
int bisbm_marginals_map(bisbm_handle h, uint32_t *labels_out /* n, host */);

/* Posterior-predictive pair scores pooled over chains (no reference counterpart: the reference keeps one partition and scores
 * nothing).  For a pair (u, v), u of type a (u < na) and v of type b (na <= v < n), one chain with labels b, block matrix m and
 * block degree sums m_r contributes the DC-SBM's expected number of edges between the two given its partition,
 *     lambda(u, v) = ((double)d(u) * (double)d(v)) * (double)m[b_u][b_v] / ((double)m_r[b_u] * (double)m_r[b_v])
 * (d = length of the node's CSR row, multi-edges count; f64, in exactly this order of operations), and 0.0 when d(u) or d(v)
 * is 0.  Over all na * nb pairs the terms of one chain add up to the number of edges.  A SAMPLE (bisbm_pair_scores_accumulate)
 * adds, for every pair, the term of every counted chain to a running f64 sum and the number of counted chains to `terms`;
 * counted = every chain, or with replica exchange on only the chains on rung 0.  The estimate is sum / terms.  The term does
 * not depend on how a chain numbers its blocks, so nothing is aligned and chains of different shapes (after
 * bisbm_agg_merge_total), wide handles, both RNG modes and several devices are all served; replica exchange over chains grouped
 * by shape is BISBM_ERR_STATE, as for the marginal histogram.  The sums are added without floating-point atomics, in an order
 * fixed by the pairs, the chain count and the shapes: the same handle and the same calls give the same bits.  Sums and `terms`
 * survive merges, splits, the switch between byte and two-byte labels and regrouping by shape.
 * set: uploads n_pairs pairs (they may repeat and may be edges), replacing earlier ones and zeroing sums and terms; n_pairs = 0
 *   frees everything.  A u outside [0, na) or a v outside [na, n) is BISBM_ERR_INVALID_ARG, bisbm_last_error names the first
 *   offending index, and the earlier pairs stay in place.
 * accumulate: one sample; BISBM_ERR_STATE before bisbm_init / bisbm_shuffle or without pairs.
 * reset: zeroes sums and terms, keeps the pairs.
 * get: sum_out[n_pairs] in the caller's order (over several devices: the per-device sums added on the host in device order) and
 *   terms; either pointer may be NULL. */
int bisbm_pair_scores_set(bisbm_handle h, uint64_t n_pairs, const uint32_t *u, const uint32_t *v);
int bisbm_pair_scores_accumulate(bisbm_handle h);
int bisbm_pair_scores_reset(bisbm_handle h);
int bisbm_pair_scores_get(bisbm_handle h, double *sum_out /* n_pairs, host */, uint64_t *terms_out);

/* Edge probabilities: the exact change of the description length when one listed edge is added or removed, pooled over chains (no
 * reference counterpart; graph-tool's get_edges_prob gives the same quantity).  For a chain with partition b,
 *     P(G +- e | b) / P(G | b) = exp(-dS_e),   dS_e = S(G +- e, b) - S(G, b),
 * S the full description length bisbm_entropy returns.  Pooled over chains it is the posterior-predictive odds of the edited graph.
 * An edge changes no label, so the field energy Phi, a clamp and constraints do not enter.
 * A PAIR is (u, v, kind): u of type a (u < na), v of type b (na <= v < n), kind BISBM_EDGE_ADD (one more edge u - v) or
 * BISBM_EDGE_REMOVE (one edge u - v less).  mu: the number of CSR entries of u equal to v, the present multiplicity.  For a chain
 * r = b_u, s = b_v; d_u, d_v: the CSR row lengths; E: the number of edges; eta_x[d] = eta[x][d] for 0 <= d <= max_degree and 0
 * outside; lg: the engine's lgamma table; lbinom: lbinom_fast; logq(k, n): the log_q bisbm_entropy uses for a block of k edge
 * ends and n nodes -- the non-fast instance in both RNG modes, the one bisbm_debug_log_q(..., fast = 0) probes.  All f64, no fused
 * multiply-add, in this order.  ADD:
 *     t_deg  = (lg(d_u+1) - lg(d_u+2)) + (lg(d_v+1) - lg(d_v+2))
 *     t_m    = lg(m_rs+1) - lg(m_rs+2)
 *     t_mr   = (lg(m_r[r]+2) - lg(m_r[r]+1)) + (lg(m_r[s]+2) - lg(m_r[s]+1))
 *     t_eta  = ((lg(eta_r[d_u]+1) - lg(eta_r[d_u])) + (lg(eta_r[d_u+1]+1) - lg(eta_r[d_u+1]+2)))
 *            + ((lg(eta_s[d_v]+1) - lg(eta_s[d_v])) + (lg(eta_s[d_v+1]+1) - lg(eta_s[d_v+1]+2)))
 *     t_q    = (logq(m_r[r]+1, n_r[r]) - logq(m_r[r], n_r[r])) + (logq(m_r[s]+1, n_r[s]) - logq(m_r[s], n_r[s]))
 *     t_mult = lg(mu+2) - lg(mu+1)
 *     t_E    = lbinom(ka kb + E, E+1) - lbinom(ka kb + E - 1, E)
 *     dS     = (((((t_deg + t_m) + t_mr) + t_eta) + t_q) + t_mult) + t_E
 * REMOVE: the same seven terms in the same order with d+2 -> d in t_deg, t_m = lg(m_rs+1) - lg(m_rs), t_mr = (lg(m_r[r]) -
 * lg(m_r[r]+1)) + ..., the second eta index d-1 instead of d+1, logq(m_r-1, n_r), t_mult = lg(mu) - lg(mu+1) and t_E =
 * lbinom(ka kb + E - 2, E-1) - lbinom(ka kb + E - 1, E).  w = (dS > 700.0) ? 0.0 : exp(-dS) with the device's exp
 * (bisbm_debug_exp).  A SAMPLE (accumulate) adds, for every pair and every counted chain, dS to dS_sum[pair] and w to
 * w_sum[pair], one f64 add each, the chains one at a time in ascending chain index (chains grouped by shape: group by group,
 * each with its own t_E), and the number of counted chains to `terms`; counted = every chain, or with replica exchange on only
 * the chains on rung 0.  There are no floating-point atomics and the result does not depend on tiles or launch geometry: a
 * sequential host loop gives the same bits.  The estimates: the mean dS = dS_sum / terms, and ln P = ln(w_sum / terms), the log
 * posterior-predictive odds.  Both RNG modes, byte and two-byte labels, chains grouped by shape, several devices and handles with
 * a clamp, constraints or fields are served; replica exchange over chains grouped by shape is BISBM_ERR_STATE, as for the pair
 * scores.  Chain state is only read.  Sums and `terms` survive merges, splits, label-width switches and regrouping.
 * set: uploads the pairs (they may repeat), replacing earlier ones and zeroing sums and terms; kind NULL: all ADD; what: 0 or
 *   BISBM_EDGE_KEEP_LAST (keep every chain's dS of the last sample for get_last: n_chains * n_pairs doubles); n_pairs = 0 frees
 *   everything.  BISBM_ERR_INVALID_ARG for a u outside [0, na), a v outside [na, n), an unknown kind, an unknown bit of `what`,
 *   a REMOVE with mu = 0: bisbm_last_error names the first offending index and the earlier pairs and sums stay in place.
 * accumulate: one sample; BISBM_ERR_STATE before bisbm_init / bisbm_shuffle or without pairs.
 * reset: zeroes sums and terms, keeps the pairs.
 * get: dS_sum[n_pairs], w_sum[n_pairs], mult_out[n_pairs] (mu) in the caller's order (several devices: the per-device sums added
 *   on the host in device order) and terms; any pointer may be NULL.
 * get_last: dS of pair `pair_index` (caller's order) in every chain at the last sample, NaN where the chain was not counted;
 *   BISBM_ERR_STATE without BISBM_EDGE_KEEP_LAST or before the first sample. */
#define BISBM_EDGE_ADD 0u
#define BISBM_EDGE_REMOVE 1u
#define BISBM_EDGE_KEEP_LAST 1u
int bisbm_edge_probs_set(bisbm_handle h, uint64_t n_pairs, const uint32_t *u, const uint32_t *v,
                         const uint8_t *kind /* NULL: all ADD */, uint32_t what);
int bisbm_edge_probs_accumulate(bisbm_handle h);
int bisbm_edge_probs_reset(bisbm_handle h);
int bisbm_edge_probs_get(bisbm_handle h, double *dS_sum, double *w_sum, uint32_t *mult_out, uint64_t *terms);
int bisbm_edge_probs_get_last(bisbm_handle h, uint64_t pair_index, double *dS_out /* n_chains, NaN where not counted */);

/* Query scores: for one node, every node of the other type scored and ranked (no reference counterpart).  A QUERY is a node q of
 * either type; its CANDIDATES are all nodes of the other type in id order: na .. n-1 for q < na, 0 .. na-1 for q >= na
 * (n_other of them).  One chain's term for (query, candidate) is exactly the pair-score term above of the pair (type-a node u,
 * type-b node v) the two form,
 *     ((double)d(u) * (double)d(v)) * (double)m[b_u][b_v] / ((double)m_r[b_u] * (double)m_r[b_v]),
 * the same f64 operations in the same order without a fused multiply-add, 0.0 where a degree is 0: bit-equal to what
 * bisbm_pair_scores_* gives one chain for that pair.  Over all candidates one chain's terms add up to d(q).  A SAMPLE
 * (bisbm_query_scores_accumulate) adds the term of every counted chain to sum[query][candidate] and the number of counted chains
 * to `terms`; counted = every chain, or with replica exchange on only the chains on rung 0.  The ORDER OF THE ADDITIONS is part
 * of the definition: per device the counted chains are added one at a time in ascending chain index (chains grouped by shape:
 * group by group in group order, ascending within a group), each with one f64 add onto the running sum -- the result does not
 * depend on tile sizes or launch geometry and a sequential loop on the host reproduces it bit for bit.  Several devices: each
 * keeps the sums of its own chains, and they are added in device order when they are read.  Nothing is aligned (the term does
 * not depend on how a chain numbers its blocks); both RNG modes, chains of different shapes and several devices are served;
 * replica exchange over chains grouped by shape is BISBM_ERR_STATE, as for the pair scores.  A handle with two-byte labels
 * (KA + KB > 256) is refused by accumulate with BISBM_ERR_UNSUPPORTED: bisbm_pair_scores_* serves it, list the pairs there.
 * Sums and terms survive merges, splits and regrouping by shape.  Memory: 8 bytes per (query, candidate) per device.
 * set: uploads n_queries nodes (they may repeat, both types may be mixed), replacing earlier ones, and allocates and zeroes
 *   sum over the queries of n_other doubles per device (64-bit cell indices; nothing is capped or subsampled: an allocation that
 *   fails is BISBM_ERR_HIP with the size in the message).  A query >= n is BISBM_ERR_INVALID_ARG, bisbm_last_error names the
 *   first offending index, and the earlier queries stay in place.  n_queries = 0 frees everything.
 * accumulate: one sample; BISBM_ERR_STATE before bisbm_init / bisbm_shuffle or without queries.
 * reset: zeroes sums and terms, keeps the queries.
 * get_row: the row of query `query_index` (its position in the array given to set) in candidate-id order; sum_out or terms_out
 *   may be NULL.
 * topk: for every query its k best candidates by pooled sum, descending, ties to the lowest node id, selected on the device:
 *   node_out[query][rank] holds global node ids, sum_out (may be NULL) their sums, bit-equal to get_row's.  With
 *   exclude_neighbours != 0 every node in the query's CSR row is not eligible (a neighbour by several edges is simply not
 *   there).  Candidates of sum 0.0 are eligible and rank last, by id.  Where fewer than k candidates are eligible the remaining
 *   entries are 0xffffffff and 0.0.  k = 0 is BISBM_ERR_INVALID_ARG; every k <= 1024 is served, a larger k is
 *   BISBM_ERR_UNSUPPORTED; BISBM_ERR_STATE while terms == 0.  Several devices: the rows are added on the first device in device
 *   order, a bounded chunk of queries at a time, and selected there. */
int bisbm_query_scores_set(bisbm_handle h, uint32_t n_queries, const uint32_t *queries);
int bisbm_query_scores_accumulate(bisbm_handle h);
int bisbm_query_scores_reset(bisbm_handle h);
int bisbm_query_scores_get_row(bisbm_handle h, uint32_t query_index, double *sum_out /* n_other, host */, uint64_t *terms_out);
int bisbm_query_scores_topk(bisbm_handle h, uint32_t k, int exclude_neighbours, uint32_t *node_out /* n_queries * k, host */,
                            double *sum_out /* n_queries * k, host, may be NULL */, uint64_t *terms_out);

/* Edge queries: for one node, every node of the other type weighed by the exact odds of the edge to it, and ranked (no reference
 * counterpart).  Queries and candidates are those of the query scores above: a QUERY is a node q of either type, its CANDIDATES
 * are all nodes of the other type in id order, na .. n-1 for q < na, 0 .. na-1 for q >= na (n_other of them).  One chain's term
 * for (query, candidate) is
 *     w = (dS > 700.0) ? 0.0 : exp(-dS)
 * with dS the ADD dS of "Edge probabilities" above for the pair (type-a node u, type-b node v) the two form: its seven terms in
 * its order, with the pair's present multiplicity mu, the same f64 operations -- bit-equal to what bisbm_edge_probs_* gives that
 * chain for the listed pair (u, v, BISBM_EDGE_ADD), also where the candidate is a neighbour of the query already, by one edge or
 * by several.  (Every two-sided term of dS is (half of u) + (half of v), and IEEE addition commutes: which of the two is the query
 * changes no bit.)  A SAMPLE (bisbm_edge_queries_accumulate) adds w of every counted chain to w_sum[query][candidate] and the
 * number of counted chains to `terms`; counted = every chain, or with replica exchange on only the chains on rung 0.  The order
 * of the additions is that of the query scores and the edge probabilities: per device one f64 add per counted chain in
 * ascending chain index (chains grouped by shape: group by group in group order, each with its own t_E), no floating-point
 * atomics, no partial sums; the result does not depend on tiles, ranges of chains or launch geometry and a sequential loop on
 * the host reproduces it bit for bit.  Several devices: each keeps the sums of its own chains, added in device order when read.
 * ln(w_sum / terms) is the posterior-predictive log odds of the graph with the edge added.  Only w_sum is kept (sums of dS can
 * be negative and are no radix keys; the mean dS stays with bisbm_edge_probs_*): 8 bytes per (query, candidate) per device.
 * Both RNG modes, chains grouped by shape, several devices, replica exchange and handles with a clamp, constraints or fields
 * are served (an edge changes no label); replica exchange over chains grouped by shape is BISBM_ERR_STATE, as for the pair
 * scores.  Chain state is only read.  Sums and terms survive merges, splits and regrouping by shape.
 * set: as bisbm_query_scores_set -- uploads n_queries nodes (they may repeat, both types may be mixed), replacing earlier ones,
 *   allocates and zeroes the sums; a query >= n is BISBM_ERR_INVALID_ARG, bisbm_last_error names the first offending index and
 *   the earlier queries and sums stay in place; n_queries = 0 frees everything.  It also finds, per query, its distinct
 *   neighbours and their mu in the CSR.
 * accumulate: one sample; BISBM_ERR_STATE before bisbm_init / bisbm_shuffle or without queries; BISBM_ERR_UNSUPPORTED on a
 *   handle with two-byte labels (KA + KB > 256): bisbm_edge_probs_* serves it, list the pairs there.
 * reset: zeroes sums and terms, keeps the queries.
 * get_row: the row of query `query_index` (its position in the array given to set) in candidate-id order: w_sum_out[n_other],
 *   mult_out[n_other] (mu of every candidate, 0 where there is no edge) and terms; every pointer may be NULL.
 * topk: the contract of bisbm_query_scores_topk on w_sum -- descending, ties to the lowest node id, with exclude_neighbours != 0
 *   the nodes of the query's CSR row are not eligible, 0xffffffff / 0.0 past the eligible candidates, values bit-equal to
 *   get_row's; k = 0 is BISBM_ERR_INVALID_ARG, k > 1024 BISBM_ERR_UNSUPPORTED, terms == 0 BISBM_ERR_STATE. */
int bisbm_edge_queries_set(bisbm_handle h, uint32_t n_queries, const uint32_t *queries);
int bisbm_edge_queries_accumulate(bisbm_handle h);
int bisbm_edge_queries_reset(bisbm_handle h);
int bisbm_edge_queries_get_row(bisbm_handle h, uint32_t query_index, double *w_sum_out /* n_other, host */,
                               uint32_t *mult_out /* n_other, host */, uint64_t *terms_out);
int bisbm_edge_queries_topk(bisbm_handle h, uint32_t k, int exclude_neighbours, uint32_t *node_out /* n_queries * k, host */,
                            double *w_sum_out /* n_queries * k, host, may be NULL */, uint64_t *terms_out);

/* Co-assignment: for one node, how often every node of its OWN type shares its block (no reference counterpart).  The posterior
 * co-assignment probability P(b_v = b_q | graph) is one row of the consensus (co-classification) matrix; the full n x n matrix
 * is never formed.  A QUERY is a node q of either type; its CANDIDATES are all nodes of its own type in id order, q included:
 * candidate j of a type-a query is node j (na of them), of a type-b query node na + j (nb of them).  A SAMPLE
 * (bisbm_coassign_accumulate) adds, for every counted chain c and every candidate v, 1 to count[query][v] iff
 * label_c(v) == label_c(q), and the number of counted chains to `terms`; counted = every chain, or with replica exchange on
 * only the chains on rung 0 (the rule of bisbm_query_scores_accumulate; replica exchange over chains grouped by shape is
 * BISBM_ERR_STATE).  The estimate of a cell is count / terms.  Label equality does not depend on how a chain numbers its
 * blocks and needs no block tables: nothing is aligned, chains grouped by shape all count, both RNG modes, several devices and
 * handles with two-byte labels (KA + KB > 256) are served, and counts survive merges, splits, regrouping by shape and the
 * change from two-byte to byte labels.  Every result is an integer: count[q][q] == terms, count[q][v] == count[v][q] when both
 * are queries, and a row adds up to the sum over the counted (sample, chain) pairs of n_r[label_c(q)].  Cells are uint32:
 * accumulate refuses with BISBM_ERR_STATE and a message when terms plus the chains about to be counted would pass 2^32 - 1
 * (over all devices together).  Several devices: each keeps the counts of its own chains, and they are added when they are
 * read; integer adds are order-free, so several device entries give the bits of one handle.  Memory: 4 bytes per (query,
 * candidate) per device, plus 4 bytes per (chain of the device, query) for the queries' labels of one sample.
 * set: uploads n_queries nodes (they may repeat -- a repeated query has a row of its own -- and both types may be mixed),
 *   replacing earlier ones, and allocates and zeroes the counts (an allocation that fails is BISBM_ERR_HIP with the size in the
 *   message).  A query >= n is BISBM_ERR_INVALID_ARG, bisbm_last_error names the first offending index, and the earlier
 *   queries stay in place.  n_queries = 0 frees everything.
 * accumulate: one sample; BISBM_ERR_STATE before bisbm_init / bisbm_shuffle or without queries.
 * reset: zeroes counts and terms, keeps the queries.
 * get_row: the row of query `query_index` (its position in the array given to set) in candidate-id order; count_out or
 *   terms_out may be NULL.
 * topk: for every query the k nodes of its own type with the largest counts, THE QUERY NODE ITSELF NEVER ELIGIBLE (another
 *   query row of the same node is a different row, but its node id is the same and is left out too), descending by count, ties
 *   to the lowest node id, selected on the device: node_out[query][rank] holds global node ids, count_out (may be NULL) their
 *   counts.  Nodes of count 0 are eligible and rank last, by id.  Where fewer than k nodes are eligible the remaining entries
 *   are 0xffffffff and 0.  k = 0 is BISBM_ERR_INVALID_ARG; every k <= 1024 is served, a larger k is BISBM_ERR_UNSUPPORTED;
 *   BISBM_ERR_STATE while terms == 0.  Several devices: the rows are added on the first device, a bounded chunk of queries at
 *   a time, and selected there.
 * Diagnostic switch: with byte labels the counting kernel compares four labels as one word and keeps byte-wide partial counts;
 * the environment variable BISBM_COASSIGN_FORM=plain, read at every accumulate, selects the form that extracts, compares and
 * adds every cell on its own instead (the A/B of tools/coassign_bench.py).  The counts are the same in both forms.
 * Out of scope: pooling over processes (one process per GPU), the full n x n matrix, a consensus partition from the rows. */
int bisbm_coassign_set(bisbm_handle h, uint32_t n_queries, const uint32_t *queries);
int bisbm_coassign_accumulate(bisbm_handle h);
int bisbm_coassign_reset(bisbm_handle h);
int bisbm_coassign_get_row(bisbm_handle h, uint32_t query_index, uint32_t *count_out /* n_own, host */, uint64_t *terms_out);
int bisbm_coassign_topk(bisbm_handle h, uint32_t k, uint32_t *node_out /* n_queries * k, host */,
                        uint32_t *count_out /* n_queries * k, host, may be NULL */, uint64_t *terms_out);

/* Fold-in queries: block posterior, recommendations and peers of a node that is NOT in the graph (no reference counterpart).
 * A VIRTUAL NODE q has a type (a or b) and a neighbour list w_0 .. w_{d-1}, d >= 1: ids of existing nodes of the OTHER type, which
 * may repeat and whose order is kept; d_q = d.  alpha > 0 is the caller's smoothing constant (the engine's proposals use the
 * model's epsilon in the same place).  For one counted chain c with labels b, quadrant m, block sums m_r and n_r, K_own blocks of
 * the virtual node's type and K_oth of the other (r, s: block indices within their types), everything in f64 with the
 * operations and in the order written here, without a fused multiply-add; there is no log or exp, only multiplies, one divide
 * per factor, frexp and ldexp, so a sequential host loop reproduces every number bit for bit:
 *   1. block weights, for every r with n_r[r] > 0: (mant, ex) = frexp((double)n_r[r]); for j = 0 .. d-1 in list order, with
 *      s = b[w_j]: x = ((double)m[r][s] + alpha) / ((double)m_r[r] + alpha * (double)K_oth); mant = mant * x;
 *      (mant, e2) = frexp(mant); ex += e2.  Blocks with n_r[r] == 0 have weight 0.
 *   2. posterior: E = max ex_r over the blocks of step 1; w_r = (ex_r - E < -1000) ? 0.0 : ldexp(mant_r, ex_r - E);
 *      Z = w_0 + w_1 + ... added in ascending r, one add at a time; P_c(r) = w_r / Z.
 *   3. recommend table, per block s of the other type: acc = the sum over ascending r of (P_c(r) * (double)m[r][s]) /
 *      (double)m_r[r], the blocks with m_r[r] == 0 or P_c(r) == 0.0 skipped; g_c[s] = acc / (double)m_r[s], 0.0 when m_r[s] == 0.
 *   4. cells.  RECOMMEND row: the candidates are all nodes v of the other type in id order, the term is
 *      ((double)d_q * (double)d(v)) * g_c[b_v], 0.0 when d(v) == 0 -- the term of bisbm_query_scores_* averaged over the block
 *      posterior.  SIMILAR row: the candidates are all nodes v of the virtual node's own type in id order, the term is P_c(b_v)
 *      -- the count of bisbm_coassign_* as a probability.
 *   5. a SAMPLE (bisbm_foldin_accumulate) adds the term of every counted chain onto sum[q][v], one chain at a time in ascending
 *      chain index with one f64 add each (chains grouped by shape: group by group in group order), and the number of counted
 *      chains to `terms`; counted = every chain, or with replica exchange on only the chains on rung 0.  Several devices: each
 *      keeps the sums of its own chains, and they are added in device order when they are read.
 * One chain's terms of a recommend row add up to d_q times the sum of P_c(r) over the blocks with m_r[r] > 0, of a similar row
 * to the sum of P_c(r) n_r[r], up to rounding.  Neither depends on how a chain numbers its blocks: nothing is aligned, both
 * RNG modes, chains grouped by shape, several devices and replica exchange are served; replica exchange over chains grouped by
 * shape is BISBM_ERR_STATE and a handle with two-byte labels BISBM_ERR_UNSUPPORTED at accumulate.  Sums and terms survive
 * merges, splits and regrouping.
 * set: replaces earlier virtual nodes and zeroes sums and terms; n_queries = 0 frees everything (the other arguments are not
 *   looked at).  list_ptr[0] = 0, list_ptr[i + 1] - list_ptr[i] = the length of node i's list.  `what`: the row kinds to keep.
 *   BISBM_ERR_INVALID_ARG, bisbm_last_error naming the first offending query and position, the earlier virtual nodes staying
 *   in place: an empty list, a list entry that is not a node of the other type, alpha not finite or <= 0, what == 0 or with
 *   an unknown bit, a type above 1.  Memory: 8 bytes per (virtual node, candidate) per kept row kind per device; nothing is
 *   capped or subsampled; an allocation that fails is BISBM_ERR_HIP with the size in the message.
 * accumulate: one sample; BISBM_ERR_STATE before bisbm_init / bisbm_shuffle or without virtual nodes.  Scratch per device: the
 *   posteriors of the sample, 8 bytes per (chain, virtual node, block of its type), kept for get_posteriors; the recommend tables,
 *   8 bytes per (chain, virtual node, block of the other type), for as many chains at a time as fit 256 MiB (at least one).
 * reset: zeroes sums and terms and forgets the last sample's posteriors; keeps the virtual nodes.
 * get_posteriors: P_c(.) of the LAST sample for every chain of the handle in handle chain order, p_out[c * stride + r], padded
 *   with 0.0 up to stride; a chain that was not counted has a row of NaN (the convention of
 *   bisbm_marginals_get_mode_assignment).  A stride below some chain's K_own is BISBM_ERR_INVALID_ARG; BISBM_ERR_STATE before
 *   the first sample.
 * get_row: the row of kind `what` (exactly one kept kind, else BISBM_ERR_INVALID_ARG) of virtual node `query_index` in
 *   candidate-id order; sum_out or terms_out may be NULL.
 * topk: for every virtual node the k best candidates of the rows of kind `what`, descending by sum, ties to the lowest node
 *   id, selected exactly on the device, with the semantics of bisbm_query_scores_topk (k = 0 BISBM_ERR_INVALID_ARG, k <= 1024
 *   else BISBM_ERR_UNSUPPORTED, 0xffffffff / 0.0 past the eligible candidates, BISBM_ERR_STATE while terms == 0).  With
 *   exclude_listed != 0 and what == RECOMMEND the nodes of the virtual node's list are not eligible; for SIMILAR exclude_listed
 *   must be 0 (a virtual node has no id of its own to leave out).
 * Out of scope: a block posterior pooled over chains (it needs alignment), neighbours of the virtual node's own type, pooling
 * over processes, two-byte labels. */
#define BISBM_FOLDIN_RECOMMEND 1u
#define BISBM_FOLDIN_SIMILAR 2u
int bisbm_foldin_set(bisbm_handle h, uint32_t n_queries, const uint8_t *type /* 0 = a, 1 = b */,
                     const uint64_t *list_ptr /* n_queries + 1 */, const uint32_t *list /* node ids */, double alpha,
                     uint32_t what /* bit mask of the rows to keep */);
int bisbm_foldin_accumulate(bisbm_handle h);
int bisbm_foldin_reset(bisbm_handle h);
int bisbm_foldin_get_posteriors(bisbm_handle h, uint32_t query_index, uint32_t stride, double *p_out /* n_chains * stride */);
int bisbm_foldin_get_row(bisbm_handle h, uint32_t what, uint32_t query_index, double *sum_out, uint64_t *terms_out);
int bisbm_foldin_topk(bisbm_handle h, uint32_t what, uint32_t k, int exclude_listed, uint32_t *node_out /* n_queries * k */,
                      double *sum_out /* n_queries * k, may be NULL */, uint64_t *terms_out);

/* Node conditionals: each node's full block posterior given the rest (no reference counterpart).  The step's dS(v: r -> s) is
 * the change of the full description length, so P(b_v = s | all other labels, graph) ~ exp(-dS(v -> s)) is the node's exact
 * full conditional in a chain.  A QUERY is an existing node v of either type; queries may repeat and may mix types;
 * queries = NULL with n_queries = n means every node in id order.
 * For one counted chain c with labels b, r = b_v, d = d(v), K_own blocks of v's type and K_oth of the other, s any block of v's
 * type, k_t the number of v's CSR entries whose label is t (multi-edges count), eta_x = eta[x][d], lg the engine's lgamma_fast
 * table, logq the Philox-mode log_q, everything in f64 without a fused multiply-add:
 *   1. dS_r = 0.0 exactly; for s != r
 *        acc   = 0.0; for t = 0 .. K_oth-1 in ascending order, the t with k_t == 0 skipped:
 *                acc = acc + ((lg(m_rt+1) + lg(m_st+1)) - (lg(m_rt-k_t+1) + lg(m_st+k_t+1)))
 *        tail1 = (lg(m_r[r]-d+1) - lg(m_r[r]+1)) + (lg(m_r[s]+d+1) - lg(m_r[s]+1))
 *        tail2 = (lg(eta_r+1) - lg(eta_r)) + (lg(eta_s+1) - lg(eta_s+2))
 *        tail3 = (logq(m_r[r]-d, n_r[r]-1) - logq(m_r[r], n_r[r])) + (logq(m_r[s]+d, n_r[s]+1) - logq(m_r[s], n_r[s]))
 *        dS_s  = ((acc + tail1) + tail2) + tail3
 *      -- the quantities of metropolis_hasting.cc:150-183.  The order of the additions is fixed by (K_own, K_oth) alone (a
 *      skipped t would add +0.0) and no floating-point atomic is used: the same handle and calls give the same bits.  It is NOT
 *      the sweep's 64-leaf butterfly: the two agree to rounding.
 *   2. FREE: the node is free in chain c iff K_own > 1 and n_r[r] > 1 (the sampler vetoes a move that empties a block, so a
 *      node alone in its block has the point mass on r as its conditional).
 *   3. weights, with the caller's finite beta > 0.  Not free: P_c(r) = 1.0, all others 0.0.  Free: dS_min = min_s dS_s
 *      (including the 0 at r); x_s = beta * (dS_s - dS_min); w_s = (x_s > 700.0) ? 0.0 : exp(-x_s); Z = w_0 + w_1 + ... in
 *      ascending s, one add at a time; P_c(s) = w_s / Z.
 *   4. label-free terms of the chain: stay = P_c(r); entropy = 0.0 - (the sum over ascending s of P_c(s) * ln P_c(s), the terms
 *      with P_c(s) == 0.0 skipped); margin = min over s != r of dS_s, taken only when the node is free.
 *   5. a SAMPLE (bisbm_conditionals_accumulate) adds every counted chain's stay and entropy to stay_sum[q] and entropy_sum[q]
 *      and, where the node is free, margin to margin_sum[q] and 1 to free[q], one chain at a time in ascending chain index
 *      with one f64 add each (chains grouped by shape: group by group in group order), and the number of counted chains to
 *      `terms`; counted = every chain, or with replica exchange on only the chains on rung 0 (the rule of
 *      bisbm_query_scores_accumulate; replica exchange over chains grouped by shape is BISBM_ERR_STATE).  Several devices: each
 *      keeps the sums of its own chains, and they are added in device order when they are read.
 *   6. SOFT MARGINALS, kept only while a reference partition is set (bisbm_conditionals_set_reference: n labels, checked as
 *      the reference of bisbm_marginals_set_reference against the handle's common shape; NULL clears it; either zeroes prob and
 *      its terms).  Every chain gets the permutation pi_c of "Label alignment before pooling" to the reference, computed afresh
 *      at this sample with the same overlap table, solver and tie rule, and prob[q][pi_c(s) - type base] += P_c(s) for every
 *      counted chain in ascending order, one f64 add each; prob has kmax = max(ka, kb) columns per query.  Refused like the
 *      aligned histogram: a wide handle BISBM_ERR_UNSUPPORTED; chains grouped by shape, or a reference made for other block
 *      counts (after a merge or split: "set it again"), BISBM_ERR_STATE.  There is no library-chosen reference: pass
 *      bisbm_get_memberships of the chain you want.
 *   7. LAST ROWS, kept only with BISBM_COND_KEEP_LAST in `what`: dS_s and P_c(s) of the last sample for every (chain of the
 *      handle, query); chains that were not counted hold NaN.  16 * n_chains * (sum over the queries of K_own) bytes.
 * Served: byte labels, chains grouped by shape (label-free sums and last rows), several devices, replica exchange (rung 0),
 * anchored or static modes being set (nothing of theirs is touched).  Chain state, random streams and running sums are only
 * read; the sums survive merges and splits.
 * set: replaces earlier queries, zeroes everything and forgets the reference; n_queries = 0 frees everything.
 *   BISBM_RNG_MT19937_COMPAT is BISBM_ERR_UNSUPPORTED (the definition is the Philox-mode arithmetic).  BISBM_ERR_INVALID_ARG,
 *   bisbm_last_error naming the first offending index and the earlier queries staying in place: a query >= n, beta not finite
 *   or <= 0, an unknown bit of `what`.  Memory per device: 40 bytes per query, 8 * kmax per query with a reference.
 * accumulate: one sample; BISBM_ERR_STATE before bisbm_init / bisbm_shuffle or without queries, BISBM_ERR_UNSUPPORTED with
 *   two-byte labels.  Scratch per device: 32 bytes per (chain, query) and, without KEEP_LAST, the rows, for as many chains at a
 *   time as fit 256 MiB (at least one); with a reference the overlap tables of the aligned histogram for every chain.
 * reset: zeroes sums, prob and terms and forgets the last rows; keeps queries, beta and the reference.
 * get_stats: n_queries entries each, any pointer may be NULL.
 * get_marginals: prob_out[n_queries * kmax] with the terms added to it since the reference was set (or the last reset);
 *   BISBM_ERR_STATE without a reference.
 * get_last: the conventions of bisbm_foldin_get_posteriors (handle chain order, row c at c * stride, padded with 0.0, a NaN
 *   row for a chain that was not counted, a stride below some chain's K_own BISBM_ERR_INVALID_ARG); BISBM_ERR_STATE without
 *   KEEP_LAST or before the first sample; dS_out or p_out may be NULL.
 * Out of scope: conditionals in mt19937-compat arithmetic, two-byte labels, pooling over processes, a library-chosen
 * reference, per-mode soft histograms.  (Top-k of the least settled nodes on the device: "Least settled" below; the row under a
 * clamp, constraints and fields: "Held conditionals" below.)  Moving nodes by these rows is bisbm_heatbath_run below. */
#define BISBM_COND_KEEP_LAST 1u
int bisbm_conditionals_set(bisbm_handle h, uint32_t n_queries, const uint32_t *queries /* NULL: all n nodes */, double beta,
                           uint32_t what);
int bisbm_conditionals_set_reference(bisbm_handle h, const uint32_t *labels /* n, NULL clears; zeroes prob */);
int bisbm_conditionals_accumulate(bisbm_handle h);
int bisbm_conditionals_reset(bisbm_handle h);
int bisbm_conditionals_get_stats(bisbm_handle h, double *stay_sum, double *entropy_sum, double *margin_sum,
                                 uint64_t *free_out /* n_queries each, any may be NULL */, uint64_t *terms_out);
int bisbm_conditionals_get_marginals(bisbm_handle h, double *prob_out /* n_queries * kmax */, uint32_t *kmax_out,
                                     uint64_t *terms_out);
int bisbm_conditionals_get_last(bisbm_handle h, uint32_t query_index, uint32_t stride, double *dS_out,
                                double *p_out /* n_chains * stride each, either may be NULL */);

/* Held conditionals: the sampler's own conditional, returned (no reference counterpart).  The calls above evaluate the model's
 * unrestricted row whatever is held.  With the switch on, bisbm_conditionals_accumulate evaluates instead the HELD ROW: the row
 * the heat-bath kernel forms under the handle's clamp ("Clamped nodes" 2.), block constraints ("Block constraints" 2.) and
 * block fields ("Block fields" 2.), the same f64 operations in the same order -- a heat-bath replay fed these rows needs no
 * host-side restriction and no field add.  The holds are read as they are at each sample; no copy is taken at switch time.
 * For query v in counted chain c, with r = b_v, clamped = v's mask byte is non-zero, A_v = the blocks of v's type that its class
 * allows (all of them without constraints; r is in A_v, because setting constraints validates the labels) and f = the field row
 * of v's class over v's type (absent without fields), in f64 with no fused multiply-add:
 *   1. dE_r = 0.0; for s != r, dE_s = dS_s + (f[s] - f[r]) with fields (the difference first, then one add) and dE_s = dS_s
 *      without, dS_s exactly as in "Node conditionals" 1.  Evaluated and reported for EVERY s of the type, inside A_v or not:
 *      dS_out of bisbm_conditionals_get_last holds dE.
 *   2. OPEN iff K_own > 1 and n_r[r] > 1 and not clamped and |A_v| > 1.
 *   3. Not open: the point mass on r.  Open: mn = min over s in A_v of dE_s (the 0 at r included); x_s = beta (dE_s - mn);
 *      w_s = (x_s > 700.0) ? 0.0 : exp(-x_s) for s in A_v and exactly 0.0 outside; Z = the w_s added in ascending s over all s
 *      (a +0.0 term keeps every bit); P(s) = w_s / Z.
 *   4. Per-chain terms: stay = P(r); entropy = 0.0 - sum P ln P in ascending s, zero terms skipped; margin = min over s in
 *      A_v, s != r, of dE_s, taken only when the node is open; `free` counts the chains in which the node is open.
 *   5. Everything downstream is unchanged and is fed these rows: pooling over chains, soft marginals through the alignment,
 *      last rows, rung-0 counting, several devices, shape groups.
 * set: on != 0 switches to the held row, 0 back to the model's row.  A call that changes the switch zeroes the label-free sums,
 *   prob and their terms and forgets the last rows (a sum over two definitions means nothing); queries, beta, `what` and the
 *   reference stay.  A call that does not change it changes nothing.  bisbm_conditionals_set puts the switch back to off, as it
 *   forgets the reference.  BISBM_ERR_STATE without queries.  Allowed wherever the conditionals are allowed; holds themselves
 *   are refused on compat, wide and shape-grouped handles, where the switch therefore changes nothing.  On with no clamp, no
 *   constraints and no fields the plain kernel runs: the plain call bit for bit.
 * Out of scope: the field and the lists inside the fold-in posteriors, a mask or a table per chain, pooling over processes,
 * per-mode soft histograms. */
int bisbm_held_conditionals_set(bisbm_handle h, int on);
int bisbm_held_conditionals_get(bisbm_handle h, int *on_out);

/* Least settled: the k queries whose pooled conditional is the least decided, selected on the device (no reference
 * counterpart).  One statistic of the current sums of bisbm_conditionals_get_stats (held rows or plain rows alike) is ranked over
 * the n_queries entries by the exact radix select of the other top-k calls: by entropy, the largest entropy_sum first; by stay,
 * the smallest stay_sum first; ties in ascending query index.  query_out holds query INDICES (queries may repeat), value_out[i]
 * the entry bisbm_conditionals_get_stats returns for query_out[i], bit for bit -- over several devices the device sums are added
 * in device order, as get_stats adds them.  Both statistics are sums of non-negative terms (stay is in [0, 1], an entropy term
 * is 0.0 - a sum of terms <= 0), so their bit patterns order as unsigned keys.  k follows bisbm_coassign_topk: k = 0
 * BISBM_ERR_INVALID_ARG, k > 1024 BISBM_ERR_UNSUPPORTED, past the n_queries entries query_out is 0xffffffff and value_out 0.0.
 * BISBM_ERR_STATE without queries or before the first sample; BISBM_ERR_INVALID_ARG for an unknown `by`.
 * Out of scope: a mean-margin ranking (`free` differs per query: a division per key). */
#define BISBM_SETTLED_BY_ENTROPY 0u   /* largest entropy_sum first */
#define BISBM_SETTLED_BY_STAY    1u   /* smallest stay_sum first */
int bisbm_least_settled_topk(bisbm_handle h, uint32_t by, uint32_t k, uint32_t *query_out /* k query indices */,
                             double *value_out /* k, may be NULL */, uint64_t *terms_out);

/* Heat-bath sweeps and greedy polishing: nodes moved by their conditionals (no reference counterpart).  Where the MH step draws
 * one target block and accepts or rejects it, a heat-bath (Gibbs) update draws the node's new block from its exact conditional
 * P(b_v = s | rest) ~ exp(-beta dS_s), and the greedy update (beta = +inf) takes the block of the lowest dS.  For every chain,
 * `sweeps` sweeps of n node updates; Philox mode and byte labels only.
 *   1. VISIT ORDER: exactly the MH sweep's.  Sweep index = the chain's sweeps_total; the type-a class first, then type b, each
 *      through the tiled keyed order of DESIGN.md section 4 with the keys Philox(seed; idx = 2 * sweeps_total (+ 1 for type b),
 *      chain = global chain id, purpose 2).  sweeps_total advances by one per sweep run, so no later call of any kind replays
 *      a visit order.
 *   2. ROW: for the visited node v with current block r, dS_s and P(s) over all blocks s of v's type as steps 1-3 of "Node
 *      conditionals" with this call's beta, the same f64 operations in the same order: bit-equal to what
 *      bisbm_conditionals_accumulate (KEEP_LAST) returns for that node on the same state.
 *   3. CHOICE, finite beta > 0: a node that is not free stays.  For a free node u = the 53-bit uniform
 *      ((x << 32 | y) >> 11) * 2^-53 of the first two words x, y of Philox(seed; idx = sweeps_total * n + position in the sweep,
 *      chain = global chain id, purpose 9); C_s = P_0 + ... + P_s, added one at a time in ascending s; the new block is the
 *      first s with u < C_s, and if there is none (C of the last block rounded below 1) the largest s with P_s > 0.
 *   4. CHOICE, beta = +inf (greedy): a node that is not free stays.  For a free node s* = the lowest s that attains min_s dS_s
 *      over all s including r; the node moves iff dS_{s*} < 0 strictly.  No random draw is used.
 *   5. APPLY: a move with s != r updates the label, m, m_r, n_r and eta as an accepted MH step does and adds dS_s onto the
 *      chain's running sum (bisbm_get_cum_dS) with one f64 add.  A node never leaves a block it is alone in (the FREE rule).
 *   6. stop_when_settled != 0: a chain stops after the first sweep in which it moved nothing; that sweep counts in sweeps_out,
 *      and sweeps_total advances only by the sweeps actually run.  Meaningful with beta = +inf (the partition is then a local
 *      minimum of the description length under single-node moves), allowed with any beta.
 *   7. moved_out[c] = moves with s != r, sweeps_out[c] = sweeps run; bisbm_get_last_counts reports the same two numbers.  The
 *      MH object's accu_r, anneal()'s early-stop bookkeeping, the population genealogy and every sum of the analysis calls
 *      (marginals, pair scores, conditionals, ...) are untouched.
 * Served: chains grouped by shape (group by group), several devices behind one handle (everything is keyed by the global chain
 * id: the result equals one device with all the chains), static or anchored modes being set.
 * Refused, with a message and nothing changed: BISBM_RNG_MT19937_COMPAT and two-byte labels BISBM_ERR_UNSUPPORTED; replica
 * exchange on BISBM_ERR_STATE (as bisbm_anneal); before bisbm_init / bisbm_shuffle BISBM_ERR_STATE; beta NaN, <= 0 or -inf
 * BISBM_ERR_INVALID_ARG.  sweeps = 0 is a no-op that returns BISBM_OK (the outputs are zeroed).
 * Inside replica exchange and population annealing the sweeps run through bisbm_tempering_run_rounds /
 * bisbm_rounds_population_run, under replica exchange at a beta per chain.  Out of scope: greedy polishing per chain,
 * mt19937-compat arithmetic, wide handles.  A move of many nodes at once is bisbm_reshuffle_run below. */
int bisbm_heatbath_run(bisbm_handle h, uint64_t sweeps, double beta, int stop_when_settled,
                       uint64_t *moved_out /* n_chains, may be NULL */, uint64_t *sweeps_out /* n_chains, may be NULL */);

/* Pair reshuffles (no reference counterpart): the nodes of two blocks of one type are divided afresh between the two in ONE
 * accepted or rejected move -- the split-merge move of Jain and Neal at a fixed block count, the "merge-split" of Peixoto
 * 2020 -- where every other sampler of the engine moves one node at a time.  Philox mode and byte labels only; f64 without a
 * fused multiply-add; exp and log are the device's (bisbm_debug_exp returns the device's exp to a host that replays a move).
 * The move is defined per chain; j = the chain's reshuffles_total, a 32-bit counter beside sweeps_total that advances by one
 * per proposed move, accepted or not, so no later call replays a draw (it wraps after 2^32 moves of one chain).
 *   1. RANDOMNESS: X(k) = the four words of Philox(seed; idx = (j << 32) | k, chain = global chain id, purpose 10); U(k) = the
 *      53-bit uniform of heat-bath step 3 from the first two words of X(k).  k = 0: the pair; k = 1: u_acc; with M members and
 *      W = ceil(M / 128), k = 2 + (i >> 7) for i < M: the launch bit of member i is bit (i & 31) of word ((i >> 5) & 3) of X(k);
 *      k = 2 + W + t * M + i: the uniform of member i in scan t (t = 0 .. scans-1: the launch scans; t = scans: the forward
 *      pass).  A slot whose member is not free is never drawn.  A call with 2 + ceil(nmax / 128) + (scans + 1) * nmax >= 2^32,
 *      nmax = max(na, nb), is BISBM_ERR_INVALID_ARG.
 *   2. PAIR: N = C(ka, 2) + C(kb, 2) unordered pairs {r < s} of blocks of one type, enumerated type a first, each type
 *      lexicographically ((0,1), (0,2), ..., (0,k-1), (1,2), ...); the pair is number (x * N) >> 32 with x the first word of
 *      X(0), in 64-bit integers.  N = 0 (ka <= 1 and kb <= 1): the move is a counted no-op (record type BISBM_RESHUFFLE_NONE).
 *      The choice never looks at the state.
 *   3. MEMBERS: the nodes of that type whose label is r or s, in ascending id; M of them (M >= 2: no block is ever empty).
 *   4. LAUNCH: member i gets s if its launch bit is set, else r; if no member got r, member 0 gets r; if none got s, member
 *      M - 1 gets s; then `scans` >= 0 restricted scans (step 5).  The result L depends on the member set, the random stream
 *      and the labels outside the set, never on how the members were divided.
 *   5. RESTRICTED SCAN STEP: the members in ascending id.  Member v is in block c of {r, s}, o is the other one.  Not free
 *      (n_r[c] == 1): v stays, the factor is 1.0, no uniform is drawn.  Free: dS_o = the entry of o of step 1 of "Node
 *      conditionals" on the current state, bit for bit (the node's current block c in the place of r there), dS_c = 0.0;
 *      dS_min = dS_o < 0.0 ? dS_o : 0.0; x = beta * (dS - dS_min); w = x > 700.0 ? 0.0 : exp(-x) for each of the two;
 *      Z = w_r + w_s in that order; P_r = w_r / Z, P_s = w_s / Z; v goes to r iff u < P_r, else to s; the factor is the P of
 *      the block it went to.  A move updates the label, m, m_r, n_r and eta as a heat-bath move does.
 *   6. REVERSE PASS: from L, the members in the same order, each FORCED to its original label.  Q_rev starts as frexp(1.0) =
 *      (0.5, 1) and is multiplied by one factor P(original label) at a time (1.0 for a member that is not free and stays):
 *      mantissa = frexp(mantissa * factor, &e), exponent += e, so thousands of members do not underflow.  dS_rev starts at
 *      0.0 and gets the dS_o of every forced move added, one at a time.  A forced move of a member that is not free, or a
 *      factor of exactly 0.0, makes Q_rev = (0.0, 0) and the move a certain rejection: from that member on nothing is
 *      evaluated or added (its own dS_o is not added either), the remaining members go to their original labels in transit
 *      (step 9), the forward pass is not run, and the record holds dS_fwd = 0.0, Q_fwd = (0.0, 0), A = 0.0.  Either way the
 *      pass ends exactly at the original state.
 *   7. FORWARD PASS: L is set again (transit), then one free scan (t = scans) yields Q_fwd and dS_fwd as above; Q_fwd > 0
 *      by construction.  The end state is the proposal.
 *   8. ACCEPT: dS = dS_fwd - dS_rev; ln A = (0.0 - beta * dS) + (log(mant_rev / mant_fwd) + (double)(exp_rev - exp_fwd) *
 *      0.6931471805599453); A = exp(ln A); accepted iff u_acc < A.  Accepted: the proposal stays and dS goes onto
 *      bisbm_get_cum_dS with one add.  Rejected: labels, m, m_r, n_r and eta return to their values before the move, integer
 *      for integer (transit), and the running sum is untouched.
 *   9. TRANSIT (original -> launch labels, original -> L, proposal or a dead reverse pass -> original): moves are applied
 *      without evaluating anything; a block may be empty on the way, and no table is read at such a state.
 * Why exp(-beta S) stays invariant: the pair and L are drawn independently of how the members are divided, so x -> y and
 * y -> x share every (pair, L); each contributes p(L) min(pi(x) q(y | L), pi(y) q(x | L)) to both directions (detailed balance).
 * A move touches about 2 n / K nodes (scans + 2) times with an evaluation and up to three times in transit.
 * Served and refused exactly as bisbm_heatbath_run: chains grouped by shape, several devices (everything is keyed by the global
 * chain id), static or anchored modes being set are served; BISBM_RNG_MT19937_COMPAT and two-byte labels
 * BISBM_ERR_UNSUPPORTED; replica exchange on BISBM_ERR_STATE; before bisbm_init / bisbm_shuffle BISBM_ERR_STATE; beta not
 * finite or <= 0 BISBM_ERR_INVALID_ARG; each with a message and nothing changed.  moves = 0 is a no-op that zeroes
 * accepted_out.  sweeps_total, accu_r, bisbm_get_last_counts, the early-stop bookkeeping, the genealogy and every analysis sum
 * are untouched.  Scratch: 6 bytes per (chain, node of the larger type) -- member id, original label, launch label --
 * allocated at the first call and freed with the handle; an allocation failure is BISBM_ERR_HIP with the size in the message.
 * get_last: the last move of the last call of every chain (r, s: global labels); BISBM_ERR_STATE while a chain has none (no
 * call yet, or its group was formed by a merge since).
 * Inside replica exchange and population annealing the moves run through bisbm_tempering_run_rounds /
 * bisbm_rounds_population_run, under replica exchange at a beta per chain.  Out of scope: moves that change Ka or Kb,
 * mt19937-compat arithmetic, wide handles, choosing the pair by the state. */
#define BISBM_RESHUFFLE_NONE 0xffffffffu
typedef struct bisbm_reshuffle_record {
    uint32_t type;     /* 0: a, 1: b, BISBM_RESHUFFLE_NONE: no pair (everything else 0) */
    uint32_t r, s, M;
    double dS_fwd, dS_rev;
    double q_fwd_mant, q_rev_mant;
    int32_t q_fwd_exp, q_rev_exp;
    double u_acc, A;
    uint32_t accepted;
    uint32_t reserved;
} bisbm_reshuffle_record;
int bisbm_reshuffle_run(bisbm_handle h, uint64_t moves, uint32_t scans, double beta,
                        uint64_t *accepted_out /* n_chains, may be NULL */);
int bisbm_reshuffle_get_last(bisbm_handle h, bisbm_reshuffle_record *out /* n_chains */);
/* The chains' reshuffles_total. */
int bisbm_reshuffle_get_total(bisbm_handle h, uint64_t *out /* n_chains */);

/* Split and merge moves (no reference counterpart): one block divided in two, or two blocks of one type made one, in ONE accepted
 * or rejected move, so that the chains sample (Ka, Kb) with the partition.  exp(-beta S), S = bisbm_entropy's full description
 * length -- which holds lbinom(Ka Kb + E - 1, E), lbinom(na - 1, Ka - 1) and lbinom(nb - 1, Kb - 1) and is therefore comparable
 * across shapes --, stays exactly invariant over the UNLABELLED partitions of every shape with k_min[t] <= K_t <= k_max[t].  It is
 * Jain and Neal's split-merge: the pair reshuffle above with one side empty before or after.  Philox mode and byte labels; f64
 * without a fused multiply-add; exp and log are the device's.  Defined per chain; j = the chain's count of proposed split / merge
 * moves (a 32-bit counter kept with the chain through every regrouping, one per proposal whatever became of it).
 *   1. RANDOMNESS: X(k) = Philox(seed; idx = (j << 32) | k, chain = global chain id, purpose 11); U(k) as in "Pair reshuffles".
 *      k = 0: kind and choice; k = 1: u_acc; launch bits and scan uniforms at the k of "Pair reshuffles" 1. (the forward pass of a
 *      split is scan t = scans; a merge draws no uniform past the launch scans).
 *   2. KIND AND CHOICE, from the shape (ka, kb) alone, K = ka + kb: bit 0 of the first word of X(0) clear: SPLIT of block
 *      (y * K) >> 32, y the second word of X(0), a global label; set: MERGE of pair number (y * N) >> 32 of the N(ka, kb) =
 *      C(ka, 2) + C(kb, 2) same-type pairs {r < s} in the enumeration of "Pair reshuffles" 2.  With t the type of the block or
 *      pair, the proposal is REFUSED -- counted as proposed, rejected, nothing evaluated -- when: a merge and N = 0
 *      (BISBM_SM_NO_PAIR); a merge and k_t <= k_min[t] (BISBM_SM_AT_K_MIN); a split and k_t >= k_max[t] (BISBM_SM_AT_K_MAX); a
 *      split and the block has fewer than 2 nodes (BISBM_SM_SINGLETON), tested in this order.
 *   3. MEMBERS AND ROLES: the nodes of r (split) or of r and s (merge), ascending id, M of them.  Member 0 is pinned: the part
 *      that holds it is HOME, the other AWAY, which counts every unordered division of the set once.  Split: home is r, away
 *      the new block.  Merge: home is the block of member 0 now.
 *   4. LAUNCH STATE L: member 0 home; member i >= 1 away iff its launch bit is set; if none is away, member M - 1 goes away;
 *      then `scans` restricted scans over members 1 .. M - 1 in ascending order.  A step is step 5 of "Pair reshuffles" with
 *      (home, away) in the place of (r, s): a member alone in its block (only the sole member of away can be) stays with the
 *      factor 1.0 and no draw; otherwise Z = w_home + w_away, the member goes home iff u < P_home, the factor is the P of where
 *      it went.  L depends on the member set and the rest of the state, never on the present division.  Getting from the
 *      present state to the launch labels is transit: no table is read.
 *   5. merge_dS(D) = S(all members in one block) - S(D) for a division D into blocks h and a of type t, with m_ht, m_at over the
 *      blocks t' of the other type in ascending order, eta_hk, eta_ak over k = 0 .. max_degree ascending, lg = the lgamma table:
 *        acc_m = 0.0; acc_m = acc_m + ((lg(m_ht' + 1) + lg(m_at' + 1)) - lg(m_ht' + m_at' + 1)) for every t'
 *        acc_e = 0.0; acc_e = acc_e + ((lg(eta_hk + 1) + lg(eta_ak + 1)) - lg(eta_hk + eta_ak + 1)) for every k
 *        tail1 = lg(m_h + m_a + 1) - (lg(m_h + 1) + lg(m_a + 1))
 *        tail2 = log_q(m_h + m_a, n_h + n_a) - (log_q(m_h, n_h) + log_q(m_a, n_a))     (log_q: bisbm_entropy's)
 *        merge_dS = (((acc_m + acc_e) + tail1) + tail2) + (T(shape merged) - T(shape of D))
 *      T(ka, kb) = (lbinom(ka kb + E - 1, E) + lbinom(na - 1, ka - 1)) + lbinom(nb - 1, kb - 1) from the host's tables
 *      (bisbm_split_merge_shape_term returns it).  An empty block adds exactly 0 to every other term of S.  No pass over the
 *      members is needed.  The closed form was chosen over two evaluations of the full description length: it costs K + D
 *      table gathers a move instead of two passes over the whole block state, and it meets the 1e-9 |S| of the tests.
 *   6. SPLIT: one free scan (t = scans) from L over members 1 .. M - 1 gives the proposal D' and Q_fwd (mantissa, exponent as in
 *      "Pair reshuffles" 6.).  dS = 0.0 - merge_dS(D');
 *      ln A = ((0.0 - beta * dS) + (log((double)K) - log((double)N(shape after)))) - (log(mant) + (double)exp * 0.6931471805599453).
 *   7. MERGE: a forced pass from L to the present division D gives Q_rev; a member that is not free forced to move, or a factor
 *      of exactly 0.0, makes Q_rev = (0.0, 0) and the move a certain rejection (ln A = -inf, A = 0.0), the members return in
 *      transit.  dS = merge_dS(D), evaluated at D before anything moves;
 *      ln A = ((0.0 - beta * dS) + (log((double)N(shape now)) - log((double)(K - 1)))) + (log(mant) + (double)exp * 0.6931471805599453).
 *   8. ACCEPT: A = exp(ln A); accepted iff u_acc < A.  Accepted: dS goes onto bisbm_get_cum_dS with one add, and the blocks are
 *      renumbered: split of a type-a block: away becomes label ka, every type-b label moves up by one; split of a type-b
 *      block: away becomes label K; merge: the merged block takes r, the labels of that type above s move down by one, and for
 *      a type-a merge every type-b label moves down by one as well.  Rejected (or refused): labels, m, m_r, n_r, eta and the
 *      running sum are what they were, integer for integer.  The invariance claim concerns the unlabelled partition only.
 * Why it is exact: a split x -> y of block b and the merge y -> x of the pair it creates share L; the forward path has
 * probability (1/2)(1/K) p(L) q(y | L), the reverse (1/2)(1/N(shape of y)) p(L) -- the merge is deterministic given the pair --
 * and the shape of x has K blocks where that of y has K + 1, which is the K - 1 of step 7.
 * An accepted move changes the chain's shape: the handle keeps its chains GROUPED BY SHAPE as after bisbm_agg_merge_total (a plain
 * handle becomes a container at the first accepted move), and a chain that reaches a shape another group already holds joins
 * that group.  Groups are formed again only after a launch in which some chain was accepted, and only the groups that lost or
 * gained a chain are rebuilt.  Every device entry regroups its own chains; results are keyed by the global chain id and do not
 * depend on the number of devices or on the grouping.  AFTER ACCEPTED MOVES THE CALLER RESETS traces, marginal histograms and
 * every analysis sum that is indexed by block labels, exactly as after bisbm_agg_merge; the numbering-free analysis calls (pair
 * scores, edge probabilities, co-assignment, fold-in, conditionals, partition distances) go on and average over (Ka, Kb).
 * k_min / k_max: per type, 1 <= k_min[t] <= k_max[t]; k_max NULL: min(n_t, 127); k_min NULL: (1, 1).  A split needs a spare
 * block of each type beside the chain's own in the kernel's state: k_max[0] + k_max[1] <= 254, and every chain must have ka +
 * kb <= 254 (BISBM_ERR_INVALID_ARG / BISBM_ERR_UNSUPPORTED).
 * Refused with a message and nothing changed: BISBM_RNG_MT19937_COMPAT and two-byte labels (BISBM_ERR_UNSUPPORTED); a clamp,
 * block constraints or block fields being set (a move renumbers blocks, as bisbm_agg_merge), replica exchange on, a population
 * in progress (bisbm_population_reset ends it), before bisbm_init / bisbm_shuffle (BISBM_ERR_STATE); beta not finite or <= 0,
 * k_min / k_max out of order (BISBM_ERR_INVALID_ARG).  moves = 0 is a no-op that zeroes accepted_out.
 * get_last: the last move of every chain (BISBM_ERR_STATE before the first call); get_total: per chain {splits proposed, splits
 * accepted, merges proposed, merges accepted} over the handle's lifetime. */
#define BISBM_SM_SPLIT 0u
#define BISBM_SM_MERGE 1u
#define BISBM_SM_EVALUATED 0u
#define BISBM_SM_SINGLETON 1u
#define BISBM_SM_AT_K_MAX 2u
#define BISBM_SM_AT_K_MIN 3u
#define BISBM_SM_NO_PAIR 4u
typedef struct bisbm_split_merge_record {
    uint32_t kind;     /* BISBM_SM_SPLIT / BISBM_SM_MERGE */
    uint32_t type;     /* 0: a, 1: b (BISBM_SM_NO_PAIR: 0) */
    uint32_t r, s;     /* global labels in the numbering before the move; split: s = the label away takes if accepted */
    uint32_t M;        /* members (BISBM_SM_SINGLETON: the block's size; other refusals: 0) */
    uint32_t refused;  /* BISBM_SM_EVALUATED, or why nothing was evaluated */
    double q_mant;     /* Q_fwd (split) / Q_rev (merge) */
    int32_t q_exp;
    uint32_t accepted;
    double dS, lnA, A, u_acc;
    uint32_t ka_before, kb_before, ka_after, kb_after;
} bisbm_split_merge_record;
int bisbm_split_merge_run(bisbm_handle h, uint64_t moves, uint32_t scans, double beta, const uint32_t *k_min /* 2, may be NULL */,
                          const uint32_t *k_max /* 2, may be NULL */, uint64_t *accepted_out /* n_chains, may be NULL */);
int bisbm_split_merge_get_last(bisbm_handle h, bisbm_split_merge_record *out /* n_chains */);
int bisbm_split_merge_get_total(bisbm_handle h, uint64_t *out /* n_chains x 4 */);
/* DIAGNOSTIC (tests and host replays; not needed to run the moves).  The group of its device entry that every chain lives in (0
 * on an entry whose chains are not grouped): two chains of one device entry with the same shape have the same group. */
int bisbm_split_merge_get_groups(bisbm_handle h, uint32_t *out /* n_chains */);
/* DIAGNOSTIC.  Host clock of the last bisbm_split_merge_run in ms, and the part of it spent forming the groups again (copying
 * chains, allocating groups, rebuilding block state); over several device entries the slowest entry's.  Either may be NULL. */
int bisbm_split_merge_get_timing(bisbm_handle h, double *call_ms, double *regroup_ms);
/* DIAGNOSTIC.  T(ka, kb) of step 5 as the library evaluates it (for a host that replays a move). */
int bisbm_split_merge_shape_term(bisbm_handle h, uint32_t ka, uint32_t kb, double *out);

/* Clamped nodes (no reference counterpart): one mask per handle, one byte per node; a non-zero byte means the node is CLAMPED
 * and no sampler changes its label, in any chain.  Partial labels, one side of a bipartite graph held, an incremental refit, or
 * a seed per block with the same label in every chain, which pins the block numbering (the raw histogram of the marginals is
 * then a marginal over chains without an alignment).  Only the nodes are held, not the edges: a clamped node counts in m, m_r,
 * n_r and eta and in every dS of its neighbours.  The other nodes are OPEN.  Philox mode and byte labels only.
 * set: the mask is copied to every device of the handle, beside the ascending lists of the open nodes of each type (n bytes
 * plus 4 bytes per open node and device); NULL or an all-zero mask clears the clamp.  Setting or clearing touches no chain
 * state: the clamp holds whatever labels every chain has at the time, and bisbm_set_memberships stays allowed under a clamp
 * (the caller's own act).  After a clear every call is bit for bit what a handle that never had a clamp does, and MH sweeps
 * run the production kernel again.  get: the mask as 0 / 1 bytes and the number of clamped nodes.
 *   1. MH SWEEPS (bisbm_anneal, bisbm_tempering_run, the MH part of the rounds): the step of a clamped node is not evaluated
 *      and the node stays.  In every counter it is a step that was not accepted: it counts in the n steps of the sweep and in
 *      the count of T < 1 steps of the early stop, never in `accepted`, and adds nothing to the running sum.  The Philox draws
 *      of a step are keyed by its position in the sweep, so no other step's draws move: the clamped chain equals the unclamped
 *      chain up to the first step at which the unclamped chain moves a clamped node.  Skipping is legal because a sweep is a
 *      composition of single-node kernels each of which leaves exp(-beta S) invariant; leaving some out leaves a composition
 *      of kernels that keep the distribution restricted to the states that agree with the clamped labels.  A handle the
 *      production kernel serves keeps it under a clamp (its held instances, two steps per pass at most), unless most of its
 *      nodes are clamped: then the generic kernel, which skips a clamped step outright, is the faster one and runs (README.md).
 *   2. HEAT-BATH SWEEPS AND POLISHING (bisbm_heatbath_run): a clamped node is a node that is not free: it stays, no draw is
 *      used, and it is counted as such a node is.  The position in the sweep of every other node, and with it its draw, is
 *      unchanged.  With beta = +inf and stop_when_settled the end state is a local minimum over the moves of the OPEN nodes
 *      only.  The work of a sweep follows the open nodes: a chunk of 64 positions without an open node reads no row.
 *   3. PAIR RESHUFFLES (bisbm_reshuffle_run): step 3 becomes "the nodes of that type whose label is r or s and that are not
 *      clamped, in ascending id"; everything indexed by the member number -- the launch bits, the uniforms of the scans, the
 *      forced first and last launch label, M < 2 a counted no-op (now possible: the record holds the pair and M, everything
 *      else 0) -- is unchanged in form.  The pair is still drawn without a look at the state.  The clamped nodes of r and s
 *      stay in n_r, m_r and m, so a member's dS sees them and its FREE test (n_r[c] > 1) counts them.  Detailed balance holds
 *      as before: which nodes are members does not depend on how the members are divided.
 *   4. SHUFFLE (bisbm_shuffle): the labels of the open nodes of each type are permuted among themselves.  For type t with F the
 *      ascending list of its open nodes: f = the keyed Feistel permutation of bisbm_shuffle (same purpose 3, same index
 *      (t << 32) | epoch, same chain key) on the domain |F|, and new[F[i]] = old[F[f(i)]] -- the unclamped shuffle of the
 *      compacted label vector, so block sizes are preserved.  |F| <= 1 leaves the type as it is.  The epoch advances as always.
 *   5. REPLICA EXCHANGE, ROUNDS, POPULATION ANNEALING: the mask is the handle's, so every kernel of a round is handed it; chain c
 *      stays, bit for bit, the chain that a one-chain handle of its global id with the same mask runs through the same moves at
 *      the temperatures it held.  bisbm_population_resample copies whole chains, so the clamped labels of the source travel
 *      with the copy: a population is meant to share its clamped labels.
 * The analysis calls, the traces, the partition distances and the block summaries only read chain state and are unchanged.
 * Served: several devices behind one handle.  Refused, with a message and nothing changed: BISBM_RNG_MT19937_COMPAT (that
 * mode exists for parity with the reference, which has no clamp) and two-byte labels BISBM_ERR_UNSUPPORTED; chains grouped by
 * shape BISBM_ERR_STATE; mask_out and n_clamped_out both NULL is allowed.  While a non-empty clamp is set bisbm_agg_merge and
 * bisbm_agg_merge_total are BISBM_ERR_STATE (a merge or split renumbers blocks; bisbm_clamp_set(h, NULL) first).
 * Out of scope: a mask per chain, mt19937-compat arithmetic, wide handles, chains grouped by shape, clamped MH sweeps in the
 * production kernel, constraints other than "stays". */
int bisbm_clamp_set(bisbm_handle h, const uint8_t *mask /* n; non-zero = held; NULL clears */);
int bisbm_clamp_get(bisbm_handle h, uint8_t *mask_out /* n, may be NULL */, uint64_t *n_clamped_out /* may be NULL */);

/* Block constraints (no reference counterpart; graph-tool's pclabel / bfield): where a clamp says "this node stays", a
 * constraint says "this node is in one of these blocks".  A taxonomy for some nodes, one side of a partly curated graph, the
 * refinement of a coarse fit inside its own blocks (every block gets children, a node chooses among the children of its
 * parent).  One set per handle: a class id per node, class_of_node[n], one byte each, at most 256 classes, and a table
 * allowed[n_classes][ka + kb], one byte per cell, non-zero meaning allowed.  Node v may sit in block s iff
 * allowed[class_of_node[v]][s] is set and s is of v's type; A_v is the set of those blocks, and the table's entries for blocks
 * of the other type are ignored.  Classes that allow disjoint sets break the label symmetry between those sets in every chain
 * without pinning a node.  Philox mode and byte labels only.
 * set: validates before anything changes.  n_classes <= 256 and every class id < n_classes, else BISBM_ERR_INVALID_ARG.  Then,
 * on every device of the handle, a kernel looks at every node's current label in every chain: a label outside A_v is
 * BISBM_ERR_STATE with a message naming the global chain id, the node and the label of the first offender.  A refusal leaves
 * the constraints that were in place on every device.  Each device keeps the class bytes (n bytes), the table as eight 32-bit
 * words per class (at most 8 KiB) and one list of the open nodes sorted by (type, class, id) (4 bytes per open node), which is
 * rebuilt whenever the clamp or the constraints change.  n_classes = 0 or a NULL pointer clears.  A table under which every
 * A_v is all blocks of v's type IS "no constraints" and is stored as a clear: the kernels are handed no table, MH sweeps run
 * the production kernel, every call is bit for bit that of a handle that never had constraints, and get reports 0 classes.
 * get: n_classes, the class bytes and the table as 0 / 1 bytes (each pointer may be NULL; without constraints 0 classes, all
 * class bytes 0, allowed_out untouched).
 *   1. MH SWEEPS: the proposal is drawn exactly as always.  If its target s is of the node's type, is not the node's own
 *      block and is not in A_v, the step is not evaluated; in every counter it is a step that was not accepted, as the step of
 *      a clamped node is: it counts in the n steps of the sweep and in the early stop's count of T < 1 steps, never in
 *      `accepted`, and adds nothing to the running sum.  A proposal of the node's own block is always allowed.  The Hastings
 *      ratio of a move inside A_v is unchanged: refusing the proposals that leave the admissible set restricts a chain that is
 *      in detailed balance with exp(-beta S) to that set, and a restriction of a reversible chain to a subset, with the refused
 *      mass put on staying, is reversible with respect to the restricted distribution.  The draws of a
 *      step are keyed by its position, so a refusal moves nobody else's draws: the constrained chain equals the unconstrained
 *      one up to the first step at which the unconstrained chain accepts a target outside A_v.  A handle the production kernel
 *      serves keeps it under constraints (its held instances, two steps per pass at most: README.md).
 *   2. HEAT-BATH SWEEPS AND POLISHING: a node with |A_v| = 1 is held exactly as a clamped node is -- in the chunk header, no
 *      row read, no draw used.  Otherwise the row is restricted to A_v: mn = the minimum of dS_s over s in A_v (the 0 at r
 *      included), w_s = exp(-beta (dS_s - mn)) for s in A_v and exactly 0.0 for s outside; Z, P, C_s and the choice are as
 *      without constraints, in the same order (a +0.0 term keeps every bit).  Greedy: the lowest s in A_v that attains mn, and
 *      only if mn < 0.  With stop_when_settled the end state is a local minimum over the admissible moves.
 *   3. PAIR RESHUFFLES: a member is an open node of r or s whose class allows BOTH r and s.  Everything indexed by the member
 *      number is unchanged in form.  A non-member is treated exactly as a clamped node: it stays in n_r, m_r and m, the FREE
 *      test counts it, and M < 2 is the counted no-op.  The member set depends on the union of the two blocks and on the
 *      constraints, not on how the union is divided, so the move and its reverse see the same members: detailed balance holds
 *      as under a clamp.
 *   4. SHUFFLE: the labels of the open nodes of each (type, class) are permuted among themselves (equal class: equal A_v, so
 *      every label stays admissible and block sizes are preserved).  For type t and class c with F the ascending list of the
 *      open nodes of that type and class: f = the keyed Feistel permutation of bisbm_shuffle on the domain |F| -- same
 *      purpose 3, same index (t << 32) | epoch, same chain id -- under the Philox key seed + c * 0x9E3779B97F4A7C15 (mod
 *      2^64), and new[F[i]] = old[F[f(i)]].  Class 0 has the key of the plain shuffle: with one class this is the clamped or
 *      unclamped shuffle, bit for bit.
 *   5. REPLICA EXCHANGE, ROUNDS, POPULATION ANNEALING: the constraints are the handle's, so every kernel of a round is handed
 *      them; chain c stays, bit for bit, the chain that a one-chain handle of its global id with the same constraints runs.  A
 *      resampled slot carries its ancestor's labels, which were admissible.
 * Constraints and a clamp are independent and may both be set.  bisbm_set_memberships under constraints refuses a vector
 * that violates them (BISBM_ERR_INVALID_ARG, naming the first node).  The analysis calls only read state and are unchanged;
 * bisbm_conditionals_* keeps reporting the UNRESTRICTED row
 * (unless bisbm_held_conditionals_set is on: "Held conditionals").  Refused, with a message and nothing changed:
 * BISBM_RNG_MT19937_COMPAT and two-byte labels BISBM_ERR_UNSUPPORTED; chains grouped by shape BISBM_ERR_STATE.  While
 * constraints are set bisbm_agg_merge and bisbm_agg_merge_total are BISBM_ERR_STATE (bisbm_constraints_set(h, 0, NULL, NULL)
 * first).
 * Out of scope: a table per chain, constraints in the production kernel (DESIGN.md section 26's follow-up serves both),
 * restricted rows in the plain bisbm_conditionals_* row (the opt-in is "Held conditionals"), mt19937-compat arithmetic, wide handles, chains grouped by shape, merges or splits
 * under constraints.  (Soft priors over blocks: "Block fields" below.) */
int bisbm_constraints_set(bisbm_handle h, uint32_t n_classes, const uint8_t *class_of_node /* n */,
                          const uint8_t *allowed /* n_classes * (ka + kb) */);   /* 0 / NULL clears */
int bisbm_constraints_get(bisbm_handle h, uint32_t *n_classes_out, uint8_t *class_of_node_out, uint8_t *allowed_out);

/* Block fields (no reference counterpart; graph-tool's bfield): soft per-node priors over blocks.  Where constraints forbid, a
 * field prefers: labels that are partly wrong, a taxonomy that is a tendency, node metadata, the children of a coarse fit a node
 * should prefer but may leave.  One set per handle, shaped like the constraints and independent of them and of the clamp (all
 * three may be set at once): a class byte per node, class_of_node[n] (its own vector, at most 256 classes), and a table
 * field[n_classes][ka + kb] of f64 energies phi in nats; a row's entries for blocks of the other type are ignored.  With
 * Phi(b) = sum_v phi[class(v)][b_v] and E = S + Phi every sampler targets exp(-beta E) instead of exp(-beta S): a node's prior
 * weight for block s is exp(-phi_s), and beta tempers the field together with the description length.  Philox mode and byte
 * labels only.
 * set: validates before anything changes.  n_classes <= 256, every class id < n_classes and every entry finite, else
 * BISBM_ERR_INVALID_ARG naming class and block (for +inf the message names bisbm_constraints_set, the way to forbid a block).  A
 * refusal leaves the fields that were in place on every device.  n_classes = 0 or a NULL pointer clears, and a table whose
 * entries are all +-0.0 IS "no fields" and is stored as a clear: the kernels are handed null pointers, MH sweeps run the
 * unfielded kernels again, every call is bit for bit that of a handle that never had fields, and get reports 0 classes.  Each
 * device keeps the n class bytes and the table in global memory (at most 512 KiB of table).
 * get: n_classes, the class bytes and the table as given (each pointer may be NULL; without fields 0 classes, all class bytes 0,
 * field_out untouched).
 * Wherever a sampler uses a node's dS(v: r -> s) it uses dE = dS + (f[s] - f[r]), f the row of v's class: the difference is
 * formed first, then there is exactly one f64 add onto the dS the kernel already has.  No draw, no Philox index and no order of
 * any sum changes.
 *   1. MH SWEEPS: the add follows the evaluation of the step's dS, before the accept line, whose form stays.  A proposal of the
 *      node's own block keeps 0, a target of the other type or barred by the constraints keeps its verdict.  Proposal and
 *      Hastings factor are untouched: the step is the Metropolis-Hastings step for exp(-beta E) with the same q.  While fields
 *      are set the sweeps of a handle the production kernel serves run its fielded instances, one step per pass
 *      (bisbm_last_pass_steps reports 1, bisbm_last_sweep_route BISBM_ROUTE_PRODUCTION | BISBM_ROUTE_FIELDS), with a clamp and
 *      constraints beside the field in the same launch; the chain is, integer for integer, the generic kernel's
 *      (BISBM_FIELD_FAST=0 in the environment pins that kernel for fielded handles; README.md).
 *   2. HEAT-BATH SWEEPS AND POLISHING: the row entry of target s != r is (((acc + tail1) + tail2) + tail3) + (f[s] - f[r]) and
 *      stays 0 at r; minimum, weights, Z, C_s, the greedy rule and the constraints' restriction follow as they are.  Polishing
 *      certifies a minimum of E over the open admissible moves.
 *   3. PAIR RESHUFFLES: a member's dS_o gets the same add before it enters the scan's weights and the pass's sum, so Q, dS_fwd,
 *      dS_rev, A and the record are those of the move under E; the record's layout does not change.
 *   4. RUNNING SUM: while fields are set bisbm_get_cum_dS advances by the dE of what was accepted, so between two reads
 *      delta cum = delta S + delta Phi.  Setting or clearing fields does not touch the sum.
 *   5. REPLICA EXCHANGE: the swap test uses E_a - E_b, E = the description length + Phi (one add per chain).
 *   6. POPULATION ANNEALING: the resampling weights and the ln Z increment use E per chain, S[c] + Phi[c] added on the host before
 *      bisbm_population_offspring, which is unchanged: the reported evidence is that of the tilted target exp(-beta E).
 *   7. bisbm_fields_energy: Phi of every chain, defined so that a host loop gives the same bits: the integer histogram
 *      count[class][block] over the nodes, then Phi = the sum over (class ascending, block ascending) of (double) count * phi,
 *      added sequentially from 0.0, zero counts skipped (a label is a block of its node's type, so only a node's own type's
 *      range is ever counted).  Without fields every Phi is 0.0.  The exchange and the resampling use this same code.
 * Unchanged: bisbm_entropy stays the description length, and every "lowest description length" choice with it (alignment
 * reference, a mode's best chain); every analysis call; bisbm_conditionals_* keeps reporting the model's row (the heat-bath row
 * is that row plus the field) (unless bisbm_held_conditionals_set is on: "Held conditionals"); the shuffle (an initialiser, not a sampler); bisbm_set_memberships.  Refused, with a message and
 * nothing changed: BISBM_RNG_MT19937_COMPAT and two-byte labels BISBM_ERR_UNSUPPORTED; chains grouped by shape BISBM_ERR_STATE.
 * While fields are set bisbm_agg_merge and bisbm_agg_merge_total are BISBM_ERR_STATE (bisbm_fields_set(h, 0, NULL, NULL) first).
 * Out of scope: fields in the production kernel, a table per chain, more than 256 distinct rows, mt19937-compat arithmetic,
 * wide handles, chains grouped by shape, merges or splits under fields, the field inside the plain bisbm_conditionals_* row (the
 * opt-in is "Held conditionals") and inside the fold-in posteriors, learning the field from metadata. */
int bisbm_fields_set(bisbm_handle h, uint32_t n_classes, const uint8_t *class_of_node /* n */,
                     const double *field /* n_classes * (ka + kb) */);   /* 0 / NULL clears */
int bisbm_fields_get(bisbm_handle h, uint32_t *n_classes_out, uint8_t *class_of_node_out, double *field_out);
int bisbm_fields_energy(bisbm_handle h, double *out /* n_chains */);

/* Partition distances and posterior modes (no reference counterpart: the reference keeps one partition).  How many different
 * answers did the chains find, which chains agree, how much of the pool sits in each answer: the all-pairs comparison of the
 * chains' partitions on the device, and a small deterministic grouping on the host.
 * Labels: chains c and d have global labels over the n nodes, type-a blocks 0 .. ka-1, type-b blocks ka .. ka+kb-1, each chain
 * with its own ka, kb (chains of different shapes are compared as they are).
 * Contingency counts: n_rs = #{v : b^c_v = r and b^d_v = s}, a_r = sum_s n_rs, b_s = sum_r n_rs; cells that mix the two types
 * are zero by construction.
 * Variation of information, in nats: VI(c, d) = ( sum_r a_r ln a_r + sum_s b_s ln b_s - 2 sum_rs n_rs ln n_rs ) / n, with
 * 0 ln 0 = 0, all arithmetic in f64; a rounding result below 0 is returned as 0.0; VI(c, c) is exactly 0.0; the matrix is
 * exactly symmetric (each pair is computed once and mirrored).
 * Partition entropy: H(c) = ln n - ( sum_r a_r ln a_r ) / n.  (NMI follows from VI and the two entropies.)
 * The counts are integers and do not depend on the order of the adds; each of the three sums is added in an order fixed by the
 * selection and the shapes (one wavefront per table: lane l adds cells l, l + 64, ... in turn, then a butterfly over the
 * lanes), so the same handle and the same call give the same bits.
 * Modes: a pure host function of a symmetric m x m matrix and a threshold tau >= 0.  i and j are in one mode when a path of
 * pairs with VI <= tau joins them (single linkage); modes are numbered by their lowest selected index; the medoid of a mode is
 * the member with the least sum of VI to the other members (ties -> the lowest index).  tau has no default: it is the caller's
 * resolution.
 *
 * The calls read the chains' labels only: random streams, running sums, the marginal histogram and the pair scores are left
 * untouched.  Served: both RNG modes, chains grouped by shape after bisbm_agg_merge_total, several devices behind one handle
 * (the first device computes; the label rows of selected chains on other devices are copied to it, peer copy or through the
 * host; the result equals a single-device handle's bit for bit), replica exchange on (every selected chain is compared
 * whatever its rung).  Refused: byte labels only (a wide handle, more than 256 blocks: BISBM_ERR_UNSUPPORTED); BISBM_ERR_STATE
 * before bisbm_init / bisbm_shuffle; BISBM_ERR_INVALID_ARG for a chain out of range or listed twice (bisbm_last_error names it).
 * The tables of all pairs are never held together.  Device scratch of a call with m selected chains, the largest shape among
 * them kaM + kbM: 16 m bytes of descriptors, 8 m^2 + 8 m bytes of sums, 8 bytes per tile of chain pairs (a tile is up to 4 x 4
 * chains), n rounded up to 256 bytes per selected chain that lives on another device, and -- only when the pairs are too few to
 * fill the device with one tile per workgroup, or a table does not fit the LDS -- integer tables of 4 (kaM^2 + kbM^2) bytes per
 * pair for as many tiles as fit 256 MiB (at least one), run in as many launches as that takes.  Scratch that cannot be
 * allocated is BISBM_ERR_HIP with the size in the message; nothing is skipped or subsampled.
 *
 * distances: chains = NULL selects all chains (n_sel must be n_chains).  vi_out[n_sel * n_sel] and h_out[n_sel] in the order
 *   of the selection; either may be NULL.
 * contingency: the table of one pair, (ka_c + kb_c) x (ka_d + kb_d), row-major, indexed by global labels.
 * modes: mode_out[m]; medoid_out (may be NULL) m entries of which the first *n_modes_out are used, as indices 0 .. m-1.
 *   BISBM_ERR_INVALID_ARG for m = 0, a negative or NaN threshold, a NaN or asymmetric entry.  Needs no device. */
int bisbm_partition_distances(bisbm_handle h, uint32_t n_sel, const uint32_t *chains, double *vi_out, double *h_out);
int bisbm_partition_contingency(bisbm_handle h, uint32_t c, uint32_t d, uint32_t *table_out);
int bisbm_partition_modes(uint32_t m, const double *vi, double threshold, uint32_t *mode_out, uint32_t *medoid_out,
                          uint32_t *n_modes_out);

/* Distances to reference partitions: the selected chains against n_refs partitions of the same n nodes that are not chains -- a
 * planted or ground-truth partition, the result of an earlier run, a medoid saved to disk.  The definitions are those above
 * with the chain as the row partition and the reference as the column partition: vi_out[i * n_refs + g] = VI(chain i of the
 * selection, reference g), h_ref_out[g] = H(reference g) (may be NULL).  Reference g has a shape of its own: its type-a labels
 * lie in [0, ref_ka[g]), its type-b labels in [ref_ka[g], ref_ka[g] + ref_kb[g]), ref_ka[g] + ref_kb[g] <= 256;
 * ref_labels[g * n + v] on the host.
 * The three sums of a VI are each added by one wavefront in the fixed order described above, so the same handle and the same
 * call give the same bits; they are added in different orders, though, so a reference that equals a chain's labels gives a VI
 * of rounding size (below 1e-10 for n < 1e5) and not necessarily exactly 0.0, and VI(c, labels of d) agrees with
 * bisbm_partition_distances' VI(c, d) to that size, not to the bit.  A negative rounding result is returned as 0.0.
 * Served and refused as bisbm_partition_distances is (labels are only read; both RNG modes, chains grouped by shape, several
 * devices with the first one computing, replica exchange on; wide handles BISBM_ERR_UNSUPPORTED, BISBM_ERR_STATE before
 * bisbm_init / bisbm_shuffle, a chain out of range or listed twice BISBM_ERR_INVALID_ARG); also BISBM_ERR_INVALID_ARG:
 * n_refs = 0, a NULL pointer other than chains and h_ref_out, a reference of more than 256 blocks, a reference label outside
 * its type's range (bisbm_last_error names the reference and the node).
 * A workgroup counts a tile of up to 4 chains x 4 references.  Device scratch of a call with m chains, r references, largest
 * shapes kaM + kbM (chains) and kaR + kbR (references): 16 (m + r) bytes of descriptors, 8 m r + 8 (m + r) bytes of sums, 8
 * bytes per tile, r rows of n rounded up to 256 bytes, staged rows of chains on other devices as above, and -- only when the
 * tiles are too few to fill the device or a table does not fit the LDS -- integer tables of 4 (kaM kaR + kbM kbR) bytes per
 * (chain, reference) for as many tiles as fit 256 MiB (at least one). */
int bisbm_partition_distances_to(bisbm_handle h, uint32_t n_sel, const uint32_t *chains /* NULL: all */, uint32_t n_refs,
                                 const uint32_t *ref_labels /* n_refs * n, host */, const uint32_t *ref_ka,
                                 const uint32_t *ref_kb /* n_refs each */, double *vi_out /* n_sel * n_refs, row = chain */,
                                 double *h_ref_out /* n_refs, may be NULL */);

/* Mode-resolved marginals (no reference counterpart).  Chains at T = 1 settle in different posterior modes
 * (bisbm_partition_distances / bisbm_partition_modes tell which).  A chain of another mode has no good permutation onto one
 * common reference, so the pooled aligned histogram smears it over the columns and its MAP describes no mode.  With modes set
 * there is one histogram PER MODE, each mode aligned to a reference of its own: "the pool holds k answers; here is each one
 * and how sure we are of every node in it".  Off (the default) nothing else in this file behaves differently.
 *
 * set_modes: chain c (index in the handle) is counted into mode mode_of_chain[c] in 0 .. n_modes-1; BISBM_MODE_NONE: the chain
 *   is not counted.  n_modes = 0 turns the feature off (the pointer may be NULL) and frees the histograms.  Every call drops
 *   all mode references, the caller's too.  BISBM_ERR_INVALID_ARG: a label >= n_modes that is not BISBM_MODE_NONE, a mode
 *   without any chain (bisbm_last_error names the chain / the mode).  BISBM_ERR_STATE: the internal histogram, pooled or per
 *   mode, holds samples (bisbm_marginals_reset first: the rule of bisbm_marginals_set_alignment); replica exchange is on
 *   (chains trade temperatures, so a chain's membership means nothing across rungs; likewise bisbm_tempering_set with L > 0
 *   is BISBM_ERR_STATE while modes are set); the chains are grouped by shape (after bisbm_agg_merge_total).
 * A sample while modes are set is bisbm_marginals_accumulate(h, NULL): every counted chain is counted through its permutation
 *   onto ITS MODE's reference -- exactly the procedure of "Label alignment before pooling": overlap table per type, the same
 *   assignment solver, the same tie rule -- into histogram g = mode_of_chain[c], and terms[g] grows by the number of chains
 *   counted into g.  bisbm_marginals_set_alignment is neither consulted nor changed.  A caller's device_counts is
 *   BISBM_ERR_UNSUPPORTED; a wide handle is BISBM_ERR_UNSUPPORTED at the sample, chains grouped by shape BISBM_ERR_STATE.
 * References: the caller's (set_mode_reference: n labels validated as bisbm_marginals_set_reference does; NULL clears), or
 *   else -- taken at the first sample after a reset -- the labels of the mode's member chain of the lowest bisbm_entropy (ties
 *   -> the lowest chain).  get_mode_reference: the labels and the chain they came from (-1: the caller's); BISBM_ERR_STATE
 *   while the mode has none.  The references live with the handle: over several devices a mode may span devices and its
 *   reference chain may live on another device than the one counting.
 * get_modes: the assignment, per mode the reference chain (-1: set by the caller, -2: none yet) and terms; any pointer may be
 *   NULL; *n_modes = 0 and nothing else written while the feature is off.
 * While modes are set bisbm_marginals_get, bisbm_marginals_map, bisbm_marginals_set_reference and
 *   bisbm_marginals_get_reference are BISBM_ERR_STATE with a message that names the per-mode call: a sum of histograms in
 *   different numberings is not a marginal.  bisbm_marginals_get_alignment keeps working: the chain's permutation onto its
 *   mode's reference at the last sample (an uncounted chain: BISBM_ERR_STATE).
 * bisbm_marginals_reset zeroes every mode's histogram and terms and drops library-chosen references; the assignment and the
 *   caller's references stay.  After a merge or split that changes the block counts the histograms start afresh at the next
 *   sample and library-chosen references are taken afresh; a caller's stale reference is BISBM_ERR_STATE ("set it again").
 * get_mode: the histogram of one mode, n * kmax counters laid out as bisbm_marginals_get's (several devices: the devices'
 *   slices added on the host).
 * map_mode: labels_out[v] = the most frequent block of v in the mode (ties -> the lowest block), in the numbering of the
 *   mode's reference; top_out[v] (may be NULL) = that block's count, so top_out[v] / terms[mode] says how settled the node is
 *   within the mode.  Several devices: the slices of the mode are added on the first device, bit for bit what one device with
 *   all the chains gives.  BISBM_ERR_STATE before the mode's first sample.
 * Memory: every device holds n_modes * n * kmax * 4 bytes (128 MB per mode at n = 1e6, kmax = 32); an allocation failure is
 *   BISBM_ERR_HIP with the size in the message.  There is no hidden cap and nothing is subsampled. */
#define BISBM_MODE_NONE 0xffffffffu
int bisbm_marginals_set_modes(bisbm_handle h, uint32_t n_modes, const uint32_t *mode_of_chain /* n_chains */);
int bisbm_marginals_get_modes(bisbm_handle h, uint32_t *n_modes, uint32_t *mode_of_chain /* n_chains */,
                              int64_t *ref_chain /* n_modes */, uint64_t *terms /* n_modes */);
int bisbm_marginals_set_mode_reference(bisbm_handle h, uint32_t mode, const uint32_t *labels /* n, NULL clears */);
int bisbm_marginals_get_mode_reference(bisbm_handle h, uint32_t mode, uint32_t *labels_out, int64_t *chain_out);
int bisbm_marginals_get_mode(bisbm_handle h, uint32_t mode, uint32_t *counts_out /* n*kmax, host */);
int bisbm_marginals_map_mode(bisbm_handle h, uint32_t mode, uint32_t *labels_out /* n */, uint32_t *top_out /* n, may be NULL */);

/* Anchored modes (no reference counterpart): mode-resolved marginals whose assignment is taken afresh at every sample, by
 * distance to one anchor partition per mode.  A chain that hops to another mode is counted there from then on, replica
 * exchange is served, and a mode's weight is the share of samples that fall into it.
 * set_mode_anchors: n_modes histograms and no fixed assignment; anchor g (anchor_labels[g * n + v], validated as
 *   bisbm_marginals_set_reference validates, against the handle's common shape) is also mode g's alignment reference, as a
 *   caller's reference (ref_chain = -1).  threshold >= 0, +inf allowed ("always the nearest"); NaN or negative:
 *   BISBM_ERR_INVALID_ARG.  n_modes = 0 turns the feature off as set_modes(0) does.  BISBM_ERR_STATE as for set_modes (the
 *   histogram holds samples; chains grouped by shape) except that replica exchange may be on, and bisbm_tempering_set with
 *   L > 0 is allowed while anchors are set.  bisbm_marginals_set_mode_reference is BISBM_ERR_STATE while anchors are set (the
 *   anchors are the references).  set_modes replaces anchors; set_mode_anchors replaces a static assignment.
 * A sample is bisbm_marginals_accumulate(h, NULL).  The counted chains are every chain, or, with replica exchange on, the
 *   chains on rung 0 at that moment.  For every counted chain c and anchor g, VI(c, g) is computed as
 *   bisbm_partition_distances_to computes it; g* is the anchor of least VI (ties -> the lowest g).  If VI(c, g*) <= threshold
 *   the chain is counted into histogram g* through its permutation onto anchor g* (the pipeline of static modes), terms[g*]
 *   and visits[c][g*] grow by one; otherwise it is not counted and `unassigned` grows by one.  `samples` grows by one per call.
 *   A wide handle and a caller's device_counts are BISBM_ERR_UNSUPPORTED.  After a merge or split that changes the block
 *   counts the next sample is BISBM_ERR_STATE ("set the anchors again").
 * bisbm_marginals_get_modes returns the last sample's assignment (BISBM_MODE_NONE: not counted or unassigned; all of them
 *   before the first sample) and terms.  get_mode_assignment: vi_out[n_chains * n_modes] of the last sample (NaN rows: chains
 *   that were not counted, every row before the first sample), the running visits_out[n_chains * n_modes], unassigned and
 *   samples; any pointer may be NULL; BISBM_ERR_STATE while no anchors are set.  get_mode, map_mode, get_mode_reference and
 *   bisbm_marginals_get_alignment work as with static modes (map_mode of a mode with terms = 0: BISBM_ERR_STATE).
 * bisbm_marginals_reset zeroes the histograms, terms, visits, unassigned and samples; anchors and threshold stay.
 * Several devices: the anchors are replicated, every device assigns and counts its own chains, terms / visits / unassigned live
 *   with the handle; the results equal those of one device with all the chains bit for bit.
 * Memory: as for static modes, plus per device n_modes anchor rows of the label stride (n rounded up to 256 bytes) and the
 *   scratch of bisbm_partition_distances_to for the device's counted chains x n_modes (no reference rows of its own); on the
 *   host 16 n_chains n_modes bytes of VI and visits and 4 n n_modes bytes of anchors. */
int bisbm_marginals_set_mode_anchors(bisbm_handle h, uint32_t n_modes, const uint32_t *anchor_labels /* n_modes * n */,
                                     double threshold);
int bisbm_marginals_get_mode_assignment(bisbm_handle h, double *vi_out /* n_chains * n_modes */,
                                        uint64_t *visits_out /* n_chains * n_modes */, uint64_t *unassigned_out,
                                        uint64_t *samples_out);

/* Block summaries (no reference counterpart): the block-level companion of the aligned node marginals.  Which groups of type-a
 * nodes attach to which groups of type-b nodes, how large every group is and how firmly the pool agrees on it: the mean and
 * the exact spread, over the counted chain samples, of the ka x kb edge-count matrix, the block sizes and the block degrees,
 * in the numbering of the node marginals taken in the same samples.  Off (the default) nothing is launched and nothing else
 * in this file behaves differently.
 *
 * A chain's block state on the device is d_m, the ka x kb quadrant (m_c[a][b] = edges between type-a block a and type-b block
 * ka + b; bisbm_get_block_state returns it mirrored into K x K), and n_r_c, m_r_c of K = ka + kb entries, all int32.
 * With the sums on, every ALIGNED sample of bisbm_marginals_accumulate also adds, for every chain c the sample counts into
 * mode g (mode 0: the pooled histogram) with pi the global-label permutation the sample just computed for c onto g's
 * reference (bisbm_marginals_get_alignment returns it):
 *     E[g][pi(a)][pi(ka + b) - ka] += m_c[a][b]   for a < ka, b < kb     edges between the aligned blocks
 *     N[g][pi(r)] += n_r_c[r]                     for r < K              block sizes
 *     D[g][pi(r)] += m_r_c[r]                     for r < K              block degrees
 *     terms[g] += 1
 * Every cell keeps three uint64 accumulators: sum adds x, sq_lo adds (x*x) & 0xffffffff, sq_hi adds (x*x) >> 32.  x < 2^31,
 * so the sum of squares is sq_hi * 2^32 + sq_lo exactly, with no carry between the words, and nothing overflows while a mode
 * holds at most 2^32 chain samples: the accumulate call is BISBM_ERR_STATE, before anything is counted, once a mode's terms
 * would pass 2^32.  Everything is an integer and every add is associative: the words depend on no thread order, on no split
 * of the chains over workgroups, on no number of device entries and on no atomics; a plain loop reproduces every word.
 * The counted chains are exactly those the node histogram of the same sample counts: all chains; under replica exchange the
 * chains on rung 0 now; with static modes a mode's members (BISBM_MODE_NONE chains are in none); with anchored modes the
 * chains within the threshold, each in its nearest anchor's mode (unassigned chains add nowhere).
 *
 * set: what = 0 turns the feature off and frees its buffers; BISBM_BLOCK_SUMS keeps the sums; BISBM_BLOCK_SUMS |
 *   BISBM_BLOCK_KEEP_LAST also keeps every counted chain's aligned tables of the last sample (4 bytes per counted chain and
 *   cell).  Every call zeroes the sums.  Anything else: BISBM_ERR_INVALID_ARG.
 * The sums live and die with the histogram they accompany: bisbm_marginals_reset zeroes them, and whatever starts the
 *   histograms afresh starts them afresh too (a merge or split that changes the block counts, bisbm_marginals_set_modes,
 *   bisbm_marginals_set_mode_anchors).  They are always the library's own: a caller's device_counts does not move them.
 * get: mode 0 for the pooled histogram, the mode otherwise.  terms, and the planes sum, sq_lo, sq_hi one after the other:
 *   e[3 * ka * kb] (cell (R, S) at R * kb + S), n[3 * K], d[3 * K]; any pointer may be NULL.  All zero before the first sample
 *   and after a change of the block counts.  BISBM_ERR_STATE while the sums are off, BISBM_ERR_INVALID_ARG for a mode that does
 *   not exist.  Several devices: every device keeps the sums of its own chains and the getter adds them on the host; integers
 *   make that the bits of one handle with all the chains.
 * get_last: the aligned tables of `chain` at the last sample, e[ka * kb], n_r[K], m_r[K], and the mode it was counted into.
 *   BISBM_ERR_STATE without BISBM_BLOCK_KEEP_LAST, before a sample, and for a chain the last sample did not count.
 * A sample that is not aligned (BISBM_ALIGN_NONE and no modes) while the sums are on: bisbm_marginals_accumulate is
 *   BISBM_ERR_STATE with a message that names bisbm_marginals_set_alignment, before anything is counted -- raw labels of
 *   several chains share no numbering.  What the aligned sample itself refuses stays refused by it: a wide handle, chains of
 *   different shapes, grouped chains under modes.
 * Memory per device: 24 bytes per mode and cell (ka * kb + 2 K cells), plus the kept tables.
 * Out of scope: unaligned samples, two-byte labels, pooling over processes, quantiles (KEEP_LAST hands a caller the per-chain
 *   tables for that), cross-moments between cells, eta. */
#define BISBM_BLOCK_SUMS 1u      /* keep the sums */
#define BISBM_BLOCK_KEEP_LAST 2u /* also keep every counted chain's aligned tables of the last sample */
int bisbm_block_sums_set(bisbm_handle h, uint32_t what);
int bisbm_block_sums_get(bisbm_handle h, uint32_t mode, uint64_t *terms, uint64_t *e /* 3*ka*kb: sum, sq_lo, sq_hi planes */,
                         uint64_t *n /* 3*K */, uint64_t *d /* 3*K */);
int bisbm_block_sums_get_last(bisbm_handle h, uint32_t chain, uint32_t *mode_out, int32_t *e /* ka*kb */, int32_t *n_r /* K */,
                              int32_t *m_r /* K */);

/* Chain traces (no reference counterpart: the reference keeps no history).  Every other analysis here compares chains with each
 * other or with a reference; this one compares a chain with its own past.  How many sweeps until the partition has forgotten
 * where it was, how many independent samples did a run give, do the chains agree on the description length: every chain keeps a
 * ring of snapshots of its own partition on the device, a record computes the label-invariant distance between now and every
 * held lag and appends to the description-length series, and a small host routine gives integrated autocorrelation times and
 * split-R-hat.
 *
 * set: every device of the handle allocates a ring of `depth` snapshots of its own chains' label rows: depth x chains of the
 *   device x label stride (n rounded up to 256) bytes on the device, and 8 bytes per (slot, chain) on the host for the cached
 *   size sum.  depth = 0 frees everything.  depth > 1024: BISBM_ERR_INVALID_ARG.  A failed allocation is BISBM_ERR_HIP with the
 *   size in the message; nothing is capped or subsampled.  Calling it again replaces the ring and forgets everything.
 *   BISBM_ERR_UNSUPPORTED while the handle holds two-byte labels.
 * record: one record for every chain c of the handle (with replica exchange on, every chain whatever its rung):
 *   1. S_c is the double bisbm_entropy returns; H_c = ln n - A_c / n with A_c = sum_r a_r ln a_r exactly as
 *      bisbm_partition_distances' h_out computes it (the same kernel: H is bit-equal to that h_out).  Both are appended to
 *      host-side series, 16 bytes per (record, chain).
 *   2. For every held age a = 1 ... min(depth, records so far) there is a snapshot b' of chain c taken a records ago.  The
 *      contingency table of (labels now, b') is counted in the layout of the partition distances (type a at r * ka + s, type b
 *      at ka * ka + r * kb + s), S_nn = sum n_rs ln n_rs is added by one wavefront in the order described there, and
 *        VI_c(a) = ((A_now + A_then) - 2 S_nn) / n   (a negative rounding result is returned as 0.0),
 *      with A_then the value cached when the snapshot was "now"; agree_c(a) = sum_r n_rr, an integer, is the number of nodes
 *      whose label is unchanged.  VI_c(a) is bit-equal to what bisbm_partition_distances_to returns for chain c against that
 *      snapshot passed as a reference of the chain's own shape.
 *   3. vi_sum[c][a-1] += VI_c(a) (one f64 add per record), agree_sum[c][a-1] += agree_c(a) (uint64), vi_last[c][a-1] = VI_c(a)
 *      (NaN for ages not yet held), pairs[a-1] += 1.
 *   4. The current rows and A_now overwrite the oldest slot (a device-to-device copy on the device's stream); records += 1.
 *   Chain state, random streams, running sums and every other analysis sum are only read.  Several devices: each device records
 *   its own chains, the results are laid out in handle chain order and equal one device with all the chains bit for bit.
 *   Served: both RNG modes (labels and bisbm_entropy only), chains grouped by shape.  BISBM_ERR_UNSUPPORTED: two-byte labels.
 *   BISBM_ERR_STATE: before bisbm_init / bisbm_shuffle, without a ring, and ("bisbm_trace_reset first") when a chain's (ka, kb)
 *   differs from what its held snapshots were taken with, as after a merge or split.  A slot overwritten by
 *   bisbm_population_resample is simply compared with the previous occupant's snapshots: callers reset after a resampling step
 *   (the genealogy is not followed).  Lags are contiguous: the caller spaces records by calling every k sweeps.
 *   A workgroup counts one chain against a tile of up to 4 ages, one table per age in LDS.  Device scratch of a record with C
 *   chains on the device, the largest shape kaM + kbM: 16 C bytes of descriptors, 8 C + 16 C ages bytes of sums, and -- only
 *   when the (chain, age tile) workgroups are too few to fill the device, or a table does not fit the LDS -- integer tables of
 *   4 (kaM^2 + kbM^2) bytes per (chain, age) for as many as fit 256 MiB (at least one tile), run in as many launches as that
 *   takes.  BISBM_PARTITION_REGIME=fused|split forces either form as for the partition distances; both give the same bits.
 * reset: forgets snapshots, sums and series, keeps depth.
 * get_lags: vi_sum, agree_sum, vi_last [n_chains * depth] (row = chain), pairs [depth], records (a scalar); any pointer may be
 *   NULL.  get_series: what = BISBM_TRACE_S or BISBM_TRACE_H, out [records * n_chains], record-major.  Both BISBM_ERR_STATE
 *   without a ring.
 * summary: a pure host function, needs no device.  x[t * C + c], T >= 4 records of C >= 1 chains, a finite window > 0 (callers
 *   pass 5.0: Sokal's convention, not a measurement).  Everything in f64, sums added one term at a time in ascending index, no
 *   fused multiply-add.  Per chain: mu = (sum_t x_t) / T; d_t = x_t - mu; gamma(k) = (sum_{t=0}^{T-1-k} d_t d_{t+k}) / T.  If
 *   gamma(0) == 0.0 the chain never moved: tau = +inf, window_out = 0.  Otherwise acc = 1.0 and for k = 1 ... floor(T/2):
 *   acc = acc + 2.0 (gamma(k) / gamma(0)), M = k, stop at the first k with (double)k >= window * acc; tau = acc, window_out = M
 *   (M == floor(T/2): the series was too short).  Split-R-hat with h = floor(T/2): the 2C sequences x[0:h, c] for c ascending,
 *   then x[T-h:T, c]; each has its mean m_j and its variance v_j (denominator h - 1); W = (sum v_j) / (2C),
 *   mbar = (sum m_j) / (2C), Bn = (sum (m_j - mbar)^2) / (2C - 1); rhat = sqrt((((double)(h-1) / (double)h) W + Bn) / W), NaN when
 *   W == 0.  tau_out [C], window_out [C], rhat_out (a scalar); each may be NULL.  BISBM_ERR_INVALID_ARG: T < 4, C = 0, a
 *   non-finite x, a window that is not finite and > 0. */
#define BISBM_TRACE_S 0 /* the description length (bisbm_entropy) */
#define BISBM_TRACE_H 1 /* the partition entropy */
int bisbm_trace_set(bisbm_handle h, uint32_t depth);
int bisbm_trace_record(bisbm_handle h);
int bisbm_trace_reset(bisbm_handle h);
int bisbm_trace_get_lags(bisbm_handle h, double *vi_sum, uint64_t *agree_sum, double *vi_last /* n_chains * depth each */,
                         uint64_t *pairs /* depth */, uint64_t *records);
int bisbm_trace_get_series(bisbm_handle h, int what, double *out /* records * n_chains */);
int bisbm_trace_summary(uint64_t T, uint32_t C, const double *x /* T * C */, double window, double *tau_out /* C */,
                        uint32_t *window_out /* C */, double *rhat_out);

/* blockmodel_t::agg_merge(engine, diff_a, diff_b, nm) (blockmodel.hh, blockmodel.cc:109-206; call sites
 * mcmc_main.cc:385,429,434,446): merge diff_a type-a and diff_b type-b blocks in every chain -- nm proposals per
 * block (single_block_change :639-669), lowest merge dS first (compute_dS :335-372), blocks renumbered in the
 * order of their first node (apply_block_moves :567-611), block state rebuilt.  Afterwards bisbm_get_ka_kb returns
 * the new counts.  A negative diff first splits one block per unit (agg_split :505-565, compute_dS(split) :374-424,
 * apply_split_moves :428-459; type a first, :110-117): every block of the type with more than one node is cut nm
 * times into random halves, the cut with the lowest dS wins, its marked nodes become block KA (type a; the type-b
 * labels move up by one) or block K (type b).  The reference's split dS indexes its split vector with a counter that
 * runs over all nodes (:402), an out-of-range read; the engine implements the intended meaning -- position = rank of
 * the node within its block -- which is what agg_split's own pass (:554-561) uses.
 * The two-type overload changes every chain's counts by the same amounts.  The selection is
 * K-scale host work, as in the reference; ranks, cut evaluation, relabelling and the rebuild run on the device.
 * BISBM_ERR_STATE when no block can be split (asked before anything about the handle changes: a refused split leaves the
 * labels, their width and the block state as they were); a split past 256 blocks switches the handle to two-byte labels.
 * Several devices / several shapes behind one handle: a request that some chain cannot meet is refused before any device or
 * group changes.  What is NOT atomic is a failure in the middle of the work (a device out of memory): the devices run side
 * by side, so the others have merged by then -- the call returns the first failing device's code, bisbm_last_error names
 * every device that failed, and the handle keeps serving per-chain calls (bisbm_get_ka_kb_chain tells which chains
 * changed shape); a caller that needs all-or-nothing keeps the labels (bisbm_get_memberships) and puts them back. */
int bisbm_agg_merge(bisbm_handle h, int diff_a, int diff_b, int nm);

/* blockmodel_t::agg_merge(engine, diff, nm) (blockmodel.cc:208-271; call site mcmc_main.cc:365): diff merges over
 * both types together, proposals redrawn while the last one taken had dS = +inf.  Which types lose blocks is up to
 * each chain's own proposals, so the chains of a handle may end with different (Ka,Kb).  The handle then keeps them
 * grouped by shape internally (kernels are launched for one shape: one launch per group from then on); every call
 * keeps working per chain -- anneal, memberships, block state (array sizes follow bisbm_get_ka_kb_chain), sum dS,
 * entropy, further merges of either overload -- except that the calls which need one common shape (bisbm_get_ka_kb, the
 * marginal histogram) return BISBM_ERR_STATE while the chains' shapes differ (later merges may bring them together again).  diff < 0 is BISBM_ERR_INVALID_ARG (this overload has no split branch). */
int bisbm_agg_merge_total(bisbm_handle h, int diff, int nm);

/* Shape queries (get_KA/get_KB blockmodel.cc:103-105, get_num_edges :81).  bisbm_get_ka_kb: the block counts all chains
 * share (BISBM_ERR_STATE while a one-argument agg_merge has left them with different ones); bisbm_get_ka_kb_chain: one chain's. */
int bisbm_get_ka_kb(bisbm_handle h, uint32_t *ka, uint32_t *kb);
int bisbm_get_ka_kb_chain(bisbm_handle h, uint32_t chain, uint32_t *ka, uint32_t *kb);
int bisbm_get_sizes(bisbm_handle h, uint64_t *n, uint64_t *num_edges, uint32_t *max_degree,
                    uint32_t *n_chains);

/* Run kernels on a caller-provided hipStream_t (NULL = the handle's own stream). */
int bisbm_set_stream(bisbm_handle h, void *hip_stream);

/* Device time of the sweep kernel of the last bisbm_anneal, measured with HIP events on the
 * launch stream, and the number of node updates it executed (all chains). */
int bisbm_last_sweep_timing(bisbm_handle h, double *kernel_ms, uint64_t *node_updates);

/* How many steps the passes of the last sweep launch evaluated at once (1, 2, 4 or 8; the largest over the
 * handle's devices / shape groups).  With at most 32 blocks of a type the depth is chosen per launch from the
 * measured speed of earlier launches; the chain does not depend on it.  Diagnostic: no
 * counterpart in the reference. */
int bisbm_last_pass_steps(bisbm_handle h, uint32_t *steps_per_pass);

/* Where the last Metropolis-Hastings launch kept eta: out = {eta_in_lds, eta_w, eta_lo_a, eta_lo_b}.  eta_in_lds = 1: all of eta
 * was in LDS (eta_w = 0), and on the production kernel no row of 1 to 255 entries left the hot step for eta's sake.  Otherwise the production
 * kernel kept a window of eta_w consecutive degrees per type in LDS, [eta_lo_a, eta_lo_a + eta_w) for type a and the same from
 * eta_lo_b for type b; a row of 1 to 255 entries took the hot step if its degree lay inside its type's window and the general
 * step otherwise.  The generic kernel has no window: its eta_in_lds and three zeros.  A handle over several devices or shape
 * groups reports its first member's plan.  Diagnostic (tests tell from it which route a row took): no counterpart in the
 * reference; the chain does not depend on it. */
int bisbm_last_eta_plan(bisbm_handle h, uint32_t out[4]);

/* Which kernel the last Metropolis-Hastings launch ran and what it carried, as BISBM_ROUTE_* bits (0 before any launch).  One step
 * per pass no longer tells the generic kernel from the production one (a fielded launch runs the production kernel's one-step
 * pass), so tests and A/B runs read the route here.  A handle over several devices or shape groups reports its first member's
 * route, as bisbm_last_eta_plan does.  Diagnostic: no counterpart in the reference; the chain does not depend on it. */
#define BISBM_ROUTE_PRODUCTION 1u /* the production kernel (bisbm_sweep_fast.hip), not the generic one */
#define BISBM_ROUTE_HELD 2u       /* the launch carried a clamp and / or block constraints */
#define BISBM_ROUTE_FIELDS 4u     /* the launch carried block fields */
int bisbm_last_sweep_route(bisbm_handle h, uint32_t *route);

/* Device numerics probe (tests): evaluates log_q(n[i], k[i]) on the device (int_part.hh:27-37).
 * fast = 0: the literal evaluation (mt19937-compat mode, entropy()); fast = 1: the Philox-mode
 * evaluation, which uses a closed form of get_v/spence for k/sqrt(n) > 21. */
int bisbm_debug_log_q(bisbm_handle h, const int32_t *n, const int32_t *k, size_t count, int fast,
                      double *out);

/* Device numerics probe (tests, host replays of "Pair reshuffles"): out[i] = exp(x[i]) as the device evaluates it. */
int bisbm_debug_exp(bisbm_handle h, const double *x, size_t count, double *out);
/* ... and out[i] = log(x[i]): the logarithm of the entropy term of the node conditionals (host statements of "Held conditionals"). */
int bisbm_debug_log(bisbm_handle h, const double *x, size_t count, double *out);

const char *bisbm_last_error(bisbm_handle h); /* h may be NULL: error of the last failed create */
int bisbm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BISBM_H */
