// bisbm_kernels.hpp -- kernel parameter blocks and launcher prototypes shared by
// bisbm_kernels.hip, bisbm_sweep_fast.hip (device) and the host side of the C ABI (bisbm_engine.hpp lists its units).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bisbm_device.hpp"
#include "bisbm_predict_skew.hpp"

struct bisbm_reshuffle_record;  // include/bisbm.h

namespace bisbm {

// Per-chain scalar state kept in HBM between kernels.
struct ChainScalars {
    double cum_dS;          // blockmodel_t::entropy_ (blockmodel.hh:100): running sum of accepted dS
    double accu_r;          // metropolis_hasting::accu_r_ (metropolis_hasting.hh:28), survives anneal calls
    double last_rate;       // return value of the last anneal
    uint64_t sweeps_total;  // Philox counter: sweeps executed over the chain's lifetime
    uint64_t last_accepted;
    uint64_t last_sweeps;
    uint32_t shuffle_epoch;  // Philox counter: shuffle_bisbm calls so far
    uint32_t engine_idx;     // std::mt19937 positions (compat mode)
    uint32_t gen_idx;
    uint32_t merge_epoch;  // Philox counter: proposal rounds of agg_merge so far
    // where the last production sweep launch ran this chain: HW_ID of the stepping and of the feeder wave, XCC_ID
    // (diagnostic, see BISBM_PLACEMENT_LOG in bisbm_anneal.hip)
    uint32_t hw_id[2];
    uint32_t xcc_id;
    uint32_t split_epoch;  // Philox counter: agg_split calls so far
    // anneal()'s early-stop bookkeeping (metropolis_hasting.cc:75,85-98) where one call runs as several launches of the
    // production kernel: the minimum of sum dS so far, the count of T < 1 steps before the step that reached it, the
    // count of T < 1 steps so far, and whether the chain has returned already (SweepParams::resume)
    double stop_emin;
    uint64_t stop_mark;
    uint64_t stop_below1;
    uint32_t stopped;
    uint32_t reshuffles_total;  // Philox counter: pair reshuffles proposed over the chain's lifetime (bisbm_reshuffle_run)
};

struct SweepParams {
    // graph (shared by all chains)
    const uint32_t* rowptr;
    const uint32_t* col;
    uint32_t n, na, nb, ka, kb, maxdeg;
    double epsilon;
    // chains
    uint32_t n_chains, first_chain_id;
    const uint32_t* chain_gids;  // global id of every chain of the launch (keys its Philox streams); NULL: first_chain_id + index
    uint8_t* labels;
    size_t label_stride;
    uint32_t* vlist;  // compat: [chain][n]
    int32_t* m;       // [chain][ka*kb]
    int32_t* m_r;     // [chain][K]
    int32_t* n_r;     // [chain][K]
    uint32_t* eta;    // [chain][K*(maxdeg+1)]
    ChainScalars* scalars;
    uint32_t* mt_engine;  // compat: [chain][624]
    uint32_t* mt_gen;
    // tables
    const double* lgamma_tab;
    uint64_t lgamma_size;
    const double* q_tab;
    uint32_t q_stride;
    const double* log_tab;
    const double* T_tab;  // host-evaluated temperatures for the pow/log schedules: entry i is step T_base + i of the call
    uint64_t T_len;
    uint64_t T_base;
    int T_zero_after;
    // schedule / run
    int schedule;
    float kw0, kw1;
    uint64_t duration, steps_await;
    // production kernel, a call that runs as several launches: steps of the call executed by the launches before (whole
    // sweeps), the call's full duration, and resume = 1 from the second launch on (the early-stop bookkeeping continues from
    // the chain's scalars; chains that have returned are skipped).  One launch per call: 0, duration, 0.
    uint64_t t_base, call_duration;
    uint32_t resume;
    uint64_t seed;
    int eta_in_lds;
    // production kernel without all of eta in LDS: the window it keeps there instead -- eta_w consecutive degrees per block of
    // the phase's own type, from eta_lo_a (type-a phase) / eta_lo_b on; nodes of other degrees take the general step
    uint32_t eta_w, eta_lo_a, eta_lo_b;
    int vlist_in_lds;
    // production kernel: one counter per SIMD of the chip (kSimdClaims entries, zeroed before the launch) through which
    // the workgroups keep their stepping waves on different SIMDs; NULL: wave `fixed_stepping_wave` (0 or 1) steps
    uint32_t* simd_claims;
    uint32_t fixed_stepping_wave;
    // production kernel: 0 = one step per pass; 1 = two consecutive steps per pass where both block counts are <= 32;
    // 2 = also four per pass where both are <= 16; 3 = also eight per pass where both are <= 8
    uint32_t pair_steps;
    // depth of this launch's passes where the block counts allow a choice (1 / 2 / 3 = two / four / eight steps per pass): the
    // host sets it from the measured speed of the launches before (bisbm_anneal)
    uint32_t pass_depth;
    // production kernel, four steps per pass with 17..32 blocks of a type: 1 = the launch updates its register copies of m_r / n_r
    // in one stage per pass (words prepared ahead of the verdicts: faster where two or more steps of a pass move), 0 = one mover
    // at a time (faster where a pass has one mover or none).  The host sets it from the accepted fraction of the launch before
    // (bisbm_anneal); the chain is the same chain either way.
    uint32_t one_stage;
    // wide mode (KA + KB > 256; generic kernel only): `labels` holds two-byte labels (label_stride counts labels, not
    // bytes), and the a x b quadrant of m is read and updated in HBM
    uint32_t wide;
    // production kernel: keep the running sum of accepted dS (and the early-stop bookkeeping's code path) also in a launch
    // that cannot stop early -- BISBM_KEEP_SUM=1: the tests that check the sum of the kernel's own dS values against the change
    // of the description length, tools/soak.py
    uint32_t keep_sum;
    // replica exchange (bisbm_tempering.hip), schedule SCHED_PER_CHAIN: the constant temperature of every chain of the launch (a
    // float, like kw0: a chain at T runs exactly as a constant-schedule launch at kwargs {T, .}); NULL otherwise
    const float* T_chain;
    // production kernel, tests only (BISBM_PREDICT_SKEW = n; 0: off): the feeder hands every n-th step of a chunk -- index n - 1
    // modulo n -- a WRONG predicted target, (prediction + 1) mod k_own, so that the passes that start from a predicted target
    // take their miss paths at a known rate (bisbm_predict_skew.hpp).  The chain is the same chain whatever the prediction says.
    uint32_t predict_skew;
    // clamped nodes (bisbm_clamp.hip), Philox mode only -- the generic kernel and the held instances of the production kernel:
    // [n] a non-zero byte holds the node -- its step counts as a step that was not accepted; NULL: no clamp
    const uint8_t* clamp;
    // block constraints (bisbm_constraints.hip), Philox mode only -- the generic kernel and the held instances of the production
    // kernel: the class byte of every node [n] and the bit
    // table of eight 32-bit words per class (bit s of a class's row: block s allowed) -- a proposal of another block of the node's
    // type outside its class's row is not evaluated and counts as a step that was not accepted; NULL: no constraints
    const uint8_t* cn_class;
    const uint32_t* cn_bits;
    // block fields (bisbm_fields.hip), generic kernel in Philox mode only: the field class byte of every node [n] and the table of
    // f64 energies [class][ka + kb] -- a step that is evaluated adds (f[s] - f[r]) of the node's row to its dS; NULL: no fields
    const uint8_t* fl_class;
    const double* fl_field;
};
// Accepted fraction of the launch before from which a four-steps launch of 17..32 blocks takes the one-stage kernel
// (SweepParams::one_stage).  Measured at 32 + 32 blocks (profiles/EXPERIMENTS.md, round 7): the one stage wins by 3.9 % where 0.72
// to 0.82 of the steps are accepted (randomised start: two to three movers per pass) and loses 1.6 % at 0.65 (chains on the planted
// partition: most accepted steps are r == s, a pass has one mover or none).  Between the two nothing is measured: the per-mover loop runs.
constexpr double kOneStageAccepted = 0.7;
// Share of clamped nodes up to which a clamped handle's MH sweeps take the production kernel (its held instances); above it the
// generic kernel runs, which skips a clamped step outright where the production kernel walks the node's row all the same.
// Measured on the bench graph at 0 / 5 / 10 / 50 / 90 / 97 / 99 % clamped (profiles/held_fast_bench.json): the
// production kernel wins at every one of them, by 1.29 x still at 99 % -- two barred steps end their pass before anything is
// evaluated, so its sweep gets cheaper with the share too -- and the two do not cross inside the measured range.  The constant
// stays at section 26's estimate, which is also a measured share: up to it the production kernel is known to win (1.54 x at 97 %),
// and a handle clamped beyond it runs the generic kernel, as every clamped handle did before -- slower than it could at 97 .. 99 %
// (404 against 312 ms at 99 %), never slower than it was.  tests/test_gpu_held_fast.py pins a 98 % clamped handle to that side.
constexpr double kHeldFastMaxClampShare = 0.97;
constexpr uint32_t kSimdClaims = 1u << 14;  // index: XCC_ID[3:0] | HW_ID se, sh, cu [15:8] | simd [5:4]

struct BuildParams {
    const uint32_t* rowptr;
    const uint32_t* col;
    uint32_t n, na, ka, kb, maxdeg, n_chains;
    const uint8_t* labels;
    size_t label_stride;
    int32_t* m;
    int32_t* m_r;
    int32_t* n_r;
    uint32_t* eta;
    uint32_t wide;  // two-byte labels, m counted in HBM (see SweepParams::wide)
};

struct ShuffleParams {
    uint32_t n, na, nb, n_chains, first_chain_id;
    const uint32_t* chain_gids;  // see SweepParams
    uint64_t seed;
    uint8_t* labels;
    const uint8_t* labels_old;  // Philox: snapshot the gather reads from
    size_t label_stride;
    ChainScalars* scalars;
    uint32_t* mt_engine;
    uint32_t wide;
    // clamped nodes (Philox mode, byte labels): the open nodes of type a (open_a of them), then of type b (open_b), each
    // ascending; the labels of a type's open nodes are permuted among themselves.  NULL: no clamp
    const uint32_t* open;
    uint32_t open_a, open_b;
    // block constraints (Philox mode, byte labels; launch_shuffle takes this list first -- it serves a clamp set beside the
    // constraints as well, whose own `open` may be set too): the open nodes sorted by (type, class, id) in `cn_open`,
    // segment g = (type, class) holds cn_open[cn_seg[g] .. cn_seg[g + 1]) and is permuted among itself under the key of its
    // class, cn_seg_key[g] = (type << 8) | class.  NULL: no constraints
    const uint32_t* cn_open;
    const uint32_t* cn_seg;      // [cn_segs + 1]
    const uint32_t* cn_seg_key;  // [cn_segs]
    uint32_t cn_segs;
};

struct EntropyParams {
    uint32_t ka, kb, maxdeg, n_chains;
    const int32_t* m;
    const int32_t* m_r;
    const int32_t* n_r;
    const uint32_t* eta;
    const double* lgamma_tab;
    uint64_t lgamma_size;
    const double* q_tab;
    uint32_t q_stride;
    const double* log_tab;
    double* out;
};

struct MarginalParams {
    uint32_t n, na, ka, kmax, n_chains;
    const uint8_t* labels;
    size_t label_stride;
    uint32_t* counts;
    uint32_t wide;  // two-byte labels (see SweepParams::wide)
    const uint32_t* rung;  // replica exchange: only chains with rung[c] == 0 are counted; NULL: every chain
};

// Pair scores (bisbm_pair_scores.hip): one sample of the chains of one engine.  Slab s of the launch adds the terms of its chains
// (chain c belongs to slab c / ceil(n_chains / slabs)) into part[s][pair]; pair_scores_fold then adds the slabs to the running sums.
struct PairScoreParams {
    uint32_t n_pairs, na, ka, kb, n_chains, slabs;
    const uint32_t* u;   // [n_pairs] type-a node
    const uint32_t* v;   // [n_pairs] type-b node
    const double* dd;    // [n_pairs] (double)d(u) * (double)d(v)
    const uint8_t* labels;
    size_t label_stride;
    uint32_t wide;         // two-byte labels, m read from HBM (see SweepParams::wide)
    const int32_t* m;      // [chain][ka*kb]
    const int32_t* m_r;    // [chain][K]
    const uint32_t* rung;  // replica exchange: only chains with rung[c] == 0 are counted; NULL: every chain
    double* part;          // [slabs][n_pairs]
};
constexpr uint32_t kPairTile = 2048;  // pairs per workgroup: 256 lanes, 8 pairs each

// Query scores (bisbm_query_scores.hip): one sample of the chains of one engine into the rows of the queries of one type.  A
// workgroup owns kQueryCandTile candidates x kQueryTile queries of the list and adds the counted chains onto its cells of `sum`
// one at a time, in ascending chain order.
struct QueryScoreParams {
    uint32_t n, na, ka, kb, n_chains;
    uint32_t type;            // 0: type-a queries (candidates na .. n-1), 1: type-b queries (candidates 0 .. na-1)
    uint32_t n_list;          // queries of this type
    uint32_t cand_tiles, q_tile0;  // the launcher's: candidate tiles of the type, first query tile of the launch
    const uint32_t* list;     // [n_list] their indices in the caller's order
    const uint32_t* queries;  // [n_queries] node of every query
    const uint64_t* off;      // [n_queries + 1] first cell of every query's row in `sum`
    const uint32_t* rowptr;
    const uint8_t* labels;    // byte labels
    size_t label_stride;      // (a multiple of 4: a lane reads four candidates' labels as one word)
    const int32_t* m;         // [chain][ka*kb]
    const int32_t* m_r;       // [chain][K]
    const uint32_t* rung;     // replica exchange: only chains with rung[c] == 0 are counted; NULL: every chain
    double* sum;
};
constexpr uint32_t kQueryCandTile = 1024;  // candidates per workgroup: 256 lanes, one word of 4 labels each
constexpr uint32_t kQueryTile = 8;         // queries per workgroup
constexpr uint32_t kQueryMaxK = 1024;      // bisbm_query_scores_topk: the largest k (the selection is kept in LDS)

// Edge queries (bisbm_edge_queries.hip): every candidate of a node weighed by the exact dS of adding the edge.
// The terms of dS that belong to (chain, block) and to (chain, block, degree) for chains c0 .. c0 + n_range - 1 of one engine:
// what the two term kernels of bisbm_edge_probs.hip fill, for the listed call and for this one alike.
struct EdgeTermParams {
    uint32_t ka, kb, maxdeg, c0, n_range;
    const int32_t *m_r, *n_r;  // [chain][K]
    const uint32_t* eta;       // [chain][K][maxdeg + 1]
    const uint32_t* rung;      // replica exchange: only chains with rung[c] == 0 are filled; NULL: every chain
    Tables tab;
    double* blk;               // [n_range][K][4] {t_mr half, t_q half} of ADD, of REMOVE
    double* etat;              // [n_range][K][maxdeg + 1][2] {lg(eta+1) - lg(eta), lg(eta+1) - lg(eta+2)}
};
hipError_t launch_edge_terms(const EdgeTermParams& p, hipStream_t stream);
// One range of chains of one engine into the rows of the queries of one type.  A workgroup owns kEdgeQueryCandTile candidates x
// kEdgeQueryTile queries of the list and adds w = exp(-dS) of the counted chains of the range onto its cells of `sum` one at a
// time, in ascending chain order; the ranges of a sample follow each other on the stream.
struct EdgeQueryParams {
    uint32_t n, na, ka, kb, maxdeg, c0, n_range;
    uint32_t type;            // 0: type-a queries (candidates na .. n-1), 1: type-b queries (candidates 0 .. na-1)
    uint32_t n_list;          // queries of this type
    uint32_t cand_tiles, q_tile0;  // the launcher's: candidate tiles of the type, first query tile of the launch
    const uint32_t* list;     // [n_list] their indices in the caller's order
    const uint32_t* queries;  // [n_queries] node of every query
    const uint64_t* off;      // [n_queries + 1] first cell of every query's row in `sum`
    const uint32_t* rowptr;
    // the present edges of every query: its distinct neighbours ascending, nbr[nbr_ptr[i]] .. nbr[nbr_ptr[i + 1] - 1], and
    // t_mult = lg(mu + 2) - lg(mu + 1) of each
    const uint64_t* nbr_ptr;  // [n_queries + 1]
    const uint32_t* nbr;
    const double* nbr_tmult;
    const uint8_t* labels;    // byte labels
    size_t label_stride;      // (a multiple of 4: a lane reads four candidates' labels as one word)
    const int32_t* m;         // [chain][ka*kb]
    const uint32_t* rung;     // replica exchange: only chains with rung[c] == 0 are counted; NULL: every chain
    const double* lg;         // the lgamma table (t_deg, t_m)
    uint64_t lg_size;
    double tE;                // t_E of ADD for this shape
    const double* blk;        // [n_range][K][4] block terms of the range
    const double* etat;       // [n_range][K][maxdeg + 1][2] eta terms of the range
    double* tm;               // [n_range][ka*kb] t_m = lg(m+1) - lg(m+2) of every cell of the quadrant, of the range
    double* sum;
};
constexpr uint32_t kEdgeQueryCandTile = 1024;  // candidates per workgroup: 256 lanes, one word of 4 labels each
constexpr uint32_t kEdgeQueryTile = 8;         // queries per workgroup
hipError_t launch_edge_queries(const EdgeQueryParams& p, hipStream_t stream);

// Top-k selection (bisbm_topk.hip): the best k candidates of every query of one chunk (q0 .. q0 + n_q - 1), for query scores,
// co-assignment and fold-in rows alike.  The candidates of query qi are the off[qi + 1] - off[qi] cells of its row, in id order;
// rows / mask hold the chunk's cells from cell off[q0] on.  A candidate is eligible iff it is not masked and is not `self`.
struct TopkCand {
    uint32_t first;  // node id of the query's first candidate (0 or na)
    uint32_t self;   // index within the row of the one candidate that is never eligible (the query's own node); 0xffffffff: none
};
template <class Key>  // the bit pattern of a cell: uint32_t counts, unsigned long long for the non-negative f64 sums
struct TopkSelectParams {
    uint32_t q0, n_q, k;
    const uint64_t* off;   // [n_queries + 1]
    const TopkCand* cand;  // [n_queries]
    const Key* rows;
    const uint8_t* mask;   // 1: not eligible; NULL: no candidate is masked
    uint32_t* node_out;    // [n_q][k] global node ids in rank order, 0xffffffff past the eligible ones
    Key* val_out;          // [n_q][k] their cells, 0 past the eligible ones
};
// The lists whose entries are masked (device pointers): query qi's are col[ptr[i]] .. col[ptr[i + 1] - 1] with i = at[qi], or
// i = qi where `at` is NULL.  The graph's CSR rows have uint32 offsets (ptr32), the lists of virtual nodes uint64 ones (ptr64).
struct TopkMaskLists {
    const uint32_t* ptr32;
    const uint64_t* ptr64;
    const uint32_t* at;
    const uint32_t* col;
};

// Co-assignment (bisbm_coassign.hip): one sample of the chains of one engine into the rows of the queries of one type.  A
// workgroup owns kCoassignCandTile candidates (nodes of the queries' own type) x kCoassignTile queries and adds 1 to a cell for
// every counted chain in which candidate and query carry the same label.  The queries' labels come from `qlab`, which the
// gather kernel fills once per sample: slot s of chain c holds the label of the query in slot s (type-a queries first, each
// type padded to whole query tiles), with byte labels replicated into all four bytes of the word.
struct CoassignParams {
    uint32_t n, na, n_chains;
    uint32_t type;            // 0: type-a queries (candidates 0 .. na-1), 1: type-b queries (candidates na .. n-1)
    uint32_t n_list;          // queries of this type
    uint32_t slot0, q_slots;  // first slot of this type and slots per chain in `qlab`
    uint32_t cand_tiles, q_tile0;  // the launcher's: candidate tiles of the type, first query tile of the launch
    int plain;                // byte labels: the extract-compare-add form instead of the packed one (the bench tool's A/B)
    const uint32_t* list;     // [n_list] their indices in the caller's order
    const uint64_t* off;      // [n_queries + 1] first cell of every query's row in `count`
    const uint8_t* labels;    // [chain][label_stride] labels, one or two bytes each
    size_t label_stride;      // in labels (a multiple of 4: a lane reads four candidates' labels as one or two words)
    const uint32_t* rung;     // replica exchange: only chains with rung[c] == 0 are counted; NULL: every chain
    const uint32_t* qlab;     // [chain][q_slots]
    uint32_t* count;
};
constexpr uint32_t kCoassignCandTile = 1024;  // candidates per workgroup: 256 lanes, four labels each
constexpr uint32_t kCoassignTile = 16;        // queries per workgroup
// qlab[c][s] = label of node queries[slot[s]] in chain c (slot[s] = 0xffffffff: a padding slot, set to 0)
struct CoassignGatherParams {
    uint32_t n_chains, q_slots;
    const uint32_t* slot;     // [q_slots] query index of every slot
    const uint32_t* queries;  // [n_queries] node of every query
    const uint8_t* labels;
    size_t label_stride;
    uint32_t* qlab;
};

// Fold-in queries (bisbm_foldin.hip): virtual nodes given by a type and a list of neighbours of the other type.  The table kernel
// turns every (counted chain, virtual node) into the node's block posterior P[k_own] and its recommend table g[k_oth]; the rows
// kernel adds one table lookup per (virtual node, candidate) and chain onto the running sums, chain by chain in ascending order.
// Slots: the type-a virtual nodes in the caller's order, then the type-b ones.  One chain's tables: the slots' rows back to back,
// n_a * ka + n_b * kb doubles of P, n_a * kb + n_b * ka doubles of g.
struct FoldinTableParams {
    uint32_t na, ka, kb;
    uint32_t chain0, n_chains;  // the chains of the launch: chain0 .. chain0 + n_chains - 1 of the engine
    uint32_t n_q, n_a;          // slots, of which type a
    uint32_t recommend;         // 0: only P is wanted
    double alpha;
    const uint32_t* order;      // [n_q] index of every slot's virtual node in the caller's order
    const uint64_t* ptr;        // [n_q + 1] by caller's index: first list entry of every virtual node
    const uint32_t* nbr;        // the lists, in the caller's order
    const uint8_t* labels;      // byte labels
    size_t label_stride;
    const int32_t* m;           // [chain][ka*kb]
    const int32_t* m_r;         // [chain][K]
    const int32_t* n_r;         // [chain][K]
    const uint32_t* rung;       // replica exchange: only chains with rung[c] == 0 are counted (the others: NaN rows of P); NULL: all
    double* P;                  // [chain of the engine][n_a * ka + n_b * kb]
    double* g;                  // [chain - chain0][n_a * kb + n_b * ka]
};
struct FoldinRowsParams {
    uint32_t chain0, n_chains;  // as above
    uint32_t first, n_cand;     // the candidates: nodes first .. first + n_cand - 1
    uint32_t lab0, k_tab;       // first label and block count of the candidates' type: a table row has k_tab entries
    uint32_t slot0, n_list;     // the slots of the virtual nodes' type
    uint32_t cand_tiles, q_tile0;  // the launcher's: candidate tiles, first tile of virtual nodes of the launch
    const uint32_t* order;      // [n_q] index of every slot's virtual node in the caller's order
    const uint64_t* ptr;        // [n_q + 1] by caller's index: the list length is the virtual node's degree
    const uint64_t* off;        // [n_queries + 1] by caller's index: first cell of the node's row in `sum`
    const uint32_t* rowptr;
    const uint8_t* labels;
    size_t label_stride;        // (a multiple of 4: a lane reads four candidates' labels as one word)
    const uint32_t* rung;
    const double* tab;          // tables of chain chain0 on: tab[c * chain_stride + type_base + (slot - slot0) * k_tab + block]
    size_t chain_stride, type_base;
    double* sum;
};
constexpr uint32_t kFoldinCandTile = 1024;  // candidates per workgroup: 256 lanes, one word of 4 labels each
constexpr uint32_t kFoldinTile = 8;         // virtual nodes per workgroup

// Node conditionals (bisbm_conditionals.hip).  The rows kernel turns every (chain of the launch, query) into the node's rows dS[k_own]
// and P[k_own] and the chain's four terms (stay, entropy, margin, free as 0.0 / 1.0); a chain that is not counted gets NaN.  One
// chain's rows: the queries' rows back to back in the caller's order; nbb[i] = the type-b queries before query i.
struct CondRowsParams {
    uint32_t na, ka, kb, maxdeg;
    uint32_t chain0, n_chains;  // the chains of the launch: chain0 .. chain0 + n_chains - 1 of the engine
    uint32_t buf_chain0;        // the row and term buffers hold the chains from this one on
    uint32_t n_q;
    double beta;
    size_t row_total;           // doubles of one chain's rows
    const uint32_t* q;          // [n_q] node of every query
    const uint32_t* nbb;        // [n_q + 1]
    const uint32_t* rowptr;
    const uint32_t* col;
    const uint8_t* labels;      // byte labels
    size_t label_stride;
    const int32_t* m;           // [chain][ka*kb]
    const int32_t* m_r;         // [chain][K]
    const int32_t* n_r;         // [chain][K]
    const uint32_t* eta;        // [chain][K*(maxdeg+1)]
    const uint32_t* rung;       // replica exchange: only chains with rung[c] == 0 are counted; NULL: every chain
    const double* lgamma_tab;
    uint64_t lgamma_size;
    const double* q_tab;
    uint32_t q_stride;
    const double* log_tab;
    double* dS;                 // [chain - buf_chain0][row_total]
    double* P;
    double* terms;              // [chain - chain0][n_q][4]
    // held rows (bisbm_held_conditionals_set; all NULL: the model's row): the heat-bath launch's pointers (HeatbathParams)
    const uint8_t* clamp;       // [n] mask bytes
    const uint8_t* cn_class;    // [n] class of every node
    const uint32_t* cn_bits;    // [classes][8]
    const uint8_t* fl_class;    // [n] field class of every node
    const double* fl_field;     // [classes][ka + kb]
};
// prob[query][perm[chain][block] - type base] += P[chain][query][block], chains in ascending order
struct CondSoftParams {
    uint32_t na, ka, kb, kmax, n_q;
    uint32_t chain0, n_chains, buf_chain0;
    size_t row_total;
    const uint32_t* q;
    const uint32_t* nbb;
    const double* P;
    const uint8_t* perm;        // [chain of the engine][ka + kb], global-label form
    double* prob;               // [n_q][kmax]
};

// agg_split (blockmodel.cc:505-565): evaluation of `n_trials` random half-cuts of every block of one type, all chains
struct SplitParams {
    const uint32_t* rowptr;
    const uint32_t* col;
    uint32_t n, na, ka, kb, n_chains, first_chain_id;
    const uint32_t* chain_gids;  // see SweepParams
    uint32_t type;              // 0: a type-a block is split, 1: a type-b block
    uint32_t trial0, n_trials;  // trials evaluated by this launch: trial0 .. trial0 + n_trials - 1
    uint32_t nm;                // trials per block of the whole call (stride of `bits`)
    uint64_t seed;
    uint8_t* labels;
    size_t label_stride;
    const int32_t* n_r;  // [chain][K]
    const ChainScalars* scalars;
    uint32_t* rank;        // [chain][n_type]: rank of every node of the type within its block (ascending id)
    const uint32_t* bits;  // compat: [chain][nm][bit_words] cut bits at position (offset of the block + rank); NULL: Philox
    uint32_t bit_words;
    int32_t* out_k;    // [chain][n_trials][k_type][k_oth]: edges from the marked nodes of block r to opposite block t
    int32_t* out_deg;  // [chain][n_trials][k_type]: degree sum of the marked nodes
    const uint32_t* chosen;  // apply: [chain][2] = {block (own-type index), trial}
    // wide handles (two-byte labels, more than 256 blocks): the rank counters ([chain][K], zeroed) and, in compat mode, the
    // first position of every block in the cut bits ([chain][k_type]) live in HBM; out_k / out_deg are zeroed by the caller
    uint32_t wide;
    uint32_t* rank_base;
    const uint32_t* block_off;
};
constexpr uint32_t PHX_SPLIT = 6;
constexpr uint32_t PHX_EXCHANGE = 7;  // replica exchange: idx = round * L + lower rung, chain = the ensemble's first global id
constexpr uint32_t PHX_RESAMPLE = 8;  // population annealing: idx = resampling step, chain = the handle's first global id
constexpr uint32_t PHX_HEATBATH = 9;  // heat-bath sweeps: idx = sweeps_total * n + position in the sweep, chain = the chain's global id

// What a launch of a "one wave owns one chain" move kernel (bisbm_wave_chain.hpp) takes, whatever the move.  The ORDER of the
// fields is load-bearing: it fixes the offsets in the kernels' argument block, and with them the compiler's scalar register
// allocation and spills (eta_in_lds in the padding after q_stride and rounds before beta keep heat-bath's offsets and figures;
// profiles/wave_chain_state.md).  After inserting or moving a field compare libbisbm_hip.resources.json with that table.
struct WaveChainParams {
    const uint32_t* rowptr;
    const uint32_t* col;
    uint32_t n, na, nb, ka, kb, maxdeg;
    uint32_t n_chains, first_chain_id;
    const uint32_t* chain_gids;  // see SweepParams
    uint8_t* labels;             // byte labels
    size_t label_stride;
    int32_t* m;                  // [chain][ka*kb]
    int32_t* m_r;                // [chain][K]
    int32_t* n_r;                // [chain][K]
    uint32_t* eta;               // [chain][K*(maxdeg+1)]
    ChainScalars* scalars;       // cum_dS advances, and what the kernel counts
    const double* lgamma_tab;
    uint64_t lgamma_size;
    const double* q_tab;
    uint32_t q_stride;
    int eta_in_lds;              // (host: which instantiation is launched)
    const double* log_tab;
    uint64_t seed;
    uint64_t rounds;             // sweeps or moves of the call
    double beta;                 // finite, > 0
    // replica exchange (bisbm_tempering_run_rounds): a beta per chain of the launch -- chain c runs at beta_rung[rung[c]], the
    // host's quotient 1.0 / (double)T of its rung's temperature (TemperState::d_beta, d_rung); NULL: `beta` for every chain
    const double* beta_rung;
    const uint32_t* rung;
};
// The chain state in LDS: the quadrant of m with an odd row stride, m_r, n_r, the k_v histogram and the list's t and k_t (4
// bytes an entry), the parked neighbour labels of a chunk, eta when it fits -- WaveChain::load carves exactly these.
constexpr uint32_t kParkedLabelBytes = kWave * kWave;
__host__ __device__ constexpr uint32_t wave_chain_stride(uint32_t kb) { return kb | 1u; }
inline size_t wave_chain_lds_bytes(uint32_t ka, uint32_t kb, uint32_t maxdeg, bool eta_in_lds) {
    const size_t K = (size_t)ka + kb, kmax = ka > kb ? ka : kb;
    size_t lds = sizeof(int32_t) * ((size_t)ka * wave_chain_stride(kb) + 2 * K + 3 * kmax) + kParkedLabelBytes;
    if (eta_in_lds) lds += sizeof(uint32_t) * K * ((size_t)maxdeg + 1);
    return (lds + 15) & ~(size_t)15;
}

// Heat-bath sweeps and greedy polishing (bisbm_heatbath.hip): `rounds` sweeps of every chain of one engine.  Of the scalars
// sweeps_total advances too; last_accepted = moves, last_sweeps = sweeps run.  `beta` is unused when greedy (never per rung).
struct HeatbathParams : WaveChainParams {
    uint32_t greedy;             // beta = +inf: the lowest argmin of dS, only strictly downhill, no draw
    uint32_t stop_when_settled;  // a chain stops after the first sweep that moved nothing
    const uint8_t* clamp;        // clamped nodes: [n] a non-zero byte holds the node as a node that is not free is held; NULL: no clamp
    // block constraints: the class byte per node and the bit table (SweepParams::cn_bits) -- the row of a node is restricted to the
    // allowed blocks of its type, a node with one allowed block is held as a clamped node is; NULL: no constraints
    const uint8_t* cn_class;
    const uint32_t* cn_bits;
    // block fields: the field class byte per node and the table (SweepParams::fl_field) -- the row entry of a target s != r gets
    // (f[s] - f[r]) of the node's row added; NULL: no fields
    const uint8_t* fl_class;
    const double* fl_field;
};

constexpr uint32_t PHX_RESHUFFLE = 10;  // pair reshuffles: idx = (reshuffles_total << 32) | k, chain = the chain's global id

// Pair reshuffles (bisbm_reshuffle.hip): `rounds` moves of every chain of one engine.  Of the scalars reshuffles_total advances too.
struct ReshuffleParams : WaveChainParams {
    uint32_t scans;
    // per-chain scratch, nmax = max(na, nb) entries each: the member ids, their original labels, their launch labels
    uint32_t* member;            // [chain][nmax]
    uint8_t* orig;               // [chain][nmax]
    uint8_t* launch;             // [chain][nmax]
    bisbm_reshuffle_record* record;  // [chain] the last move of the call
    unsigned long long* accepted;    // [chain] accepted moves of the call
    const uint8_t* clamp;            // clamped nodes: [n] a node with a non-zero byte is no member of any move; NULL: no clamp
    // block constraints: a node whose class does not allow BOTH blocks of the pair is no member either; NULL: no constraints
    const uint8_t* cn_class;
    const uint32_t* cn_bits;
    // block fields: a member's dS_o gets (f[o] - f[c]) of its row added before it enters the weights and the pass's sum; NULL: no fields
    const uint8_t* fl_class;
    const double* fl_field;
};
hipError_t launch_exp_probe(const double* x, size_t count, double* out, hipStream_t stream);

hipError_t launch_split_rank(const SplitParams& p, hipStream_t stream);
hipError_t launch_split_eval(const SplitParams& p, hipStream_t stream);
hipError_t launch_split_apply(const SplitParams& p, hipStream_t stream);
hipError_t launch_labels_to_wide(const uint8_t* labels, uint8_t* wide_labels, size_t label_stride, uint32_t n, uint32_t n_chains,
                                 hipStream_t stream);

// beta of chain `chain` of a heat-bath or reshuffle launch: read once at the head of the kernel, the same in every lane
template <class P>
__device__ __forceinline__ double chain_beta_of(const P& p, uint32_t chain) {
    return p.beta_rung ? p.beta_rung[p.rung[chain]] : p.beta;
}

// global id of chain `chain` of a launch
template <class P>
__device__ __forceinline__ uint32_t chain_gid_of(const P& p, uint32_t chain) {
    return p.chain_gids ? p.chain_gids[chain] : p.first_chain_id + chain;
}

// metropolis_hasting.cc:10-37, arithmetic types as the C++ promotes them
__device__ __forceinline__ double temperature_of(const SweepParams& p, uint64_t t) {
    switch (p.schedule) {
        case SCHED_CONSTANT:
            return (double)p.kw0;
        case SCHED_PER_CHAIN:  // (replica exchange; the sweep kernels run chain blockIdx.x)
            return (double)p.T_chain[blockIdx.x];
        case SCHED_ABRUPT:
            return ((float)t < p.kw0) ? 1. : 0.;
        case SCHED_LINEAR:
            return (double)(p.kw0 - p.kw1 * (float)t);
        case SCHED_EXPONENTIAL:
            if (t < p.T_len) return p.T_tab[t];  // host table: glibc pow, incl. the subnormal tail
            if (p.T_zero_after) return 0.;
            return (double)p.kw0 * pow((double)p.kw1, (double)t);
        default: {  // SCHED_LOGARITHMIC
            if (t < p.T_len) return p.T_tab[t];
            const float x = (float)t + p.kw1;
            const unsigned long long i = (unsigned long long)x;
            return (double)p.kw0 / (i == 0 ? 0. : log((double)i));
        }
    }
}

// The production kernel's temperatures: the pow / log schedules come from the host table only (glibc, the reference's own
// values) -- bisbm_anneal hands every launch the slice of the call it covers, so no pow() / log() is compiled into that
// kernel (they cost it 30 - 110 spilled vector registers in the cooling-schedule variants).
__device__ __forceinline__ double temperature_tabled(const SweepParams& p, uint64_t t) {
    switch (p.schedule) {
        case SCHED_CONSTANT:
            return (double)p.kw0;
        case SCHED_ABRUPT:
            return ((float)t < p.kw0) ? 1. : 0.;
        case SCHED_LINEAR:
            return (double)(p.kw0 - p.kw1 * (float)t);
        case SCHED_PER_CHAIN:  // (replica exchange; the production kernel runs chain blockIdx.x)
            return (double)p.T_chain[blockIdx.x];
        default: {  // SCHED_EXPONENTIAL, SCHED_LOGARITHMIC
            const uint64_t i = t - p.T_base;
            return i < p.T_len ? p.T_tab[i] : 0.;  // (past the table: the exponential schedule after it has underflowed to 0)
        }
    }
}

// Production kernel: does a launch keep anneal()'s early-stop bookkeeping (metropolis_hasting.cc:85-98)?  It can only ever fire
// below T = 1 and when steps_await can be reached within the call.  A launch that does not keep it does not keep the running sum
// of accepted dS either (nobody looks at it during the launch): bisbm_anneal then advances the chain's sum by the change of the
// block-state part of the description length over the call (entropy_kernel before and after; the two agree to ~1e-13 relative,
// tests/test_gpu_scale.py), which takes the sum out of every pass.
__host__ __device__ inline bool sweep_fast_tracks_minimum(int schedule, float kw0, uint64_t steps_await, uint64_t call_duration) {
    return (schedule != SCHED_CONSTANT || (double)kw0 < 1.) && steps_await <= call_duration;
}
// scalars[c].cum_dS += after[c] - before[c]
hipError_t launch_sum_from_entropy(ChainScalars* scalars, const double* before, const double* after, uint32_t n_chains, hipStream_t stream);

hipError_t launch_sweep(const SweepParams& p, int rng_mode, size_t lds_bytes, hipStream_t stream);
hipError_t launch_sweep_fast(const SweepParams& p, size_t lds_bytes, hipStream_t stream);
// held: a launch with clamped nodes and / or block constraints (two more hand-off words per step: 1 KiB); fielded: a launch with block
// fields (the two held words and the field class: 1.5 KiB).  Unfielded launches get the bytes they always got.
size_t sweep_fast_lds_bytes(uint32_t ka, uint32_t kb, uint32_t maxdeg, bool eta_in_lds, uint32_t eta_window, bool held = false, bool fielded = false);
hipError_t launch_state_build(const BuildParams& p, hipStream_t stream);
// `labels` is the byte base of the label array; wide: two-byte labels (label_stride counts labels in both cases)
hipError_t launch_labels_broadcast(const uint32_t* src, uint8_t* labels, bool wide, size_t label_stride, uint32_t n,
                                   uint32_t first_chain, uint32_t n_chains, hipStream_t stream);
hipError_t launch_labels_widen(const uint8_t* labels, bool wide, uint32_t* dst, uint32_t n, hipStream_t stream);
hipError_t launch_labels_narrow(const uint8_t* wide_labels, uint8_t* labels, size_t label_stride, uint32_t n, uint32_t n_chains,
                                hipStream_t stream);
// relabelling after block merges: map1 / fmap are [n_chains][map_len] tables of labels (bytes, or two bytes when wide), first is
// [n_chains][map_len] (preset to ~0); map_len = the block count before the call rounded up to a multiple of 256
hipError_t launch_merge_first(const uint8_t* labels, bool wide, size_t label_stride, uint32_t n, uint32_t n_chains, uint32_t map_len,
                              const void* map1, uint32_t* first, hipStream_t stream);
hipError_t launch_merge_relabel(uint8_t* labels, bool wide, size_t label_stride, uint32_t n, uint32_t n_chains, uint32_t map_len,
                                const void* fmap, hipStream_t stream);
hipError_t launch_shuffle(const ShuffleParams& p, int rng_mode, hipStream_t stream);
hipError_t launch_entropy(const EntropyParams& p, hipStream_t stream);
hipError_t launch_marginals(const MarginalParams& p, hipStream_t stream);
// MAP labels of `rows` nodes from the histogram rows at `counts` (node `first` on), with the winning counts where top_out is
// not NULL; a += b over `count` counters
hipError_t launch_marginal_map(const uint32_t* counts, uint32_t rows, uint32_t kmax, uint32_t first, uint32_t n, uint32_t na,
                               uint32_t ka, uint16_t* labels_out, uint32_t* top_out, hipStream_t stream);
hipError_t launch_counts_add(uint32_t* a, const uint32_t* b, size_t count, hipStream_t stream);
// dd[i] = (double)d(u[i]) * (double)d(v[i]) from the CSR row lengths
hipError_t launch_pair_degrees(const uint32_t* rowptr, const uint32_t* u, const uint32_t* v, uint32_t n_pairs, double* dd, hipStream_t stream);
hipError_t launch_pair_scores(const PairScoreParams& p, hipStream_t stream);
// sum[i] += part[0][i] + ... + part[slabs - 1][i], added in slab order
hipError_t launch_pair_scores_fold(double* sum, const double* part, uint32_t slabs, uint32_t n_pairs, hipStream_t stream);
uint32_t pair_score_slabs(uint64_t n_pairs, uint32_t n_chains);
hipError_t launch_query_scores(const QueryScoreParams& p, hipStream_t stream);
hipError_t launch_coassign_gather(const CoassignGatherParams& p, bool wide, hipStream_t stream);
hipError_t launch_coassign_count(const CoassignParams& p, bool wide, hipStream_t stream);
hipError_t launch_foldin_tables(const FoldinTableParams& p, hipStream_t stream);
hipError_t launch_foldin_rows(const FoldinRowsParams& p, bool recommend, hipStream_t stream);
// bisbm_topk.hip: mask[cell of (query, entry)] = 1 for every entry of the lists of queries q0 .. q0 + n_q - 1 (mask: the
// chunk's, zeroed; off / cand as TopkSelectParams); the selection; a += b over `count` cells (Key / T: uint32_t and the 64-bit type)
hipError_t launch_topk_mask(const TopkMaskLists& lists, uint32_t q0, uint32_t n_q, const uint64_t* off, const TopkCand* cand, uint8_t* mask,
                            hipStream_t stream);
template <class Key>
hipError_t launch_topk_select(const TopkSelectParams<Key>& p, hipStream_t stream, bool ascending = false);
template <class T>
hipError_t launch_rows_add(T* a, const T* b, uint64_t count, hipStream_t stream);
hipError_t launch_cond_rows(const CondRowsParams& p, hipStream_t stream);
// the terms of n_chains chains ([chain][n_q][4]) onto stat[3][n_q] and free_cnt[n_q], chain by chain in ascending order
hipError_t launch_cond_pool(const double* terms, uint32_t n_q, uint32_t n_chains, double* stat, unsigned long long* free_cnt, hipStream_t stream);
hipError_t launch_cond_soft(const CondSoftParams& p, hipStream_t stream);
hipError_t launch_log_q_probe(const Tables& tab, const int32_t* n, const int32_t* k, size_t count, double* out,
                              int fast, hipStream_t stream);

}  // namespace bisbm
