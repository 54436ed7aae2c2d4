// bisbm_engine.hpp -- what the translation units of the host side share (internal; the C ABI is include/bisbm.h): the handle,
// the host-built tables, error / allocation helpers (DeviceBuf: the one owner of a device buffer that grows on demand; DeviceGuard:
// the caller's current device put back), the aligned-sample pipeline that the pooled and the mode-resolved marginals share and the one
// walk over container handles (chains of several shapes: `groups`; several devices: `devs`): leaves / each_leaf / device_entries /
// any_grouped / any_wide / shared_shape / leaf_of_chain.
//
//   bisbm_tables.cpp     host-built numeric tables, temperature tables (no HIP)
//   bisbm_handle.hip     create / destroy / labels in and out / init / shuffle / getters / entropy; the walk over a handle
//   bisbm_anneal.hip     bisbm_anneal: LDS plan, launch slicing (table slices, pass depth), bookkeeping across launches
//   bisbm_marginals.hip  per-node label histogram, MAP labels of one engine
//   bisbm_multi.hip      several devices behind one handle: creation, dispatch, pooling (RCCL / peer copies)
//   bisbm_merge.hip      agg_merge / agg_split between anneals, chains of one handle in different shapes
//   bisbm_align.hip      aligned marginal samples: every counted chain renumbered to the reference of its mode, then counted (the
//                        overlap, assignment and counting kernels; one mode of every chain: the pooled aligned histogram)
//   bisbm_tempering.hip  replica exchange: temperature ladders over ensembles of chains, the exchange kernel; rounds of MH sweeps,
//                        heat-bath sweeps and pair reshuffles at a beta per chain, the per-rung tally
//   bisbm_population.hip  population annealing: offspring counts on the host, the kernel that copies chain states between slots
//   bisbm_pair_scores.hip  posterior-predictive pair scores pooled over chains: its kernels and its part of the C ABI
//   bisbm_edge_probs.hip   exact edge probabilities: dS of adding or removing a listed edge, pooled over chains; kernels and C ABI
//   bisbm_query_scores.hip  query scores: every candidate of a node scored over the chains; kernels and C ABI
//   bisbm_edge_queries.hip  edge queries: every candidate of a node weighed by the exact dS of adding the edge; kernel and C ABI
//   bisbm_coassign.hip   co-assignment: how often every node of a query's own type shares its block; kernels and C ABI
//   bisbm_foldin.hip     fold-in queries: block posterior, recommendations and peers of a node that is not in the graph; kernels and C ABI
//   bisbm_topk.hip       the best k candidates of every query, for the three units above: the mask, select and add kernels, the
//                        host driver of the *_topk calls and the reader of the *_get_row calls (bisbm_cand_lanes.hpp: how the
//                        three accumulate kernels lay candidates over lanes)
//   bisbm_conditionals.hip  node conditionals: dS of every target block of a node, the conditional and its pooled terms, soft marginals; kernels and C ABI
//   bisbm_heatbath.hip   heat-bath sweeps and greedy polishing: nodes moved by their conditionals; kernel and C ABI (and the host
//                        side of the chain state it shares with the reshuffle kernel: bisbm_wave_chain.hpp)
//   bisbm_reshuffle.hip  pair reshuffles: two blocks' nodes divided afresh in one accepted or rejected move; kernel and C ABI
//   bisbm_split_merge.hip  split and merge moves: a block divided in two or two made one, the chains regrouped by shape; kernels and C ABI
//   bisbm_partition.hip  chain-by-chain partition distances (contingency tables, VI, entropies), grouping into modes
//   bisbm_mode_marginals.hip  mode-resolved marginals, host side: the chains' modes, a reference and a histogram slice per mode
//   bisbm_block_sums.hip  block summaries: the aligned block matrix, sizes and degrees summed over the counted chains of an
//                        aligned sample; kernel and C ABI
//   bisbm_trace.hip      chain traces: a ring of each chain's own snapshots, lagged distances to them, the S / H series, tau and R-hat
//   bisbm_clamp.hip      clamped nodes: the mask, the lists of the open nodes, the clamped shuffle kernel; C ABI
//   bisbm_constraints.hip  block constraints: a class per node and a table of allowed blocks per class; the validation kernel,
//                        the list of the open nodes by (type, class); C ABI
//   bisbm_fields.hip     block fields: a class per node and a table of f64 energies per class and block; the kernel of a
//                        chain's field energy Phi; C ABI
//
// Reference lines cited as <file>:<line> relative to /root/reference/src.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <queue>
#include <random>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/bisbm.h"
#include "bisbm_kernels.hpp"
#include "bisbm_pass_policy.hpp"

namespace bisbm {

// ------------------------------------------------------------------------------------------
// host-built tables (the reference builds the same tables on the host at construction:
// blockmodel.cc:47-48 -> support/cache.cc:64-91, support/int_part.cc:34-51); bisbm_tables.cpp
// ------------------------------------------------------------------------------------------
struct HostTables {
    std::vector<double> lg;  // lg[i] = lgamma(i), lg[0] = +inf
    std::vector<double> lo;  // lo[i] = log(i), lo[0] = 0 (safelog, cache.hh:38-44)
    std::vector<double> q;   // (10001) x (kcap+1)
    uint32_t kcap = 0;
};
std::shared_ptr<HostTables> get_tables(uint64_t lg_size, uint32_t kcap);
double h_lgamma_fast(const HostTables& t, uint64_t x);                // cache.hh:82-93
double h_lbinom_fast(const HostTables& t, uint64_t N, uint64_t k);    // util.hh:41-47
// metropolis_hasting.cc:10-13,20-23 with the host libm for steps t0 .. t0 + len - 1 of a call
std::vector<double> schedule_table(int schedule, float kw0, float kw1, uint64_t t0, uint64_t len, int* zero_after);

template <class T>
hipError_t dalloc(T** p, size_t count) {
    return hipMalloc((void**)p, sizeof(T) * std::max<size_t>(count, 1));
}

// A device buffer with one owner: freed when its owner goes, grown on demand.  It is allocated on whatever device is current
// (as dalloc).  Growing does NOT keep the contents: no caller needs them kept.
template <class T>
class DeviceBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;  // elements

public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    DeviceBuf& operator=(DeviceBuf&& o) noexcept {  // (what this one held goes with `o`)
        std::swap(p_, o.p_), std::swap(cap_, o.cap_);
        return *this;
    }
    ~DeviceBuf() { reset(); }
    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    // room for `count` elements: an allocation that has it is kept, otherwise it is replaced; empty after a failure
    hipError_t reserve(size_t count) {
        if (p_ && cap_ >= count) return hipSuccess;
        reset();
        const hipError_t e = dalloc(&p_, count);
        if (e == hipSuccess)
            cap_ = count;
        else
            p_ = nullptr;
        return e;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr, cap_ = 0;
    }
};

// The calling thread's current device, put back when the call returns: the calls that visit every device of a handle on the
// caller's thread must not move a torch caller's later "current device" allocations with them.
struct DeviceGuard {
    int saved = -1;
    DeviceGuard() {
        if (hipGetDevice(&saved) != hipSuccess) saved = -1;
    }
    ~DeviceGuard() {
        if (saved >= 0) (void)hipSetDevice(saved);
    }
};

// Aligned marginal samples (bisbm_align.hip): the pooled histogram with the alignment on is the mode-resolved one with a single
// mode that holds every chain, and both run through one pipeline.  The reference partition the chains of a histogram are
// aligned to:
struct AlignRef {
    bool has = false;
    int64_t chain = -1;           // chain the reference came from; -1: set by the caller
    uint32_t ka = 0, kb = 0;
    std::vector<uint32_t> labels; // n labels
};
// What an engine that runs the kernels (a plain handle, a group, a device entry) keeps of its aligned samples: the list of its
// counted chains sorted by (mode, chain) -- everything on the device is indexed by the position in it --, the buffers and the
// last permutations.
struct AlignScratch {
    uint64_t list_uploaded = 0, ref_uploaded = 0;  // serials of what d_list / d_mode / d_range and what d_ref hold
    std::vector<uint32_t> list;   // counted chains of this engine (index in the engine), sorted by (mode, chain)
    std::vector<uint32_t> pos;    // [n_chains of the engine] position in `list`, BISBM_MODE_NONE: not counted
    DeviceBuf<uint32_t> d_list;   // [counted] `list`
    DeviceBuf<uint32_t> d_mode;   // [counted] mode of every list position: its row of d_ref
    DeviceBuf<uint32_t> d_range;  // [modes + 1] list positions of every mode
    DeviceBuf<uint8_t> d_ref;     // [modes][label_stride] the references
    DeviceBuf<uint32_t> d_tab;    // [counted][ka*ka + kb*kb] overlap tables
    DeviceBuf<uint8_t> d_perm;    // [counted][ka + kb] permutations, global-label form
    DeviceBuf<uint64_t> d_tot;    // [counted][2] overlap totals per type
    bool have_perm = false;
    uint32_t perm_ka = 0, perm_kb = 0;
};

// Label alignment of the pooled marginal histogram.  The mode, the reference and `samples` belong to the handle the caller
// holds; `scratch` belongs to the engines that run the kernels.
struct AlignState {
    int mode = 0;                 // BISBM_ALIGN_NONE / BISBM_ALIGN_REFERENCE
    bool samples = false;         // the internal histogram holds samples (a mode change is refused then)
    AlignRef ref;
    uint64_t serial = 0;          // bumped whenever the reference changes
    AlignScratch scratch;         // kernel-running engine
};

// Replica exchange (bisbm_tempering.hip).  The ladder and the round counter belong to the handle the caller holds and are
// copied to every device entry; the buffers belong to the engines that run the kernels (a plain handle, a device entry).
struct TemperState {
    uint32_t L = 0;               // rungs per ensemble; 0: tempering off
    std::vector<float> ladder;    // L temperatures, non-decreasing
    uint64_t round = 0;           // exchange rounds since bisbm_tempering_set
    // kernel-running engine
    DeviceBuf<float> d_T;                   // [chain] temperature of the chain's rung (SweepParams::T_chain)
    DeviceBuf<uint32_t> d_rung;             // [chain] rung of the chain (MarginalParams::rung)
    DeviceBuf<uint32_t> d_at;               // [ensemble][L] the chain (index in the engine) on every rung
    DeviceBuf<float> d_ladder;              // L temperatures
    DeviceBuf<unsigned long long> d_stats;  // [2][L - 1] attempted, accepted exchanges per rung pair
    DeviceBuf<double> d_beta;               // [L] 1.0 / (double)ladder[i], the host's quotient (HeatbathParams / ReshuffleParams::beta_rung)
    DeviceBuf<unsigned long long> d_rung_stats;  // [L][6] per rung: MH steps, accepted, heat-bath steps, moves, reshuffles proposed, accepted
};

// Population annealing (bisbm_population.hip).  The genealogy and the running totals belong to the handle the caller holds; the
// job list belongs to the engines that run the copy kernel (a plain handle, a device entry).
struct PopulationState {
    std::vector<uint32_t> ancestor;  // [n_chains] chain of the last reset every slot's state descends from; empty: the identity
    uint64_t rounds = 0;             // resampling steps since the last reset: the index of the next step's Philox draw
    double log_ratio_total = 0;      // running sum of the steps' log ratios
    // kernel-running engine
    DeviceBuf<uint2> d_jobs;         // [dead slots of the engine] (dead slot, parent), indices in the engines of the launch
};

// Pair scores (bisbm_pair_scores.hip).  The buffers belong to the engine that owns the graph on a device (a plain handle, the
// container of shape groups, a device entry); the container of device entries keeps only `n`.  The pairs are held sorted by
// (u, v) -- the type-a gather of the kernel then walks the label array forwards --, `order` leads back to the caller's index.
struct PairScoreState {
    uint64_t n = 0;               // pairs set (0: none)
    uint64_t terms = 0;           // chain terms added to every sum since the last set / reset
    DeviceBuf<uint32_t> d_u;      // [n] type-a node of every pair, sorted order
    DeviceBuf<uint32_t> d_v;      // [n] type-b node
    DeviceBuf<double> d_dd;       // [n] (double)d(u) * (double)d(v)
    DeviceBuf<double> d_sum;      // [n] running sums, sorted order
    DeviceBuf<double> d_part;     // [slabs][n] partial sums of one sample
    std::vector<uint32_t> order;  // sorted position -> index in the caller's arrays
};

// Edge probabilities (bisbm_edge_probs.hip).  As PairScoreState: the buffers belong to the engine that owns the graph on a device,
// the container of device entries keeps only `n`; the pairs are held sorted by (u, v).
constexpr uint32_t kEdgeProbsTile = 1024;  // pairs per workgroup of the dS kernel: 256 lanes, 4 pairs each
struct EdgeProbState {
    uint64_t n = 0;               // pairs listed (0: none)
    uint64_t terms = 0;           // chain terms added to every sum since the last set / reset
    uint32_t what = 0;            // BISBM_EDGE_KEEP_LAST
    bool have_last = false;       // d_last holds a sample
    DeviceBuf<uint32_t> d_u, d_v;         // [n] type-a node, type-b node of every pair, sorted order
    DeviceBuf<uint32_t> d_du, d_dv;       // [n] their degrees
    DeviceBuf<uint8_t> d_kind;            // [n] BISBM_EDGE_ADD / BISBM_EDGE_REMOVE
    DeviceBuf<double> d_tdeg, d_tmult;    // [n] the chain-independent terms of dS, in the form of the pair's kind
    DeviceBuf<double> d_dS_sum, d_w_sum;  // [n] running sums, sorted order
    DeviceBuf<double> d_blk;      // [chains of a launch][K][4] block terms
    DeviceBuf<double> d_etat;     // [chains of a launch][K][max_degree + 1][2] eta terms
    DeviceBuf<uint32_t> d_row;    // KEEP_LAST over shape groups: [chains of a launch] row of d_last of every chain
    DeviceBuf<double> d_last;     // KEEP_LAST: [chains of the engine][n] dS of the last sample, NaN: not counted
    std::vector<uint32_t> order;  // sorted position -> index in the caller's arrays
    std::vector<uint32_t> pos;    // index in the caller's arrays -> sorted position
    std::vector<uint32_t> mult;   // [n] present multiplicity of every pair, sorted order
};

// What topk_select (bisbm_topk.hip) needs of device memory for one chunk of queries, T: the cell type of the rows.  It is on the
// engine whose device selects (a plain handle, the first device entry).
template <class T>
struct TopkScratch {
    DeviceBuf<uint8_t> d_mask;     // one byte per cell: the candidates that are not eligible
    DeviceBuf<T> d_rows, d_stage;  // several devices: the chunk's rows added in device order, one device's part
    DeviceBuf<uint32_t> d_node;    // [chunk][k] selected nodes
    DeviceBuf<T> d_val;            // [chunk][k] their cells
};

// Query scores (bisbm_query_scores.hip).  The sums belong to the engine that owns the graph on a device (a plain handle, the
// container of shape groups, a device entry); the container of device entries keeps the host side (n, q, off) only.
struct QueryScoreState {
    uint32_t n = 0;               // queries set (0: none)
    uint32_t n_a = 0;             // ... of type a
    uint64_t terms = 0;           // chain terms added to every sum since the last set / reset
    std::vector<uint32_t> q;      // [n] node of every query, caller's order
    std::vector<uint64_t> off;    // [n + 1] first cell of every query's row; off[n]: cells in all
    DeviceBuf<uint32_t> d_q;      // [n] `q`
    DeviceBuf<uint64_t> d_off;    // [n + 1] `off`
    DeviceBuf<uint32_t> d_list;   // [n] indices of the type-a queries, then of the type-b queries, each ascending
    DeviceBuf<double> d_sum;      // [off[n]] running sums, query by query, candidates in id order
    DeviceBuf<TopkCand> d_cand;   // [n] topk: every query's first candidate (the other type's first node), no self
    TopkScratch<double> topk;
};

// Edge queries (bisbm_edge_queries.hip).  As QueryScoreState: the sums belong to the engine that owns the graph on a device, the
// container of device entries keeps the host side (n, q, off, nbr_ptr, nbr, mult) only.
struct EdgeQueryState {
    uint32_t n = 0;               // queries set (0: none)
    uint32_t n_a = 0;             // ... of type a
    uint64_t terms = 0;           // chain terms added to every sum since the last set / reset
    std::vector<uint32_t> q;      // [n] node of every query, caller's order
    std::vector<uint64_t> off;    // [n + 1] first cell of every query's row; off[n]: cells in all
    std::vector<uint64_t> nbr_ptr;  // [n + 1] first entry of every query's distinct neighbours
    std::vector<uint32_t> nbr;    // the distinct neighbours of every query, ascending
    std::vector<uint32_t> mult;   // ... and how many CSR entries of the query each has
    DeviceBuf<uint32_t> d_q;      // [n] `q`
    DeviceBuf<uint64_t> d_off;    // [n + 1] `off`
    DeviceBuf<uint32_t> d_list;   // [n] indices of the type-a queries, then of the type-b queries, each ascending
    DeviceBuf<uint64_t> d_nbr_ptr;  // `nbr_ptr`
    DeviceBuf<uint32_t> d_nbr;    // `nbr`
    DeviceBuf<double> d_nbr_tmult;  // lg(mu + 2) - lg(mu + 1) of every entry of `nbr`, from the host's table
    DeviceBuf<double> d_sum;      // [off[n]] running sums of w, query by query, candidates in id order
    DeviceBuf<double> d_blk;      // [chains of a launch][K][4] block terms
    DeviceBuf<double> d_etat;     // [chains of a launch][K][max_degree + 1][2] eta terms
    DeviceBuf<double> d_tm;       // [chains of a launch][ka*kb] t_m terms
    DeviceBuf<TopkCand> d_cand;   // [n] topk: every query's first candidate (the other type's first node), no self
    TopkScratch<double> topk;
};

// Co-assignment (bisbm_coassign.hip).  As QueryScoreState: the counts belong to the engine that owns the graph on a device, the
// container of device entries keeps the host side (n, q, off) only.
struct CoassignState {
    uint32_t n = 0;               // queries set (0: none)
    uint32_t n_a = 0;             // ... of type a
    uint32_t q_slots = 0;         // slots per chain in d_qlab: both types padded to whole query tiles
    uint64_t terms = 0;           // counted (sample, chain) pairs since the last set / reset
    std::vector<uint32_t> q;      // [n] node of every query, caller's order
    std::vector<uint64_t> off;    // [n + 1] first cell of every query's row; off[n]: cells in all
    DeviceBuf<uint32_t> d_q;      // [n] `q`
    DeviceBuf<uint64_t> d_off;    // [n + 1] `off`
    DeviceBuf<uint32_t> d_list;   // [n] indices of the type-a queries, then of the type-b queries, each ascending
    DeviceBuf<uint32_t> d_slot;   // [q_slots] query index of every slot of d_qlab, 0xffffffff: padding
    DeviceBuf<uint32_t> d_qlab;   // [chains of the engine sampled][q_slots] the queries' labels of one sample
    DeviceBuf<uint32_t> d_count;  // [off[n]] counts, query by query, candidates in id order
    DeviceBuf<TopkCand> d_cand;   // [n] topk: every query's first candidate (its own type's first node) and its own cell
    TopkScratch<uint32_t> topk;
};

// Fold-in queries (bisbm_foldin.hip).  As QueryScoreState: the sums, the tables and the posteriors of the last sample belong to
// the engine that owns the graph on a device, the container of device entries keeps the host side only.  A row kind that is not
// kept has no cells (its `off` is all 0).
struct FoldinState {
    uint32_t n = 0;               // virtual nodes set (0: none)
    uint32_t n_a = 0;             // ... of type a
    uint32_t what = 0;            // BISBM_FOLDIN_RECOMMEND | BISBM_FOLDIN_SIMILAR: the row kinds kept
    double alpha = 0;
    uint64_t terms = 0;           // chain terms added to every sum since the last set / reset
    std::vector<uint8_t> type;    // [n] 0: a, 1: b, caller's order
    std::vector<uint64_t> ptr;    // [n + 1] first list entry of every virtual node, caller's order
    std::vector<uint32_t> list;   // the lists
    std::vector<uint32_t> slot;   // [n] slot of every virtual node: the type-a ones in order, then the type-b ones
    std::vector<uint64_t> off[2]; // [n + 1] first cell of every node's recommend / similar row
    DeviceBuf<TopkCand> d_cand[2];  // [n] topk: the first candidate of every node's recommend / similar row, no self
    DeviceBuf<uint64_t> d_ptr;    // [n + 1] `ptr`
    DeviceBuf<uint32_t> d_nbr;    // `list`
    DeviceBuf<uint32_t> d_order;  // [n] caller's index of every slot
    DeviceBuf<uint64_t> d_off[2]; // `off`
    DeviceBuf<double> d_sum[2];   // running sums of the recommend / similar rows
    DeviceBuf<double> d_P;        // posteriors of the last sample: the segments below back to back
    DeviceBuf<double> d_g;        // recommend tables of one chunk of chains
    // the last sample's posteriors, one segment per leaf: chains ridx[..] of this engine, shape (ka, kb), from d_P[base] on
    struct Segment {
        uint32_t ka = 0, kb = 0;
        size_t base = 0;
        std::vector<uint32_t> chain;
    };
    std::vector<Segment> segments;
    TopkScratch<double> topk;
};

// Node conditionals (bisbm_conditionals.hip).  As FoldinState: the sums, the soft marginals and the rows of the last sample belong
// to the engine that owns the graph on a device, the container of device entries keeps the host side (n, q, nbb, ref) only.  A
// chain's rows: the queries' rows back to back in the caller's order, K_own doubles each -- query i starts at
// (i - nbb[i]) * ka + nbb[i] * kb.
struct ConditionalState {
    uint32_t n = 0;               // queries set (0: none)
    uint32_t n_b = 0;             // ... of type b
    uint32_t what = 0;            // BISBM_COND_KEEP_LAST
    double beta = 0;
    bool held = false;            // bisbm_held_conditionals_set: the rows are the held ones (on every engine of the handle)
    uint64_t terms = 0;           // chain terms added to the label-free sums since the last set / reset
    uint64_t prob_terms = 0;      // ... to the soft marginals (they start afresh whenever the reference is set)
    std::vector<uint32_t> q;      // [n] node of every query, caller's order
    std::vector<uint32_t> nbb;    // [n + 1] type-b queries before every query
    AlignRef ref;                 // the caller's reference partition of the soft marginals (has: they are kept)
    uint64_t ref_serial = 0;      // bumped whenever the reference changes
    DeviceBuf<uint32_t> d_q;      // [n] `q`
    DeviceBuf<uint32_t> d_nbb;    // [n + 1] `nbb`
    DeviceBuf<double> d_stat;     // [3][n] stay_sum, entropy_sum, margin_sum
    DeviceBuf<unsigned long long> d_free;  // [n] counted chains in which the query's node was free
    DeviceBuf<double> d_prob;     // [n][max(ref.ka, ref.kb)] soft marginals
    size_t prob_cells = 0;
    DeviceBuf<double> d_dS, d_P;  // rows: of the last sample, the segments below back to back (KEEP_LAST), else of one chunk of chains
    DeviceBuf<double> d_terms;    // [chunk][n][4] stay, entropy, margin, free of one chunk of chains
    // the last sample's rows, one segment per leaf: chains ridx[..] of this engine, shape (ka, kb), from d_dS[base] / d_P[base] on
    struct Segment {
        uint32_t ka = 0, kb = 0;
        size_t base = 0;
        std::vector<uint32_t> chain;
    };
    std::vector<Segment> segments;
    AlignScratch scratch;         // (its own: the permutations of a conditional sample are not the marginal histogram's)
    // bisbm_least_settled_topk, on the device that selects: one row of n cells -- its bounds {0, n}, its TopkCand {0, none}
    DeviceBuf<uint64_t> d_sel_off;
    DeviceBuf<TopkCand> d_sel_cand;
    TopkScratch<double> topk;
};

// Pair reshuffles (bisbm_reshuffle.hip).  Everything belongs to the engine that runs the kernel (a plain handle, a group, a
// device entry): the scratch of the moves, and the records and accepted counts of the last call as the host read them back.
struct ReshuffleState {
    DeviceBuf<uint8_t> d_scratch;  // [chains][max(na, nb)] member ids (4 bytes), then original labels, then launch labels (1 each)
    DeviceBuf<bisbm_reshuffle_record> d_record;    // [chains] the last move of the last call
    DeviceBuf<unsigned long long> d_accepted;      // [chains] accepted moves of the last call
    std::vector<bisbm_reshuffle_record> last;      // (empty: no call yet)
    std::vector<unsigned long long> accepted;
};

// Split and merge moves (bisbm_split_merge.hip).  Everything belongs to the device entry (a plain handle, an entry of `devs`),
// indexed by the entry's own chain order whatever the grouping by shape of the moment: the groups come and go with the moves.
struct SplitMergeState {
    std::vector<uint32_t> proposed;                 // [chains] j: split / merge moves proposed so far (empty: none yet)
    std::vector<uint64_t> totals;                   // [chains][4] splits proposed, accepted, merges proposed, accepted
    std::vector<bisbm_split_merge_record> last;     // [chains] (empty: no call yet)
    double call_ms = 0, regroup_ms = 0;             // host clock of the last call on this entry, and its part spent forming groups
    // scratch of one launch over all groups of the entry, each group a slice: the chains' state with a spare block per type
    DeviceBuf<uint8_t> d_labels;                    // [chains][label_stride]
    DeviceBuf<int32_t> d_m, d_m_r, d_n_r;
    DeviceBuf<uint32_t> d_eta;
    DeviceBuf<uint8_t> d_scratch;                   // as ReshuffleState::d_scratch
    DeviceBuf<bisbm_split_merge_record> d_record;   // [chains]
    DeviceBuf<uint32_t> d_proposed;                 // [chains] `proposed` in launch order
    DeviceBuf<uint8_t> d_jobs;                      // the regrouping's copy jobs (the unit's ChainCopy, as bytes)
};

// Partition distances (bisbm_partition.hip).  The scratch of the calls, on the engine whose device computes (a plain handle, the
// container of shape groups, the first device entry); nothing of it outlives a call in meaning, it is only kept to be reused.
struct PartitionState {
    DeviceBuf<uint8_t> d_desc;    // [selection] row pointer, ka, kb of every selected chain (the unit's ChainDesc, as bytes)
    DeviceBuf<uint2> d_tiles;     // [tiles] (row tile, column tile)
    DeviceBuf<double> d_A;        // [selection] sum_r a_r ln a_r
    DeviceBuf<double> d_snn;      // [selection][selection] sum_rs n_rs ln n_rs of every pair i < j
    DeviceBuf<uint32_t> d_tab;    // few pairs: the integer tables of one launch
    DeviceBuf<uint8_t> d_stage;   // label rows of selected chains that live on another device
    DeviceBuf<uint8_t> d_refs;    // distances_to: the caller's reference partitions as byte rows, padded like label rows
};

// Chain traces (bisbm_trace.hip).  The depth, the sums and the series belong to the handle the caller holds, in its chain order;
// the ring and the scratch belong to every device entry (a plain handle, an entry of `devs`) for its own chains, whatever their
// grouping by shape.
struct TraceState {
    uint32_t depth = 0;              // snapshots held per chain; 0: off
    uint64_t records = 0;            // records since the last set / reset; the next one goes to slot records % depth
    std::vector<double> A_ring;      // [depth][n_chains] sum_r a_r ln a_r of every held snapshot
    std::vector<uint32_t> snap_ka, snap_kb;  // [n_chains] the shape the held snapshots were taken with
    std::vector<double> vi_sum, vi_last;     // [n_chains][depth]
    std::vector<uint64_t> agree_sum;         // [n_chains][depth]
    std::vector<uint64_t> pairs;             // [depth]
    std::vector<double> S, H;        // [records][n_chains]
    // device entry
    DeviceBuf<uint8_t> d_ring;       // [depth][chains of the entry][label_stride] label rows
    DeviceBuf<uint8_t> d_desc;       // [chains] row pointer, ka, kb of the current partitions (ChainDesc, as bytes)
    DeviceBuf<double> d_A;           // [chains] sum_r a_r ln a_r now
    DeviceBuf<double> d_snn;         // [chains][ages] sum_rs n_rs ln n_rs
    DeviceBuf<unsigned long long> d_agree;   // [chains][ages] sum_r n_rr
    DeviceBuf<uint32_t> d_tab;       // few workgroups or a table beyond the LDS: the integer tables of one launch
};

// Mode-resolved marginals (bisbm_mode_marginals.hip).  The assignment of chains to modes, the references and `terms` belong to
// the handle the caller holds; `scratch` and the histogram slices belong to the engines that run the kernels (a plain handle, a
// device entry: chains grouped by shape are refused).
struct ModeState {
    uint32_t n_modes = 0;            // 0: off
    std::vector<uint32_t> of_chain;  // [n_chains] mode of every chain of the handle, BISBM_MODE_NONE: not counted
    std::vector<AlignRef> refs;      // [n_modes]
    std::vector<uint64_t> terms;     // [n_modes] chain samples in every mode's histogram
    uint64_t list_serial = 0;        // bumped whenever the assignment changes
    uint64_t ref_serial = 0;         // bumped whenever a reference changes
    // anchored modes (bisbm_marginals_set_mode_anchors): refs are the anchors, of_chain is the last sample's assignment
    bool anchored = false;
    double threshold = 0;            // a chain farther than this from its nearest anchor is not counted
    std::vector<double> vi_last;     // [n_chains][n_modes] VI of the last sample, NaN rows: chains that were not counted
    std::vector<uint64_t> visits;    // [n_chains][n_modes] samples of chain c counted into mode g
    uint64_t unassigned = 0, samples = 0;
    uint64_t pending_unassigned = 0; // counted chains of the sample under way that are beyond the threshold
    // kernel-running engine
    DeviceBuf<uint8_t> d_anchor;     // [n_modes][label_stride] the anchors as byte rows (anchored modes only)
    AlignScratch scratch;            // (its own, not AlignState's: a pooled sample's permutations are not a mode's)
    DeviceBuf<uint32_t> d_counts;    // [slices][n][max(hist_ka, hist_kb)] one histogram per mode
    uint32_t slices = 0, hist_ka = 0, hist_kb = 0;  // what d_counts holds (slices 0: nothing)
    DeviceBuf<uint32_t> d_sum, d_stage;  // map_mode over several devices: the slices of a mode added on the first device
    DeviceBuf<uint16_t> d_lab;       // map_mode: labels
    DeviceBuf<uint32_t> d_top;       // map_mode: winning counts
};

// Block summaries (bisbm_block_sums.hip).  What is kept, the shape, the terms and the last sample's assignment belong to the
// handle the caller holds; the sums belong to every device entry (a plain handle, an entry of `devs`: the groups of an entry add
// into its buffer as they do into its histogram), the last sample's tables to the engines that run the kernels.
struct BlockSumState {
    uint32_t what = 0;               // BISBM_BLOCK_SUMS | BISBM_BLOCK_KEEP_LAST; 0: off
    uint32_t ka = 0, kb = 0;         // the shape the sums were started with
    uint64_t serial = 1;             // bumped whenever the sums start afresh (it never goes back: a buffer zeroed for an older one is stale)
    std::vector<uint64_t> terms;     // [modes] chain samples in every mode's sums (empty: no sample since they started)
    std::vector<uint32_t> last_mode; // [n_chains] the mode the last sample counted every chain into, BISBM_MODE_NONE: none (empty: no sample)
    // device entry
    DeviceBuf<unsigned long long> d_sums;  // [slices][3][ka*kb + 2 K] sum, sq_lo, sq_hi of the cells E, N, D
    uint64_t zeroed = 0;             // the serial d_sums was zeroed for
    uint32_t slices = 0;
    // kernel-running engine
    DeviceBuf<int32_t> d_last;       // [list position][ka*kb + 2 K] the aligned tables of the last sample (KEEP_LAST)
    uint64_t last_serial = 0;        // the serial d_last was written under
};

// Clamped nodes (bisbm_clamp.hip).  The mask as the caller gave it belongs to the handle the caller holds; the device copy and
// the lists of the open nodes belong to every device entry (a plain handle, an entry of `devs`: chains grouped by shape are refused).
struct ClampState {
    uint64_t n_clamped = 0;        // non-zero bytes of the mask; 0: no clamp, and no kernel is handed the mask
    std::vector<uint8_t> mask;     // [n] 0 / 1 (empty: no clamp)
    // device entry
    uint32_t open_a = 0, open_b = 0;  // open nodes of type a / of type b
    DeviceBuf<uint8_t> d_mask;     // [n]
    DeviceBuf<uint32_t> d_open;    // [open_a + open_b] the open nodes of type a, then of type b, each ascending
    const uint8_t* mask_or_null() const { return n_clamped ? d_mask.get() : nullptr; }
};

// Block constraints (bisbm_constraints.hip).  The class bytes and the table belong to the handle the caller holds and, with
// the device copies, to every device entry (chains grouped by shape are refused).  n_classes == 0: no constraints, and no kernel
// is handed a pointer -- a table under which every node may sit in every block of its type is stored as that.
struct ConstraintState {
    uint32_t n_classes = 0;
    std::vector<uint8_t> cls;      // [n] class of every node
    std::vector<uint8_t> allowed;  // [n_classes][K] 0 / 1 as given
    std::vector<uint32_t> bits;    // [n_classes][8] the bit table
    // device entry
    DeviceBuf<uint8_t> d_class;    // [n]
    DeviceBuf<uint32_t> d_bits;    // [n_classes][8]
    // the shuffle's list: the nodes that are open under the clamp in place, sorted by (type, class, id); segment g holds
    // d_open[seg[g] .. seg[g + 1]) and has the key (type << 8) | class.  Rebuilt when the clamp or the constraints change.
    DeviceBuf<uint32_t> d_open, d_seg, d_seg_key;
    uint32_t n_segs = 0;
    const uint8_t* class_or_null() const { return n_classes ? d_class.get() : nullptr; }
    const uint32_t* bits_or_null() const { return n_classes ? d_bits.get() : nullptr; }
    bool allows(uint64_t v, uint32_t s) const { return ((bits[(size_t)cls[v] * 8 + (s >> 5)] >> (s & 31u)) & 1u) != 0u; }
};

// Block fields (bisbm_fields.hip).  The class bytes and the table belong to the handle the caller holds and, with the device
// copies, to every device entry (chains grouped by shape are refused).  n_classes == 0: no fields, and no kernel is handed a
// pointer -- a table of zeros is stored as that.
struct FieldState {
    uint32_t n_classes = 0;
    std::vector<uint8_t> cls;    // [n] field class of every node
    std::vector<double> field;   // [n_classes][K] as given
    // device entry
    DeviceBuf<uint8_t> d_class;  // [n]
    DeviceBuf<double> d_field;   // [n_classes][K]
    DeviceBuf<double> d_phi;     // [n_chains] Phi of every chain (fields_energy_device)
    const uint8_t* class_or_null() const { return n_classes ? d_class.get() : nullptr; }
    const double* field_or_null() const { return n_classes ? d_field.get() : nullptr; }
};

}  // namespace bisbm

// ------------------------------------------------------------------------------------------
// the handle
// ------------------------------------------------------------------------------------------
struct bisbm_engine {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    // shape
    uint64_t n = 0, na = 0, nb = 0, num_edges = 0, nnz = 0;
    uint32_t ka = 0, kb = 0, K = 0, maxdeg = 0, n_chains = 0, first_chain_id = 0;
    double epsilon = 0;
    int rng_mode = 0;
    uint64_t seed = 0, gen_seed = 0;
    bool state_ready = false;
    // device memory
    uint32_t* d_rowptr = nullptr;
    uint32_t* d_col = nullptr;
    uint8_t* d_labels = nullptr;      // [chain][label_stride] labels: bytes, or two bytes each while `wide`
    uint8_t* d_labels_tmp = nullptr;
    size_t label_stride = 0;          // in labels
    bool wide = false;                // KA + KB > 256 (a --merge run starts at one block per node): generic kernel only,
                                      // two-byte labels, m read and updated in HBM; back to bytes once K <= 256
    size_t lbytes() const { return wide ? 2 : 1; }
    uint32_t* d_vlist = nullptr;
    int32_t* d_m = nullptr;
    int32_t* d_m_r = nullptr;
    int32_t* d_n_r = nullptr;
    uint32_t* d_eta = nullptr;
    bisbm::ChainScalars* d_scalars = nullptr;
    uint32_t* d_simd_claims = nullptr;  // production kernel: stepping-wave claims per SIMD, zeroed before every launch
    uint32_t* d_mt_engine = nullptr;
    uint32_t* d_mt_gen = nullptr;
    double* d_lgamma = nullptr;
    double* d_logtab = nullptr;
    double* d_q = nullptr;
    bisbm::DeviceBuf<double> d_T;  // temperature table of the pow / log schedules (bisbm_anneal)
    double* d_tmp_f64 = nullptr;  // n_chains doubles
    // block-state part of the description length of every chain as the last production launch without early-stop bookkeeping
    // left it (such launches do not keep the running sum of accepted dS: bisbm_anneal advances it by the change of this,
    // sweep_fast_tracks_minimum); valid while nothing else has changed the block state since
    double* d_ent_prev = nullptr;
    bool ent_prev_valid = false;
    uint32_t* d_stage_u32 = nullptr;  // n uint32 staging
    uint32_t* d_counts = nullptr;     // internal marginal buffer n*kmax
    uint32_t counts_kmax = 0;         // columns d_counts was sized for
    uint32_t counts_cols = 0;         // columns of the histogram it currently holds (max(KA, KB) at the last reset)
    uint32_t counts_ka = 0, counts_kb = 0;  // ... and the block counts it was started for: a column means a block of that numbering
    // does the internal histogram hold samples of these block counts?  (Not of their maximum alone: 3 + 2 and 3 + 1 blocks share
    // a row length and no numbering.)
    bool counts_fit(uint32_t ka_now, uint32_t kb_now) const { return d_counts && counts_ka == ka_now && counts_kb == kb_now; }
    uint32_t cap_ka = 0, cap_kb = 0;  // block counts d_m / d_m_r / d_n_r / d_eta are allocated for
    std::shared_ptr<bisbm::HostTables> tab;
    uint32_t q_stride = 0;
    // chain-independent part of entropy()
    double ent_deg = 0, ent_multi = 0;
    // nodes of every degree 0..256 per type (256: all longer rows), shared with the sub-engines: what the production kernel's
    // eta window is placed by (bisbm_anneal)
    std::shared_ptr<std::vector<uint64_t>> deg_count;
    // last sweep timing
    double last_kernel_ms = 0;
    uint64_t last_updates = 0;
    uint32_t last_pass_steps = 0;  // steps per pass of the last sweep launch (1, 2, 4, 8)
    uint32_t last_route = 0;       // BISBM_ROUTE_* bits of the last MH sweep launch (a container: its first member's); 0: none yet
    uint32_t last_eta_plan[4] = {0, 0, 0, 0};  // {eta_in_lds, eta_w, eta_lo_a, eta_lo_b} of the last sweep launch (a container: its first member's)
    // which depth of pass (two / four / eight steps) the next production launch runs: chosen from the timed launches so far
    // (bisbm_pass_policy.hpp); belongs to a partition: init / shuffle / merges / splits reset it
    bisbm::PassDepthPolicy passes;
    double last_acc_frac = -1.;  // accepted fraction of the last timed sweep launch (-1: none yet): picks SweepParams::one_stage
    // Chains with different block counts (after a one-argument agg_merge, blockmodel.cc:208-271: every run ends where it
    // ends).  Kernels are launched for one (KA, KB), so the handle then becomes a CONTAINER: its chains live in
    // sub-engines, one per distinct shape (`groups`), which borrow the graph and the tables from it (`root`); chain c of
    // the handle is chain where[c].second of group where[c].first.  A sub-engine knows the global id of each of its
    // chains (`gids`, the key of the Philox streams) and its index in the handle (`ridx`).
    std::vector<bisbm_engine*> groups;
    std::vector<std::pair<uint32_t, uint32_t>> where;
    bisbm_engine* root = nullptr;
    std::vector<uint32_t> gids, ridx;
    uint32_t* d_gids = nullptr;
    uint32_t gid(size_t c) const { return gids.empty() ? first_chain_id + (uint32_t)c : gids[c]; }
    // Several devices behind one handle (bisbm_create_multi): the handle is a container of one full engine per device
    // (`devs`; graph and tables replicated, one stream and one host thread per device); chains dev_first[i] ..
    // dev_first[i + 1] - 1 of the handle live in devs[i], in order, so global chain ids -- the keys of the random streams --
    // do not depend on the number of devices.  `pool`: what the pooling of the marginal histogram over the devices needs.
    std::vector<bisbm_engine*> devs;
    std::vector<uint32_t> dev_first;
    struct DevicePool* pool = nullptr;
    uint64_t counts_rows = 0;  // rows of the internal marginal buffer (n, or n rounded up to a multiple of the device count)
    bisbm::AlignState align;
    bisbm::TemperState temper;
    bisbm::PopulationState population;
    bisbm::PairScoreState pairs;
    bisbm::EdgeProbState edges;
    bisbm::QueryScoreState queries;
    bisbm::EdgeQueryState edge_queries;
    bisbm::CoassignState coassign;
    bisbm::FoldinState foldin;
    bisbm::ConditionalState cond;
    bisbm::ReshuffleState reshuffle;
    bisbm::SplitMergeState split_merge;
    bisbm::PartitionState partition;
    bisbm::ModeState modes;
    bisbm::TraceState trace;
    bisbm::BlockSumState blocks;
    bisbm::ClampState clamp;
    bisbm::ConstraintState constraints;
    bisbm::FieldState fields;
};

namespace bisbm {

extern thread_local std::string g_create_error;  // message of a failed bisbm_create (there is no handle to hold it)

int fail(bisbm_engine* h, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return fail((h), BISBM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// room for `count` elements in a DeviceBuf, or the call fails with the function, the buffer and the size in the message
// (RESERVE_AS: the function is the C call a shared helper works for)
#define RESERVE_AS(h, fn, buf, count)                                                                                       \
    do {                                                                                                                    \
        const size_t n_ = (count);                                                                                          \
        hipError_t e_ = (buf).reserve(n_);                                                                                  \
        if (e_ != hipSuccess)                                                                                               \
            return fail((h), BISBM_ERR_HIP, "%s: %zu bytes of device memory for " #buf " could not be allocated: %s", (fn), \
                        n_ * sizeof(*(buf).get()), hipGetErrorString(e_));                                                  \
    } while (0)
#define RESERVE(h, buf, count) RESERVE_AS(h, __func__, buf, count)

void free_chain_arrays(bisbm_engine* h);
void free_all(bisbm_engine* h);
void mt_seed_host(uint32_t* mt, uint64_t seed);  // std::mt19937(seed): seed mod 2^32
// phx_draw and u53 of bisbm_device.hpp on the host: the same integers
inline void philox_host(uint64_t seed, uint32_t chain, uint32_t purpose, uint64_t idx, uint32_t out[4]) {
    uint32_t c0 = (uint32_t)idx, c1 = (uint32_t)(idx >> 32), c2 = chain, c3 = purpose;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}
inline double u53_host(uint32_t hi, uint32_t lo) { return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1.0p-53; }
inline void forget_pass_speeds(bisbm_engine* h) {
    h->passes.reset();
    h->last_acc_frac = -1.;
}
int rebuild_state(bisbm_engine* h);
// block-state part of entropy() of every chain into d_out (n_chains doubles on the device), on the handle's stream, no sync
int launch_block_entropy(bisbm_engine* h, double* d_out);

// container handles (bisbm_engine::groups): run `f` on every group, first error wins
template <class F>
int each_group(bisbm_engine* h, F f) {
    for (bisbm_engine* g : h->groups) {
        const int rc = f(g);
        if (rc) {
            h->err = g->err;
            return rc;
        }
    }
    return BISBM_OK;
}
// do all chains under the handle have one shape (again)?  If so the ka / kb / K of the containers on the way follow it.
bool common_shape(bisbm_engine* h);
// ... and the block counts they share, or BISBM_ERR_STATE with the one message of that refusal (the marginal calls, alignment)
int shared_shape(bisbm_engine* h, uint32_t* ka, uint32_t* kb);
// ... and gather one value per chain from the groups into the handle's chain order
template <class T, class F>
int gather_groups(bisbm_engine* h, T* out, F f) {
    return each_group(h, [&](bisbm_engine* g) {
        std::vector<T> tmp(g->n_chains);
        const int rc = f(g, tmp.data());
        if (rc == BISBM_OK && out)
            for (size_t j = 0; j < tmp.size(); ++j) out[g->ridx[j]] = tmp[j];
        return rc;
    });
}

// LDS of the generic kernel without the optional parts (eta, the visit list): the a x b quadrant of m (odd row stride; in
// HBM while wide), m_r, n_r, the k_v histogram, staged rows; compat mode adds two mt19937 states and their tempered outputs.
// Wide mode (KA + KB > 256) therefore ends where m_r / n_r / the histogram leave the 160 KiB of a CU -- about 11 000 to
// 18 000 blocks depending on the split and the RNG mode -- well below what two-byte labels could name.
size_t generic_lds_base_bytes(uint32_t ka, uint32_t kb, bool wide, int rng_mode);
constexpr size_t kLdsPerCu = 160 * 1024;

// fn(c) for every chain, on up to 16 host threads when there are enough chains.  An exception that left a worker thread
// (std::bad_alloc from a chain's host-side merge state) would end the process through std::terminate, and one that left
// the calling thread would cross the C boundary: both are caught here and reported as `false`.
template <class F>
bool for_each_chain(size_t C, F&& fn) {
    std::atomic<bool> ok{true};
    auto guarded = [&](size_t c) {
        try {
            fn(c);
        } catch (...) {
            ok = false;
        }
    };
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(16, std::thread::hardware_concurrency()), C / 4));
    if (nt <= 1) {
        for (size_t c = 0; c < C; ++c) guarded(c);
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back([&, t] {
                for (size_t c = t; c < C; c += nt) guarded(c);
            });
        for (auto& x : th) x.join();
    }
    return ok;
}

// ---- several devices behind one handle (bisbm_multi.hip) ------------------------------------------------------------------
inline uint32_t dev_of_chain(const bisbm_engine* h, uint32_t chain, uint32_t* local) {
    uint32_t i = 0;
    while (i + 1 < h->devs.size() && chain >= h->dev_first[i + 1]) ++i;
    *local = chain - h->dev_first[i];
    return i;
}

// fn(engine of device i, i) on one host thread per device
template <class F>
int on_devices(bisbm_engine* h, F&& fn) {
    const size_t nd = h->devs.size();
    std::vector<int> rcs(nd, BISBM_OK);
    if (nd == 1) {
        rcs[0] = fn(h->devs[0], (size_t)0);
    } else {
        std::vector<std::thread> th;
        for (size_t i = 0; i < nd; ++i)
            th.emplace_back([&, i] {
                try {
                    rcs[i] = fn(h->devs[i], i);
                } catch (...) {
                    rcs[i] = BISBM_ERR_STATE;
                    h->devs[i]->err = "out of host memory";
                }
            });
        for (auto& t : th) t.join();
    }
    // the first failing device's code is returned; the message names every device that failed (the others have done their
    // part of the call: see bisbm_agg_merge in include/bisbm.h for what that means for calls that change state)
    int rc = BISBM_OK;
    std::string msg;
    for (size_t i = 0; i < nd; ++i)
        if (rcs[i]) {
            if (!rc) rc = rcs[i];
            msg += (msg.empty() ? "" : "; ") + ("device " + std::to_string(h->devs[i]->device) + ": " + h->devs[i]->err);
        }
    if (rc) h->err = msg;
    return rc;
}

// ---- one walk over a handle: a plain engine, a container of shape groups, a container of device entries (bisbm_handle.hip) ----
// the device entries: the handle itself, or `devs`
std::vector<bisbm_engine*> device_entries(bisbm_engine* h);
// the engines that run kernels under the handle (a plain handle; its groups; the device entries and their groups), in device
// order, then group order
std::vector<bisbm_engine*> leaves(bisbm_engine* h);
// f(device entry) of every device entry, in device order
template <class F>
auto per_device(bisbm_engine* h, F f) {
    std::vector<decltype(f(h))> out;
    for (bisbm_engine* d : device_entries(h)) out.push_back(f(d));
    return out;
}
// the chain terms all device entries have added since the last set / reset of the feature whose state is `state`
template <class S>
uint64_t total_terms(bisbm_engine* h, S bisbm_engine::*state) {
    uint64_t t = 0;
    for (bisbm_engine* d : device_entries(h)) t += (d->*state).terms;
    return t;
}
// the indices of the type-a queries (q[i] < na), then of the type-b ones, each ascending, into `list`; returns how many are type a
inline uint32_t partition_by_type(const std::vector<uint32_t>& q, uint64_t na, std::vector<uint32_t>& list) {
    list.resize(q.size());
    std::iota(list.begin(), list.end(), 0u);
    return (uint32_t)(std::stable_partition(list.begin(), list.end(), [&](uint32_t i) { return q[i] < na; }) - list.begin());
}

// ---- rows of cells per query, one set per device entry (bisbm_topk.hip; T: uint32_t, double) ------------------------------
// `cells`: every device entry's cells, in device order (per_device).  `len` cells from cell `at` on into `out`: over several
// devices the entries' cells added on the host in device order.
template <class T>
int read_row(bisbm_engine* h, const std::vector<const T*>& cells, uint64_t at, size_t len, T* out);
// The tail of the three *_topk calls (`fn`: the call's name, for the messages): the best k candidates of every query into
// node_out / val_out ([queries][k]; val_out may be NULL).  off: the host's first cell of every query's row; w, d_off, d_cand:
// the scratch and the tables of the first device entry, which selects; lists: what to mask, NULL: nothing.  Walks the queries in
// chunks of at most kTopkChunkCells cells (BISBM_TOPK_CHUNK_CELLS=<n> in the environment, read at every call: n instead, for the
// tests), never less than one query.  ascending: the smallest cells first (f64 rows without a mask only).
template <class T>
int topk_select(bisbm_engine* h, const char* fn, const std::vector<const T*>& cells, const std::vector<uint64_t>& off, TopkScratch<T>& w,
                const uint64_t* d_off, const TopkCand* d_cand, const TopkMaskLists* lists, uint32_t k, uint32_t* node_out, T* val_out,
                bool ascending = false);

// edge probabilities and edge queries: how many consecutive chains of `e` one launch serves -- as many as keep the eta terms
// under the byte cap of a launch; bisbm_edge_probs.hip
uint32_t edge_range_chains(const bisbm_engine* e);

bool any_grouped(bisbm_engine* h);  // does the handle, or one of its device entries, keep its chains grouped by shape?
bool any_wide(bisbm_engine* h);     // does some leaf hold two-byte labels?
// the leaf that runs chain `chain` of the handle, and the chain's index there
bisbm_engine* leaf_of_chain(bisbm_engine* h, uint32_t chain, uint32_t* local);
// f(leaf, index there) for the leaf of one chain; the leaf's message becomes the handle's when it fails
template <class F>
int on_leaf_of_chain(bisbm_engine* h, uint32_t chain, F f) {
    bisbm_engine* e = leaf_of_chain(h, chain, &chain);
    const int rc = f(e, chain);
    if (rc && e != h) h->err = e->err;
    return rc;
}
// f(leaf) for every leaf: one host thread per device entry, the groups of an entry in order
template <class F>
int each_leaf(bisbm_engine* h, F&& f) {
    if (!h->devs.empty())
        return on_devices(h, [&](bisbm_engine* d, size_t) { return each_leaf(d, f); });
    if (!h->groups.empty()) return each_group(h, [&](bisbm_engine* g) { return f(g); });
    return f(h);
}

int multi_anneal(bisbm_engine* h, int schedule, const float kwargs[2], uint64_t duration_steps, uint64_t steps_await, double* acc_rate_out);
int multi_marginals_get(bisbm_engine* h, uint32_t* counts_out);
int multi_marginals_map(bisbm_engine* h, uint32_t* labels_out);
void multi_free(bisbm_engine* h);
// MAP labels from the internal histogram of one engine (no pooling); bisbm_marginals.hip
int single_marginals_map(bisbm_engine* h, uint32_t* labels_out);
// bisbm_entropy's full description length is t[0] + (block-state part) + t[1] + ... + t[7], added in that order (bisbm_handle.hip)
void entropy_terms(const bisbm_engine* h, double t[8]);
// bisbm_anneal on a kernel-running engine with a temperature per chain (T_chain: device pointer, NULL: none); bisbm_anneal.hip
int anneal_engine(bisbm_engine* h, int schedule, const float kwargs[2], uint64_t duration_steps, uint64_t steps_await,
                  double* acc_rate_out, const float* T_chain);
// A launch of a wave-chain move kernel (bisbm_wave_chain.hpp) on a kernel-running engine: the fields every such kernel takes
// (per_rung as below), then where eta goes -- LDS when the kernel's own arrays (own_bytes) and the chain state with eta stay
// within 40 KiB -- and the LDS bytes to launch with, BISBM_ERR_UNSUPPORTED when they exceed kLdsPerCu; bisbm_heatbath.hip
void wave_chain_fill(const bisbm_engine* h, double beta, bool per_rung, WaveChainParams& p);
int wave_chain_plan(bisbm_engine* h, size_t own_bytes, WaveChainParams& p, size_t& lds);
// `sweeps` heat-bath sweeps of a kernel-running engine on its stream; per_rung: every chain at the beta of its rung
// (TemperState::d_beta, d_rung) instead of `beta`; sync: wait for the stream before returning; bisbm_heatbath.hip
int heatbath_engine(bisbm_engine* h, uint64_t sweeps, double beta, int stop_when_settled, bool per_rung, bool sync);
// `moves` pair reshuffles of a kernel-running engine on its stream, per_rung as above; read_back: wait for the stream and copy the
// records and accepted counts of the call to the host (ReshuffleState::last / accepted), otherwise they stay on the device and
// `last` is emptied; bisbm_reshuffle.hip
int reshuffle_engine(bisbm_engine* h, uint64_t moves, uint32_t scans, double beta, bool per_rung, bool read_back);
int reshuffle_read_back(bisbm_engine* h);  // ... the copy alone, after a wait for the stream
// chains of one handle in different shapes (bisbm_merge.hip): a sub-engine of `root` for `count` chains of shape (ka, kb) with its
// own per-chain arrays, stream and events, graph and tables borrowed (NULL and `err` when an allocation fails); and root->where
// from the groups' ridx.  The split and merge moves regroup with them.
bisbm_engine* new_group(bisbm_engine* root, uint32_t ka, uint32_t kb, uint32_t count, std::string& err);
void remap_groups(bisbm_engine* root);
// block constraints: the shuffle's list of a device entry (ConstraintState::d_open) from the entry's constraints and the clamp
// mask given (0 / 1 bytes, empty: none); nothing to do without constraints.  bisbm_clamp_set calls it for every mask it puts in
// place; bisbm_constraints.hip
int constraints_rebuild_open(bisbm_engine* e, const std::vector<uint8_t>& clamp_mask);
// block fields: Phi of every chain of a kernel-running engine that has fields, into its FieldState::d_phi on its stream (no
// wait); what bisbm_fields_energy, the exchange round and the resampling step all read.  bisbm_fields.hip
int fields_energy_device(bisbm_engine* e);
// BISBM_ERR_INVALID_ARG when a move of up to max(na, nb) members with `scans` launch scans could use 2^32 draws or more
int reshuffle_check_scans(bisbm_engine* h, uint32_t scans);
// bisbm_marginals_accumulate with the alignment on; bisbm_align.hip
int align_accumulate(bisbm_engine* h, uint32_t* device_counts);
// replica exchange is on and some engine under `h` keeps its chains grouped by shape: BISBM_ERR_STATE with the message of the
// marginal histogram (a group engine knows no rungs), BISBM_OK otherwise; bisbm_marginals.hip
int refuse_rungs_over_groups(bisbm_engine* h);
// ---- the aligned-sample pipeline, for the pooled histogram and the mode-resolved ones alike; bisbm_align.hip ----
int overlap_mode(uint32_t T);  // which overlap-table placement serves tables of T cells: 0 per wave in LDS, 1 per workgroup, 2 HBM
// step 1: the overlap table tab[y] of every list position y < n_pos: the labels of chain list[y] with row ref_row[y] of `ref`
struct OverlapParams {
    const uint8_t* labels;     // [chain][label_stride]
    size_t label_stride;
    const uint8_t* ref;        // [rows][label_stride] (n used)
    const uint32_t* list;      // [position] chain
    const uint32_t* ref_row;   // [position] row of `ref`
    uint32_t n, na, ka, kb, nodes_per_block;  // (nodes_per_block: the launcher's)
    uint32_t* tab;             // [position][ka*ka + kb*kb], zeroed
};
hipError_t launch_overlap(const OverlapParams& p, uint32_t n_pos, hipStream_t stream);
// step 2: the assignment of `n_tables` overlap tables (tab[i][ka*ka + kb*kb]) into perm[i][ka + kb] and tot[i][2]
hipError_t launch_align_assign(const uint32_t* tab, uint32_t ka, uint32_t kb, uint8_t* perm, uint64_t* tot, uint32_t n_tables, hipStream_t stream);
// What one aligned sample counts: the chains of the handle sorted into `n_modes` histograms, each with its reference.
struct AlignPlan {
    uint32_t n_modes = 1;
    const uint32_t* of_chain = nullptr;  // [chains of the handle] mode of every chain, BISBM_MODE_NONE: not counted; NULL: all in mode 0
    const AlignRef* refs = nullptr;      // [n_modes]
    uint64_t list_serial = 0, ref_serial = 0;  // move with of_chain / with a reference
    uint32_t block_what = 0;    // block summaries (bisbm_block_sums.hip): what the sample also keeps, 0: nothing
    uint64_t block_serial = 0;  // BlockSumState::serial of the sums it adds to
    bool cold_only = false;  // the list is the identity and the counting kernel skips the chains off rung 0 (pooled plan under
                             // replica exchange; an anchored plan lists the cold chains itself)
};
// One aligned sample of the chains of kernel-running engine e (chains first .. of the handle) into counts[mode][n][kmax]: the
// three steps over e's list of counted chains.  plan.cold_only: the counting kernel takes list position y for chain y and
// counts it while it is on rung 0.
int aligned_sample(bisbm_engine* e, AlignScratch& s, const AlignPlan& plan, uint32_t first, uint32_t* counts);
// ---- block summaries; bisbm_block_sums.hip ----
// Before an aligned sample of the handle counts anything: mode_now[c] is the mode the sample counts chain c into
// (BISBM_MODE_NONE: none).  Sums of another shape or mode count start afresh, BISBM_ERR_STATE when a mode's terms would pass
// 2^32; the plan is told what to keep.  Nothing happens while the sums are off.
int block_sums_prepare(bisbm_engine* h, uint32_t ka, uint32_t kb, const std::vector<uint32_t>& mode_now, AlignPlan& plan);
// ... and after it succeeded: the terms and the last sample's assignment
void block_sums_commit(bisbm_engine* h, const std::vector<uint32_t>& mode_now, const AlignPlan& plan);
// the sums start afresh (with the histograms they accompany)
void block_sums_restart(bisbm_engine* h);
// the kernel of one aligned sample of engine e, on e's stream after the counting kernel: list positions [0, n_pos) of s
int block_sums_sample(bisbm_engine* e, AlignScratch& s, const AlignPlan& plan, uint32_t n_pos);
// BISBM_ERR_UNSUPPORTED while some leaf holds two-byte labels
int refuse_wide_labels(bisbm_engine* h, uint32_t ka, uint32_t kb);
// BISBM_ERR_INVALID_ARG unless every label of a caller's reference is a block of its node's type
int check_reference_labels(bisbm_engine* h, const uint32_t* labels, uint32_t ka, uint32_t kb);
// the library's reference: the labels of the chain of the lowest description length S[c] among those with counted(c) (ties ->
// the lowest chain; there is one)
template <class Pred>
int pick_reference(bisbm_engine* h, const std::vector<double>& S, Pred counted, uint32_t ka, uint32_t kb, AlignRef& r) {
    int64_t pick = -1;
    for (uint32_t c = 0; c < S.size(); ++c)
        if (counted(c) && (pick < 0 || S[c] < S[pick])) pick = c;
    std::vector<uint32_t> lab((size_t)h->n);
    if (int rc = bisbm_get_memberships(h, (uint32_t)pick, lab.data())) return rc;
    r.labels.swap(lab);
    r.has = true, r.chain = pick, r.ka = ka, r.kb = kb;
    return BISBM_OK;
}
// the permutation and the overlap total of list position y of the last sample of e
int read_alignment(bisbm_engine* h, bisbm_engine* e, const AlignScratch& s, uint32_t y, uint32_t* perm_out, uint64_t* overlap_out);
// mode-resolved marginals (include/bisbm.h); bisbm_mode_marginals.hip
int mode_accumulate(bisbm_engine* h, uint32_t* device_counts);  // bisbm_marginals_accumulate while modes are set
int mode_reset(bisbm_engine* h);                                // ... bisbm_marginals_reset
int mode_get_alignment(bisbm_engine* h, uint32_t chain, uint32_t* perm_out, uint64_t* overlap_out);  // ... bisbm_marginals_get_alignment
// VI[i][g] of chain chains[i] (index in kernel-running engine e) with row g of d_refs (n_refs byte rows of ref_stride bytes on
// e's device, of e's shape) into vi[chains.size() * n_refs]: the kernels and the arithmetic of bisbm_partition_distances_to, on
// e's stream with e's scratch; bisbm_partition.hip
int partition_distances_rows(bisbm_engine* e, const std::vector<uint32_t>& chains, const uint8_t* d_refs, size_t ref_stride, uint32_t n_refs, double* vi);
// BISBM_ERR_STATE with a message that names the per-mode call while modes are set, BISBM_OK otherwise
int refuse_while_modes(bisbm_engine* h, const char* call, const char* per_mode_call);

}  // namespace bisbm
