// bisbm.hpp -- C++ mirror of the reference's class API over the C ABI (include/bisbm.h).
//
// A caller written against the reference (src/mcmc_main.cc) keeps its shape: the same type aliases
// (types.hh:8-29), `blockmodel_t` with the constructor of blockmodel.hh:22-23, `metropolis_hasting`
// with `anneal` (metropolis_hasting.hh:48-53) taking one of the five `*_schedule` functions, the
// loaders of graph_utilities.hh and `output_vec` of output_functions.hh.  All chain state lives in
// the HIP library; this header only forwards.  Errors of the library are thrown as std::runtime_error
// (the reference is noexcept-and-terminate).
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bisbm.h"
#include "../../include/bisbm_io.h"

namespace bisbm_host {

using edge_t = std::pair<size_t, size_t>;  // types.hh:8-12
using edge_list_t = std::vector<edge_t>;
using uint_vec_t = std::vector<unsigned int>;
using int_vec_t = std::vector<int>;
using float_vec_t = std::vector<float>;
using int_mat_t = std::vector<std::vector<int>>;
using uint_mat_t = std::vector<std::vector<unsigned int>>;

// adj_list_t of the reference (vector<vector<size_t>>) in CSR form: row v = neighbours of v in edge-file order
struct adj_list_t {
    std::vector<uint64_t> rowptr;
    std::vector<uint32_t> col;
    size_t size() const { return rowptr.empty() ? 0 : rowptr.size() - 1; }
};

// ---- graph_utilities.hh:10-17 ----
inline bool load_edge_list(edge_list_t& edge_list, const std::string& path) {
    edge_list.clear();
    uint64_t *a = nullptr, *b = nullptr;
    const long n = bisbm_io_read_edge_list(path.c_str(), &a, &b);
    if (n < 0) return false;
    edge_list.reserve((size_t)n);
    for (long i = 0; i < n; ++i) edge_list.emplace_back((size_t)a[i], (size_t)b[i]);
    bisbm_io_free(a);
    bisbm_io_free(b);
    return true;
}

inline bool load_memberships(uint_vec_t& memberships, const std::string& path) {
    memberships.clear();
    uint32_t* p = nullptr;
    const long n = bisbm_io_read_memberships(path.c_str(), &p);
    if (n < 0) return false;
    memberships.assign(p, p + n);
    bisbm_io_free(p);
    return true;
}

// The clamp file of --clamp (include/bisbm_io.h): node ids separated by white space -> a mask of n bytes, 1 = listed.  On a
// failure `error` names the file, and the token where one is at fault.
inline bool load_clamp(std::vector<uint8_t>& mask, const std::string& path, size_t n, std::string& error) {
    uint8_t* p = nullptr;
    char msg[512];
    if (bisbm_io_read_clamp(path.c_str(), n, &p, msg, sizeof(msg)) < 0) {
        error = msg;
        return false;
    }
    mask.assign(p, p + n);
    bisbm_io_free(p);
    return true;
}

// The constraints file of --constraints (include/bisbm_io.h): one line per constrained node, its id and its allowed blocks ->
// the class of every node (n bytes) and the table of n_classes x (ka + kb) bytes for constrain().  On a failure `error` names the
// file, and the token where one is at fault.
inline bool load_constraints(uint32_t& n_classes, std::vector<uint8_t>& class_of_node, std::vector<uint8_t>& allowed, const std::string& path,
                             size_t n, size_t na, size_t ka, size_t kb, std::string& error) {
    uint8_t *pc = nullptr, *pa = nullptr;
    char msg[512];
    const long classes = bisbm_io_read_constraints(path.c_str(), n, na, (uint32_t)ka, (uint32_t)kb, &pc, &pa, msg, sizeof(msg));
    if (classes < 0) {
        error = msg;
        return false;
    }
    n_classes = (uint32_t)classes;
    class_of_node.assign(pc, pc + n);
    allowed.assign(pa, pa + (size_t)classes * (ka + kb));
    bisbm_io_free(pc);
    bisbm_io_free(pa);
    return true;
}

// The fields file of --fields (include/bisbm_io.h): one line per node with a prior, its id and block:weight pairs -> the field
// class of every node (n bytes) and the table of n_classes x (ka + kb) energies (-ln weight) for set_fields().  On a failure
// `error` names the file, and the token where one is at fault.
inline bool load_fields(uint32_t& n_classes, std::vector<uint8_t>& class_of_node, std::vector<double>& field, const std::string& path, size_t n,
                        size_t na, size_t ka, size_t kb, std::string& error) {
    uint8_t* pc = nullptr;
    double* pf = nullptr;
    char msg[512];
    const long classes = bisbm_io_read_fields(path.c_str(), n, na, (uint32_t)ka, (uint32_t)kb, &pc, &pf, msg, sizeof(msg));
    if (classes < 0) {
        error = msg;
        return false;
    }
    n_classes = (uint32_t)classes;
    class_of_node.assign(pc, pc + n);
    field.assign(pf, pf + (size_t)classes * (ka + kb));
    bisbm_io_free(pc);
    bisbm_io_free(pf);
    return true;
}

inline adj_list_t edge_to_adj(const edge_list_t& edge_list, size_t num_vertices = 0) {
    size_t n = num_vertices;
    for (auto const& e : edge_list) n = std::max(n, std::max(e.first, e.second) + 1);  // graph_utilities.cc:39-44
    std::vector<uint64_t> a(edge_list.size()), b(edge_list.size());
    for (size_t i = 0; i < edge_list.size(); ++i) {
        a[i] = edge_list[i].first;
        b[i] = edge_list[i].second;
    }
    adj_list_t adj;
    adj.rowptr.assign(n + 1, 0);
    adj.col.assign(2 * edge_list.size() + 1, 0);
    bisbm_io_edges_to_csr(a.data(), b.data(), a.size(), n, adj.rowptr.data(), adj.col.data());
    adj.col.resize(2 * edge_list.size());
    return adj;
}

// load_edge_list + edge_to_adj with the optional binary CSR cache of include/bisbm_io.h (num_vertices as in edge_to_adj)
inline bool load_adj_cached(adj_list_t& adj, const std::string& path, size_t num_vertices, bool use_cache, bool* hit = nullptr) {
    uint64_t* rp = nullptr;
    uint32_t* cl = nullptr;
    uint64_t ne = 0;
    int h = 0;
    if (bisbm_io_load_csr(path.c_str(), num_vertices, use_cache ? 1 : 0, &rp, &cl, &ne, &h) != 0) return false;
    adj.rowptr.assign(rp, rp + num_vertices + 1);
    adj.col.assign(cl, cl + 2 * ne);
    bisbm_io_free(rp);
    bisbm_io_free(cl);
    if (hit) *hit = h != 0;
    return true;
}

// Ingest-time renumbering for ids without structure (include/bisbm_io.h): new_id[v] = id of node v in the engine's graph
inline std::vector<uint32_t> locality_order(const adj_list_t& adj, size_t na) {
    std::vector<uint32_t> new_id(adj.size());
    if (bisbm_io_locality_order(adj.size(), na, adj.rowptr.data(), adj.col.data(), new_id.data()) != 0)
        throw std::runtime_error("locality_order: bad graph");
    return new_id;
}
inline adj_list_t permute_adj(const adj_list_t& adj, const std::vector<uint32_t>& new_id) {
    adj_list_t out;
    out.rowptr.assign(adj.rowptr.size(), 0);
    out.col.assign(adj.col.size() + 1, 0);
    if (bisbm_io_permute_csr(adj.size(), adj.rowptr.data(), adj.col.data(), new_id.data(), out.rowptr.data(), out.col.data()) != 0)
        throw std::runtime_error("permute_adj: bad permutation");
    out.col.resize(adj.col.size());
    return out;
}

// ---- output_functions.hh:20-29 ----
template <typename T>
void output_vec(const T& vec, std::ostream& stream = std::clog) {
    for (auto it = vec.begin(); it != vec.end(); ++it) stream << *it << " ";
    stream << "\n";
}

// ---- cooling schedules, metropolis_hasting.hh:13-21 / metropolis_hasting.cc:10-37 ----
// The functions exist so that `&exponential_schedule` etc. can be passed to anneal() as in the reference;
// the kernels evaluate the same expressions (pow/log ones from a host table built with these very calls).
inline double exponential_schedule(size_t t, float_vec_t kw) noexcept { return kw[0] * std::pow(kw[1], t); }
inline double linear_schedule(size_t t, float_vec_t kw) noexcept { return kw[0] - kw[1] * t; }
inline double logarithmic_schedule(size_t t, float_vec_t kw) noexcept {
    const float x = t + kw[1];
    const size_t i = (size_t)x;
    return kw[0] / (i == 0 ? 0. : std::log((double)i));
}
inline double constant_schedule(size_t, float_vec_t kw) noexcept { return kw[0]; }
inline double abrupt_cool_schedule(size_t t, float_vec_t kw) noexcept { return t < kw[0] ? 1. : 0.; }
using schedule_fn = double (*)(size_t, float_vec_t);

// The stage plan of the merge drivers, support/util.hh:99-145: the side with the larger drop goes down geometrically
// (floor(start / ratio^i) until <= end), the other side gets the same number of points with the ratio
// pow(start / end [integer division], 1 / (n - 1)).
inline std::pair<std::vector<int>, std::vector<int>> geospace(long start_a_in, long end_a_in, long start_b_in,
                                                              long end_b_in, double ratio) {
    if (ratio <= 1.) return {std::vector<int>{0}, std::vector<int>{0}};
    int start_a = (int)start_a_in, end_a = (int)end_a_in, start_b = (int)start_b_in, end_b = (int)end_b_in;
    const bool reverse = start_a - end_a < start_b - end_b;
    if (reverse) {
        std::swap(start_a, start_b);
        std::swap(end_a, end_b);
    }
    std::vector<int> ga, gb;
    int d = start_a;
    for (size_t i = 1; d > end_a; ++i) {
        ga.push_back(d);
        d = (int)std::floor(start_a / std::pow(ratio, (double)i));
    }
    ga.push_back(end_a);
    const size_t n = ga.size();
    const double r_ = std::pow((double)(start_b / end_b), 1. / (double)(n - 1));
    for (size_t idx = 0; idx + 1 < n; ++idx) gb.push_back((int)std::floor(start_b / std::pow(r_, (double)idx)));
    gb.push_back(end_b);
    return reverse ? std::make_pair(gb, ga) : std::make_pair(ga, gb);
}

struct engine_options {  // what the reference does not have: chains, device, RNG definition
    uint32_t n_chains = 1;
    uint32_t first_chain_id = 0;
    int device = 0;
    std::vector<int> devices;  // more than one entry: the chains are spread over these devices behind one handle (bisbm_create_multi)
    int rng_mode = BISBM_RNG_MT19937_COMPAT;
    uint64_t seed = 0;      // std::mt19937 engine(seed) of mcmc_main.cc:242, or the Philox key
    uint64_t gen_seed = 0;  // the hidden blockmodel_t::gen (blockmodel.hh:17-18); the reference seeds it from random_device
};

class blockmodel_t {
public:
    // blockmodel.hh:22-23; `g` is accepted and unused exactly like in the reference
    blockmodel_t(const uint_vec_t& memberships, uint_vec_t types, size_t /*g*/, size_t KA, size_t KB, double epsilon,
                 const adj_list_t* adj_list_ptr, const engine_options& opt = engine_options())
        : KA_(KA), KB_(KB), n_chains_(opt.n_chains) {
        size_t na = 0, nb = 0;
        for (auto t : types) (t == 0 ? na : nb) += 1;
        n_ = na + nb, na_ = na;
        const int rc = opt.devices.size() > 1
                           ? bisbm_create_multi(&h_, n_, na, nb, adj_list_ptr->rowptr.data(), adj_list_ptr->col.data(), (uint32_t)KA,
                                                (uint32_t)KB, epsilon, opt.n_chains, opt.first_chain_id, opt.devices.data(),
                                                (int)opt.devices.size(), opt.rng_mode, opt.seed, opt.gen_seed)
                           : bisbm_create(&h_, n_, na, nb, adj_list_ptr->rowptr.data(), adj_list_ptr->col.data(), (uint32_t)KA,
                                          (uint32_t)KB, epsilon, opt.n_chains, opt.first_chain_id,
                                          opt.devices.empty() ? opt.device : opt.devices[0], opt.rng_mode, opt.seed, opt.gen_seed);
        if (rc != BISBM_OK) throw std::runtime_error(std::string("bisbm_create: ") + bisbm_last_error(nullptr));
        check(bisbm_set_memberships(h_, BISBM_ALL_CHAINS, memberships.data()));
    }
    ~blockmodel_t() {
        if (h_) bisbm_destroy(h_);
    }
    blockmodel_t(const blockmodel_t&) = delete;
    blockmodel_t& operator=(const blockmodel_t&) = delete;

    void init_bisbm() { check(bisbm_init(h_)); }  // blockmodel.cc:682-688
    // blockmodel.cc:672-680; the engine lives in the library, the arguments keep the reference's signature
    void shuffle_bisbm(std::mt19937& /*engine*/, size_t /*NA*/, size_t /*NB*/) { check(bisbm_shuffle(h_)); }
    void shuffle_bisbm() { check(bisbm_shuffle(h_)); }

    const uint_vec_t* get_memberships(uint32_t chain = 0) {  // blockmodel.cc:87
        memberships_.resize(n_);
        check(bisbm_get_memberships(h_, chain, memberships_.data()));
        return &memberships_;
    }
    // blockmodel.cc:109-206 and :208-271 (call sites mcmc_main.cc:365,385,429,434,446); the engine lives in the
    // library.  Negative diffs (agg_split) throw: not provided, see include/bisbm.h.
    void agg_merge(std::mt19937& /*engine*/, int diff_a, int diff_b, int nm) { agg_merge(diff_a, diff_b, nm); }
    void agg_merge(std::mt19937& /*engine*/, int diff, int nm) { agg_merge(diff, nm); }
    void agg_merge(int diff_a, int diff_b, int nm) {
        check(bisbm_agg_merge(h_, diff_a, diff_b, nm));
        refresh_k();
    }
    void agg_merge(int diff, int nm) {
        check(bisbm_agg_merge_total(h_, diff, nm));
        refresh_k();
    }
    // block counts of one chain (the one-argument agg_merge lets every chain end with its own, blockmodel.cc:208-271)
    std::pair<size_t, size_t> ka_kb(uint32_t chain) const {
        uint32_t ka = 0, kb = 0;
        check(bisbm_get_ka_kb_chain(h_, chain, &ka, &kb));
        return {ka, kb};
    }
    size_t get_KA() const noexcept { return KA_; }
    size_t get_KB() const noexcept { return KB_; }
    int get_num_edges() const {
        uint64_t e = 0;
        bisbm_get_sizes(h_, nullptr, &e, nullptr, nullptr);
        return (int)e;
    }
    double get_entropy(uint32_t chain = 0) {  // blockmodel.cc:91
        std::vector<double> v(n_chains_);
        check(bisbm_get_cum_dS(h_, v.data()));
        return v[chain];
    }
    std::vector<double> entropy_all() {
        std::vector<double> v(n_chains_);
        check(bisbm_entropy(h_, v.data()));
        return v;
    }
    double entropy(uint32_t chain = 0) { return entropy_all()[chain]; }  // blockmodel.cc:753-787
    void summary(uint32_t chain = 0) {                                    // blockmodel.cc:748-751
        std::clog << "(Ka, Kb) = (" << KA_ << ", " << KB_ << ") \n";
        std::clog << "entropy: " << entropy(chain) << "\n";
    }
    // Marginal histogram over samples and chains (what README.md:49-53 describes for "marginalization" and the reference's
    // code never does): reset, add the present labels of every chain, read the MAP label of every node
    // (most frequent block, ties -> lowest index) in the reference's block numbering.
    void marginals_reset() { check(bisbm_marginals_reset(h_)); }
    void marginals_accumulate() { check(bisbm_marginals_accumulate(h_, nullptr)); }
    // label alignment before pooling (include/bisbm.h): on / off, and the chain the reference was taken from (-1: the caller's)
    void marginals_set_alignment(bool on) { check(bisbm_marginals_set_alignment(h_, on ? BISBM_ALIGN_REFERENCE : BISBM_ALIGN_NONE)); }
    std::vector<uint32_t> marginals_reference_labels() {
        std::vector<uint32_t> labels(n_);
        check(bisbm_marginals_get_reference(h_, labels.data(), nullptr));
        return labels;
    }
    int64_t marginals_reference_chain() {
        int64_t chain = -1;
        check(bisbm_marginals_get_reference(h_, nullptr, &chain));
        return chain;
    }
    // block summaries (include/bisbm.h): what every aligned sample also keeps (0: off), one mode's raw words (three planes
    // each: sum, sq_lo, sq_hi) with its terms, a counted chain's aligned tables of the last sample with its mode
    void block_sums_set(uint32_t what) { check(bisbm_block_sums_set(h_, what)); }
    uint64_t block_sums(uint32_t mode, std::vector<uint64_t>& e, std::vector<uint64_t>& n, std::vector<uint64_t>& d) {
        uint32_t ka = 0, kb = 0;
        check(bisbm_get_ka_kb(h_, &ka, &kb));
        e.assign((size_t)3 * ka * kb, 0), n.assign((size_t)3 * (ka + kb), 0), d.assign((size_t)3 * (ka + kb), 0);
        uint64_t terms = 0;
        check(bisbm_block_sums_get(h_, mode, &terms, e.data(), n.data(), d.data()));
        return terms;
    }
    uint32_t block_sums_last(uint32_t chain, std::vector<int32_t>& e, std::vector<int32_t>& n_r, std::vector<int32_t>& m_r) {
        uint32_t ka = 0, kb = 0, mode = 0;
        check(bisbm_get_ka_kb_chain(h_, chain, &ka, &kb));
        e.assign((size_t)ka * kb, 0), n_r.assign((size_t)ka + kb, 0), m_r.assign((size_t)ka + kb, 0);
        check(bisbm_block_sums_get_last(h_, chain, &mode, e.data(), n_r.data(), m_r.data()));
        return mode;
    }
    // replica exchange (include/bisbm.h): the ladder, sweeps with an exchange round every `every` sweeps, swaps per rung pair
    void tempering_set(const std::vector<float>& ladder) { check(bisbm_tempering_set(h_, (uint32_t)ladder.size(), ladder.data())); }
    void tempering_run(uint64_t sweeps, uint32_t every) { check(bisbm_tempering_run(h_, sweeps, every, nullptr)); }
    void tempering_stats(size_t L, std::vector<uint64_t>& attempted, std::vector<uint64_t>& accepted, uint64_t& rounds) {
        attempted.assign(L - 1, 0);
        accepted.assign(L - 1, 0);
        check(bisbm_tempering_stats(h_, attempted.data(), accepted.data(), &rounds));
    }
    // rounds of mixed moves under replica exchange (include/bisbm.h): per round the recipe's MH sweeps, heat-bath sweeps and pair
    // reshuffles of every chain at its rung's temperature, then one exchange; what each move did per rung (L rows of 6 counts)
    void tempering_rounds(uint64_t rounds, const bisbm_round_recipe& recipe, bool exchange = true) {
        check(bisbm_tempering_run_rounds(h_, rounds, &recipe, exchange ? 1 : 0));
    }
    std::vector<uint64_t> tempering_rung_stats(size_t L) {
        std::vector<uint64_t> out(6 * L);
        check(bisbm_tempering_rung_stats(h_, out.data()));
        return out;
    }
    // population annealing (include/bisbm.h): one resampling step (the parent of every slot, the step's log ratio); a run over
    // non-increasing temperatures (log ratio and distinct ancestors per step, acceptance rate per chain); the genealogy
    std::vector<uint32_t> population_resample(double beta_from, double beta_to, double& log_ratio) {
        std::vector<uint32_t> parent(n_chains_);
        check(bisbm_population_resample(h_, beta_from, beta_to, parent.data(), &log_ratio));
        return parent;
    }
    void population_run(const std::vector<float>& temps, uint64_t sweeps_per_step, std::vector<double>& log_ratio,
                        std::vector<uint32_t>& distinct, std::vector<double>& rates) {
        const size_t steps = temps.empty() ? 0 : temps.size() - 1;
        log_ratio.assign(steps, 0.);
        distinct.assign(steps, 0);
        rates.assign(n_chains_, 0.);
        check(bisbm_population_run(h_, (uint32_t)temps.size(), temps.data(), sweeps_per_step, log_ratio.data(), distinct.data(), rates.data()));
    }
    void population_rounds(const std::vector<float>& temps, uint64_t rounds_per_step, const bisbm_round_recipe& recipe, std::vector<double>& log_ratio,
                           std::vector<uint32_t>& distinct, std::vector<double>& rates) {
        const size_t steps = temps.empty() ? 0 : temps.size() - 1;
        log_ratio.assign(steps, 0.);
        distinct.assign(steps, 0);
        rates.assign(n_chains_, 0.);
        check(bisbm_rounds_population_run(h_, (uint32_t)temps.size(), temps.data(), rounds_per_step, &recipe, log_ratio.data(), distinct.data(), rates.data()));
    }
    std::vector<uint32_t> population_state(uint64_t& rounds, double& log_ratio_total) {
        std::vector<uint32_t> ancestor(n_chains_);
        check(bisbm_population_get(h_, ancestor.data(), &rounds, &log_ratio_total));
        return ancestor;
    }
    void population_reset() { check(bisbm_population_reset(h_)); }
    // heat-bath sweeps and greedy polishing (include/bisbm.h): `sweeps` sweeps in which every node draws its block from its
    // conditional ~ exp(-beta dS) (the moves per chain); greedy sweeps until a whole sweep moves nothing, at most max_sweeps
    // (moves and sweeps per chain)
    std::vector<uint64_t> heatbath_sweeps(uint64_t sweeps, double beta = 1.0) {
        std::vector<uint64_t> moved(n_chains_);
        check(bisbm_heatbath_run(h_, sweeps, beta, 0, moved.data(), nullptr));
        return moved;
    }
    void polish(uint64_t max_sweeps, std::vector<uint64_t>& moved, std::vector<uint64_t>& sweeps) {
        moved.assign(n_chains_, 0);
        sweeps.assign(n_chains_, 0);
        check(bisbm_heatbath_run(h_, max_sweeps, std::numeric_limits<double>::infinity(), 1, moved.data(), sweeps.data()));
    }
    // clamped nodes (include/bisbm.h): a non-zero byte of the mask (n bytes) holds the node at the label every chain has for it,
    // through every sampler; an empty or all-zero mask clears the clamp.  The mask in place and how many nodes it holds.
    void clamp(const std::vector<uint8_t>& mask) {
        if (!mask.empty() && mask.size() != n_) throw std::runtime_error("clamp: the mask has one byte per node");
        check(bisbm_clamp_set(h_, mask.empty() ? nullptr : mask.data()));
    }
    void unclamp() { check(bisbm_clamp_set(h_, nullptr)); }
    std::vector<uint8_t> clamped(uint64_t* n_clamped = nullptr) {
        std::vector<uint8_t> mask(n_);
        check(bisbm_clamp_get(h_, mask.data(), n_clamped));
        return mask;
    }
    // block constraints (include/bisbm.h): node v may sit in block s iff allowed[class_of_node[v] * (KA + KB) + s] is set (and s is
    // of v's type), through every sampler and in every chain; every chain's labels must satisfy them when they are set
    void constrain(uint32_t n_classes, const std::vector<uint8_t>& class_of_node, const std::vector<uint8_t>& allowed) {
        if (class_of_node.size() != n_) throw std::runtime_error("constrain: class_of_node has one byte per node");
        check(bisbm_constraints_set(h_, n_classes, class_of_node.data(), allowed.data()));
    }
    void unconstrain() { check(bisbm_constraints_set(h_, 0, nullptr, nullptr)); }
    uint32_t constraints(std::vector<uint8_t>& class_of_node, std::vector<uint8_t>& allowed) {
        uint32_t n_classes = 0;
        check(bisbm_constraints_get(h_, &n_classes, nullptr, nullptr));
        uint32_t ka = 0, kb = 0;
        check(bisbm_get_ka_kb(h_, &ka, &kb));
        class_of_node.assign(n_, 0);
        allowed.assign((size_t)n_classes * (ka + kb), 0);
        check(bisbm_constraints_get(h_, nullptr, class_of_node.data(), allowed.data()));
        return n_classes;
    }
    // block fields (include/bisbm.h): node v has the prior weight exp(-field[class_of_node[v] * (KA + KB) + s]) for block s of its
    // type, through every sampler and in every chain: the target is exp(-beta (S + Phi))
    void set_fields(uint32_t n_classes, const std::vector<uint8_t>& class_of_node, const std::vector<double>& field) {
        if (class_of_node.size() != n_) throw std::runtime_error("set_fields: class_of_node has one byte per node");
        check(bisbm_fields_set(h_, n_classes, class_of_node.data(), field.data()));
    }
    void clear_fields() { check(bisbm_fields_set(h_, 0, nullptr, nullptr)); }
    uint32_t fields(std::vector<uint8_t>& class_of_node, std::vector<double>& field) {
        uint32_t n_classes = 0;
        check(bisbm_fields_get(h_, &n_classes, nullptr, nullptr));
        uint32_t ka = 0, kb = 0;
        check(bisbm_get_ka_kb(h_, &ka, &kb));
        class_of_node.assign(n_, 0);
        field.assign((size_t)n_classes * (ka + kb), 0.);
        check(bisbm_fields_get(h_, nullptr, class_of_node.data(), field.data()));
        return n_classes;
    }
    std::vector<double> field_energy() {  // Phi per chain
        uint32_t chains = 0;
        check(bisbm_get_sizes(h_, nullptr, nullptr, nullptr, &chains));
        std::vector<double> out(chains);
        check(bisbm_fields_energy(h_, out.data()));
        return out;
    }
    // pair reshuffles (include/bisbm.h): `moves` moves per chain in which the nodes of two blocks of one type are divided afresh
    // and accepted or rejected as a whole (the accepted moves per chain); the record of every chain's last move.  The default
    // of 3 scans is a convention from the literature, not a measurement.
    std::vector<uint64_t> reshuffle(uint64_t moves, uint32_t scans = 3, double beta = 1.0) {
        std::vector<uint64_t> accepted(n_chains_);
        check(bisbm_reshuffle_run(h_, moves, scans, beta, accepted.data()));
        return accepted;
    }
    std::vector<bisbm_reshuffle_record> reshuffle_last() {
        std::vector<bisbm_reshuffle_record> rec(n_chains_);
        check(bisbm_reshuffle_get_last(h_, rec.data()));
        return rec;
    }
    // split and merge moves (include/bisbm.h): `moves` moves per chain in which one block is divided in two or two blocks of one
    // type are made one, accepted or rejected as a whole (the accepted moves per chain) -- the chains then differ in shape
    // (ka_kb(chain)) and everything indexed by block labels is reset by the caller, as after agg_merge; k_max {0, 0}: min(n_t, 127)
    std::vector<uint64_t> split_merge(uint64_t moves, uint32_t scans = 3, double beta = 1.0, std::array<uint32_t, 2> k_min = {1, 1},
                                      std::array<uint32_t, 2> k_max = {0, 0}) {
        std::vector<uint64_t> accepted(n_chains_);
        check(bisbm_split_merge_run(h_, moves, scans, beta, k_min.data(), k_max[0] || k_max[1] ? k_max.data() : nullptr, accepted.data()));
        refresh_k();
        return accepted;
    }
    std::vector<bisbm_split_merge_record> split_merge_last() {
        std::vector<bisbm_split_merge_record> rec(n_chains_);
        check(bisbm_split_merge_get_last(h_, rec.data()));
        return rec;
    }
    // ... per chain {splits proposed, splits accepted, merges proposed, merges accepted}
    std::vector<uint64_t> split_merge_total() {
        std::vector<uint64_t> out(4 * (size_t)n_chains_);
        check(bisbm_split_merge_get_total(h_, out.data()));
        return out;
    }
    // pair scores (include/bisbm.h): the pairs (u of type a, v of type b), a sample of every counted chain, the sums and the
    // number of chain terms in them (the estimate of a pair is sum / terms)
    void pair_scores_set(const std::vector<uint32_t>& u, const std::vector<uint32_t>& v) {
        if (u.size() != v.size()) throw std::runtime_error("pair_scores_set: u and v differ in length");
        check(bisbm_pair_scores_set(h_, u.size(), u.data(), v.data()));
        n_pairs_ = u.size();
    }
    void pair_scores_accumulate() { check(bisbm_pair_scores_accumulate(h_)); }
    void pair_scores_reset() { check(bisbm_pair_scores_reset(h_)); }
    std::vector<double> pair_scores(uint64_t& terms) {
        std::vector<double> sum(n_pairs_);
        check(bisbm_pair_scores_get(h_, sum.data(), &terms));
        return sum;
    }
    // edge probabilities (include/bisbm.h): the pairs with their kinds (BISBM_EDGE_ADD / BISBM_EDGE_REMOVE), a sample of every
    // counted chain, the sums of dS and exp(-dS), the present multiplicities and the number of chain terms in the sums
    void edge_probs_set(const std::vector<uint32_t>& u, const std::vector<uint32_t>& v, const std::vector<uint8_t>& kind, bool keep_last = false) {
        if (u.size() != v.size() || u.size() != kind.size()) throw std::runtime_error("edge_probs_set: u, v and kind differ in length");
        check(bisbm_edge_probs_set(h_, u.size(), u.data(), v.data(), kind.data(), keep_last ? BISBM_EDGE_KEEP_LAST : 0u));
        n_edge_pairs_ = u.size();
    }
    void edge_probs_accumulate() { check(bisbm_edge_probs_accumulate(h_)); }
    void edge_probs_reset() { check(bisbm_edge_probs_reset(h_)); }
    void edge_probs(std::vector<double>& dS_sum, std::vector<double>& w_sum, std::vector<uint32_t>& mult, uint64_t& terms) {
        dS_sum.assign(n_edge_pairs_, 0.), w_sum.assign(n_edge_pairs_, 0.), mult.assign(n_edge_pairs_, 0u);
        check(bisbm_edge_probs_get(h_, dS_sum.data(), w_sum.data(), mult.data(), &terms));
    }
    // query scores (include/bisbm.h): the query nodes (either type), a sample of every counted chain, one query's row over its
    // candidates (all nodes of the other type, in id order), and every query's k best candidates selected on the device
    // (nodes / sums [queries * k], 0xffffffff / 0.0 past the eligible ones; the estimate of an entry is sum / terms)
    void query_scores_set(const std::vector<uint32_t>& queries) {
        check(bisbm_query_scores_set(h_, (uint32_t)queries.size(), queries.data()));
        queries_ = queries;
    }
    void query_scores_accumulate() { check(bisbm_query_scores_accumulate(h_)); }
    void query_scores_reset() { check(bisbm_query_scores_reset(h_)); }
    std::vector<double> query_scores_row(uint32_t query_index, uint64_t& terms) {
        if (query_index >= queries_.size()) throw std::runtime_error("query_scores_row: no such query");
        std::vector<double> sum(queries_[query_index] < na_ ? n_ - na_ : na_);
        check(bisbm_query_scores_get_row(h_, query_index, sum.data(), &terms));
        return sum;
    }
    void query_scores_topk(uint32_t k, bool exclude_neighbours, std::vector<uint32_t>& nodes, std::vector<double>& sums, uint64_t& terms) {
        nodes.assign(queries_.size() * (size_t)k, 0);
        sums.assign(queries_.size() * (size_t)k, 0.);
        check(bisbm_query_scores_topk(h_, k, exclude_neighbours ? 1 : 0, nodes.data(), sums.data(), &terms));
    }
    // edge queries (include/bisbm.h): the query nodes (either type), a sample of every counted chain, one query's row of
    // w_sum = sum of exp(-dS) over its candidates with their present multiplicities, and every query's k best candidates selected
    // on the device (nodes / w_sums [queries * k], 0xffffffff / 0.0 past the eligible ones; the log odds of an entry are
    // ln(w_sum / terms))
    void edge_queries_set(const std::vector<uint32_t>& queries) {
        check(bisbm_edge_queries_set(h_, (uint32_t)queries.size(), queries.data()));
        edge_queries_ = queries;
    }
    void edge_queries_accumulate() { check(bisbm_edge_queries_accumulate(h_)); }
    void edge_queries_reset() { check(bisbm_edge_queries_reset(h_)); }
    void edge_queries_row(uint32_t query_index, std::vector<double>& w_sum, std::vector<uint32_t>& mult, uint64_t& terms) {
        if (query_index >= edge_queries_.size()) throw std::runtime_error("edge_queries_row: no such query");
        const size_t len = edge_queries_[query_index] < na_ ? n_ - na_ : na_;
        w_sum.assign(len, 0.), mult.assign(len, 0u);
        check(bisbm_edge_queries_get_row(h_, query_index, w_sum.data(), mult.data(), &terms));
    }
    void edge_queries_topk(uint32_t k, bool exclude_neighbours, std::vector<uint32_t>& nodes, std::vector<double>& w_sums, uint64_t& terms) {
        nodes.assign(edge_queries_.size() * (size_t)k, 0);
        w_sums.assign(edge_queries_.size() * (size_t)k, 0.);
        check(bisbm_edge_queries_topk(h_, k, exclude_neighbours ? 1 : 0, nodes.data(), w_sums.data(), &terms));
    }
    // co-assignment (include/bisbm.h): the query nodes (either type), a sample of every counted chain, one query's row over the
    // nodes of its own type in id order, and every query's k most often co-assigned nodes selected on the device (nodes / counts
    // [queries * k], 0xffffffff / 0 past the eligible ones; the estimate of an entry is count / terms)
    void coassign_set(const std::vector<uint32_t>& queries) {
        check(bisbm_coassign_set(h_, (uint32_t)queries.size(), queries.data()));
        coassign_queries_ = queries;
    }
    void coassign_accumulate() { check(bisbm_coassign_accumulate(h_)); }
    void coassign_reset() { check(bisbm_coassign_reset(h_)); }
    std::vector<uint32_t> coassign_row(uint32_t query_index, uint64_t& terms) {
        if (query_index >= coassign_queries_.size()) throw std::runtime_error("coassign_row: no such query");
        std::vector<uint32_t> count(coassign_queries_[query_index] < na_ ? na_ : n_ - na_);
        check(bisbm_coassign_get_row(h_, query_index, count.data(), &terms));
        return count;
    }
    void coassign_topk(uint32_t k, std::vector<uint32_t>& nodes, std::vector<uint32_t>& counts, uint64_t& terms) {
        nodes.assign(coassign_queries_.size() * (size_t)k, 0);
        counts.assign(coassign_queries_.size() * (size_t)k, 0);
        check(bisbm_coassign_topk(h_, k, nodes.data(), counts.data(), &terms));
    }
    // fold-in queries (include/bisbm.h): virtual nodes given by a type (0: a, 1: b) and a list of neighbours of the other type; a
    // sample of every counted chain; one node's block posterior per chain at the last sample ([n_chains * stride]); one node's
    // row of kind `what` (BISBM_FOLDIN_RECOMMEND: over the other type's nodes, BISBM_FOLDIN_SIMILAR: over its own type's); every
    // node's k best candidates of one kind selected on the device (the estimate of an entry is sum / terms)
    void foldin_set(const std::vector<uint8_t>& types, const std::vector<std::vector<uint32_t>>& lists, double alpha,
                    uint32_t what = BISBM_FOLDIN_RECOMMEND | BISBM_FOLDIN_SIMILAR) {
        if (types.size() != lists.size()) throw std::runtime_error("foldin_set: one list per virtual node");
        std::vector<uint64_t> ptr(1, 0);
        std::vector<uint32_t> flat;
        for (auto const& l : lists) {
            flat.insert(flat.end(), l.begin(), l.end());
            ptr.push_back(flat.size());
        }
        check(bisbm_foldin_set(h_, (uint32_t)types.size(), types.data(), ptr.data(), flat.data(), alpha, what));
        foldin_types_ = types;
    }
    void foldin_accumulate() { check(bisbm_foldin_accumulate(h_)); }
    void foldin_reset() { check(bisbm_foldin_reset(h_)); }
    std::vector<double> foldin_posteriors(uint32_t query_index, uint32_t stride) {
        std::vector<double> p((size_t)n_chains_ * stride);
        check(bisbm_foldin_get_posteriors(h_, query_index, stride, p.data()));
        return p;
    }
    std::vector<double> foldin_row(uint32_t what, uint32_t query_index, uint64_t& terms) {
        if (query_index >= foldin_types_.size()) throw std::runtime_error("foldin_row: no such virtual node");
        const bool cand_b = what == BISBM_FOLDIN_RECOMMEND ? foldin_types_[query_index] == 0 : foldin_types_[query_index] != 0;
        std::vector<double> sum(cand_b ? n_ - na_ : na_);
        check(bisbm_foldin_get_row(h_, what, query_index, sum.data(), &terms));
        return sum;
    }
    void foldin_topk(uint32_t what, uint32_t k, bool exclude_listed, std::vector<uint32_t>& nodes, std::vector<double>& sums, uint64_t& terms) {
        nodes.assign(foldin_types_.size() * (size_t)k, 0);
        sums.assign(foldin_types_.size() * (size_t)k, 0.);
        check(bisbm_foldin_topk(h_, what, k, exclude_listed ? 1 : 0, nodes.data(), sums.data(), &terms));
    }
    // node conditionals (include/bisbm.h, "Node conditionals"): the queries (existing nodes of either type; empty + all = true:
    // every node), beta and whether the last sample's rows are kept; the caller's reference of the soft marginals (empty:
    // cleared); one sample of every counted chain; the pooled label-free sums; the soft marginals ([n_queries * kmax]); one
    // query's dS and P rows per chain at the last sample ([n_chains * stride] each)
    void conditionals_set(const std::vector<uint32_t>& nodes, double beta = 1.0, bool keep_last = false, bool all = false) {
        const uint32_t nq = all ? (uint32_t)n_ : (uint32_t)nodes.size();
        check(bisbm_conditionals_set(h_, nq, all ? nullptr : nodes.data(), beta, keep_last ? BISBM_COND_KEEP_LAST : 0u));
        n_conditionals_ = nq;
    }
    void conditionals_set_reference(const std::vector<uint32_t>& labels) {
        if (!labels.empty() && labels.size() != n_) throw std::runtime_error("conditionals_set_reference: n labels");
        check(bisbm_conditionals_set_reference(h_, labels.empty() ? nullptr : labels.data()));
    }
    void conditionals_accumulate() { check(bisbm_conditionals_accumulate(h_)); }
    void conditionals_reset() { check(bisbm_conditionals_reset(h_)); }
    struct conditional_stats_t {
        std::vector<double> stay, entropy, margin;
        std::vector<uint64_t> free;
        uint64_t terms = 0;
    };
    conditional_stats_t conditionals_stats() {
        conditional_stats_t s;
        s.stay.assign(n_conditionals_, 0.), s.entropy.assign(n_conditionals_, 0.), s.margin.assign(n_conditionals_, 0.);
        s.free.assign(n_conditionals_, 0);
        check(bisbm_conditionals_get_stats(h_, s.stay.data(), s.entropy.data(), s.margin.data(), s.free.data(), &s.terms));
        return s;
    }
    std::vector<double> conditionals_marginals(uint32_t& kmax, uint64_t& terms) {
        check(bisbm_conditionals_get_marginals(h_, nullptr, &kmax, &terms));
        std::vector<double> prob((size_t)n_conditionals_ * kmax);
        check(bisbm_conditionals_get_marginals(h_, prob.data(), &kmax, &terms));
        return prob;
    }
    void conditionals_last(uint32_t query_index, uint32_t stride, std::vector<double>& dS, std::vector<double>& p) {
        dS.assign((size_t)n_chains_ * stride, 0.), p.assign((size_t)n_chains_ * stride, 0.);
        check(bisbm_conditionals_get_last(h_, query_index, stride, dS.data(), p.data()));
    }
    // held conditionals and the least settled queries (include/bisbm.h, "Held conditionals", "Least settled"): the switch between
    // the held row (the heat-bath kernel's, under the handle's clamp, constraints and fields) and the model's row; the k queries
    // with the largest entropy sum (BISBM_SETTLED_BY_ENTROPY) or the smallest stay sum (BISBM_SETTLED_BY_STAY), as query indices
    void conditionals_held(bool on = true) { check(bisbm_held_conditionals_set(h_, on ? 1 : 0)); }
    bool conditionals_is_held() {
        int on = 0;
        check(bisbm_held_conditionals_get(h_, &on));
        return on != 0;
    }
    void least_settled(uint32_t by, uint32_t k, std::vector<uint32_t>& queries, std::vector<double>& values, uint64_t& terms) {
        queries.assign(k, 0), values.assign(k, 0.);
        check(bisbm_least_settled_topk(h_, by, k, queries.data(), values.data(), &terms));
    }
    // rung of every chain under replica exchange (bisbm_tempering_get)
    std::vector<uint32_t> tempering_rungs() {
        std::vector<uint32_t> rung(n_chains_);
        check(bisbm_tempering_get(h_, rung.data(), nullptr));
        return rung;
    }
    // partition distances and modes (include/bisbm.h): the VI matrix of the listed chains (row-major, in their order), and its
    // grouping by single linkage at `threshold` -- mode per listed chain, medoid per mode (positions in the list)
    std::vector<double> partition_distances(const std::vector<uint32_t>& chains) {
        std::vector<double> vi(chains.size() * chains.size());
        check(bisbm_partition_distances(h_, (uint32_t)chains.size(), chains.data(), vi.data(), nullptr));
        return vi;
    }
    // chains against reference partitions that are no chains (bisbm_partition_distances_to): refs holds n labels per reference,
    // shapes (ka, kb) per reference; returns vi[chains][references], H of the references into h_ref when given
    std::vector<double> partition_distances_to(const std::vector<uint32_t>& chains, const std::vector<uint32_t>& refs,
                                               const std::vector<uint32_t>& ref_ka, const std::vector<uint32_t>& ref_kb,
                                               std::vector<double>* h_ref = nullptr) {
        if (ref_ka.size() != ref_kb.size() || refs.size() != ref_ka.size() * n_)
            throw std::runtime_error("partition_distances_to: n labels and one (ka, kb) per reference");
        std::vector<double> vi(chains.size() * ref_ka.size());
        if (h_ref) h_ref->assign(ref_ka.size(), 0.);
        check(bisbm_partition_distances_to(h_, (uint32_t)chains.size(), chains.data(), (uint32_t)ref_ka.size(), refs.data(), ref_ka.data(),
                                           ref_kb.data(), vi.data(), h_ref ? h_ref->data() : nullptr));
        return vi;
    }
    // chain traces (include/bisbm.h): the ring, one record, the lag sums and a series ([records][chains]); summary on the host
    void trace_set(uint32_t depth) { check(bisbm_trace_set(h_, depth)); }
    void trace_reset() { check(bisbm_trace_reset(h_)); }
    void trace_record() { check(bisbm_trace_record(h_)); }
    uint64_t trace_lags(uint32_t depth, std::vector<double>& vi_sum, std::vector<uint64_t>& agree_sum, std::vector<uint64_t>& pairs) {
        vi_sum.assign((size_t)n_chains_ * depth, 0.), agree_sum.assign((size_t)n_chains_ * depth, 0), pairs.assign(depth, 0);
        uint64_t records = 0;
        check(bisbm_trace_get_lags(h_, vi_sum.data(), agree_sum.data(), nullptr, pairs.data(), &records));
        return records;
    }
    std::vector<double> trace_series(int what, uint64_t records) {
        std::vector<double> x((size_t)records * n_chains_);
        check(bisbm_trace_get_series(h_, what, x.data()));
        return x;
    }
    static void trace_summary(const std::vector<double>& x, uint64_t T, uint32_t C, double window, std::vector<double>& tau,
                              std::vector<uint32_t>& win, double& rhat) {
        tau.assign(C, 0.), win.assign(C, 0);
        if (bisbm_trace_summary(T, C, x.data(), window, tau.data(), win.data(), &rhat) != BISBM_OK)
            throw std::runtime_error(std::string("bisbm: ") + bisbm_last_error(nullptr));
    }
    static void partition_modes(const std::vector<double>& vi, size_t m, double threshold, std::vector<uint32_t>& mode,
                                std::vector<uint32_t>& medoids) {
        mode.assign(m, 0);
        medoids.assign(m, 0);
        uint32_t n_modes = 0;
        if (bisbm_partition_modes((uint32_t)m, vi.data(), threshold, mode.data(), medoids.data(), &n_modes) != BISBM_OK)
            throw std::runtime_error(std::string("bisbm: ") + bisbm_last_error(nullptr));
        medoids.resize(n_modes);
    }
    // mode-resolved marginals (include/bisbm.h): the chains' modes (BISBM_MODE_NONE: not counted; an empty vector turns the
    // feature off), what the samples made of them, a caller's reference of a mode, a mode's histogram and its MAP labels with
    // every node's winning count
    void marginals_set_modes(uint32_t n_modes, const std::vector<uint32_t>& mode_of_chain) {
        if (n_modes && mode_of_chain.size() != n_chains_) throw std::runtime_error("marginals_set_modes: one mode per chain");
        check(bisbm_marginals_set_modes(h_, n_modes, n_modes ? mode_of_chain.data() : nullptr));
    }
    uint32_t marginals_modes(std::vector<uint32_t>& mode_of_chain, std::vector<int64_t>& ref_chain, std::vector<uint64_t>& terms) {
        uint32_t n_modes = 0;
        check(bisbm_marginals_get_modes(h_, &n_modes, nullptr, nullptr, nullptr));
        mode_of_chain.assign(n_chains_, BISBM_MODE_NONE);
        ref_chain.assign(n_modes, -2);
        terms.assign(n_modes, 0);
        check(bisbm_marginals_get_modes(h_, &n_modes, mode_of_chain.data(), ref_chain.data(), terms.data()));
        return n_modes;
    }
    // anchored modes (include/bisbm.h): n labels per anchor, n_modes anchors; every sample counts each chain into the mode of
    // its nearest anchor within the threshold.  marginals_mode_assignment: visits[chain][mode], unassigned, samples
    void marginals_set_mode_anchors(uint32_t n_modes, const std::vector<uint32_t>& anchors, double threshold) {
        if (anchors.size() != (size_t)n_modes * n_) throw std::runtime_error("marginals_set_mode_anchors: n labels per anchor");
        check(bisbm_marginals_set_mode_anchors(h_, n_modes, n_modes ? anchors.data() : nullptr, threshold));
    }
    void marginals_mode_assignment(uint32_t n_modes, std::vector<uint64_t>& visits, uint64_t& unassigned, uint64_t& samples,
                                   std::vector<double>* vi = nullptr) {
        visits.assign((size_t)n_chains_ * n_modes, 0);
        if (vi) vi->assign((size_t)n_chains_ * n_modes, 0.);
        check(bisbm_marginals_get_mode_assignment(h_, vi ? vi->data() : nullptr, visits.data(), &unassigned, &samples));
    }
    void marginals_set_mode_reference(uint32_t mode, const std::vector<uint32_t>* labels) {
        if (labels && labels->size() != n_) throw std::runtime_error("marginals_set_mode_reference: one label per node");
        check(bisbm_marginals_set_mode_reference(h_, mode, labels ? labels->data() : nullptr));
    }
    std::vector<uint32_t> marginals_get_mode(uint32_t mode) {
        uint32_t ka = 0, kb = 0;
        check(bisbm_get_ka_kb(h_, &ka, &kb));
        std::vector<uint32_t> counts(n_ * std::max(ka, kb));
        check(bisbm_marginals_get_mode(h_, mode, counts.data()));
        return counts;
    }
    std::vector<uint32_t> marginals_map_mode(uint32_t mode, std::vector<uint32_t>* top = nullptr) {
        std::vector<uint32_t> lab(n_);
        if (top) top->assign(n_, 0);
        check(bisbm_marginals_map_mode(h_, mode, lab.data(), top ? top->data() : nullptr));
        return lab;
    }
    // the marginal estimate of README.md:49-53: every node's most frequent block, pooled over the handle's devices on the
    // devices (bisbm_marginals_map)
    uint_vec_t marginal_map_labels(size_t /*NA*/) {
        std::vector<uint32_t> lab(n_);
        check(bisbm_marginals_map(h_, lab.data()));
        return uint_vec_t(lab.begin(), lab.end());
    }
    // {eta_in_lds, eta_w, eta_lo_a, eta_lo_b} of the last MH launch (include/bisbm.h, bisbm_last_eta_plan)
    std::array<uint32_t, 4> last_eta_plan() const {
        std::array<uint32_t, 4> out{};
        check(bisbm_last_eta_plan(h_, out.data()));
        return out;
    }
    // BISBM_ROUTE_* bits of the last MH launch: which kernel ran, and whether it carried a hold or fields (bisbm_last_sweep_route)
    uint32_t last_route() const {
        uint32_t route = 0;
        check(bisbm_last_sweep_route(h_, &route));
        return route;
    }
    bisbm_handle handle() const { return h_; }
    uint32_t n_chains() const { return n_chains_; }

private:
    void check(int rc) const {
        if (rc != BISBM_OK) throw std::runtime_error(std::string("bisbm: ") + bisbm_last_error(h_));
    }
    void refresh_k() {
        uint32_t ka = 0, kb = 0;
        check(bisbm_get_ka_kb_chain(h_, 0, &ka, &kb));  // (chain 0's: after agg_merge(diff, nm) chains may differ, see ka_kb())
        KA_ = ka;
        KB_ = kb;
    }
    bisbm_handle h_ = nullptr;
    size_t KA_, KB_, n_ = 0, na_ = 0, n_pairs_ = 0, n_edge_pairs_ = 0;
    std::vector<uint32_t> queries_, edge_queries_, coassign_queries_;
    std::vector<uint8_t> foldin_types_;
    uint32_t n_conditionals_ = 0;
    uint32_t n_chains_;
    uint_vec_t memberships_;
};

class metropolis_hasting {
public:
    // metropolis_hasting.hh:48-53.  Returns the acceptance rate of chain 0; rates() has all chains.
    double anneal(blockmodel_t& blockmodel, schedule_fn cooling_schedule, const float_vec_t& kwargs, size_t duration,
                  size_t steps_await, std::mt19937& /*engine*/) {
        return anneal(blockmodel, cooling_schedule, kwargs, duration, steps_await);
    }
    double anneal(blockmodel_t& blockmodel, schedule_fn cooling_schedule, const float_vec_t& kwargs, size_t duration,
                  size_t steps_await) {
        int id;
        if (cooling_schedule == &exponential_schedule)
            id = BISBM_SCHED_EXPONENTIAL;
        else if (cooling_schedule == &linear_schedule)
            id = BISBM_SCHED_LINEAR;
        else if (cooling_schedule == &logarithmic_schedule)
            id = BISBM_SCHED_LOGARITHMIC;
        else if (cooling_schedule == &constant_schedule)
            id = BISBM_SCHED_CONSTANT;
        else if (cooling_schedule == &abrupt_cool_schedule)
            id = BISBM_SCHED_ABRUPT_COOL;
        else
            throw std::runtime_error("anneal: pass one of the five *_schedule functions");
        float kw[2] = {kwargs.size() > 0 ? kwargs[0] : 0.f, kwargs.size() > 1 ? kwargs[1] : 0.f};
        rates_.assign(blockmodel.n_chains(), 0.);
        const int rc = bisbm_anneal(blockmodel.handle(), id, kw, duration, steps_await, rates_.data());
        if (rc != BISBM_OK) throw std::runtime_error(std::string("bisbm_anneal: ") + bisbm_last_error(blockmodel.handle()));
        return rates_[0];
    }
    const std::vector<double>& rates() const { return rates_; }

private:
    std::vector<double> rates_;
};

}  // namespace bisbm_host
