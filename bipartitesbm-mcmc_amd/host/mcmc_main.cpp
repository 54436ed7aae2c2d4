// mcmc_main.cpp -- the reference's command line (src/mcmc_main.cc) re-hosted on the HIP engine.
//
// Same flags (mcmc_main.cc:55-93), same validation messages and exit codes (:99-239), same initial
// partition rules (:241-326), same stdout contract: the label vector through output_vec (trailing blank,
// newline), "acceptance ratio" and summary() on clog (:483-485).  Boost.program_options is replaced by a
// small parser with the same surface (long/short names, `--opt=value`, multitoken options).
// Extra flags: --chains, --device, --devices, --rng {mt19937-compat,philox}, --gen_seed, --csr_cache, --reorder, --marginalize, --align,
// --tempering, --exchange_every, --population, --population_sweeps, --score_pairs, --edge_probs, --recommend, --recommend_edges, --include_edges, --modes, --mode_marginals, --reassign, --similar, --foldin, --foldin_alpha,
// --conditionals, --conditionals_beta, --polish, --heatbath, --reshuffle, --reshuffle_scans, --trace, --rung_moves, --population_moves,
// --clamp, --constraints, --fields, --split_merge, --split_merge_scans, --k_min, --k_max, --shape_counts.
// The agglomerative drivers (:349-451) run through bisbm_agg_merge.  --merge starts at one block per node: while
// KA + KB > 256 the library runs its wide mode (two-byte labels, generic kernel), up to about 14 000 blocks (bisbm_check_shape).
// Negative diffs (agg_split) run through the same call (blockmodel.cc:110-117).
#include <algorithm>
#include <chrono>
#include <limits>
#include <cmath>
#include <numeric>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <atomic>
#include <vector>

#include "bisbm.hpp"

using namespace bisbm_host;

namespace {

struct option_spec {
    const char* long_name;
    char short_name;  // 0 = none
    int kind;         // 0 = flag, 1 = single value, 2 = multitoken
};

const option_spec kOptions[] = {
    {"edge_list_path", 'e', 1}, {"membership_path", 0, 1}, {"mb", 0, 2},          {"n", 'n', 2},
    {"types", 'y', 2},          {"burn_in", 'b', 1},       {"sampling_steps", 't', 1},
    {"sampling_frequency", 'f', 1}, {"bisbm_partition", 'z', 2}, {"uni", 0, 0},
    {"cooling_schedule", 'c', 1}, {"cooling_schedule_kwargs", 'a', 2}, {"steps_await", 'x', 1},
    {"epsilon", 'E', 1},        {"randomize", 'r', 0},     {"merge", 'g', 0},      {"nature", 'u', 0},
    {"seed", 'd', 1},           {"help", 'h', 0},
    // engine extras
    {"chains", 0, 1},           {"device", 0, 1},          {"devices", 0, 1},          {"rng", 0, 1},          {"gen_seed", 0, 1},
    {"csr_cache", 0, 0},        {"reorder", 0, 0},         {"marginalize", 0, 0},      {"align", 0, 0},
    {"tempering", 0, 2},        {"exchange_every", 0, 1},  {"score_pairs", 0, 2},
    {"edge_probs", 0, 2},
    {"population", 0, 2},       {"population_sweeps", 0, 1},
    {"recommend", 0, 2},        {"include_edges", 0, 0},
    {"recommend_edges", 0, 2},
    {"similar", 0, 2},
    {"foldin", 0, 2},           {"foldin_alpha", 0, 1},
    {"conditionals", 0, 2},     {"conditionals_beta", 0, 1},
    {"conditionals_held", 0, 0}, {"least_settled", 0, 2},
    {"modes", 0, 2},            {"mode_marginals", 0, 1},  {"reassign", 0, 0},
    {"polish", 0, 1},           {"heatbath", 0, 0},
    {"reshuffle", 0, 1},        {"reshuffle_scans", 0, 1},
    {"split_merge", 0, 1},      {"split_merge_scans", 0, 1}, {"k_min", 0, 2},       {"k_max", 0, 2},       {"shape_counts", 0, 1},
    {"trace", 0, 2},            {"block_summary", 0, 1},
    {"rung_moves", 0, 2},       {"population_moves", 0, 2},
    {"clamp", 0, 1},            {"constraints", 0, 1},
    {"fields", 0, 1},
};

// a / b of two integers (b > 0) as the nearest double, ties to even: a quotient of 55 or 56 bits with the remainder folded
// into its lowest bit rounds once, in the conversion
double exact_quotient(unsigned __int128 a, unsigned __int128 b) {
    if (a == 0) return 0.;
    auto bits = [](unsigned __int128 x) {
        int n = 0;
        for (; x; x >>= 1) ++n;
        return n;
    };
    const int shift = 55 - (bits(a) - bits(b));
    if (shift >= 0)
        a <<= shift;
    else
        b <<= -shift;
    const unsigned __int128 q = a / b;
    const uint64_t folded = (uint64_t)q | (a % b ? 1u : 0u);
    return std::ldexp((double)folded, -shift);
}
// the moments of a block-summary cell (include/bisbm.h, "Block summaries") from its three words: sum / terms, and
// (sum of squares * terms - sum^2) / terms^2 in integers with one division at the end; NaN without terms
double block_mean(uint64_t sum, uint64_t terms) { return terms ? exact_quotient(sum, terms) : std::nan(""); }
double block_variance(uint64_t sum, uint64_t sq_lo, uint64_t sq_hi, uint64_t terms) {
    if (!terms) return std::nan("");
    const unsigned __int128 s2 = ((unsigned __int128)sq_hi << 32) + sq_lo;
    return exact_quotient(s2 * terms - (unsigned __int128)sum * sum, (unsigned __int128)terms * terms);
}

const option_spec* find_long(const std::string& name) {
    for (auto const& o : kOptions)
        if (name == o.long_name) return &o;
    return nullptr;
}
const option_spec* find_short(char c) {
    for (auto const& o : kOptions)
        if (o.short_name && o.short_name == c) return &o;
    return nullptr;
}
bool looks_like_option(const char* s) {
    if (s[0] != '-' || s[1] == '\0') return false;
    if (s[1] == '-') return true;
    return !(s[1] >= '0' && s[1] <= '9') && s[1] != '.';  // "-3" / "-.5" are values
}

using var_map_t = std::map<std::string, std::vector<std::string>>;

bool parse_command_line(int argc, char const* argv[], var_map_t& vm, std::string& err) {
    for (int i = 1; i < argc; ++i) {
        std::string tok = argv[i];
        const option_spec* spec = nullptr;
        std::string inline_value;
        bool has_inline = false;
        if (tok.rfind("--", 0) == 0) {
            const size_t eq = tok.find('=');
            const std::string name = tok.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            spec = find_long(name);
            if (!spec) {
                err = "unrecognised option '" + tok + "'";
                return false;
            }
            if (eq != std::string::npos) {
                inline_value = tok.substr(eq + 1);
                has_inline = true;
            }
        } else if (tok.size() >= 2 && tok[0] == '-') {
            spec = find_short(tok[1]);
            if (!spec) {
                err = "unrecognised option '" + tok + "'";
                return false;
            }
            if (tok.size() > 2) {
                inline_value = tok.substr(2);
                has_inline = true;
            }
        } else {
            err = "too many positional options have been specified on the command line";
            return false;
        }
        auto& values = vm[spec->long_name];
        if (spec->kind == 0) {
            values.push_back("");
            continue;
        }
        if (has_inline) values.push_back(inline_value);
        if (spec->kind == 1) {
            if (!has_inline) {
                if (i + 1 >= argc) {
                    err = std::string("the required argument for option '--") + spec->long_name + "' is missing";
                    return false;
                }
                values.push_back(argv[++i]);
            }
        } else {
            while (i + 1 < argc && !looks_like_option(argv[i + 1])) values.push_back(argv[++i]);
            if (values.empty()) {
                err = std::string("the required argument for option '--") + spec->long_name + "' is missing";
                return false;
            }
        }
    }
    return true;
}

uint_vec_t to_uints(const std::vector<std::string>& v) {
    uint_vec_t out;
    for (auto const& s : v) out.push_back((unsigned)std::strtoul(s.c_str(), nullptr, 10));
    return out;
}

void print_help(const char* argv0) {
    std::clog << "MCMC algorithms for the bipartiteSBM (final output only)\n";
    std::clog << "Usage:\n  " << argv0 << " [--option_1=value] [--option_s2=value] ...\n";
    std::clog << "Options:\n"
                 "  -e [ --edge_list_path ] arg           Path to edge list file.\n"
                 "  --membership_path arg                 Path to membership file.\n"
                 "  --mb arg                              Memberships given on the command line.\n"
                 "  -n [ --n ] arg                        Block sizes vector.\n"
                 "  -y [ --types ] arg                    Block types vector (NA NB).\n"
                 "  -b [ --burn_in ] arg (=1000)          Burn-in time (parsed, unused: mcmc_main.cc:61).\n"
                 "  -t [ --sampling_steps ] arg (=1000)   Length of the annealing process, in MH steps.\n"
                 "  -f [ --sampling_frequency ] arg (=10) (parsed, unused: mcmc_main.cc:64).\n"
                 "  -z [ --bisbm_partition ] arg          bipartite number of blocks to be inferred.\n"
                 "  --uni                                 (parsed, unused).\n"
                 "  -c [ --cooling_schedule ] arg (=abrupt_cool)\n"
                 "                                        exponential, linear, logarithmic, constant, abrupt_cool.\n"
                 "  -a [ --cooling_schedule_kwargs ] arg  Arguments of the cooling schedule (floats).\n"
                 "  -x [ --steps_await ] arg (=1000)      Stop after x steps without a new minimum.\n"
                 "  -E [ --epsilon ] arg (=1)             epsilon of the smart proposal.\n"
                 "  -r [ --randomize ]                    Randomize initial block state.\n"
                 "  -g [ --merge ]                        Start from one block per node and merge down to -z KA KB.\n"
                 "  -u [ --nature ]                       With --merge: merge until a type has fewer than sqrt(2E)/2 blocks.\n"
                 "  -d [ --seed ] arg                     Seed of the mt19937 engine (clock if absent).\n"
                 "  -h [ --help ]                         Produce this help message.\n"
                 "Engine:\n"
                 "  --chains arg (=1)                     Independent chains; the labels of the chain with the lowest\n"
                 "                                        description length are printed.\n"
                 "  --device arg (=0)                     HIP device ordinal.\n"
                 "  --devices arg                         Comma-separated HIP device ordinals: the --chains are spread over them\n"
                 "                                        (contiguous ranges, one handle; results do not depend on the split).\n"
                 "  --rng arg                             mt19937-compat (the reference's draw sequence: the default when -d\n"
                 "                                        is given) or philox (the production chain: the default otherwise).\n"
                 "  --gen_seed arg (=seed+1)              Seed of the reference's hidden second engine (blockmodel.hh:18).\n"
                 "  --reorder                             Renumber the nodes for memory locality before the run (ids without\n"
                 "                                        structure); labels are read and printed in the caller's numbering.\n"
                 "                                        The run is a different, equally valid chain than without the flag.\n"
                 "  --marginalize                         The marginalization mode of README.md:49-94 (the reference parses -b and\n"
                 "                                        -f and drops them): T = 1, -b burn-in steps, then -t steps with a\n"
                 "                                        sample every -f steps (whole sweeps, at least one between samples);\n"
                 "                                        prints every node's most frequent block over samples and chains.\n"
                 "  --align                               With --marginalize: match every chain's block labels to those of the\n"
                 "                                        lowest-description-length chain before pooling (needed for --chains > 1).\n"
                 "  --tempering arg                       With --marginalize: replica exchange over a ladder T0 <= ... <= T{L-1}\n"
                 "                                        (L >= 2 temperatures > 0; --chains a multiple of L; Philox mode): the\n"
                 "                                        chains run in ensembles of L, neighbouring rungs propose to swap\n"
                 "                                        temperatures, and only the chains at T0 are sampled.  The swap\n"
                 "                                        acceptance of every rung pair is reported on stderr.\n"
                 "  --exchange_every arg (=1)             With --tempering: sweeps between exchange rounds.\n"
                 "  --rung_moves MH HB RS SCANS           With --tempering: burn-in and the gaps between samples run as ROUNDS of MH\n"
                 "                                        Metropolis-Hastings sweeps, HB heat-bath sweeps and RS pair reshuffles (SCANS\n"
                 "                                        scans each) of every chain at its rung's temperature, then one exchange;\n"
                 "                                        -b and -f, divided by the node count as always, then count rounds instead\n"
                 "                                        of sweeps.  What each move did per rung is reported on stderr.\n"
                 "  --population arg                      Population annealing over temperatures T0 >= ... >= TL (at least 2, each\n"
                 "                                        > 0; Philox mode) in place of the -c / -a schedule: every chain runs\n"
                 "                                        --population_sweeps sweeps at T0; then, for every further temperature,\n"
                 "                                        the --chains are resampled by description length (chains with a high\n"
                 "                                        one are replaced by copies of chains with a low one) and run that many\n"
                 "                                        sweeps at it.  Prints the chain of the lowest description length; the\n"
                 "                                        log ratio ln Z(1/T_k) / Z(1/T_{k-1}) and the distinct ancestors of every\n"
                 "                                        step, and the total, are reported on stderr.\n"
                 "  --population_sweeps arg (=1)          With --population: sweeps per temperature.\n"
                 "  --population_moves MH HB RS SCANS     With --population: every temperature after the first runs --population_sweeps\n"
                 "                                        ROUNDS of MH Metropolis-Hastings sweeps, HB heat-bath sweeps and RS pair\n"
                 "                                        reshuffles (SCANS scans each) instead of that many sweeps.\n"
                 "  --polish N                            After the annealing run or the merges and before the labels are printed:\n"
                 "                                        up to N greedy sweeps (every node to its block of least description\n"
                 "                                        length, only strictly downhill; Philox mode) until a whole sweep moves\n"
                 "                                        nothing.  Moves and sweeps of every chain are reported on stderr.\n"
                 "  --heatbath                            With --marginalize: burn-in and the sweeps between samples are heat-bath\n"
                 "                                        sweeps (every node draws its block from its exact conditional; Philox\n"
                 "                                        mode, not with --tempering) instead of Metropolis-Hastings sweeps.\n"
                 "  --reshuffle M                         With --marginalize: M pair reshuffles per chain after the burn-in and after\n"
                 "                                        every block of sweeps between samples (the nodes of two blocks of one type\n"
                 "                                        divided afresh and accepted or rejected as a whole; Philox mode, not with\n"
                 "                                        --tempering).  The acceptance is reported on stderr.\n"
                 "  --reshuffle_scans arg (=3)            With --reshuffle: restricted Gibbs scans before the proposal (3 is the\n"
                 "                                        convention of the literature, not a measurement).\n"
                 "  --split_merge M                       With --marginalize and --shape_counts: M split or merge moves per chain after\n"
                 "                                        the burn-in and after every block of sweeps between samples (one block\n"
                 "                                        divided in two, or two blocks of one type made one, accepted or rejected as\n"
                 "                                        a whole), so the chains sample (Ka, Kb) with the partition; Philox mode.\n"
                 "                                        Standard output: the labels of the lowest description length seen.\n"
                 "  --split_merge_scans arg (=3)          With --split_merge: restricted Gibbs scans before the proposal.\n"
                 "  --k_min A B (=1 1)                    With --split_merge: the fewest blocks of type a and of type b.\n"
                 "  --k_max A B                           With --split_merge: the most blocks per type (default: min(n_t, 127)).\n"
                 "  --shape_counts OUT                    With --split_merge: OUT gets one line per visited shape, `ka kb visits S`:\n"
                 "                                        the visits over samples and chains, the lowest description length seen.\n"
                 "  --clamp PATH                          PATH holds node ids separated by white space (any order, repeats allowed):\n"
                 "                                        these nodes keep the labels of --membership_path (required) through every\n"
                 "                                        sweep, reshuffle and exchange round of the run, in every chain; the other\n"
                 "                                        nodes are sampled as always.  Philox mode (--rng philox); not with --merge,\n"
                 "                                        --nature or a -z that differs from the block counts of the membership file.\n"
                 "  --constraints PATH                    PATH holds one line per constrained node: the node id, then the blocks it\n"
                 "                                        may sit in (global labels, blocks of its own type).  Through every sweep,\n"
                 "                                        reshuffle and exchange round of the run a listed node stays inside its\n"
                 "                                        list, in every chain; the labels of --membership_path (required) must\n"
                 "                                        satisfy the lists.  Philox mode (--rng philox); not with --merge, --nature\n"
                 "                                        or a -z that differs from the block counts of the membership file.\n"
                 "  --fields PATH                         PATH holds one line per node with a prior: the node id, then block:weight\n"
                 "                                        pairs (global labels, blocks of its own type, weights above 0; an unlisted\n"
                 "                                        block has weight 1).  Every sweep, reshuffle, exchange round and resampling\n"
                 "                                        step of the run then targets the posterior times these weights, in every\n"
                 "                                        chain: a preference, not a rule (--constraints forbids).  The blocks are\n"
                 "                                        those of --membership_path (required).  Philox mode (--rng philox); not with\n"
                 "                                        --merge, --nature or a -z that differs from the membership file's counts.\n"
                 "  --score_pairs IN OUT                  With --marginalize: IN holds one pair `u v` per line (u of type a, v of\n"
                 "                                        type b); every sample adds every sampled chain's expected edge count\n"
                 "                                        between the two, and OUT receives `u v score` per pair in input order\n"
                 "                                        (score = the mean over samples and chains, printed with %.17g).\n"
                 "  --edge_probs IN OUT                   With --marginalize: IN holds one line `u v`, `u v +` or `u v -` per pair (u of\n"
                 "                                        type a, v of type b; + or nothing: add one edge u - v, -: remove one, which\n"
                 "                                        must be there); every sample adds every sampled chain's exact change dS of\n"
                 "                                        the description length under that edit and exp(-dS), and OUT receives\n"
                 "                                        `u v kind mult mean_dS log_prob` per pair in input order (mult: the edge's\n"
                 "                                        present multiplicity, log_prob = ln mean exp(-dS); %.17g).\n"
                 "  --recommend QUERIES OUT K             With --marginalize: QUERIES holds one node id per line (either type);\n"
                 "                                        every sample adds every sampled chain's expected edge count between the\n"
                 "                                        node and EVERY node of the other type, and OUT receives the K best\n"
                 "                                        candidates of every query that are not its neighbours already, as\n"
                 "                                        `query candidate score` lines in rank order (score descending, ties to\n"
                 "                                        the lowest id; score = the mean over samples and chains, %.17g).\n"
                 "  --recommend_edges QUERIES OUT K       With --marginalize: QUERIES as for --recommend; every sample adds, for the\n"
                 "                                        node and EVERY node of the other type, every sampled chain's exp(-dS) of\n"
                 "                                        the exact change dS of the description length when the edge between the\n"
                 "                                        two is added (the quantity of --edge_probs), and OUT receives the K best\n"
                 "                                        candidates of every query that are not its neighbours already, as\n"
                 "                                        `query candidate score log_prob` lines in rank order (score = mean\n"
                 "                                        exp(-dS) descending, ties to the lowest id; log_prob = ln score; %.17g).\n"
                 "  --include_edges                       With --recommend or --recommend_edges: the query's neighbours are ranked\n"
                 "                                        as well.\n"
                 "  --similar QUERIES OUT K               With --marginalize: QUERIES holds one node id per line (either type);\n"
                 "                                        every sample counts, for EVERY node of the query's own type, the\n"
                 "                                        sampled chains in which it shares the query's block, and OUT receives\n"
                 "                                        the K nodes that do so most often (the query itself left out) as\n"
                 "                                        `query node probability` lines in rank order (count descending, ties\n"
                 "                                        to the lowest id; probability = count / (samples x chains), %.17g).\n"
                 "  --foldin QUERIES OUT K                With --marginalize and --foldin_alpha: QUERIES holds one node that is NOT\n"
                 "                                        in the graph per line, `a|b id id id ...`: its type and its neighbours,\n"
                 "                                        nodes of the other type (ids as in the edge list file; they may repeat).\n"
                 "                                        Every sample gives it a block posterior in every sampled chain; OUT\n"
                 "                                        receives, per line of QUERIES, `line recommend node score` for the K\n"
                 "                                        nodes of the other type with the largest expected edge count (the listed\n"
                 "                                        ones left out), then `line similar node probability` for the K nodes of\n"
                 "                                        its own type most likely to share its block (means over samples and\n"
                 "                                        chains, %.17g; lines count from 0, empty lines not counted).\n"
                 "  --foldin_alpha A                      With --foldin: the smoothing constant of the block posterior, A > 0.\n"
                 "  --conditionals QUERIES OUT            With --marginalize: QUERIES holds one node id per line (either type);\n"
                 "                                        every sample evaluates, in every sampled chain, the node's full\n"
                 "                                        conditional over the blocks of its type given all other labels, and OUT\n"
                 "                                        receives `node stay entropy margin` per line of QUERIES: the mean\n"
                 "                                        probability of its current block, the mean entropy of the conditional\n"
                 "                                        (nats) and the mean cost of the cheapest other block (nats; over the\n"
                 "                                        chains where the node is not alone in its block, nan if there is none),\n"
                 "                                        %.17g.  With --align the line goes on with the node's soft marginal over\n"
                 "                                        the blocks of its type (the conditionals averaged through the alignment).\n"
                 "  --conditionals_beta B                 With --conditionals: the inverse temperature of the conditional, B > 0\n"
                 "                                        (default 1).\n"
                 "  --conditionals_held                   With --conditionals: evaluate the held row instead -- the conditional the\n"
                 "                                        samplers sample under --clamp, --constraints and --fields (a clamped node\n"
                 "                                        is a point mass, a barred block has probability 0, the field is added).\n"
                 "  --least_settled OUT K [entropy|stay]  With --conditionals: OUT receives `query node value` for the K lines of\n"
                 "                                        QUERIES (counted from 0) with the largest mean entropy (the default) or\n"
                 "                                        the smallest mean stay, selected on the device, %.17g; ties in line order.\n"
                 "  --modes OUT THRESHOLD                 With --marginalize: after the last sample the sampled chains' partitions\n"
                 "                                        are compared (variation of information, nats) and grouped into modes:\n"
                 "                                        chains joined by a path of pairs with VI <= THRESHOLD share a mode.  OUT\n"
                 "                                        receives `chain mode VI-to-the-mode's-medoid` per sampled chain; the\n"
                 "                                        modes' sizes, shares and medoids are reported on stderr.\n"
                 "  --mode_marginals PREFIX               With --marginalize --modes: the chains are grouped into modes after the\n"
                 "                                        burn-in and every mode gets a histogram of its own, aligned to its own\n"
                 "                                        lowest-description-length chain.  PREFIX.<g>.txt receives `label count`\n"
                 "                                        per node for mode g (the node's most frequent block within the mode and\n"
                 "                                        how many chain samples chose it); stdout gets the labels of the heaviest\n"
                 "                                        mode.  Not with --tempering (unless --reassign).\n"
                 "  --reassign                            With --mode_marginals: the grouping only picks one anchor per mode (its\n"
                 "                                        lowest-description-length chain); every sample counts each chain into the\n"
                 "                                        mode of its nearest anchor if its VI to it is <= THRESHOLD.  Allowed with\n"
                 "                                        --tempering (the chains at T0 are counted).  PREFIX.assignment.txt\n"
                 "                                        receives `chain visits-per-mode` per chain and a last line `unassigned N`;\n"
                 "                                        a mode's reported share is its share of the samples.\n"
                 "  --trace OUT DEPTH                     With --marginalize: every chain keeps its last DEPTH sampled partitions\n"
                 "                                        (1 <= DEPTH <= 1024) and every sample is compared with them.  OUT receives\n"
                 "                                        `lag pairs mean_VI mean_changed` per lag (in samples; means over the\n"
                 "                                        chains: VI in nats, the share of nodes whose label differs), then\n"
                 "                                        `tau_S window` per chain, in chain order (the integrated autocorrelation\n"
                 "                                        time of the description length, in samples, Sokal's window with c = 5;\n"
                 "                                        window = samples / 2 means the run was too short), then one line with\n"
                 "                                        rhat_S, the split R-hat of the description length over the chains.\n"
                 "  --block_summary OUT                   With --marginalize --align, or with --modes ... --mode_marginals ...\n"
                 "                                        (--reassign included): every sample also sums the counted chains' block\n"
                 "                                        states in the numbering of the node marginals.  OUT receives one section\n"
                 "                                        per mode (the pooled histogram is mode 0): `mode g terms T ka KA kb KB`,\n"
                 "                                        then the lines n_mean, n_sd, m_r_mean, m_r_sd (KA + KB values each: block\n"
                 "                                        sizes and degrees) and e_mean R, e_sd R for every type-a block R (KB\n"
                 "                                        values each: edges to every type-b block), all printed with %.17g.\n"
                 "  --csr_cache                           Keep a binary CSR beside the edge list (<path>.bisbm_csr, checked\n"
                 "                                        against the file's size and mtime); the text file stays the input.\n";
}

}  // namespace

int main(int argc, char const* argv[]) {
    var_map_t var_map;
    std::string err;
    if (!parse_command_line(argc, argv, var_map, err)) {
        std::cerr << err << "\n";
        return 1;
    }
    auto count = [&](const char* k) { return var_map.count(k) ? var_map[k].size() : (size_t)0; };
    auto single = [&](const char* k, const char* dflt) { return count(k) ? var_map[k].back() : std::string(dflt); };

    if (count("help") > 0 || argc == 1) {  // mcmc_main.cc:99-105
        print_help(argv[0]);
        return 0;
    }
    if (count("align") && !count("marginalize")) {
        std::cerr << "--align aligns the chains' block labels before pooling: it needs --marginalize.\n";
        return 1;
    }
    if (count("score_pairs") && !count("marginalize")) {
        std::cerr << "--score_pairs scores pairs of nodes over the samples of the chains: it needs --marginalize.\n";
        return 1;
    }
    if (count("score_pairs") && var_map["score_pairs"].size() != 2) {
        std::cerr << "Invalid --score_pairs. Two paths: the file of pairs to read and the file of scores to write.\n";
        return 1;
    }
    if (count("edge_probs") && !count("marginalize")) {
        std::cerr << "--edge_probs weighs edges over the samples of the chains: it needs --marginalize.\n";
        return 1;
    }
    if (count("edge_probs") && var_map["edge_probs"].size() != 2) {
        std::cerr << "Invalid --edge_probs. Two paths: the file of pairs to read and the file of results to write.\n";
        return 1;
    }
    if ((count("recommend") || count("include_edges")) && !count("marginalize")) {
        std::cerr << "--recommend ranks the candidates of nodes over the samples of the chains: it needs --marginalize.\n";
        return 1;
    }
    if (count("recommend_edges") && !count("marginalize")) {
        std::cerr << "--recommend_edges ranks the candidates of nodes over the samples of the chains: it needs --marginalize.\n";
        return 1;
    }
    if (count("include_edges") && !count("recommend") && !count("recommend_edges")) {
        std::cerr << "--include_edges keeps a query's neighbours among its candidates: it needs --recommend.\n";
        return 1;
    }
    uint32_t recommend_k = 0;
    if (var_map.count("recommend")) {
        if (var_map["recommend"].size() != 3) {
            std::cerr << "Invalid --recommend. Three arguments: the file of query nodes to read, the file to write and K.\n";
            return 1;
        }
        const std::string tok = var_map["recommend"][2];
        char* end = nullptr;
        const unsigned long k = std::strtoul(tok.c_str(), &end, 10);
        if (tok.empty() || *end != '\0' || tok[0] == '-' || tok[0] == '+' || k == 0 || k > 0xffffffffUL) {
            std::cerr << "Invalid --recommend. K must be a positive integer, e.g. --recommend queries.txt out.txt 10.\n";
            return 1;
        }
        recommend_k = (uint32_t)k;
    }
    uint32_t recommend_edges_k = 0;
    if (var_map.count("recommend_edges")) {
        if (var_map["recommend_edges"].size() != 3) {
            std::cerr << "Invalid --recommend_edges. Three arguments: the file of query nodes to read, the file to write and K.\n";
            return 1;
        }
        const std::string tok = var_map["recommend_edges"][2];
        char* end = nullptr;
        const unsigned long k = std::strtoul(tok.c_str(), &end, 10);
        if (tok.empty() || *end != '\0' || tok[0] == '-' || tok[0] == '+' || k == 0 || k > 0xffffffffUL) {
            std::cerr << "Invalid --recommend_edges. K must be a positive integer, e.g. --recommend_edges queries.txt out.txt 10.\n";
            return 1;
        }
        recommend_edges_k = (uint32_t)k;
    }
    if (count("similar") && !count("marginalize")) {
        std::cerr << "--similar counts the chains in which nodes share a block over the samples of the chains: it needs --marginalize.\n";
        return 1;
    }
    uint32_t similar_k = 0;
    if (var_map.count("similar")) {
        if (var_map["similar"].size() != 3) {
            std::cerr << "Invalid --similar. Three arguments: the file of query nodes to read, the file to write and K.\n";
            return 1;
        }
        const std::string tok = var_map["similar"][2];
        char* end = nullptr;
        const unsigned long k = std::strtoul(tok.c_str(), &end, 10);
        if (tok.empty() || *end != '\0' || tok[0] == '-' || tok[0] == '+' || k == 0 || k > 0xffffffffUL) {
            std::cerr << "Invalid --similar. K must be a positive integer, e.g. --similar queries.txt out.txt 10.\n";
            return 1;
        }
        if (k > 1024) {  // (bisbm_coassign_topk's limit, known before a device is touched)
            std::cerr << "Invalid --similar. K is at most 1024, the most nodes the selection on the device returns per query.\n";
            return 1;
        }
        similar_k = (uint32_t)k;
    }
    if ((count("foldin") || count("foldin_alpha")) && !count("marginalize")) {
        std::cerr << "--foldin folds nodes that are not in the graph into the samples of the chains: it needs --marginalize.\n";
        return 1;
    }
    if (count("foldin_alpha") && !count("foldin")) {
        std::cerr << "--foldin_alpha sets the smoothing constant of the fold-in queries: it needs --foldin.\n";
        return 1;
    }
    if ((count("conditionals") || count("conditionals_beta")) && !count("marginalize")) {
        std::cerr << "--conditionals evaluates the nodes' full conditionals at the samples of the chains: it needs --marginalize.\n";
        return 1;
    }
    if (count("conditionals_beta") && !count("conditionals")) {
        std::cerr << "--conditionals_beta sets the inverse temperature of the node conditionals: it needs --conditionals.\n";
        return 1;
    }
    if (count("conditionals_held") && !count("conditionals")) {
        std::cerr << "--conditionals_held evaluates the node conditionals under the clamp, the constraints and the fields: it needs --conditionals.\n";
        return 1;
    }
    if (count("least_settled") && !count("conditionals")) {
        std::cerr << "--least_settled ranks the query nodes of the node conditionals: it needs --conditionals.\n";
        return 1;
    }
    uint32_t least_settled_k = 0, least_settled_by = BISBM_SETTLED_BY_ENTROPY;
    if (var_map.count("least_settled")) {
        const std::vector<std::string>& a = var_map["least_settled"];
        char* end = nullptr;
        const unsigned long long k = a.size() >= 2 ? std::strtoull(a[1].c_str(), &end, 10) : 0;
        if (a.size() < 2 || a.size() > 3 || a[1].empty() || a[1][0] == '-' || *end != '\0' || k == 0 || k > 1024 ||
            (a.size() == 3 && a[2] != "entropy" && a[2] != "stay")) {
            std::cerr << "Invalid --least_settled. The file to write, K in [1, 1024] and optionally entropy or stay, e.g. --least_settled out.txt 10 stay.\n";
            return 1;
        }
        least_settled_k = (uint32_t)k;
        if (a.size() == 3 && a[2] == "stay") least_settled_by = BISBM_SETTLED_BY_STAY;
    }
    double conditionals_beta = 1.;
    if (var_map.count("conditionals")) {
        if (var_map["conditionals"].size() != 2) {
            std::cerr << "Invalid --conditionals. Two arguments: the file of query nodes to read and the file to write.\n";
            return 1;
        }
        if (count("conditionals_beta")) {
            const std::string b = single("conditionals_beta", "");
            char* end = nullptr;
            conditionals_beta = std::strtod(b.c_str(), &end);
            if (b.empty() || *end != '\0' || !std::isfinite(conditionals_beta) || !(conditionals_beta > 0.)) {
                std::cerr << "Invalid --conditionals_beta. A finite number > 0, e.g. --conditionals_beta 1.\n";
                return 1;
            }
        }
    }
    uint32_t foldin_k = 0;
    double foldin_alpha = 0.;
    if (var_map.count("foldin")) {
        if (var_map["foldin"].size() != 3) {
            std::cerr << "Invalid --foldin. Three arguments: the file of virtual nodes to read, the file to write and K.\n";
            return 1;
        }
        const std::string tok = var_map["foldin"][2];
        char* end = nullptr;
        const unsigned long k = std::strtoul(tok.c_str(), &end, 10);
        if (tok.empty() || *end != '\0' || tok[0] == '-' || tok[0] == '+' || k == 0 || k > 0xffffffffUL) {
            std::cerr << "Invalid --foldin. K must be a positive integer, e.g. --foldin new_nodes.txt out.txt 10.\n";
            return 1;
        }
        if (k > 1024) {  // (bisbm_foldin_topk's limit, known before a device is touched)
            std::cerr << "Invalid --foldin. K is at most 1024, the most nodes the selection on the device returns per row.\n";
            return 1;
        }
        foldin_k = (uint32_t)k;
        if (!count("foldin_alpha")) {
            std::cerr << "--foldin needs --foldin_alpha A, the smoothing constant of the block posterior (A > 0; the model's -E epsilon is a usual choice).\n";
            return 1;
        }
        const std::string a = single("foldin_alpha", "");
        foldin_alpha = std::strtod(a.c_str(), &end);
        if (a.empty() || *end != '\0' || !std::isfinite(foldin_alpha) || !(foldin_alpha > 0.)) {
            std::cerr << "Invalid --foldin_alpha. A finite number > 0, e.g. --foldin_alpha 0.1.\n";
            return 1;
        }
    }
    double modes_threshold = 0.;
    if (var_map.count("modes") && !count("marginalize")) {
        std::cerr << "--modes groups the sampled chains' partitions into modes: it needs --marginalize.\n";
        return 1;
    }
    if (var_map.count("modes")) {
        if (var_map["modes"].size() != 2) {
            std::cerr << "Invalid --modes. Two arguments: the file to write and the VI threshold (nats) that joins two chains.\n";
            return 1;
        }
        const std::string tok = var_map["modes"][1];
        char* end = nullptr;
        modes_threshold = std::strtod(tok.c_str(), &end);
        if (tok.empty() || *end != '\0' || !std::isfinite(modes_threshold) || !(modes_threshold >= 0.)) {
            std::cerr << "Invalid --modes. The threshold must be a finite number >= 0 (nats), e.g. --modes modes.txt 0.05.\n";
            return 1;
        }
    }
    uint32_t trace_depth = 0;
    if (var_map.count("trace") && !count("marginalize")) {
        std::cerr << "--trace compares every sample of a chain with its earlier samples: it needs --marginalize.\n";
        return 1;
    }
    if (var_map.count("trace")) {
        if (var_map["trace"].size() != 2) {
            std::cerr << "Invalid --trace. Two arguments: the file to write and the number of earlier samples every chain keeps.\n";
            return 1;
        }
        const std::string tok = var_map["trace"][1];
        char* end = nullptr;
        const unsigned long long d = std::strtoull(tok.c_str(), &end, 10);
        if (tok.empty() || *end != '\0' || tok[0] == '-' || d < 1 || d > 1024) {
            std::cerr << "Invalid --trace. The depth must be an integer in 1 .. 1024, e.g. --trace trace.txt 16.\n";
            return 1;
        }
        trace_depth = (uint32_t)d;
    }
    if (count("block_summary") && !(count("marginalize") && (count("align") || count("mode_marginals")))) {
        std::cerr << "--block_summary sums the chains' block states in the numbering of aligned samples: it needs --marginalize with --align, or with --modes "
                     "and --mode_marginals.\n";
        return 1;
    }
    if (count("mode_marginals") && !var_map.count("modes")) {
        std::cerr << "--mode_marginals counts one histogram per mode: it needs --modes (with --marginalize) for the grouping.\n";
        return 1;
    }
    if (count("reassign") && !count("mode_marginals")) {
        std::cerr << "--reassign counts every sample into the mode of its nearest anchor: it needs --mode_marginals (with --marginalize --modes).\n";
        return 1;
    }
    if (count("mode_marginals") && count("tempering") && !count("reassign")) {
        std::cerr << "--mode_marginals gives every chain a mode of its own: it cannot be combined with --tempering, where chains trade temperatures.\n";
        return 1;
    }
    // replica exchange: the ladder and the exchange period are checked before anything else runs
    std::vector<float> ladder;
    uint32_t exchange_every = 1;
    if ((count("tempering") || count("exchange_every")) && !count("marginalize")) {
        std::cerr << "--tempering runs replica exchange for the marginals of the coldest chains: it needs --marginalize.\n";
        return 1;
    }
    if (count("exchange_every") && !count("tempering")) {
        std::cerr << "--exchange_every sets the period of the exchange rounds: it needs --tempering.\n";
        return 1;
    }
    if (count("tempering")) {
        for (const std::string& tok : var_map["tempering"]) {
            char* end = nullptr;
            const float T = std::strtof(tok.c_str(), &end);
            if (tok.empty() || *end != '\0' || !std::isfinite(T) || !(T > 0.f) || (!ladder.empty() && T < ladder.back())) {
                std::cerr << "Invalid --tempering. A non-decreasing ladder of at least 2 finite temperatures > 0, e.g. --tempering 1 1.5 2.5 4.\n";
                return 1;
            }
            ladder.push_back(T);
        }
        if (ladder.size() < 2) {
            std::cerr << "Invalid --tempering. A non-decreasing ladder of at least 2 finite temperatures > 0, e.g. --tempering 1 1.5 2.5 4.\n";
            return 1;
        }
        if (count("exchange_every")) {
            const std::string v = single("exchange_every", "1");
            char* end = nullptr;
            const unsigned long k = std::strtoul(v.c_str(), &end, 10);
            if (v.empty() || *end != '\0' || v[0] == '-' || k > 0xffffffffUL) {
                std::cerr << "Invalid --exchange_every. Sweeps between exchange rounds: an integer >= 0 (0: no exchanges).\n";
                return 1;
            }
            exchange_every = (uint32_t)k;
        }
    }
    // greedy polishing and heat-bath sampling: checked before anything else runs (the RNG mode below, once it is known)
    uint64_t polish_sweeps = 0;
    if (count("polish")) {
        if (count("marginalize")) {
            std::cerr << "--polish moves the annealed chains to a local minimum before they are printed: it cannot be combined with --marginalize.\n";
            return 1;
        }
        const std::string v = single("polish", "");
        char* end = nullptr;
        const unsigned long long k = std::strtoull(v.c_str(), &end, 10);
        if (v.empty() || *end != '\0' || v[0] == '-' || k == 0) {
            std::cerr << "Invalid --polish. The largest number of greedy sweeps: an integer >= 1, e.g. --polish 100.\n";
            return 1;
        }
        polish_sweeps = k;
    }
    if (count("heatbath") && !count("marginalize")) {
        std::cerr << "--heatbath runs the sweeps of the marginalization mode as heat-bath sweeps: it needs --marginalize.\n";
        return 1;
    }
    if (count("heatbath") && count("tempering")) {
        std::cerr << "--heatbath cannot be combined with --tempering: heat-bath sweeps inside replica exchange are asked for with --rung_moves MH HB RS SCANS.\n";
        return 1;
    }
    uint64_t reshuffle_moves = 0;
    uint32_t reshuffle_scans = 3;
    if (count("reshuffle_scans") && !count("reshuffle")) {
        std::cerr << "--reshuffle_scans sets the scans of the pair reshuffles: it needs --reshuffle.\n";
        return 1;
    }
    if (count("reshuffle")) {
        if (!count("marginalize")) {
            std::cerr << "--reshuffle runs pair reshuffles between the sweeps of the marginalization mode: it needs --marginalize.\n";
            return 1;
        }
        if (count("tempering")) {
            std::cerr << "--reshuffle cannot be combined with --tempering: pair reshuffles inside replica exchange are asked for with --rung_moves MH HB RS SCANS.\n";
            return 1;
        }
        const std::string v = single("reshuffle", ""), t = single("reshuffle_scans", "3");
        char *end = nullptr, *end2 = nullptr;
        const unsigned long long k = std::strtoull(v.c_str(), &end, 10), sc = std::strtoull(t.c_str(), &end2, 10);
        if (v.empty() || *end != '\0' || v[0] == '-' || k == 0) {
            std::cerr << "Invalid --reshuffle. The moves per chain after every block of sweeps: an integer >= 1, e.g. --reshuffle 10.\n";
            return 1;
        }
        if (t.empty() || *end2 != '\0' || t[0] == '-' || sc > 0xffffffffull) {
            std::cerr << "Invalid --reshuffle_scans. An integer >= 0, e.g. --reshuffle_scans 3.\n";
            return 1;
        }
        reshuffle_moves = k, reshuffle_scans = (uint32_t)sc;
    }
    // --split_merge M [--split_merge_scans T] [--k_min A B] [--k_max A B] --shape_counts OUT
    uint64_t split_merge_moves = 0;
    uint32_t split_merge_scans = 3;
    std::array<uint32_t, 2> sm_k_min{1, 1}, sm_k_max{0, 0};  // (k_max {0, 0}: the library's default)
    std::string shape_counts_path;
    for (const char* name : {"split_merge_scans", "k_min", "k_max", "shape_counts"})
        if (count(name) && !count("split_merge")) {
            std::cerr << "--" << name << " belongs to the split and merge moves: it needs --split_merge.\n";
            return 1;
        }
    if (count("split_merge")) {
        if (!count("marginalize")) {
            std::cerr << "--split_merge runs split and merge moves between the sweeps of the marginalization mode: it needs --marginalize.\n";
            return 1;
        }
        if (!count("shape_counts")) {
            std::cerr << "--split_merge changes the chains' block counts, so there is no pooled label histogram: it needs --shape_counts OUT for the histogram of visited shapes.\n";
            return 1;
        }
        for (const char* other : {"tempering", "population", "align", "reshuffle", "clamp", "constraints", "fields", "modes", "mode_marginals", "block_summary",
                                  "trace", "recommend", "recommend_edges", "score_pairs", "edge_probs", "similar", "foldin", "conditionals", "polish"})
            if (count(other)) {
                std::cerr << "--split_merge cannot be combined with --" << other
                          << ": the moves renumber blocks and change the chains' block counts (marginalize(split_merges=) of the Python package keeps the numbering-free sums).\n";
                return 1;
            }
        const std::string v = single("split_merge", ""), t = single("split_merge_scans", "3");
        char *end = nullptr, *end2 = nullptr;
        const unsigned long long k = std::strtoull(v.c_str(), &end, 10), sc = std::strtoull(t.c_str(), &end2, 10);
        if (v.empty() || *end != '\0' || v[0] == '-' || k == 0) {
            std::cerr << "Invalid --split_merge. The moves per chain after every block of sweeps: an integer >= 1, e.g. --split_merge 4.\n";
            return 1;
        }
        if (t.empty() || *end2 != '\0' || t[0] == '-' || sc > 0xffffffffull) {
            std::cerr << "Invalid --split_merge_scans. An integer >= 0, e.g. --split_merge_scans 3.\n";
            return 1;
        }
        for (const char* name : {"k_min", "k_max"}) {
            if (!count(name)) continue;
            auto const& vals = var_map.at(name);
            std::array<uint32_t, 2>& dst = std::string(name) == "k_min" ? sm_k_min : sm_k_max;
            bool ok = vals.size() == 2;
            for (size_t i = 0; ok && i < 2; ++i) {
                char* e = nullptr;
                const unsigned long long x = std::strtoull(vals[i].c_str(), &e, 10);
                ok = !vals[i].empty() && *e == '\0' && vals[i][0] != '-' && x >= 1 && x <= 254;
                dst[i] = (uint32_t)x;
            }
            if (!ok) {
                std::cerr << "Invalid --" << name << ". Two integers >= 1, the blocks of type a and of type b, e.g. --" << name << " 1 1.\n";
                return 1;
            }
        }
        if (count("k_max") && (sm_k_min[0] > sm_k_max[0] || sm_k_min[1] > sm_k_max[1] || sm_k_max[0] + sm_k_max[1] > 254)) {
            std::cerr << "Invalid --k_max. At least --k_min per type and at most 254 blocks in all.\n";
            return 1;
        }
        shape_counts_path = single("shape_counts", "");
        if (shape_counts_path.empty()) {
            std::cerr << "Invalid --shape_counts. A path to write, e.g. --shape_counts shapes.txt.\n";
            return 1;
        }
        split_merge_moves = k, split_merge_scans = (uint32_t)sc;
    }
    // the moves of a round (--rung_moves with --tempering, --population_moves with --population): four integers MH HB RS SCANS
    bisbm_round_recipe rung_moves{}, population_moves{};
    bool have_rung_moves = false, have_population_moves = false;
    for (const char* name : {"rung_moves", "population_moves"}) {
        if (!count(name)) continue;
        const bool pop = std::string(name) == "population_moves";
        const char* needs = pop ? "population" : "tempering";
        if (!count(needs)) {
            std::cerr << "--" << name << " sets the moves of a round of --" << needs << ": it needs --" << needs << ".\n";
            return 1;
        }
        uint32_t v[4] = {0, 0, 0, 0};
        bool ok = var_map[name].size() == 4;
        for (size_t i = 0; ok && i < 4; ++i) {
            const std::string& tok = var_map[name][i];
            char* end = nullptr;
            const unsigned long long k = std::strtoull(tok.c_str(), &end, 10);
            ok = !tok.empty() && tok[0] >= '0' && tok[0] <= '9' && *end == '\0' && k < (1ull << 32);
            v[i] = (uint32_t)k;
        }
        if (!ok || (!v[0] && !v[1] && !v[2])) {
            std::cerr << "Invalid --" << name << ". Four integers >= 0, MH HB RS SCANS, not all of MH HB RS zero, e.g. --" << name << " 1 0 2 3.\n";
            return 1;
        }
        (pop ? population_moves : rung_moves) = bisbm_round_recipe{v[0], v[1], v[2], v[3]};
        (pop ? have_population_moves : have_rung_moves) = true;
    }
    // population annealing: the temperatures and the sweeps per temperature are checked before anything else runs (one more
    // refusal, an initial partition without the -z block counts, waits below until the partition has been read: before the
    // ka != KA branch, which would merge down to -z instead of running the population)
    std::vector<float> population;
    uint64_t population_sweeps = 1;
    if (count("population_sweeps") && !count("population")) {
        std::cerr << "--population_sweeps sets the sweeps per temperature of a population run: it needs --population.\n";
        return 1;
    }
    if (count("population")) {
        if (count("marginalize")) {
            std::cerr << "--population anneals the chains and prints the best one: it cannot be combined with --marginalize. For marginals of an annealed "
                         "population use the Python interface: population_anneal, then marginalize with no burn-in.\n";
            return 1;
        }
        for (const std::string& tok : var_map["population"]) {
            char* end = nullptr;
            const float T = std::strtof(tok.c_str(), &end);
            if (tok.empty() || *end != '\0' || !std::isfinite(T) || !(T > 0.f) || (!population.empty() && T > population.back())) {
                population.clear();
                break;
            }
            population.push_back(T);
        }
        if (population.size() < 2) {
            std::cerr << "Invalid --population. At least 2 finite temperatures > 0 that do not rise, e.g. --population 4 2.5 1.5 1.\n";
            return 1;
        }
        if (count("population_sweeps")) {
            const std::string v = single("population_sweeps", "1");
            char* end = nullptr;
            const unsigned long long k = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || *end != '\0' || v[0] == '-' || v[0] == '+') {
                std::cerr << "Invalid --population_sweeps. Sweeps per temperature: an integer >= 0.\n";
                return 1;
            }
            population_sweeps = k;
        }
        if (count("merge")) {
            std::cerr << "--population replaces the cooling schedule of the annealing run: it cannot be combined with --merge.\n";
            return 1;
        }
        if (single("rng", count("seed") ? "mt19937-compat" : "philox") != "philox") {  // (-d alone selects mt19937-compat)
            std::cerr << "--population runs in Philox mode only (mt19937-compat is the reference's verification path): add --rng philox.\n";
            return 1;
        }
    }
    if (count("edge_list_path") == 0) {
        std::cerr << "edge_list_path is required (-e flag)\n";
        return 1;
    }
    size_t NA = 0, NB = 0;
    uint_vec_t types_init;
    uint_vec_t y = to_uints(var_map["types"]);
    if (count("types") == 0) {
        std::cerr << "types is required for bisbm mode (-y flag)\n";
        return 1;
    } else if (y.size() != 2) {
        std::cerr << "Number of types must be equal to 2!\n";
        return 1;
    } else {
        NA = y[0];
        NB = y[1];
        types_init.assign(NA + NB, 0);
        for (size_t i = NA; i < NA + NB; ++i) types_init[i] = 1;
    }
    // --score_pairs: the pairs are read and checked before any device is touched (ids as in the edge list file)
    edge_list_t score_pairs;
    if (count("score_pairs")) {
        const std::string in = var_map["score_pairs"][0];
        if (!load_edge_list(score_pairs, in)) {
            std::cerr << "[error] --score_pairs: cannot read " << in << "\n";
            return 1;
        }
        for (size_t i = 0; i < score_pairs.size(); ++i)
            if (score_pairs[i].first >= NA || score_pairs[i].second < NA || score_pairs[i].second >= NA + NB) {
                std::cerr << "[error] --score_pairs: pair " << i << " (" << score_pairs[i].first << " " << score_pairs[i].second
                          << ") must name a type-a node [0, " << NA << ") and a type-b node [" << NA << ", " << NA + NB << ")\n";
                return 1;
            }
    }
    // --edge_probs: the pairs are read and checked before any device is touched (ids as in the edge list file); that every `-`
    // names an edge of the graph is checked once the graph is loaded, below
    edge_list_t edge_prob_pairs;
    std::vector<uint8_t> edge_prob_kinds;
    if (count("edge_probs")) {
        const std::string in = var_map["edge_probs"][0];
        std::ifstream file(in);
        if (!file) {
            std::cerr << "[error] --edge_probs: cannot read " << in << "\n";
            return 1;
        }
        std::string text;
        for (size_t line_no = 1; std::getline(file, text); ++line_no) {
            std::istringstream fields(text);
            std::vector<std::string> tok;
            for (std::string t; fields >> t;) tok.push_back(t);
            if (tok.empty()) continue;
            auto is_id = [](const std::string& t) { return !t.empty() && t.size() <= 18 && t.find_first_not_of("0123456789") == std::string::npos; };
            if (tok.size() < 2 || tok.size() > 3 || !is_id(tok[0]) || !is_id(tok[1]) || (tok.size() == 3 && tok[2] != "+" && tok[2] != "-")) {
                std::cerr << "[error] --edge_probs: line " << line_no << " of " << in << " is not `u v`, `u v +` or `u v -`: " << text << "\n";
                return 1;
            }
            edge_prob_pairs.emplace_back((size_t)std::stoull(tok[0]), (size_t)std::stoull(tok[1]));
            edge_prob_kinds.push_back(tok.size() == 3 && tok[2] == "-" ? BISBM_EDGE_REMOVE : BISBM_EDGE_ADD);
        }
        for (size_t i = 0; i < edge_prob_pairs.size(); ++i)
            if (edge_prob_pairs[i].first >= NA || edge_prob_pairs[i].second < NA || edge_prob_pairs[i].second >= NA + NB) {
                std::cerr << "[error] --edge_probs: pair " << i << " (" << edge_prob_pairs[i].first << " " << edge_prob_pairs[i].second
                          << ") must name a type-a node [0, " << NA << ") and a type-b node [" << NA << ", " << NA + NB << ")\n";
                return 1;
            }
    }
    // --recommend: the queries are read and checked before any device is touched (ids as in the edge list file)
    std::vector<uint32_t> recommend_queries;
    if (var_map.count("recommend")) {
        const std::string in = var_map["recommend"][0];
        std::ifstream file(in);
        if (!file) {
            std::cerr << "[error] --recommend: cannot read " << in << "\n";
            return 1;
        }
        std::string text;
        for (size_t line_no = 1; std::getline(file, text); ++line_no) {
            const size_t b = text.find_first_not_of(" \t\r");
            if (b == std::string::npos) continue;  // (an empty line)
            const size_t e = text.find_last_not_of(" \t\r");
            const std::string tok = text.substr(b, e - b + 1);
            char* end = nullptr;
            const unsigned long long id = std::strtoull(tok.c_str(), &end, 10);
            if (*end != '\0' || tok[0] == '-' || tok[0] == '+' || id >= NA + NB) {
                std::cerr << "[error] --recommend: line " << line_no << " of " << in << " (" << tok << ") must name a node [0, " << NA + NB << ")\n";
                return 1;
            }
            recommend_queries.push_back((uint32_t)id);
        }
    }
    // --recommend_edges: likewise
    std::vector<uint32_t> recommend_edges_queries;
    if (var_map.count("recommend_edges")) {
        const std::string in = var_map["recommend_edges"][0];
        std::ifstream file(in);
        if (!file) {
            std::cerr << "[error] --recommend_edges: cannot read " << in << "\n";
            return 1;
        }
        std::string text;
        for (size_t line_no = 1; std::getline(file, text); ++line_no) {
            const size_t b = text.find_first_not_of(" \t\r");
            if (b == std::string::npos) continue;  // (an empty line)
            const size_t e = text.find_last_not_of(" \t\r");
            const std::string tok = text.substr(b, e - b + 1);
            char* end = nullptr;
            const unsigned long long id = std::strtoull(tok.c_str(), &end, 10);
            if (*end != '\0' || tok[0] == '-' || tok[0] == '+' || id >= NA + NB) {
                std::cerr << "[error] --recommend_edges: line " << line_no << " of " << in << " (" << tok << ") must name a node [0, " << NA + NB
                          << ")\n";
                return 1;
            }
            recommend_edges_queries.push_back((uint32_t)id);
        }
    }
    // --similar: likewise
    std::vector<uint32_t> similar_queries;
    if (var_map.count("similar")) {
        const std::string in = var_map["similar"][0];
        std::ifstream file(in);
        if (!file) {
            std::cerr << "[error] --similar: cannot read " << in << "\n";
            return 1;
        }
        std::string text;
        for (size_t line_no = 1; std::getline(file, text); ++line_no) {
            const size_t b = text.find_first_not_of(" \t\r");
            if (b == std::string::npos) continue;  // (an empty line)
            const size_t e = text.find_last_not_of(" \t\r");
            const std::string tok = text.substr(b, e - b + 1);
            char* end = nullptr;
            const unsigned long long id = std::strtoull(tok.c_str(), &end, 10);
            if (*end != '\0' || tok[0] == '-' || tok[0] == '+' || id >= NA + NB) {
                std::cerr << "[error] --similar: line " << line_no << " of " << in << " (" << tok << ") must name a node [0, " << NA + NB << ")\n";
                return 1;
            }
            similar_queries.push_back((uint32_t)id);
        }
    }
    // --conditionals: likewise
    std::vector<uint32_t> conditional_queries;
    if (var_map.count("conditionals")) {
        const std::string in = var_map["conditionals"][0];
        std::ifstream file(in);
        if (!file) {
            std::cerr << "[error] --conditionals: cannot read " << in << "\n";
            return 1;
        }
        std::string text;
        for (size_t line_no = 1; std::getline(file, text); ++line_no) {
            const size_t b = text.find_first_not_of(" \t\r");
            if (b == std::string::npos) continue;  // (an empty line)
            const size_t e = text.find_last_not_of(" \t\r");
            const std::string tok = text.substr(b, e - b + 1);
            char* end = nullptr;
            const unsigned long long id = std::strtoull(tok.c_str(), &end, 10);
            if (*end != '\0' || tok[0] == '-' || tok[0] == '+' || id >= NA + NB) {
                std::cerr << "[error] --conditionals: line " << line_no << " of " << in << " (" << tok << ") must name a node [0, " << NA + NB << ")\n";
                return 1;
            }
            conditional_queries.push_back((uint32_t)id);
        }
    }
    // --foldin: the virtual nodes are read and checked before any device is touched (ids as in the edge list file)
    std::vector<uint8_t> foldin_types;
    std::vector<std::vector<uint32_t>> foldin_lists;
    if (var_map.count("foldin")) {
        const std::string in = var_map["foldin"][0];
        std::ifstream file(in);
        if (!file) {
            std::cerr << "[error] --foldin: cannot read " << in << "\n";
            return 1;
        }
        std::string text;
        for (size_t line_no = 1; std::getline(file, text); ++line_no) {
            std::istringstream words(text);
            std::string tok;
            if (!(words >> tok)) continue;  // (an empty line)
            if (tok != "a" && tok != "b") {
                std::cerr << "[error] --foldin: line " << line_no << " of " << in << " must begin with the node's type, a or b (found " << tok << ")\n";
                return 1;
            }
            const bool type_b = tok == "b";
            std::vector<uint32_t> ids;
            while (words >> tok) {
                char* end = nullptr;
                const unsigned long long id = std::strtoull(tok.c_str(), &end, 10);
                if (*end != '\0' || tok[0] == '-' || tok[0] == '+') {
                    std::cerr << "[error] --foldin: line " << line_no << " of " << in << ": " << tok << " is not a node id\n";
                    return 1;
                }
                if (type_b ? id >= NA : (id < NA || id >= NA + NB)) {
                    std::cerr << "[error] --foldin: line " << line_no << " of " << in << ": the neighbours of a type-" << (type_b ? "b" : "a")
                              << " node are type-" << (type_b ? "a" : "b") << " nodes [" << (type_b ? 0 : NA) << ", " << (type_b ? NA : NA + NB)
                              << "), " << tok << " is not\n";
                    return 1;
                }
                ids.push_back((uint32_t)id);
            }
            if (ids.empty()) {
                std::cerr << "[error] --foldin: line " << line_no << " of " << in << " names no neighbour\n";
                return 1;
            }
            foldin_types.push_back(type_b ? 1 : 0);
            foldin_lists.push_back(ids);
        }
    }
    const std::string cooling_schedule = single("cooling_schedule", "abrupt_cool");
    const size_t sampling_steps = std::strtoull(single("sampling_steps", "1000").c_str(), nullptr, 10);
    const size_t steps_await = std::strtoull(single("steps_await", "1000").c_str(), nullptr, 10);
    const double epsilon = std::strtod(single("epsilon", "1").c_str(), nullptr);
    float_vec_t kwargs(2, 0);
    if (count("cooling_schedule_kwargs") == 0) {  // defaults, mcmc_main.cc:134-153
        if (cooling_schedule == "exponential") {
            kwargs[0] = 1;
            kwargs[1] = 0.99f;
        }
        if (cooling_schedule == "linear") {
            kwargs[0] = (float)(sampling_steps + 1);
            kwargs[1] = 1;
        }
        if (cooling_schedule == "logarithmic") {
            kwargs[0] = 1;
            kwargs[1] = 1;
        }
        if (cooling_schedule == "constant") kwargs[0] = 1;
        if (cooling_schedule == "abrupt_cool") kwargs[0] = (float)steps_await;
    } else {  // checks, mcmc_main.cc:155-218
        auto const& a = var_map["cooling_schedule_kwargs"];
        kwargs.assign(std::max<size_t>(2, a.size()), 0);
        for (size_t i = 0; i < a.size(); ++i) kwargs[i] = std::strtof(a[i].c_str(), nullptr);
        if (cooling_schedule == "exponential") {
            if (kwargs[0] <= 0) {
                std::cerr << "Invalid cooling schedule argument for linear schedule: T_0 must be grater than 0.\n";
                std::cerr << "Passed value: T_0=" << kwargs[0] << "\n";
                return 1;
            }
            if (kwargs[1] <= 0 || kwargs[1] >= 1) {
                std::cerr << "Invalid cooling schedule argument for exponential schedule: alpha must be in ]0,1[.\n";
                std::cerr << "Passed value: alpha=" << kwargs[1] << "\n";
                return 1;
            }
        } else if (cooling_schedule == "linear") {
            if (kwargs[0] <= 0) {
                std::cerr << "Invalid cooling schedule argument for linear schedule: T_0 must be grater than 0.\n";
                std::cerr << "Passed value: T_0=" << kwargs[0] << "\n";
                return 1;
            }
            if (kwargs[1] <= 0 || kwargs[1] > kwargs[0]) {
                std::cerr << "Invalid cooling schedule argument for linear schedule: eta must be in ]0, T_0].\n";
                std::cerr << "Passed value: T_0=" << kwargs[0] << ", eta=" << kwargs[1] << "\n";
                return 1;
            }
            if (kwargs[1] * sampling_steps > kwargs[0]) {
                std::cerr << "Invalid cooling schedule argument for linear schedule: eta * sampling_steps must be "
                             "smaller or equal to T_0.\n";
                std::cerr << "Passed value: eta*sampling_steps=" << kwargs[1] * sampling_steps << ", T_0=" << kwargs[0]
                          << "\n";
                return 1;
            }
        } else if (cooling_schedule == "logarithmic") {
            if (kwargs[0] <= 0) {
                std::cerr << "Invalid cooling schedule argument for logarithmic schedule: c must be greater than 0.\n";
                std::cerr << "Passed value: c=" << kwargs[0] << "\n";
                return 1;
            }
            if (kwargs[1] <= 0) {
                std::cerr << "Invalid cooling schedule argument for logarithmic schedule: d must be greater than 0.\n";
                std::cerr << "Passed value: d=" << kwargs[1] << "\n";
                return 1;
            }
        } else if (cooling_schedule == "constant") {
            if (kwargs[0] <= 0) {
                std::cerr << "Invalid cooling schedule argument for constant schedule: temperature must be greater "
                             "than 0.\n";
                std::cerr << "Passed value: T=" << kwargs[0] << "\n";
                return 1;
            }
        } else if (cooling_schedule == "abrupt_cool") {
            if (kwargs[0] <= 0) {
                std::cerr << "Invalid cooling schedule argument for abrupt_cool schedule: tau must be larger than 0. \n";
                std::cerr << "Passed value: tau=" << kwargs[0] << "\n";
                return 1;
            }
        } else {
            std::cerr << "Invalid cooling schedule. Options are exponential, linear, logarithmic, abrupt_cool.\n";
            return 1;
        }
    }
    // mcmc_main.cc:219-226 tests var_map.count("epsilon"), which is always 1 because of the default value
    bool randomize = count("randomize") > 0;
    const bool merge = count("merge") > 0, nature = count("nature") > 0;
    if (count("clamp")) {  // (what can be refused before anything is loaded)
        if (!count("membership_path")) {
            std::cerr << "--clamp holds the listed nodes at the labels of a membership file: it needs --membership_path.\n";
            return 1;
        }
        if (merge || nature) {
            std::cerr << "--clamp cannot be combined with " << (merge ? "--merge" : "--nature") << ": a merge renumbers the blocks whose labels the clamp holds.\n";
            return 1;
        }
    }
    if (count("constraints")) {
        if (!count("membership_path")) {
            std::cerr << "--constraints needs a start that satisfies the lists: it needs --membership_path.\n";
            return 1;
        }
        if (merge || nature) {
            std::cerr << "--constraints cannot be combined with " << (merge ? "--merge" : "--nature") << ": a merge renumbers the blocks that the lists name.\n";
            return 1;
        }
    }
    if (count("fields")) {
        if (!count("membership_path")) {
            std::cerr << "--fields names the blocks of a membership file: it needs --membership_path.\n";
            return 1;
        }
        if (merge || nature) {
            std::cerr << "--fields cannot be combined with " << (merge ? "--merge" : "--nature") << ": a merge renumbers the blocks that the file names.\n";
            return 1;
        }
    }
    size_t seed;
    if (count("seed") == 0)
        seed = (size_t)std::chrono::high_resolution_clock::now().time_since_epoch().count();  // :236-239
    else
        seed = std::strtoull(single("seed", "0").c_str(), nullptr, 10);

    // ---- initial partition, mcmc_main.cc:241-326 ----
    uint_vec_t memberships_init, n = to_uints(var_map["n"]), z = to_uints(var_map["bisbm_partition"]);
    uint_vec_t mb = to_uints(var_map["mb"]);
    size_t N = 0, KA = 0, KB = 0;
    bool prepared = false;
    if (count("membership_path") != 0) {
        std::clog << "Loading nodes' membership from membership_path.\n";
        if (!load_memberships(memberships_init, single("membership_path", ""))) {
            std::clog << "WARNING: error in loading memberships, read memberships from block sizes\n";
        } else {
            randomize = false;
            unsigned max_n_ka = 0, max_n_kb = 0;
            for (size_t i = 0; i < memberships_init.size(); ++i) {
                if (i < y[0] && memberships_init[i] > max_n_ka) max_n_ka = memberships_init[i];
                if (memberships_init[i] > max_n_kb) max_n_kb = memberships_init[i];
            }
            KA = max_n_ka + 1;
            KB = max_n_kb - max_n_ka;
            prepared = true;
            N = memberships_init.size();
            std::clog << " ---- read membership from file! ---- \n";
        }
    } else if (count("mb") > 0) {
        size_t accu = 0;
        for (auto it : n) accu += it;
        if (mb.size() != accu) {
            std::cerr << "[error] input vector size of memberships is different from the number of nodes \n";
            output_vec(mb, std::cerr);
            std::cerr << "#mb = " << mb.size() << "; while #nodes = " << accu << ". \n";
            return 1;
        }
        memberships_init = mb;
        if (z.size() < 2) {
            std::cerr << "number of partitions is required (-z flag)\n";
            return 1;
        }
        KA = z[0];
        KB = z[1];
        N = memberships_init.size();
        prepared = true;
    }
    if (!prepared) {
        if (count("n") == 0) {
            std::cerr << "n is required (-n flag) if one does not specify the membership of nodes\n";
            return 1;
        }
        for (size_t r = 0; r < n.size(); ++r)
            for (size_t i = 0; i < n[r]; ++i) memberships_init.push_back((unsigned)r);
        if (z.size() < 2) {
            std::cerr << "number of partitions is required (-z flag)\n";
            return 1;
        }
        KA = z[0];
        KB = z[1];
        N = memberships_init.size();
    }
    if (memberships_init.size() != types_init.size()) {  // :328-333
        std::cerr << memberships_init.size() << ", " << types_init.size() << '\n';
        std::cerr << "Types do not sum to the number of vertices!\n";
        return 1;
    }

    // ---- graph, mcmc_main.cc:335-339 ----
    adj_list_t adj_list_loaded;
    if (count("csr_cache")) {  // same arrays as the two calls below, kept in a binary file beside the text
        if (!load_adj_cached(adj_list_loaded, single("edge_list_path", ""), N, true)) {
            std::cerr << "[error] cannot read the edge list, or it names a node id >= " << N << "\n";
            return 1;
        }
    } else {
        edge_list_t edge_list;
        load_edge_list(edge_list, single("edge_list_path", ""));
        adj_list_loaded = edge_to_adj(edge_list, N);
    }
    for (size_t i = 0; i < edge_prob_pairs.size(); ++i) {  // --edge_probs: a `-` needs its edge (still no device touched)
        if (edge_prob_kinds[i] != BISBM_EDGE_REMOVE) continue;
        const size_t u = edge_prob_pairs[i].first, v = edge_prob_pairs[i].second;
        const uint32_t* row = adj_list_loaded.col.data();
        if (std::find(row + adj_list_loaded.rowptr[u], row + adj_list_loaded.rowptr[u + 1], (uint32_t)v) == row + adj_list_loaded.rowptr[u + 1]) {
            std::cerr << "[error] --edge_probs: pair " << i << " (" << u << " " << v << " -) removes an edge the graph does not hold\n";
            return 1;
        }
    }
    // --reorder: the engine works on a renumbered graph; memberships go in and come out in the caller's numbering
    std::vector<uint32_t> new_id;
    if (count("reorder")) {
        new_id = locality_order(adj_list_loaded, NA);
        adj_list_loaded = permute_adj(adj_list_loaded, new_id);
        uint_vec_t moved(memberships_init.size());
        for (size_t v = 0; v < memberships_init.size(); ++v) moved[new_id[v]] = memberships_init[v];
        memberships_init.swap(moved);
    }
    auto emit_labels = [&](const uint_vec_t& engine_labels) {
        if (new_id.empty()) {
            output_vec<uint_vec_t>(engine_labels, std::cout);
            return;
        }
        uint_vec_t mine(engine_labels.size());
        for (size_t v = 0; v < mine.size(); ++v) mine[v] = engine_labels[new_id[v]];
        output_vec<uint_vec_t>(mine, std::cout);
    };
    const adj_list_t& adj_list = adj_list_loaded;
    // --clamp: the mask, in the engine's numbering (--reorder: the engine knows node v by new_id[v])
    std::vector<uint8_t> clamp_mask;
    if (count("clamp")) {
        if (!prepared) {
            std::cerr << "--clamp holds the listed nodes at the labels of --membership_path, which could not be read.\n";
            return 1;
        }
        if (z.size() >= 2 && (z[0] != KA || z[1] != KB)) {
            std::cerr << "--clamp: -z " << z[0] << " " << z[1] << " differs from the " << KA << " + " << KB
                      << " blocks of the membership file, and the merge or split that would follow renumbers blocks.\n";
            return 1;
        }
        std::string why;
        if (!load_clamp(clamp_mask, single("clamp", ""), N, why)) {
            std::cerr << "[error] --clamp: " << why << "\n";
            return 1;
        }
        if (!new_id.empty()) {
            std::vector<uint8_t> moved(clamp_mask.size());
            for (size_t v = 0; v < clamp_mask.size(); ++v) moved[new_id[v]] = clamp_mask[v];
            clamp_mask.swap(moved);
        }
        std::clog << "clamp: " << std::count(clamp_mask.begin(), clamp_mask.end(), (uint8_t)1) << " of " << N << " nodes held\n";
    }
    // --constraints: the class of every node, in the engine's numbering, and the table of allowed blocks per class
    uint32_t cn_classes = 0;
    std::vector<uint8_t> cn_class, cn_allowed;
    if (count("constraints")) {
        if (!prepared) {
            std::cerr << "--constraints needs the labels of --membership_path as a start that satisfies the lists, and the file could not be read.\n";
            return 1;
        }
        if (z.size() >= 2 && (z[0] != KA || z[1] != KB)) {
            std::cerr << "--constraints: -z " << z[0] << " " << z[1] << " differs from the " << KA << " + " << KB
                      << " blocks of the membership file, and the merge or split that would follow renumbers blocks.\n";
            return 1;
        }
        std::string why;
        if (!load_constraints(cn_classes, cn_class, cn_allowed, single("constraints", ""), N, NA, KA, KB, why)) {
            std::cerr << "[error] --constraints: " << why << "\n";
            return 1;
        }
        if (!new_id.empty()) {
            std::vector<uint8_t> moved(cn_class.size());
            for (size_t v = 0; v < cn_class.size(); ++v) moved[new_id[v]] = cn_class[v];
            cn_class.swap(moved);
        }
        std::clog << "constraints: " << (N - (size_t)std::count(cn_class.begin(), cn_class.end(), (uint8_t)0)) << " of " << N << " nodes listed, "
                  << cn_classes << " class(es)\n";
    }
    // --fields: the field class of every node, in the engine's numbering, and the table of energies per class
    uint32_t fl_classes = 0;
    std::vector<uint8_t> fl_class;
    std::vector<double> fl_field;
    if (count("fields")) {
        if (!prepared) {
            std::cerr << "--fields names the blocks of --membership_path, which could not be read.\n";
            return 1;
        }
        if (z.size() >= 2 && (z[0] != KA || z[1] != KB)) {
            std::cerr << "--fields: -z " << z[0] << " " << z[1] << " differs from the " << KA << " + " << KB
                      << " blocks of the membership file, and the merge or split that would follow renumbers blocks.\n";
            return 1;
        }
        std::string why;
        if (!load_fields(fl_classes, fl_class, fl_field, single("fields", ""), N, NA, KA, KB, why)) {
            std::cerr << "[error] --fields: " << why << "\n";
            return 1;
        }
        if (!new_id.empty()) {
            std::vector<uint8_t> moved(fl_class.size());
            for (size_t v = 0; v < fl_class.size(); ++v) moved[new_id[v]] = fl_class[v];
            fl_class.swap(moved);
        }
        std::clog << "fields: " << (N - (size_t)std::count(fl_class.begin(), fl_class.end(), (uint8_t)0)) << " of " << N << " nodes listed, "
                  << fl_classes << " class(es)\n";
    }

    // K implied by the initial labels vs. requested (mcmc_main.cc:406-419)
    size_t ka = 0, kb = 0;
    for (size_t t = 0; t < NA + NB; ++t) {
        if (types_init[t] == 0 && memberships_init[t] > ka)
            ka = memberships_init[t];
        else if (types_init[t] == 1 && memberships_init[t] > kb)
            kb = memberships_init[t];
    }
    kb -= ka;
    ka += 1;
    engine_options opt;
    opt.n_chains = (uint32_t)std::strtoul(single("chains", "1").c_str(), nullptr, 10);
    opt.device = std::atoi(single("device", "0").c_str());
    if (count("devices")) {
        const std::string list = single("devices", "");
        for (size_t pos = 0; pos <= list.size();) {
            const size_t comma = std::min(list.find(',', pos), list.size());
            const std::string item = list.substr(pos, comma - pos);
            char* end = nullptr;
            const long d = std::strtol(item.c_str(), &end, 10);
            if (item.empty() || *end != '\0' || d < 0) {
                std::cerr << "Invalid --devices. A comma-separated list of device ordinals, e.g. 0,1,2,3.\n";
                return 1;
            }
            opt.devices.push_back((int)d);
            pos = comma + 1;
        }
        if (opt.devices.size() > opt.n_chains) {
            std::cerr << "--devices lists " << opt.devices.size() << " devices for --chains " << opt.n_chains << ": every device needs a chain.\n";
            return 1;
        }
        opt.device = opt.devices[0];
    }
    // Without -d the reference seeds its engines from the clock and random_device (mcmc_main.cc:242, blockmodel.hh:17-18): there
    // is no draw sequence to reproduce, so the production chain (Philox) runs.  With -d the default is the verification mode
    // that reproduces the reference's own mt19937 sequence for that seed -- an order of magnitude slower per step.
    const bool seed_given = count("seed") != 0;
    const std::string rng = single("rng", seed_given ? "mt19937-compat" : "philox");
    if (!count("rng") && seed_given)
        std::clog << "rng: mt19937-compat (-d given: the reference's draw sequence for this seed; --rng philox runs the production chain, "
                     "about ten times faster per step)\n";
    if (rng != "mt19937-compat" && rng != "philox") {
        std::cerr << "Invalid --rng. Options are mt19937-compat, philox.\n";
        return 1;
    }
    opt.rng_mode = rng == "philox" ? BISBM_RNG_PHILOX : BISBM_RNG_MT19937_COMPAT;
    if (count("fields") && opt.rng_mode != BISBM_RNG_PHILOX) {
        std::cerr << "--fields runs in Philox mode only (mt19937-compat is the reference's verification path, and the reference has no fields): add --rng philox.\n";
        return 1;
    }
    if (count("constraints") && opt.rng_mode != BISBM_RNG_PHILOX) {
        std::cerr << "--constraints runs in Philox mode only (mt19937-compat is the reference's verification path, and the reference has no constraints): add --rng philox.\n";
        return 1;
    }
    if (count("clamp") && opt.rng_mode != BISBM_RNG_PHILOX) {
        std::cerr << "--clamp runs in Philox mode only (mt19937-compat is the reference's verification path, and the reference has no clamp): add --rng philox.\n";
        return 1;
    }
    if ((polish_sweeps || count("heatbath") || reshuffle_moves || split_merge_moves) && opt.rng_mode != BISBM_RNG_PHILOX) {
        std::cerr << (polish_sweeps ? "--polish" : count("heatbath") ? "--heatbath" : reshuffle_moves ? "--reshuffle" : "--split_merge")
                  << " runs in Philox mode only (mt19937-compat is the reference's verification path): add --rng philox.\n";
        return 1;
    }
    if (!ladder.empty()) {
        if (opt.n_chains % ladder.size()) {
            std::cerr << "--tempering with " << ladder.size() << " temperatures needs --chains a multiple of " << ladder.size() << " (got " << opt.n_chains
                      << ").\n";
            return 1;
        }
        // --devices: the chains are split into contiguous ranges, the first n_chains % devices one chain longer (bisbm_create_multi);
        // every range must hold whole ensembles
        const size_t nd = opt.devices.size();
        if (nd > 1 && ((opt.n_chains / nd) % ladder.size() || (opt.n_chains % nd) != 0)) {
            std::cerr << "--tempering with " << ladder.size() << " temperatures over " << nd << " devices needs --chains a multiple of "
                      << ladder.size() * nd << " (every device's share a multiple of " << ladder.size() << "; got " << opt.n_chains << ").\n";
            return 1;
        }
        if (opt.rng_mode != BISBM_RNG_PHILOX) {
            std::cerr << "--tempering runs in Philox mode only (mt19937-compat is the reference's verification path): add --rng philox.\n";
            return 1;
        }
    }
    opt.seed = seed;
    opt.gen_seed = count("gen_seed") ? std::strtoull(single("gen_seed", "0").c_str(), nullptr, 10) : seed + 1;

    // ---- agglomerative drivers, mcmc_main.cc:349-451 ----
    const double sigma = 1.01;  // :349
    const float_vec_t agg_merge_kwargs(1, 0.f);
    // --polish: greedy sweeps of every chain until a whole sweep moves nothing, before the best chain is picked
    auto polish_chains = [&](blockmodel_t& blockmodel, uint32_t first_chain) {
        if (!polish_sweeps) return;
        std::vector<uint64_t> moved, sweeps;
        blockmodel.polish(polish_sweeps, moved, sweeps);
        std::ostringstream lines;  // (one write: the runs of --merge --nature --chains report from threads of their own)
        for (size_t c = 0; c < moved.size(); ++c)
            lines << "polish: chain " << first_chain + c << " moved " << moved[c] << " node(s) in " << sweeps[c] << " sweep(s)\n";
        std::clog << lines.str();
    };
    auto print_best = [&](blockmodel_t& blockmodel, bool with_k) {
        polish_chains(blockmodel, 0);
        uint32_t best = 0;
        if (opt.n_chains > 1) {
            const std::vector<double> dl = blockmodel.entropy_all();
            for (uint32_t c = 1; c < opt.n_chains; ++c)
                if (dl[c] < dl[best]) best = c;
            std::clog << "chains " << opt.n_chains << ", printing chain " << best << "\n";
        }
        blockmodel.summary(best);
        if (with_k) std::cout << blockmodel.get_KA() << " " << blockmodel.get_KB() << " ";  // :401-403
        emit_labels(*blockmodel.get_memberships(best));
    };
    // one stage per pair of the plan: merge, then a greedy sweep except after the last stage (:380-396, :425-444)
    auto staged_merges = [&](blockmodel_t& blockmodel, metropolis_hasting& algorithm, const std::vector<int>& ka_s,
                             const std::vector<int>& kb_s) -> bool {
        for (size_t i = 0; i + 1 < ka_s.size(); ++i) {
            blockmodel.agg_merge(-(ka_s[i + 1] - ka_s[i]), -(kb_s[i + 1] - kb_s[i]), 10);
            if (i != ka_s.size() - 2) {
                if (cooling_schedule != "abrupt_cool") {
                    std::cerr << "Only abrupt cooling annealing is supported.";
                    return false;
                }
                algorithm.anneal(blockmodel, &abrupt_cool_schedule, agg_merge_kwargs, (NA + NB) * 1, steps_await);
            }
        }
        return true;
    };
    if (merge) {
        // the start is one block per node (:350-353): ask the library whether it serves that many blocks (its wide mode ends at
        // about 14 000) before the expensive part starts
        if (NA + NB > 65535 || bisbm_check_shape((uint32_t)NA, (uint32_t)NB, opt.rng_mode) != BISBM_OK) {
            std::cerr << "[error] --merge starts from one block per node (" << NA + NB << " blocks): "
                      << (NA + NB > 65535 ? "block labels are at most two bytes on the device" : bisbm_last_error(nullptr))
                      << ". Start from an initial partition of fewer blocks (-n / --mb / --membership_path with a larger -z "
                         "than wanted is merged down the same way, mcmc_main.cc:419-450).\n";
            return 3;
        }
        try {
            std::iota(memberships_init.begin(), memberships_init.end(), 0);  // every node its own block (:350)
            if (nature && opt.n_chains > 1) {
                // agg_merge(engine, diff, nm) lets every run end with its own (Ka,Kb) (blockmodel.cc:208-271), and in this
                // driver every run also has its own stage sizes (ceil of ITS block count) and its own last stage: --nature
                // --chains N therefore runs every chain in a handle of its own with its global chain id (same streams as in
                // one handle), and prints the best.  (One handle does serve chains of
                // different shapes -- bisbm_agg_merge_total -- but applies one diff to all of them per call.)
                // The runs are independent handles: up to eight of them are in flight at a time, each on a host thread of its own
                // (its handle has its own stream; with --devices they take turns over the listed devices).
                if (cooling_schedule != "abrupt_cool" &&  // (the reference notices inside its first merge stage, :370-376)
                    std::min(NA, NB) >= (size_t)std::ceil(std::sqrt(2. * (double)(adj_list.col.size() / 2)) / 2)) {
                    std::cerr << "Only abrupt cooling annealing is supported.";
                    return 1;
                }
                struct run_result {
                    double dl = std::numeric_limits<double>::infinity();
                    uint_vec_t labels;
                    size_t ka = 0, kb = 0;
                    std::string error;
                };
                std::vector<run_result> runs(opt.n_chains);
                auto run_one = [&](uint32_t c) {
                    try {
                        engine_options one = opt;
                        one.n_chains = 1;
                        one.first_chain_id = opt.first_chain_id + c;
                        if (!opt.devices.empty()) one.device = opt.devices[c % opt.devices.size()];  // (--devices: the runs take turns)
                        one.devices.clear();
                        blockmodel_t blockmodel(memberships_init, types_init, NA + NB, NA, NB, epsilon, &adj_list, one);
                        blockmodel.init_bisbm();
                        metropolis_hasting algorithm;
                        size_t tKA = NA, tKB = NB, tGroups = NA + NB;
                        const size_t ceiling = (size_t)std::ceil(std::sqrt(2. * blockmodel.get_num_edges()) / 2);
                        while (tKA >= ceiling && tKB >= ceiling) {  // :357-377
                            blockmodel.agg_merge((int)std::ceil(tGroups * (sigma - 1) / sigma), 10);
                            tKA = blockmodel.get_KA();
                            tKB = blockmodel.get_KB();
                            tGroups = tKA + tKB;
                            algorithm.anneal(blockmodel, &abrupt_cool_schedule, agg_merge_kwargs, (NA + NB) * 1, steps_await);
                        }
                        algorithm.anneal(blockmodel, &abrupt_cool_schedule, kwargs, sampling_steps, steps_await);  // :398
                        polish_chains(blockmodel, c);
                        runs[c].dl = blockmodel.entropy_all()[0];
                        runs[c].labels = *blockmodel.get_memberships(0);
                        runs[c].ka = blockmodel.get_KA();
                        runs[c].kb = blockmodel.get_KB();
                    } catch (const std::exception& e) {
                        runs[c].error = e.what();
                    }
                };
                {
                    const uint32_t width = std::min<uint32_t>(opt.n_chains, 8u);
                    std::vector<std::thread> pool;
                    std::atomic<uint32_t> next{0};
                    for (uint32_t t = 0; t < width; ++t)
                        pool.emplace_back([&] {
                            for (uint32_t c = next++; c < opt.n_chains; c = next++) run_one(c);
                        });
                    for (auto& t : pool) t.join();
                }
                double best_dl = std::numeric_limits<double>::infinity();
                uint_vec_t best_labels;
                size_t best_ka = 0, best_kb = 0, best_chain = 0;
                for (uint32_t c = 0; c < opt.n_chains; ++c) {
                    if (!runs[c].error.empty()) throw std::runtime_error(runs[c].error);
                    if (runs[c].dl < best_dl) {  // (the first of equals, as when the runs went one after the other)
                        best_dl = runs[c].dl;
                        best_labels = runs[c].labels;
                        best_ka = runs[c].ka;
                        best_kb = runs[c].kb;
                        best_chain = c;
                    }
                }
                std::clog << "chains " << opt.n_chains << ", printing chain " << best_chain << "\n";
                std::clog << "(Ka, Kb) = (" << best_ka << ", " << best_kb << ") \n";  // summary(), blockmodel.cc:748-751
                std::clog << "entropy: " << best_dl << "\n";
                std::cout << best_ka << " " << best_kb << " ";  // :401-403
                emit_labels(best_labels);
                return 0;
            }
            blockmodel_t blockmodel(memberships_init, types_init, NA + NB, NA, NB, epsilon, &adj_list, opt);
            blockmodel.init_bisbm();
            metropolis_hasting algorithm;
            if (nature) {  // :354-376
                size_t tKA = NA, tKB = NB, tGroups = NA + NB;
                const size_t ceiling = (size_t)std::ceil(std::sqrt(2. * blockmodel.get_num_edges()) / 2);
                while (tKA >= ceiling && tKB >= ceiling) {
                    blockmodel.agg_merge((int)std::ceil(tGroups * (sigma - 1) / sigma), 10);
                    tKA = blockmodel.get_KA();
                    tKB = blockmodel.get_KB();
                    tGroups = tKA + tKB;
                    if (cooling_schedule != "abrupt_cool") {
                        std::cerr << "Only abrupt cooling annealing is supported.";
                        return 1;
                    }
                    algorithm.anneal(blockmodel, &abrupt_cool_schedule, agg_merge_kwargs, (NA + NB) * 1, steps_await);
                }
            } else {  // :377-397
                const auto plan = geospace((long)NA, (long)KA, (long)NB, (long)KB, sigma);
                if (!staged_merges(blockmodel, algorithm, plan.first, plan.second)) return 1;
            }
            algorithm.anneal(blockmodel, &abrupt_cool_schedule, kwargs, sampling_steps, steps_await);  // :398
            print_best(blockmodel, nature);
        } catch (const std::exception& e) {
            std::cerr << e.what() << "\n";
            return 3;
        }
        return 0;
    }
    if (ka != KA || kb != KB) {  // the initial partition has other block counts than asked for (:419-450)
        if (count("fields")) {
            std::cerr << "--fields: the initial partition has " << ka << " + " << kb << " blocks, not " << KA << " + " << KB
                      << ", and the merge or split that would follow renumbers blocks.\n";
            return 1;
        }
        if (count("constraints")) {
            std::cerr << "--constraints: the initial partition has " << ka << " + " << kb << " blocks, not " << KA << " + " << KB
                      << ", and the merge or split that would follow renumbers blocks.\n";
            return 1;
        }
        if (count("clamp")) {
            std::cerr << "--clamp: the initial partition has " << ka << " + " << kb << " blocks, not " << KA << " + " << KB
                      << ", and the merge or split that would follow renumbers blocks.\n";
            return 1;
        }
        if (!population.empty()) {
            std::cerr << "--population replaces the cooling schedule of the annealing run: the initial partition must have the -z block counts.\n";
            return 1;
        }
        try {
            int diff_a = (int)ka - (int)KA, diff_b = (int)kb - (int)KB;
            blockmodel_t blockmodel(memberships_init, types_init, ka + kb, ka, kb, epsilon, &adj_list, opt);
            blockmodel.init_bisbm();
            metropolis_hasting algorithm;
            if (diff_a >= 0 && diff_b >= 0) {
                const auto plan = geospace((long)(KA + diff_a), (long)KA, (long)(KB + diff_b), (long)KB, sigma);
                if (plan.first.size() == 1) blockmodel.agg_merge(diff_a, diff_b, 10);
                if (!staged_merges(blockmodel, algorithm, plan.first, plan.second)) return 1;
            } else {
                blockmodel.agg_merge(diff_a, diff_b, 100);  // :446 (negative diffs: agg_split)
            }
            algorithm.anneal(blockmodel, &abrupt_cool_schedule, kwargs, sampling_steps, steps_await);  // :447
            print_best(blockmodel, false);
        } catch (const std::exception& e) {
            std::cerr << e.what() << "\n";
            return 3;
        }
        return 0;
    }

    if (var_map.count("marginalize")) {
        // The marginalization mode README.md:49-94 describes and the reference's main never runs (-b and -f are parsed
        // and dropped, mcmc_main.cc:61-65): constant T = 1; -b burn-in steps; then -t sampling steps with a sample every
        // -f steps; every sample adds every chain's labels to a per-node histogram; the output line is each node's most
        // frequent block.  Steps are executed in whole sweeps, as anneal() does (duration / N), with at least one sweep
        // between samples.
        try {
            const size_t N = NA + NB;
            const size_t burn_in = std::strtoull(single("burn_in", "1000").c_str(), nullptr, 10);
            const size_t freq = std::strtoull(single("sampling_frequency", "10").c_str(), nullptr, 10);
            const size_t sweeps_between = std::max<size_t>(1, freq / N);
            const size_t n_samples = sampling_steps / (sweeps_between * N);
            blockmodel_t blockmodel(memberships_init, types_init, KA + KB, KA, KB, epsilon, &adj_list, opt);
            if (!clamp_mask.empty()) blockmodel.clamp(clamp_mask);
            if (cn_classes) blockmodel.constrain(cn_classes, cn_class, cn_allowed);
            if (fl_classes) blockmodel.set_fields(fl_classes, fl_class, fl_field);
            if (randomize)
                blockmodel.shuffle_bisbm();
            else
                blockmodel.init_bisbm();
            metropolis_hasting algorithm;
            const float_vec_t t1{1.f, 0.f};
            const size_t never = std::numeric_limits<size_t>::max();
            // with --tempering every chain runs at its rung's temperature and the exchange rounds run between the sweeps
            if (!ladder.empty()) blockmodel.tempering_set(ladder);
            uint64_t reshuffles_proposed = 0, reshuffles_accepted = 0;
            auto advance = [&](size_t sweeps) {
                if (have_rung_moves)  // (`sweeps` counts rounds)
                    blockmodel.tempering_rounds(sweeps, rung_moves);
                else if (!ladder.empty())
                    blockmodel.tempering_run(sweeps, exchange_every);
                else if (count("heatbath"))
                    blockmodel.heatbath_sweeps(sweeps, 1.0);
                else
                    algorithm.anneal(blockmodel, &constant_schedule, t1, sweeps * N, never);
                if (reshuffle_moves) {  // after every block of sweeps
                    for (uint64_t a : blockmodel.reshuffle(reshuffle_moves, reshuffle_scans, 1.0)) reshuffles_accepted += a;
                    reshuffles_proposed += reshuffle_moves * opt.n_chains;
                }
            };
            if (split_merge_moves) {
                // the chains sample (Ka, Kb): no pooled histogram; the visited shapes are counted and the best state of each kept
                uint64_t proposed = 0, accepted = 0;
                auto advance_shapes = [&](size_t sweeps) {
                    advance(sweeps);
                    for (uint64_t a : blockmodel.split_merge(split_merge_moves, split_merge_scans, 1.0, sm_k_min, sm_k_max)) accepted += a;
                    proposed += split_merge_moves * opt.n_chains;
                };
                if (burn_in >= N) advance_shapes(burn_in / N);
                struct Best {
                    uint64_t visits = 0;
                    bool have = false;
                    double S = 0;
                    uint_vec_t labels;
                };
                std::map<std::pair<size_t, size_t>, Best> shapes;
                for (size_t sample = 0; sample < n_samples; ++sample) {
                    advance_shapes(sweeps_between);
                    const std::vector<double> dl = blockmodel.entropy_all();
                    for (uint32_t c = 0; c < opt.n_chains; ++c) {
                        Best& b = shapes[blockmodel.ka_kb(c)];
                        b.visits += 1;
                        if (!b.have || dl[c] < b.S) b.have = true, b.S = dl[c], b.labels = *blockmodel.get_memberships(c);
                    }
                }
                std::clog << "marginalize: burn-in " << burn_in / N << " sweeps, " << n_samples << " samples " << sweeps_between
                          << " sweep(s) apart, " << opt.n_chains << " chain(s)\n";
                std::clog << "split_merge: " << accepted << " of " << proposed << " split / merge move(s) accepted (" << split_merge_scans << " scan(s))\n";
                if (n_samples == 0) {
                    std::cerr << "[error] --marginalize: -t " << sampling_steps << " steps hold no sample (" << sweeps_between * N << " steps per sample)\n";
                    return 1;
                }
                std::ofstream out(shape_counts_path);
                out.precision(17);
                const Best* best = nullptr;
                for (auto const& kv : shapes) {
                    out << kv.first.first << " " << kv.first.second << " " << kv.second.visits << " " << kv.second.S << "\n";
                    if (!best || kv.second.S < best->S) best = &kv.second;
                }
                if (!out) {
                    std::cerr << "[error] --shape_counts: cannot write " << shape_counts_path << "\n";
                    return 1;
                }
                emit_labels(best->labels);
                return 0;
            }
            if (burn_in >= N) advance(burn_in / N);
            blockmodel.marginals_reset();
            if (count("align")) blockmodel.marginals_set_alignment(true);
            // the sampled chains grouped into modes at `modes_threshold` (--modes): sel = the chains, mode per selected chain,
            // medoid per mode (positions in sel), vi = their distance matrix
            std::vector<uint32_t> sel, mode, medoids;
            std::vector<double> vi;
            auto group_modes = [&] {
                sel.clear();
                const std::vector<uint32_t> rung = ladder.empty() ? std::vector<uint32_t>(opt.n_chains, 0) : blockmodel.tempering_rungs();
                for (uint32_t c = 0; c < opt.n_chains; ++c)
                    if (rung[c] == 0) sel.push_back(c);
                vi = blockmodel.partition_distances(sel);
                blockmodel_t::partition_modes(vi, sel.size(), modes_threshold, mode, medoids);
            };
            const bool per_mode = count("mode_marginals") > 0, reassign = count("reassign") > 0;
            if (per_mode) {  // the grouping after the burn-in decides which histogram a chain is counted into
                group_modes();
                if (reassign) {
                    // ... or only the anchors: every mode's member of the lowest description length; every sample then counts
                    // each (cold) chain into the mode of its nearest anchor within the threshold
                    const std::vector<double> dl = blockmodel.entropy_all();
                    std::vector<uint32_t> anchors;
                    for (size_t k = 0; k < medoids.size(); ++k) {
                        size_t low = sel.size();
                        for (size_t i = 0; i < sel.size(); ++i)
                            if (mode[i] == k && (low == sel.size() || dl[sel[i]] < dl[sel[low]])) low = i;
                        const uint_vec_t* lab = blockmodel.get_memberships(sel[low]);
                        anchors.insert(anchors.end(), lab->begin(), lab->end());
                    }
                    blockmodel.marginals_set_mode_anchors((uint32_t)medoids.size(), anchors, modes_threshold);
                } else {
                    blockmodel.marginals_set_modes((uint32_t)medoids.size(), mode);
                }
            }
            if (count("score_pairs")) {  // (--reorder: the engine knows the nodes by their new ids)
                std::vector<uint32_t> pu, pv;
                for (auto const& pr : score_pairs) {
                    pu.push_back(new_id.empty() ? (uint32_t)pr.first : new_id[pr.first]);
                    pv.push_back(new_id.empty() ? (uint32_t)pr.second : new_id[pr.second]);
                }
                blockmodel.pair_scores_set(pu, pv);
            }
            if (!edge_prob_pairs.empty()) {  // (--reorder: the engine knows the nodes by their new ids)
                std::vector<uint32_t> pu, pv;
                for (auto const& pr : edge_prob_pairs) {
                    pu.push_back(new_id.empty() ? (uint32_t)pr.first : new_id[pr.first]);
                    pv.push_back(new_id.empty() ? (uint32_t)pr.second : new_id[pr.second]);
                }
                blockmodel.edge_probs_set(pu, pv, edge_prob_kinds);
            }
            if (!recommend_queries.empty()) {  // (--reorder: the engine knows the nodes by their new ids)
                std::vector<uint32_t> q;
                for (uint32_t v : recommend_queries) q.push_back(new_id.empty() ? v : new_id[v]);
                blockmodel.query_scores_set(q);
            }
            if (!recommend_edges_queries.empty()) {
                std::vector<uint32_t> q;
                for (uint32_t v : recommend_edges_queries) q.push_back(new_id.empty() ? v : new_id[v]);
                blockmodel.edge_queries_set(q);
            }
            if (!similar_queries.empty()) {
                std::vector<uint32_t> q;
                for (uint32_t v : similar_queries) q.push_back(new_id.empty() ? v : new_id[v]);
                blockmodel.coassign_set(q);
            }
            if (!foldin_types.empty()) {  // (--reorder: the engine knows the nodes by their new ids)
                std::vector<std::vector<uint32_t>> lists = foldin_lists;
                if (!new_id.empty())
                    for (auto& l : lists)
                        for (uint32_t& v : l) v = new_id[v];
                blockmodel.foldin_set(foldin_types, lists, foldin_alpha);
            }
            const bool soft = count("align") && !per_mode;  // the soft marginals take the aligned histogram's reference
            if (!conditional_queries.empty()) {
                std::vector<uint32_t> q;
                for (uint32_t v : conditional_queries) q.push_back(new_id.empty() ? v : new_id[v]);
                blockmodel.conditionals_set(q, conditionals_beta);
                if (count("conditionals_held")) blockmodel.conditionals_held(true);
            }
            if (trace_depth) {
                blockmodel.trace_set(trace_depth);
                blockmodel.trace_reset();
            }
            if (count("block_summary")) blockmodel.block_sums_set(BISBM_BLOCK_SUMS);
            for (size_t sample = 0; sample < n_samples; ++sample) {
                advance(sweeps_between);
                blockmodel.marginals_accumulate();
                if (trace_depth) blockmodel.trace_record();
                if (!conditional_queries.empty()) {
                    if (soft && sample == 0) blockmodel.conditionals_set_reference(blockmodel.marginals_reference_labels());
                    blockmodel.conditionals_accumulate();
                }
                if (!foldin_types.empty()) blockmodel.foldin_accumulate();
                if (!score_pairs.empty()) blockmodel.pair_scores_accumulate();
                if (!edge_prob_pairs.empty()) blockmodel.edge_probs_accumulate();
                if (!recommend_queries.empty()) blockmodel.query_scores_accumulate();
                if (!recommend_edges_queries.empty()) blockmodel.edge_queries_accumulate();
                if (!similar_queries.empty()) blockmodel.coassign_accumulate();
            }
            std::clog << "marginalize: burn-in " << burn_in / N << " sweeps, " << n_samples << " samples " << sweeps_between
                      << " sweep(s) apart, " << opt.n_chains << " chain(s) pooled\n";
            if (reshuffle_moves)
                std::clog << "reshuffle: " << reshuffles_accepted << " of " << reshuffles_proposed << " pair reshuffle(s) accepted (" << reshuffle_scans
                          << " scan(s))\n";
            if (n_samples == 0) {
                std::cerr << "[error] --marginalize: -t " << sampling_steps << " steps hold no sample (" << sweeps_between * N
                          << " steps per sample)\n";
                return 1;
            }
            if (!ladder.empty()) {
                std::vector<uint64_t> att, acc;
                uint64_t rounds = 0;
                blockmodel.tempering_stats(ladder.size(), att, acc, rounds);
                std::clog << "tempering: " << opt.n_chains / ladder.size() << " ensemble(s) of " << ladder.size() << " rungs, " << rounds
                          << " exchange round(s), " << opt.n_chains / ladder.size() << " chain(s) at T0 = " << ladder[0] << " sampled; swap acceptance:";
                for (size_t i = 0; i + 1 < ladder.size(); ++i)
                    std::clog << " " << ladder[i] << "<->" << ladder[i + 1] << " " << acc[i] << "/" << att[i] << " ("
                              << (att[i] ? (double)acc[i] / (double)att[i] : 0.) << ")";
                std::clog << "\n";
                if (have_rung_moves) {
                    const std::vector<uint64_t> rs = blockmodel.tempering_rung_stats(ladder.size());
                    std::clog << "rung moves: rounds of " << rung_moves.mh_sweeps << " MH sweep(s), " << rung_moves.heatbath_sweeps << " heat-bath sweep(s), "
                              << rung_moves.reshuffles << " reshuffle(s) of " << rung_moves.reshuffle_scans << " scan(s); per rung:";
                    for (size_t i = 0; i < ladder.size(); ++i) {
                        const uint64_t* r = rs.data() + 6 * i;
                        std::clog << " T=" << ladder[i] << " mh " << r[1] << "/" << r[0] << " heatbath " << r[3] << "/" << r[2] << " reshuffle " << r[5] << "/" << r[4]
                                  << " (" << (r[4] ? (double)r[5] / (double)r[4] : 0.) << ")";
                    }
                    std::clog << "\n";
                }
            }
            if (count("align") && !per_mode)
                std::clog << "align: labels matched to chain " << blockmodel.marginals_reference_chain() << " (lowest description length)\n";
            if (trace_depth) {
                const std::string out_path = var_map["trace"][0];
                std::ofstream out(out_path);
                std::vector<double> vi_sum, tau;
                std::vector<uint64_t> agree_sum, pairs;
                std::vector<uint32_t> win;
                const uint64_t records = blockmodel.trace_lags(trace_depth, vi_sum, agree_sum, pairs);
                char line[160];
                for (uint32_t a = 0; a < trace_depth; ++a) {  // means over the chains; a lag that was never held: nan
                    double vi = 0., agree = 0.;
                    for (uint32_t c = 0; c < opt.n_chains; ++c) vi += vi_sum[(size_t)c * trace_depth + a], agree += (double)agree_sum[(size_t)c * trace_depth + a];
                    const double den = pairs[a] ? (double)pairs[a] * (double)opt.n_chains : std::nan("");
                    std::snprintf(line, sizeof(line), "%u %llu %.17g %.17g\n", a + 1, (unsigned long long)pairs[a], vi / den, 1. - agree / (den * (double)N));
                    out << line;
                }
                double rhat = std::nan("");
                if (records >= 4) {
                    blockmodel_t::trace_summary(blockmodel.trace_series(BISBM_TRACE_S, records), records, opt.n_chains, 5.0, tau, win, rhat);
                } else {  // (too few samples for a summary)
                    tau.assign(opt.n_chains, std::nan("")), win.assign(opt.n_chains, 0);
                }
                for (uint32_t c = 0; c < opt.n_chains; ++c) {
                    std::snprintf(line, sizeof(line), "%.17g %u\n", tau[c], win[c]);
                    out << line;
                }
                std::snprintf(line, sizeof(line), "%.17g\n", rhat);
                out << line;
                out.close();
                if (!out) {
                    std::cerr << "[error] --trace: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "trace: " << records << " record(s) of " << opt.n_chains << " chain(s), " << trace_depth << " lag(s) -> " << out_path << "\n";
            }
            if (count("score_pairs")) {
                const std::string out_path = var_map["score_pairs"][1];
                std::ofstream out(out_path);
                uint64_t terms = 0;
                const std::vector<double> sum = score_pairs.empty() ? std::vector<double>() : blockmodel.pair_scores(terms);
                char line[128];
                for (size_t i = 0; i < score_pairs.size(); ++i) {
                    std::snprintf(line, sizeof(line), "%zu %zu %.17g\n", score_pairs[i].first, score_pairs[i].second, sum[i] / (double)terms);
                    out << line;
                }
                out.close();
                if (!out) {
                    std::cerr << "[error] --score_pairs: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "score_pairs: " << score_pairs.size() << " pair(s), " << terms << " chain term(s) each -> " << out_path << "\n";
            }
            if (count("edge_probs")) {
                const std::string out_path = var_map["edge_probs"][1];
                std::ofstream out(out_path);
                uint64_t terms = 0;
                std::vector<double> dS_sum, w_sum;
                std::vector<uint32_t> mult;
                if (!edge_prob_pairs.empty()) blockmodel.edge_probs(dS_sum, w_sum, mult, terms);
                char line[192];
                for (size_t i = 0; i < edge_prob_pairs.size(); ++i) {
                    std::snprintf(line, sizeof(line), "%zu %zu %c %u %.17g %.17g\n", edge_prob_pairs[i].first, edge_prob_pairs[i].second,
                                  edge_prob_kinds[i] == BISBM_EDGE_REMOVE ? '-' : '+', mult[i], dS_sum[i] / (double)terms, std::log(w_sum[i] / (double)terms));
                    out << line;
                }
                out.close();
                if (!out) {
                    std::cerr << "[error] --edge_probs: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "edge_probs: " << edge_prob_pairs.size() << " pair(s), " << terms << " chain term(s) each -> " << out_path << "\n";
            }
            if (var_map.count("recommend")) {
                const std::string out_path = var_map["recommend"][1];
                std::ofstream out(out_path);
                uint64_t terms = 0;
                std::vector<uint32_t> nodes;
                std::vector<double> sums;
                if (!recommend_queries.empty()) blockmodel.query_scores_topk(recommend_k, !count("include_edges"), nodes, sums, terms);
                std::vector<uint32_t> old_id(new_id.size());
                for (size_t v = 0; v < new_id.size(); ++v) old_id[new_id[v]] = (uint32_t)v;
                char line[128];
                for (size_t i = 0; i < recommend_queries.size(); ++i)
                    for (size_t r = 0; r < recommend_k; ++r) {
                        const uint32_t node = nodes[i * recommend_k + r];
                        if (node == 0xffffffffu) continue;  // (fewer than K candidates are eligible)
                        std::snprintf(line, sizeof(line), "%u %u %.17g\n", recommend_queries[i], new_id.empty() ? node : old_id[node],
                                      sums[i * recommend_k + r] / (double)terms);
                        out << line;
                    }
                out.close();
                if (!out) {
                    std::cerr << "[error] --recommend: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "recommend: " << recommend_queries.size() << " query node(s), " << recommend_k << " candidate(s) each, " << terms
                          << " chain term(s) per score -> " << out_path << "\n";
            }
            if (var_map.count("recommend_edges")) {
                const std::string out_path = var_map["recommend_edges"][1];
                std::ofstream out(out_path);
                uint64_t terms = 0;
                std::vector<uint32_t> nodes;
                std::vector<double> sums;
                if (!recommend_edges_queries.empty()) blockmodel.edge_queries_topk(recommend_edges_k, !count("include_edges"), nodes, sums, terms);
                std::vector<uint32_t> old_id(new_id.size());
                for (size_t v = 0; v < new_id.size(); ++v) old_id[new_id[v]] = (uint32_t)v;
                char line[160];
                for (size_t i = 0; i < recommend_edges_queries.size(); ++i)
                    for (size_t r = 0; r < recommend_edges_k; ++r) {
                        const uint32_t node = nodes[i * recommend_edges_k + r];
                        if (node == 0xffffffffu) continue;  // (fewer than K candidates are eligible)
                        const double score = sums[i * recommend_edges_k + r] / (double)terms;
                        std::snprintf(line, sizeof(line), "%u %u %.17g %.17g\n", recommend_edges_queries[i], new_id.empty() ? node : old_id[node], score,
                                      score > 0 ? std::log(score) : -INFINITY);
                        out << line;
                    }
                out.close();
                if (!out) {
                    std::cerr << "[error] --recommend_edges: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "recommend_edges: " << recommend_edges_queries.size() << " query node(s), " << recommend_edges_k << " candidate(s) each, "
                          << terms << " chain term(s) per score -> " << out_path << "\n";
            }
            if (var_map.count("similar")) {
                const std::string out_path = var_map["similar"][1];
                std::ofstream out(out_path);
                uint64_t terms = 0;
                std::vector<uint32_t> nodes, counts;
                if (!similar_queries.empty()) blockmodel.coassign_topk(similar_k, nodes, counts, terms);
                std::vector<uint32_t> old_id(new_id.size());
                for (size_t v = 0; v < new_id.size(); ++v) old_id[new_id[v]] = (uint32_t)v;
                char line[128];
                for (size_t i = 0; i < similar_queries.size(); ++i)
                    for (size_t r = 0; r < similar_k; ++r) {
                        const uint32_t node = nodes[i * similar_k + r];
                        if (node == 0xffffffffu) continue;  // (fewer than K nodes are eligible)
                        std::snprintf(line, sizeof(line), "%u %u %.17g\n", similar_queries[i], new_id.empty() ? node : old_id[node],
                                      (double)counts[i * similar_k + r] / (double)terms);
                        out << line;
                    }
                out.close();
                if (!out) {
                    std::cerr << "[error] --similar: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "similar: " << similar_queries.size() << " query node(s), " << similar_k << " node(s) each, " << terms
                          << " chain term(s) per count -> " << out_path << "\n";
            }
            if (var_map.count("foldin")) {
                const std::string out_path = var_map["foldin"][1];
                std::ofstream out(out_path);
                uint64_t terms = 0;
                std::vector<uint32_t> old_id(new_id.size());
                for (size_t v = 0; v < new_id.size(); ++v) old_id[new_id[v]] = (uint32_t)v;
                std::vector<uint32_t> nodes[2];
                std::vector<double> sums[2];
                if (!foldin_types.empty()) {
                    blockmodel.foldin_topk(BISBM_FOLDIN_RECOMMEND, foldin_k, true, nodes[0], sums[0], terms);
                    blockmodel.foldin_topk(BISBM_FOLDIN_SIMILAR, foldin_k, false, nodes[1], sums[1], terms);
                }
                char line[128];
                for (size_t i = 0; i < foldin_types.size(); ++i)
                    for (int kind = 0; kind < 2; ++kind)
                        for (size_t r = 0; r < foldin_k; ++r) {
                            const uint32_t node = nodes[kind][i * foldin_k + r];
                            if (node == 0xffffffffu) continue;  // (fewer than K nodes are eligible)
                            std::snprintf(line, sizeof(line), "%zu %s %u %.17g\n", i, kind ? "similar" : "recommend", new_id.empty() ? node : old_id[node],
                                          sums[kind][i * foldin_k + r] / (double)terms);
                            out << line;
                        }
                out.close();
                if (!out) {
                    std::cerr << "[error] --foldin: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "foldin: " << foldin_types.size() << " virtual node(s), " << foldin_k << " node(s) per row, alpha " << foldin_alpha << ", "
                          << terms << " chain term(s) per sum -> " << out_path << "\n";
            }
            if (var_map.count("conditionals")) {
                const std::string out_path = var_map["conditionals"][1];
                std::ofstream out(out_path);
                blockmodel_t::conditional_stats_t st;
                std::vector<double> prob;
                uint32_t kmax = 0;
                uint64_t prob_terms = 0;
                if (!conditional_queries.empty()) {
                    st = blockmodel.conditionals_stats();
                    if (soft) prob = blockmodel.conditionals_marginals(kmax, prob_terms);
                }
                char num[64];
                for (size_t i = 0; i < conditional_queries.size(); ++i) {
                    const double vals[3] = {st.stay[i] / (double)st.terms, st.entropy[i] / (double)st.terms,
                                            st.free[i] ? st.margin[i] / (double)st.free[i] : std::numeric_limits<double>::quiet_NaN()};
                    out << conditional_queries[i];
                    for (double x : vals) {
                        std::snprintf(num, sizeof(num), " %.17g", x);
                        out << num;
                    }
                    if (soft) {
                        const size_t k_own = conditional_queries[i] < NA ? KA : KB;
                        for (size_t s = 0; s < k_own; ++s) {
                            std::snprintf(num, sizeof(num), " %.17g", prob[i * kmax + s] / (double)prob_terms);
                            out << num;
                        }
                    }
                    out << "\n";
                }
                out.close();
                if (!out) {
                    std::cerr << "[error] --conditionals: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "conditionals: " << conditional_queries.size() << " query node(s), beta " << conditionals_beta << ", " << st.terms
                          << " chain term(s) per sum" << (soft ? ", soft marginals" : "") << (count("conditionals_held") ? ", held rows" : "") << " -> " << out_path
                          << "\n";
            }
            if (var_map.count("least_settled")) {
                const std::string out_path = var_map["least_settled"][0];
                std::ofstream out(out_path);
                std::vector<uint32_t> ranked;
                std::vector<double> values;
                uint64_t terms = 0;
                if (!conditional_queries.empty()) blockmodel.least_settled(least_settled_by, least_settled_k, ranked, values, terms);
                char num[64];
                for (size_t i = 0; i < ranked.size() && ranked[i] != 0xffffffffu; ++i) {
                    std::snprintf(num, sizeof(num), " %.17g", values[i] / (double)terms);
                    out << ranked[i] << " " << conditional_queries[ranked[i]] << num << "\n";
                }
                out.close();
                if (!out) {
                    std::cerr << "[error] --least_settled: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "least_settled: " << least_settled_k << " of " << conditional_queries.size() << " query node(s) by "
                          << (least_settled_by == BISBM_SETTLED_BY_STAY ? "stay" : "entropy") << " -> " << out_path << "\n";
            }
            if (count("block_summary")) {
                // one section per mode: terms, then the means and standard deviations of the sizes, the degrees and the edge counts
                const std::string out_path = var_map["block_summary"][0];
                std::ofstream out(out_path);
                uint32_t n_modes = 1;
                if (per_mode) {
                    std::vector<uint32_t> of_chain;
                    std::vector<int64_t> ref_chain;
                    std::vector<uint64_t> terms;
                    n_modes = blockmodel.marginals_modes(of_chain, ref_chain, terms);
                }
                char num[40];
                for (uint32_t g = 0; g < n_modes; ++g) {
                    std::vector<uint64_t> e, n, d;
                    const uint64_t terms = blockmodel.block_sums(g, e, n, d);
                    out << "mode " << g << " terms " << terms << " ka " << KA << " kb " << KB << "\n";
                    // what = 0: the mean, 1: the standard deviation of `count` cells whose planes are `cells` apart
                    auto row = [&](const char* name, const uint64_t* w, size_t cells, size_t count, int what) {
                        out << name;
                        for (size_t i = 0; i < count; ++i) {
                            const double v = what == 0 ? block_mean(w[i], terms) : std::sqrt(block_variance(w[i], w[cells + i], w[2 * cells + i], terms));
                            std::snprintf(num, sizeof(num), " %.17g", v);
                            out << num;
                        }
                        out << "\n";
                    };
                    const size_t K = KA + KB;
                    row("n_mean", n.data(), K, K, 0);
                    row("n_sd", n.data(), K, K, 1);
                    row("m_r_mean", d.data(), K, K, 0);
                    row("m_r_sd", d.data(), K, K, 1);
                    for (size_t R = 0; R < KA; ++R) row(("e_mean " + std::to_string(R)).c_str(), e.data() + R * KB, KA * KB, KB, 0);
                    for (size_t R = 0; R < KA; ++R) row(("e_sd " + std::to_string(R)).c_str(), e.data() + R * KB, KA * KB, KB, 1);
                }
                out.close();
                if (!out) {
                    std::cerr << "[error] --block_summary: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "block_summary: " << n_modes << " mode(s) -> " << out_path << "\n";
            }
            uint_vec_t heaviest_labels;
            if (per_mode) {
                std::vector<uint32_t> of_chain;
                std::vector<int64_t> ref_chain;
                std::vector<uint64_t> terms;
                const uint32_t M = blockmodel.marginals_modes(of_chain, ref_chain, terms);
                // a mode's share: of the counted chains (a fixed assignment), of the samples (--reassign)
                std::vector<double> size(M, 0.);
                double all = (double)sel.size();
                std::vector<uint64_t> visits;
                uint64_t unassigned = 0, n_counted = 0;
                if (reassign) {
                    blockmodel.marginals_mode_assignment(M, visits, unassigned, n_counted);
                    all = (double)unassigned;
                    for (uint32_t g = 0; g < M; ++g) size[g] = (double)terms[g], all += (double)terms[g];
                } else {
                    for (uint32_t c : of_chain)
                        if (c != BISBM_MODE_NONE) size[c] += 1.;
                }
                uint32_t heaviest = 0;
                std::clog << "mode_marginals: " << M << " mode(s)\n";
                for (uint32_t g = 0; g < M; ++g) {
                    if (size[g] > size[heaviest]) heaviest = g;  // (ties -> the lowest mode)
                    std::vector<uint32_t> top(N, 0);
                    // (--reassign: a mode that no sample fell into has no MAP; its file holds zeroes)
                    const std::vector<uint32_t> lab = terms[g] ? blockmodel.marginals_map_mode(g, &top) : std::vector<uint32_t>(N, 0);
                    const std::string out_path = var_map["mode_marginals"][0] + "." + std::to_string(g) + ".txt";
                    std::ofstream out(out_path);
                    double settled = 0.;
                    for (size_t v = 0; v < N; ++v) {  // (--reorder: the engine knows node v by new_id[v])
                        const size_t e = new_id.empty() ? v : new_id[v];
                        out << lab[e] << " " << top[e] << "\n";
                        if (terms[g]) settled += (double)top[e] / (double)terms[g];
                    }
                    out.close();
                    if (!out) {
                        std::cerr << "[error] --mode_marginals: cannot write " << out_path << "\n";
                        return 1;
                    }
                    std::clog << "mode " << g << ": share " << size[g] / all << ", reference ";
                    if (reassign)
                        std::clog << "its anchor";
                    else
                        std::clog << "chain " << opt.first_chain_id + (uint32_t)ref_chain[g];
                    std::clog << ", " << terms[g] << " term(s), mean top/terms " << settled / (double)N << " -> " << out_path << "\n";
                    if (g == heaviest) heaviest_labels = uint_vec_t(lab.begin(), lab.end());
                }
                if (reassign) {  // one line per chain: its visits per mode; a last line: the samples beyond the threshold
                    const std::string out_path = var_map["mode_marginals"][0] + ".assignment.txt";
                    std::ofstream out(out_path);
                    for (uint32_t c = 0; c < opt.n_chains; ++c) {
                        out << opt.first_chain_id + c;
                        for (uint32_t g = 0; g < M; ++g) out << " " << visits[(size_t)c * M + g];
                        out << "\n";
                    }
                    out << "unassigned " << unassigned << "\n";
                    out.close();
                    if (!out) {
                        std::cerr << "[error] --mode_marginals: cannot write " << out_path << "\n";
                        return 1;
                    }
                    std::clog << "reassign: " << n_counted << " sample(s), " << unassigned << " chain sample(s) beyond the threshold -> " << out_path << "\n";
                }
            }
            if (var_map.count("modes")) {  // (a partition's distance to another does not depend on the node numbering: --reorder is fine)
                group_modes();
                const size_t m = sel.size();
                const std::vector<double> dl = blockmodel.entropy_all();
                const std::string out_path = var_map["modes"][0];
                std::ofstream out(out_path);
                char line[128];
                for (size_t i = 0; i < m; ++i) {
                    std::snprintf(line, sizeof(line), "%u %u %.17g\n", opt.first_chain_id + sel[i], mode[i], vi[i * m + medoids[mode[i]]]);
                    out << line;
                }
                out.close();
                if (!out) {
                    std::cerr << "[error] --modes: cannot write " << out_path << "\n";
                    return 1;
                }
                std::clog << "modes: " << medoids.size() << "\n";
                for (size_t k = 0; k < medoids.size(); ++k) {
                    size_t size = 0, low = m;
                    for (size_t i = 0; i < m; ++i)
                        if (mode[i] == k) {
                            ++size;
                            if (low == m || dl[sel[i]] < dl[sel[low]]) low = i;
                        }
                    std::clog << "mode " << k << ": " << size << " chain(s), share " << (double)size / (double)m << ", medoid chain "
                              << opt.first_chain_id + sel[medoids[k]] << ", lowest description length chain " << opt.first_chain_id + sel[low] << "\n";
                }
            }
            emit_labels(per_mode ? heaviest_labels : blockmodel.marginal_map_labels(NA));
        } catch (const std::exception& e) {
            std::cerr << e.what() << "\n";
            return 3;
        }
        return 0;
    }

    try {
        blockmodel_t blockmodel(memberships_init, types_init, KA + KB, KA, KB, epsilon, &adj_list, opt);  // :453
        if (!clamp_mask.empty()) blockmodel.clamp(clamp_mask);
        if (cn_classes) blockmodel.constrain(cn_classes, cn_class, cn_allowed);
        if (fl_classes) blockmodel.set_fields(fl_classes, fl_class, fl_field);
        if (randomize)
            blockmodel.shuffle_bisbm();
        else
            blockmodel.init_bisbm();
        metropolis_hasting algorithm;
        if (!population.empty()) {
            // population annealing in place of the cooling schedule: the sweeps at T0, then a resampling step and the sweeps per
            // further temperature
            const float_vec_t t0{population[0], 0.f};
            if (population_sweeps) algorithm.anneal(blockmodel, &constant_schedule, t0, population_sweeps * (NA + NB), (size_t)1 << 60);
            std::vector<double> log_ratio, rates;
            std::vector<uint32_t> distinct;
            if (have_population_moves)
                blockmodel.population_rounds(population, population_sweeps, population_moves, log_ratio, distinct, rates);
            else
                blockmodel.population_run(population, population_sweeps, log_ratio, distinct, rates);
            char line[160];
            for (size_t k = 0; k < log_ratio.size(); ++k) {
                std::snprintf(line, sizeof(line), "population step %zu: T %g -> %g, log ratio %.17g, distinct ancestors %u\n", k + 1,
                              (double)population[k], (double)population[k + 1], log_ratio[k], distinct[k]);
                std::clog << line;
            }
            uint64_t rounds = 0;
            double total = 0.;
            blockmodel.population_state(rounds, total);
            std::snprintf(line, sizeof(line), "population: %llu steps, log ratio total %.17g\n", (unsigned long long)rounds, total);
            std::clog << line;
            polish_chains(blockmodel, 0);
            uint32_t best = 0;
            const std::vector<double> dl = blockmodel.entropy_all();
            for (uint32_t c = 1; c < opt.n_chains; ++c)
                if (dl[c] < dl[best]) best = c;
            std::clog << "chains " << opt.n_chains << ", printing chain " << best << "\n";
            std::clog << "acceptance ratio " << rates[best] << "\n";
            blockmodel.summary(best);
            emit_labels(*blockmodel.get_memberships(best));
            return 0;
        }
        schedule_fn fn = cooling_schedule == "exponential"   ? &exponential_schedule
                         : cooling_schedule == "linear"      ? &linear_schedule
                         : cooling_schedule == "logarithmic" ? &logarithmic_schedule
                         : cooling_schedule == "constant"    ? &constant_schedule
                                                             : &abrupt_cool_schedule;
        algorithm.anneal(blockmodel, fn, kwargs, sampling_steps, steps_await);  // :462-482
        polish_chains(blockmodel, 0);
        uint32_t best = 0;
        if (opt.n_chains > 1) {
            const std::vector<double> dl = blockmodel.entropy_all();
            for (uint32_t c = 1; c < opt.n_chains; ++c)
                if (dl[c] < dl[best]) best = c;
            std::clog << "chains " << opt.n_chains << ", printing chain " << best << "\n";
        }
        std::clog << "acceptance ratio " << algorithm.rates()[best] << "\n";  // :483
        blockmodel.summary(best);                                            // :484
        emit_labels(*blockmodel.get_memberships(best));  // :485
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 3;
    }
    return 0;
}
