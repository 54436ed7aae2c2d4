"""Seeded graphs shared by the CPU and the GPU test modules (no GPU, no product code: numpy + the oracle's CSR)."""
import importlib

import numpy as np

import oracle_lib as O

SYN = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")


def random_graph(seed, na, nb, ne, ka, kb, hubs=0, isolated=0):
    a, b = SYN.planted_edges(na - isolated, nb - isolated, ne, max(ka, 1), max(kb, 1), seed=seed)
    b = b - (na - isolated) + na  # keep b ids in [na, na+nb-isolated)
    if hubs:  # a few nodes with degree ~150 (several rounds of the feeder's walk); hubs == 1: one node with degree > 255
        rng = np.random.default_rng(seed + 100)
        n_hub_edges = 150 * hubs if hubs > 1 else 600
        ha = rng.integers(0, hubs, n_hub_edges).astype(np.uint64)
        hb = (na + rng.integers(0, nb - isolated, n_hub_edges)).astype(np.uint64)
        a, b = np.concatenate([a, ha]), np.concatenate([b, hb])
    rowptr, col = O.edge_to_csr(a, b, na + nb)
    return rowptr, col


def unequal_groups_graph(seed, sizes_a, sizes_b, mean_degree):
    """Planted groups of unequal sizes (block i of type a goes with block i of type b; both lists have the same length): per
    edge, a is uniform over the type-a nodes, the block of b is a's with probability 0.8 and otherwise uniform over the blocks,
    and b is uniform inside its block.  (na + nb) * mean_degree / 2 edges, multi-edges kept.  Returns (rowptr, col), na, nb."""
    sizes_a, sizes_b = np.asarray(sizes_a, dtype=np.int64), np.asarray(sizes_b, dtype=np.int64)
    na, nb, k = int(sizes_a.sum()), int(sizes_b.sum()), len(sizes_a)
    ne = (na + nb) * mean_degree // 2
    rng = np.random.default_rng(seed)
    a = rng.integers(0, na, ne)
    block_a = np.searchsorted(np.cumsum(sizes_a), a, side="right")
    block_b = np.where(rng.random(ne) < 0.8, block_a, rng.integers(0, k, ne))
    first_b = np.concatenate([[0], np.cumsum(sizes_b)[:-1]])
    b = na + first_b[block_b] + (rng.random(ne) * sizes_b[block_b]).astype(np.int64)
    return O.edge_to_csr(a.astype(np.uint64), b.astype(np.uint64), na + nb), na, nb


CASES = [
    # name, na, nb, edges, ka, kb, eps, hubs, isolated
    ("tiny", 12, 9, 40, 3, 2, 0.5, 0, 0),
    ("ka1", 40, 30, 300, 1, 4, 1.0, 0, 0),
    ("hubs_isolated", 300, 200, 3000, 5, 7, 1.0, 3, 4),
    ("huge_hub", 300, 200, 3000, 5, 7, 1.0, 1, 0),    # degree > 255: beyond the byte counters of the feeder's walk
    ("wideK", 400, 300, 6000, 70, 3, 2.0, 0, 0),       # K_type > 64: chunked lane loops
    # KA + KB > 256: the library's wide mode (two-byte labels, m read and updated in HBM) -- where a --merge run starts
    ("wide_labels", 400, 300, 6000, 200, 150, 1.0, 2, 0),
    ("big_m_r", 150, 150, 60000, 2, 3, 1.0, 0, 0),     # m_r > 10^4: log_q_approx on the device
    # production kernel's hot step: m_r > 10^4 and k / sqrt(n) > 18 (closed-form log_q tier), K <= 32 ...
    ("direct_tier", 20000, 20000, 100000, 2, 2, 1.0, 0, 0),
    # ... both block counts > 32 (six-level scans and sums) with every m_r <= 10^4: the K > 32 path on the q TABLE ...
    ("direct_tier_wide", 72000, 72000, 216000, 40, 33, 1.0, 0, 0),
    # ... both block counts > 32 in the closed-form tier (blocks of ~3000 nodes, m_r ~ 2 x 10^4, k / sqrt(n) ~ 22) ...
    ("direct_tier_k40", 120000, 120000, 720000, 40, 33, 1.0, 0, 0),
    # ... k / sqrt(n) around 23: the closed-form tier as well (the name is of the time the tier began at 24)
    ("mid_tier", 5300, 5300, 26500, 2, 2, 1.0, 0, 0),
    # ... k / sqrt(n) around 10 (blocks of ~1200 nodes): the converged log_q tier in the hot step
    ("mid_tier_low", 2400, 2400, 28800, 2, 2, 1.0, 0, 0),
    # ... k / sqrt(n) around 15.5 (blocks of 1900 nodes, m_r ~ 15000): log_q_closed2 in every block, 13 <= u <= 18
    ("closed2_tier", 3800, 3800, 30000, 2, 2, 1.0, 0, 0),
    # ... and a dense graph (mean degree 40, blocks of 1000 nodes): k / sqrt(n) around 5, the low converged tier
    ("dense_low_tier", 2000, 2000, 80000, 2, 2, 1.0, 0, 0),
    # K = 32 + 32 with a hub of degree 600: eta (64 x 601 words) does not fit the LDS budget and stays in HBM while the
    # K <= 32 kernel evaluates two steps per pass
    ("k32_eta_in_hbm", 3000, 3000, 60000, 32, 32, 1.0, 1, 0),
    # the same for the four- and eight-steps-per-pass variants (both block counts <= 16, <= 8)
    ("k16_eta_in_hbm", 3000, 3000, 60000, 16, 13, 1.0, 1, 0),
    ("k8_eta_in_hbm", 3000, 3000, 60000, 8, 7, 1.0, 1, 0),
    # ... and the one-step-per-pass variant (a block count above 32) with eta outside the LDS (a window of it inside)
    ("k64_eta_in_hbm", 3000, 3000, 60000, 50, 64, 1.0, 1, 0),
    # epsilon = 0 (legal in the reference: -E 0): no uniform component in the proposal, denominators m_r[t] alone
    ("eps0", 300, 200, 3000, 5, 7, 0.0, 0, 4),
    ("eps0_direct", 20000, 20000, 100000, 2, 2, 0.0, 0, 0),
    # no edges at all: every node has degree 0 (uniform proposals over all K blocks, blockmodel.cc:616-617)
    ("edgeless", 10, 8, 0, 2, 2, 1.0, 0, 0),
]
CASE = {c[0]: c for c in CASES}

# The log_q tier every block of a case reaches after shuffle_bisbm, for the cases whose name or comment claims one
# (tests/test_oracle.py guards this, so that a case drifting into another tier fails instead of passing vacuously).
CASE_TIERS = {"big_m_r": "literal", "direct_tier": "closed", "direct_tier_wide": "table", "direct_tier_k40": "closed",
              "mid_tier": "closed", "mid_tier_low": "mid", "dense_low_tier": "low", "eps0_direct": "closed", "closed2_tier": "closed2"}

# Shapes of the heat-bath replays alone (tests/test_gpu_heatbath.py; the layout of CASES, graphs from random_graph(11, ...)): the
# lane-chunk edges of heatbath_kernel.  They stay out of CASES, so the GPU-vs-oracle matrix does not grow by them.
HEATBATH_CASES = {c[0]: c for c in [
    # 64 targets in phase a (one full chunk of lanes), 65 in phase b (a second chunk of one lane); eta in LDS
    ("hb_k64_k65", 400, 400, 4000, 64, 65, 1.0, 0, 0),
    # 130 targets in phase a: three chunks of lanes
    ("hb_k130", 400, 400, 4000, 130, 3, 1.0, 0, 0),
    # 100 type-b blocks and a type-a hub of degree ~610: a non-zero list longer than one wave; eta in HBM
    ("hb_long_list", 300, 200, 3000, 3, 100, 1.0, 1, 0),
    # 10 + 10 blocks and the hub: eta in HBM with few rows, so the entries of r and s are rewritten and re-read often
    ("hb_eta_in_hbm", 300, 200, 3000, 10, 10, 1.0, 1, 0),
]}

# Shapes of the held MH sweeps above 64 blocks of a type alone (tests/test_gpu_held_wide.py, pinned on the host by
# tests/test_oracle_holds.py; the layout of CASES, graphs from random_graph(11, ...)): there the generic kernel is the only MH route.
# The smallest shapes that reach each edge; outside CASES, so the GPU-vs-oracle matrix does not grow by them.
HELD_WIDE_CASES = {c[0]: c for c in [
    # 70 type-a blocks: the proposal's inverse CDF of type a walks two chunks of lanes
    ("held_k70_k3", 400, 300, 6000, 70, 3, 2.0, 0, 0),
    # 130 type-b blocks: three chunks; words 0 to 4 of a constraint row; isolated nodes (uniform proposals over 133 blocks)
    ("held_k3_k130", 300, 400, 6000, 3, 130, 1.0, 0, 4),
    # 256 blocks, the limit of byte labels: bit 31 of word 7; type b in three chunks, the last of one lane
    ("held_k127_k129", 400, 400, 6000, 127, 129, 1.0, 2, 0),
    # a hub of degree above 600 beside 103 blocks: eta stays outside LDS in the generic kernel
    ("held_k3_k100_hub", 300, 400, 4000, 3, 100, 1.0, 1, 0),
]}

# ------------------------------------------------------------------ row shapes (tests/test_row_shapes.py, tests/test_gpu_row_shapes.py)
# The production sweep kernel's edges along the length and the make-up of an adjacency row (kRowCap = 255, byte k_v counters, ids
# read four at a time and sixteen a round, the eta window).  Outside CASES, so the GPU-vs-oracle matrix does not grow by them.
ROW_LADDER = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 254, 255, 256, 257, 300)
ROW_ISOLATED = 2  # rows of no entries per type, as random_graph makes them
ROW_BAND = tuple(range(128, 192, 4))  # 20 + 27, sparse graph: rows of 128 .. 188 entries in one block, side by side in the ids (below)
ROW_BALLAST = 8   # rows of 250 entries per type in the dense graphs: with them more rows lie in a window that ends at 255 than in one that ends below
# id: na, nb, ka, kb, graph seed, the last rows of col[] in the sparse and in the dense graph, the dense graph's plain degrees.
# The dense graph exists where the production kernel keeps a window of eta in LDS (every shape but 8 + 7): its plain degrees are
# chosen so that the window, which is placed where most nodes are, ends at 255.
ROW_SHAPES = {
    "8+7": (331, 299, 8, 7, 41, "255", None, None),
    "16+13": (601, 549, 16, 13, 42, "1", "3", (36, 44)),
    "20+27": (843, 811, 20, 27, 43, "3", "255", (160, 230)),
    "40+33": (1211, 1109, 40, 33, 44, "1", "255", (140, 200)),
    "64+50": (1223, 1217, 64, 50, 45, "3", "255", (212, 228)),
}


def _matched_edges(rng, ids_a, deg_a, block_a, ids_b, deg_b, block_b, ka, kb, p_in):
    """Edges between two node lists with exactly the given degrees (the sums are equal): every stub of a type-a node asks for a
    type-b block -- the partner a_block * kb // ka of its own with probability p_in, else a uniform one -- and gets a stub of it
    while the block has one; the stubs left over on both sides are paired at random.  Multi-edges are kept."""
    pa, pb = rng.permutation(int(deg_a.sum())), rng.permutation(int(deg_b.sum()))
    sa, own = np.repeat(ids_a, deg_a)[pa], np.repeat(block_a, deg_a)[pa]
    want = np.where(rng.random(len(sa)) < p_in, own * kb // ka, rng.integers(0, kb, len(sa)))
    sb, sb_blk = np.repeat(ids_b, deg_b)[pb], np.repeat(block_b, deg_b)[pb]
    out_b = np.full(len(sa), -1, dtype=np.int64)
    left = []
    for t in range(kb):
        asks, has = np.flatnonzero(want == t), sb[sb_blk == t]
        k = min(len(asks), len(has))
        out_b[asks[:k]] = has[:k]
        left.append(has[k:])
    rest = np.flatnonzero(out_b < 0)
    out_b[rest] = rng.permutation(np.concatenate(left))
    return sa.astype(np.uint64), out_b.astype(np.uint64)


def row_shape_graph(sid, dense=False):
    """The graph of a row of ROW_SHAPES.  Plain nodes form a planted graph with prescribed degrees (1 + Poisson(5): mean about 6;
    dense: uniform over the shape's range); every special node of one type lies apart from the others (all but the band) and its edges go to plain
    nodes of the other type only, so it keeps its degree exactly:
      * the ladder: one node of every degree of ROW_LADDER (dense: up to 255), to uniform plain nodes;
      * concentrated rows, whose neighbours are dealt out over the plain nodes of planted blocks of the other type (local block
        numbers): "one_block" 255 entries in the other type's last block, "half" 128 entries in block 2, "split" 128 + 127 in
        blocks 4 and 5, which share a word of the kernel's byte counters, and "copies": the type-a node and the type-b node of this
        name share one edge 255 times (the one special row whose neighbour is no plain node);
      * 20 + 27, sparse graph: the band, one row of every length of ROW_BAND with all its entries in block 3, at the end of each type's
        ids: bytes with the top bit set and every pattern of the bits below it, in rows that the sweep's visit order (local in the
        ids) often puts into one pass -- under the planted labels a mover with 128 .. 188 edges in a column is followed within the
        pass by a step that reads that column;
      * ROW_ISOLATED rows of no entries, and in the dense graph ROW_BALLAST rows of 250 entries to uniform plain nodes;
      * type b ends with a row of 1, 3 or 255 entries ("255": behind a row of 2), the last row of col[].
    Returns dict(rowptr, col, labels, na, nb, ka, kb, special={type: {name: node}}, ladder=the degrees)."""
    na, nb, ka, kb, seed, end_sparse, end_dense, plain_range = ROW_SHAPES[sid]
    end = end_dense if dense else end_sparse
    rng = np.random.default_rng(seed + (500 if dense else 0))
    ladder = tuple(d for d in ROW_LADDER if d <= 255 or not dense)
    labels = O.contiguous_labels(na, nb, ka, kb).astype(np.int64)
    names = ["ladder%d" % d for d in ladder] + ["one_block", "half", "split", "copies"] + ["isolated%d" % i for i in range(ROW_ISOLATED)]
    names += ["ballast%d" % i for i in range(ROW_BALLAST if dense else 0)]
    band = ROW_BAND if sid == "20+27" and not dense else ()
    special, plain = {}, {}
    for t, (first, size) in enumerate(((0, na), (na, nb))):
        tail = ["band%d" % d for d in band] + {"a": [], "1": ["end"], "3": ["end"], "255": ["before_end", "end"]}["a" if t == 0 else end]
        spread = size - len(tail) - 1
        order = rng.permutation(len(names))  # (which special sits where: no run of the ladder along the ids)
        special[t] = {names[j]: first + 1 + (i * spread) // len(names) for i, j in enumerate(order)}
        for i, name in enumerate(tail):
            special[t][name] = first + size - len(tail) + i
        assert len(set(special[t].values())) == len(special[t])
        plain[t] = np.setdiff1d(np.arange(first, first + size), np.array(list(special[t].values())))
    deg = {}
    for t in (0, 1):
        if dense:
            deg[t] = rng.integers(plain_range[0], plain_range[1] + 1, len(plain[t]))
        else:
            deg[t] = 1 + rng.poisson(5.0, len(plain[t]))
    diff = int(deg[0].sum() - deg[1].sum())  # the two sums made equal on the longer side, one edge a node
    t_fix = 1 if diff > 0 else 0
    deg[t_fix] = deg[t_fix] + abs(diff) // len(deg[t_fix]) + (np.arange(len(deg[t_fix])) < abs(diff) % len(deg[t_fix]))
    a, b = _matched_edges(rng, plain[0], deg[0], labels[plain[0]], plain[1], deg[1], labels[plain[1]] - ka, ka, kb, 0.8)
    ea, eb = [a], [b]

    def add(node, others):
        others = np.asarray(others, dtype=np.uint64)
        mine = np.full(len(others), node, dtype=np.uint64)
        ea.append(mine if node < na else others)
        eb.append(others if node < na else mine)

    for t in (0, 1):
        oth, k_oth, base_oth = plain[1 - t], (kb, ka)[t], (ka, 0)[t]
        in_block = lambda blk: oth[labels[oth] - base_oth == blk]
        deal = lambda blk, count: np.resize(rng.permutation(in_block(blk)), count)
        for d in ladder:
            add(special[t]["ladder%d" % d], rng.choice(oth, d))
        for i in range(ROW_BALLAST if dense else 0):
            add(special[t]["ballast%d" % i], rng.choice(oth, 250))
        for d in band:
            add(special[t]["band%d" % d], deal(3, d))
        add(special[t]["one_block"], deal(k_oth - 1, 255))
        add(special[t]["half"], deal(2, 128))
        add(special[t]["split"], np.concatenate([deal(4, 128), deal(5, 127)]))
        if "end" in special[t]:
            add(special[t]["end"], rng.choice(oth, int(end)))
        if "before_end" in special[t]:
            add(special[t]["before_end"], rng.choice(oth, 2))
    add(special[0]["copies"], np.full(255, special[1]["copies"]))
    rowptr, col = O.edge_to_csr(np.concatenate(ea), np.concatenate(eb), na + nb)
    return dict(rowptr=rowptr, col=col, labels=labels.astype(np.uint32), na=na, nb=nb, ka=ka, kb=kb, special=special, ladder=ladder,
                end=end, dense=dense)


def row_shape_rows(g):
    """[(type, name, node, degree)] of the ladder, the concentrated rows and the last rows of col[] of a row-shape graph: the rows the tests ask about"""
    out = []
    for t in (0, 1):
        for name, v in sorted(g["special"][t].items(), key=lambda kv: kv[1]):
            if not name.startswith(("isolated", "ballast", "band")):
                out.append((t, name, v, int(g["rowptr"][v + 1] - g["rowptr"][v])))
    return out


def row_k_v(g, v, labels=None):
    """k_v of node v in numpy: how many entries of its row lie in every block of the other type"""
    labels = g["labels"] if labels is None else labels
    k_oth, base = (g["kb"], g["ka"]) if v < g["na"] else (g["ka"], 0)
    row = g["col"][int(g["rowptr"][v]):int(g["rowptr"][v + 1])]
    return np.bincount(np.asarray(labels)[row].astype(np.int64) - base, minlength=k_oth)


LOG_Q_TIERS = ("table", "closed", "closed2", "mid", "low", "literal")


def log_q_tiers(m_r, n_r):
    """The tier in which the Philox-mode log_q(n = m_r, k = n_r) is evaluated (bisbm_device.hpp log_q / log_q_approx<true>,
    and the hot step's hot_log_q in bisbm_sweep_fast.hip), per block: n <= 10^4 the q table; k^4 < n the small-k sum; else by
    u^2 = k^2 / n with k = min(k, n): > 18^2 log_q_closed, [13^2, 18^2] log_q_closed2, [8^2, 13^2) log_q_mid, [2.5^2, 8^2)
    log_q_low, below the literal series ("literal" covers the small-k sum as well).  The same exact integer tests."""
    n = np.asarray(m_r, dtype=np.int64)
    k = np.minimum(np.asarray(n_r, dtype=np.int64), n)
    k2 = k * k
    return np.select([n <= 10000, (k < 256) & (k2 * k2 < n), k2 > 324 * n, k2 >= 169 * n, k2 >= 64 * n, 4 * k2 >= 25 * n],
                     ["table", "literal", "closed", "closed2", "mid", "low"], "literal")


def tier_counts(m_r, n_r):
    t = log_q_tiers(m_r, n_r)
    return {name: int((t == name).sum()) for name in LOG_Q_TIERS}


# ------------------------------------------------------------------ a graph small enough to enumerate
# 6 + 6 nodes, two planted groups per type (a0-a2 ~ b0-b2, a3-a5 ~ b3-b5) plus two bridging edges and one
# double edge; K = 2 + 2.  State space: 2^6 x 2^6 label vectors, of which (2^6 - 2)^2 = 3844 have no empty block
# (apply_mcmc_moves never empties a block, blockmodel.cc:467-471).
ENUM_NA = ENUM_NB = 6
ENUM_EDGES = [(0, 6), (0, 7), (1, 6), (1, 8), (2, 7), (2, 8), (2, 6), (3, 9), (3, 10), (4, 9), (4, 11), (5, 10),
              (5, 11), (5, 9), (1, 9), (4, 7), (0, 6)]
ENUM_EPS = 1.0


def enumerable_graph():
    a = np.array([e[0] for e in ENUM_EDGES], dtype=np.uint64)
    b = np.array([e[1] for e in ENUM_EDGES], dtype=np.uint64)
    rowptr, col = O.edge_to_csr(a, b, ENUM_NA + ENUM_NB)
    return rowptr, col


def enumerable_states():
    """All label vectors of the enumerable graph with four non-empty blocks, and exp(-S) normalised, S = entropy()
    (blockmodel.cc:753-787) from the oracle: the stationary distribution of the reference's chain at T = 1."""
    rowptr, col = enumerable_graph()
    na, nb = ENUM_NA, ENUM_NB
    o = O.OracleModel(rowptr, col, na, nb, 2, 2, ENUM_EPS, O.contiguous_labels(na, nb, 2, 2))
    states, S = [], []
    for x in range(1, 2 ** na - 1):
        la = [(x >> i) & 1 for i in range(na)]
        for y in range(1, 2 ** nb - 1):
            lab = np.array(la + [2 + ((y >> i) & 1) for i in range(nb)], dtype=np.uint32)
            o.set_memberships(lab)
            o.init_bisbm()
            states.append(state_code(lab))
            S.append(o.entropy())
    S = np.array(S)
    w = np.exp(-(S - S.min()))
    return np.array(states), w / w.sum(), S


def state_code(labels):
    """12 labels -> integer (bit i = second block of the node's type)."""
    lab = np.asarray(labels).astype(np.int64)
    bits = np.concatenate([lab[:ENUM_NA], lab[ENUM_NA:] - 2])
    return int((bits << np.arange(len(bits))).sum())


def chi_square(codes, states, prob, min_expected=8.0):
    """Pearson chi-square of sampled state codes against `prob` over `states`; states with an expected count below
    min_expected are pooled into one bin.  Returns (statistic, dof, p_value)."""
    from scipy import stats
    n = len(codes)
    index = {int(s): i for i, s in enumerate(states)}
    obs = np.zeros(len(states))
    for c in codes:
        obs[index[int(c)]] += 1  # KeyError = a state with an empty block was reached
    exp = prob * n
    big = exp >= min_expected
    o = np.concatenate([obs[big], [obs[~big].sum()]])
    e = np.concatenate([exp[big], [exp[~big].sum()]])
    if e[-1] < min_expected:  # fold a thin tail into the smallest regular bin
        j = int(np.argmin(e[:-1]))
        o[j] += o[-1]
        e[j] += e[-1]
        o, e = o[:-1], e[:-1]
    stat = float(((o - e) ** 2 / e).sum())
    dof = len(e) - 1
    return stat, dof, float(stats.chi2.sf(stat, dof))
