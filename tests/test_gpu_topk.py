"""GPU tests of the one top-k selection behind bisbm_query_scores_topk, bisbm_coassign_topk and bisbm_foldin_topk (both row
kinds): small graphs whose rows tie heavily, every k around the 256 candidates one step of the compaction holds, and the chunk
walk of the host driver forced onto small chunks with BISBM_TOPK_CHUNK_CELLS.

The model of every result is distributed.numpy_query_topk applied to the rows *_get_row returns, with the exclusions of the call
(the query's own node, its neighbours, the listed nodes); nodes are compared with `==`, values on their bit patterns.  The test
also PROVES from the rows, on the host, that its inputs hold the cases it is there for (COVER below): a case that no input
produces fails test_the_inputs_hold_every_case."""
import functools
import importlib

import numpy as np
import pytest

import oracle_lib as O

B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
REC, SIM = B.FOLDIN_RECOMMEND, B.FOLDIN_SIMILAR
KS = (1, 255, 256, 257, B.QUERY_MAX_K)
STRETCH = 256  # candidates one step of the ordered compaction takes
ENTRIES = ("query", "coassign", "foldin_rec", "foldin_sim")
# name: na, nb, ka, kb, chains.  "star": one type-b node that is every type-a node's only neighbour.
GRAPHS = {"257+256": (257, 256, 3, 2, 1), "1025+255": (1025, 255, 2, 3, 4), "903+3": (903, 3, 3, 2, 2), "star": (300, 1, 2, 1, 4)}
CHUNK_GRAPH, CHUNK_CELLS = "1025+255", 600  # a row of 1025 cells is longer than the cap; two rows of 255 fit under it
# what every entry point must meet somewhere in GRAPHS: (a) a tie at the k-th place over more than one stretch, (b) fewer
# eligible candidates than k, (c) no eligible candidate with / without a mask, (d) the candidate counts, (e) the query list
COUNTS = {1, 255, 256, 257, 1025}
COVER = {"query": {"a", "b", "c_mask", "e"}, "coassign": {"a", "b", "c_nomask", "e"}, "foldin_rec": {"a", "b", "c_mask", "e"},
         "foldin_sim": {"a", "b", "e"}}


def _graph(name):
    """few edges per node (every node of "star" has its one), so degrees -- and with them scores -- repeat"""
    na, nb = GRAPHS[name][:2]
    rng = np.random.default_rng(len(name) + na)
    if name == "star":
        a, b = np.arange(na), np.full(na, na)
    else:
        a = np.concatenate([np.arange(na), rng.integers(0, na, nb + na // 2)])
        b = na + np.concatenate([rng.integers(0, nb, na), np.arange(nb), rng.integers(0, nb, na // 2)])
    return B.edge_to_adj((a.astype(np.uint64), b.astype(np.uint64)), na + nb)


def _queries(na, nb):
    """11 queries, the types interleaved (and two neighbours of either type, for a chunk of two short rows), node 5 twice"""
    q = np.array([0, na, 5, na + nb - 1, na - 1, na + nb // 2, 5, 17, na + min(1, nb - 1), na, na // 2])
    assert len(q) == 11 and ((q[:-1] < na) != (q[1:] < na)).sum() >= 8 and (q == 5).sum() == 2
    return q


def _virtual_nodes(na, nb):
    """11 virtual nodes, the types interleaved as those of _queries, node 2 given again as node 6; lists of 1 to 300 entries
    with repeats"""
    rng = np.random.default_rng(na + nb)
    nodes = []
    for i, size in enumerate([1, 2, 8, 3, 300, 1, 0, 5, 2, 40, 1]):
        if "abababaabba"[i] == "a":
            nodes.append(("a", (na + rng.integers(0, nb, size)).tolist()))
        else:
            nodes.append(("b", rng.integers(0, na, size).tolist()))
    nodes[6] = ("a", list(nodes[2][1]))
    types = [t for t, _ in nodes]
    assert len(nodes) == 11 and all(x != y for x, y in zip(types[:5], types[1:6]))
    return nodes


def _chunks(lengths, cap):
    """the chunk walk of the host driver over rows of the given lengths: whole queries while they fit, never less than one"""
    out, q0 = [], 0
    while q0 < len(lengths):
        q1 = q0 + 1
        while q1 < len(lengths) and sum(lengths[q0:q1 + 1]) <= cap:
            q1 += 1
        out.append(lengths[q0:q1])
        q0 = q1
    return out


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _check(call, rows, firsts, excluded, masked, cover):
    """call(k) == numpy_query_topk of every row for every k of KS; the cases met go to `cover`.  Returns the raw results."""
    raw = []
    for k in KS:
        nodes, vals, terms = call(k)
        assert nodes.shape == vals.shape == (len(rows), k) and terms > 0
        raw.append((nodes.copy(), _bits(vals).copy()))
        for i, row in enumerate(rows):
            excl = np.unique(np.asarray(excluded[i], dtype=np.int64))
            assert ((excl >= 0) & (excl < len(row))).all()
            idx, val = D.numpy_query_topk(row.astype(np.float64), k, excl)
            want = np.where(idx == NONE, NONE, idx.astype(np.int64) + firsts[i]).astype(np.uint32)
            assert (nodes[i] == want).all(), (k, i, nodes[i], want)
            assert (_bits(vals[i]) == _bits(val.astype(vals.dtype))).all(), (k, i)
            cover.add(("count", len(row)))
            eligible = np.setdiff1d(np.arange(len(row)), excl)
            if len(eligible) < k:
                assert (nodes[i, len(eligible):] == NONE).all() and (vals[i, len(eligible):] == 0).all()
                cover.add("b")
            if len(eligible) == 0:
                cover.add("c_mask" if masked else "c_nomask")
            if len(eligible) > k:
                kth = row[idx[k - 1]]
                tied = eligible[row[eligible] == kth]
                taken = np.isin(tied, idx).sum()
                if taken < len(tied) and len(np.unique(tied // STRETCH)) > 1:
                    cover.add("a")
    return raw


@functools.lru_cache(maxsize=None)
def _case(name, devices=None, chunk_cells=None):
    """Every top-k call on one graph checked against the rows; returns ({entry point: cases met}, {call: raw results}, the row
    lengths per entry point).  chunk_cells: the value of BISBM_TOPK_CHUNK_CELLS the caller has set (part of the cache key)."""
    na, nb, ka, kb, chains = GRAPHS[name]
    rowptr, col = _graph(name)
    kw = {"devices": list(devices)} if devices else {}
    chains = max(chains, len(devices or ()))  # (every device entry runs a chain)
    m = B.BlockModel(O.contiguous_labels(na, nb, ka, kb), syn.types_vector(na, nb), ka + kb, ka, kb, 1.0, (rowptr, col),
                     n_chains=chains, seed=11, **kw)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    queries, vnodes = _queries(na, nb), _virtual_nodes(na, nb)
    cover = {e: {"e"} for e in ENTRIES}  # (e) is what _queries / _virtual_nodes assert
    raw, lengths = {}, {}

    m.query_scores_set(queries)
    m.query_scores_accumulate()
    rows = [m.query_scores(i)[0] for i in range(len(queries))]
    firsts = [na if q < na else 0 for q in queries]
    lengths["query"] = [len(r) for r in rows]
    for excl in (False, True):
        nbrs = [np.unique(col[int(rowptr[q]):int(rowptr[q + 1])].astype(np.int64)) - f if excl else [] for q, f in zip(queries, firsts)]
        raw["query", excl] = _check(lambda k: m.query_topk(k, exclude_edges=excl), rows, firsts, nbrs, excl, cover["query"])

    m.coassign_set(queries)
    m.coassign_accumulate()
    rows = [m.coassignment(i)[0] for i in range(len(queries))]
    firsts = [0 if q < na else na for q in queries]
    lengths["coassign"] = [len(r) for r in rows]
    assert all(r.dtype == np.uint32 for r in rows)
    raw["coassign"] = _check(m.coassign_topk, rows, firsts, [[q - f] for q, f in zip(queries, firsts)], False, cover["coassign"])

    m.foldin_set(vnodes, 0.25)
    m.foldin_accumulate()
    for what, entry in ((REC, "foldin_rec"), (SIM, "foldin_sim")):
        rows = [m.foldin_scores(i, what)[0] for i in range(len(vnodes))]
        firsts = [na if (t == "a") == (what == REC) else 0 for t, _ in vnodes]
        lengths[entry] = [len(r) for r in rows]
        for excl in ((False, True) if what == REC else (False,)):
            listed = [np.unique(np.asarray(ids, dtype=np.int64)) - f if excl else [] for (_, ids), f in zip(vnodes, firsts)]
            raw[entry, excl] = _check(lambda k: m.foldin_topk(what, k, exclude_listed=excl), rows, firsts, listed, excl, cover[entry])
    m.close()
    return cover, raw, lengths


@pytest.mark.parametrize("name", list(GRAPHS))
def test_topk_is_the_host_ranking_of_the_rows(name, monkeypatch):
    monkeypatch.delenv("BISBM_TOPK_CHUNK_CELLS", raising=False)
    _case(name)


def test_the_inputs_hold_every_case(monkeypatch):
    monkeypatch.delenv("BISBM_TOPK_CHUNK_CELLS", raising=False)
    met = {e: set() for e in ENTRIES}
    for name in GRAPHS:
        for e, cases in _case(name)[0].items():
            met[e] |= cases
    for e in ENTRIES:
        missing = (COVER[e] | {("count", c) for c in COUNTS}) - met[e]
        assert not missing, (e, sorted(map(str, missing)))


def _same_results(a, b):
    assert a.keys() == b.keys()
    for key in a:
        for (n0, v0), (n1, v1) in zip(a[key], b[key]):
            assert (n0 == n1).all() and (v0 == v1).all(), key


@pytest.mark.parametrize("name", list(GRAPHS))
def test_a_device_listed_twice(name, monkeypatch):
    monkeypatch.delenv("BISBM_TOPK_CHUNK_CELLS", raising=False)
    _case(name, devices=(0, 0))


@pytest.mark.parametrize("devices", [None, (0, 0)])
def test_small_chunks_select_the_same(devices, monkeypatch):
    """the 11 queries in at least three chunks, one of them a single query whose row is longer than the cap: the same bits.

    What this does NOT prove is that a second chunk ran: the chunking asserted here is this file's own statement of the walk
    (_chunks), and nothing the C ABI returns tells how the library walked.  A library that ignored the variable (or misread its
    value) would pass as well.  With the variable read, the test is what keeps the chunk offsets (rows from cell off[q0] on,
    results at q0 * k, the other devices' rows from the same cell) from going wrong unnoticed."""
    monkeypatch.delenv("BISBM_TOPK_CHUNK_CELLS", raising=False)
    _, whole, lengths = _case(CHUNK_GRAPH, devices)
    for entry in ENTRIES:
        chunks = _chunks(lengths[entry], CHUNK_CELLS)
        assert len(chunks) >= 3 and any(len(c) == 1 and c[0] > CHUNK_CELLS for c in chunks) and any(len(c) > 1 for c in chunks), (entry, chunks)
    monkeypatch.setenv("BISBM_TOPK_CHUNK_CELLS", str(CHUNK_CELLS))
    _, chunked, _ = _case(CHUNK_GRAPH, devices, CHUNK_CELLS)
    _same_results(whole, chunked)
