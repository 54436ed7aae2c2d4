"""GPU tests of the block constraints (include/bisbm.h, "Block constraints").

Every sampler is held to what the header says of a node with a list of allowed blocks: the heat-bath sweeps to the host replay of
tests/test_gpu_heatbath.py with the row restricted (distributed.numpy_heatbath_choice(..., allowed=)), the pair reshuffles to the
host replay of tests/test_gpu_reshuffle.py over the members whose class allows both blocks, the MH sweeps to the oracle sweep by
sweep, the shuffle to the oracle's shuffle of every (type, class)'s compacted labels under the class's key, all of them together
to the exact distribution of the enumerable graph over its 240 admissible states.  Labels, counts and the block state are
integers; running sums and records are compared on bit patterns."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_gpu_heatbath import _assert_state_is_a_rebuild, _bits, _case, _model, _refused
from test_gpu_reshuffle import _Helper, _draw, _pair_of_move
from test_tempering import philox, u53

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed
syn = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")

pytestmark = pytest.mark.gpu

SEED = 21
FIRST_ID = 5
INF = float("inf")
CLASS_KEY = 0x9E3779B97F4A7C15


@pytest.fixture(autouse=True)
def _every_launch_keeps_its_own_sum(monkeypatch):
    """the unconstrained MH sweeps of these tests keep the sum of their own dS values (tests/test_gpu_heatbath.py does the same)"""
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


def _visit(gid, sweep, na, nb):
    L = O.lib()
    return [int(L.orc_philox_visit(SEED, gid, sweep, na, nb, i)) for i in range(na + nb)]


def _state(m, c):
    return (m.get_memberships(c), m.get_m(c), m.get_m_r(c), m.get_n_r(c), m.get_eta_rk_(c))


def _same_state(x, y):
    return all((u == v).all() for u, v in zip(x, y))


def _one_start(m, c):
    """every chain of `m` gets the labels of chain c (the counters and the Philox streams stay the chains' own), so that one
    table can admit all of them; returns the labels"""
    lab = m.get_memberships(c)
    m.set_memberships(lab)
    m.init_bisbm()
    return lab.astype(np.int64)


def _rows(ka, kb, *sets):
    """a table: class 0 allows everything, class i the blocks of sets[i - 1] of each type it names (a type it does not name: all)"""
    K = ka + kb
    out = [np.ones(K, dtype=bool)]
    for s in sets:
        s = sorted(s)
        row = np.ones(K, dtype=bool)
        if any(x < ka for x in s):
            row[:ka] = False
        if any(x >= ka for x in s):
            row[ka:] = False
        row[s] = True
        out.append(row)
    return np.array(out)


def _pair_rows(ka, kb):
    """class 1 + b: block b and the next block of its type"""
    return _rows(ka, kb, *([{b, (b + 1) % ka} for b in range(ka)] + [{ka + b, ka + (b + 1) % kb} for b in range(kb)]))


def _admissible(m, cls, allowed, na):
    ok = True
    for c in range(m.n_chains):
        lab = m.get_memberships(c)
        ok = ok and bool(allowed[cls, lab].all()) and bool((lab[:na] < m.KA).all()) and bool((lab[na:] >= m.KA).all())
    return ok


# ------------------------------------------------------------------------------------------------------- 1. heat bath
def _heatbath_replay(name, sweeps, make, beta=1.0, clamp=None):
    """chain 2 of a three-chain handle with first chain id 5, after a shuffle and three unconstrained MH sweeps, every chain set to
    chain 2's labels; make(visit order of the first replayed sweep, labels) -> (class_of_node, allowed).  The rows dS come from a
    one-chain helper's conditionals_last (the unrestricted row), the restricted P is built on the host with the device's exp and
    the choice is numpy_heatbath_choice(..., allowed=).  Returns a dict of what the callers assert their edge on."""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains, greedy = na + nb, 3, beta == INF
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    c, gid, sweep0 = chains - 1, FIRST_ID + chains - 1, 3
    lab = _one_start(m, c)
    first_order = _visit(gid, sweep0, na, nb)
    cls, allowed = make(first_order, lab.copy())
    cls, allowed = np.asarray(cls, dtype=np.uint8), np.asarray(allowed, dtype=bool)
    mask = np.zeros(n, dtype=bool) if clamp is None else np.asarray(clamp(first_order, lab.copy()), dtype=bool)
    if mask.any():
        m.clamp(mask)
    m.constrain(cls, allowed)
    got_cls, got_allowed = m.constraints()
    assert (got_cls == cls).all() and (got_allowed == allowed).all()
    start = lab.copy()
    cum, S0 = m.get_entropy()[c], m.entropy()[c]
    helper = _model(name, 1, labels=lab.astype(np.uint32))
    helper.conditionals_set(None, 1.0 if greedy else beta, keep_last=True)

    def sync():
        helper.set_memberships(lab.astype(np.uint32))
        helper.init_bisbm()
        helper.conditionals_accumulate()
    sync()
    if greedy:
        moved_gpu, sweeps_gpu = m.polish(sweeps)
    else:
        moved_gpu, sweeps_gpu = m.heatbath_sweeps(sweeps, beta), None
    seen = {"free": 0, "single": 0, "restricted": 0, "min_outside": 0, "second_chunk": 0, "zero_outside": 0, "unrestricted_rows": 0}
    moved, total, ran = 0, 0.0, 0
    for sw in range(sweeps):
        order = first_order if sw == 0 else _visit(gid, sweep0 + sw, na, nb)
        moved_before = moved
        for pos, v in enumerate(order):
            k_own, lo = (ka, 0) if v < na else (kb, ka)
            r = int(lab[v]) - lo
            A = allowed[cls[v], lo:lo + k_own].copy()
            assert A[r]
            free = k_own > 1 and int((lab == lab[v]).sum()) > 1 and not mask[v]
            seen["single"] += bool(free and A.sum() == 1)
            free = free and A.sum() > 1
            seen["free"] += free
            dS, P_all = (np.asarray(x[0][:k_own], dtype=np.float64) for x in helper.conditionals_last(v))
            P = P_all
            if free and not greedy:
                x = beta * (dS - dS[A].min())
                w = np.where((x > 700.0) | ~A, 0.0, m.debug_exp(-np.minimum(x, 700.0)))
                Z = 0.0
                for y in w:
                    Z = Z + float(y)
                P = w / Z
                if A.all():  # (the row of a node that is not restricted is the device's own row: the exponentials are the device's)
                    assert P.tobytes() == P_all.tobytes(), (v, P, P_all)
                    seen["unrestricted_rows"] += 1
                seen["zero_outside"] += bool((P[~A] == 0.0).all() and (~A).any())
            if free:
                seen["restricted"] += not A.all()
                seen["min_outside"] += bool(dS.min() < 0.0 and not A[int(np.argmin(dS))] and dS[A].min() > dS.min())
                seen["second_chunk"] += bool(k_own > 64 and A[64:].any() and not A.all())
            o = philox(SEED, gid, B.PHILOX_PURPOSE_HEATBATH, (sweep0 + sw) * n + pos)
            s = D.numpy_heatbath_choice(dS, P, r, free, u53(o[0], o[1]), greedy, allowed=A)
            assert A[s]
            if s != r:
                lab[v] = lo + s
                cum = cum + dS[s]
                total = total + dS[s]
                moved += 1
                sync()
        ran += 1
        if greedy and moved == moved_before:
            break
    assert seen["free"] > 0 and moved > 0, (seen, moved)
    got = m.get_memberships(c)
    assert (got[mask] == start[mask]).all()
    assert (got == lab).all(), np.flatnonzero(got != lab)
    assert int(moved_gpu[c]) == moved
    if greedy:
        assert int(sweeps_gpu[c]) == ran
    acc, sw_counts = m.last_counts()
    assert int(acc[c]) == moved and int(sw_counts[c]) == ran
    for x, y in zip(_state(m, c)[1:], _state(helper, 0)[1:]):
        assert (x == y).all()
    assert _bits(m.get_entropy()[c]) == _bits(cum)
    S1 = m.entropy()[c]
    print("%s beta %g: %d classes, %d moves in %d sweep(s), sum dS %.6f, S %.6f -> %.6f, %s" % (name, beta, len(allowed), moved, ran, total, S0, S1, seen))
    assert abs((S1 - S0) - total) <= 1e-9 * abs(S0)
    assert _admissible(m, cls, allowed, na)
    for other in range(chains - 1):  # (the other chains ran too: consistent, and inside their lists)
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    m.close()
    helper.close()
    seen.update(order=first_order, cls=cls, allowed=allowed, mask=mask, start=start)
    return seen


def test_heat_bath_sweeps_on_the_tiny_graph_with_two_classes_are_the_host_replay():
    """12 + 9 nodes, 3 + 2 blocks: class 1 allows the type-a blocks {0, 1} and the type-b block {3} alone (its type-b nodes are held)"""
    def make(order, lab):
        allowed = _rows(3, 2, {0, 1, 3})
        cls = np.where((np.arange(21) % 2 == 1) & allowed[1][lab], 1, 0)
        return cls, allowed
    seen = _heatbath_replay("tiny", 3, make)
    assert seen["restricted"] > 0 and seen["single"] > 0 and seen["zero_outside"] > 0 and seen["unrestricted_rows"] > 0


def _hub_outside(order, deg, na):
    """the type-a node of the highest degree that is not at the positions 64 .. 191"""
    taken = set(order[64:192])
    return max((v for v in range(na) if v not in taken), key=lambda v: deg[v])


def _chunk_classes(order, lab, na, nb, ka, kb, deg):
    """hubs_isolated: the classes 1 .. K allow one block each, the classes K + 1 .. 2K a block and the next of its type.  Positions
    64 .. 127 of the type-a phase hold one-block classes only, positions 128 .. 191 as well but for position 150; of the other
    nodes every second one may choose between two blocks; the hub is unrestricted."""
    K = ka + kb
    allowed = np.concatenate([_rows(ka, kb, *[{b} for b in range(K)]), _pair_rows(ka, kb)[1:]])
    cls = np.where(np.arange(na + nb) % 2 == 0, 1 + K + lab, 0)
    held = np.asarray(order[64:192])
    cls[held] = 1 + lab[held]
    cls[order[150]] = 0
    cls[_hub_outside(order, deg, na)] = 0
    return cls, allowed


def test_heat_bath_sweep_with_a_skipped_chunk_and_a_chunk_of_one_free_node_is_the_host_replay():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    deg = np.diff(rowptr.astype(np.int64))
    seen = _heatbath_replay(name, 1, lambda order, lab: _chunk_classes(order, lab, na, nb, ka, kb, deg))
    order, cls, allowed = seen["order"], seen["cls"], seen["allowed"]
    hub = _hub_outside(order, deg, na)
    one_block = allowed[cls][:, :ka].sum(axis=1) == 1  # (of the type-a blocks)
    assert all(v < na for v in order[:192])
    assert one_block[order[64:128]].all()
    assert int((~one_block[order[128:192]]).sum()) == 1 and not one_block[order[150]]
    assert deg[hub] > 64 and cls[hub] == 0
    assert seen["single"] >= 100 and seen["restricted"] > 0 and seen["unrestricted_rows"] > 0


def test_heat_bath_sweep_with_a_clamp_on_top_of_the_constraints_is_the_host_replay():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    seen = _heatbath_replay(name, 1, lambda order, lab: (np.where(np.arange(na + nb) % 2 == 0, 1 + lab, 0), _pair_rows(ka, kb)),
                            clamp=lambda order, lab: np.arange(na + nb) % 5 == 0)
    assert seen["restricted"] > 0 and seen["mask"].sum() == 100


def test_heat_bath_sweep_over_70_blocks_reaches_the_second_lane_chunk():
    """70 + 3 blocks: class 1 allows only the type-a blocks 64 .. 69, class 2 the blocks 60 .. 67 on both sides of lane chunk 64"""
    name = "wideK"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)

    def make(order, lab):
        allowed = _rows(ka, kb, set(range(64, 70)), set(range(60, 68)))
        cls = np.zeros(na + nb, dtype=np.int64)
        cls[allowed[2][lab] & (lab < ka)] = 2
        cls[allowed[1][lab] & (lab < ka) & (np.arange(na + nb) % 2 == 0)] = 1
        return cls, allowed
    seen = _heatbath_replay(name, 1, make)
    assert (seen["cls"] == 1).sum() > 3 and (seen["cls"] == 2).sum() > 3
    assert seen["second_chunk"] > 3 and seen["restricted"] > 6


def test_64_and_65_targets_under_constraints_are_the_host_replay():
    """64 type-a blocks (one full chunk of lanes) and 65 type-b blocks (a second chunk of one lane): class 1 allows the type-a blocks
    32 .. 63, class 2 the type-b blocks 62 .. 64 of the type, the last of which is the lane of the second chunk"""
    name = "hb_k64_k65"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)

    def make(order, lab):
        allowed = _rows(ka, kb, set(range(32, 64)), {ka + 62, ka + 63, ka + 64})
        cls = np.zeros(na + nb, dtype=np.int64)
        cls[allowed[1][lab] & (lab < ka)] = 1
        cls[allowed[2][lab] & (lab >= ka)] = 2
        return cls, allowed
    seen = _heatbath_replay(name, 1, make)
    assert (seen["cls"] == 1).sum() > 10 and (seen["cls"] == 2).sum() >= 3 and seen["second_chunk"] >= 1


def test_greedy_sweeps_under_constraints_take_the_lowest_allowed_minimum():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    seen = _heatbath_replay(name, 2, lambda order, lab: (np.where(np.arange(na + nb) % 2 == 0, 1 + lab, 0), _pair_rows(ka, kb)), beta=INF)
    assert seen["min_outside"] > 0  # (a node whose best block is not in its list was reached, and took the best of the list or stayed)


# -------------------------------------------------------------------------------------------------------- 2. polishing
def test_polish_settles_over_the_admissible_moves_and_leaves_inadmissible_downhill_moves():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    m = _model(name, 2)
    m.shuffle_bisbm()
    m.run_sweeps(1)
    lab = _one_start(m, 0)
    cls, allowed = 1 + lab, _pair_rows(ka, kb)
    m.constrain(cls, allowed)
    moved, sweeps = m.polish(100)
    assert (sweeps < 100).all() and (moved > 0).all()
    m.conditionals_set(None, 1.0, keep_last=True)
    m.conditionals_accumulate()
    for c in range(2):
        after = m.get_memberships(c).astype(np.int64)
        assert allowed[cls, after].all()
        free = np.bincount(after, minlength=ka + kb)[after] > 1
        kept_outside = 0
        for v in range(n):
            lo, k = (0, ka) if v < na else (ka, kb)
            dS = np.asarray(m.conditionals_last(v)[0][c][:k])
            A = allowed[cls[v], lo:lo + k]
            assert not (free[v] and (dS[A] < 0).any()), (c, v)
            kept_outside += bool(free[v] and (dS[~A] < 0).any())
        assert kept_outside > 0, c  # (the constraints are what holds them)
        _assert_state_is_a_rebuild(m, rowptr, col, c)
    m.close()


# ------------------------------------------------------------------------------------------------------- 3. reshuffles
def _reshuffle_replay(m, c, gid, name, moves, scans, beta, cls, allowed, mask=None):
    """tests/test_gpu_reshuffle.py::_replay_moves with the members filtered to the open nodes whose class allows both blocks of the
    pair; a move with fewer than two members is a counted no-op.  Returns per move (pair, M, original and launch labels)."""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    mask = np.zeros(na + nb, dtype=bool) if mask is None else mask
    lab = m.get_memberships(c).astype(np.int64)
    cum, S0 = m.get_entropy()[c], m.entropy()[c]
    j0 = int(m.reshuffles_total()[c])
    helper = _Helper(name, lab, beta)
    exp = lambda x: m.debug_exp([float(x)])[0]
    accepted_gpu = m.reshuffle(moves, scans, beta)
    got = m.reshuffle_last()[c]
    out, n_acc, total = [], 0, 0.0
    for j in range(j0, j0 + moves):
        t, rg, sg = _pair_of_move(SEED, gid, j, ka, kb)
        own0 = t * ka
        lo, hi = (na, na + nb) if t else (0, na)
        in_pair = [v for v in range(lo, hi) if lab[v] in (rg, sg)]
        members = [v for v in in_pair if not mask[v] and allowed[cls[v], rg] and allowed[cls[v], sg]]
        M, W = len(members), (len(members) + 127) >> 7
        last = j == j0 + moves - 1
        if M < 2:
            if last:
                assert (got["type"], got["r"], got["s"], got["M"]) == (t, rg, sg, M) and not got["accepted"]
                assert got["dS_fwd"] == 0.0 and got["dS_rev"] == 0.0 and got["A"] == 0.0 and got["u_acc"] == 0.0
            out.append({"pair": (t, rg, sg), "M": M, "in_pair": len(in_pair), "orig": lab[members].copy(), "launch": None, "accepted": False})
            continue
        orig = lab[members].copy()
        bits = [(_draw(SEED, gid, j, 2 + (i >> 7))[(i >> 5) & 3] >> (i & 31)) & 1 for i in range(M)]
        launch = np.asarray(D.numpy_reshuffle_launch(bits, rg, sg))
        lab[members] = launch

        def scan(scan_t=None, forced=None):
            factors, dsum = [], 0.0
            for i, v in enumerate(members):
                cur = int(lab[v])
                o = sg if cur == rg else rg
                free = int((lab == cur).sum()) > 1  # (the nodes of the block that are no members count)
                dS_o = helper.dS(lab, v, o - own0) if free else None
                if forced is None:
                    U = _draw(SEED, gid, j, 2 + W + scan_t * M + i)
                    to_r, f, dead = D.numpy_reshuffle_step(dS_o, cur == rg, free, beta, u=u53(U[0], U[1]), exp=exp)
                else:
                    to_r, f, dead = D.numpy_reshuffle_step(dS_o, cur == rg, free, beta, forced_to_r=int(forced[i]) == rg, exp=exp)
                if dead:
                    return factors, dsum, True
                factors.append(f)
                if (rg if to_r else sg) != cur:
                    lab[v] = rg if to_r else sg
                    dsum = dsum + dS_o
            return factors, dsum, False
        for s_t in range(scans):
            scan(scan_t=s_t)
        L = lab[members].copy()
        f_rev, dS_rev, dead = scan(forced=orig)
        lab[members] = orig
        q_rev = (0.0, 0) if dead else D.numpy_reshuffle_q(f_rev)
        if dead:
            dS_fwd, q_fwd, A, acc = 0.0, (0.0, 0), 0.0, False
        else:
            lab[members] = L
            f_fwd, dS_fwd, _ = scan(scan_t=scans)
            q_fwd = D.numpy_reshuffle_q(f_fwd)
            A, acc = D.numpy_reshuffle_accept(dS_fwd, dS_rev, q_fwd, q_rev, beta, 0.0)
        U = _draw(SEED, gid, j, 1)
        u_acc = u53(U[0], U[1])
        if last:
            assert (got["type"], got["r"], got["s"], got["M"]) == (t, rg, sg, M)
            assert got["u_acc"] == u_acc
            assert _bits(got["dS_fwd"]) == _bits(dS_fwd) and _bits(got["dS_rev"]) == _bits(dS_rev), (got, dS_fwd, dS_rev)
            assert got["q_fwd"][1] == q_fwd[1] and got["q_rev"][1] == q_rev[1], (got, q_fwd, q_rev)
            assert _bits(got["q_fwd"][0]) == _bits(q_fwd[0]) and _bits(got["q_rev"][0]) == _bits(q_rev[0]), (got, q_fwd, q_rev)
            assert got["A"] == A or abs(got["A"] - A) <= 1e-12 * abs(A), (got["A"], A)
            assert got["accepted"] == (u_acc < got["A"])
            acc = got["accepted"]
        else:
            acc = u_acc < A
        if acc:
            cum = cum + (dS_fwd - dS_rev)
            total = total + (dS_fwd - dS_rev)
            n_acc += 1
        else:
            lab[members] = orig
        out.append({"pair": (t, rg, sg), "M": M, "in_pair": len(in_pair), "orig": orig, "launch": launch, "accepted": bool(acc)})
    after = m.get_memberships(c)
    assert (after == lab).all()
    assert allowed[cls, after].all()
    assert int(accepted_gpu[c]) == n_acc
    assert int(m.reshuffles_total()[c]) == j0 + moves
    for got_x, want_x in zip(_state(m, c)[1:], helper.state(lab)):
        assert (got_x == want_x).all()
    assert _bits(m.get_entropy()[c]) == _bits(cum)
    S1 = m.entropy()[c]
    print("%s: %d move(s), %d scan(s): pairs %s, M %s of %s, accepted %d, sum dS %.6f" % (name, moves, scans, [x["pair"] for x in out], [x["M"] for x in out], [x["in_pair"] for x in out], n_acc, total))
    assert abs((S1 - S0) - total) <= 1e-9 * abs(S0)
    helper.m.close()
    return out


@pytest.mark.parametrize("name,moves,scans", [("tiny", 4, 1), ("hubs_isolated", 2, 3), ("wideK", 2, 2)])
def test_reshuffles_are_the_host_replay_over_the_filtered_members(name, moves, scans):
    """every third node is unrestricted, the others may sit in their block and the next of its type (wideK: 70 blocks of type a, the
    membership test of a pair reads the second and the third word of a class's row)"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains, c = 3, 2
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.shuffle_bisbm()
    m.run_sweeps(3)
    lab = _one_start(m, c)
    cls, allowed = np.where(np.arange(na + nb) % 3 == 0, 0, 1 + lab), _pair_rows(ka, kb)
    m.constrain(cls, allowed)
    out = _reshuffle_replay(m, c, FIRST_ID + c, name, moves, scans, 1.0, cls, allowed)
    assert any(x["M"] >= 2 for x in out)
    assert any(x["M"] < x["in_pair"] for x in out)  # (a node that may not sit in both sat in a chosen pair)
    assert _admissible(m, cls, allowed, na)
    for other in range(chains - 1):
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    m.close()


def _constructed(kind):
    """tiny, chain 2 of three with first id 5: the pair of the chain's move 0 is (r, s); class 1 allows every block but s, class 2
    every block but r.  "none": the nodes of r are of class 1 and those of s of class 2 -- nobody may sit in both; "one": as
    before but for one node of s; "block": the nodes of r are of class 1 and the nodes of s unrestricted -- r is held by
    nodes that are no members."""
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains, c = 3, 2
    gid = FIRST_ID + c
    t, rg, sg = _pair_of_move(SEED, gid, 0, ka, kb)
    lab = O.contiguous_labels(na, nb, ka, kb).astype(np.int64)
    allowed = np.ones((3, ka + kb), dtype=bool)
    allowed[1, sg] = False
    allowed[2, rg] = False
    cls = np.zeros(na + nb, dtype=np.int64)
    cls[lab == rg] = 1
    if kind != "block":
        cls[lab == sg] = 2
    if kind == "one":
        cls[np.flatnonzero(lab == sg)[0]] = 0
    m = _model(name, chains, first_chain_id=FIRST_ID, labels=lab.astype(np.uint32))
    m.init_bisbm()
    m.constrain(cls, allowed)
    before = _state(m, c), m.get_entropy()[c]
    out = _reshuffle_replay(m, c, gid, name, 1, 1, 1.0, cls, allowed)[0]
    assert out["pair"] == (t, rg, sg)
    return m, c, out, before, int((lab == rg).sum()), int((lab == sg).sum()), rg, sg


@pytest.mark.parametrize("kind,members", [("none", 0), ("one", 1)])
def test_a_pair_with_fewer_than_two_members_is_a_counted_no_op(kind, members):
    m, c, out, before, n_r, n_s, rg, sg = _constructed(kind)
    assert out["M"] == members and out["in_pair"] == n_r + n_s
    assert _same_state(_state(m, c), before[0]) and _bits(m.get_entropy()[c]) == _bits(before[1])
    assert int(m.reshuffles_total()[c]) == 1
    m.close()


def test_a_block_held_only_by_nodes_that_are_no_members_gets_members_from_the_launch():
    m, c, out, before, n_r, n_s, rg, sg = _constructed("block")
    assert out["M"] == n_s >= 2 and (out["orig"] == sg).all()
    assert (out["launch"] == rg).any() and (out["launch"] == sg).any()  # (the launch put a member into r)
    assert int((m.get_memberships(c) == rg).sum()) >= n_r  # (the nodes of r stayed)
    m.close()


# --------------------------------------------------------------------------------------------- 4. MH against the oracle
LOW_T = 0.3


def test_mh_sweeps_follow_the_oracle_up_to_its_first_move_out_of_a_list():
    """Sweep by sweep: the oracle, set to the device's labels, runs the unconstrained sweep; p* = the first position at which it
    put a node into a block outside the node's list.  Up to p* the device made the oracle's steps; in a sweep without a p* it made
    all of them, and accepted exactly as many (a refused proposal was not accepted by the oracle either)."""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains, c = na + nb, 3, 2
    gid = FIRST_ID + c
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.init_bisbm()
    base = 3
    m.run_sweeps(base)  # (unconstrained, from the contiguous labels: the chain is still settling when the constraints are set)
    lab = _one_start(m, c)
    rng = np.random.default_rng(4)
    listed = rng.random(n) < 0.06
    cls, allowed = np.where(listed, 1 + lab, 0), _pair_rows(ka, kb)
    m.constrain(cls, allowed)
    o = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, O.contiguous_labels(na, nb, ka, kb))
    o.seed_philox(SEED, gid)
    o.init_bisbm()
    o.anneal("constant", [1.0], base * n, 1 << 60)  # (the oracle's sweep counter follows the device's)
    assert (o.memberships() == m.get_memberships(c)).all()
    with_p, without_p = 0, 0
    for sweep in range(base, base + 50):
        T = 1.0 if sweep < base + 10 else LOW_T
        lab0 = m.get_memberships(c)
        S_before, cum_before = m.entropy()[c], m.get_entropy()[c]
        o.set_memberships(lab0)
        o.init_bisbm()
        m.run_sweeps(1, temperature=T)
        o.anneal("constant", [T], n, 1 << 60)
        lab_d, lab_o = m.get_memberships(c), o.memberships()
        order = _visit(gid, sweep, na, nb)
        p_star = next((p for p, v in enumerate(order) if not allowed[cls[v], lab_o[v]]), None)
        assert allowed[cls, lab_d].all(), sweep
        before = order[:p_star] if p_star is not None else order
        assert (lab_d[before] == lab_o[before]).all(), (sweep, p_star)
        acc_d, sw_d = (int(x[c]) for x in m.last_counts())
        assert sw_d == 1
        if p_star is None:
            without_p += 1
            assert (lab_d == lab_o).all(), sweep
            assert acc_d == o.last_accepted, (sweep, acc_d, o.last_accepted)
        else:
            with_p += 1
            assert lab_d[order[p_star]] == lab0[order[p_star]]  # (the refused step left the node where it was)
        _assert_state_is_a_rebuild(m, rowptr, col, c)
        S_after, cum_after = m.entropy()[c], m.get_entropy()[c]
        assert abs((cum_after - cum_before) - (S_after - S_before)) <= 1e-9 * abs(S_before), sweep
    print("MH under lists for %d nodes: %d sweeps with a p*, %d without" % (listed.sum(), with_p, without_p))
    assert with_p >= 5 and without_p >= 5, (with_p, without_p)
    assert _admissible(m, cls, allowed, na)
    for other in range(chains - 1):
        _assert_state_is_a_rebuild(m, rowptr, col, other)
    m.close()


# ------------------------------------------------------------------------------------------ 5. stationary distribution
ENUM_LISTS = {0: [0, 1], 1: [0, 1], 2: [1, 2], 3: [1, 2], 4: [0], 5: [2], 6: [3], 7: [4]}  # (nodes 8 .. 11 are free)
_ENUM = {}


def _code(labels):
    lab = np.asarray(labels).astype(np.int64)
    digits = np.concatenate([lab[:6], lab[6:] - 3])
    return int((digits * 3 ** np.arange(12)).sum())


def _enumeration():
    """the admissible states of the enumerable graph at 3 + 2 blocks without an empty block, and their S from the oracle"""
    if not _ENUM:
        rowptr, col = cases.enumerable_graph()
        na, nb = cases.ENUM_NA, cases.ENUM_NB
        o = O.OracleModel(rowptr, col, na, nb, 3, 2, cases.ENUM_EPS, O.contiguous_labels(na, nb, 3, 2))
        choices = [ENUM_LISTS.get(v, [3, 4]) for v in range(12)]
        states, S = [], []
        for idx in np.ndindex(*[len(ch) for ch in choices]):
            lab = np.array([choices[v][i] for v, i in enumerate(idx)], dtype=np.uint32)
            if (np.bincount(lab, minlength=5) == 0).any():
                continue
            o.set_memberships(lab)
            o.init_bisbm()
            states.append(_code(lab))
            S.append(o.entropy())
        assert len(states) == 240 == len(set(states))
        _ENUM["states"], _ENUM["S"] = np.array(states), np.array(S)
    return _ENUM["states"], _ENUM["S"]


@pytest.mark.parametrize("sampler,beta", [("mh", 1.0), ("mh", 5.0 / 3.0), ("heatbath", 1.0), ("reshuffle", 1.0)])
def test_constrained_chains_sample_the_target_over_the_admissible_states(sampler, beta):
    rowptr, col = cases.enumerable_graph()
    na, nb = cases.ENUM_NA, cases.ENUM_NB
    chains, moves = 8192, 400
    cls, allowed = B.constraints_from_lists(na + nb, 5, ENUM_LISTS, na=na, ka=3)
    start = B.admissible_start(na, nb, 3, 2, cls, allowed)
    g = B.BlockModel(start, syn.types_vector(na, nb), 5, 3, 2, cases.ENUM_EPS, (rowptr, col), n_chains=chains, rng="philox", seed=4242)
    g.constrain(cls, allowed)
    g.shuffle_bisbm()
    if sampler == "mh":
        g.run_sweeps(moves, temperature=1.0 / beta)
    elif sampler == "heatbath":
        g.heatbath_sweeps(moves, beta)
    else:
        g.reshuffle(moves, 1, beta)
    codes = np.array([_code(g.get_memberships(c)) for c in range(chains)])
    g.close()
    states, S = _enumeration()
    target = np.exp(-beta * (S - S.min()))
    stat, dof, p = cases.chi_square(codes, states, target / target.sum())  # (KeyError: a constraint was broken)
    flat = np.exp(-beta * (S - S.min()) / 1.25)
    p_flat = cases.chi_square(codes, states, flat / flat.sum())[2]
    print("%s under constraints, beta = %g: chi2 = %.1f on %d dof, p = %.3g; flattened target p = %.3g" % (sampler, beta, stat, dof, p, p_flat))
    assert p > 1e-3, (stat, dof, p)
    assert p_flat < 1e-6


# ------------------------------------------------------------------------------------------------------------ 6. shuffle
def test_the_shuffle_permutes_every_class_as_the_oracle_shuffles_its_compacted_labels():
    """300 + 200 nodes, three chains, a clamp on top.  Class c bans one block per type, so its nodes are picked among those that
    no chain holds there: class 1 has no open node (all clamped), class 2 one open type-a node, class 3 type-b nodes only, class 0
    more than 64 open nodes of each type.  The reference of every class is an edgeless oracle on the compacted labels, seeded with
    the class's key seed + c * 0x9E3779B97F4A7C15 mod 2^64."""
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains = na + nb, 3
    m = _model(name, chains, first_chain_id=FIRST_ID)
    m.shuffle_bisbm()
    m.run_sweeps(2)  # (every chain its own labels)
    start = [m.get_memberships(c).astype(np.int64) for c in range(chains)]
    allowed = np.ones((4, ka + kb), dtype=bool)
    for c in (1, 2, 3):
        allowed[c, (c - 1) % ka] = allowed[c, ka + (c - 1) % kb] = False
    fits = lambda c: np.flatnonzero(np.all([allowed[c, s] for s in start], axis=0))
    cls = np.zeros(n, dtype=np.int64)
    mask = np.random.default_rng(5).random(n) < 0.3
    ones = fits(1)
    cls[ones[ones < na][:6]] = 1
    mask[cls == 1] = True
    twos = [v for v in fits(2) if v < na and cls[v] == 0][:5]
    cls[twos] = 2
    mask[twos] = True
    mask[twos[2]] = False
    threes = [v for v in fits(3) if v >= na][:70]
    cls[threes] = 3
    mask[threes[::2]] = False
    assert len(threes) == 70
    m.clamp(mask)
    m.constrain(cls, allowed)
    segs = {}
    for t, lo, hi in ((0, 0, na), (1, na, n)):
        for c in range(4):
            segs[(t, c)] = lo + np.flatnonzero(~mask[lo:hi] & (cls[lo:hi] == c))
    sizes = {k: len(F) for k, F in segs.items()}
    assert sizes[(0, 1)] == 0 and sizes[(0, 2)] == 1 and sizes[(1, 2)] == 0 and sizes[(0, 0)] > 64 and sizes[(1, 0)] > 64 and sizes[(1, 3)] >= 35, sizes
    oracles = {}
    for ch in range(chains):
        for c in range(4):
            Fa, Fb = segs[(0, c)], segs[(1, c)]
            F = np.concatenate([Fa, Fb])
            if not len(F):
                continue
            edgeless = (np.zeros(len(F) + 1, dtype=np.uint64), np.zeros(1, dtype=np.uint32))
            o = O.OracleModel(edgeless[0], edgeless[1], len(Fa), len(Fb), ka, kb, eps, start[ch][F])
            o.seed_philox((SEED + c * CLASS_KEY) % (1 << 64), FIRST_ID + ch)
            o.shuffle_bisbm()  # (epoch 0: the handle's first shuffle above)
            o.set_memberships(start[ch][F])
            oracles[(ch, c)] = (o, F)
    for call in range(2):
        m.shuffle_bisbm()
        for ch in range(chains):
            got = m.get_memberships(ch)
            want = start[ch].copy()
            for c in range(4):
                if (ch, c) not in oracles:
                    continue
                o, F = oracles[(ch, c)]
                o.shuffle_bisbm()
                want[F] = o.memberships()
            assert (got[mask] == start[ch][mask]).all(), (call, ch)
            assert (got == want).all(), (call, ch, np.flatnonzero(got != want))
            assert allowed[cls, got].all()
            for t, lo, hi in ((0, 0, na), (1, na, n)):
                for c in range(4):  # block sizes are preserved class by class
                    sel = lo + np.flatnonzero(cls[lo:hi] == c)
                    assert (np.bincount(got[sel], minlength=ka + kb) == np.bincount(start[ch][sel], minlength=ka + kb)).all()
            _assert_state_is_a_rebuild(m, rowptr, col, ch)
        assert any((m.get_memberships(ch) != start[ch]).any() for ch in range(chains)), call
    m.close()


def test_one_class_of_many_nodes_is_the_clamped_and_the_unclamped_shuffle():
    """everybody is of class 0 but node 0, whose class 1 bans a block it is not in: alone in its segment it stays, as a clamped
    node does, and class 0 has the key of the plain shuffle -- the handle equals one on which node 0 is clamped instead"""
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    mask = np.arange(na + nb) % 4 == 1
    table = np.ones((2, ka + kb), dtype=bool)
    table[1, 1] = False
    cls = np.zeros(na + nb, dtype=np.uint8)
    cls[0] = 1
    for clamp in (False, True):
        a, b = _model(name, 3, first_chain_id=FIRST_ID), _model(name, 3, first_chain_id=FIRST_ID)
        held = mask.copy() if clamp else np.zeros(na + nb, dtype=bool)
        if clamp:
            a.clamp(held)
        a.constrain(cls, table)
        assert a.constraints()[0] is not None
        held[0] = True
        b.clamp(held)
        for call in range(2):
            a.shuffle_bisbm(), b.shuffle_bisbm()
            assert all(_same_state(_state(a, c), _state(b, c)) for c in range(3)), (clamp, call)
        if clamp:  # the list follows the clamp: cleared on a, and on b reduced to node 0, the two still agree
            a.unclamp()
            only = np.zeros(na + nb, dtype=bool)
            only[0] = True
            b.clamp(only)
            a.shuffle_bisbm(), b.shuffle_bisbm()
            assert all(_same_state(_state(a, c), _state(b, c)) for c in range(3))
        a.close(), b.close()


# ----------------------------------------------------------------------------------------------------------- 7. dispatch
def _three_calls(m):
    out = []
    m.run_sweeps(1)
    out.append(([m.get_memberships(c) for c in range(m.n_chains)], m.last_counts()[0].copy(), _bits(m.get_entropy()).copy()))
    moved = m.heatbath_sweeps(1, 1.0)
    out.append(([m.get_memberships(c) for c in range(m.n_chains)], moved, _bits(m.get_entropy()).copy()))
    acc = m.reshuffle(2, 1, 1.0)
    out.append(([m.get_memberships(c) for c in range(m.n_chains)], acc, _bits(m.get_entropy()).copy()))
    m.shuffle_bisbm()
    out.append(([m.get_memberships(c) for c in range(m.n_chains)], acc, _bits(m.get_entropy()).copy()))
    return out


def _half_lists(name):
    """every second node may sit in the block the contiguous start gives it and the next of its type"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    lab = O.contiguous_labels(na, nb, ka, kb).astype(np.int64)
    return np.where(np.arange(na + nb) % 2 == 0, 1 + lab, 0), _pair_rows(ka, kb)


def test_device_entries_behind_one_handle_give_one_handles_constrained_chains():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    cls, allowed = _half_lists(name)
    runs = []
    for kw in ({}, {"devices": [0, 0, 0]}):
        m = _model(name, 6, first_chain_id=3, **kw)
        m.init_bisbm()
        m.constrain(cls, allowed)
        got = m.constraints()
        assert (got[0] == cls).all() and (got[1] == allowed).all()
        runs.append(_three_calls(m))
        assert _admissible(m, cls, allowed, na)
        m.close()
    for (l1, n1, s1), (l2, n2, s2) in zip(*runs):
        assert all((x == y).all() for x, y in zip(l1, l2)) and (n1 == n2).all() and (s1 == s2).all()


def test_a_refusal_on_one_device_entry_leaves_the_constraints_in_place_on_all():
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    cls, allowed = _half_lists(name)
    m = _model(name, 6, first_chain_id=3, devices=[0, 0, 0])
    m.init_bisbm()
    m.constrain(cls, allowed)
    lab = m.get_memberships(5).astype(np.int64)
    assert allowed[0].all() and cls[1] == 0 and lab[1] != 2
    lab[1] = 2  # (an unrestricted node of the last chain, on the last entry, into another block)
    m.set_memberships(lab.astype(np.uint32), chain=5)
    m.init_bisbm()
    tight = _rows(ka, kb, *[{b} for b in range(ka + kb)])  # (every node in the block of the contiguous start)
    msg = _refused(lambda: m.constrain(1 + O.contiguous_labels(na, nb, ka, kb).astype(np.int64), tight), B.BISBM_ERR_STATE)
    assert "chain 8" in msg and "node 1 " in msg and "block 2" in msg, msg
    got = m.constraints()
    assert (got[0] == cls).all() and (got[1] == allowed).all()
    a = _three_calls(m)
    m.close()
    one = _model(name, 6, first_chain_id=3)
    one.init_bisbm()
    one.constrain(cls, allowed)
    one.set_memberships(lab.astype(np.uint32), chain=5)
    one.init_bisbm()
    for (l1, n1, s1), (l2, n2, s2) in zip(a, _three_calls(one)):
        assert all((x == y).all() for x, y in zip(l1, l2)) and (n1 == n2).all() and (s1 == s2).all()
    one.close()


def test_replica_exchange_rounds_under_constraints_are_the_one_chain_handles():
    """the construction of tests/test_gpu_tempered_moves.py on southernWomen: 4 chains as 2 ensembles of 2 rungs, 3 rounds of {1 MH
    sweep, 1 heat-bath sweep, 1 reshuffle}, every chain against the one-chain handle of its global id with the same constraints,
    run through the same calls at the temperature tempering_get reported"""
    rowptr, col, na, nb = O.load_graph("southernWomen")
    ka = kb = 3
    lab0 = O.contiguous_labels(na, nb, ka, kb).astype(np.int64)
    cls, allowed = np.where(np.arange(na + nb) % 2 == 0, 1 + lab0, 0), _pair_rows(ka, kb)
    ladder, chains, first = [1.0, 1.5], 4, 4

    def model(n_chains, first_id):
        m = B.BlockModel(lab0.astype(np.uint32), syn.types_vector(na, nb), ka + kb, ka, kb, 0.001, (rowptr, col), n_chains=n_chains, seed=SEED,
                         first_chain_id=first_id)
        m.init_bisbm()
        m.constrain(cls, allowed)
        m.shuffle_bisbm()
        return m
    m = model(chains, first)
    ones = [model(1, first + c) for c in range(chains)]
    for c, one in enumerate(ones):
        assert _same_state(_state(m, c), _state(one, 0))
    m.set_tempering(ladder)
    changed_rung = False
    for r in range(3):
        T_now = m.tempering_state()[1]
        m.tempering_rounds(1, mh=1, heatbath=1, reshuffles=1, scans=1)
        for c, one in enumerate(ones):
            T = float(T_now[c])
            changed_rung = changed_rung or T != float(np.float32(ladder[c % 2]))
            one.run_sweeps(1, temperature=T)
            one.heatbath_sweeps(1, 1.0 / T)
            one.reshuffle(1, 1, 1.0 / T)
            assert _same_state(_state(m, c), _state(one, 0)), (r, c)
            assert _bits(m.get_entropy())[c] == _bits(one.get_entropy())[0], (r, c)
    assert _admissible(m, cls, allowed, na)
    print("replica exchange under constraints: a chain ran a round off its first rung: %s" % changed_rung)
    for x in ones + [m]:
        x.close()


def test_the_slots_of_a_resampling_step_are_admissible():
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    chains = 16
    cls, allowed = _half_lists(name)
    m = _model(name, chains)
    m.init_bisbm()
    m.constrain(cls, allowed)
    m.shuffle_bisbm()
    m.run_sweeps(2)
    labels = [m.get_memberships(c) for c in range(chains)]
    S = m.entropy()
    parent, _ = m.population_resample(1.0, 1.0 + 1.0 / S.std())
    assert len(set(parent.tolist())) < chains  # (some slot took another chain's state)
    for c in range(chains):
        assert (m.get_memberships(c) == labels[int(parent[c])]).all(), c
    m.heatbath_sweeps(1, 1.0)
    m.run_sweeps(1)
    m.reshuffle(1, 1, 1.0)
    assert _admissible(m, cls, allowed, na)
    m.close()


# ----------------------------------------------------------------------------------------------------------- 8. clearing
@pytest.mark.parametrize("how", ["unconstrain", "all_allowing"])
def test_cleared_constraints_leave_the_handle_of_one_that_never_had_any(how):
    name = "hubs_isolated"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, chains = na + nb, 3
    cls, allowed = _half_lists(name)
    a = _model(name, chains, first_chain_id=FIRST_ID)
    a.init_bisbm()
    a.constrain(cls, allowed)
    a.shuffle_bisbm()
    a.run_sweeps(1)
    if how == "unconstrain":
        a.unconstrain()
    else:  # every class allows every block of some type, and the nodes are of that type
        table = np.ones((2, ka + kb), dtype=bool)
        table[0, ka:] = False
        table[1, :ka] = False
        a.constrain((np.arange(n) >= na).astype(np.uint8), table)
    assert a.constraints() == (None, None)
    b = _model(name, chains, first_chain_id=FIRST_ID)
    b.shuffle_bisbm()   # (the shuffle epoch of a)
    b.run_sweeps(1)     # (... and its sweep counter)
    for c in range(chains):
        b.set_memberships(a.get_memberships(c), chain=c)
    b.init_bisbm()
    cum_a, cum_b = a.get_entropy(), b.get_entropy()

    def step(m, base):
        out = []
        m.run_sweeps(2)
        out.append((m.last_counts()[0].copy(), m.last_pass_steps()))
        out.append(m.heatbath_sweeps(1, 1.0))
        out.append(m.reshuffle(2, 1, 1.0))
        rec = [{k: (_bits(v).tolist() if isinstance(v, float) else v) for k, v in x.items()} for x in m.reshuffle_last()]
        m.shuffle_bisbm()
        return out, rec, [_state(m, c) for c in range(chains)], _bits(m.get_entropy() - base)
    ra, rb = step(a, cum_a), step(b, cum_b)
    assert ra[0][0][1] == rb[0][0][1] and ra[0][0][1] > 1  # (the production kernel runs again: more than one step per pass)
    for x, y in zip(ra[0], rb[0]):
        assert (np.asarray(x[0] if isinstance(x, tuple) else x) == np.asarray(y[0] if isinstance(y, tuple) else y)).all()
    assert ra[1] == rb[1]
    assert all(_same_state(x, y) for x, y in zip(ra[2], rb[2]))
    a.close()
    b.close()


# ----------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_and_the_round_trip():
    name = "tiny"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n = na + nb
    cls, allowed = _half_lists(name)
    m = _model(name, 2, first_chain_id=FIRST_ID)
    m.init_bisbm()
    k = B.C.c_uint32(99)
    assert B.lib().bisbm_constraints_get(m._h, B.C.byref(k), None, None) == B.BISBM_OK and k.value == 0
    assert m.constraints() == (None, None)
    m.constrain(cls, allowed.astype(np.uint8) * 7)  # (any non-zero byte)
    got = m.constraints()
    assert got[0].dtype == np.uint8 and (got[0] == cls).all() and got[1].dtype == bool and (got[1] == allowed).all()
    assert B.lib().bisbm_constraints_get(m._h, B.C.byref(k), None, None) == B.BISBM_OK and k.value == len(allowed)
    assert B.lib().bisbm_constraints_get(m._h, None, None, None) == B.BISBM_OK
    state = [_state(m, c) for c in range(2)]
    # a label outside its list: chain 1 (global id 6) gets node 4 -- of a class -- moved to a block its class bans
    lab = m.get_memberships(1).astype(np.int64)
    assert cls[4] != 0
    banned = int(np.flatnonzero(~allowed[cls[4], :ka])[0])
    bad = lab.copy()
    bad[4] = banned
    msg = _refused(lambda: m.set_memberships(bad.astype(np.uint32), chain=1), B.BISBM_ERR_INVALID_ARG)
    assert "node 4" in msg and "label %d" % banned in msg, msg
    assert all(_same_state(_state(m, c), state[c]) for c in range(2))
    m.unconstrain()
    m.set_memberships(bad.astype(np.uint32), chain=1)
    m.init_bisbm()
    msg = _refused(lambda: m.constrain(cls, allowed), B.BISBM_ERR_STATE)
    assert "chain %d" % (FIRST_ID + 1) in msg and "node 4" in msg and "block %d" % banned in msg, msg
    assert m.constraints() == (None, None)
    m.set_memberships(lab.astype(np.uint32), chain=1)
    m.init_bisbm()
    m.constrain(cls, allowed)
    # ... and with constraints in place a refused set keeps them
    tight = _rows(ka, kb, *[{b} for b in range(ka + kb)])
    moved = m.get_memberships(0).astype(np.int64)
    assert cls[1] == 0
    moved[1] = (moved[1] + 1) % ka
    m.set_memberships(moved.astype(np.uint32), chain=0)
    m.init_bisbm()
    msg = _refused(lambda: m.constrain(1 + O.contiguous_labels(na, nb, ka, kb).astype(np.int64), tight), B.BISBM_ERR_STATE)
    assert "chain %d" % FIRST_ID in msg and "node 1 " in msg, msg
    got = m.constraints()
    assert (got[0] == cls).all() and (got[1] == allowed).all()
    # arguments
    assert "class" in _refused(lambda: B.BlockModel._check(m, B.lib().bisbm_constraints_set(
        m._h, 2, B._p(np.full(n, 2, dtype=np.uint8), B._u8p), B._p(np.ones(2 * (ka + kb), dtype=np.uint8), B._u8p))), B.BISBM_ERR_INVALID_ARG)
    assert "256" in _refused(lambda: B.BlockModel._check(m, B.lib().bisbm_constraints_set(
        m._h, 257, B._p(np.zeros(n, dtype=np.uint8), B._u8p), B._p(np.ones(257 * (ka + kb), dtype=np.uint8), B._u8p))), B.BISBM_ERR_INVALID_ARG)
    for bad_call in (lambda: m.constrain(cls[:-1], allowed), lambda: m.constrain(cls, allowed[:, :-1]), lambda: m.constrain(cls + 40, allowed),
                     lambda: m.constrain(cls.astype(np.float64), allowed)):
        with pytest.raises(ValueError):
            bad_call()
    got = m.constraints()
    assert (got[0] == cls).all() and (got[1] == allowed).all()
    # merges
    state = [_state(m, c) for c in range(2)]
    assert "bisbm_constraints_set(h, 0, NULL, NULL)" in _refused(lambda: m.agg_merge(1, 0), B.BISBM_ERR_STATE)
    assert "bisbm_constraints_set(h, 0, NULL, NULL)" in _refused(lambda: m.agg_merge(1), B.BISBM_ERR_STATE)
    assert all(_same_state(_state(m, c), state[c]) for c in range(2)) and m.ka_kb(0) == (ka, kb)
    m.unconstrain()
    m.agg_merge(1, 0)  # (allowed again)
    assert m.ka_kb(0) == (ka - 1, kb)
    m.close()
    compat = _model(name, 2, rng="mt19937-compat")
    compat.init_bisbm()
    assert "MT19937" in _refused(lambda: compat.constrain(cls, allowed), B.BISBM_ERR_UNSUPPORTED)
    assert compat.constraints() == (None, None)
    compat.close()
    wide = _model("wide_labels", 2)
    wide.init_bisbm()
    (_, _), wna, wnb, wka, wkb, _ = _case("wide_labels")
    table = np.ones((1, wka + wkb), dtype=bool)
    table[0, 0] = False
    assert "byte labels" in _refused(lambda: wide.constrain(np.zeros(wna + wnb, dtype=np.uint8), table), B.BISBM_ERR_UNSUPPORTED)
    assert wide.constraints() == (None, None)
    wide.close()
    from test_gpu_pair_scores import _merge_until_mixed, _mixed_shapes_model
    g, deg, gna, gnb = _mixed_shapes_model()
    _merge_until_mixed(g)
    assert len({g.ka_kb(c) for c in range(g.n_chains)}) > 1
    labels = [g.get_memberships(c) for c in range(g.n_chains)]
    assert "block counts" in _refused(lambda: g.constrain(np.zeros(g.n, dtype=np.uint8), np.ones((1, g.K), dtype=bool)), B.BISBM_ERR_STATE)
    assert all((x == g.get_memberships(c)).all() for c, x in enumerate(labels))
    g.close()


# --------------------------------------------------------------------------------------------- 10. the CLI and marginalize
def test_the_command_line_keeps_the_listed_nodes_inside_their_lists(tmp_path):
    rowptr, col, na, nb = O.load_graph("n_1000")
    n = na + nb
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    # a membership file that is deliberately NOT the planted partition at the listed nodes: they sit one block further, and their
    # lists hold that block and the one after it -- never the planted one
    planted = O.contiguous_labels(na, nb, 4, 6).astype(np.int64)
    listed = np.arange(7, n, 20)
    nxt = lambda b: np.where(b < 4, (b + 1) % 4, 4 + (b - 4 + 1) % 6)
    labels = planted.copy()
    labels[listed] = nxt(planted[listed])
    lists = {int(v): [int(labels[v]), int(nxt(labels[v]))] for v in listed}
    mb, cn = tmp_path / "labels.txt", tmp_path / "constraints.txt"
    mb.write_text("".join("%d\n" % x for x in labels))
    cn.write_text("".join("%d %d %d\n" % (v, lists[v][1], lists[v][0]) for v in reversed(sorted(lists))) + "%d %d %d\n" % (listed[0], *lists[int(listed[0])]))
    base = [cli, "-e", el, "-y", str(na), str(nb), "-z", "4", "6", "--membership_path", str(mb), "-d", "5", "--rng", "philox", "--chains", "4",
            "-b", str(3 * n), "-t", str(4 * n), "-f", str(2 * n), "--marginalize"]
    r = subprocess.run(base + ["--constraints", str(cn)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "constraints: %d of %d nodes listed, 11 class(es)" % (len(listed), n) in r.stderr, r.stderr
    out = np.array(r.stdout.split(), dtype=np.int64)
    assert len(out) == n and all(out[v] in lists[int(v)] for v in listed)
    free = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert free.returncode == 0, free.stderr
    free_out = np.array(free.stdout.split(), dtype=np.int64)
    assert any(free_out[v] not in lists[int(v)] for v in listed)  # (without the lists they go back to the planted block)
    cn.write_text("3 1 0\n1000 4\n")
    bad = subprocess.run(base + ["--constraints", str(cn)], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 1 and "'1000'" in bad.stderr and bad.stdout == ""
    cn.write_text("3 1 2\n")  # (node 3 sits in block 0 of the membership file)
    bad = subprocess.run(base + ["--constraints", str(cn)], capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "node 3" in bad.stderr and bad.stdout == "", (bad.returncode, bad.stderr)


def test_marginalize_sets_the_constraints_before_the_burn_in():
    rowptr, col, na, nb = O.load_graph("n_1000")
    n, chains = na + nb, 8
    planted = O.contiguous_labels(na, nb, 4, 6).astype(np.int64)
    cls, allowed = np.where(np.arange(n) % 20 == 0, 1 + planted, 0), _pair_rows(4, 6)
    for kw in ({}, {"sampler": "heatbath"}, {"reshuffles": 1}, {"tempering": [1.0, 1.3], "rung_moves": {"mh": 1, "heatbath": 1, "reshuffles": 1}}):
        m = B.BlockModel(planted, syn.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=chains, seed=5)
        m.init_bisbm()
        labels, counts = B.marginalize(m, 2, 2, 1, constraints=(cls, allowed), **kw)[:2]
        assert (m.constraints()[0] == cls).all() and allowed[cls, labels].all(), kw
        assert _admissible(m, cls, allowed, na), kw
        m.close()
    m = B.BlockModel(planted, syn.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=chains, seed=5)
    m.init_bisbm()
    out = B.marginalize_modes(m, 1, 2, 1, threshold=0.5, constraints=(cls, allowed))
    assert _admissible(m, cls, allowed, na) and out["labels"].shape[1] == n
    m.close()
    m = B.BlockModel(planted, syn.types_vector(na, nb), 10, 4, 6, 1.0, (rowptr, col), n_chains=chains, seed=5)
    m.init_bisbm()
    m.constrain(cls, allowed)
    res = B.population_anneal(m, [2.0, 1.5, 1.0], 1, rung_moves={"mh": 1, "heatbath": 1, "reshuffles": 1})
    assert _admissible(m, cls, allowed, na) and len(res["log_ratio"]) == 2
    m.close()


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "constrained_refinement.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "coarse" in r.stdout and "constrained refit" in r.stdout and "every node inside its parent's children: True" in r.stdout, r.stdout
