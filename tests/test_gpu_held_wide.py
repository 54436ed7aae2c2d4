"""GPU tests of held Metropolis-Hastings sweeps above 64 blocks of a type against the held oracle.

Above 64 blocks of a type the generic kernel (sweep_kernel<RNG_PHILOX>, csrc/bisbm_kernels.hip) is the only MH route: estimate mode,
and every handle on its way down from a merge.  tests/test_gpu_held_oracle.py stops at 50 + 64 blocks, where BISBM_FORCE_GENERIC=1
runs that kernel at shapes the production kernel serves too.  The shapes here (cases.HELD_WIDE_CASES) are the smallest that reach
what runs above 64 only, or first meets a hold there: a barred target found in the second or third chunk of the proposal's inverse
CDF (70, 129, 130 blocks of a type), words 4 to 7 of a class's row of the constraint table and bit 31 of word 7 (block 255), the
field row at strides up to 256, the clamp path with eta outside LDS at more than 64 blocks, and the constrained shuffle's bisection
over 512 segments.

The matrix is test_gpu_held_oracle.test_every_held_call_is_the_held_oracles on these shapes, with its helpers: three chains, first
chain id 5, one oracle per chain, the nine calls of _call_list; after every call and per chain labels, m, m_r, n_r, eta, both
columns of last_counts() and the return value are the oracle's, the running sum passes sum_dS_close, under fields its advance is
that of S + Phi, clamped labels stay and every label is inside its list.  Nothing is forced: there is one route, and it is asserted
(one step per pass; ROUTE_HELD / ROUTE_FIELDS as the hold has it; ROUTE_PRODUCTION clear).

The conditions on the inputs -- the margin, the vacuity guards, labels that reach the last block, bit 255 both set and clear in the
table of the 256-block shape, a cooling call that one chain leaves early and another does not -- are asserted on the oracle's side
before the device is touched (matrix_inputs, early_stop_inputs); tests/test_oracle_holds.py walks the same functions over every
case on the host, so a case that drifts fails there first.

What the oracles give under SEED (pytest -s prints it): smallest margin; steps of clamped nodes / barred targets / accepted moves /
decisions the field turned, over the nine calls and three chains.
  held_k70_k3       clamp 1.6e-4; 12660/0/8930/0      constraints 9.0e-6; 0/13505/9813/0   both 4.0e-4; 12660/9294/6480/0
                    fields 6.4e-4; 0/0/14853/3648     all 6.8e-6; 12660/9365/6326/2156
  held_k3_k130      clamp 1.4e-3; 12660/0/7868/0      constraints 1.7e-3; 0/14006/8001/0   both 8.3e-4; 12660/9671/5479/0
                    fields 6.2e-4; 0/0/13004/1712     all 1.4e-3; 12660/9742/5480/782
  held_k127_k129    clamp 5.6e-4; 14280/0/3653/0      constraints 5.0e-3; 0/12571/3561/0   both 1.7e-4; 14280/8842/2549/0
                    fields 2.1e-3; 0/0/5375/1020      all 4.2e-4; 14280/8902/2543/444
  held_k3_k100_hub  clamp 8.2e-5; 12660/0/8672/0      constraints 7.7e-4; 0/14010/9764/0   both 4.9e-4; 12660/9810/6401/0
                    fields 2.6e-5; 0/0/14587/2493     all 4.2e-5; 12660/9842/6151/1057
The eta plan the device reports: held_k70_k3 (1, 0, 0, 0), eta in LDS; the other three (0, 0, 0, 0) -- eta alone has 226, 179 and
248 KiB there.  A case takes 0.05 to 0.4 s on the device."""
import importlib

import numpy as np
import pytest

import cases
import oracle_lib as O
import test_gpu_held_oracle as H
from test_gpu_constraints import CLASS_KEY
from test_gpu_heatbath import _assert_state_is_a_rebuild, _case, _model
from test_gpu_held_oracle import HOLDS, SEED, _assert_inputs, _call_list, _device, _reference, _run, _tables
from test_gpu_held_fast import CHAINS, ENV, FIRST_ID

B = importlib.import_module("bipartitesbm-mcmc_amd")

pytestmark = pytest.mark.gpu

NAMES = list(cases.HELD_WIDE_CASES)
# (name, hold) -> the Philox seed of the case where SEED fails a condition on the inputs.  No matrix case does; under SEED the
# early-stop case of held_k3_k100_hub ends its cooling call after [2, 3, 2] sweeps -- every chain early, none runs to the end
SEEDS = {("held_k3_k100_hub", "early stop"): 22}
# the cooling call with steps_await = n // 16, under "all": the sweeps the three oracles ran when the case was written (printed
# beside what they run now; the condition is that one chain stops early and one does not)
EARLY_STOP_SWEEPS = {"held_k70_k3": [2, 4, 4], "held_k3_k130": [4, 1, 4], "held_k127_k129": [4, 3, 4], "held_k3_k100_hub": [4, 3, 4]}
LDS_BUDGET = 40 * 1024  # (bisbm_anneal.hip's LDS plan: eta goes to LDS when the chain state with it stays within 160 KiB / 4)


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")


# ------------------------------------------------------------------------------------------------------------------ lists
def strided_lists(name, seed=3):
    """test_gpu_held_fast._half_lists finds no admissible start at these block counts (its 40 classes of about ten nodes are dealt
    round-robin over the lowest allowed blocks, and the high blocks stay empty).  Here: a tenth of each type unlisted (class 0); the
    i-th listed node gets the blocks b with b mod 4 in {i mod 4, i mod 4 + 1} of its type (below four blocks: all but one), so that
    four classes of a hundred nodes each cover every block; three nodes per type get a single block, five of the wider type the
    first and the last block of it.  Returns (class_of_node, allowed, start labels)."""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    rng = np.random.default_rng(seed)
    lists = {}
    for lo, cnt, b0, k in ((0, na, 0, ka), (na, nb, ka, kb)):
        listed = np.flatnonzero(rng.random(cnt) >= 0.1)
        for i, v in enumerate(listed):
            j = i % 4
            lists[lo + int(v)] = ([b0 + b for b in range(k) if b % 4 in (j, (j + 1) % 4)] if k >= 4
                                  else [b0 + b for b in range(k) if b != j % k])
        for v in rng.choice(cnt, size=3, replace=False):
            lists[lo + int(v)] = [b0 + int(rng.integers(k))]
    lo, cnt, b0, k = (0, na, 0, ka) if ka >= kb else (na, nb, ka, kb)
    for v in rng.choice(cnt, size=5, replace=False):
        lists[lo + int(v)] = [b0, b0 + k - 1]
    cls, allowed = B.constraints_from_lists(na + nb, ka + kb, lists, na=na, ka=ka)
    return cls, allowed, B.admissible_start(na, nb, ka, kb, cls, allowed)


def _wide_tables(name, hold):
    """test_gpu_held_oracle._tables with the lists of these shapes in its cache: the 30 % clamp of default_rng(77) and the field of
    random_field(default_rng(79), n, K) are that file's"""
    if name not in H._LISTS:
        H._LISTS[name] = strided_lists(name)
    return _tables(name, hold)


# ----------------------------------------------------------------------------------------- the oracles' side of the cases
_REF = {}  # (one entry at a time, as in test_gpu_held_oracle.py)


def matrix_reference(name, hold):
    key = ("matrix", name, hold)
    if key not in _REF:
        (rowptr, col), na, nb, ka, kb, eps = _case(name)
        _REF.clear()
        t = _wide_tables(name, hold)
        calls = _call_list(na + nb)
        _REF[key] = (t, calls) + _reference(name, t, SEEDS.get((name, hold), SEED), calls)
    return _REF[key]


def matrix_inputs(name, hold):
    """the conditions on the inputs of a matrix case, asserted on the oracles alone; returns (t, calls, start, ref)"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    K = ka + kb
    t, calls, start, ref = matrix_reference(name, hold)
    _assert_inputs((name, hold), t, ref)
    for c in range(CHAINS):  # the labels the oracles hold after the calls reach the last block of the shape
        assert int(ref[-1]["chains"][c]["state"][0].max()) == K - 1, (name, hold, c)
    if t["cn"] is not None:
        cls, allowed = t["cn"]
        for c in range(CHAINS):  # (the start is admissible, and so is what the oracle made of it)
            assert allowed[cls, start[c]].all() and allowed[cls, ref[-1]["chains"][c]["state"][0]].all(), (name, hold, c)
        if name == "held_k127_k129":  # bit 31 of word 7, set in one class's row and clear in another's, and a node in block 255
            assert K == 256 and allowed[:, 255].any() and not allowed[:, 255].all(), (name, hold)
            assert any((start[c] == 255).any() or (ref[-1]["chains"][c]["state"][0] == 255).any() for c in range(CHAINS)), (name, hold)
        words = {int(s) >> 5 for s in range(K) if not allowed[:, s].all()}  # the words of a row in which some class bars a block
        assert words == set(range((K + 31) >> 5)), (name, hold, sorted(words))
    return t, calls, start, ref


def early_stop_reference(name):
    key = ("early stop", name)
    if key not in _REF:
        (rowptr, col), na, nb, ka, kb, eps = _case(name)
        n = na + nb
        _REF.clear()
        t = _wide_tables(name, "all")
        calls = _call_list(n)[:3]
        calls[2] = calls[2][:3] + (n // 16,)  # (steps_await = n / 2 is reached by no chain of these shapes: the sweeps are [4, 4, 4])
        _REF[key] = (t, calls) + _reference(name, t, SEEDS.get((name, "early stop"), SEED), calls)
    return _REF[key]


def early_stop_inputs(name):
    """the cooling call with steps_await = n // 16 under all three holds: on the oracles at least one chain returns early and at
    least one does not; returns (t, calls, start, ref)"""
    t, calls, start, ref = early_stop_reference(name)
    _assert_inputs((name, "early stop"), t, ref)
    sweeps = [c["sweeps"] for c in ref[2]["chains"]]
    print("%s: the cooling call ran %s sweeps (%s when the case was written)" % (name, sweeps, EARLY_STOP_SWEEPS[name]))
    assert min(sweeps) < 4 and max(sweeps) == 4, (name, sweeps)
    return t, calls, start, ref


# ------------------------------------------------------------------------------------------------------------ the device
def _route_of(t):
    return (B.ROUTE_HELD if t["mask"] is not None or t["cn"] is not None else 0) | (B.ROUTE_FIELDS if t["fl"] is not None else 0)


def _run_generic(m, t, start, ref, calls, what, na, ka):
    """test_gpu_held_oracle._run call by call, the route asserted after each: one step per pass on the generic kernel"""
    for i in range(len(calls)):
        _run(m, t, start, ref[i:i + 1], calls[i:i + 1], what + (i,), na, ka, fast=False)
        assert m.last_pass_steps() == 1 and m.last_route() == _route_of(t), (what, i, m.last_pass_steps(), m.last_route())
        assert not m.last_route() & B.ROUTE_PRODUCTION


def _assert_eta_plan(name, m, rowptr, K):
    """held_k3_k100_hub is for eta outside LDS, held_k70_k3 for eta inside.  The other two: eta alone, K rows of maxdeg + 1 words (179
    and 226 KiB), is past the whole budget, so it is outside there as well"""
    maxdeg = int(np.diff(rowptr).max())
    plan = m.last_eta_plan()
    print("%s: eta plan %s (K = %d, largest degree %d: eta has %d bytes)" % (name, plan, K, maxdeg, 4 * K * (maxdeg + 1)))
    if name == "held_k70_k3":
        assert plan[0] == 1, (name, plan, maxdeg)
    else:
        assert 4 * K * (maxdeg + 1) > LDS_BUDGET and plan[0] == 0, (name, plan, maxdeg)
    assert name != "held_k3_k100_hub" or maxdeg > 600
    assert plan[1:] == (0, 0, 0)  # (the window is the production kernel's)


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_every_held_call_above_64_blocks_is_the_held_oracles(name, hold):
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    t, calls, start, ref = matrix_inputs(name, hold)
    m = _device(name, t, SEEDS.get((name, hold), SEED))
    _run_generic(m, t, start, ref, calls, (name, hold), na, ka)
    _assert_eta_plan(name, m, rowptr, ka + kb)
    m.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_cooling_call_that_one_chain_leaves_early_is_the_oracles_above_64_blocks(name):
    """entropy_min, the count of T < 1 steps and "this chain has returned" through barred steps, steps of clamped nodes and fielded
    decisions in the generic kernel's own loop: a chain that has returned stops, the others run on"""
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    t, calls, start, ref = early_stop_inputs(name)
    m = _device(name, t, SEEDS.get((name, "early stop"), SEED))
    _run_generic(m, t, start, ref, calls, (name, "early stop"), na, ka)
    m.close()


# ------------------------------------------------------------------------------------------- the shuffle over 512 segments
def _class_size(c):
    """open nodes per type of class c >= 1: 273 of each type's 400 nodes in all, which leaves class 0 more than a wave of open ones"""
    return 3 if c % 64 == 0 else 2 if c % 16 == 0 else 1


def test_the_shuffle_over_512_segments_permutes_every_class_as_the_oracle_shuffles_its_compacted_labels():
    """held_k127_k129, three chains behind a shuffle and two sweeps: 256 classes, each with open nodes of both types -- the 512
    (type, class) segments that shuffle_philox_constrained_kernel's bisection is sized for.  Class c >= 1 bans one block per type
    and has one to three open nodes per type, picked among those that no chain holds in a banned block (every sixteenth class a
    clamped node of each type beside them); class 0 has the rest, more than 64 open nodes per type.  The clamp is a random 30 % of
    the nodes from which the picked open nodes are taken out: 255 + 65 open nodes of a type do not fit beside 120 clamped ones in
    400.  The reference is that of tests/test_gpu_constraints.py: an edgeless oracle per (chain, class) on the compacted labels,
    keyed seed + c * 0x9E3779B97F4A7C15 mod 2^64."""
    name = "held_k127_k129"
    (rowptr, col), na, nb, ka, kb, eps = _case(name)
    n, K, n_cls = na + nb, ka + kb, 256
    m = _model(name, CHAINS, first_chain_id=FIRST_ID)
    m.shuffle_bisbm()
    m.run_sweeps(2)  # (every chain its own labels)
    start = [m.get_memberships(c).astype(np.int64) for c in range(CHAINS)]
    allowed = np.ones((n_cls, K), dtype=bool)
    for c in range(1, n_cls):
        allowed[c, (c - 1) % ka] = allowed[c, ka + (c - 1) % kb] = False
    assert {s >> 5 for s in range(K) if not allowed[:, s].all()} == set(range(8))  # (bans in every word of a row)
    fits = lambda c: np.all([allowed[c, s] for s in start], axis=0)
    cls = np.zeros(n, dtype=np.int64)
    mask = np.random.default_rng(5).random(n) < 0.3
    for lo, hi in ((0, na), (na, n)):
        for c in range(1, n_cls):
            free = lo + np.flatnonzero(fits(c)[lo:hi] & (cls[lo:hi] == 0))
            picked = free[:_class_size(c)]
            assert len(picked) == _class_size(c)
            cls[picked], mask[picked] = c, False
            if c % 16 == 0:  # a clamped member: no position of the segment
                held = [v for v in free[_class_size(c):] if mask[v]][:1]
                assert len(held) == 1
                cls[held] = c
    m.clamp(mask)
    m.constrain(cls, allowed)
    segs = {}
    for t, lo, hi in ((0, 0, na), (1, na, n)):
        for c in range(n_cls):
            segs[(t, c)] = lo + np.flatnonzero(~mask[lo:hi] & (cls[lo:hi] == c))
    sizes = {k: len(F) for k, F in segs.items()}
    assert sum(1 for s in sizes.values() if s > 0) == 512, sizes
    assert sizes[(0, 0)] > 64 and sizes[(1, 0)] > 64 and all(sizes[(t, c)] == _class_size(c) for t in (0, 1) for c in range(1, n_cls)), sizes
    assert int((mask & (cls > 0)).sum()) == 2 * 15 and int(mask.sum()) >= 64
    oracles = {}
    for ch in range(CHAINS):
        for c in range(n_cls):
            Fa, Fb = segs[(0, c)], segs[(1, c)]
            F = np.concatenate([Fa, Fb])
            edgeless = (np.zeros(len(F) + 1, dtype=np.uint64), np.zeros(1, dtype=np.uint32))
            o = O.OracleModel(edgeless[0], edgeless[1], len(Fa), len(Fb), ka, kb, eps, start[ch][F])
            o.seed_philox((SEED + c * CLASS_KEY) % (1 << 64), FIRST_ID + ch)
            o.shuffle_bisbm()  # (epoch 0: the handle's first shuffle above)
            o.set_memberships(start[ch][F])
            oracles[(ch, c)] = (o, F)
    for call in range(2):
        m.shuffle_bisbm()
        for ch in range(CHAINS):
            got = m.get_memberships(ch)
            want = start[ch].copy()
            for c in range(n_cls):
                o, F = oracles[(ch, c)]
                o.shuffle_bisbm()
                want[F] = o.memberships()
            assert (got[mask] == start[ch][mask]).all(), (call, ch)
            assert (got == want).all(), (call, ch, np.flatnonzero(got != want))
            assert allowed[cls, got].all()
            for t, lo, hi in ((0, 0, na), (1, na, n)):  # block sizes are preserved class by class
                pairs = cls[lo:hi] * K
                assert (np.bincount(pairs + got[lo:hi], minlength=n_cls * K) == np.bincount(pairs + start[ch][lo:hi], minlength=n_cls * K)).all()
            _assert_state_is_a_rebuild(m, rowptr, col, ch)
        assert any((m.get_memberships(ch) != start[ch]).any() for ch in range(CHAINS)), call
    m.close()
