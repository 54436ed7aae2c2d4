"""Model-based random testing of the holds on the GPU (-m gpu): random call sequences that set, change and clear a clamp, block
constraints and block fields between anneals under every schedule -- the transitions that change the kernel route, the sizing of
the held LDS, the eta_in_lds decision and the depth cap -- on random small graphs, Philox mode, several chains, with the held
oracle (oracle/bisbm_oracle.c, tests/test_oracle_holds.py) as the model: after every call each chain's labels, block state,
description length and running sum must equal its oracle run's, and after every anneal the return value and last_counts() too.
tests/test_gpu_fuzz.py and its seeds stay as they are: it walks merges, splits, wide labels and the compat mode, none of which a
held handle serves.

Every anneal also asserts the margin condition of tests/test_gpu_held_oracle.py on the oracle's side (no accept test within a
relative 1e-9 of its threshold).  SEEDS was fixed on the host by walking the oracle side of every sequence alone (run_sequence with
device=False); the one thing that walk cannot follow is a shuffle under a clamp or constraints, after which the model is re-seated
on the device's labels (the held shuffle has its own tests): there the host walk keeps the model's labels."""
import importlib
import os

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_gpu_fuzz import _check
from test_oracle_holds import half_table, random_field

pytestmark = pytest.mark.gpu

B = importlib.import_module("bipartitesbm-mcmc_amd")
SYN = importlib.import_module("bipartitesbm-mcmc_amd.synthetic")
BIG = 1 << 60
MAX_SHARE = 0.97  # kHeldFastMaxClampShare (csrc/bisbm_kernels.hpp)

# 48 sequences; an even seed with seed % 6 == 4 has one type at 65 .. 100 blocks (generic kernel only), one with seed % 6 == 2 sets a
# hold and then makes a constant call of segmented length, an odd one with seed % 8 == 7 has both block counts <= 8 (deep passes
# when unheld) and sets a hold, anneals, clears and anneals again (run_sequence's script).  A seed with a call at margin <= 1e-9 would have been replaced by the next integer: none was.
SEEDS = list(range(48))
# BISBM_FUZZ_HOLD_SEEDS=N widens the hunt (further sequences of the same kinds)
SEEDS = SEEDS + list(range(48, int(os.environ.get("BISBM_FUZZ_HOLD_SEEDS", "48"))))


def _check_fielded(g, os_, phi, what):
    """_check of tests/test_gpu_fuzz.py with |S| + |Phi| in the place of |S|: under fields the running sum advances by dS + dPhi"""
    ent, cum = np.atleast_1d(g.entropy()), np.atleast_1d(g.get_entropy())
    for c, o in enumerate(os_):
        assert (g.get_memberships(c) == o.memberships()).all(), (what, c)
        assert (g.get_m(c) == o.m()).all() and (g.get_m_r(c) == o.m_r()).all(), (what, c)
        assert (g.get_n_r(c) == o.n_r()).all() and (g.get_eta_rk_(c) == o.eta()).all(), (what, c)
        assert abs(ent[c] - o.entropy()) <= 1e-9 * max(1.0, abs(o.entropy())), (what, c)
        assert abs(cum[c] - o.get_entropy()) <= 1e-9 * max(1.0, abs(o.get_entropy())) + 1e-12 * (abs(o.entropy()) + abs(phi[c])), (what, c)


def _trivial_table(cls, allowed, na, ka):
    """every A_v is all blocks of v's type: the library stores such a table as a clear"""
    n = len(cls)
    return bool(allowed[cls[:na], :ka].all() and allowed[cls[na:], ka:].all()) if n else True


def _assert_holds_are(g, hold, what):
    assert (g.clamped() == hold["mask"]).all(), what
    cls, allowed = g.constraints()
    if hold["cn"] is None:
        assert cls is None and allowed is None, what
    else:
        assert (cls == hold["cn"][0]).all() and (np.asarray(allowed) != 0).tolist() == (hold["cn"][1] != 0).tolist(), what
    cls, field = g.fields()
    if hold["fl"] is None:
        assert cls is None and field is None, what
    else:
        assert (cls == hold["fl"][0]).all() and np.asarray(field).tobytes() == hold["fl"][1].tobytes(), what


def run_sequence(seed, device=True, monkeypatch=None):
    """One sequence.  device=False walks the oracle side alone (no GPU): the margins and the counters of every anneal.  Returns
    (log, smallest margin, counters, shape).  The counters also say what the sequence covered: anneals under a clamp or lists, under a
    field, held constant T = 0 calls, held calls of segmented length, unheld launches that had to have their depth back
    (tests/test_oracle_holds.py adds them up over SEEDS on the host)."""
    rng = np.random.default_rng(77000 + seed)
    wide, small, long_call = seed % 6 == 4, seed % 8 == 7, seed % 6 == 2
    na, nb = int(rng.integers(20, 121)), int(rng.integers(20, 121))
    if wide:
        na = int(rng.integers(105, 121))
    n = na + nb
    ne = int(rng.integers(2, 8) * n)
    if small:
        ka, kb = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    else:
        ka, kb = int(rng.integers(1, min(na, 40) + 1)), int(rng.integers(1, min(nb, 40) + 1))
    if wide:
        ka = int(rng.integers(65, 101))
    rowptr, col = cases.random_graph(int(rng.integers(1 << 30)), na, nb, ne, ka, kb, hubs=int(rng.integers(0, 3)), isolated=int(rng.integers(0, 3)))
    eps = float(rng.choice([1.0, 0.5, 0.001, 0.0, 3.0]))
    chains = int(rng.integers(1, 5))
    labels = O.contiguous_labels(na, nb, ka, kb)
    s0 = int(rng.integers(1 << 20))
    if small and monkeypatch is not None:
        monkeypatch.setenv("BISBM_PASS_DEPTH", "8")  # (the deepest pass the launch may run, not a policy's choice: the chain is the same chain)
    g = B.BlockModel(labels, SYN.types_vector(na, nb), ka + kb, ka, kb, eps, (rowptr, col), n_chains=chains, rng="philox", seed=s0) if device else None
    os_ = []
    for c in range(chains):
        o = O.OracleModel(rowptr, col, na, nb, ka, kb, eps, labels)
        o.seed_philox(s0, c)
        os_.append(o)
    mh = B.MetropolisHasting()
    hold = dict(mask=np.zeros(n, dtype=bool), cn=None, fl=None)
    held = lambda: bool(hold["mask"].any()) or hold["cn"] is not None  # (a clamp or constraints: what the held kernels serve)
    any_hold = lambda: held() or hold["fl"] is not None
    phi = lambda: [B.numpy_field_energy(o.memberships(), hold["fl"][0], hold["fl"][1], na, ka) if hold["fl"] is not None else 0.0 for o in os_]

    def check(what):
        if not device:
            return
        if hold["fl"] is None:
            _check(g, os_, what)
        else:
            _check_fielded(g, os_, phi(), what)

    def both(call):
        if device:
            call(g)
        for o in os_:
            call(o)

    both(lambda x: x.shuffle_bisbm() if seed % 3 else x.init_bisbm())
    check("start")
    log, margin = [], float("inf")
    seen = dict(clamped=0, barred=0, fielded=0, turned=0, accepted=0, anneals=0, held_anneals=0, fielded_anneals=0, held_cold=0, held_long=0, depth_back=0, cleared_clamps=0, cleared_lists=0)
    cleared_since = False
    # The first calls of two kinds of sequence are scripted, so that what the kind is for happens whatever the draws are:
    #   both block counts <= 8: a clamp or lists, an anneal under them (at T = 0 in every third), everything cleared, an unheld anneal at
    #   T > 0 -- the launch that must have its depth back;
    #   the segmented length: a clamp, lists or a field, then the long constant call -- cut into launches, or not, on a held handle.
    script = []
    if small:
        script = [dict(op=("clamp", "constrain")[(seed // 8) % 2], how="set"), dict(op="anneal", cold=(seed // 8) % 3 == 0), dict(op="clear_all"),
                  dict(op="anneal", warm=True)]
    elif long_call:
        script = [dict(op=("clamp", "constrain", "fields")[(seed // 6) % 3], how="set"), dict(op="anneal", long=True)]
    for step in range(int(rng.integers(8, 13))):
        op = str(rng.choice(["anneal"] * 8 + ["clamp", "clamp", "constrain", "constrain", "fields", "fields", "set", "init", "shuffle", "bad"]))
        forced = script[step] if step < len(script) else {}
        op = forced.get("op", op)
        what = (seed, log, op)
        if op == "anneal":
            sched, kw = [("constant", [float(rng.choice([1.0, 0.5, 2.0, 0.0]))]), ("linear", [2.0, 1.5 / (3 * n)]),
                         ("abrupt_cool", [float(rng.integers(0, 2 * n))]), ("exponential", [3.0, 0.999]), ("logarithmic", [1.0, 2.0])][int(rng.integers(5))]
            dur = int(rng.integers(1, 4)) * n
            kind = int(rng.integers(4)) if rng.random() < 0.45 else 3
            if forced.get("cold"):
                sched, kw = "constant", [0.0]
            if forced.get("warm") and sched == "constant" and kw[0] == 0.0:
                kw = [1.0]
            if forced.get("long"):
                seg = (100000 + n - 1) // n  # (bisbm_anneal: sweeps per launch of a segmented call)
                sched, kw = "constant", [float(rng.choice([1.0, 2.0, 0.5]))]
                dur = int(rng.integers(2 * seg, 3 * seg + 2)) * n + int(rng.integers(0, n))
                kind = int(rng.integers(4))
            wait = [0, int(rng.integers(1, n)), int(rng.integers(n, max(n + 1, dur))), BIG][kind]
            want = [o.anneal(sched, kw, dur, wait) for o in os_]
            margin = min([margin] + [o.last_margin for o in os_])
            assert margin > 1e-9, (what, sched, margin, "an accept test too close to its threshold: replace the seed")
            for o in os_:
                for k, v in o.hold_counts().items():
                    seen[k] += v
                seen["accepted"] += o.last_accepted
            seen["anneals"] += 1
            cold = sched == "constant" and kw[0] == 0.0
            depth_back = small and cleared_since and not any_hold() and not cold  # (a cleared hold gave the depth back)
            seen["held_anneals"] += int(held())
            seen["fielded_anneals"] += int(hold["fl"] is not None)
            seen["held_cold"] += int(held() and hold["fl"] is None and cold)
            seen["held_long"] += int(bool(forced.get("long")) and any_hold())
            seen["depth_back"] += int(depth_back)
            if device:
                got = np.atleast_1d(mh.anneal(g, sched, kw, dur, wait))
                acc, sw = g.last_counts()
                for c, o in enumerate(os_):
                    assert got[c] == want[c], (what, sched, c, got[c], want[c])
                    assert int(acc[c]) == o.last_accepted and int(sw[c]) == o.last_sweeps, (what, sched, c)
                # the route, as bisbm_anneal.hip's dispatch alone gives it
                steps = g.last_pass_steps()
                if hold["fl"] is not None:
                    assert steps == 1, (what, steps)
                elif held() and float(hold["mask"].sum()) > MAX_SHARE * float(n):
                    assert steps == 1, (what, steps)
                elif held() and ka <= 64 and kb <= 64:
                    assert steps <= 2, (what, steps)
                elif held():
                    assert steps == 1, (what, steps)
                elif depth_back:
                    assert steps > 2, (what, steps)
            log.append("anneal:%s" % sched)
        elif op == "clamp":
            share = float(rng.choice([0.0, 0.05, 0.3, 0.6, 0.98]))
            if forced.get("how") == "set":
                share = float(rng.choice([0.05, 0.3, 0.6]))
            mask = rng.random(n) < share
            cleared_since = cleared_since or (bool(hold["mask"].any()) and not mask.any())
            hold["mask"] = mask
            both(lambda x: x.clamp(mask))
            log.append("clamp:%g" % share)
        elif op == "constrain":
            kind = 2 if forced.get("how") == "set" else int(rng.integers(5))
            if kind == 0:  # a clear
                cleared_since = cleared_since or hold["cn"] is not None
                hold["cn"] = None
                if device:
                    g.unconstrain()
                for o in os_:
                    o.constrain(None, None)
                log.append("constrain:clear")
            else:
                now = np.stack([o.memberships() for o in os_])
                cls, allowed = half_table(rng, now, na, ka, kb, pools=int(rng.integers(1, 120)))  # (few classes: their rows fill up with the chains' labels; many: about a node per class)
                if kind == 1:
                    allowed[:] = 1  # an all-allowing table: stored as a clear
                trivial = _trivial_table(cls, allowed, na, ka)
                cleared_since = cleared_since or (hold["cn"] is not None and trivial)
                hold["cn"] = None if trivial else (cls, allowed)
                both(lambda x: x.constrain(cls, allowed))
                log.append("constrain:%s" % ("all" if trivial else "lists"))
                if trivial and forced.get("how") == "set":  # (one block per type: no list can bar anything, a clamp stands in)
                    hold["mask"] = rng.random(n) < 0.3
                    both(lambda x: x.clamp(hold["mask"]))
                    log.append("clamp:0.3")
        elif op == "fields":
            kind = 2 if forced.get("how") == "set" else int(rng.integers(4))
            if kind == 0:
                hold["fl"] = None
                if device:
                    g.clear_fields()
                for o in os_:
                    o.set_fields(None, None)
                log.append("fields:clear")
            else:
                cls, field = random_field(rng, n, ka + kb, n_classes=int(rng.integers(2 if forced else 1, 7)), scale=float(rng.choice([0.3, 1.5])), shift=int(rng.integers(4)))
                if kind == 1:
                    field[:] = 0.0  # a zero table: stored as a clear
                hold["fl"] = None if not field.any() else (cls, field)
                both(lambda x: x.set_fields(cls, field))
                log.append("fields:%s" % ("zero" if hold["fl"] is None else "table"))
        elif op == "clear_all":
            cleared_since = cleared_since or held()
            seen["cleared_clamps"] += int(hold["mask"].any())
            seen["cleared_lists"] += int(hold["cn"] is not None)
            hold.update(mask=np.zeros(n, dtype=bool), cn=None, fl=None)
            if device:
                g.unclamp()
                g.unconstrain()
                g.clear_fields()
            for o in os_:
                o.clamp(None)
                o.constrain(None, None)
                o.set_fields(None, None)
            log.append("clear")
        elif op == "set":  # the labels of another chain: admissible, since every chain's labels are
            c = int(rng.integers(chains))
            lab = os_[int(rng.integers(chains))].memberships()
            if device:
                g.set_memberships(lab, chain=c)
                g.init_bisbm()
            os_[c].set_memberships(lab)
            for o in os_:
                o.init_bisbm()
            log.append("set")
        elif op == "init":
            both(lambda x: x.init_bisbm())
            log.append("init")
        elif op == "shuffle":
            before = [o.memberships() for o in os_]
            both(lambda x: x.shuffle_bisbm())  # (the oracle's: the plain shuffle, and its epoch moves as the device's does)
            if held():  # the held shuffle keeps clamped labels and lists (its own tests): the model is re-seated on the device's labels
                for c, o in enumerate(os_):
                    lab = g.get_memberships(c) if device else before[c]  # (host walk: see the module's docstring)
                    assert (lab[hold["mask"]] == before[c][hold["mask"]]).all(), (what, c)
                    assert hold["cn"] is None or hold["cn"][1][hold["cn"][0], lab].all(), (what, c)
                    assert (np.bincount(lab, minlength=ka + kb) == np.bincount(before[c], minlength=ka + kb)).all(), (what, c)
                    o.set_memberships(lab)
                    o.init_bisbm()
            log.append("shuffle:%s" % ("held" if held() else "plain"))
        else:  # a call that must fail and leave everything as it was
            lab0 = os_[0].memberships()
            kinds = []
            if any_hold():
                kinds.append("merge")
            if hold["cn"] is not None:
                cls, allowed = hold["cn"]
                outside = [(v, s) for v in range(n) for s in (range(ka) if v < na else range(ka, ka + kb)) if not allowed[cls[v], s]]
                if outside:
                    kinds.append("set")
            movable = [v for v in range(n) if (ka if v < na else kb) >= 2]
            if movable:
                kinds.append("table")
            kind_i, pick = int(rng.integers(1 << 20)), int(rng.integers(1 << 20))  # (drawn whatever follows: the host walk draws what the device walk draws)
            if not kinds or not device:
                log.append("bad:none" if not kinds else "bad:host")
                continue
            kind = kinds[kind_i % len(kinds)]
            with pytest.raises(B.BisbmError) as e:
                if kind == "merge":
                    g.agg_merge(1 if ka > 1 else 0, 0 if ka > 1 else 1, 5)
                elif kind == "set":
                    v, s = outside[pick % len(outside)]
                    bad = lab0.copy()
                    bad[v] = s
                    g.set_memberships(bad, chain=0)
                else:
                    v = movable[pick % len(movable)]
                    t_cls = np.zeros(n, dtype=np.uint8)
                    t_cls[v] = 1
                    t_allowed = np.ones((2, ka + kb), dtype=np.uint8)
                    t_allowed[1, lab0[v]] = 0
                    g.constrain(t_cls, t_allowed)
            assert e.value.code == {"merge": B.BISBM_ERR_STATE, "set": B.BISBM_ERR_INVALID_ARG, "table": B.BISBM_ERR_STATE}[kind], (what, kind, e.value)
            _assert_holds_are(g, hold, (what, kind))
            log.append("bad:%s" % kind)
        check((seed, log))
    if device:
        _assert_holds_are(g, hold, (seed, log, "end"))
        g.close()
    assert not small or (seen["depth_back"] >= 1 and seen["held_anneals"] >= 1), (seed, log, seen)
    assert not long_call or seen["held_long"] >= 1, (seed, log, seen)
    return log, margin, seen, (na, nb, ka, kb, chains, eps)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_call_sequences_with_holds(seed, monkeypatch):
    for k in ("BISBM_FORCE_GENERIC", "BISBM_HELD_FAST", "BISBM_PASS_DEPTH", "BISBM_T_TABLE_CAP", "BISBM_LAUNCH_STEPS", "BISBM_SINGLE_STEPS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BISBM_KEEP_SUM", "1")
    log, margin, seen, (na, nb, ka, kb, chains, eps) = run_sequence(seed, device=True, monkeypatch=monkeypatch)
    print("seed %d %d+%d nodes, %d+%d blocks, %d chains, eps %g: %s; smallest margin %.3g, steps of clamped nodes %d, barred targets %d, accepted %d, "
          "fielded steps %d of which the field turned %d" % (seed, na, nb, ka, kb, chains, eps, " ".join(log), margin, seen["clamped"], seen["barred"],
                                                           seen["accepted"], seen["fielded"], seen["turned"]))
