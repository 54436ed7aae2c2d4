"""CPU checks of the held conditionals and the least-settled ranking (include/bisbm.h, "Held conditionals", "Least settled"): the
numpy model of the held row against a literal double loop on bit patterns, the definition tied to the tilted, restricted
stationary distribution of the enumerable graph on the oracle, the numpy model of the ranking, and the drop-in boundary (header,
ctypes table, BlockModel, the C++ mirror, marginalize's and the command line's refusals)."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import oracle_lib as O
from test_conditionals import TOL_DS_REL_S, _oracle_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bipartitesbm-mcmc_amd")
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed

CALLS = ["bisbm_held_conditionals_set", "bisbm_held_conditionals_get", "bisbm_least_settled_topk"]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _literal(dS, r, free, beta, clamped, allowed, f):
    """steps 1 to 4 of "Held conditionals", one scalar operation after the other"""
    K = len(dS)
    A = [True] * K if allowed is None else [bool(a) for a in allowed]
    dE = []
    for s in range(K):
        if s == r:
            dE.append(0.0)
        elif f is None:
            dE.append(float(dS[s]))
        else:
            diff = float(f[s]) - float(f[r])
            dE.append(float(dS[s]) + diff)
    is_open = K > 1 and free and not clamped and sum(A) > 1
    margin = None
    if not is_open:
        P = [1.0 if s == r else 0.0 for s in range(K)]
    else:
        mn = 0.0  # (the 0 at r)
        for s in range(K):
            if A[s] and dE[s] < mn:
                mn = dE[s]
        w = []
        for s in range(K):
            x = beta * (dE[s] - mn)
            w.append(0.0 if (x > 700.0 or not A[s]) else float(np.exp(-x)))
        Z = w[0]
        for y in w[1:]:
            Z = Z + y
        P = [y / Z for y in w]
        margin = min(dE[s] for s in range(K) if s != r and A[s])
    acc = 0.0
    for y in P:
        if y != 0.0:
            acc = acc + y * float(np.log(y))
    return dE, P, P[r], 0.0 - acc, margin


ROWS = [
    # name, dS row, r, free, beta, clamped, allowed, f
    ("no_hold", [0.0, 1.5, -0.25, 3.0, 7.75], 0, True, 1.0, False, None, None),
    ("no_hold_beta", [2.0, 0.0, -1.0, 0.5], 1, True, 0.37, False, None, None),
    ("no_hold_not_free", [0.0, -5.0, 2.0], 0, False, 1.0, False, None, None),
    ("clamped", [0.0, -5.0, 2.0], 0, True, 1.0, True, None, None),
    ("clamped_with_field", [0.0, -5.0, 2.0], 0, True, 1.0, True, [1, 1, 0], [0.5, -1.0, 2.0]),
    ("one_allowed", [3.0, 0.0, -2.0], 1, True, 1.0, False, [0, 1, 0], None),
    ("minimum_outside_A", [0.0, -9.0, 1.0, -0.5, 4.0], 0, True, 1.0, False, [1, 0, 1, 1, 0], None),
    ("minimum_outside_A_all_others_dearer", [0.0, -9.0, 1.0, 0.5], 0, True, 2.0, False, [1, 0, 1, 1], None),
    ("field_plus_800", [0.0, 1.0, -1.0, 2.0], 0, True, 1.0, False, None, [0.0, 800.0, 0.0, 0.25]),   # x > 700 -> exactly 0.0
    ("field_minus_800", [0.0, 1.0, -1.0, 2.0], 0, True, 1.0, False, None, [0.0, -800.0, 0.0, 0.25]),  # everything but s = 1 -> 0.0
    ("field_minus_800_barred", [0.0, 1.0, -1.0, 2.0], 0, True, 1.0, False, [1, 0, 1, 1], [0.0, -800.0, 0.0, 0.25]),
    ("field_rounds", [0.0, 0.1, 0.2, 0.3], 3, True, 1.0, False, None, [0.1, 0.7, 1e-17, 0.3]),  # (f[s] - f[r]) first, then one add
    ("ties_in_min", [0.0, -2.0, -2.0, 1.0, -2.0], 0, True, 1.0, False, [1, 1, 0, 1, 1], None),
    ("tie_with_r", [0.0, 0.0, 0.0], 1, True, 3.0, False, [1, 1, 1], [1.0, 1.0, 1.0]),
    ("k_own_1", [0.0], 0, False, 1.0, False, [1], [0.3]),
    ("own_block_counts_as_allowed", [0.0, 1.0, 2.0], 0, True, 1.0, False, [0, 1, 1], None),
]


@pytest.mark.parametrize("name,dS,r,free,beta,clamped,allowed,f", ROWS, ids=[c[0] for c in ROWS])
def test_numpy_model_is_the_literal_loop(name, dS, r, free, beta, clamped, allowed, f):
    if name == "own_block_counts_as_allowed":  # (the literal loop takes A_v as the header defines it: r is in it)
        lit_allowed = [1, 1, 1]
    else:
        lit_allowed = allowed
    dE, P, stay, ent, margin = D.numpy_held_conditional_row(np.array(dS), r, free, beta, clamped=clamped, allowed_own=allowed,
                                                            f_own=None if f is None else np.array(f))
    dEl, Pl, stay_l, ent_l, margin_l = _literal(dS, r, free, beta, clamped, lit_allowed, f)
    assert (_bits(dE) == _bits(dEl)).all() and (_bits(P) == _bits(Pl)).all()
    assert _bits([stay])[0] == _bits([stay_l])[0] and _bits([ent])[0] == _bits([ent_l])[0]
    assert margin == margin_l
    assert ent >= 0.0 and not math.copysign(1.0, ent) < 0 and 0.0 <= stay <= 1.0
    assert abs(sum(Pl) - 1.0) <= (len(dS) + 4) * 2.0 ** -52
    if allowed is not None:
        assert all(P[s] == 0.0 for s in range(len(dS)) if not lit_allowed[s])
    if name.startswith("no_hold"):  # no hold: numpy_conditional_row, bit for bit
        P0, stay0, ent0, margin0 = D.numpy_conditional_row(np.array(dS), r, free, beta)
        assert (_bits(P) == _bits(P0)).all() and _bits([stay, ent]).tolist() == _bits([stay0, ent0]).tolist() and margin == margin0
        assert (_bits(dE) == _bits(dS)).all()
    if name in ("clamped", "clamped_with_field", "one_allowed", "k_own_1"):
        assert P[r] == 1.0 and sum(P) == 1.0 and ent == 0.0 and margin is None
    if name == "clamped_with_field":  # dE is reported all the same, inside A_v or not
        assert dE[1] == -5.0 + (-1.0 - 0.5) and dE[2] == 2.0 + (2.0 - 0.5)
    if name.startswith("minimum_outside_A"):
        assert P[1] == 0.0 and margin == (-0.5 if len(dS) == 5 else 0.5) and max(P) < 1.0
    if name == "field_plus_800":
        assert P[1] == 0.0 and P[0] > 0.0
    if name.startswith("field_minus_800"):
        if allowed is None:
            assert P[1] == 1.0 and [P[0], P[2], P[3]] == [0.0, 0.0, 0.0] and stay == 0.0 and ent == 0.0
        else:
            assert P[1] == 0.0 and P[2] > P[0] > P[3] > 0.0
    if name == "field_rounds":
        assert dE[2] == 0.2 + (1e-17 - 0.3)


def test_a_device_exp_is_taken_where_one_is_given():
    calls = []

    def exp(x):
        calls.append(np.array(x))
        return np.exp(x) * 0.5
    dE, P, stay, ent, margin = D.numpy_held_conditional_row(np.array([0.0, 1.0]), 0, True, 1.0, exp=exp)
    P0 = D.numpy_held_conditional_row(np.array([0.0, 1.0]), 0, True, 1.0)[1]
    assert len(calls) == 1 and (_bits(P) == _bits(P0)).all()  # (a common factor of 1 / 2 drops out exactly)


def _enum_holds():
    """classes over the 6 + 6 nodes of the enumerable graph: class 0 allows everything, class 1 the first block of either type,
    class 2 the second; three field classes of about a nat"""
    n, K = cases.ENUM_NA + cases.ENUM_NB, 4
    cls = np.zeros(n, dtype=np.uint8)
    cls[[0, 7]] = 1
    cls[[4, 10]] = 2
    allowed = np.array([[1, 1, 1, 1], [1, 0, 1, 0], [0, 1, 0, 1]], dtype=bool)
    fcls = (np.arange(n) % 3).astype(np.uint8)
    field = np.random.default_rng(8).normal(scale=1.0, size=(3, K))
    field[0] = 0.0
    return cls, allowed, fcls, field


def test_held_softmax_is_the_exact_conditional_of_the_tilted_restricted_distribution(record_property):
    """P(b_v = s | rest) of exp(-(S + Phi)) over the admissible states without an empty block, against the held softmax of the
    oracle's dS rows, at 40 seeded admissible states.  The field difference is exact to rounding, so the bound is the one of
    tests/test_conditionals.py: |P - P_exact| <= 2e-9 |S| P_exact + 1e-15."""
    rowptr, col = cases.enumerable_graph()
    na = nb = cases.ENUM_NA
    n = na + nb
    cls, allowed, fcls, field = _enum_holds()
    states, prob, _ = cases.enumerable_states()
    labels_of = {}
    weight = {}
    for i, code in enumerate(states):
        bits = [(int(code) >> j) & 1 for j in range(n)]
        lab = np.array(bits[:na] + [2 + b for b in bits[na:]], dtype=np.int64)
        if not allowed[cls, lab].all():
            continue
        labels_of[int(code)] = lab
        weight[int(code)] = prob[i] * math.exp(-B.numpy_field_energy(lab, fcls, field, na, 2))
    admissible = sorted(labels_of)
    assert 40 < len(admissible) < len(states)
    rng = np.random.default_rng(3)
    seen = {"open": 0, "barred": 0, "alone": 0}
    worst_P = 0.0
    for code in rng.choice(admissible, 40, replace=False):
        code = int(code)
        labels = labels_of[code].astype(np.uint32)
        rows, worst, S, n_r = _oracle_rows(rowptr, col, na, nb, 2, 2, cases.ENUM_EPS, labels)
        assert worst <= TOL_DS_REL_S * S
        for v in range(n):
            lo = 0 if v < na else 2
            r = int(labels[v]) - lo
            free = n_r[labels[v]] > 1
            A = allowed[cls[v], lo:lo + 2]
            dE, P, stay, ent, margin = D.numpy_held_conditional_row(rows[v], r, free, 1.0, allowed_own=A, f_own=field[fcls[v], lo:lo + 2])
            other = code ^ (1 << v)
            exact = np.zeros(2)
            if other in weight:
                assert free and A.all()
                seen["open"] += 1
                exact[r] = weight[code] / (weight[code] + weight[other])
                exact[1 - r] = weight[other] / (weight[code] + weight[other])
                assert margin == dE[1 - r] and _bits(dE[1 - r]) == _bits(B.numpy_field_row(rows[v], r, field[fcls[v], lo:lo + 2])[1 - r])
            else:
                seen["barred"] += not A.all()
                seen["alone"] += not free
                exact[r] = 1.0
                assert margin is None and ent == 0.0
            err = np.abs(P - exact)
            assert (err <= 2 * TOL_DS_REL_S * S * exact + 1e-15).all(), (code, v, P, exact)
            worst_P = max(worst_P, float(err.max()))
            assert stay == P[r]
    assert seen["open"] > 0 and seen["barred"] > 0 and seen["alone"] > 0, seen
    record_property("worst_P_abs", worst_P)


def test_numpy_ranking_orders_values_then_indices_and_refuses_negative_sums():
    v = np.array([0.5, 0.0, 2.0, 0.5, 2.0, 0.0])
    idx, val = D.numpy_least_settled(v, 4, "entropy")
    assert idx.tolist() == [2, 4, 0, 3] and val.tolist() == [2.0, 2.0, 0.5, 0.5]
    idx, val = D.numpy_least_settled(v, 8, "stay")
    assert idx.tolist() == [1, 5, 0, 3, 2, 4, 0xFFFFFFFF, 0xFFFFFFFF] and val.tolist() == [0.0, 0.0, 0.5, 0.5, 2.0, 2.0, 0.0, 0.0]
    # the precondition of the device's unsigned keys: bit patterns of non-negative doubles order as the values do
    x = np.abs(np.random.default_rng(1).normal(size=1000)) * 10.0 ** np.random.default_rng(2).integers(-300, 300, 1000)
    assert (np.argsort(x.view(np.uint64), kind="stable") == np.argsort(x, kind="stable")).all()
    for bad in (np.array([0.0, -0.0]), np.array([1.0, -1e-300]), np.array([np.nan])):
        with pytest.raises(AssertionError):
            D.numpy_least_settled(bad, 1)


def test_the_calls_are_declared_exported_bound_and_mirrored():
    text = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert re.search(r"#define\s+BISBM_SETTLED_BY_ENTROPY\s+0u", code) and re.search(r"#define\s+BISBM_SETTLED_BY_STAY\s+1u", code)
    assert (B.SETTLED_BY_ENTROPY, B.SETTLED_BY_STAY) == (0, 1)
    # what the existing tests pin stays: the prefix's fixed list, the two sentences, the ABI version
    assert not [f for f in re.findall(r"\b(bisbm_conditionals_[a-z_]+)\s*\(", code) if "held" in f or "settled" in f]
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    assert "bisbm_conditionals_* keeps reporting the UNRESTRICTED row" in text
    assert "bisbm_conditionals_* keeps reporting the UNRESTRICTED row (unless bisbm_held_conditionals_set is on" in flat
    assert "keeps reporting the model's row (the heat-bath row is that row plus the field) (unless bisbm_held_conditionals_set is on" in flat
    assert "node conditionals (bisbm_conditionals_*)" in flat
    assert re.search(r"#define\s+BISBM_ABI_VERSION\s+3\b", code)
    assert "top-k of the least settled nodes on the device (with n doubles" not in flat
    if not os.path.exists(B.LIB_PATH):
        B.build()
    raw = C.CDLL(B.LIB_PATH)
    for name in CALLS + ["bisbm_debug_log"]:  # (the device's logarithm for the host statement: beside bisbm_debug_exp)
        assert hasattr(raw, name), "libbisbm_hip.so does not export %s" % name
        assert name in B.ABI
    assert re.search(r"\bint\s+bisbm_debug_log\s*\(", code) and callable(B.BlockModel.debug_log)
    for method in ("conditionals_held", "conditionals_is_held", "least_settled"):
        assert callable(getattr(B.BlockModel, method))
    assert B.numpy_held_conditional_row is D.numpy_held_conditional_row and B.numpy_least_settled is D.numpy_least_settled
    mirror = open(os.path.join(PKG, "host", "bisbm.hpp")).read()
    for name in CALLS:
        assert name in mirror, "host/bisbm.hpp does not wrap %s" % name


class _Untouched:
    """a model no call may reach: marginalize refuses before anything is set or run"""

    def __getattr__(self, name):
        raise AssertionError("the model was touched: %s" % name)


@pytest.mark.parametrize("fn", ["marginalize", "marginalize_modes"])
def test_marginalize_refuses_the_extras_without_conditionals(fn):
    call = getattr(B, fn)
    kw = {"threshold": 0.5} if fn == "marginalize_modes" else {}
    with pytest.raises(ValueError, match="conditionals="):
        call(_Untouched(), 1, 1, 1, conditionals_held=True, **kw)
    with pytest.raises(ValueError, match="conditionals="):
        call(_Untouched(), 1, 1, 1, least_settled=(3, "stay"), **kw)
    with pytest.raises(ValueError, match="least_settled must be"):
        call(_Untouched(), 1, 1, 1, conditionals=(None,), least_settled=(3, "margin"), **kw)


def test_the_command_line_refuses_the_flags_without_conditionals(tmp_path):
    cli = os.path.join(PKG, "bin", "mcmc")
    if not os.path.exists(cli):
        B.build()
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    base = [cli, "-e", el, "-y", "500", "500", "-z", "4", "6", "--marginalize"]
    r = subprocess.run(base + ["--conditionals_held"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--conditionals_held" in r.stderr and "it needs --conditionals." in r.stderr and r.stdout == ""
    r = subprocess.run(base + ["--least_settled", str(tmp_path / "o.txt"), "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--least_settled" in r.stderr and "it needs --conditionals." in r.stderr and r.stdout == ""
    q = tmp_path / "q.txt"
    q.write_text("0\n1\n")
    cond = ["--conditionals", str(q), str(tmp_path / "c.txt")]
    for bad in (["3"], [str(tmp_path / "o.txt")], [str(tmp_path / "o.txt"), "0"], [str(tmp_path / "o.txt"), "1025"],
                [str(tmp_path / "o.txt"), "3", "margin"], [str(tmp_path / "o.txt"), "x"]):
        r = subprocess.run(base + cond + ["--least_settled"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Invalid --least_settled." in r.stderr and r.stdout == "", (bad, r.stderr)
    assert not (tmp_path / "o.txt").exists() and not (tmp_path / "c.txt").exists()
    help_text = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert "--conditionals_held" in help_text.stdout + help_text.stderr and "--least_settled OUT K" in help_text.stdout + help_text.stderr
