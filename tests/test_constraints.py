"""Block constraints (include/bisbm.h, "Block constraints") without a device: the declarations and the binding, the host
statements the GPU tests hold the kernels to (the `allowed=` keyword of distributed.numpy_conditional_row and
numpy_heatbath_choice, distributed.numpy_constrained_shuffle) against literal loops, the pure helpers constraints_from_lists
and admissible_start, the loader of the constraints file, the refusals of the command line that need no device, and the
loader once more as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bipartitesbm-mcmc_amd")
B = importlib.import_module("bipartitesbm-mcmc_amd")
D = B.distributed


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_declares_both_calls_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    assert re.search(r"#define\s+BISBM_ABI_VERSION\s+3\b", text)
    assert re.search(r"\bint\s+bisbm_constraints_set\s*\(\s*bisbm_handle\s+h\s*,\s*uint32_t\s+n_classes\s*,\s*const\s+uint8_t\s*\*\s*class_of_node[^;]*"
                     r"const\s+uint8_t\s*\*\s*allowed", text)
    assert re.search(r"\bint\s+bisbm_constraints_get\s*\(\s*bisbm_handle\s+h\s*,\s*uint32_t\s*\*\s*n_classes_out\s*,\s*uint8_t\s*\*\s*class_of_node_out\s*,"
                     r"\s*uint8_t\s*\*\s*allowed_out", text)
    assert "Block constraints" in text and "bisbm_conditionals_* keeps reporting the UNRESTRICTED row" in text
    io = open(os.path.join(ROOT, "include", "bisbm_io.h")).read()
    assert "bisbm_io_read_constraints" in io
    for name in ("bisbm_constraints_set", "bisbm_constraints_get", "bisbm_io_read_constraints"):
        assert name in B.ABI
    L = B.lib()  # (every symbol of the table is bound, or this raises)
    assert L.bisbm_abi_version() == 3
    for name in ("constrain", "unconstrain", "constraints"):
        assert callable(getattr(B.BlockModel, name))
    for name in ("constraints_from_lists", "admissible_start", "load_constraints"):
        assert callable(getattr(B, name))
    assert callable(D.numpy_constrained_shuffle)


def test_every_new_symbol_is_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libbisbm_hip.so")], capture_output=True, text=True, check=True).stdout
    for name in ("bisbm_constraints_set", "bisbm_constraints_get", "bisbm_io_read_constraints"):
        assert re.search(r" T %s$" % name, out, re.M), name


def test_the_units_list_names_the_new_unit():
    build = importlib.import_module("bipartitesbm-mcmc_amd.build")
    assert "bisbm_constraints.hip" in build.SOURCES
    assert "bisbm_constraints.hip" in open(os.path.join(PKG, "csrc", "bisbm_engine.hpp")).read()


# ------------------------------------------------------------------------------------------------- the restricted row
def _literal_row(dS, r, beta, A):
    """include/bisbm.h, "Block constraints", 2., term by term: (P, the greedy choice)"""
    K = len(dS)
    A = [bool(a) or s == r for s, a in enumerate(A)]
    mn = 0.0
    for s in range(K):
        if A[s] and s != r and dS[s] < mn:
            mn = dS[s]
    w = []
    for s in range(K):
        x = beta * ((0.0 if s == r else dS[s]) - mn)
        w.append(0.0 if (not A[s] or x > 700.0) else math.exp(-x))
    Z = 0.0
    for y in w:
        Z = Z + y
    greedy = r
    if mn < 0.0:
        greedy = min(s for s in range(K) if A[s] and s != r and dS[s] == mn)
    return [y / Z for y in w], greedy


def _draw(P, u, r):
    C, last = 0.0, r
    for s, y in enumerate(P):
        C = C + y
        if y > 0.0:
            last = s
        if u < C:
            return s
    return last


def test_a_row_whose_unrestricted_minimum_lies_outside_the_allowed_blocks():
    dS = np.array([0.0, -5.0, 1.5, -0.25, 2.0])
    r, A = 0, [1, 0, 1, 1, 0]  # (block 1, the minimum of the whole row, is not allowed)
    P, stay, H, margin = D.numpy_conditional_row(dS, r, True, 1.0, allowed=A)
    want, greedy = _literal_row(dS.tolist(), r, 1.0, A)
    assert P[1] == 0.0 and P[4] == 0.0 and not np.signbit(P[[1, 4]]).any()  # exactly +0.0
    assert np.allclose(P, want, rtol=1e-15, atol=0) and stay == P[r] and margin == -0.25
    assert abs(P.sum() - 1.0) < 1e-15 and P[3] > P[0] > P[2] > 0.0
    free_row = D.numpy_conditional_row(dS, r, True, 1.0)[0]
    assert free_row[1] > 0.9  # (without the keyword the row follows block 1)
    assert D.numpy_heatbath_choice(dS, P, r, True, 0.0, True, allowed=A) == greedy == 3
    assert D.numpy_heatbath_choice(dS, P, r, True, 0.0, True) == 1
    for u in (0.0, 0.2, 0.5, 0.9, 1.0 - 2.0 ** -53):
        s = D.numpy_heatbath_choice(dS, P, r, True, u, False, allowed=A)
        assert s == _draw(want, u, r) and A[s]


def test_a_greedy_tie_between_an_allowed_and_a_disallowed_target():
    dS = np.array([-1.0, 0.5, -1.0, 0.0, -1.0])
    r = 3
    assert D.numpy_heatbath_choice(dS, None, r, True, 0.0, True) == 0
    assert D.numpy_heatbath_choice(dS, None, r, True, 0.0, True, allowed=[0, 1, 1, 1, 1]) == 2  # (block 0 ties and is not allowed)
    assert D.numpy_heatbath_choice(dS, None, r, True, 0.0, True, allowed=[0, 1, 0, 1, 0]) == r  # (what is left is uphill)
    assert D.numpy_heatbath_choice(dS, None, r, True, 0.0, True, allowed=[0, 0, 0, 1, 0]) == r  # (one allowed block: held)
    assert D.numpy_heatbath_choice(dS, None, r, True, 0.0, True, allowed=[1, 0, 0, 0, 0]) == 0  # (r itself is always allowed)
    P = D.numpy_conditional_row(dS, r, True, 2.0, allowed=[0, 0, 0, 1, 0])[0]
    assert P.tolist() == [0.0, 0.0, 0.0, 1.0, 0.0]


def test_without_the_keyword_and_with_an_all_allowing_one_the_rows_are_todays():
    rng = np.random.default_rng(3)
    for K in (2, 3, 7, 65):
        for _ in range(20):
            dS = rng.normal(0, 3, K)
            r = int(rng.integers(K))
            dS[r] = 0.0
            beta, u, free = float(rng.uniform(0.2, 3)), float(rng.random()), bool(rng.random() < 0.8)
            base = D.numpy_conditional_row(dS, r, free, beta)
            for allowed in (None, np.ones(K, dtype=np.uint8)):
                got = D.numpy_conditional_row(dS, r, free, beta, allowed=allowed)
                assert got[0].tobytes() == base[0].tobytes() and got[1:] == base[1:]
                for greedy in (False, True):
                    assert D.numpy_heatbath_choice(dS, got[0], r, free, u, greedy, allowed=allowed) == \
                        D.numpy_heatbath_choice(dS, base[0], r, free, u, greedy)
            A = rng.random(K) < 0.5
            P = D.numpy_conditional_row(dS, r, free, beta, allowed=A)[0]
            want, greedy = _literal_row(dS.tolist(), r, beta, A.tolist())
            if free and (A | (np.arange(K) == r)).sum() > 1:
                assert np.allclose(P, want, rtol=1e-14, atol=0) and ((P == 0.0) | A | (np.arange(K) == r)).all()
                assert D.numpy_heatbath_choice(dS, P, r, free, u, True, allowed=A) == greedy
                assert D.numpy_heatbath_choice(dS, P, r, free, u, False, allowed=A) == _draw(P.tolist(), u, r)
            else:
                assert P[r] == 1.0 and P.sum() == 1.0
                assert D.numpy_heatbath_choice(dS, P, r, free, u, False, allowed=A) == r


# ----------------------------------------------------------------------------------------------- the constrained shuffle
def _literal_shuffle(labels, mask, na, cls, perms):
    out = list(labels)
    for t, (lo, hi) in enumerate(((0, na), (na, len(labels)))):
        for c in sorted(set(cls[lo:hi])):
            F = [v for v in range(lo, hi) if not mask[v] and cls[v] == c]
            f = perms.get((t, c), list(range(len(F))))
            assert len(f) == len(F)
            for i in range(len(F)):
                out[F[i]] = labels[F[f[i]]]
    return out


def test_the_constrained_shuffle_is_the_literal_loop():
    rng = np.random.default_rng(11)
    na, nb = 9, 7
    n = na + nb
    labels = np.concatenate([rng.integers(0, 3, na), 3 + rng.integers(0, 2, nb)]).astype(np.uint32)
    #            type a: class 0 x4, class 1 x3 (all clamped: no open node), class 2 x2 (one open)   type b: class 0 x1, class 3 x6
    cls = np.array([0, 1, 0, 2, 1, 0, 2, 1, 0, 3, 3, 0, 3, 3, 3, 3], dtype=np.uint8)
    mask = np.zeros(n, dtype=np.uint8)
    mask[[1, 4, 7, 6, 10]] = 1
    sizes = {(0, 0): 4, (0, 1): 0, (0, 2): 1, (1, 0): 1, (1, 3): 5}
    for _ in range(5):
        perms = {k: rng.permutation(m).tolist() for k, m in sizes.items() if m > 1}
        got = D.numpy_constrained_shuffle(labels, mask, na, cls, perms)
        assert got.tolist() == _literal_shuffle(labels.tolist(), mask.tolist(), na, cls.tolist(), perms)
        assert (got[mask != 0] == labels[mask != 0]).all()
        for t, lo, hi in ((0, 0, na), (1, na, n)):
            for c in np.unique(cls[lo:hi]):  # block sizes are preserved class by class
                sel = np.flatnonzero(cls[lo:hi] == c) + lo
                assert (np.bincount(got[sel], minlength=5) == np.bincount(labels[sel], minlength=5)).all()
        full = dict(perms)
        full[(0, 2)], full[(1, 0)], full[(0, 1)] = [0], [0], []  # (entries for the classes of one and of no open node change nothing)
        assert (D.numpy_constrained_shuffle(labels, mask, na, cls, full) == got).all()
    assert (D.numpy_constrained_shuffle(labels, None, na, np.zeros(n, dtype=np.uint8), {(0, 0): np.arange(na)[::-1], (1, 0): np.arange(nb)}) ==
            np.concatenate([labels[:na][::-1], labels[na:]])).all()
    one = D.numpy_constrained_shuffle(labels, mask, na, np.zeros(n, dtype=np.uint8), {(0, 0): np.arange(5)[::-1], (1, 0): np.arange(6)})
    assert (one == D.numpy_clamped_shuffle(labels, mask, na, np.arange(5)[::-1], np.arange(6))).all()  # (one class: the clamped shuffle)
    with pytest.raises(ValueError):
        D.numpy_constrained_shuffle(labels, mask, na, cls, {(0, 0): [0, 1, 2], (1, 3): list(range(5))})
    with pytest.raises(ValueError):
        D.numpy_constrained_shuffle(labels, mask, na, cls, {(0, 0): [0, 0, 1, 2], (1, 3): list(range(5))})


# ------------------------------------------------------------------------------------------------------ the pure helpers
def test_constraints_from_lists_turns_distinct_lists_into_classes():
    cls, allowed = B.constraints_from_lists(8, 5, {5: [3], 1: [0, 1], 2: [1, 0, 1], 7: [0, 1, 2, 3, 4], 6: [4, 3]})
    assert cls.dtype == np.uint8 and cls.tolist() == [0, 1, 1, 0, 0, 2, 3, 0]  # (node 7 lists everything: class 0)
    assert allowed.dtype == bool and allowed.astype(int).tolist() == [[1, 1, 1, 1, 1], [1, 1, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 1, 1]]
    cls, allowed = B.constraints_from_lists(8, 5, {5: [3], 1: [0, 1], 6: [3, 4]}, na=4, ka=3)  # (typed: the other type's columns set)
    assert cls.tolist() == [0, 1, 0, 0, 0, 2, 0, 0]  # (3 and 4 are all of type b: node 6 is class 0)
    assert allowed.astype(int).tolist() == [[1, 1, 1, 1, 1], [1, 1, 0, 1, 1], [1, 1, 1, 1, 0]]
    cls, allowed = B.constraints_from_lists(4, 3, {})
    assert cls.tolist() == [0, 0, 0, 0] and allowed.tolist() == [[True, True, True]]
    for bad in ({9: [0]}, {1: []}, {1: [5]}, {1: [-1]}):
        with pytest.raises(ValueError):
            B.constraints_from_lists(8, 5, bad)
    with pytest.raises(ValueError):
        B.constraints_from_lists(8, 5, {1: [3]}, na=4, ka=3)


def _lists(count):
    return {v: [b for b in range(9) if (v + 1) >> b & 1] for v in range(count)}


def test_255_distinct_lists_fit_and_257_raise():
    cls, allowed = B.constraints_from_lists(300, 10, _lists(255))
    assert allowed.shape == (256, 10) and cls[:255].tolist() == list(range(1, 256)) and not cls[255:].any()
    for count in (256, 257):  # (class 0 is one of the 256 class ids)
        with pytest.raises(ValueError):
            B.constraints_from_lists(300, 10, _lists(count))


def test_admissible_start_deals_every_class_over_its_blocks():
    na, nb, ka, kb = 7, 5, 3, 2
    cls = np.array([0, 1, 1, 0, 2, 1, 0, 0, 3, 3, 0, 3], dtype=np.uint8)
    allowed = np.array([[1, 1, 1, 1, 1], [0, 1, 1, 1, 1], [1, 0, 0, 0, 0], [1, 1, 1, 0, 1]], dtype=bool)
    lab = B.admissible_start(na, nb, ka, kb, cls, allowed)
    assert lab.dtype == np.uint32
    assert lab.tolist() == [0, 1, 2, 1, 0, 1, 2, 3, 4, 4, 4, 4]
    assert all(allowed[cls[v], lab[v]] for v in range(na + nb)) and (lab[:na] < ka).all() and (lab[na:] >= ka).all()
    with pytest.raises(ValueError, match="empty"):  # nobody may sit in block 2
        B.admissible_start(3, 2, 3, 2, np.zeros(5, dtype=np.uint8), np.array([[1, 1, 0, 1, 1]]))
    with pytest.raises(ValueError, match="no block"):
        B.admissible_start(3, 2, 3, 2, np.zeros(5, dtype=np.uint8), np.array([[0, 0, 0, 1, 1]]))


# ------------------------------------------------------------------------------------------------------------ the loader
def _write(tmp_path, text):
    p = tmp_path / "constraints.txt"
    p.write_text(text)
    return str(p)


NA, NB, KA, KB = 6, 4, 3, 2


def test_the_loader_takes_lines_in_any_order_and_a_node_repeated_with_the_same_blocks(tmp_path):
    cls, allowed = B.load_constraints(_write(tmp_path, "7 4\n\n 0 1\t0 \r\n3  2\n0 0 1\n9 4"), NA, NB, KA, KB)
    assert cls.dtype == np.uint8 and cls.tolist() == [2, 0, 0, 3, 0, 0, 0, 1, 0, 1]
    assert allowed.dtype == bool and allowed.astype(int).tolist() == [[1, 1, 1, 1, 1], [1, 1, 1, 0, 1], [1, 1, 0, 1, 1], [0, 0, 1, 1, 1]]
    lists = {7: [4], 0: [0, 1], 3: [2], 9: [4]}  # the pure helper gives the same classes up to their numbering
    c2, a2 = B.constraints_from_lists(NA + NB, KA + KB, lists, na=NA, ka=KA)
    assert (a2[c2] == allowed[cls]).all()


def test_an_empty_file_constrains_nobody(tmp_path):
    for text in ("", "\n", "  \n\t\r\n"):
        cls, allowed = B.load_constraints(_write(tmp_path, text), NA, NB, KA, KB)
        assert cls.tolist() == [0] * 10 and allowed.tolist() == [[True] * 5]


@pytest.mark.parametrize("text,token", [
    ("1 0\n10 3\n", "10"),                                        # an id >= n
    ("1 0\n2 5\n", "5"),                                          # a block >= K
    ("1 0\n2 3\n", "3"),                                          # a block of the other type
    ("7 1\n", "1"),
    ("1 0\nx2 1\n", "x2"),                                        # a letter
    ("1 0\n2 1a\n", "1a"),
    ("1 -0\n", "-0"),
    ("18446744073709551616 0\n", "18446744073709551616"),         # 2^64
    ("1 99999999999999999999999\n", "99999999999999999999999"),
    ("1 0\n1 1\n", "1"),                                          # a repeat with a different list
    ("4\n", "4"),                                                 # no block at all
])
def test_the_loader_rejects_a_malformed_line_and_names_the_token(tmp_path, text, token):
    with pytest.raises(ValueError) as e:
        B.load_constraints(_write(tmp_path, text), NA, NB, KA, KB)
    assert "'%s'" % token in str(e.value), str(e.value)


def test_the_loader_reports_a_file_that_is_not_there(tmp_path):
    with pytest.raises(FileNotFoundError):
        B.load_constraints(str(tmp_path / "none.txt"), NA, NB, KA, KB)


def test_the_loader_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "sanitize_constraints")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-pthread", "-o", exe, os.path.join(ROOT, "tests", "native", "sanitize_constraints.cpp"), os.path.join(PKG, "csrc", "bisbm_io.cpp")],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])


# -------------------------------------------------------------------------------------------------------- the command line
CLI = os.path.join(PKG, "bin", "mcmc")
EL = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
BASE = ["-e", EL, "-y", "500", "500", "-z", "3", "3", "-n", "167", "167", "166", "167", "167", "166", "--rng", "philox"]


def _labels_file(tmp_path):
    p = tmp_path / "labels.txt"
    p.write_text("".join("%d\n" % (v * 3 // 500 if v < 500 else 3 + (v - 500) * 3 // 500) for v in range(1000)))
    return str(p)


def test_help_lists_the_flag():
    if not os.path.exists(CLI):
        B.build()
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    assert "--constraints PATH" in r.stdout + r.stderr


def test_the_command_line_refuses_constraints_without_a_membership_file(tmp_path):
    if not os.path.exists(CLI):
        B.build()
    r = subprocess.run([CLI] + BASE + ["--marginalize", "--constraints", _write(tmp_path, "1 0 1\n")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    assert "--constraints" in r.stderr and "--membership_path" in r.stderr, r.stderr


@pytest.mark.parametrize("flag", ["--merge", "--nature"])
def test_the_command_line_refuses_constraints_with_a_merge(tmp_path, flag):
    if not os.path.exists(CLI):
        B.build()
    r = subprocess.run([CLI] + BASE + ["--membership_path", _labels_file(tmp_path), "--constraints", _write(tmp_path, "1 0 1\n"), flag],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    assert "--constraints" in r.stderr and flag in r.stderr, r.stderr


def test_the_command_line_names_the_token_of_a_malformed_file(tmp_path):
    if not os.path.exists(CLI):
        B.build()
    r = subprocess.run([CLI] + BASE + ["--membership_path", _labels_file(tmp_path), "--constraints", _write(tmp_path, "1 0 1\n2 7x\n")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    assert "--constraints" in r.stderr and "'7x'" in r.stderr, r.stderr


def test_the_command_line_refuses_constraints_in_compat_mode(tmp_path):
    if not os.path.exists(CLI):
        B.build()
    args = [a for a in BASE if a not in ("--rng", "philox")] + ["--rng", "mt19937-compat"]
    r = subprocess.run([CLI] + args + ["--membership_path", _labels_file(tmp_path), "--constraints", _write(tmp_path, "1 0 1\n")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    assert "--constraints" in r.stderr and "--rng philox" in r.stderr, r.stderr
