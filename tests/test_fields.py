"""Block fields (include/bisbm.h, "Block fields") without a device: the declarations and the binding, the host statements the GPU
tests hold the kernels to (numpy_field_energy, numpy_field_row) against literal loops, the pure helper fields_from_weights, the
loader of the fields file and the refusals of the command line that need no device."""
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

NEW = ("bisbm_fields_set", "bisbm_fields_get", "bisbm_fields_energy", "bisbm_io_read_fields")


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_declares_the_calls_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "bisbm.h")).read()
    assert re.search(r"#define\s+BISBM_ABI_VERSION\s+3\b", text)
    assert re.search(r"\bint\s+bisbm_fields_set\s*\(\s*bisbm_handle\s+h\s*,\s*uint32_t\s+n_classes\s*,\s*const\s+uint8_t\s*\*\s*class_of_node[^;]*"
                     r"const\s+double\s*\*\s*field", text)
    assert re.search(r"\bint\s+bisbm_fields_get\s*\(\s*bisbm_handle\s+h\s*,\s*uint32_t\s*\*\s*n_classes_out\s*,\s*uint8_t\s*\*\s*class_of_node_out\s*,"
                     r"\s*double\s*\*\s*field_out", text)
    assert re.search(r"\bint\s+bisbm_fields_energy\s*\(\s*bisbm_handle\s+h\s*,\s*double\s*\*\s*out", text)
    assert "Block fields" in text and "delta cum = delta S + delta Phi" in text and "tilted target" in text
    assert "bisbm_io_read_fields" in open(os.path.join(ROOT, "include", "bisbm_io.h")).read()
    for name in NEW:
        assert name in B.ABI
    L = B.lib()  # (every symbol of the table is bound, or this raises)
    assert L.bisbm_abi_version() == 3
    for name in ("set_fields", "clear_fields", "fields", "field_energy"):
        assert callable(getattr(B.BlockModel, name))
    for name in ("fields_from_weights", "numpy_field_energy", "numpy_field_row", "load_fields"):
        assert callable(getattr(B, name))
    mirror = open(os.path.join(PKG, "host", "bisbm.hpp")).read()
    for name in ("set_fields", "clear_fields", "field_energy", "load_fields"):
        assert name in mirror


def test_every_new_symbol_is_exported_and_the_unit_is_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libbisbm_hip.so")], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r" T %s$" % name, out, re.M), name
    build = importlib.import_module("bipartitesbm-mcmc_amd.build")
    assert "bisbm_fields.hip" in build.SOURCES
    assert "bisbm_fields.hip" in open(os.path.join(PKG, "csrc", "bisbm_engine.hpp")).read()


# ------------------------------------------------------------------------------------------------------ the host models
def test_numpy_field_energy_is_the_loop_of_the_definition():
    rng = np.random.default_rng(3)
    na, nb, ka, kb = 7, 5, 3, 2
    labels = np.concatenate([rng.integers(0, ka, na), ka + rng.integers(0, kb, nb)])
    cls = rng.integers(0, 4, na + nb)
    cls[cls == 2] = 0  # (class 2 is empty)
    field = rng.normal(size=(4, ka + kb))
    field[:, 1] = [0.1, 1e16, -1e16, 0.3]  # (an order of the adds that shows)
    count = {}
    for v in range(na + nb):
        count[(int(cls[v]), int(labels[v]))] = count.get((int(cls[v]), int(labels[v])), 0) + 1
    phi = 0.0
    for c in range(4):
        for b in range(ka + kb):
            if count.get((c, b)):
                phi = phi + float(count[(c, b)]) * float(field[c, b])
    got = B.numpy_field_energy(labels, cls, field, na, ka)
    assert isinstance(got, float) and np.float64(got).tobytes() == np.float64(phi).tobytes()
    assert B.numpy_field_energy(labels, cls, np.zeros((4, 5)), na, ka) == 0.0
    # an entry of the other type's range is never counted
    other = field.copy()
    other[:, :] = 0.0
    other[0, ka:] = 5.0
    only_a = np.zeros(na + nb, dtype=np.int64)
    assert B.numpy_field_energy(labels, only_a, other, na, ka) == 5.0 * nb
    bad = labels.copy()
    bad[0] = ka  # (a type-a node in a type-b block)
    with pytest.raises(ValueError):
        B.numpy_field_energy(bad, cls, field, na, ka)


def test_numpy_field_row_adds_the_difference_formed_first():
    row = np.array([0.0, 1e-17, -3.5, 2.25])
    f = np.array([1.0, 1.0 + 2.0 ** -52, 0.25, -1e300])
    for r in range(4):
        got = B.numpy_field_row(row, r, f)
        for s in range(4):
            want = 0.0 if s == r else float(row[s]) + (float(f[s]) - float(f[r]))
            assert np.float64(got[s]).tobytes() == np.float64(want).tobytes(), (r, s)
    # (row + f[s]) - f[r] would round differently: 1e-17 + 1.0000000000000002 loses the 1e-17
    got = B.numpy_field_row(row, 0, f)
    assert got[1] == 1e-17 + 2.0 ** -52 and (row[1] + f[1]) - f[0] != got[1]


# ------------------------------------------------------------------------------------------------- fields_from_weights
def test_fields_from_weights_gives_equal_rows_one_class():
    cls, field = B.fields_from_weights(8, 5, {1: {0: 2.0, 2: 0.5}, 3: {2: 0.5, 0: 2.0}, 4: {1: 3.0}, 6: {3: 1.0}, 7: {4: 0.25}}, na=5, ka=3)
    assert cls.dtype == np.uint8 and cls.tolist() == [0, 1, 0, 1, 2, 0, 0, 3]  # (weight 1 alone is the zero row: class 0)
    assert field.shape == (4, 5) and field.dtype == np.float64 and not field[0].any()
    assert field[1].tolist() == [-math.log(2.0), 0.0, -math.log(0.5), 0.0, 0.0]
    assert field[2].tolist() == [0.0, -math.log(3.0), 0.0, 0.0, 0.0] and field[3, 4] == -math.log(0.25)
    cls, field = B.fields_from_weights(3, 4, {})
    assert cls.tolist() == [0, 0, 0] and field.shape == (1, 4) and not field.any()


def test_fields_from_weights_takes_255_rows_and_refuses_the_256th():
    w = {v: {0: 1.0 + v} for v in range(1, 256)}
    cls, field = B.fields_from_weights(300, 3, w)
    assert field.shape == (256, 3) and cls[255] == 255 and cls[0] == 0 and cls[256:].max() == 0
    w[256] = {0: 1000.0}
    with pytest.raises(ValueError, match="255 distinct rows"):
        B.fields_from_weights(300, 3, w)


def test_fields_from_weights_refusals():
    with pytest.raises(ValueError, match="constrain"):
        B.fields_from_weights(4, 4, {0: {1: 0.0}})
    for w in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite and above 0"):
            B.fields_from_weights(4, 4, {0: {1: w}})
    with pytest.raises(ValueError, match="not in"):
        B.fields_from_weights(4, 4, {4: {1: 2.0}})
    with pytest.raises(ValueError, match="not in"):
        B.fields_from_weights(4, 4, {0: {4: 2.0}})
    with pytest.raises(ValueError, match="other type"):
        B.fields_from_weights(4, 4, {0: {2: 2.0}}, na=2, ka=2)
    with pytest.raises(ValueError, match="other type"):
        B.fields_from_weights(4, 4, {3: {1: 2.0}}, na=2, ka=2)
    B.fields_from_weights(4, 4, {0: {2: 2.0}})  # (without na, ka the row is taken as given)


# ------------------------------------------------------------------------------------------------------------ the loader
def _load(tmp_path, text, na=4, nb=3, ka=3, kb=2):
    path = tmp_path / "fields.txt"
    path.write_text(text)
    return B.load_fields(str(path), na, nb, ka, kb)


def test_the_loader_reads_lines_in_any_order_and_phi_is_minus_log(tmp_path):
    weights = [0.3, 7.0, 1e-3, 2.5e2, 0.9999999, 3.0]
    text = "6 3:%r\t4:%r\n\n0 2:%r 0:%r\n 2  0:%r 2:%r \n5 4:1\n6 4:%r 3:%r\n" % (weights[0], weights[1], weights[2], weights[3], weights[3], weights[2],
                                                                               weights[1], weights[0])
    cls, field = _load(tmp_path, text)
    assert cls.dtype == np.uint8 and cls.tolist() == [2, 0, 2, 0, 0, 0, 1]  # (node 5's weight 1 is the zero row; node 6 repeats its row)
    assert field.shape == (3, 5) and not field[0].any()
    for got, w in ((field[1, 3], weights[0]), (field[1, 4], weights[1]), (field[2, 2], weights[2]), (field[2, 0], weights[3])):
        want = -math.log(w)
        assert abs(got - want) <= math.ulp(want), (got, want)
    a, b = B.fields_from_weights(7, 5, {6: {3: weights[0], 4: weights[1]}, 0: {2: weights[2], 0: weights[3]}, 2: {0: weights[3], 2: weights[2]}}, na=4, ka=3)
    assert sorted(map(bytes, (r.tobytes() for r in b))) == sorted(map(bytes, (r.tobytes() for r in field)))
    assert (b[a] == field[cls]).all()  # (the same row for every node, whatever the class numbering)
    cls, field = _load(tmp_path, "")
    assert cls.tolist() == [0] * 7 and field.shape == (1, 5) and not field.any()
    with pytest.raises(FileNotFoundError):
        B.load_fields(str(tmp_path / "missing.txt"), 4, 3, 3, 2)


@pytest.mark.parametrize("text,names", [
    ("1 0:2\n1 0:3\n", ["'1'", "twice"]),           # a node repeated with another row is an error (the last line does not win)
    ("7 0:2\n", ["'7'", "out of range"]),           # an id >= n
    ("1 5:2\n", ["'5:2'", "out of range"]),         # a block >= K
    ("1 3:2\n", ["'3:2'", "type of node 1"]),       # a block of the other type
    ("5 0:2\n", ["'0:2'", "type of node 5"]),
    ("1 0:0\n", ["'0:0'", "--constraints"]),        # weight 0: that is what constraints are for
    ("1 0:0.0e0\n", ["--constraints"]),
    ("1 0:-2\n", ["'0:-2'", "above 0"]),            # a negative weight
    ("1 0:x\n", ["'0:x'", "not a weight"]),         # a letter
    ("1 0:inf\n", ["'0:inf'", "not a weight"]),
    ("1 0:nan\n", ["not a weight"]),
    ("1 0:1e999\n", ["'0:1e999'", "finite"]),
    ("1 0:\n", ["not a weight"]),
    ("1 a:2\n", ["'a'", "not a block"]),
    ("x 0:2\n", ["'x'", "not a node id"]),
    ("1 0\n", ["'0'", "block:weight"]),
    ("1\n", ["'1'", "no block:weight"]),
    ("1 0:2 0:3\n", ["listed twice"]),
    ("18446744073709551616 0:2\n", ["out of range"]),
])
def test_the_loader_names_the_token_of_a_malformed_line(tmp_path, text, names):
    with pytest.raises(ValueError) as e:
        _load(tmp_path, "0 0:2\n" + text)
    for name in names:
        assert name in str(e.value), (name, str(e.value))
    assert "fields.txt" in str(e.value)


def test_the_loader_refuses_the_256th_distinct_row(tmp_path):
    lines = ["%d 0:%d\n" % (v, v + 2) for v in range(255)]
    cls, field = _load(tmp_path, "".join(lines), na=300, nb=1, ka=1, kb=1)
    assert field.shape == (256, 2) and cls[254] == 255
    with pytest.raises(ValueError, match="256th distinct row"):
        _load(tmp_path, "".join(lines) + "255 0:1000\n", na=300, nb=1, ka=1, kb=1)


# --------------------------------------------------------------------------------------------------------------- the CLI
def test_the_command_line_refuses_fields_without_a_start_or_with_a_merge(tmp_path):
    cli = os.path.join(PKG, "bin", "mcmc")
    el = os.path.join(ROOT, "tests", "golden", "bisbm-n_1000-ka_4-kb_6.edgelist")
    fl = tmp_path / "fields.txt"
    fl.write_text("0 0:2\n")
    base = [cli, "-e", el, "-y", "500", "500", "-z", "4", "6", "--fields", str(fl)]
    r = subprocess.run(base, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--membership_path" in r.stderr and r.stdout == ""
    mb = tmp_path / "labels.txt"
    mb.write_text("0\n")
    for flag in ("--merge", "--nature"):
        r = subprocess.run(base + ["--membership_path", str(mb), flag], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--fields cannot be combined with " + flag in r.stderr and r.stdout == ""
    help_text = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert "--fields PATH" in help_text.stdout + help_text.stderr
