"""Heat-bath sweeps and pair reshuffles inside replica exchange (include/bisbm.h, "Heat-bath sweeps and pair reshuffles inside
replica exchange") without a device: the Python-side checks of a round recipe and of the `rung_moves` keyword, the combinations
that keep raising, the numpy model of the per-rung tally that the GPU tests hold bisbm_tempering_rung_stats to, the declared
symbols and the CLI's refusals."""
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = importlib.import_module("bipartitesbm-mcmc_amd")


class _NoSweeps:
    """a model that must not be asked to run anything"""
    n, shard, n_chains = 10, None, 4

    def __getattr__(self, name):
        raise AssertionError("the model was touched: " + name)


# ---------------------------------------------------------------------------------------------------- recipe and keyword
def test_round_recipe():
    r = B.round_recipe(1, 0, 2, 3)
    assert (r.mh_sweeps, r.heatbath_sweeps, r.reshuffles, r.reshuffle_scans) == (1, 0, 2, 3)
    r = B.round_recipe(mh=0, heatbath=np.int64(4), reshuffles=0, scans=0)
    assert (r.mh_sweeps, r.heatbath_sweeps, r.reshuffles, r.reshuffle_scans) == (0, 4, 0, 0)
    for bad, what in (((0, 0, 0, 3), "runs nothing"), ((-1, 0, 1, 3), "outside"), ((1, 0, 1, 1 << 32), "outside"),
                      ((1.5, 0, 0, 3), "not an integer"), ((1, True, 0, 3), "not an integer")):
        with pytest.raises(ValueError) as e:
            B.round_recipe(*bad)
        assert what in str(e.value), (bad, str(e.value))


def test_rung_moves_keyword():
    assert B.rung_moves_recipe({}) == {"mh": 1, "heatbath": 0, "reshuffles": 0, "scans": 3}
    assert B.rung_moves_recipe({"mh": 0, "heatbath": 2}) == {"mh": 0, "heatbath": 2, "reshuffles": 0, "scans": 3}
    for bad, what in (({"mh": 0}, "runs nothing"), ({"sweeps": 1}, "unknown keys"), ([1, 0, 2, 3], "must be a dict"),
                      ({"reshuffles": -2}, "outside")):
        with pytest.raises(ValueError) as e:
            B.rung_moves_recipe(bad)
        assert what in str(e.value), (bad, str(e.value))


def test_rung_moves_needs_a_ladder():
    moves = {"mh": 1, "reshuffles": 2}
    with pytest.raises(ValueError, match="needs tempering"):
        B.marginalize(_NoSweeps(), 1, 1, 1, rung_moves=moves)
    with pytest.raises(ValueError, match="needs tempering"):
        B.marginalize_modes(_NoSweeps(), 1, 1, 1, 0.1, rung_moves=moves)
    with pytest.raises(ValueError, match="runs nothing"):  # (a bad recipe is refused before the ladder is set)
        B.marginalize(_NoSweeps(), 1, 1, 1, tempering=[1.0, 2.0], rung_moves={"mh": 0})
    with pytest.raises(ValueError, match="unknown keys"):
        B.population_anneal(_NoSweeps(), [2.0, 1.0], 1, rung_moves={"hb": 1})


def test_the_old_combinations_still_raise_and_point_to_rung_moves():
    with pytest.raises(ValueError, match="rung_moves"):
        B.marginalize(_NoSweeps(), 1, 1, 1, tempering=[1.0, 2.0], reshuffles=2)
    with pytest.raises(ValueError, match="rung_moves"):
        B.marginalize(_NoSweeps(), 1, 1, 1, tempering=[1.0, 2.0], sampler="heatbath")
    with pytest.raises(ValueError, match="rung_moves"):
        B.marginalize_modes(_NoSweeps(), 1, 1, 1, 0.1, reassign=True, sampler="heatbath", tempering=[1.0, 2.0])
    # ... also when rung_moves is given beside them
    with pytest.raises(ValueError, match="tempering"):
        B.marginalize(_NoSweeps(), 1, 1, 1, tempering=[1.0, 2.0], reshuffles=2, rung_moves={"mh": 1})


# ---------------------------------------------------------------------------------------------------- the tally
def test_numpy_rung_tally():
    """Every chain's deltas go to the row of the rung it holds; scalars stand for one value per chain."""
    L = 3
    stats = np.zeros((L, 6), dtype=np.uint64)
    rung = np.array([0, 1, 2, 2, 0, 1])
    B.numpy_rung_tally(stats, rung, mh_steps=10, mh_accepted=[1, 2, 3, 4, 5, 6], heatbath_steps=20, heatbath_moves=[6, 5, 4, 3, 2, 1],
                       reshuffles=2, reshuffles_accepted=[0, 1, 0, 1, 2, 0])
    assert stats.tolist() == [[20, 6, 40, 8, 4, 2], [20, 8, 40, 6, 4, 1], [20, 7, 40, 7, 4, 1]]
    # a second round after an exchange of rungs 0 and 1 in both ensembles, MH only: the other columns stay
    B.numpy_rung_tally(stats, np.array([1, 0, 2, 2, 1, 0]), mh_steps=10, mh_accepted=[1, 1, 1, 1, 1, 1])
    assert stats.tolist() == [[40, 8, 40, 8, 4, 2], [40, 10, 40, 6, 4, 1], [40, 9, 40, 7, 4, 1]]
    assert stats[:, 0].sum() == 2 * 6 * 10
    assert B.RUNG_STAT_COLUMNS == ("mh_steps", "mh_accepted", "heatbath_steps", "heatbath_moves", "reshuffles", "reshuffles_accepted")


# ---------------------------------------------------------------------------------------------------- symbols
def test_declared_symbols_are_bound_and_refuse_a_null_handle():
    for name in ("bisbm_tempering_run_rounds", "bisbm_tempering_rung_stats", "bisbm_rounds_population_run"):
        assert name in B.ABI
    L = B.lib()
    rec = B.round_recipe(1, 1, 1, 1)
    import ctypes as C
    assert L.bisbm_tempering_run_rounds(None, 1, C.byref(rec), 1) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_tempering_rung_stats(None, None) == B.BISBM_ERR_INVALID_ARG
    assert L.bisbm_rounds_population_run(None, 0, None, 1, C.byref(rec), None, None, None) == B.BISBM_ERR_INVALID_ARG
    assert C.sizeof(B.RoundRecipe) == 16
    hpp = open(os.path.join(ROOT, "bipartitesbm-mcmc_amd", "host", "bisbm.hpp")).read()
    assert "bisbm_tempering_run_rounds" in hpp and "bisbm_rounds_population_run" in hpp and "bisbm_tempering_rung_stats" in hpp


# ---------------------------------------------------------------------------------------------------- CLI
def _cli():
    cli = os.path.join(ROOT, "bipartitesbm-mcmc_amd", "bin", "mcmc")
    if not os.path.exists(cli):
        B.build(force=True)
    return cli


GRAPH = ["-e", os.path.join(ROOT, "tests", "golden", "southernWomen.edgelist"), "-y", "18", "14", "-z", "2", "2", "-n", "9", "9", "7", "7"]
INVALID = "Invalid --%s. Four integers >= 0, MH HB RS SCANS, not all of MH HB RS zero, e.g. --%s 1 0 2 3.\n"


@pytest.mark.parametrize("args, message", [
    (["--marginalize", "--rung_moves", "1", "0", "2", "3"], "--rung_moves sets the moves of a round of --tempering: it needs --tempering.\n"),
    (["--population_moves", "1", "0", "2", "3"], "--population_moves sets the moves of a round of --population: it needs --population.\n"),
    (["--marginalize", "--tempering", "1", "2", "--rung_moves", "1", "0", "2"], INVALID % ("rung_moves", "rung_moves")),
    (["--marginalize", "--tempering", "1", "2", "--rung_moves", "0", "0", "0", "3"], INVALID % ("rung_moves", "rung_moves")),
    (["--marginalize", "--tempering", "1", "2", "--rung_moves", "1", "x", "2", "3"], INVALID % ("rung_moves", "rung_moves")),
    (["--marginalize", "--tempering", "1", "2", "--rung_moves", "1", "-1", "2", "3"], INVALID % ("rung_moves", "rung_moves")),
    (["--population", "2", "1", "--population_moves", "0", "0", "0", "0"], INVALID % ("population_moves", "population_moves")),
])
def test_cli_refusals(args, message):
    """Refused with one line before the device is touched."""
    r = subprocess.run([_cli()] + GRAPH + args, capture_output=True, text=True, timeout=120)
    assert (r.returncode, r.stdout) == (1, "")
    assert r.stderr.endswith(message), r.stderr


def test_cli_still_refuses_the_old_combinations_and_names_the_new_flag():
    for extra in (["--heatbath"], ["--reshuffle", "2"]):
        r = subprocess.run([_cli()] + GRAPH + ["--marginalize", "--tempering", "1", "2", "--chains", "2", "--rng", "philox"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert (r.returncode, r.stdout) == (1, "")
        assert extra[0] in r.stderr and "--tempering" in r.stderr and "--rung_moves" in r.stderr, r.stderr


def test_cli_help_names_the_flags():
    r = subprocess.run([_cli(), "--help"], capture_output=True, text=True, timeout=120)
    assert "--rung_moves MH HB RS SCANS" in r.stderr and "--population_moves MH HB RS SCANS" in r.stderr
