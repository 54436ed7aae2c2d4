"""The four-steps pass of the one-stage kernels takes its pair tests from the feeder wave, on the GPU (-m gpu).

A row of step_quad32 is committed only if its scan found the target the feeder predicted, so the feeder knows every input of a
pair's clash test but the later step's margins and hands the rest over as the pair word (csrc/bisbm_pair_word.hpp;
tests/test_pair_word.py checks the word against the test it replaces on the CPU).  Here the kernel that reads the word -- the pinned
one-stage kernel, BISBM_PASS_DEPTH = 4 and BISBM_ONE_STAGE = 1 -- must give, to the bit, the chain of the per-mover kernel
(BISBM_ONE_STAGE = 0, which still works every pair out in the pass), of two steps per pass, of single steps and chain 0 of the
oracle: rates, counts, sweeps done, labels, m, m_r, n_r, eta and, kept step by step, the bits of the running sum.  With
BISBM_PREDICT_SKEW = 1, 3 and 4 wrong predictions put wrong targets into pair fields; those rows must never reach a commit.
Shapes, calls (a constant one and a cooling one), 4 chains and 3 sweeps are test_gpu_quad32_predicted_target.py's: el32 (32 + 32
blocks, all of eta in LDS), hubs32 (20 + 27, an eta window) and k24_7 (the upper leaf of one type empty).

The precondition, on the CPU from the oracle alone: on each shape passes of depth four commit one, two, three and four steps
(each at least 5 % of the passes -- every position of the new ballot layout is read with an earlier mover in front of it) and at
least 100 shared-block and 100 column clashes occur in three sweeps (both outcomes of the margin test)."""
import numpy as np
import pytest

import oracle_lib as O
import test_gpu_quad32_predicted_target as Q

gpu = pytest.mark.gpu  # (the first test below runs on the CPU)

SHAPES = Q.QUAD32  # hubs32, el32, k24_7


def _fresh_oracle(sid):
    na, nb, ne, ka, kb, _ = Q.SHAPES[sid]
    rowptr, col, labels = Q._graph(sid)
    o = O.OracleModel(rowptr, col, na, nb, ka, kb, 1.0, labels)
    o.seed_philox(Q.SEED, 0)
    o.shuffle_bisbm()
    return o


@pytest.mark.parametrize("sid", SHAPES)
def test_the_shape_exercises_every_pair_position(sid):
    steps, passes, shares = _fresh_oracle(sid).depth_probe(3, 4)
    pairs = _fresh_oracle(sid).pair_probe(3)
    print(sid, "steps", steps, "passes", passes, "shares", ["%.3f" % s for s in shares], "row clashes", pairs["row_clashes"],
          "column clashes", pairs["column_clashes"])
    assert passes > 0 and len(shares) == 4
    assert min(shares) >= 0.05, (sid, shares)
    assert pairs["row_clashes"] >= 100 and pairs["column_clashes"] >= 100, (sid, pairs)


@gpu
@pytest.mark.parametrize("keep", ("0", "1"))
@pytest.mark.parametrize("sid", SHAPES)
def test_the_handed_pair_tests_give_the_same_chain(sid, keep, monkeypatch):
    oracle = Q._oracle(sid)
    refs = [(Q._run(monkeypatch, sid, {"BISBM_PASS_DEPTH": "4", "BISBM_ONE_STAGE": "0"}, keep), 4, "per mover"),
            (Q._run(monkeypatch, sid, {"BISBM_PASS_DEPTH": "2"}, keep), 2, "depth 2"),
            (Q._run(monkeypatch, sid, {"BISBM_SINGLE_STEPS": "1"}, keep), 1, "single steps")]
    for ref, steps, name in refs:
        assert [s["pass_steps"] for s in ref] == [steps] * len(oracle), (sid, keep, name)
    for skew in Q.SKEWS:
        got = Q._run(monkeypatch, sid, dict({"BISBM_PASS_DEPTH": "4", "BISBM_ONE_STAGE": "1"}, **Q._skew_env(skew)), keep)
        assert [s["pass_steps"] for s in got] == [4] * len(oracle), (sid, keep, skew)
        for ref, steps, name in refs:
            Q._same_chains(got, ref, keep, (sid, keep, skew, name))
        for j, want in enumerate(oracle):
            what = (sid, keep, skew, "oracle", j)
            assert got[j]["rates"][0] == want["rate"], what
            assert got[j]["acc"][0] == want["acc"] and got[j]["sweeps"][0] == want["sweeps"], what
            for a, b in zip(got[j]["state"][0], want["state"]):
                assert (np.asarray(a) == np.asarray(b)).all(), what
