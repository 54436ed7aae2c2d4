"""One held Metropolis-Hastings sweep on the host, written out in Python from the oracle's pieces (no GPU, no product code): a
second, literal implementation of the step include/bisbm.h defines under a clamp, block constraints and block fields.  Shared by
tests/test_gpu_fields.py (the device against this replay) and tests/test_oracle_holds.py (orc_anneal against it)."""
import numpy as np

import oracle_lib as O
from test_tempering import philox, u53

INF = float("inf")


def visit(seed, gid, sweep, na, nb):
    L = O.lib()
    return [int(L.orc_philox_visit(seed, gid, sweep, na, nb, i)) for i in range(na + nb)]


def mh_replay_sweep(probe, lab, cls, field, gid, sweep, T, na, nb, ka, seed, exp, clamp=None, constraints=None):
    """One MH sweep on the host, from the oracle's pieces: the proposal from propose_philox with the step's draws, dS and the
    Hastings factor from transition_ratio, dE = dS + (f[s] - f[r]) where a field is given (cls, field; None for none), the accept
    uniform of the step.  clamp: a boolean mask, a clamped node's step is one that was not accepted.  constraints: (class_of_node,
    allowed[n_classes][K]); a target of the node's type that is not its own block and not allowed is not evaluated.  `probe` is an
    oracle model WITHOUT holds used for its state alone.  Returns (labels, accepted, the smallest relative distance of the two sides
    of an accept test, whether some decision differs from the one dS alone gives)."""
    n = na + nb
    lab = lab.copy()
    Tf = float(np.float32(T))
    probe.set_memberships(lab.astype(np.uint32))
    probe.init_bisbm()
    accepted, margin, differs = 0, INF, False
    for p, v in enumerate(visit(seed, gid, sweep, na, nb)):
        if clamp is not None and clamp[v]:
            continue
        A, Bw = philox(seed, gid, 0, sweep * n + p), philox(seed, gid, 1, sweep * n + p)
        s = int(probe.propose_philox(v, u53(A[0], A[1]), u53(A[2], A[3]), u53(Bw[0], Bw[1])))
        r = int(lab[v])
        u_acc = u53(Bw[2], Bw[3])
        if s == r:
            accepted += int(probe.n_r()[r] > 1)  # (u < 1: accepted unless the veto of a node alone in its block)
            continue
        if (s < ka) != (r < ka):
            continue
        if constraints is not None and not constraints[1][constraints[0][v]][s]:
            continue
        dS, accu_r = probe.transition_ratio(v, s)
        dE = dS
        if field is not None:
            f = field[cls[v]]
            dE = dS + (float(f[s]) - float(f[r]))
        rhs = accu_r * exp(-dE * (1.0 / Tf))
        plain = u_acc < accu_r * exp(-dS * (1.0 / Tf))
        margin = min(margin, abs(u_acc - rhs) / max(u_acc, rhs))
        differs = differs or (plain != (u_acc < rhs))
        if u_acc < rhs and probe.n_r()[r] > 1:
            lab[v] = s
            accepted += 1
            probe.set_memberships(lab.astype(np.uint32))
            probe.init_bisbm()
    return lab, accepted, margin, differs

