"""Chain sharding over the GPUs of one node (one process per GPU, torch.distributed; backend
"nccl" is RCCL over xGMI on ROCm, "gloo" in CPU tests).

The reference is single-chain and single-process (no parallel axis exists); the
engine adds exactly one: independent chains.  Chains never exchange anything during sweeps, so the
sweep kernels run with no collective.  Collectives appear only where chains are pooled:

  * all_gather of per-chain scalars (sum dS / description length, acceptance rate, counts);
  * marginals: every rank histograms its own chains into counts[n, kmax]; the pooled histogram is a
    reduce_scatter over node ranges, the MAP label an argmax on each rank's node range, the full
    label vector an all_gather of uint8 labels (int32 above 256 blocks).  On the fully connected xGMI topology
    a reduce_scatter moves 1/world of the buffer per link concurrently instead of a ring's
    per-link-bound all_reduce.

A chain's random stream is keyed by its GLOBAL chain id, so results do not depend on world_size.
"""
import numpy as np


def shard_chains(total_chains, world_size, rank):
    """Contiguous chain range of `rank`: returns (first_chain_id, n_local).  The first
    total % world ranks get one extra chain."""
    if world_size < 1 or not (0 <= rank < world_size):
        raise ValueError("bad rank/world_size")
    base, extra = divmod(int(total_chains), int(world_size))
    n_local = base + (1 if rank < extra else 0)
    first = rank * base + min(rank, extra)
    return first, n_local


def _dist():
    import torch.distributed as dist
    return dist


class ChainShard:
    """The chains one rank owns, plus the pooling collectives.

    `group` is a torch.distributed process group (None = default).  All tensors passed in must
    live on the device the backend needs (CUDA/HIP for nccl, CPU for gloo)."""

    def __init__(self, total_chains, rank=None, world_size=None, group=None):
        dist = _dist()
        self.group = group
        if world_size is None:
            world_size = dist.get_world_size(group) if dist.is_initialized() else 1
        if rank is None:
            rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.rank, self.world_size = int(rank), int(world_size)
        self.total_chains = int(total_chains)
        self.first_chain_id, self.n_local = shard_chains(total_chains, world_size, rank)
        self.counts = [shard_chains(total_chains, world_size, r)[1] for r in range(world_size)]

    # -- per-chain scalars ------------------------------------------------------------------
    def all_gather_chain_values(self, local):
        """local: tensor [n_local, ...] -> tensor [total_chains, ...] in global chain order."""
        import torch
        dist = _dist()
        if self.world_size == 1:
            return local.clone()
        pad = max(self.counts)
        buf = torch.zeros((pad,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        buf[: self.n_local] = local
        out = [torch.empty_like(buf) for _ in range(self.world_size)]
        dist.all_gather(out, buf, group=self.group)
        return torch.cat([o[:c] for o, c in zip(out, self.counts)], dim=0)

    # -- marginals --------------------------------------------------------------------------
    def lowest_chain_labels(self, model):
        """(global chain id, labels uint32 [n]) of the chain of the lowest description length over all ranks (ties -> the
        lowest global chain id): the reference partition of an aligned marginalisation.  The description lengths are
        all-gathered, the owning rank broadcasts the chain's labels.  With replica exchange on (model.set_tempering) only the
        chains on rung 0 compete."""
        import torch
        dist = _dist()
        dev = _collective_device(self)
        S = np.asarray(model.entropy(), dtype=np.float64).reshape(-1)
        if getattr(model, "tempering_L", 0):
            S = np.where(model.tempering_state()[0] == 0, S, np.inf)
        local = torch.as_tensor(S)
        allv = self.all_gather_chain_values(local.to(dev)).cpu().numpy()
        best = int(np.argmin(allv))  # (the first minimum: the lowest global chain id among ties)
        owner = next(r for r in range(self.world_size) if best < sum(self.counts[: r + 1]))
        if owner == self.rank:
            lab = torch.as_tensor(np.asarray(model.get_memberships(best - self.first_chain_id), dtype=np.int64)).to(dev)
        else:
            lab = torch.zeros(model.n, dtype=torch.int64, device=dev)
        if self.world_size > 1:
            src = dist.get_global_rank(self.group, owner) if self.group is not None else owner
            dist.broadcast(lab, src=src, group=self.group)
        return best, lab.cpu().numpy().astype(np.uint32)

    def node_range(self, n, rank=None):
        """Node rows [lo, hi) of the pooled histogram that `rank` reduces in map_labels (the n % world last rows are
        summed on every rank)."""
        rank = self.rank if rank is None else rank
        per = n // self.world_size
        return rank * per, (rank + 1) * per

    def pooled_marginals(self, local_counts):
        """all_reduce(sum) of counts[n, kmax] (int32): every rank gets the pooled histogram."""
        dist = _dist()
        out = local_counts.clone()
        if self.world_size > 1:
            dist.all_reduce(out, op=dist.ReduceOp.SUM, group=self.group)
        return out

    def pooled_pair_scores(self, model):
        """(sum float64 [P], terms) of the pair scores over all ranks: every rank's own sums (model.pair_scores(): the chains
        it owns) and term counts are all-reduced.  Every rank must have set the same pairs."""
        import torch
        dist = _dist()
        local, terms = model.pair_scores()
        if self.world_size == 1:
            return local, terms
        dev = _collective_device(self)
        s = torch.as_tensor(local).to(dev)
        t = torch.tensor([terms], dtype=torch.int64, device=dev)
        dist.all_reduce(s, op=dist.ReduceOp.SUM, group=self.group)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return s.cpu().numpy(), int(t.item())

    def map_labels(self, local_counts, na, ka):
        """MAP block of every node from the pooled histogram: reduce_scatter by node range, argmax on
        the owned rows (ties -> lowest block, like numpy), all_gather of the labels.  Returns a tensor [n] of
        block indices in the reference's numbering (type-b blocks offset by ka): uint8 while every label fits a
        byte (ka + kmax <= 256), int32 otherwise (wide handles, two-byte labels inside the library).

        The histogram is handed to reduce_scatter_tensor as it is -- rows [0, world * (n // world)) are a view, not
        a padded copy (the buffer is 1 GB at BASELINE configs[4]); the fewer than `world` rows that do not divide
        evenly are summed with one small all_reduce and labelled on every rank."""
        import torch
        dist = _dist()
        n, kmax = local_counts.shape
        lab_dtype = torch.uint8 if int(ka) + int(kmax) <= 256 else torch.int32

        def label_rows(rows, first_node):
            node = torch.arange(first_node, first_node + rows.shape[0], device=rows.device)
            return (_argmax_first(rows) + torch.where(node >= na, ka, 0)).to(lab_dtype)

        if self.world_size == 1:
            return label_rows(local_counts, 0)
        per = n // self.world_size
        n_main = per * self.world_size
        parts = []
        if per > 0:
            mine = torch.empty((per, kmax), dtype=local_counts.dtype, device=local_counts.device)
            dist.reduce_scatter_tensor(mine, local_counts[:n_main], op=dist.ReduceOp.SUM, group=self.group)
            out = torch.empty(n_main, dtype=lab_dtype, device=mine.device)
            dist.all_gather_into_tensor(out, label_rows(mine, self.rank * per).contiguous(), group=self.group)
            parts.append(out)
        if n_main < n:
            tail = local_counts[n_main:].clone()
            dist.all_reduce(tail, op=dist.ReduceOp.SUM, group=self.group)
            parts.append(label_rows(tail, n_main))
        return torch.cat(parts) if len(parts) > 1 else parts[0]


def _collective_device(shard):
    """where the tensors of a collective live: the current GPU for nccl, the host for gloo (and without a process group)"""
    import torch
    dist = _dist()
    if dist.is_initialized() and dist.get_backend(shard.group) == "nccl":
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cpu")


def _argmax_first(counts):
    """argmax along dim 1 returning the FIRST maximal column (torch.argmax does not promise which)."""
    import torch
    mx = counts.max(dim=1, keepdim=True).values
    k = counts.shape[1]
    idx = torch.arange(k, device=counts.device).expand_as(counts)
    return torch.where(counts == mx, idx, torch.full_like(idx, k)).min(dim=1).values


def numpy_marginals(labels_by_chain, na, ka, kb):
    """Host restatement of the marginal histogram for small cases: labels_by_chain [chains, n] ->
    counts[n, max(ka,kb)] (used by tests to check the device kernel and the collectives)."""
    labels_by_chain = np.asarray(labels_by_chain)
    n = labels_by_chain.shape[1]
    kmax = max(ka, kb)
    counts = np.zeros((n, kmax), dtype=np.int32)
    base = np.where(np.arange(n) >= na, ka, 0)
    for row in labels_by_chain:
        np.add.at(counts, (np.arange(n), row.astype(np.int64) - base), 1)
    return counts


def numpy_pair_scores(labels_by_chain, m_by_chain, m_r_by_chain, deg, pairs):
    """Host restatement of one sample of the pair scores (include/bisbm.h): for every pair (u, v) the sum over the given
    chains of ((double)d(u) * (double)d(v)) * (double)m[b_u, b_v] / ((double)m_r[b_u] * (double)m_r[b_v]), 0.0 where a degree
    is 0, in exactly this order of f64 operations -- one chain's term equals the device's bit for bit.  The arguments are what
    get_memberships / get_m / get_m_r return per chain (global labels, the full K x K matrix), as lists: the chains may have
    different shapes.  `deg`: the degree of every node (multi-edges count); `pairs`: integer array [P, 2]."""
    pairs = np.asarray(pairs).reshape(-1, 2).astype(np.int64)
    u, v = pairs[:, 0], pairs[:, 1]
    deg = np.asarray(deg)
    dd = deg[u].astype(np.float64) * deg[v].astype(np.float64)
    live = dd != 0
    total = np.zeros(len(pairs), dtype=np.float64)
    for labels, m, m_r in zip(labels_by_chain, m_by_chain, m_r_by_chain):
        labels = np.asarray(labels).astype(np.int64)
        m, m_r = np.asarray(m), np.asarray(m_r)
        bu, bv = labels[u][live], labels[v][live]
        term = np.zeros(len(pairs), dtype=np.float64)
        term[live] = (dd[live] * m[bu, bv].astype(np.float64)) / (m_r[bu].astype(np.float64) * m_r[bv].astype(np.float64))
        total += term
    return total


def numpy_edge_multiplicity(rowptr, col, pairs):
    """mu of every pair (u, v): the number of entries of u's CSR row equal to v (include/bisbm.h, "Edge probabilities")."""
    pairs = np.asarray(pairs).reshape(-1, 2).astype(np.int64)
    rowptr, col = np.asarray(rowptr).astype(np.int64), np.asarray(col).astype(np.int64)
    return np.array([int((col[rowptr[u]:rowptr[u + 1]] == v).sum()) for u, v in pairs], dtype=np.uint32)


def numpy_edge_dS(m, m_r, n_r, eta, deg, labels, ka, kb, E, u, v, kind, mult, lg, logq):
    """Host statement of one chain's dS of one pair (include/bisbm.h, "Edge probabilities"): the seven terms in the stated order,
    Python floats (f64, no fused multiply-add).  m, m_r, n_r, eta: the chain's block state as get_m / get_m_r / get_n_r /
    get_eta_rk_ return it (global labels, the full K x K matrix, eta [K, max_degree + 1]); deg: the degree of every node;
    labels: the chain's; E: the number of edges; kind 0: ADD, 1: REMOVE; mult: the pair's present multiplicity.  lg(i): the
    lgamma table's entry (lg(0) = +inf); logq(edges of the block, nodes of the block): the log_q of the description length, in
    the argument order the entropy kernel calls it with."""
    r, s = int(labels[u]), int(labels[v])
    du, dv, mu = int(deg[u]), int(deg[v]), int(mult)
    mrs, mr, ms, nr, ns = int(m[r][s]), int(m_r[r]), int(m_r[s]), int(n_r[r]), int(n_r[s])
    D = len(eta[0])

    def eta_at(x, d):
        return int(eta[x][d]) if 0 <= d < D else 0

    def lbinom(N, k):
        if N == 0 or k == 0 or k > N:
            return 0.0
        return (lg(N + 1) - lg(k + 1)) - lg(N - k + 1)
    cells = int(ka) * int(kb)
    E = int(E)
    if int(kind) == 0:
        t_deg = (lg(du + 1) - lg(du + 2)) + (lg(dv + 1) - lg(dv + 2))
        t_m = lg(mrs + 1) - lg(mrs + 2)
        t_mr = (lg(mr + 2) - lg(mr + 1)) + (lg(ms + 2) - lg(ms + 1))
        du2, dv2, mr2, ms2 = du + 1, dv + 1, mr + 1, ms + 1
        t_mult = lg(mu + 2) - lg(mu + 1)
        t_E = lbinom(cells + E, E + 1) - lbinom(cells + E - 1, E)
    else:
        t_deg = (lg(du + 1) - lg(du)) + (lg(dv + 1) - lg(dv))
        t_m = lg(mrs + 1) - lg(mrs)
        t_mr = (lg(mr) - lg(mr + 1)) + (lg(ms) - lg(ms + 1))
        du2, dv2, mr2, ms2 = du - 1, dv - 1, mr - 1, ms - 1
        t_mult = lg(mu) - lg(mu + 1)
        t_E = lbinom(cells + E - 2, E - 1) - lbinom(cells + E - 1, E)
    eu0, eu1, ev0, ev1 = eta_at(r, du), eta_at(r, du2), eta_at(s, dv), eta_at(s, dv2)
    t_eta = (((lg(eu0 + 1) - lg(eu0)) + (lg(eu1 + 1) - lg(eu1 + 2)))
             + ((lg(ev0 + 1) - lg(ev0)) + (lg(ev1 + 1) - lg(ev1 + 2))))
    t_q = (logq(mr2, nr) - logq(mr, nr)) + (logq(ms2, ns) - logq(ms, ns))
    return (((((t_deg + t_m) + t_mr) + t_eta) + t_q) + t_mult) + t_E


def numpy_edge_query_mult(rowptr, col, na, queries):
    """mu of every (query, candidate) of the edge queries (include/bisbm.h, "Edge queries"): one uint32 row per query over the
    nodes of the other type in id order -- how many entries of the query's CSR row name the candidate."""
    rowptr, col = np.asarray(rowptr).astype(np.int64), np.asarray(col).astype(np.int64)
    n, na = len(rowptr) - 1, int(na)
    rows = []
    for q in np.asarray(queries, dtype=np.int64).tolist():
        first, n_other = (na, n - na) if q < na else (0, na)
        rows.append(np.bincount(col[rowptr[q]:rowptr[q + 1]] - first, minlength=n_other).astype(np.uint32))
    return rows


def numpy_edge_query_rows(m, m_r, n_r, eta, deg, labels, na, ka, kb, E, queries, mult, lg, logq):
    """Host statement of one chain's rows of the edge queries (include/bisbm.h, "Edge queries"): for every query the ADD dS of
    numpy_edge_dS for all its candidates (the nodes of the other type in id order) at once -- the same seven terms from the same
    f64 operations in the same order, elementwise over the candidates, so every entry carries the bits of numpy_edge_dS for the
    pair (type-a node, type-b node) that query and candidate form.  Arguments as numpy_edge_dS; `queries`: node ids of either
    type; `mult`: the rows of numpy_edge_query_mult.  Returns a list of float64 rows; w is (dS > 700.0) ? 0.0 : exp(-dS)."""
    m, m_r, n_r, eta = np.asarray(m), np.asarray(m_r), np.asarray(n_r), np.asarray(eta)
    deg, labels = np.asarray(deg).astype(np.int64), np.asarray(labels).astype(np.int64)
    n, na, ka, kb, E = len(labels), int(na), int(ka), int(kb), int(E)
    K, D = ka + kb, eta.shape[1]

    def lbinom(N, k):
        if N == 0 or k == 0 or k > N:
            return 0.0
        return (lg(N + 1) - lg(k + 1)) - lg(N - k + 1)

    def table(keys, f):
        """f over the distinct keys, spread back: a float64 array shaped like `keys` (the last axis holds a key's parts)"""
        keys = np.asarray(keys, dtype=np.int64)
        flat = keys.reshape(-1, keys.shape[-1])
        uniq, inv = np.unique(flat, axis=0, return_inverse=True)
        vals = np.array([f(*row) for row in uniq.tolist()], dtype=np.float64)
        return vals[np.asarray(inv).reshape(-1)].reshape(keys.shape[:-1])
    # per block: the halves of t_mr and t_q
    h_mr = table(np.stack([m_r], axis=-1), lambda a: lg(a + 2) - lg(a + 1))
    h_q = table(np.stack([m_r, n_r], axis=-1), lambda a, b: logq(a + 1, b) - logq(a, b))
    # per node: the halves of t_deg and t_eta
    h_deg = table(np.stack([deg], axis=-1), lambda d: lg(d + 1) - lg(d + 2))
    e0 = eta[labels, deg].astype(np.int64)
    e1 = np.where(deg + 1 < D, eta[labels, np.minimum(deg + 1, D - 1)], 0).astype(np.int64)
    h_eta = table(np.stack([e0, e1], axis=-1), lambda a, b: (lg(a + 1) - lg(a)) + (lg(b + 1) - lg(b + 2)))
    # per cell of the quadrant: t_m
    t_m = table(np.stack([m[:ka, ka:K]], axis=-1), lambda a: lg(a + 1) - lg(a + 2))
    cells = ka * kb
    t_E = lbinom(cells + E, E + 1) - lbinom(cells + E - 1, E)
    rows = []
    for q, mu in zip(np.asarray(queries, dtype=np.int64).tolist(), mult):
        if q < na:  # the query is u, the candidates are the v
            u, v = np.full(n - na, q, dtype=np.int64), np.arange(na, n)
        else:
            u, v = np.arange(na), np.full(na, q, dtype=np.int64)
        r, s = labels[u], labels[v]
        t_mult = table(np.stack([np.asarray(mu)], axis=-1), lambda a: lg(a + 2) - lg(a + 1))
        dS = (h_deg[u] + h_deg[v]) + t_m[r, s - ka]
        dS = dS + (h_mr[r] + h_mr[s])
        dS = dS + (h_eta[u] + h_eta[v])
        dS = dS + (h_q[r] + h_q[s])
        dS = dS + t_mult
        rows.append(dS + t_E)
    return rows


QUERY_NONE = 0xFFFFFFFF  # bisbm_query_scores_topk: an entry past the eligible candidates


def numpy_query_topk(row, k, excluded=()):
    """Host statement of the ranking of bisbm_query_scores_topk for one query: `row` holds the sums of its candidates in id
    order, `excluded` the candidate indices that are not eligible (any order, repeats allowed).  Returns (index uint32 [k], sum
    float64 [k]): the eligible candidates by sum descending, ties to the lowest index; entries past the eligible ones are
    QUERY_NONE / 0.0.  The indices count within the row: add the first candidate's node id for global ids."""
    row = np.asarray(row, dtype=np.float64)
    ids = np.arange(len(row))
    keep = np.ones(len(row), dtype=bool)
    keep[np.asarray(excluded, dtype=np.int64)] = False
    ids = ids[keep]
    order = ids[np.lexsort((ids, -row[ids]))][:int(k)]
    idx = np.full(int(k), QUERY_NONE, dtype=np.uint32)
    val = np.zeros(int(k), dtype=np.float64)
    idx[:len(order)] = order
    val[:len(order)] = row[order]
    return idx, val


def numpy_coassign(labels_by_chain, queries, na):
    """Host statement of one or more samples of bisbm_coassign_accumulate: `labels_by_chain` holds the n labels of every counted
    (sample, chain) pair, in any order (the counts are integers).  Returns one uint32 row per query, in the queries' order (they
    may repeat): over the nodes of the query's own type in id order (0 .. na-1 for q < na, na .. n-1 otherwise), in how many of
    the given label vectors the node carries the query's label.  The query's own cell is the number of vectors."""
    rows = []
    for q in np.asarray(queries, dtype=np.int64):
        q = int(q)
        row = None
        for lab in labels_by_chain:
            lab = np.asarray(lab)
            own = lab[:na] if q < na else lab[na:]
            row = np.zeros(len(own), dtype=np.uint32) if row is None else row
            row += (own == lab[q]).astype(np.uint32)
        rows.append(row)
    return rows


def _foldin_blocks(m, m_r, n_r, ka, qtype):
    """the block state as the virtual node's type sees it: (m [K_own, K_oth], m_r and n_r of its own blocks, m_r of the other type's)"""
    m, m_r, n_r = np.asarray(m), np.asarray(m_r), np.asarray(n_r)
    K, ka = len(m_r), int(ka)
    a, b = np.arange(ka), np.arange(ka, K)
    quad = m[np.ix_(a, b)]  # (the type-a row, type-b column quadrant the engine keeps)
    if qtype:
        return quad.T, m_r[b], n_r[b], m_r[a]
    return quad, m_r[a], n_r[a], m_r[b]


def numpy_conditional_row(dS_row, r_local, free, beta, allowed=None):
    """Host statement of steps 3 and 4 of the node conditionals (include/bisbm.h, "Node conditionals") for one chain and one
    query: (P [K_own], stay, entropy, margin) from the row dS_s over the blocks of the node's type, the node's block within its
    type, whether the node is free (K_own > 1 and it is not alone in its block) and beta, with the operations in the order the
    header states.  margin is None for a node that is not free.  The exponential and the logarithm are numpy's: the device's may
    differ from them in the last bits, everything else is bit for bit.  `allowed` (None: every block): a 0 / 1 vector over the
    blocks of the type, the node's A_v of the block constraints (include/bisbm.h, "Block constraints", 2.) -- the row is then
    the restricted one of the heat-bath sweeps: the minimum is over A_v (r included), a block outside A_v has weight exactly 0.0,
    the margin is over the other blocks of A_v (None when there is none), and a node with one allowed block is not free."""
    dS = np.asarray(dS_row, dtype=np.float64)
    K, r, beta = len(dS), int(r_local), float(beta)
    if allowed is not None:
        A = np.asarray(allowed) != 0
        A[r] = True  # (the node's own block is always allowed)
        free = bool(free) and int(A.sum()) > 1
        if free:
            x = beta * (dS - dS[A].min())
            w = np.where((x > 700.0) | ~A, 0.0, np.exp(-np.minimum(x, 700.0)))
            Z = float(w[0])
            for y in w[1:]:
                Z = Z + float(y)
            P = w / Z
            others = A.copy()
            others[r] = False
            margin = float(dS[others].min())
            acc = 0.0
            for y in P:
                if y != 0.0:
                    acc = acc + float(y) * float(np.log(y))
            return P, float(P[r]), 0.0 - acc, margin
    if not free:
        P = np.zeros(K, dtype=np.float64)
        P[r] = 1.0
        margin = None
    else:
        x = beta * (dS - dS.min())
        w = np.where(x > 700.0, 0.0, np.exp(-np.minimum(x, 700.0)))
        Z = float(w[0])
        for y in w[1:]:
            Z = Z + float(y)
        P = w / Z
        margin = float(np.delete(dS, r).min())
    acc = 0.0
    for y in P:
        if y != 0.0:
            acc = acc + float(y) * float(np.log(y))
    return P, float(P[r]), 0.0 - acc, margin


def numpy_held_conditional_row(dS_row, r_loc, free, beta, clamped=False, allowed_own=None, f_own=None, exp=np.exp, log=np.log):
    """Host statement of the held row (include/bisbm.h, "Held conditionals") for one chain and one query: (dE [K_own], P [K_own],
    stay, entropy, margin) from the model's row dS_s over the blocks of the node's type, the node's block within its type,
    whether the node is free in the model's sense (K_own > 1 and it is not alone in its block) and beta.  clamped: the node's
    mask byte is non-zero.  allowed_own (None: every block): a 0 / 1 vector over the blocks of the type, the node's A_v (its own
    block always counts as allowed).  f_own (None: no fields): the entries of its class's field row over the same blocks.
    `exp`, `log`: the exponential (BlockModel.debug_exp for the device's bits) and the logarithm, each called with an array.
    margin is None for a node that is not open.  With no hold it is numpy_conditional_row bit for bit."""
    dS = np.asarray(dS_row, dtype=np.float64)
    K, r, beta = len(dS), int(r_loc), float(beta)
    dE = np.zeros(K, dtype=np.float64)
    for s in range(K):
        if s != r:
            dE[s] = float(dS[s]) + (float(f_own[s]) - float(f_own[r])) if f_own is not None else float(dS[s])
    A = np.ones(K, dtype=bool) if allowed_own is None else np.asarray(allowed_own) != 0
    A[r] = True
    is_open = K > 1 and bool(free) and not clamped and int(A.sum()) > 1
    margin = None
    if not is_open:
        P = np.zeros(K, dtype=np.float64)
        P[r] = 1.0
    else:
        mn = 0.0
        for s in range(K):
            if A[s] and dE[s] < mn:
                mn = float(dE[s])
        x = beta * (dE - mn)
        w = np.where((x > 700.0) | ~A, 0.0, np.asarray(exp(np.where(A, -np.minimum(x, 700.0), 0.0)), dtype=np.float64))
        Z = float(w[0])
        for y in w[1:]:
            Z = Z + float(y)
        P = w / Z
        others = A.copy()
        others[r] = False
        margin = float(dE[others].min())
    acc = 0.0
    lnP = np.asarray(log(np.where(P != 0.0, P, 1.0)), dtype=np.float64)
    for y, ln in zip(P, lnP):
        if y != 0.0:
            acc = acc + float(y) * float(ln)
    return dE, P, float(P[r]), 0.0 - acc, margin


def numpy_least_settled(values, k, by="entropy"):
    """Host statement of bisbm_least_settled_topk: (query indices uint32 [k], values float64 [k]) from one statistic of
    BlockModel.conditionals_stats -- the largest entropy sums first, or (by="stay") the smallest stay sums first, ties in ascending
    query index; past the entries the index is 0xffffffff and the value 0.0.  The device orders the bit patterns as unsigned keys,
    which is the order of the values only for sums of non-negative terms: asserted here."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    assert not np.isnan(v).any() and not (v.view(np.uint64) >> np.uint64(63)).any(), "a negative or NaN sum: the bit patterns do not order as unsigned keys"
    order = np.lexsort((np.arange(len(v)), v if by == "stay" else -v))[:int(k)]
    idx = np.full(int(k), 0xFFFFFFFF, dtype=np.uint32)
    val = np.zeros(int(k), dtype=np.float64)
    idx[:len(order)] = order
    val[:len(order)] = v[order]
    return idx, val


def numpy_heatbath_choice(dS_row, P_row, r, free, u, greedy, allowed=None):
    """Host statement of steps 3 and 4 of the heat-bath sweeps (include/bisbm.h, "Heat-bath sweeps and greedy polishing") for one
    visited node: the node's new block within its type from its rows dS_s and P(s), its current block r within its type, whether
    it is free, the uniform u of the step and whether the call is greedy (beta = +inf; u and P_row are not looked at then).  A
    node that is not free stays.  Bit for bit the device's choice when the rows are the device's.  `allowed` (None: every
    block): the node's A_v of the block constraints as a 0 / 1 vector over the blocks of the type -- a node with one allowed block
    stays, the greedy choice is the lowest block of A_v that attains the minimum over A_v (r's 0 included), and the drawn choice
    walks P_row, which is then the restricted row (0.0 outside A_v), as always."""
    r = int(r)
    if allowed is not None:
        A = [bool(x) for x in allowed]
        A[r] = True
        free = bool(free) and sum(A) > 1
    if not free:
        return r
    if greedy:
        dS = [float(x) for x in dS_row]
        if allowed is not None:
            mn = 0.0
            for s in range(len(dS)):
                if A[s] and s != r and dS[s] < mn:
                    mn = dS[s]
            if not mn < 0.0:
                return r
            for s in range(len(dS)):
                if A[s] and s != r and dS[s] == mn:
                    return s
        best = 0
        for s in range(1, len(dS)):
            if dS[s] < dS[best]:
                best = s
        return best if dS[best] < 0.0 else r
    u = float(u)
    C, last = 0.0, r
    for s, y in enumerate(P_row):
        y = float(y)
        C = y if s == 0 else C + y
        if y > 0.0:
            last = s
        if u < C:
            return s
    return last


def numpy_reshuffle_pair(x, ka, kb):
    """Host statement of step 2 of the pair reshuffles (include/bisbm.h, "Pair reshuffles"): (type, r, s) -- r < s within the
    type -- of the pair that the first word x of the move's draw 0 selects among the C(ka, 2) + C(kb, 2) pairs, type a first,
    each type lexicographically; None when the shape has no pair."""
    ka, kb = int(ka), int(kb)
    pa = ka * (ka - 1) // 2
    N = pa + kb * (kb - 1) // 2
    if N == 0:
        return None
    pi = (int(x) * N) >> 32
    t, k = (0, ka) if pi < pa else (1, kb)
    pi -= pa * t
    r = 0
    while pi >= k - 1 - r:
        pi -= k - 1 - r
        r += 1
    return t, r, r + 1 + pi


def numpy_reshuffle_launch(bits, r, s):
    """Host statement of the first half of step 4: the launch labels of the M members from their launch bits -- s where the bit
    is set, else r; if no member got r, member 0 gets r; if none got s, the last member gets s."""
    lab = [int(s) if b else int(r) for b in bits]
    if int(r) not in lab:
        lab[0] = int(r)
    if int(s) not in lab:
        lab[-1] = int(s)
    return lab


def numpy_reshuffle_step(dS_o, c_is_r, free, beta, u=None, forced_to_r=None, exp=np.exp):
    """Host statement of step 5 (and of one member of steps 6 and 7) for a member in block c of {r, s}: (goes to r?, factor, dead).
    dS_o: the dS of its other block (ignored when it is not free); c_is_r: whether c is r; free: n_r[c] > 1.  A free scan passes
    the uniform `u`; a forced pass passes `forced_to_r`, whether the member's original label is r.  dead: the forced move of a
    member that is not free, or a factor of exactly 0.0 -- Q becomes (0.0, 0) and nothing more is evaluated.  `exp`: the
    exponential -- the device's (BlockModel.debug_exp) reproduces the device bit for bit, numpy's to the last bits."""
    c_is_r = bool(c_is_r)
    if not free:
        if forced_to_r is not None and bool(forced_to_r) != c_is_r:
            return bool(forced_to_r), 0.0, True
        return c_is_r, 1.0, False
    dS_o, beta = float(dS_o), float(beta)
    mn = dS_o if dS_o < 0.0 else 0.0
    x_c, x_o = beta * (0.0 - mn), beta * (dS_o - mn)
    w_c = 0.0 if x_c > 700.0 else float(exp(np.float64(-x_c)))
    w_o = 0.0 if x_o > 700.0 else float(exp(np.float64(-x_o)))
    w_r, w_s = (w_c, w_o) if c_is_r else (w_o, w_c)
    Z = w_r + w_s
    P_r, P_s = w_r / Z, w_s / Z
    to_r = (float(u) < P_r) if forced_to_r is None else bool(forced_to_r)
    f = P_r if to_r else P_s
    return to_r, f, f == 0.0


def numpy_reshuffle_q(factors):
    """Q of a pass as (mantissa, exponent): frexp(1.0) multiplied by one factor at a time with a frexp after every multiply; a
    factor of 0.0 ends the pass at (0.0, 0)"""
    import math
    m, e = 0.5, 1
    for f in factors:
        if float(f) == 0.0:
            return 0.0, 0
        m, e2 = math.frexp(m * float(f))
        e += e2
    return m, e


def numpy_reshuffle_accept(dS_fwd, dS_rev, q_fwd, q_rev, beta, u_acc):
    """Host statement of step 8: (A, accepted) from the two sums of dS, the two Q as (mantissa, exponent), beta and u_acc.  A
    dead reverse pass (q_rev mantissa 0.0) is A = 0.0 and a rejection."""
    if float(q_rev[0]) == 0.0:
        return 0.0, False
    dS = float(dS_fwd) - float(dS_rev)
    with np.errstate(over="ignore"):
        lnA = (0.0 - float(beta) * dS) + (float(np.log(np.float64(q_rev[0]) / np.float64(q_fwd[0]))) + float(int(q_rev[1]) - int(q_fwd[1])) * 0.6931471805599453)
        A = float(np.exp(np.float64(lnA)))
    return A, float(u_acc) < A


def numpy_split_merge_choice(x, y, ka, kb, k_min=(1, 1), k_max=None, size_of=None):
    """Host statement of step 2 of the split and merge moves (include/bisbm.h, "Split and merge moves"): (kind, type, r, s,
    refused) from the first two words x, y of the move's draw 0 and the shape -- kind 0: a split of global label r (s: the
    label the new block takes), kind 1: a merge of the pair r < s, global labels; refused: 0, or 4 (a merge without a pair;
    type, r, s are 0 then), 3 (a merge of a type at k_min), 2 (a split of a type at k_max), 1 (a split of a block of fewer than
    two nodes; only when `size_of`, a function of the global label, is given), tested in this order.  k_max None: no bound."""
    ka, kb = int(ka), int(kb)
    K = ka + kb
    if int(x) & 1:
        pair = numpy_reshuffle_pair(y, ka, kb)
        if pair is None:
            return 1, 0, 0, 0, 4
        t, r, s = pair
        k = kb if t else ka
        return 1, t, r + t * ka, s + t * ka, 3 if k <= int(k_min[t]) else 0
    b = (int(y) * K) >> 32
    t = 1 if b >= ka else 0
    k = kb if t else ka
    refused = 0
    if k_max is not None and k >= int(k_max[t]):
        refused = 2
    elif size_of is not None and int(size_of(b)) < 2:
        refused = 1
    return 0, t, b, (K if t else ka), refused


def numpy_split_merge_roles(member_labels):
    """Host statement of step 3: (home label, away mask) of the present division of the members (ascending id) -- home is the
    block of member 0, whatever its label, so every unordered division has exactly one description."""
    lab = [int(l) for l in member_labels]
    return lab[0], [l != lab[0] for l in lab]


def numpy_split_merge_launch(bits):
    """Host statement of the first half of step 4: which of the M members are launched away -- member 0 never (its bit is not
    looked at), member i >= 1 iff its launch bit is set, and member M - 1 if that left nobody away."""
    away = [False] + [bool(b) for b in list(bits)[1:]]
    if not any(away):
        away[-1] = True
    return away


def numpy_split_merge_step(dS_o, in_home, free, beta, u=None, forced_home=None, exp=np.exp):
    """Host statement of one restricted step of step 4, 6 or 7 for a member i >= 1: (goes home?, factor, dead) -- the step of
    numpy_reshuffle_step with (home, away) in the place of (r, s): Z = w_home + w_away, home iff u < P_home.  Only the sole
    member of away can be not free."""
    return numpy_reshuffle_step(dS_o, in_home, free, beta, u=u, forced_to_r=forced_home, exp=exp)


def numpy_split_merge_dS(m_h, m_a, eta_h, eta_a, mr_h, mr_a, nr_h, nr_a, T_merged, T_divided, lgamma, log_q):
    """Host statement of step 5: merge_dS = S(blocks h and a made one) - S(as they are), from their rows of m over the other
    type's blocks (ascending), their eta rows over the degrees 0 .. max_degree, their m_r and n_r and the shape terms T of the
    two shapes; lgamma(i) and log_q(n, k) are the tables' (callables)."""
    acc_m = 0.0
    for x, y in zip(m_h, m_a):
        x, y = int(x), int(y)
        acc_m = acc_m + ((lgamma(x + 1) + lgamma(y + 1)) - lgamma(x + y + 1))
    acc_e = 0.0
    for x, y in zip(eta_h, eta_a):
        x, y = int(x), int(y)
        acc_e = acc_e + ((lgamma(x + 1) + lgamma(y + 1)) - lgamma(x + y + 1))
    mr_h, mr_a, nr_h, nr_a = int(mr_h), int(mr_a), int(nr_h), int(nr_a)
    tail1 = lgamma(mr_h + mr_a + 1) - (lgamma(mr_h + 1) + lgamma(mr_a + 1))
    tail2 = log_q(mr_h + mr_a, nr_h + nr_a) - (log_q(mr_h, nr_h) + log_q(mr_a, nr_a))
    return (((acc_m + acc_e) + tail1) + tail2) + (float(T_merged) - float(T_divided))


def numpy_split_merge_pairs(ka, kb):
    """N(ka, kb) = C(ka, 2) + C(kb, 2)"""
    return int(ka) * (int(ka) - 1) // 2 + int(kb) * (int(kb) - 1) // 2


def numpy_split_merge_accept(kind, merge_dS, q, beta, u_acc, ka, kb, t, exp=np.exp, log=np.log):
    """Host statement of steps 6 to 8: (dS, ln A, A, accepted) of a split (kind 0; merge_dS of the proposal, q = Q_fwd) or a
    merge (kind 1; merge_dS of the present division, q = Q_rev) of type t from the shape (ka, kb) BEFORE the move.  q is
    (mantissa, exponent); a dead forced pass (mantissa 0.0) is ln A = -inf, A = 0.0 and a rejection."""
    ka, kb, beta = int(ka), int(kb), float(beta)
    K = ka + kb
    if kind == 1 and float(q[0]) == 0.0:
        return float(merge_dS), -np.inf, 0.0, False
    ln_q = float(log(np.float64(q[0]))) + float(int(q[1])) * 0.6931471805599453
    if kind == 1:
        dS = float(merge_dS)
        lnA = ((0.0 - beta * dS) + (float(log(np.float64(numpy_split_merge_pairs(ka, kb)))) - float(log(np.float64(K - 1))))) + ln_q
    else:
        dS = 0.0 - float(merge_dS)
        after = numpy_split_merge_pairs(ka + (1 - t), kb + t)
        lnA = ((0.0 - beta * dS) + (float(log(np.float64(K))) - float(log(np.float64(after))))) - ln_q
    with np.errstate(over="ignore"):
        A = float(exp(np.float64(lnA)))
    return dS, lnA, A, float(u_acc) < A


def numpy_split_merge_renumber(labels, kind, t, r, s, ka, kb, away_nodes=None):
    """Host statement of the numbering after an accepted move (step 8): (labels, ka, kb).  Split (kind 0) of block r of type t
    with the nodes `away_nodes` leaving it: of type a, away becomes label ka and every type-b label moves up by one; of type b,
    away becomes label ka + kb.  Merge (kind 1) of r < s: the nodes of s take r, the labels of that type above s move down by
    one, and for a type-a merge every type-b label moves down by one as well."""
    lab = np.array(labels, dtype=np.int64)
    ka, kb = int(ka), int(kb)
    if kind == 0:
        if t == 0:
            lab[lab >= ka] += 1
            lab[np.asarray(away_nodes, dtype=np.int64)] = ka
            return lab, ka + 1, kb
        lab[np.asarray(away_nodes, dtype=np.int64)] = ka + kb
        return lab, ka, kb + 1
    lab[lab == int(s)] = int(r)
    lab[lab > int(s)] -= 1
    return (lab, ka - 1, kb) if t == 0 else (lab, ka, kb - 1)


def numpy_clamped_shuffle(labels, mask, na, perm_a, perm_b):
    """The shuffle under a clamp (include/bisbm.h, "Clamped nodes", 4.) on the host, given the two permutations of the
    compacted label vectors: with F the ascending list of the open (mask == 0) nodes of a type and f its permutation of
    range(len(F)), new[F[i]] = old[F[f[i]]]; the clamped nodes keep their labels.  perm_a / perm_b: f of type a (nodes
    0 .. na-1) and of type b, of lengths |F_a| and |F_b| (0 and 1 included: nothing moves)."""
    labels = np.asarray(labels)
    held = np.asarray(mask) != 0
    out = labels.copy()
    for lo, hi, perm in ((0, int(na), perm_a), (int(na), len(labels), perm_b)):
        F = lo + np.flatnonzero(~held[lo:hi])
        perm = np.asarray(perm, dtype=np.int64)
        if len(perm) != len(F) or sorted(perm.tolist()) != list(range(len(F))):
            raise ValueError("a permutation of the %d open nodes of the type is needed" % len(F))
        out[F] = labels[F[perm]]
    return out


def numpy_constrained_shuffle(labels, mask, na, class_of_node, perms):
    """The shuffle under block constraints (include/bisbm.h, "Block constraints", 4.) on the host, given the permutation of
    every (type, class): with F the ascending list of the open (mask == 0; mask None: all) nodes of type t and class c and
    f = perms[(t, c)] a permutation of range(len(F)), new[F[i]] = old[F[f[i]]]; every other node keeps its label.  A (type,
    class) without an open node needs no entry, one with a single open node may have [0] or none."""
    labels = np.asarray(labels)
    cls = np.asarray(class_of_node)
    held = np.zeros(len(labels), dtype=bool) if mask is None else np.asarray(mask) != 0
    out = labels.copy()
    for t, (lo, hi) in enumerate(((0, int(na)), (int(na), len(labels)))):
        for c in np.unique(cls[lo:hi]):
            F = lo + np.flatnonzero(~held[lo:hi] & (cls[lo:hi] == c))
            if len(F) <= 1 and (t, int(c)) not in perms:
                continue
            perm = np.asarray(perms[(t, int(c))], dtype=np.int64)
            if len(perm) != len(F) or sorted(perm.tolist()) != list(range(len(F))):
                raise ValueError("a permutation of the %d open nodes of type %d and class %d is needed" % (len(F), t, c))
            out[F] = labels[F[perm]]
    return out


def numpy_foldin_posterior(labels, m, m_r, n_r, ka, qtype, neighbours, alpha):
    """Host statement of steps 1 and 2 of the fold-in queries (include/bisbm.h, "Fold-in queries") for one chain and one virtual
    node: the posterior P[K_own] over the blocks of its type, bit for bit what the device computes.  `labels`, `m`, `m_r`, `n_r`:
    what get_memberships / get_m / get_m_r / get_n_r return for the chain (global labels, the full K x K matrix); `ka`: the
    chain's type-a block count; `qtype`: 0 (a) or 1 (b); `neighbours`: the list, in order.  The blocks are taken side by side,
    the list one entry after the other, which is the order of operations of every single block."""
    labels = np.asarray(labels).astype(np.int64)
    quad, mr, nr, mr_oth = _foldin_blocks(m, m_r, n_r, ka, qtype)
    oth0 = 0 if qtype else int(ka)
    alpha = float(alpha)
    live = nr > 0
    mant, ex = np.frexp(np.where(live, nr, 0).astype(np.float64))
    ex = ex.astype(np.int64)
    den = mr.astype(np.float64) + alpha * float(len(mr_oth))
    for w in np.asarray(neighbours, dtype=np.int64):
        x = (quad[:, labels[w] - oth0].astype(np.float64) + alpha) / den
        mant = mant * x
        mant, e2 = np.frexp(mant)
        ex = ex + e2
    rel = np.where(live, ex - ex[live].max(), 0)
    wgt = np.where(live & (rel >= -1000), np.ldexp(mant, np.maximum(rel, -1000).astype(np.int32)), 0.0)
    Z = float(wgt[0])
    for x in wgt[1:]:
        Z = Z + float(x)
    return wgt / Z


def numpy_foldin_tables(labels, m, m_r, n_r, ka, qtype, neighbours, alpha):
    """(P [K_own], g [K_oth]): the posterior of numpy_foldin_posterior and the recommend table of step 3, the sum over the
    virtual node's blocks taken in ascending order for all blocks of the other type side by side."""
    P = numpy_foldin_posterior(labels, m, m_r, n_r, ka, qtype, neighbours, alpha)
    quad, mr, nr, mr_oth = _foldin_blocks(m, m_r, n_r, ka, qtype)
    acc = np.zeros(len(mr_oth), dtype=np.float64)
    for r in range(len(mr)):
        if mr[r] == 0 or P[r] == 0.0:
            continue
        acc = acc + (P[r] * quad[r].astype(np.float64)) / float(mr[r])
    g = np.zeros(len(mr_oth), dtype=np.float64)
    has = mr_oth != 0
    g[has] = acc[has] / mr_oth[has].astype(np.float64)
    return P, g


def numpy_foldin_rows(labels, deg, na, ka, qtype, d_q, P, g):
    """(recommend row, similar row) of one chain (step 4): the terms of all nodes of the other type and of the virtual node's own
    type, each in id order.  `deg`: the degree of every node; `d_q`: the length of the virtual node's list."""
    labels, deg = np.asarray(labels).astype(np.int64), np.asarray(deg)
    a, b = slice(0, na), slice(na, len(labels))
    own, oth, own0, oth0 = (b, a, int(ka), 0) if qtype else (a, b, 0, int(ka))
    rec = (float(d_q) * deg[oth].astype(np.float64)) * np.asarray(g)[labels[oth] - oth0]
    return rec, np.asarray(P)[labels[own] - own0].astype(np.float64)
