"""Marginalisation driver: what the reference's README describes for "marginalize" mode
(`/root/reference/README.md:49-53,96-104`) and its CLI never implements (`-b/--burn_in` and
`-f/--sampling_frequency` are parsed at `src/mcmc_main.cc:61-65` and then unused).

Semantics (the README prose is the only specification): constant temperature T = 1; `burn_in` sweeps are
discarded; then `n_samples` samples are taken `sampling_frequency` sweeps apart; a sample adds every chain's
label of every node to a per-node histogram; the marginal estimate of a node is its most frequent block
(ties -> lowest block index).

Pooling over ranks stays on the device: every rank's chains are histogrammed by the marginals kernel
straight into a torch tensor on the rank's GPU (`bisbm_marginals_accumulate(device_counts)`), that tensor is
reduce-scattered by node range (`ChainShard.map_labels`: RCCL over xGMI with the nccl backend), each rank takes the
argmax of its rows, and the uint8 labels are all-gathered -- no host copy of the n x kmax histogram anywhere.  (With
the gloo backend of the CPU tests the same tensor is moved to the host first: gloo reduces host tensors.)
"""
import numpy as np


def marginalize(model, burn_in_sweeps, n_samples, sampling_frequency_sweeps, shard=None, device_counts=None,
                return_counts=None, align=False, tempering=None, exchange_every=1, score_pairs=None, recommend=None,
                similar=None, foldin=None, conditionals=None, sampler="mh", reshuffles=0, reshuffle_scans=3, trace=None, rung_moves=None, blocks=False,
                clamp=None, constraints=None, fields=None, conditionals_held=False, least_settled=None, edge_probs=None,
                recommend_edges=None, split_merges=0, split_merge_scans=3, k_min=(1, 1), k_max=None):
    """Runs the chain(s) of `model` (a BlockModel whose state is already initialised by init_bisbm() /
    shuffle_bisbm()) and returns (labels, counts):
      labels  uint32 [n]         MAP block of every node in the reference's numbering
      counts  [n, max(KA,KB)]    pooled histogram (column = block index within the node's type); None when
                                 return_counts is False.  Default: returned on a single rank, NOT returned when the chains
                                 are spread over ranks (there the pooled histogram costs an all_reduce of the whole
                                 n x kmax buffer, 1 GB at BASELINE configs[4], on top of the reduce_scatter the labels need)
    `shard`: a distributed.ChainShard when chains are spread over ranks.
    `device_counts`: a torch int32 tensor [n, kmax] on the model's device to accumulate into (it is NOT zeroed: samples
    add to what it holds); by default one is allocated when pooling over ranks, and the library's internal buffer is
    used for a single rank.  The library's kernels run on the handle's own (non-blocking) stream, so whatever torch
    still has in flight on the tensor (its zero fill, a caller's writes) is waited for here before the first sample
    is added -- the stream contract include/bisbm.h states for `device_counts`.
    `align`: count every chain's labels through its permutation onto a reference partition (include/bisbm.h, "Label
    alignment before pooling"); pooling more than one chain gives a marginal only then.  The mode is turned on for the run and
    stays on.  The reference: one the caller set (model.marginals_set_reference), or else the lowest-description-length chain
    at the first sample -- over all ranks when the chains are spread (all-gathered description lengths, ties -> the lowest
    global chain id; the owning rank broadcasts its labels and every rank sets them before the first sample).
    `tempering`: a temperature ladder T0 <= ... <= T{L-1} (include/bisbm.h, "Replica exchange"): the chains run in ensembles of L
    consecutive global ids, burn-in and the gaps between samples run through model.tempering_run(sweeps, exchange_every), and
    only the chains on rung 0 (T0) are counted -- over ranks each rank histograms its own cold chains, and the aligned reference
    is the lowest-description-length rung-0 chain.  Tempering is turned on for the run (rungs and statistics reset) and stays
    on: model.tempering_stats() reports the swaps afterwards.
    `score_pairs`: an integer array [P, 2] of (type-a node, type-b node) pairs (include/bisbm.h, "Posterior-predictive pair
    scores"): set, with zeroed sums, before the first sample, and every sample also adds every counted chain's term to every
    pair's sum (with `tempering` the chains on rung 0 only).  The return value does not change: model.pair_scores() gives
    (sum, terms) afterwards, shard.pooled_pair_scores(model) the same over ranks.
    `edge_probs`: (pairs, kinds) or (pairs,) as model.edge_probs_set takes them (include/bisbm.h, "Edge probabilities"): set, with
    zeroed sums, before the first sample, and every sample also adds every counted chain's dS and exp(-dS) to every pair's sums
    -- wherever `score_pairs` takes a sample.  The return value does not change: model.edge_probs() gives the sums and the
    estimates afterwards.  The chains of this rank only.
    `recommend`: (queries, k) or (queries, k, exclude_edges) (include/bisbm.h, "Query scores"): the queries are set, with zeroed
    sums, before the first sample, every sample also adds every counted chain's term to every (query, candidate) sum, and the
    return value becomes (labels, counts, model.recommend(k, exclude_edges)) -- the chains of this rank only.
    `recommend_edges`: (queries, k) or (queries, k, exclude_edges) (include/bisbm.h, "Edge queries"): the queries are set, with
    zeroed sums, before the first sample, every sample also adds every counted chain's exp(-dS) of adding the edge to every (query,
    candidate) sum, and model.recommend_edges(k, exclude_edges) -- (nodes, w_sum, log_prob) -- is appended to the return
    value, after `recommend`'s element when both are asked for.  The chains of this rank only.
    `similar`: (queries, k) (include/bisbm.h, "Co-assignment"): the queries are set, with zeroed counts, before the first sample,
    every sample also counts in which chains every node of a query's own type shares its block, and model.similar(k) -- (nodes,
    count / terms, terms) -- is appended as the last element of the return value.  The chains of this rank only: pooling over
    ranks is out of scope.
    `foldin`: (nodes, k) or (nodes, k, alpha) (include/bisbm.h, "Fold-in queries"; nodes as model.foldin_set takes them): the
    virtual nodes are set, with zeroed sums, before the first sample, every sample also adds every counted chain's terms to their
    rows, and (model.foldin_recommend(k), model.foldin_similar(k)) is appended as the last element of the return value.  The
    chains of this rank only.
    `conditionals`: (nodes, beta) or (nodes,) (include/bisbm.h, "Node conditionals"; nodes as model.conditionals_set takes them,
    None: every node): the queries are set, with zeroed sums, before the first sample, every marginal sample also takes one
    conditional sample, and model.conditionals_stats() is appended to the return value; with `align` the soft marginals use the
    reference the aligned histogram uses (taken over after the first marginal sample) and model.conditionals_marginals() --
    (prob, terms) -- is appended after the stats.  The chains of this rank only.
    `sampler`: "mh" (the default: model.run_sweeps) or "heatbath" -- burn-in and the gaps between samples run through
    model.heatbath_sweeps(sweeps, 1.0) (include/bisbm.h, "Heat-bath sweeps and greedy polishing"); with `tempering` a ValueError
    (heat-bath sweeps inside replica exchange are asked for with `rung_moves`).
    `reshuffles`: m > 0 runs model.reshuffle(m, reshuffle_scans, 1.0) after every block of sweeps -- the burn-in and every gap
    between samples (include/bisbm.h, "Pair reshuffles"; 3 scans are the convention of the literature, not a measurement); with
    `tempering` a ValueError (`rung_moves` is the keyword for that).  model.reshuffle_stats = {"proposed", "accepted"} (totals over the chains of this rank) reports
    the acceptance afterwards.
    `rung_moves`: with `tempering` only (ValueError without): a dict with some of the keys "mh" (default 1), "heatbath" (0),
    "reshuffles" (0), "scans" (3).  Burn-in and the gaps between samples then run as ROUNDS of model.tempering_rounds -- per round
    that many MH sweeps, heat-bath sweeps and pair reshuffles of every chain at its rung's temperature, then one exchange --
    and `burn_in_sweeps` and `sampling_frequency_sweeps` count rounds; `exchange_every` is not used.
    model.tempering_rung_stats() reports what each move did per rung afterwards.
    `trace`: depth > 0 (include/bisbm.h, "Chain traces"): a ring of that many snapshots per chain is set, with everything
    forgotten, before the first sample, and every sample is followed by one model.trace_record().  The return value does not
    change: model.trace_lags() / model.trace_series() give the lag curves and the series afterwards (lags in units of
    sampling_frequency_sweeps), trace_summary() tau and R-hat.  The chains of this rank only.
    `blocks`: with `align` only (ValueError without, before any sweep: raw labels of several chains share no numbering)
    (include/bisbm.h, "Block summaries"): the block sums are turned on, zeroed, before the first sample (after the reset), and
    every sample also sums the counted chains' aligned block matrices, sizes and degrees.  The return value does not change:
    model.block_summary() gives the means and standard deviations afterwards.  The chains of this rank only.
    `clamp`: node ids or a mask, as model.clamp takes them (include/bisbm.h, "Clamped nodes"): set before the burn-in and left
    set, so these nodes keep the labels every chain has for them at the call through the whole run, whatever the sampler
    (`sampler`, `reshuffles`, `tempering`, `rung_moves`).  When every block holds a clamped node with the same label in every
    chain the block numbering is pinned, and the pooled histogram is a marginal over chains without `align`.
    `constraints`: (class_of_node, allowed) as model.constrain takes them (include/bisbm.h, "Block constraints"): set before the
    burn-in and left set, so every node stays inside the blocks its class allows through the whole run, whatever the sampler.
    Classes that allow disjoint sets of blocks keep those sets apart in every chain.
    `fields`: (class_of_node, field) as model.set_fields takes them (include/bisbm.h, "Block fields"): set before the burn-in and
    left set, so every sampler of the run targets exp(-beta (S + Phi)); the marginals are those of the tilted posterior.
    `conditionals_held`: with `conditionals` only (ValueError without, before anything is set): the conditional samples evaluate
    the held row (include/bisbm.h, "Held conditionals"), the conditional the run's samplers sample under the clamp, the
    constraints and the fields as they are at each sample.
    `least_settled`: (k, by) or (k,) with `conditionals` only (ValueError without), by = "entropy" (the default) or "stay"
    (include/bisbm.h, "Least settled"): model.least_settled(k, by) -- (query indices, nodes, values, terms) -- is appended after
    the conditionals' stats (and their soft marginals).
    `split_merges`: m > 0 runs model.split_merge(m, split_merge_scans, 1.0, k_min, k_max) after every block of sweeps -- the
    burn-in and every gap between samples (include/bisbm.h, "Split and merge moves") -- so the chains sample (Ka, Kb) with the
    partition, and the return value becomes (shape_counts, best): shape_counts {(ka, kb): visits} over samples and chains, best
    {(ka, kb): (S, labels)} the lowest description length seen at a sample in every visited shape with its labels.  The pooled
    label histogram needs one common shape and is refused there, with everything that rests on it or on a block numbering
    (`align`, `blocks`, `device_counts`, `return_counts`, `trace`, `tempering`, `clamp`, `constraints`, `fields`, `recommend`,
    `recommend_edges`, `reshuffles`, chains spread over ranks: ValueError before anything runs); the numbering-free options
    `score_pairs`, `edge_probs`, `similar`, `foldin` and `conditionals` stay and then average over the posterior of (Ka, Kb) --
    the results of `similar`, `foldin` and `conditionals` are appended as above (model.pair_scores() and model.edge_probs() give
    the sums of the other two, as always).  model.split_merge_stats = {"proposed", "accepted"} reports the acceptance."""
    _check_conditional_extras(conditionals, conditionals_held, least_settled)
    if int(split_merges) < 0 or int(split_merge_scans) < 0:
        raise ValueError("split_merges and split_merge_scans must not be negative")
    if split_merges:
        refused = {"align": align, "blocks": blocks, "device_counts": device_counts is not None, "return_counts": bool(return_counts),
                   "trace": bool(trace), "tempering": tempering is not None, "rung_moves": rung_moves is not None, "clamp": clamp is not None,
                   "constraints": constraints is not None, "fields": fields is not None, "recommend": recommend is not None,
                   "recommend_edges": recommend_edges is not None, "reshuffles": bool(reshuffles), "conditionals_held": conditionals_held,
                   "least_settled": least_settled is not None, "shard": shard is not None and shard.world_size > 1}
        bad = sorted(k for k, v in refused.items() if v)
        if bad:
            raise ValueError("split_merges changes the chains' block counts: the pooled label histogram and everything that rests on one "
                             "block numbering is refused with it (%s)" % ", ".join(bad))
        return _marginalize_shapes(model, burn_in_sweeps, n_samples, sampling_frequency_sweeps, sampler, int(split_merges), int(split_merge_scans),
                                   k_min, k_max, score_pairs, edge_probs, similar, foldin, conditionals)
    if clamp is not None:
        model.clamp(clamp)
    if constraints is not None:
        model.constrain(*constraints)
    if fields is not None:
        model.set_fields(*fields)
    if blocks and not align:
        raise ValueError("blocks=True needs align=True: the block sums are taken in the numbering of the aligned histogram")
    n = model.n
    multi = shard is not None and shard.world_size > 1
    if return_counts is None:
        return_counts = not multi
    advance = _advance(model, tempering, exchange_every, sampler, reshuffles, reshuffle_scans, rung_moves)
    if burn_in_sweeps > 0:
        advance(burn_in_sweeps)
    if score_pairs is not None:
        model.pair_scores_set(score_pairs)
        model.pair_scores_reset()
    if edge_probs is not None:
        model.edge_probs_set(edge_probs[0], edge_probs[1] if len(edge_probs) > 1 else None)
        model.edge_probs_reset()
    if recommend is not None:
        model.query_scores_set(recommend[0])
        model.query_scores_reset()
    if recommend_edges is not None:
        model.edge_queries_set(recommend_edges[0])
        model.edge_queries_reset()
    if similar is not None:
        model.coassign_set(similar[0])
        model.coassign_reset()
    if foldin is not None:
        model.foldin_set(foldin[0], foldin[2] if len(foldin) > 2 else None)
    if conditionals is not None:
        model.conditionals_set(conditionals[0], conditionals[1] if len(conditionals) > 1 else 1.0)
        if conditionals_held:
            model.conditionals_held(True)
    _trace_start(model, trace)
    taken = [0]

    def conditional_sample():
        if trace:
            model.trace_record()
        if conditionals is None:
            return
        if align and taken[0] == 0:  # (the aligned histogram has its reference from its first sample on)
            model.conditionals_set_reference(model.marginals_reference()[0])
        model.conditionals_accumulate()
        taken[0] += 1

    def result(labels, counts):
        out = (labels, counts)
        if recommend is not None:
            out += (model.recommend(int(recommend[1]), bool(recommend[2]) if len(recommend) > 2 else True),)
        if recommend_edges is not None:
            out += (model.recommend_edges(int(recommend_edges[1]), bool(recommend_edges[2]) if len(recommend_edges) > 2 else True),)
        if similar is not None:
            out += (model.similar(int(similar[1])),)
        if foldin is not None:
            out += ((model.foldin_recommend(int(foldin[1])), model.foldin_similar(int(foldin[1]))),)
        if conditionals is not None:
            out += (model.conditionals_stats(),)
            if align:
                out += (model.conditionals_marginals(),)
            if least_settled is not None:
                out += (model.least_settled(int(least_settled[0]), least_settled[1] if len(least_settled) > 1 else "entropy"),)
        return out
    if device_counts is None and not multi:
        # one rank, no caller buffer: the library's own histogram
        model.marginals_reset()
        if align:
            model.marginals_set_alignment(True)
        if blocks:
            model.block_sums_set(True)
        for _ in range(int(n_samples)):
            if sampling_frequency_sweeps > 0:
                advance(sampling_frequency_sweeps)
            model.marginals_accumulate(None)
            if score_pairs is not None:
                model.pair_scores_accumulate()
            if edge_probs is not None:
                model.edge_probs_accumulate()
            if recommend is not None:
                model.query_scores_accumulate()
            if recommend_edges is not None:
                model.edge_queries_accumulate()
            if similar is not None:
                model.coassign_accumulate()
            if foldin is not None:
                model.foldin_accumulate()
            conditional_sample()
        counts = model.marginals_get().astype(np.int64)
        base = np.where(np.arange(n) >= model.na, model.KA, 0)
        return result((counts.argmax(axis=1) + base).astype(np.uint32), (counts if return_counts else None))

    import torch
    if device_counts is None:
        device_counts = torch.zeros((n, model.kmax), dtype=torch.int32, device=model.counts_device())
    if (not isinstance(device_counts, torch.Tensor) or device_counts.dtype != torch.int32
            or tuple(device_counts.shape) != (n, model.kmax) or not device_counts.is_contiguous()):
        raise ValueError("device_counts must be a contiguous torch.int32 tensor of shape (n, max(KA, KB)) on the model's device")
    if device_counts.is_cuda:
        # torch.zeros / the caller's kernels ran on torch's stream, bisbm_marginals_accumulate adds with plain (non-atomic)
        # read-modify-writes on the library's stream: order the two before the first sample.  (The other direction needs
        # nothing: bisbm_marginals_accumulate returns after its kernel has finished.)
        torch.cuda.current_stream(device_counts.device).synchronize()
    if align:
        model.marginals_set_alignment(True)
        if multi:
            model.marginals_set_reference(shard.lowest_chain_labels(model)[1])
        else:
            _drop_library_reference(model)
    if blocks:
        model.block_sums_set(True)
    for _ in range(int(n_samples)):
        if sampling_frequency_sweeps > 0:
            advance(sampling_frequency_sweeps)
        model.marginals_accumulate(device_counts.data_ptr())  # adds into the tensor, on the device
        if score_pairs is not None:
            model.pair_scores_accumulate()
        if edge_probs is not None:
            model.edge_probs_accumulate()
        if recommend is not None:
            model.query_scores_accumulate()
        if recommend_edges is not None:
            model.edge_queries_accumulate()
        if similar is not None:
            model.coassign_accumulate()
        if foldin is not None:
            model.foldin_accumulate()
        conditional_sample()
    if not multi:
        from .distributed import _argmax_first
        arg = _argmax_first(device_counts)
        node = torch.arange(n, device=device_counts.device)
        labels = (arg + torch.where(node >= model.na, model.KA, 0)).cpu().numpy().astype(np.uint32)
        return result(labels, (device_counts.cpu().numpy().astype(np.int64) if return_counts else None))
    send = device_counts if _uses_cuda_backend(shard) else device_counts.cpu()
    labels = shard.map_labels(send, model.na, model.KA).cpu().numpy().astype(np.uint32)
    counts = shard.pooled_marginals(send).cpu().numpy().astype(np.int64) if return_counts else None
    return result(labels, counts)


def _marginalize_shapes(model, burn_in_sweeps, n_samples, sampling_frequency_sweeps, sampler, moves, scans, k_min, k_max, score_pairs, edge_probs,
                        similar, foldin, conditionals):
    """marginalize(..., split_merges=moves): see there"""
    if sampler not in ("mh", "heatbath"):
        raise ValueError("sampler must be \"mh\" or \"heatbath\"")
    model.split_merge_stats = {"proposed": 0, "accepted": 0}

    def advance(sweeps):
        if sampler == "mh":
            model.run_sweeps(int(sweeps))
        else:
            model.heatbath_sweeps(int(sweeps), 1.0)
        acc = model.split_merge(moves, scans, 1.0, k_min, k_max)
        model.split_merge_stats["proposed"] += moves * model.n_chains
        model.split_merge_stats["accepted"] += int(acc.sum())
    if burn_in_sweeps > 0:
        advance(burn_in_sweeps)
    if score_pairs is not None:
        model.pair_scores_set(score_pairs)
        model.pair_scores_reset()
    if edge_probs is not None:
        model.edge_probs_set(edge_probs[0], edge_probs[1] if len(edge_probs) > 1 else None)
        model.edge_probs_reset()
    if similar is not None:
        model.coassign_set(similar[0])
        model.coassign_reset()
    if foldin is not None:
        model.foldin_set(foldin[0], foldin[2] if len(foldin) > 2 else None)
    if conditionals is not None:
        model.conditionals_set(conditionals[0], conditionals[1] if len(conditionals) > 1 else 1.0)
    shape_counts, best = {}, {}
    for _ in range(int(n_samples)):
        if sampling_frequency_sweeps > 0:
            advance(sampling_frequency_sweeps)
        S = model.entropy()
        lowest = {}
        for c in range(model.n_chains):
            shape = model.ka_kb(c)
            shape_counts[shape] = shape_counts.get(shape, 0) + 1
            if shape not in lowest or S[c] < S[lowest[shape]]:
                lowest[shape] = c
        for shape, c in lowest.items():
            if shape not in best or S[c] < best[shape][0]:
                best[shape] = (float(S[c]), model.get_memberships(c))
        if score_pairs is not None:
            model.pair_scores_accumulate()
        if edge_probs is not None:
            model.edge_probs_accumulate()
        if similar is not None:
            model.coassign_accumulate()
        if foldin is not None:
            model.foldin_accumulate()
        if conditionals is not None:
            model.conditionals_accumulate()
    out = (shape_counts, best)
    if similar is not None:
        out += (model.similar(int(similar[1])),)
    if foldin is not None:
        out += ((model.foldin_recommend(int(foldin[1])), model.foldin_similar(int(foldin[1]))),)
    if conditionals is not None:
        out += (model.conditionals_stats(),)
    return out


def marginalize_modes(model, burn_in_sweeps, n_samples, sampling_frequency_sweeps, threshold=None, mode_of_chain=None, shard=None,
                      reassign=False, tempering=None, exchange_every=1, sampler="mh", trace=None, rung_moves=None, blocks=False, clamp=None,
                      constraints=None, fields=None, conditionals=None, conditionals_held=False, least_settled=None):
    """Mode-resolved marginals (include/bisbm.h, "Mode-resolved marginals"): the chains are grouped into posterior modes and
    every mode gets an aligned histogram and a MAP of its own, in the numbering of its own reference.
    Exactly one of `threshold` and `mode_of_chain`: with `threshold` the grouping is model.partition_modes(threshold) taken
    after the burn-in; `mode_of_chain` is a caller's grouping (per chain its mode, or MODE_NONE for a chain not to count).
    The model's histogram is reset and its modes are set for the run (they stay set); every mode's reference is its member
    chain of the lowest description length at the first sample.  Returns a dict (M modes):
      modes      the grouping used: the dict of partition_modes, or the mode_of_chain array
      labels     uint32 [M, n]        MAP block of every node within the mode
      top        uint32 [M, n]        that block's count; top / terms[g] says how settled the node is within mode g
      counts     int64  [M, n, kmax]  the histograms
      terms      uint64 [M]           chain samples in every histogram
      weights    [M]                  each mode's share of the counted chains
      ref_chain  int64  [M]           the chain every mode's reference came from (-1: the caller's)
      moved      the number of chains whose set of co-members under the same threshold differs after the last sample (0 with
                 `mode_of_chain`): whether the chains stayed in their modes while they were sampled
    `reassign`: anchored modes (include/bisbm.h, "Anchored modes").  The grouping (with `threshold`, after the burn-in) only
    chooses the anchors -- the labels of every mode's `lowest_entropy` chain -- and every sample counts each chain into the mode
    of its nearest anchor if its VI to it is <= threshold.  The dict then also has `unassigned` (counted chains beyond the
    threshold, over all samples) and `visits` uint64 [n_chains, M]; `weights` are the sample shares
    terms / (sum of terms + unassigned), `moved` is the number of chains counted into more than one mode, and `ref_chain` is -1
    throughout.  `tempering` (with `reassign` only; ValueError otherwise): a temperature ladder as in marginalize(); burn-in
    and the gaps between samples run through model.tempering_run(sweeps, exchange_every), the grouping and every sample take
    the chains on rung 0.  `mode_of_chain` with `reassign` is a ValueError: the anchors come from a grouping.
    `rung_moves` (with `tempering` only): the moves of a round, as in marginalize(); burn-in and gaps count rounds then.
    `sampler`: "mh" or "heatbath", as in marginalize().  `trace`: a depth, as in marginalize() -- one model.trace_record() after
    every sample; the dict does not change.
    `blocks`: the block sums (include/bisbm.h, "Block summaries") are turned on, zeroed, before the first sample; the dict does
    not change, model.block_summary(g) gives mode g's block matrix, sizes and degrees with their spread afterwards.
    `clamp`: node ids or a mask, as in marginalize(): set before the burn-in and left set.
    `constraints`: (class_of_node, allowed), as in marginalize(): set before the burn-in and left set.
    `fields`: (class_of_node, field), as in marginalize(): set before the burn-in and left set.
    `conditionals`: (nodes, beta) or (nodes,), as in marginalize(): the queries are set before the first sample, every sample
    also takes one conditional sample of every counted chain (pooled over the modes: per-mode conditionals are not kept, and
    there are no soft marginals), and the dict gets "conditionals": model.conditionals_stats().  `conditionals_held` and
    `least_settled` = (k, by), both with `conditionals` only (ValueError without), as in marginalize(): the held row, and
    "least_settled": model.least_settled(k, by) in the dict.
    Chains spread over ranks (`shard`, or model.shard, with world_size > 1) raise ValueError: pooling modes across ranks is
    not done here."""
    if (threshold is None) == (mode_of_chain is None):
        raise ValueError("exactly one of threshold and mode_of_chain must be given")
    if tempering is not None and not reassign:
        raise ValueError("tempering needs reassign=True: chains that trade temperatures have no fixed mode")
    if reassign and mode_of_chain is not None:
        raise ValueError("reassign takes its anchors from a grouping: give threshold, not mode_of_chain")
    _check_conditional_extras(conditionals, conditionals_held, least_settled)
    shard = shard if shard is not None else getattr(model, "shard", None)
    if shard is not None and getattr(shard, "world_size", 1) > 1:
        raise ValueError("marginalize_modes serves the chains of one rank: pooling modes across ranks is not done here")
    from . import mode_assignment
    if mode_of_chain is not None:
        moc, n_modes = mode_assignment(mode_of_chain, model.n_chains)
    if clamp is not None:
        model.clamp(clamp)
    if constraints is not None:
        model.constrain(*constraints)
    if fields is not None:
        model.set_fields(*fields)
    advance = _advance(model, tempering, exchange_every, sampler, rung_moves=rung_moves)
    if burn_in_sweeps > 0:
        advance(burn_in_sweeps)
    if threshold is not None:
        modes = model.partition_modes(threshold)
        moc, n_modes = mode_assignment(modes, model.n_chains)
    else:
        modes = moc.copy()
    model.marginals_reset()
    if reassign:
        anchors = np.array([model.get_memberships(int(c)) for c in modes["lowest_entropy"]], dtype=np.uint32)
        model.marginals_set_mode_anchors(anchors, threshold)
    else:
        model.marginals_set_modes(moc, n_modes)
    if blocks:
        model.block_sums_set(True)
    if conditionals is not None:
        model.conditionals_set(conditionals[0], conditionals[1] if len(conditionals) > 1 else 1.0)
        if conditionals_held:
            model.conditionals_held(True)
    _trace_start(model, trace)
    for _ in range(int(n_samples)):
        if sampling_frequency_sweeps > 0:
            advance(sampling_frequency_sweeps)
        model.marginals_accumulate(None)
        if trace:
            model.trace_record()
        if conditionals is not None:
            model.conditionals_accumulate()
    extras = {}
    if conditionals is not None:
        extras["conditionals"] = model.conditionals_stats()
        if least_settled is not None:
            extras["least_settled"] = model.least_settled(int(least_settled[0]), least_settled[1] if len(least_settled) > 1 else "entropy")
    state = model.marginals_modes()
    labels = np.zeros((n_modes, model.n), dtype=np.uint32)
    top = np.zeros((n_modes, model.n), dtype=np.uint32)
    counts = np.zeros((n_modes, model.n, model.kmax), dtype=np.int64)
    for g in range(n_modes):
        counts[g] = model.marginals_get(mode=g)
        if int(state["terms"][g]) > 0:
            labels[g], top[g] = model.marginals_map(mode=g, return_top=True)
    if reassign:
        visits = model.marginals_mode_assignment()["visits"]
        return {"modes": modes, "labels": labels, "top": top, "counts": counts, "terms": state["terms"], "weights": state["weights"],
                "ref_chain": state["ref_chain"], "moved": int(((visits > 0).sum(axis=1) > 1).sum()), "unassigned": state["unassigned"],
                "visits": visits, **extras}
    moved = 0
    if threshold is not None:
        after = model.partition_modes(threshold, chains=modes["chains"])
        moved = int(sum(_co_members(modes, c) != _co_members(after, c) for c in range(len(modes["chains"]))))
    return {"modes": modes, "labels": labels, "top": top, "counts": counts, "terms": state["terms"], "weights": state["weights"],
            "ref_chain": state["ref_chain"], "moved": moved, **extras}


def _check_conditional_extras(conditionals, conditionals_held, least_settled):
    """conditionals_held / least_settled of marginalize() / marginalize_modes(): refused without `conditionals`, and a malformed
    `least_settled`, before anything is set or run."""
    if conditionals is None and conditionals_held:
        raise ValueError("conditionals_held=True switches the row of the node conditionals: it needs conditionals=(nodes, beta)")
    if conditionals is None and least_settled is not None:
        raise ValueError("least_settled ranks the queries of the node conditionals: it needs conditionals=(nodes, beta)")
    if least_settled is not None:
        if not 1 <= len(least_settled) <= 2 or (len(least_settled) > 1 and least_settled[1] not in ("entropy", "stay")):
            raise ValueError("least_settled must be (k, by) or (k,), by = \"entropy\" or \"stay\"")


def _trace_start(model, trace):
    """trace=depth of marginalize() / marginalize_modes(): the ring set and everything forgotten before the first sample."""
    if trace is None or int(trace) == 0:
        return
    if int(trace) < 0:
        raise ValueError("trace must be a depth >= 0")
    model.trace_set(int(trace))
    model.trace_reset()


def _advance(model, tempering, exchange_every, sampler, reshuffles=0, reshuffle_scans=3, rung_moves=None):
    """The call that runs the sweeps of the burn-in and between samples: MH at T = 1, heat-bath sweeps at beta = 1, or -- with
    a ladder, which is set here -- replica exchange.  reshuffles > 0: every such block of sweeps is followed by that many pair
    reshuffles at beta = 1.  rung_moves (with a ladder only): the blocks are rounds of model.tempering_rounds."""
    if rung_moves is not None and tempering is None:
        raise ValueError("rung_moves describes the rounds of replica exchange: it needs tempering=ladder")
    if sampler not in ("mh", "heatbath"):
        raise ValueError("sampler must be \"mh\" or \"heatbath\", not %r" % (sampler,))
    if int(reshuffles) < 0 or int(reshuffle_scans) < 0:
        raise ValueError("reshuffles and reshuffle_scans must not be negative")
    if int(reshuffles) > 0:
        if tempering is not None:
            raise ValueError("reshuffles cannot be combined with tempering: pair reshuffles inside replica exchange are asked for with "
                             "rung_moves={\"mh\": 1, \"reshuffles\": m, \"scans\": t}")
        sweeps_only = _advance(model, None, exchange_every, sampler)
        model.reshuffle_stats = {"proposed": 0, "accepted": 0}

        def block(sweeps):
            sweeps_only(sweeps)
            acc = model.reshuffle(int(reshuffles), int(reshuffle_scans), 1.0)
            model.reshuffle_stats["proposed"] += int(reshuffles) * model.n_chains
            model.reshuffle_stats["accepted"] += int(acc.sum())
        return block
    if tempering is not None:
        if sampler == "heatbath":
            raise ValueError("sampler=\"heatbath\" cannot be combined with tempering: heat-bath sweeps inside replica exchange are asked "
                             "for with rung_moves={\"mh\": 0, \"heatbath\": k}")
        if rung_moves is not None:
            from . import rung_moves_recipe
            recipe = rung_moves_recipe(rung_moves)
            model.set_tempering(tempering)
            return lambda rounds: model.tempering_rounds(rounds, **recipe)
        model.set_tempering(tempering)
        return lambda sweeps: model.tempering_run(sweeps, exchange_every)
    if sampler == "heatbath":
        return lambda sweeps: model.heatbath_sweeps(sweeps, 1.0)
    return model.run_sweeps


def _co_members(grouping, i):
    """The chains that share a mode with the i-th selected chain of a partition_modes dict."""
    mode = np.asarray(grouping["mode"])
    return frozenset(np.asarray(grouping["chains"])[mode == mode[i]].tolist())


def _drop_library_reference(model):
    """A reference the library took at an earlier run (no reset since) is taken afresh; a caller's stays."""
    from . import BisbmError
    try:
        chain = model.marginals_reference()[1]
    except BisbmError:
        return
    if chain >= 0:
        model.marginals_set_reference(None)


def _uses_cuda_backend(shard):
    import torch.distributed as dist
    return dist.is_initialized() and dist.get_backend(shard.group) == "nccl"
