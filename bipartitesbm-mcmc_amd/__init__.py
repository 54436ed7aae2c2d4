"""bipartitesbm-mcmc_amd -- host-side mirror of the reference's class API over the HIP C ABI.

The product is ``libbisbm_hip.so`` (csrc/, C ABI in include/bisbm.h): HIP kernels for gfx950 that
replace ``metropolis_hasting::anneal/step/transition_ratio`` and the hot part of ``blockmodel_t``
of junipertcy/bipartiteSBM-MCMC.  This module only binds it with ctypes and mirrors the names a
user of the reference knows (``blockmodel_t`` -> :class:`BlockModel`, ``metropolis_hasting`` ->
:class:`MetropolisHasting``, the five ``*_schedule`` functions, ``load_edge_list`` /
``edge_to_adj`` / ``load_memberships`` / ``output_vec``).

There is no CPU fallback: if the shared library cannot be loaded, importing the bound functions
raises, and ``bisbm_create`` fails with BISBM_ERR_NO_DEVICE when no HIP device is present.

The directory name contains a hyphen; load it with
``importlib.import_module("bipartitesbm-mcmc_amd")``.
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbisbm_hip.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

# --------------------------------------------------------------------------- enums of include/bisbm.h
BISBM_OK = 0
BISBM_ERR_INVALID_ARG = 1
BISBM_ERR_NOT_BIPARTITE = 2
BISBM_ERR_UNSUPPORTED = 3
BISBM_ERR_NO_DEVICE = 4
BISBM_ERR_HIP = 5
BISBM_ERR_STATE = 6
ALIGN_NONE = 0
ALIGN_REFERENCE = 1
MODE_NONE = 0xFFFFFFFF  # BISBM_MODE_NONE: a chain that no mode counts
RNG_PHILOX = 0
RNG_MT19937_COMPAT = 1
ALL_CHAINS = -1
# bisbm_query_scores_*: candidates x queries of one workgroup of the accumulate kernel and the largest k of the top-k selection
# (csrc/bisbm_kernels.hpp: kQueryCandTile, kQueryTile, kQueryMaxK), and the entry past a query's eligible candidates
QUERY_CAND_TILE, QUERY_TILE, QUERY_MAX_K = 1024, 8, 1024
QUERY_NONE = 0xFFFFFFFF
# bisbm_coassign_*: candidates x queries of one workgroup of the counting kernel (csrc/bisbm_kernels.hpp: kCoassignCandTile,
# kCoassignTile); the largest k of bisbm_coassign_topk is QUERY_MAX_K, an entry past the eligible nodes QUERY_NONE
COASSIGN_CAND_TILE, COASSIGN_TILE = 1024, 16
# bisbm_edge_probs_*: the kinds of a pair (BISBM_EDGE_ADD, BISBM_EDGE_REMOVE), the bit of `what` that keeps the last sample's dS
# (BISBM_EDGE_KEEP_LAST) and the pairs of one workgroup of the dS kernel (csrc/bisbm_engine.hpp: kEdgeProbsTile)
EDGE_ADD, EDGE_REMOVE, EDGE_KEEP_LAST = 0, 1, 1
EDGE_PROBS_TILE = 1024
# bisbm_edge_queries_*: candidates x queries of one workgroup of the accumulate kernel (csrc/bisbm_kernels.hpp: kEdgeQueryCandTile,
# kEdgeQueryTile); the largest k of bisbm_edge_queries_topk is QUERY_MAX_K, an entry past the eligible candidates QUERY_NONE
EDGE_QUERY_CAND_TILE, EDGE_QUERY_TILE = 1024, 8
# bisbm_foldin_*: the row kinds (BISBM_FOLDIN_RECOMMEND, BISBM_FOLDIN_SIMILAR) and candidates x virtual nodes of one workgroup of
# the rows kernel (csrc/bisbm_kernels.hpp: kFoldinCandTile, kFoldinTile); the largest k of bisbm_foldin_topk is QUERY_MAX_K
FOLDIN_RECOMMEND, FOLDIN_SIMILAR = 1, 2
FOLDIN_CAND_TILE, FOLDIN_TILE = 1024, 8
# bisbm_conditionals_*: the bit of `what` that keeps the last sample's rows
COND_KEEP_LAST = 1
# bisbm_least_settled_topk: the statistic that is ranked (BISBM_SETTLED_BY_ENTROPY, BISBM_SETTLED_BY_STAY); the largest k is
# QUERY_MAX_K, an entry past the queries QUERY_NONE
SETTLED_BY_ENTROPY, SETTLED_BY_STAY = 0, 1
# the Philox purpose of the heat-bath draw (csrc/bisbm_kernels.hpp: PHX_HEATBATH; DESIGN.md section 4 lists them all)
PHILOX_PURPOSE_HEATBATH = 9
# ... and of the pair reshuffles (PHX_RESHUFFLE), and the record type of a move without a pair (BISBM_RESHUFFLE_NONE)
PHILOX_PURPOSE_RESHUFFLE = 10
RESHUFFLE_NONE = 0xFFFFFFFF
# ... of the split and merge moves (bisbm_split_merge.hip: PHX_SPLIT_MERGE), the kinds of a move (BISBM_SM_SPLIT, BISBM_SM_MERGE) and
# why a proposal was refused without an evaluation (BISBM_SM_EVALUATED: it was not)
PHILOX_PURPOSE_SPLIT_MERGE = 11
SM_SPLIT, SM_MERGE = 0, 1
SM_EVALUATED, SM_SINGLETON, SM_AT_K_MAX, SM_AT_K_MIN, SM_NO_PAIR = 0, 1, 2, 3, 4
# bisbm_trace_get_series: which series (BISBM_TRACE_S, BISBM_TRACE_H)
TRACE_S, TRACE_H = 0, 1
# bisbm_block_sums_set: keep the sums; also keep every counted chain's aligned tables of the last sample
BLOCK_SUMS, BLOCK_KEEP_LAST = 1, 2
# bisbm_last_sweep_route (BISBM_ROUTE_*): the production kernel ran; the launch carried a clamp or constraints; it carried fields
ROUTE_PRODUCTION, ROUTE_HELD, ROUTE_FIELDS = 1, 2, 4
_RNG = {"philox": RNG_PHILOX, "mt19937-compat": RNG_MT19937_COMPAT, "compat": RNG_MT19937_COMPAT}

_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)
_f32p = C.POINTER(C.c_float)


class RoundRecipe(C.Structure):
    """bisbm_round_recipe (include/bisbm.h, "Heat-bath sweeps and pair reshuffles inside replica exchange")"""
    _fields_ = [("mh_sweeps", C.c_uint32), ("heatbath_sweeps", C.c_uint32), ("reshuffles", C.c_uint32), ("reshuffle_scans", C.c_uint32)]


class ReshuffleRecord(C.Structure):
    """bisbm_reshuffle_record (include/bisbm.h, "Pair reshuffles")"""
    _fields_ = [("type", C.c_uint32), ("r", C.c_uint32), ("s", C.c_uint32), ("M", C.c_uint32),
                ("dS_fwd", C.c_double), ("dS_rev", C.c_double), ("q_fwd_mant", C.c_double), ("q_rev_mant", C.c_double),
                ("q_fwd_exp", C.c_int32), ("q_rev_exp", C.c_int32), ("u_acc", C.c_double), ("A", C.c_double),
                ("accepted", C.c_uint32), ("reserved", C.c_uint32)]


class SplitMergeRecord(C.Structure):
    """bisbm_split_merge_record (include/bisbm.h, "Split and merge moves")"""
    _fields_ = [("kind", C.c_uint32), ("type", C.c_uint32), ("r", C.c_uint32), ("s", C.c_uint32), ("M", C.c_uint32), ("refused", C.c_uint32),
                ("q_mant", C.c_double), ("q_exp", C.c_int32), ("accepted", C.c_uint32),
                ("dS", C.c_double), ("lnA", C.c_double), ("A", C.c_double), ("u_acc", C.c_double),
                ("ka_before", C.c_uint32), ("kb_before", C.c_uint32), ("ka_after", C.c_uint32), ("kb_after", C.c_uint32)]


# every symbol include/bisbm.h and include/bisbm_io.h declare: (restype, argtypes)
ABI = {
    "bisbm_abi_version": (C.c_int, []),
    "bisbm_check_shape": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int]),
    "bisbm_create_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint64, C.c_uint64, C.c_uint64, _u64p, _u32p, C.c_uint32, C.c_uint32,
                                     C.c_double, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_uint64, C.c_uint64]),
    "bisbm_device_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _u32p]),
    "bisbm_marginals_map": (C.c_int, [C.c_void_p, _u32p]),
    "bisbm_last_error": (C.c_char_p, [C.c_void_p]),
    "bisbm_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint64, C.c_uint64, C.c_uint64, _u64p, _u32p,
                               C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                               C.c_uint64, C.c_uint64]),
    "bisbm_destroy": (C.c_int, [C.c_void_p]),
    "bisbm_set_memberships": (C.c_int, [C.c_void_p, C.c_int64, _u32p]),
    "bisbm_init": (C.c_int, [C.c_void_p]),
    "bisbm_shuffle": (C.c_int, [C.c_void_p]),
    "bisbm_anneal": (C.c_int, [C.c_void_p, C.c_int, _f32p, C.c_uint64, C.c_uint64, _f64p]),
    "bisbm_get_memberships": (C.c_int, [C.c_void_p, C.c_uint32, _u32p]),
    "bisbm_get_block_state": (C.c_int, [C.c_void_p, C.c_uint32, _i32p, _i32p, _i32p, _u32p]),
    "bisbm_get_cum_dS": (C.c_int, [C.c_void_p, _f64p]),
    "bisbm_entropy": (C.c_int, [C.c_void_p, _f64p]),
    "bisbm_get_last_counts": (C.c_int, [C.c_void_p, _u64p, _u64p]),
    "bisbm_marginals_accumulate": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bisbm_marginals_reset": (C.c_int, [C.c_void_p]),
    "bisbm_marginals_get": (C.c_int, [C.c_void_p, _u32p]),
    "bisbm_marginals_set_alignment": (C.c_int, [C.c_void_p, C.c_int]),
    "bisbm_marginals_set_reference": (C.c_int, [C.c_void_p, _u32p]),
    "bisbm_marginals_get_reference": (C.c_int, [C.c_void_p, _u32p, C.POINTER(C.c_int64)]),
    "bisbm_marginals_get_alignment": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, _u64p]),
    "bisbm_align_assignment": (C.c_int, [C.c_uint32, _u32p, _u32p, _u64p]),
    "bisbm_marginals_set_modes": (C.c_int, [C.c_void_p, C.c_uint32, _u32p]),
    "bisbm_marginals_get_modes": (C.c_int, [C.c_void_p, _u32p, _u32p, C.POINTER(C.c_int64), _u64p]),
    "bisbm_marginals_set_mode_reference": (C.c_int, [C.c_void_p, C.c_uint32, _u32p]),
    "bisbm_marginals_set_mode_anchors": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, C.c_double]),
    "bisbm_marginals_get_mode_assignment": (C.c_int, [C.c_void_p, _f64p, _u64p, _u64p, _u64p]),
    "bisbm_marginals_get_mode_reference": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, C.POINTER(C.c_int64)]),
    "bisbm_marginals_get_mode": (C.c_int, [C.c_void_p, C.c_uint32, _u32p]),
    "bisbm_marginals_map_mode": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, _u32p]),
    "bisbm_tempering_set": (C.c_int, [C.c_void_p, C.c_uint32, _f32p]),
    "bisbm_tempering_run": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, _f64p]),
    "bisbm_tempering_get": (C.c_int, [C.c_void_p, _u32p, _f32p]),
    "bisbm_tempering_stats": (C.c_int, [C.c_void_p, _u64p, _u64p, _u64p]),
    "bisbm_tempering_run_rounds": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(RoundRecipe), C.c_int]),
    "bisbm_tempering_rung_stats": (C.c_int, [C.c_void_p, _u64p]),
    "bisbm_rounds_population_run": (C.c_int, [C.c_void_p, C.c_uint32, _f32p, C.c_uint64, C.POINTER(RoundRecipe), _f64p, _u32p, _f64p]),
    "bisbm_population_offspring": (C.c_int, [C.c_uint32, _f64p, C.c_double, C.c_double, _u32p, _u32p, _f64p]),
    "bisbm_population_resample": (C.c_int, [C.c_void_p, C.c_double, C.c_double, _u32p, _f64p]),
    "bisbm_population_run": (C.c_int, [C.c_void_p, C.c_uint32, _f32p, C.c_uint64, _f64p, _u32p, _f64p]),
    "bisbm_population_get": (C.c_int, [C.c_void_p, _u32p, _u64p, _f64p]),
    "bisbm_population_reset": (C.c_int, [C.c_void_p]),
    "bisbm_pair_scores_set": (C.c_int, [C.c_void_p, C.c_uint64, _u32p, _u32p]),
    "bisbm_pair_scores_accumulate": (C.c_int, [C.c_void_p]),
    "bisbm_pair_scores_reset": (C.c_int, [C.c_void_p]),
    "bisbm_pair_scores_get": (C.c_int, [C.c_void_p, _f64p, _u64p]),
    "bisbm_edge_probs_set": (C.c_int, [C.c_void_p, C.c_uint64, _u32p, _u32p, _u8p, C.c_uint32]),
    "bisbm_edge_probs_accumulate": (C.c_int, [C.c_void_p]),
    "bisbm_edge_probs_reset": (C.c_int, [C.c_void_p]),
    "bisbm_edge_probs_get": (C.c_int, [C.c_void_p, _f64p, _f64p, _u32p, _u64p]),
    "bisbm_edge_probs_get_last": (C.c_int, [C.c_void_p, C.c_uint64, _f64p]),
    "bisbm_edge_queries_set": (C.c_int, [C.c_void_p, C.c_uint32, _u32p]),
    "bisbm_edge_queries_accumulate": (C.c_int, [C.c_void_p]),
    "bisbm_edge_queries_reset": (C.c_int, [C.c_void_p]),
    "bisbm_edge_queries_get_row": (C.c_int, [C.c_void_p, C.c_uint32, _f64p, _u32p, _u64p]),
    "bisbm_edge_queries_topk": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, _u32p, _f64p, _u64p]),
    "bisbm_query_scores_set": (C.c_int, [C.c_void_p, C.c_uint32, _u32p]),
    "bisbm_query_scores_accumulate": (C.c_int, [C.c_void_p]),
    "bisbm_query_scores_reset": (C.c_int, [C.c_void_p]),
    "bisbm_query_scores_get_row": (C.c_int, [C.c_void_p, C.c_uint32, _f64p, _u64p]),
    "bisbm_query_scores_topk": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, _u32p, _f64p, _u64p]),
    "bisbm_coassign_set": (C.c_int, [C.c_void_p, C.c_uint32, _u32p]),
    "bisbm_coassign_accumulate": (C.c_int, [C.c_void_p]),
    "bisbm_coassign_reset": (C.c_int, [C.c_void_p]),
    "bisbm_coassign_get_row": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, _u64p]),
    "bisbm_coassign_topk": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, _u32p, _u64p]),
    "bisbm_foldin_set": (C.c_int, [C.c_void_p, C.c_uint32, _u8p, _u64p, _u32p, C.c_double, C.c_uint32]),
    "bisbm_foldin_accumulate": (C.c_int, [C.c_void_p]),
    "bisbm_foldin_reset": (C.c_int, [C.c_void_p]),
    "bisbm_foldin_get_posteriors": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _f64p]),
    "bisbm_foldin_get_row": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _f64p, _u64p]),
    "bisbm_foldin_topk": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, _u32p, _f64p, _u64p]),
    "bisbm_conditionals_set": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, C.c_double, C.c_uint32]),
    "bisbm_conditionals_set_reference": (C.c_int, [C.c_void_p, _u32p]),
    "bisbm_conditionals_accumulate": (C.c_int, [C.c_void_p]),
    "bisbm_conditionals_reset": (C.c_int, [C.c_void_p]),
    "bisbm_conditionals_get_stats": (C.c_int, [C.c_void_p, _f64p, _f64p, _f64p, _u64p, _u64p]),
    "bisbm_conditionals_get_marginals": (C.c_int, [C.c_void_p, _f64p, _u32p, _u64p]),
    "bisbm_conditionals_get_last": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _f64p, _f64p]),
    "bisbm_held_conditionals_set": (C.c_int, [C.c_void_p, C.c_int]),
    "bisbm_held_conditionals_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "bisbm_least_settled_topk": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _u32p, _f64p, _u64p]),
    "bisbm_heatbath_run": (C.c_int, [C.c_void_p, C.c_uint64, C.c_double, C.c_int, _u64p, _u64p]),
    "bisbm_reshuffle_run": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, _u64p]),
    "bisbm_reshuffle_get_last": (C.c_int, [C.c_void_p, C.POINTER(ReshuffleRecord)]),
    "bisbm_reshuffle_get_total": (C.c_int, [C.c_void_p, _u64p]),
    "bisbm_split_merge_run": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, _u32p, _u32p, _u64p]),
    "bisbm_split_merge_get_last": (C.c_int, [C.c_void_p, C.POINTER(SplitMergeRecord)]),
    "bisbm_split_merge_get_total": (C.c_int, [C.c_void_p, _u64p]),
    "bisbm_split_merge_get_groups": (C.c_int, [C.c_void_p, _u32p]),
    "bisbm_split_merge_get_timing": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "bisbm_split_merge_shape_term": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _f64p]),
    "bisbm_clamp_set": (C.c_int, [C.c_void_p, _u8p]),
    "bisbm_clamp_get": (C.c_int, [C.c_void_p, _u8p, _u64p]),
    "bisbm_constraints_set": (C.c_int, [C.c_void_p, C.c_uint32, _u8p, _u8p]),
    "bisbm_constraints_get": (C.c_int, [C.c_void_p, _u32p, _u8p, _u8p]),
    "bisbm_fields_set": (C.c_int, [C.c_void_p, C.c_uint32, _u8p, _f64p]),
    "bisbm_fields_get": (C.c_int, [C.c_void_p, _u32p, _u8p, _f64p]),
    "bisbm_fields_energy": (C.c_int, [C.c_void_p, _f64p]),
    "bisbm_debug_exp": (C.c_int, [C.c_void_p, _f64p, C.c_size_t, _f64p]),
    "bisbm_debug_log": (C.c_int, [C.c_void_p, _f64p, C.c_size_t, _f64p]),
    "bisbm_partition_distances": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, _f64p, _f64p]),
    "bisbm_partition_distances_to": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, C.c_uint32, _u32p, _u32p, _u32p, _f64p, _f64p]),
    "bisbm_partition_contingency": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _u32p]),
    "bisbm_partition_modes": (C.c_int, [C.c_uint32, _f64p, C.c_double, _u32p, _u32p, _u32p]),
    "bisbm_trace_set": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bisbm_trace_record": (C.c_int, [C.c_void_p]),
    "bisbm_trace_reset": (C.c_int, [C.c_void_p]),
    "bisbm_trace_get_lags": (C.c_int, [C.c_void_p, _f64p, _u64p, _f64p, _u64p, _u64p]),
    "bisbm_trace_get_series": (C.c_int, [C.c_void_p, C.c_int, _f64p]),
    "bisbm_trace_summary": (C.c_int, [C.c_uint64, C.c_uint32, _f64p, C.c_double, _f64p, _u32p, _f64p]),
    "bisbm_block_sums_set": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bisbm_block_sums_get": (C.c_int, [C.c_void_p, C.c_uint32, _u64p, _u64p, _u64p, _u64p]),
    "bisbm_block_sums_get_last": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, _i32p, _i32p, _i32p]),
    "bisbm_get_ka_kb": (C.c_int, [C.c_void_p, _u32p, _u32p]),
    "bisbm_get_ka_kb_chain": (C.c_int, [C.c_void_p, C.c_uint32, _u32p, _u32p]),
    "bisbm_agg_merge": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "bisbm_agg_merge_total": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "bisbm_get_sizes": (C.c_int, [C.c_void_p, _u64p, _u64p, _u32p, _u32p]),
    "bisbm_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bisbm_last_sweep_timing": (C.c_int, [C.c_void_p, _f64p, _u64p]),
    "bisbm_last_pass_steps": (C.c_int, [C.c_void_p, _u32p]),
    "bisbm_last_eta_plan": (C.c_int, [C.c_void_p, _u32p]),
    "bisbm_last_sweep_route": (C.c_int, [C.c_void_p, _u32p]),
    "bisbm_debug_log_q": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_size_t, C.c_int, _f64p]),
    "bisbm_io_read_edge_list": (C.c_long, [C.c_char_p, C.POINTER(_u64p), C.POINTER(_u64p)]),
    "bisbm_io_read_memberships": (C.c_long, [C.c_char_p, C.POINTER(_u32p)]),
    "bisbm_io_read_clamp": (C.c_long, [C.c_char_p, C.c_uint64, C.POINTER(_u8p), C.c_char_p, C.c_size_t]),
    "bisbm_io_read_constraints": (C.c_long, [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(_u8p), C.POINTER(_u8p),
                                             C.c_char_p, C.c_size_t]),
    "bisbm_io_read_fields": (C.c_long, [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(_u8p), C.POINTER(_f64p),
                                        C.c_char_p, C.c_size_t]),
    "bisbm_io_edges_to_csr": (C.c_int, [_u64p, _u64p, C.c_size_t, C.c_uint64, _u64p, _u32p]),
    "bisbm_io_load_csr": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(_u64p), C.POINTER(_u32p), _u64p,
                                    C.POINTER(C.c_int)]),
    "bisbm_io_locality_order": (C.c_int, [C.c_uint64, C.c_uint64, _u64p, _u32p, _u32p]),
    "bisbm_io_permute_csr": (C.c_int, [C.c_uint64, _u64p, _u32p, _u32p, _u64p, _u32p]),
    "bisbm_io_format_labels": (C.c_size_t, [_u32p, C.c_size_t, C.c_char_p, C.c_size_t]),
    "bisbm_io_free": (None, [C.c_void_p]),
}

_lib = None


def build(force=False, verbose=False):
    """Compile csrc/ with hipcc for gfx950 into libbisbm_hip.so (in-tree)."""
    spec = importlib.util.spec_from_file_location("_bisbm_build", os.path.join(_HERE, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(force=force, verbose=verbose)


def lib():
    """The loaded C-ABI library.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libbisbm_hip.so is not built (run __graft_entry__.build() or "
                "`python bipartitesbm-mcmc_amd/build.py`); the engine has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class BisbmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bisbm error %d: %s" % (code, msg))
        self.code = code


def _p(a, t):
    return a.ctypes.data_as(t)


# --------------------------------------------------------------------------- cooling schedules
# metropolis_hasting.cc:10-37.  The reference passes a function pointer to anneal(); here the five
# functions are callables that also carry the id the kernel switches on.
class _Schedule:
    def __init__(self, name, sid):
        self.__name__ = name
        self.id = sid

    def __repr__(self):
        return "<%s>" % self.__name__


exponential_schedule = _Schedule("exponential_schedule", 0)
linear_schedule = _Schedule("linear_schedule", 1)
logarithmic_schedule = _Schedule("logarithmic_schedule", 2)
constant_schedule = _Schedule("constant_schedule", 3)
abrupt_cool_schedule = _Schedule("abrupt_cool_schedule", 4)
SCHEDULES = {
    "exponential": exponential_schedule, "linear": linear_schedule, "logarithmic": logarithmic_schedule,
    "constant": constant_schedule, "abrupt_cool": abrupt_cool_schedule,
}


def _schedule_id(s):
    if isinstance(s, _Schedule):
        return s.id
    if isinstance(s, str):
        return SCHEDULES[s].id
    return int(s)


# --------------------------------------------------------------------------- graph / membership I/O
def load_edge_list(path):
    """graph_utilities.cc:20-34 -> (a, b) uint64 arrays, one entry per line of the file."""
    L = lib()
    a, b = _u64p(), _u64p()
    n = L.bisbm_io_read_edge_list(os.fsencode(path), C.byref(a), C.byref(b))
    if n < 0:
        raise FileNotFoundError(path)
    ea = np.ctypeslib.as_array(a, shape=(max(n, 1),))[:n].copy()
    eb = np.ctypeslib.as_array(b, shape=(max(n, 1),))[:n].copy()
    L.bisbm_io_free(a)
    L.bisbm_io_free(b)
    return ea, eb


def load_memberships(path):
    """graph_utilities.cc:5-18 -> uint32 labels."""
    L = lib()
    p = _u32p()
    n = L.bisbm_io_read_memberships(os.fsencode(path), C.byref(p))
    if n < 0:
        raise FileNotFoundError(path)
    out = np.ctypeslib.as_array(p, shape=(max(n, 1),))[:n].copy()
    L.bisbm_io_free(p)
    return out


def load_clamp(path, n):
    """The clamp file of ``mcmc --clamp`` (include/bisbm_io.h): node ids < n separated by white space, any order, repeats
    allowed, an empty file an empty clamp -> bool mask [n].  ValueError, with the token named, for a token that is no node id."""
    L = lib()
    p = _u8p()
    err = C.create_string_buffer(512)
    count = L.bisbm_io_read_clamp(os.fsencode(path), int(n), C.byref(p), err, len(err))
    if count == -1:
        raise FileNotFoundError(path)
    if count < 0:
        raise ValueError(err.value.decode())
    out = np.ctypeslib.as_array(p, shape=(max(int(n), 1),))[:int(n)].astype(bool)
    L.bisbm_io_free(p)
    return out


def load_constraints(path, na, nb, ka, kb):
    """The constraints file of ``mcmc --constraints`` (include/bisbm_io.h): one line per constrained node, its id and then its
    allowed blocks -> (class_of_node uint8 [n], allowed bool [n_classes, ka + kb]) for BlockModel.constrain; class 0 allows
    everything and holds the unlisted nodes.  ValueError, with the token named, for a malformed line."""
    L = lib()
    pc, pa = _u8p(), _u8p()
    err = C.create_string_buffer(512)
    n = int(na) + int(nb)
    count = L.bisbm_io_read_constraints(os.fsencode(path), n, int(na), int(ka), int(kb), C.byref(pc), C.byref(pa), err, len(err))
    if count == -1:
        raise FileNotFoundError(path)
    if count < 0:
        raise ValueError(err.value.decode())
    K = int(ka) + int(kb)
    cls = np.ctypeslib.as_array(pc, shape=(max(n, 1),))[:n].copy()
    allowed = np.ctypeslib.as_array(pa, shape=(count * K,)).reshape(count, K).astype(bool)
    L.bisbm_io_free(pc)
    L.bisbm_io_free(pa)
    return cls, allowed


def constraints_from_lists(n, K, lists, na=None, ka=None):
    """(class_of_node uint8 [n], allowed bool [n_classes, K]) from {node: [allowed blocks]}: unlisted nodes get class 0, which
    allows everything, and every distinct list (as a set) gets the next class -- at most 255 of them beside class 0, so that a
    class id is one byte; more is a ValueError.  With `na` and `ka` (the type-a nodes are 0 .. na-1, the type-a blocks
    0 .. ka-1) the columns of the other type are set, as the loader of the command line sets them, and a list that names a
    block of the other type is a ValueError; without them the row is the list as given (the engine ignores the other type)."""
    n, K = int(n), int(K)
    cls = np.zeros(n, dtype=np.uint8)
    rows, index = [np.ones(K, dtype=bool)], {}
    for v in sorted(lists):
        blocks = sorted(set(int(s) for s in lists[v]))
        if not 0 <= int(v) < n:
            raise ValueError("node %r is not in [0, %d)" % (v, n))
        if not blocks or blocks[0] < 0 or blocks[-1] >= K:
            raise ValueError("node %r: a non-empty list of blocks in [0, %d) is needed" % (v, K))
        row = np.zeros(K, dtype=bool)
        row[blocks] = True
        if na is not None:
            tb = int(v) >= int(na)
            if any((s >= int(ka)) != tb for s in blocks):
                raise ValueError("node %r: a block of the other type is listed" % (v,))
            row[:int(ka)] |= tb
            row[int(ka):] |= not tb
        key = row.tobytes()
        if key == rows[0].tobytes():
            continue
        if key not in index:
            if len(rows) == 256:
                raise ValueError("more than 255 distinct lists beside class 0: a class id is one byte")
            index[key] = len(rows)
            rows.append(row)
        cls[int(v)] = index[key]
    return cls, np.array(rows)


def admissible_start(na, nb, ka, kb, class_of_node, allowed):
    """A label vector that the constraints admit: the nodes of each (type, class), in ascending id, are dealt round-robin over
    the allowed blocks of their type in ascending order.  ValueError when a class allows a node nothing, or when a block ends
    up empty (no sampler ever empties a block, so such a start could not be left)."""
    na, nb, ka, kb = int(na), int(nb), int(ka), int(kb)
    cls = np.asarray(class_of_node)
    allowed = np.asarray(allowed) != 0
    out = np.zeros(na + nb, dtype=np.uint32)
    for lo, hi, b0, b1 in ((0, na, 0, ka), (na, na + nb, ka, ka + kb)):
        for c in np.unique(cls[lo:hi]):
            blocks = b0 + np.flatnonzero(allowed[c, b0:b1])
            nodes = lo + np.flatnonzero(cls[lo:hi] == c)
            if not len(blocks):
                raise ValueError("class %d allows node %d no block of its type" % (c, nodes[0]))
            out[nodes] = blocks[np.arange(len(nodes)) % len(blocks)]
    empty = np.flatnonzero(np.bincount(out, minlength=ka + kb) == 0)
    if len(empty):
        raise ValueError("block %d ends up empty" % empty[0])
    return out


def load_fields(path, na, nb, ka, kb):
    """The fields file of ``mcmc --fields`` (include/bisbm_io.h): one line per node with a prior, its id and then block:weight
    pairs -> (class_of_node uint8 [n], field float64 [n_classes, ka + kb]) for BlockModel.set_fields; phi = -ln weight, class 0
    is the zero row and holds the unlisted nodes.  A node repeated with another row is an error.  ValueError, with the token
    named, for a malformed line."""
    L = lib()
    pc, pf = _u8p(), _f64p()
    err = C.create_string_buffer(512)
    n = int(na) + int(nb)
    count = L.bisbm_io_read_fields(os.fsencode(path), n, int(na), int(ka), int(kb), C.byref(pc), C.byref(pf), err, len(err))
    if count == -1:
        raise FileNotFoundError(path)
    if count < 0:
        raise ValueError(err.value.decode())
    K = int(ka) + int(kb)
    cls = np.ctypeslib.as_array(pc, shape=(max(n, 1),))[:n].copy()
    field = np.ctypeslib.as_array(pf, shape=(max(count * K, 1),))[:count * K].reshape(count, K).copy()
    L.bisbm_io_free(pc)
    L.bisbm_io_free(pf)
    return cls, field


def fields_from_weights(n, K, weights, na=None, ka=None):
    """(class_of_node uint8 [n], field float64 [n_classes, K]) from {node: {block: weight}}: the energy of a listed block is
    phi = -ln weight, an unlisted block has weight 1 (phi = 0), an unlisted node gets class 0, whose row is zero.  Every distinct
    row gets the next class -- at most 255 of them beside class 0, so that a class id is one byte; more is a ValueError.  A weight
    that is <= 0 or not finite is a ValueError (0 would forbid the block: that is what constraints are for).  With `na` and `ka`
    (the type-a nodes are 0 .. na-1, the type-a blocks 0 .. ka-1) a block of the other type is a ValueError; without them the
    row is taken as given (the engine ignores the other type's entries)."""
    import math
    n, K = int(n), int(K)
    cls = np.zeros(n, dtype=np.uint8)
    rows, index = [np.zeros(K, dtype=np.float64)], {}
    index[rows[0].tobytes()] = 0
    for v in sorted(weights):
        if not 0 <= int(v) < n:
            raise ValueError("node %r is not in [0, %d)" % (v, n))
        row = np.zeros(K, dtype=np.float64)
        for s, w in weights[v].items():
            s, w = int(s), float(w)
            if not 0 <= s < K:
                raise ValueError("node %r: block %d is not in [0, %d)" % (v, s, K))
            if na is not None and (s >= int(ka)) != (int(v) >= int(na)):
                raise ValueError("node %r: block %d is a block of the other type" % (v, s))
            if w == 0.0:
                raise ValueError("node %r, block %d: a weight of 0 forbids the block; use constraints (BlockModel.constrain) for that" % (v, s))
            if not (w > 0.0) or not math.isfinite(w):
                raise ValueError("node %r, block %d: weight %r is not finite and above 0" % (v, s, w))
            row[s] = 0.0 - math.log(w)
        key = row.tobytes()
        if key not in index:
            if len(rows) == 256:
                raise ValueError("more than 255 distinct rows beside class 0: a class id is one byte")
            index[key] = len(rows)
            rows.append(row)
        cls[int(v)] = index[key]
    return cls, np.array(rows)


def numpy_field_energy(labels, class_of_node, field, na, ka):
    """Phi of one label vector as bisbm_fields_energy defines it (include/bisbm.h, "Block fields", 7.), bit for bit: the integer
    histogram count[class][block] over the nodes, then the sum over (class ascending, block ascending, the own type's range of
    the nodes counted) of float(count) * phi, added sequentially from 0.0 with zero counts skipped."""
    labels = np.asarray(labels).astype(np.int64)
    cls = np.asarray(class_of_node).astype(np.int64)
    field = np.asarray(field, dtype=np.float64)
    n_classes, K = field.shape
    na, ka = int(na), int(ka)
    count = np.zeros((n_classes, K), dtype=np.int64)
    for v in range(len(labels)):
        b = int(labels[v])
        if (b >= ka) != (v >= na):
            raise ValueError("label %d of node %d is not a block of the node's type" % (b, v))
        count[cls[v], b] += 1
    phi = 0.0
    for c in range(n_classes):
        for b in range(K):
            if count[c, b]:
                phi = phi + float(count[c, b]) * float(field[c, b])
    return phi


def numpy_field_row(row, r_loc, f_own):
    """The heat-bath row under block fields (include/bisbm.h, "Block fields", 2.) from the model's row dS_s over the blocks of
    the node's type (BlockModel.conditionals_last), the node's block within its type and the entries of its class's field row
    over the same blocks: row[s] + (f[s] - f[r]) for s != r, and 0 at r.  Bit for bit the device's row."""
    row = np.asarray(row, dtype=np.float64)
    f = np.asarray(f_own, dtype=np.float64)
    r = int(r_loc)
    out = np.zeros(len(row), dtype=np.float64)
    for s in range(len(row)):
        if s != r:
            out[s] = float(row[s]) + (float(f[s]) - float(f[r]))
    return out


def edge_to_adj(edge_list, num_vertices):
    """graph_utilities.cc:36-49, as CSR (rowptr uint64[n+1], col uint32[2E]); rows keep file order."""
    L = lib()
    a = np.ascontiguousarray(edge_list[0], dtype=np.uint64)
    b = np.ascontiguousarray(edge_list[1], dtype=np.uint64)
    rowptr = np.zeros(num_vertices + 1, dtype=np.uint64)
    col = np.zeros(max(2 * len(a), 1), dtype=np.uint32)
    rc = L.bisbm_io_edges_to_csr(_p(a, _u64p), _p(b, _u64p), len(a), num_vertices, _p(rowptr, _u64p),
                                 _p(col, _u32p))
    if rc != 0:
        raise ValueError("edge list has a node id >= %d" % num_vertices)
    return rowptr, col[: 2 * len(a)]


def load_graph(path, num_vertices, cache=False):
    """load_edge_list + edge_to_adj (graph_utilities.cc:20-49) in one call -> (rowptr, col).  cache=True keeps a binary
    CSR beside the text file (`<path>.bisbm_csr`, validated against the file's size and mtime and rebuilt when they
    change); the text format stays the source of truth.  `load_graph.last_cache_hit` tells where the arrays came from."""
    L = lib()
    rp, cl = _u64p(), _u32p()
    ne, hit = C.c_uint64(), C.c_int()
    rc = L.bisbm_io_load_csr(os.fsencode(path), int(num_vertices), int(bool(cache)), C.byref(rp), C.byref(cl), C.byref(ne),
                             C.byref(hit))
    if rc == -1:
        raise FileNotFoundError(path)
    if rc != 0:
        raise ValueError("edge list has a node id >= %d" % num_vertices)
    rowptr = np.ctypeslib.as_array(rp, shape=(num_vertices + 1,)).copy()
    col = np.ctypeslib.as_array(cl, shape=(max(2 * ne.value, 1),))[: 2 * ne.value].copy()
    L.bisbm_io_free(rp)
    L.bisbm_io_free(cl)
    load_graph.last_cache_hit = bool(hit.value)
    return rowptr, col


class LocalityOrder:
    """A renumbering of the nodes (type a within [0, na), type b within [na, n)) made by :func:`locality_order`:
    ``new_id[v]`` is the id node v has in the renumbered graph."""

    def __init__(self, new_id):
        self.new_id = np.ascontiguousarray(new_id, dtype=np.uint32)
        if len(self.new_id) and (self.new_id.max() >= len(self.new_id) or len(np.unique(self.new_id)) != len(self.new_id)):
            raise ValueError("new_id is not a permutation")
        self.old_id = np.empty_like(self.new_id)
        self.old_id[self.new_id] = np.arange(len(self.new_id), dtype=np.uint32)

    def apply(self, rowptr, col):
        """CSR of the renumbered graph (rows keep their edge order)."""
        L = lib()
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        rp = np.zeros_like(rowptr)
        cl = np.zeros(max(len(col), 1), dtype=np.uint32)
        if L.bisbm_io_permute_csr(len(rowptr) - 1, _p(rowptr, _u64p), _p(col, _u32p), _p(self.new_id, _u32p), _p(rp, _u64p),
                                  _p(cl, _u32p)) != 0:
            raise ValueError("bad permutation")
        return rp, cl[: len(col)]

    def to_new(self, per_node):
        """a per-node vector in the caller's numbering -> the engine's (e.g. initial memberships)"""
        return np.asarray(per_node)[self.old_id]

    def to_old(self, per_node):
        """a per-node vector from the engine -> the caller's numbering (e.g. get_memberships())"""
        return np.asarray(per_node)[self.new_id]


def locality_order(rowptr, col, na, nb):
    """Ingest-time renumbering for graphs whose ids carry no structure (include/bisbm_io.h): returns a LocalityOrder."""
    L = lib()
    rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
    col = np.ascontiguousarray(col, dtype=np.uint32)
    n = int(na) + int(nb)
    new_id = np.zeros(n, dtype=np.uint32)
    if L.bisbm_io_locality_order(n, int(na), _p(rowptr, _u64p), _p(col, _u32p), _p(new_id, _u32p)) != 0:
        raise ValueError("bad graph")
    return LocalityOrder(new_id)


def output_vec(vec, stream=None):
    """output_functions.hh:20-29: elements separated by blanks, trailing blank, newline."""
    L = lib()
    v = np.ascontiguousarray(vec, dtype=np.uint32)
    size = L.bisbm_io_format_labels(_p(v, _u32p), len(v), None, 0)
    buf = C.create_string_buffer(size + 2)
    L.bisbm_io_format_labels(_p(v, _u32p), len(v), buf, size + 2)
    text = buf.raw[:size].decode()
    (stream or sys.stderr).write(text)
    return text


# --------------------------------------------------------------------------- blockmodel_t
class BlockModel:
    """Mirror of ``blockmodel_t`` (blockmodel.hh:13-153) for ``n_chains`` independent chains.

    ``BlockModel(memberships, types, g, KA, KB, epsilon, adj)`` follows the reference constructor
    (blockmodel.hh:22-23): ``types`` is the 0/1 vector with all type-a nodes first (only the two
    counts are used), ``g`` is accepted and ignored like in the reference, ``adj`` is the CSR pair
    returned by :func:`edge_to_adj`.  Keyword extras select the chain-parallel parts the reference
    does not have.
    """

    def __init__(self, memberships, types, g, KA, KB, epsilon, adj, *, n_chains=1, rng="philox", seed=0,
                 gen_seed=0, device=0, first_chain_id=0, devices=None):
        """``devices``: a list of HIP device ordinals -- the chains are spread over them as contiguous ranges behind ONE handle
        (``bisbm_create_multi``); every result equals what a single device with all the chains gives."""
        L = lib()
        self._L = L
        types = np.asarray(types)
        self.na = int((types == 0).sum())
        self.nb = int((types == 1).sum())
        if self.na + self.nb != len(types) or (self.na and self.nb and types[: self.na].any()):
            raise ValueError("types must be 0 for the first NA nodes and 1 for the remaining NB")
        self.n = self.na + self.nb
        self.KA, self.KB = int(KA), int(KB)
        self.K = self.KA + self.KB
        self.alignment = ALIGN_NONE  # marginals_set_alignment
        self.tempering_L = 0  # rungs of the replica-exchange ladder (set_tempering); 0: off
        self.mixed_shapes = False  # True once a one-argument agg_merge left the chains with different block counts
        self.epsilon = float(epsilon)
        self.n_chains = int(n_chains)
        self.device = int(device)
        rowptr = np.ascontiguousarray(adj[0], dtype=np.uint64)
        col = np.ascontiguousarray(adj[1], dtype=np.uint32)
        if len(rowptr) != self.n + 1:
            raise ValueError("adjacency has %d rows, types has %d nodes" % (len(rowptr) - 1, self.n))
        # A process that also uses torch.cuda (pooled marginals: a torch device tensor is handed to the library) must let
        # torch bring the device up first: its wheel carries its own HIP runtime, and the other order leaves torch
        # without a GPU.  Only done when the caller has imported torch already.
        _torch = sys.modules.get("torch")
        if _torch is not None:
            try:
                if _torch.cuda.is_available():
                    _torch.cuda.init()
            except Exception:
                pass
        h = C.c_void_p()
        self.devices = [int(d) for d in devices] if devices is not None else [int(device)]
        if devices is not None:
            self.device = self.devices[0]
            devs = (C.c_int * len(self.devices))(*self.devices)
            rc = L.bisbm_create_multi(C.byref(h), self.n, self.na, self.nb, _p(rowptr, _u64p), _p(col, _u32p), self.KA,
                                      self.KB, self.epsilon, self.n_chains, int(first_chain_id), devs, len(self.devices),
                                      _RNG[rng] if isinstance(rng, str) else int(rng), int(seed), int(gen_seed))
        else:
            rc = L.bisbm_create(C.byref(h), self.n, self.na, self.nb, _p(rowptr, _u64p), _p(col, _u32p), self.KA,
                                self.KB, self.epsilon, self.n_chains, int(first_chain_id), int(device),
                                _RNG[rng] if isinstance(rng, str) else int(rng), int(seed), int(gen_seed))
        if rc != BISBM_OK:
            raise BisbmError(rc, (L.bisbm_last_error(None) or b"").decode())
        self._h = h
        md, ne = C.c_uint32(), C.c_uint64()
        L.bisbm_get_sizes(h, None, C.byref(ne), C.byref(md), None)
        self.max_degree = md.value
        self.num_edges = ne.value
        self.set_memberships(memberships)

    # -- plumbing
    def _check(self, rc):
        if rc != BISBM_OK:
            raise BisbmError(rc, (self._L.bisbm_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.bisbm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        self._check(self._L.bisbm_set_stream(self._h, C.c_void_p(hip_stream)))

    # -- state
    def set_memberships(self, memberships, chain=ALL_CHAINS):
        mb = np.ascontiguousarray(memberships, dtype=np.uint32)
        if len(mb) != self.n:
            raise ValueError("memberships has %d entries, graph has %d nodes" % (len(mb), self.n))
        self._check(self._L.bisbm_set_memberships(self._h, int(chain), _p(mb, _u32p)))

    def init_bisbm(self):
        """blockmodel.cc:682-688"""
        self._check(self._L.bisbm_init(self._h))

    def shuffle_bisbm(self, engine=None, NA=None, NB=None):
        """blockmodel.cc:672-680 (the engine lives in the library; arguments kept for signature parity)"""
        self._check(self._L.bisbm_shuffle(self._h))

    # -- getters (blockmodel.cc:77-107)
    def get_memberships(self, chain=0):
        out = np.zeros(self.n, dtype=np.uint32)
        self._check(self._L.bisbm_get_memberships(self._h, int(chain), _p(out, _u32p)))
        return out

    def ka_kb(self, chain=0):
        """(KA, KB) of one chain: after a one-argument agg_merge the chains of a model may have different block counts."""
        ka, kb = C.c_uint32(), C.c_uint32()
        self._check(self._L.bisbm_get_ka_kb_chain(self._h, int(chain), C.byref(ka), C.byref(kb)))
        return ka.value, kb.value

    def _block_state(self, chain, want):
        K, D = sum(self.ka_kb(chain)), self.max_degree + 1
        m = np.zeros((K, K), dtype=np.int32) if "m" in want else None
        m_r = np.zeros(K, dtype=np.int32) if "m_r" in want else None
        n_r = np.zeros(K, dtype=np.int32) if "n_r" in want else None
        eta = np.zeros((K, D), dtype=np.uint32) if "eta" in want else None
        self._check(self._L.bisbm_get_block_state(
            self._h, int(chain), _p(m, _i32p) if m is not None else None,
            _p(m_r, _i32p) if m_r is not None else None, _p(n_r, _i32p) if n_r is not None else None,
            _p(eta, _u32p) if eta is not None else None))
        return m, m_r, n_r, eta

    def get_m(self, chain=0):
        return self._block_state(chain, ("m",))[0]

    def get_m_r(self, chain=0):
        return self._block_state(chain, ("m_r",))[1]

    def get_n_r(self, chain=0):
        return self._block_state(chain, ("n_r",))[2]

    def get_eta_rk_(self, chain=0):
        return self._block_state(chain, ("eta",))[3]

    def get_entropy(self):
        """Running sum of accepted dS per chain (blockmodel.cc:91)."""
        out = np.zeros(self.n_chains, dtype=np.float64)
        self._check(self._L.bisbm_get_cum_dS(self._h, _p(out, _f64p)))
        return out

    def entropy(self):
        """Full description length per chain (blockmodel.cc:753-787)."""
        out = np.zeros(self.n_chains, dtype=np.float64)
        self._check(self._L.bisbm_entropy(self._h, _p(out, _f64p)))
        return out

    def summary(self, stream=None):
        """blockmodel.cc:748-751"""
        s = stream or sys.stderr
        s.write("(Ka, Kb) = (%d, %d) \n" % (self.KA, self.KB))
        s.write("entropy: %s\n" % _fmt_g6(self.entropy()[0]))

    # -- agglomerative merges between anneals (blockmodel.cc:109-271)
    def _refresh_k(self):
        """KA / KB / K of the model: the counts all chains share, or -- once a one-argument agg_merge has left the chains
        with different ones (``mixed_shapes``) -- those of chain 0; ``ka_kb(chain)`` is always per chain."""
        ka, kb = C.c_uint32(), C.c_uint32()
        rc = self._L.bisbm_get_ka_kb(self._h, C.byref(ka), C.byref(kb))  # one call whatever the chain count:
        self.mixed_shapes = rc == BISBM_ERR_STATE                          # BISBM_ERR_STATE = the chains differ in shape
        if rc not in (BISBM_OK, BISBM_ERR_STATE):
            self._check(rc)
        self.KA, self.KB = self.ka_kb(0)
        self.K = self.KA + self.KB

    def agg_merge(self, diff_a, diff_b=None, nm=10):
        """``agg_merge(engine, diff_a, diff_b, nm)`` (blockmodel.cc:109-206) or, with ``diff_b=None``,
        ``agg_merge(engine, diff, nm)`` (:208-271), in every chain."""
        if diff_b is None:
            rc = self._L.bisbm_agg_merge_total(self._h, int(diff_a), int(nm))
        else:
            rc = self._L.bisbm_agg_merge(self._h, int(diff_a), int(diff_b), int(nm))
        self._check(rc)
        self._refresh_k()

    def get_KA(self):
        return self.KA

    def get_KB(self):
        return self.KB

    def get_num_edges(self):
        return self.num_edges

    def last_counts(self):
        acc = np.zeros(self.n_chains, dtype=np.uint64)
        sw = np.zeros(self.n_chains, dtype=np.uint64)
        self._check(self._L.bisbm_get_last_counts(self._h, _p(acc, _u64p), _p(sw, _u64p)))
        return acc, sw

    def last_sweep_timing(self):
        ms, upd = C.c_double(), C.c_uint64()
        self._check(self._L.bisbm_last_sweep_timing(self._h, C.byref(ms), C.byref(upd)))
        return ms.value, upd.value

    def last_pass_steps(self):
        """Steps per pass of the last sweep launch (1, 2, 4, 8): chosen per launch, never changes the chain."""
        k = C.c_uint32()
        self._check(self._L.bisbm_last_pass_steps(self._h, C.byref(k)))
        return k.value

    def last_route(self):
        """ROUTE_* bits of the last MH launch: ROUTE_PRODUCTION (the production kernel ran, not the generic one), ROUTE_HELD (it
        carried a clamp or constraints), ROUTE_FIELDS (it carried block fields); 0 before any launch.  Never changes the chain."""
        r = C.c_uint32()
        self._check(self._L.bisbm_last_sweep_route(self._h, C.byref(r)))
        return r.value

    def last_eta_plan(self):
        """(eta_in_lds, eta_w, eta_lo_a, eta_lo_b) of the last MH launch: all of eta in LDS, or the production kernel's window of
        eta_w degrees from eta_lo_a / eta_lo_b per type (rows of 1 to 255 entries inside it take the hot step); never changes the chain."""
        out = (C.c_uint32 * 4)()
        self._check(self._L.bisbm_last_eta_plan(self._h, out))
        return tuple(int(x) for x in out)

    # -- marginals (README.md:49-53)
    @property
    def kmax(self):
        return max(self.KA, self.KB)

    def run_sweeps(self, sweeps, temperature=1.0):
        """`sweeps` sweeps at constant temperature (the "marginalize" regime: -c constant -a 1)."""
        return MetropolisHasting().anneal(self, constant_schedule, [temperature], int(sweeps) * self.n, 1 << 60)

    # -- heat-bath sweeps and greedy polishing (include/bisbm.h, "Heat-bath sweeps and greedy polishing")
    def _heatbath(self, sweeps, beta, stop_when_settled):
        moved = np.zeros(self.n_chains, dtype=np.uint64)
        sw = np.zeros(self.n_chains, dtype=np.uint64)
        self._check(self._L.bisbm_heatbath_run(self._h, int(sweeps), float(beta), int(stop_when_settled), _p(moved, _u64p), _p(sw, _u64p)))
        return moved, sw

    def heatbath_sweeps(self, sweeps, beta=1.0):
        """`sweeps` heat-bath (Gibbs) sweeps: every node in the MH sweep's visit order draws its block from its exact
        conditional ~ exp(-beta dS).  Returns the moves per chain (uint64 [n_chains])."""
        return self._heatbath(sweeps, beta, False)[0]

    def polish(self, max_sweeps=100):
        """Greedy sweeps (beta = +inf: every free node to the lowest block of least dS, only strictly downhill) until a whole
        sweep moves nothing, at most `max_sweeps`.  Returns (moved, sweeps) per chain; a chain has settled -- it is a local
        minimum of the description length under single-node moves -- when its last sweep moved nothing, which
        sweeps < max_sweeps implies.  Under a clamp() the minimum is over the moves of the open nodes only."""
        return self._heatbath(max_sweeps, float("inf"), True)

    # -- pair reshuffles (include/bisbm.h, "Pair reshuffles")
    def reshuffle(self, moves, scans=3, beta=1.0):
        """`moves` pair reshuffles per chain: the nodes of two blocks of one type are divided afresh between the two by
        `scans` restricted Gibbs scans from a random launch state and one more that is the proposal, accepted or rejected as a
        whole, so exp(-beta S) stays exactly invariant.  The default of 3 scans is a convention from the literature (Jain and
        Neal's split-merge), not a measurement.  Returns the accepted moves per chain (uint64 [n_chains])."""
        acc = np.zeros(self.n_chains, dtype=np.uint64)
        self._check(self._L.bisbm_reshuffle_run(self._h, int(moves), int(scans), float(beta), _p(acc, _u64p)))
        return acc

    def reshuffle_last(self):
        """The last move of the last reshuffle() of every chain: a list of dicts with type (0: a, 1: b, RESHUFFLE_NONE: the
        shape has no pair), r, s (global labels), M, dS_fwd, dS_rev, q_fwd and q_rev as (mantissa, exponent), u_acc, A, accepted."""
        rec = (ReshuffleRecord * self.n_chains)()
        self._check(self._L.bisbm_reshuffle_get_last(self._h, rec))
        return [{"type": x.type, "r": x.r, "s": x.s, "M": x.M, "dS_fwd": x.dS_fwd, "dS_rev": x.dS_rev,
                 "q_fwd": (x.q_fwd_mant, x.q_fwd_exp), "q_rev": (x.q_rev_mant, x.q_rev_exp), "u_acc": x.u_acc, "A": x.A,
                 "accepted": bool(x.accepted)} for x in rec]

    def reshuffles_total(self):
        """Pair reshuffles proposed over every chain's lifetime (the index of the next move's Philox draws)."""
        out = np.zeros(self.n_chains, dtype=np.uint64)
        self._check(self._L.bisbm_reshuffle_get_total(self._h, _p(out, _u64p)))
        return out

    # -- split and merge moves (include/bisbm.h, "Split and merge moves")
    def split_merge(self, moves, scans=3, beta=1.0, k_min=(1, 1), k_max=None):
        """`moves` split or merge moves per chain: one block divided in two by `scans` restricted Gibbs scans from a random
        launch state and one more that is the proposal, or two blocks of one type made one, accepted or rejected as a whole, so
        that exp(-beta S) stays exactly invariant over the unlabelled partitions of every shape with k_min <= (Ka, Kb) <= k_max
        (k_max None: min(n_t, 127) per type).  An accepted move changes the chain's shape: the chains are kept grouped by shape
        (ka_kb(chain)), and traces, marginal histograms and every sum indexed by block labels must be reset by the caller, exactly
        as after agg_merge.  Returns the accepted moves per chain (uint64 [n_chains])."""
        acc = np.zeros(self.n_chains, dtype=np.uint64)
        lo = np.ascontiguousarray(k_min, dtype=np.uint32)
        hi = None if k_max is None else np.ascontiguousarray(k_max, dtype=np.uint32)
        if lo.shape != (2,) or (hi is not None and hi.shape != (2,)):
            raise ValueError("k_min and k_max are pairs (type a, type b)")
        self._check(self._L.bisbm_split_merge_run(self._h, int(moves), int(scans), float(beta), _p(lo, _u32p),
                                                  None if hi is None else _p(hi, _u32p), _p(acc, _u64p)))
        self._refresh_k()
        return acc

    def split_merge_last(self):
        """The last split or merge move of every chain: a list of dicts with kind (SM_SPLIT / SM_MERGE), type, r, s (global labels
        before the move; a split's s: the label the new block takes), M, refused (SM_EVALUATED, or why nothing was evaluated),
        q as (mantissa, exponent), dS, lnA, A, u_acc, accepted, before and after as (ka, kb)."""
        rec = (SplitMergeRecord * self.n_chains)()
        self._check(self._L.bisbm_split_merge_get_last(self._h, rec))
        return [{"kind": x.kind, "type": x.type, "r": x.r, "s": x.s, "M": x.M, "refused": x.refused, "q": (x.q_mant, x.q_exp),
                 "dS": x.dS, "lnA": x.lnA, "A": x.A, "u_acc": x.u_acc, "accepted": bool(x.accepted),
                 "before": (x.ka_before, x.kb_before), "after": (x.ka_after, x.kb_after)} for x in rec]

    def split_merge_total(self):
        """Per chain, over the handle's lifetime: uint64 [n_chains][4] -- splits proposed, splits accepted, merges proposed,
        merges accepted; a row's proposals add up to the index of the chain's next move's Philox draws."""
        out = np.zeros((self.n_chains, 4), dtype=np.uint64)
        self._check(self._L.bisbm_split_merge_get_total(self._h, _p(out, _u64p)))
        return out

    def chain_groups(self):
        """The shape group of its device entry that every chain lives in (uint32 [n_chains]; all 0 while an entry's chains are
        not grouped): chains of one device entry with the same shape share a group."""
        out = np.zeros(self.n_chains, dtype=np.uint32)
        self._check(self._L.bisbm_split_merge_get_groups(self._h, _p(out, _u32p)))
        return out

    def split_merge_timing(self):
        """(ms of the last split_merge() call by the host clock, ms of it spent forming the groups again) -- diagnostic"""
        a, b = np.zeros(1, dtype=np.float64), np.zeros(1, dtype=np.float64)
        self._check(self._L.bisbm_split_merge_get_timing(self._h, _p(a, _f64p), _p(b, _f64p)))
        return float(a[0]), float(b[0])

    def split_merge_shape_term(self, ka, kb):
        """T(ka, kb), the part of the description length that depends on the shape alone, as the library evaluates it."""
        out = np.zeros(1, dtype=np.float64)
        self._check(self._L.bisbm_split_merge_shape_term(self._h, int(ka), int(kb), _p(out, _f64p)))
        return float(out[0])

    # -- clamped nodes (include/bisbm.h, "Clamped nodes")
    def clamp(self, nodes_or_mask):
        """Holds nodes at the labels every chain has for them now: no sampler changes a clamped node's label, in any chain (MH
        sweeps, heat-bath sweeps and polish(), reshuffles, shuffle_bisbm(), the rounds of replica exchange and population
        annealing).  `nodes_or_mask`: an array of node ids, or a boolean / uint8 array of length n (non-zero: held).  A new call
        replaces the mask; an empty one is unclamp().  polish() then certifies a local minimum over the moves of the open
        nodes only.  While a clamp is set MH sweeps run the generic kernel (slower; README.md), and agg_merge is refused."""
        a = np.asarray(nodes_or_mask)
        if a.dtype == np.bool_ or (a.dtype == np.uint8 and a.ndim == 1 and len(a) == self.n):
            if a.shape != (self.n,):
                raise ValueError("a clamp mask has one entry per node (%d), not %s" % (self.n, a.shape))
            mask = np.ascontiguousarray(a != 0, dtype=np.uint8)
        else:
            if a.size and (a.dtype.kind not in "iu" or a.min() < 0 or a.max() >= self.n):
                raise ValueError("clamped node ids must be integers in [0, %d)" % self.n)
            mask = np.zeros(self.n, dtype=np.uint8)
            mask[a.astype(np.int64).ravel()] = 1
        self._check(self._L.bisbm_clamp_set(self._h, _p(mask, _u8p)))

    def unclamp(self):
        """Clears the clamp: from here on every call is bit for bit what a model that never had one does."""
        self._check(self._L.bisbm_clamp_set(self._h, None))

    def clamped(self):
        """The clamp as a bool mask of length n (all False: none)."""
        mask = np.zeros(self.n, dtype=np.uint8)
        self._check(self._L.bisbm_clamp_get(self._h, _p(mask, _u8p), None))
        return mask.astype(bool)

    # -- block constraints (include/bisbm.h, "Block constraints")
    def constrain(self, class_of_node, allowed):
        """Restricts every node to the blocks its class allows, in every chain and through every sampler: `class_of_node` is
        an array of n class ids (at most 256 classes), `allowed` a [n_classes, KA + KB] table, non-zero meaning allowed (the
        entries for blocks of the other type are ignored).  Every chain's current labels must be admissible
        (admissible_start gives such a start); a new call replaces the constraints, and a table that allows every node every
        block of its type is unconstrain().  May be combined with clamp().  While constraints are set MH sweeps run the
        generic kernel (slower; README.md), polish() certifies a minimum over the admissible moves, and agg_merge is refused."""
        cls = np.asarray(class_of_node)
        table = np.asarray(allowed)
        if cls.shape != (self.n,) or cls.dtype.kind not in "iub":
            raise ValueError("class_of_node has one integer per node (%d), not %s %s" % (self.n, cls.dtype, cls.shape))
        if table.ndim != 2 or table.shape[1] != self.K or not 1 <= table.shape[0] <= 256:
            raise ValueError("allowed is a [n_classes <= 256, %d] table, not %s" % (self.K, table.shape))
        if cls.size and (cls.min() < 0 or cls.max() >= table.shape[0]):
            raise ValueError("class ids must be in [0, %d)" % table.shape[0])
        cls8 = np.ascontiguousarray(cls, dtype=np.uint8)
        tab8 = np.ascontiguousarray(table != 0, dtype=np.uint8)
        self._check(self._L.bisbm_constraints_set(self._h, int(table.shape[0]), _p(cls8, _u8p), _p(tab8, _u8p)))

    def unconstrain(self):
        """Clears the constraints: from here on every call is bit for bit what a model that never had any does."""
        self._check(self._L.bisbm_constraints_set(self._h, 0, None, None))

    def constraints(self):
        """(class_of_node uint8 [n], allowed bool [n_classes, KA + KB]) as set; without constraints (None, None)."""
        k = np.zeros(1, dtype=np.uint32)
        self._check(self._L.bisbm_constraints_get(self._h, _p(k, _u32p), None, None))
        if not int(k[0]):
            return None, None
        cls = np.zeros(self.n, dtype=np.uint8)
        table = np.zeros((int(k[0]), self.K), dtype=np.uint8)
        self._check(self._L.bisbm_constraints_get(self._h, None, _p(cls, _u8p), _p(table, _u8p)))
        return cls, table.astype(bool)

    # -- block fields (include/bisbm.h, "Block fields")
    def set_fields(self, class_of_node, field):
        """Gives every node a soft prior over blocks, in every chain and through every sampler: `class_of_node` is an array of n
        class ids (at most 256 classes), `field` a [n_classes, KA + KB] table of finite energies phi in nats (the entries for
        blocks of the other type are ignored).  With Phi = the sum of phi[class(v)][b_v] over the nodes every sampler targets
        exp(-beta (S + Phi)): a node's prior weight for block s is exp(-phi_s) (fields_from_weights builds the pair from
        weights).  A new call replaces the fields, a table of zeros is clear_fields().  Independent of clamp() and constrain().
        While fields are set MH sweeps run the production kernel's fielded instances, one step per pass (README.md), get_entropy() advances by dS + dPhi, polish()
        certifies a minimum of S + Phi, replica exchange and population annealing weigh S + Phi, and agg_merge is refused;
        entropy() stays the description length."""
        cls = np.asarray(class_of_node)
        table = np.asarray(field, dtype=np.float64)
        if cls.shape != (self.n,) or cls.dtype.kind not in "iub":
            raise ValueError("class_of_node has one integer per node (%d), not %s %s" % (self.n, cls.dtype, cls.shape))
        if table.ndim != 2 or table.shape[1] != self.K or not 1 <= table.shape[0] <= 256:
            raise ValueError("field is a [n_classes <= 256, %d] table, not %s" % (self.K, table.shape))
        if cls.size and (cls.min() < 0 or cls.max() >= table.shape[0]):
            raise ValueError("class ids must be in [0, %d)" % table.shape[0])
        cls8 = np.ascontiguousarray(cls, dtype=np.uint8)
        tab = np.ascontiguousarray(table, dtype=np.float64)
        self._check(self._L.bisbm_fields_set(self._h, int(table.shape[0]), _p(cls8, _u8p), _p(tab, _f64p)))

    def clear_fields(self):
        """Clears the fields: from here on every call is bit for bit what a model that never had any does."""
        self._check(self._L.bisbm_fields_set(self._h, 0, None, None))

    def fields(self):
        """(class_of_node uint8 [n], field float64 [n_classes, KA + KB]) as set; without fields (None, None)."""
        k = np.zeros(1, dtype=np.uint32)
        self._check(self._L.bisbm_fields_get(self._h, _p(k, _u32p), None, None))
        if not int(k[0]):
            return None, None
        cls = np.zeros(self.n, dtype=np.uint8)
        table = np.zeros((int(k[0]), self.K), dtype=np.float64)
        self._check(self._L.bisbm_fields_get(self._h, None, _p(cls, _u8p), _p(table, _f64p)))
        return cls, table

    def field_energy(self):
        """Phi per chain (bisbm_fields_energy; numpy_field_energy is its host statement); zeros without fields."""
        out = np.zeros(self.n_chains, dtype=np.float64)
        self._check(self._L.bisbm_fields_energy(self._h, _p(out, _f64p)))
        return out

    def debug_exp(self, x):
        """exp(x) as the device evaluates it (the host replays of the pair reshuffles take their exponentials from here)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros(len(x), dtype=np.float64)
        self._check(self._L.bisbm_debug_exp(self._h, _p(x, _f64p), len(x), _p(out, _f64p)))
        return out

    def debug_log(self, x):
        """log(x) as the device evaluates it (the entropy term of numpy_held_conditional_row on the device's bits)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros(len(x), dtype=np.float64)
        self._check(self._L.bisbm_debug_log(self._h, _p(x, _f64p), len(x), _p(out, _f64p)))
        return out

    # -- replica exchange (include/bisbm.h, "Replica exchange")
    def set_tempering(self, ladder):
        """Replica exchange over ensembles of L = len(ladder) consecutive chains (chain g L + i starts on rung i); ``None`` or
        an empty ladder turns it off.  The ladder is checked here first (validate_ladder), the chain count too."""
        if ladder is None or len(ladder) == 0:
            self._check(self._L.bisbm_tempering_set(self._h, 0, None))
            self.tempering_L = 0
            return
        lad = validate_ladder(ladder)
        if self.n_chains % len(lad):
            raise ValueError("%d chains are not a multiple of the ladder's %d rungs" % (self.n_chains, len(lad)))
        self._check(self._L.bisbm_tempering_set(self._h, len(lad), _p(lad, _f32p)))
        self.tempering_L = len(lad)

    def tempering_run(self, sweeps, exchange_every=1):
        """`sweeps` sweeps of every chain at its rung's temperature, an exchange round after every complete block of
        `exchange_every` sweeps (0: none).  Returns the acceptance rate per chain (a float for one chain)."""
        rates = np.zeros(self.n_chains, dtype=np.float64)
        self._check(self._L.bisbm_tempering_run(self._h, int(sweeps), int(exchange_every), _p(rates, _f64p)))
        return float(rates[0]) if self.n_chains == 1 else rates

    def tempering_state(self):
        """(rung uint32 [n_chains], temperature float32 [n_chains]) of every chain."""
        rung = np.zeros(self.n_chains, dtype=np.uint32)
        T = np.zeros(self.n_chains, dtype=np.float32)
        self._check(self._L.bisbm_tempering_get(self._h, _p(rung, _u32p), _p(T, _f32p)))
        return rung, T

    def tempering_stats(self):
        """(attempted uint64 [L - 1], accepted uint64 [L - 1], rounds): exchanges per rung pair (i, i + 1) since set_tempering."""
        P = max(self.tempering_L - 1, 1)
        att = np.zeros(P, dtype=np.uint64)
        acc = np.zeros(P, dtype=np.uint64)
        rounds = C.c_uint64()
        self._check(self._L.bisbm_tempering_stats(self._h, _p(att, _u64p), _p(acc, _u64p), C.byref(rounds)))
        return att, acc, rounds.value

    def tempering_rounds(self, rounds, mh=1, heatbath=0, reshuffles=0, scans=3, exchange=True):
        """`rounds` rounds of replica exchange with mixed moves: per round `mh` MH sweeps of every chain at its rung's
        temperature T_c, then `heatbath` heat-bath sweeps and `reshuffles` pair reshuffles (`scans` launch scans each) at
        beta_c = 1 / T_c, then one exchange round (exchange=False: none).  tempering_rung_stats() reports what each move did
        on every rung."""
        rec = round_recipe(mh, heatbath, reshuffles, scans)
        if int(rounds) < 0:
            raise ValueError("rounds must not be negative")
        self._check(self._L.bisbm_tempering_run_rounds(self._h, int(rounds), C.byref(rec), 1 if exchange else 0))

    def tempering_rung_stats(self):
        """Per rung since set_tempering, uint64 [L] each: {"mh_steps", "mh_accepted", "heatbath_steps", "heatbath_moves",
        "reshuffles", "reshuffles_accepted"} -- what the chains did while they held the rung."""
        out = np.zeros(6 * max(self.tempering_L, 1), dtype=np.uint64)
        self._check(self._L.bisbm_tempering_rung_stats(self._h, _p(out, _u64p)))
        out = out.reshape(-1, 6)
        return {name: out[:, i].copy() for i, name in enumerate(RUNG_STAT_COLUMNS)}

    # -- population annealing (include/bisbm.h, "Population annealing")
    def population_resample(self, beta_from, beta_to):
        """One resampling step of all chains from inverse temperature beta_from to beta_to >= beta_from: every dead slot takes
        its parent's state.  Returns (parent uint32 [n_chains], the step's estimate of ln Z(beta_to) / Z(beta_from))."""
        parent = np.zeros(self.n_chains, dtype=np.uint32)
        lr = C.c_double()
        self._check(self._L.bisbm_population_resample(self._h, float(beta_from), float(beta_to), _p(parent, _u32p), C.byref(lr)))
        return parent, lr.value

    def population_run(self, temps, sweeps_per_step):
        """For every temperature after the first: a resampling step from the one before, then `sweeps_per_step` sweeps of every
        chain at it.  The caller has equilibrated the chains at temps[0].  Returns {"log_ratio" f64 [steps], "distinct" uint32
        [steps] (distinct ancestors after every step), "rates" f64 [n_chains]}."""
        T = validate_population_temps(temps)
        lr = np.zeros(len(T) - 1, dtype=np.float64)
        distinct = np.zeros(len(T) - 1, dtype=np.uint32)
        rates = np.zeros(self.n_chains, dtype=np.float64)
        self._check(self._L.bisbm_population_run(self._h, len(T), _p(T, _f32p), int(sweeps_per_step), _p(lr, _f64p),
                                                 _p(distinct, _u32p), _p(rates, _f64p)))
        return {"log_ratio": lr, "distinct": distinct, "rates": rates}

    def population_rounds(self, temps, rounds_per_step, mh=1, heatbath=0, reshuffles=0, scans=3):
        """population_run with, after every resampling step, `rounds_per_step` rounds of `mh` MH sweeps, `heatbath` heat-bath
        sweeps and `reshuffles` pair reshuffles at the step's temperature.  Returns the dict of population_run (rates: of the
        MH steps)."""
        T = validate_population_temps(temps)
        rec = round_recipe(mh, heatbath, reshuffles, scans)
        if int(rounds_per_step) < 0:
            raise ValueError("rounds_per_step must not be negative")
        lr = np.zeros(len(T) - 1, dtype=np.float64)
        distinct = np.zeros(len(T) - 1, dtype=np.uint32)
        rates = np.zeros(self.n_chains, dtype=np.float64)
        self._check(self._L.bisbm_rounds_population_run(self._h, len(T), _p(T, _f32p), int(rounds_per_step), C.byref(rec), _p(lr, _f64p),
                                                        _p(distinct, _u32p), _p(rates, _f64p)))
        return {"log_ratio": lr, "distinct": distinct, "rates": rates}

    def population_state(self):
        """{"ancestor" uint32 [n_chains], "rounds", "log_ratio_total"} since the last population_reset."""
        anc = np.zeros(self.n_chains, dtype=np.uint32)
        rounds, tot = C.c_uint64(), C.c_double()
        self._check(self._L.bisbm_population_get(self._h, _p(anc, _u32p), C.byref(rounds), C.byref(tot)))
        return {"ancestor": anc, "rounds": rounds.value, "log_ratio_total": tot.value}

    def population_reset(self):
        self._check(self._L.bisbm_population_reset(self._h))

    def counts_device(self):
        """torch device a caller-owned marginal histogram must live on."""
        import torch
        return torch.device("cuda", self.device)

    def marginals_reset(self):
        self._check(self._L.bisbm_marginals_reset(self._h))

    def marginals_accumulate(self, device_ptr=None):
        """One sample of every chain's labels into the internal histogram (device_ptr None) or ADDED to the caller's
        device buffer of n * kmax uint32 / int32 at `device_ptr` (e.g. torch_tensor.data_ptr())."""
        self._check(self._L.bisbm_marginals_accumulate(self._h, C.c_void_p(device_ptr) if device_ptr else None))

    def marginals_get(self, mode=None):
        """The internal histogram [n, kmax]; with `mode` the histogram of that mode (marginals_set_modes)."""
        out = np.zeros((self.n, self.kmax), dtype=np.uint32)
        if mode is None:
            self._check(self._L.bisbm_marginals_get(self._h, _p(out, _u32p)))
        else:
            self._check(self._L.bisbm_marginals_get_mode(self._h, int(mode), _p(out, _u32p)))
        return out

    # -- mode-resolved marginals (include/bisbm.h, "Mode-resolved marginals")
    def marginals_set_modes(self, mode_of_chain=None, n_modes=None):
        """One aligned histogram per posterior mode.  `mode_of_chain`: per chain its mode 0 .. M-1 or MODE_NONE (not counted);
        or the dict partition_modes() returns (chains outside its selection become MODE_NONE); None turns the feature off.
        `n_modes`: M (default: the highest mode + 1).  Refused while the histogram holds samples (marginals_reset first)."""
        if mode_of_chain is None:
            self._check(self._L.bisbm_marginals_set_modes(self._h, 0, None))
            return
        moc, n_modes = mode_assignment(mode_of_chain, self.n_chains, n_modes)
        self._check(self._L.bisbm_marginals_set_modes(self._h, n_modes, _p(moc, _u32p)))

    def marginals_set_mode_anchors(self, anchors, threshold):
        """Anchored modes (include/bisbm.h, "Anchored modes"): one histogram per row of `anchors` [M, n]; at every sample each
        counted chain goes into the mode of its nearest anchor (VI, ties -> the lowest mode) if that VI is <= `threshold`
        (float('inf'): always).  Allowed with replica exchange on.  None or an empty array turns the feature off."""
        if anchors is None or np.size(anchors) == 0:
            self._check(self._L.bisbm_marginals_set_mode_anchors(self._h, 0, None, 0.0))
            return
        a = np.ascontiguousarray(np.atleast_2d(anchors), dtype=np.uint32)
        if a.ndim != 2 or a.shape[1] != self.n:
            raise ValueError("anchors must have shape (n_modes, %d), got %s" % (self.n, a.shape))
        self._check(self._L.bisbm_marginals_set_mode_anchors(self._h, a.shape[0], _p(a, _u32p), float(threshold)))

    def marginals_mode_assignment(self):
        """Anchored modes, as a dict: `vi` float64 [n_chains, M] of the last sample (NaN rows: chains that were not counted),
        `visits` uint64 [n_chains, M] (samples of chain c counted into mode g), `unassigned` (counted chains beyond the
        threshold, over all samples), `samples`."""
        nm = C.c_uint32()
        self._check(self._L.bisbm_marginals_get_modes(self._h, C.byref(nm), None, None, None))
        M = max(nm.value, 1)
        vi = np.zeros((self.n_chains, M), dtype=np.float64)
        visits = np.zeros((self.n_chains, M), dtype=np.uint64)
        un, sm = C.c_uint64(), C.c_uint64()
        self._check(self._L.bisbm_marginals_get_mode_assignment(self._h, _p(vi, _f64p), _p(visits, _u64p), C.byref(un), C.byref(sm)))
        return {"vi": vi, "visits": visits, "unassigned": un.value, "samples": sm.value}

    def _anchored_unassigned(self):
        """`unassigned` while anchors are set, None otherwise."""
        un = C.c_uint64()
        if self._L.bisbm_marginals_get_mode_assignment(self._h, None, None, C.byref(un), None) != BISBM_OK:
            return None
        return un.value

    def marginals_modes(self):
        """What marginals_set_modes set and what the samples made of it, as a dict: `n_modes`, `mode_of_chain` uint32
        [n_chains], `ref_chain` int64 [M] (-1: the caller's reference, -2: none yet), `terms` uint64 [M] (chain samples in
        every mode's histogram), `weights` [M] (each mode's share of the counted chains).  n_modes = 0: the feature is off.
        While anchors are set (marginals_set_mode_anchors): `mode_of_chain` is the last sample's assignment, there is
        `unassigned` as well, and `weights` are the sample shares terms / (sum of terms + unassigned)."""
        nm = C.c_uint32()
        self._check(self._L.bisbm_marginals_get_modes(self._h, C.byref(nm), None, None, None))
        M = nm.value
        moc = np.full(self.n_chains, MODE_NONE, dtype=np.uint32)
        ref = np.zeros(max(M, 1), dtype=np.int64)
        terms = np.zeros(max(M, 1), dtype=np.uint64)
        self._check(self._L.bisbm_marginals_get_modes(self._h, C.byref(nm), _p(moc, _u32p), _p(ref, C.POINTER(C.c_int64)), _p(terms, _u64p)))
        un = self._anchored_unassigned() if M else None
        if un is not None:
            t = terms[:M].astype(np.float64)
            return {"n_modes": M, "mode_of_chain": moc, "ref_chain": ref[:M], "terms": terms[:M], "unassigned": un,
                    "weights": t / max(float(t.sum()) + un, 1.0)}
        size = np.bincount(moc[moc != MODE_NONE].astype(np.int64), minlength=M)[:M]
        return {"n_modes": M, "mode_of_chain": moc, "ref_chain": ref[:M], "terms": terms[:M],
                "weights": size / max(int(size.sum()), 1)}

    def marginals_set_alignment(self, mode):
        """ALIGN_REFERENCE (or True): every chain's labels are counted through its permutation onto the reference partition
        (include/bisbm.h, "Label alignment before pooling"); ALIGN_NONE (False, the default): raw labels.  Holds across resets;
        refused while the internal histogram holds samples of the other mode."""
        self._check(self._L.bisbm_marginals_set_alignment(self._h, int(mode)))
        self.alignment = int(mode)

    def marginals_set_reference(self, labels=None, mode=None):
        """n labels of the present block counts as the reference of the alignment; None: the lowest-description-length chain,
        taken at the next aligned sample.  With `mode`: the reference of that mode (marginals_set_modes)."""
        def call(ptr):
            if mode is None:
                return self._L.bisbm_marginals_set_reference(self._h, ptr)
            return self._L.bisbm_marginals_set_mode_reference(self._h, int(mode), ptr)
        if labels is None:
            self._check(call(None))
            return
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        if len(lab) != self.n:
            raise ValueError("reference has %d labels, graph has %d nodes" % (len(lab), self.n))
        self._check(call(_p(lab, _u32p)))

    def marginals_reference(self, mode=None):
        """(labels uint32 [n], chain): the reference of the alignment and the chain it came from (-1: set by the caller).  With
        `mode`: the reference of that mode."""
        out = np.zeros(self.n, dtype=np.uint32)
        chain = C.c_int64()
        if mode is None:
            self._check(self._L.bisbm_marginals_get_reference(self._h, _p(out, _u32p), C.byref(chain)))
        else:
            self._check(self._L.bisbm_marginals_get_mode_reference(self._h, int(mode), _p(out, _u32p), C.byref(chain)))
        return out, chain.value

    def marginals_alignment(self, chain):
        """(perm uint32 [KA + KB], overlap): chain's permutation of the last aligned sample in global-label form (label r was
        counted as perm[r]) and its overlap with the reference."""
        ka, kb = self.ka_kb(chain)
        perm = np.zeros(ka + kb, dtype=np.uint32)
        tot = C.c_uint64()
        self._check(self._L.bisbm_marginals_get_alignment(self._h, int(chain), _p(perm, _u32p), C.byref(tot)))
        return perm, tot.value

    def marginals_map(self, mode=None, return_top=False):
        """MAP block of every node from the internal histogram (most frequent block, ties -> the lowest), pooled over the
        handle's devices on the devices (``bisbm_marginals_map``: reduce-scatter -> argmax -> all-gather).  With `mode`: the
        MAP of that mode's histogram in the numbering of the mode's reference, and with `return_top` also every node's winning
        count (labels, top): top / terms of the mode says how settled the node is within it."""
        out = np.zeros(self.n, dtype=np.uint32)
        if mode is None:
            if return_top:
                raise ValueError("return_top needs a mode (marginals_set_modes)")
            self._check(self._L.bisbm_marginals_map(self._h, _p(out, _u32p)))
            return out
        top = np.zeros(self.n, dtype=np.uint32)
        self._check(self._L.bisbm_marginals_map_mode(self._h, int(mode), _p(out, _u32p), _p(top, _u32p)))
        return (out, top) if return_top else out

    # -- pair scores (include/bisbm.h, "Posterior-predictive pair scores")
    def pair_scores_set(self, pairs):
        """The pairs to score: an integer array [P, 2] of (type-a node, type-b node); replaces earlier pairs and zeroes the
        sums.  An empty array frees everything."""
        pr = np.asarray(pairs)
        if pr.size == 0:
            pr = np.zeros((0, 2), dtype=np.uint32)
        if pr.ndim != 2 or pr.shape[1] != 2 or not np.issubdtype(pr.dtype, np.integer):
            raise ValueError("pairs must be an integer array of shape (P, 2)")
        if len(pr) and (pr.min() < 0 or pr.max() > 0xFFFFFFFF):
            raise ValueError("a node id of a pair is outside [0, 2^32)")
        u = np.ascontiguousarray(pr[:, 0], dtype=np.uint32)
        v = np.ascontiguousarray(pr[:, 1], dtype=np.uint32)
        self._check(self._L.bisbm_pair_scores_set(self._h, len(u), _p(u, _u32p), _p(v, _u32p)))
        self.n_pairs = len(u)

    def pair_scores_accumulate(self):
        """One sample: every counted chain's term lambda(u, v) is added to every pair's sum (with replica exchange on, the
        chains on rung 0 only)."""
        self._check(self._L.bisbm_pair_scores_accumulate(self._h))

    def pair_scores_reset(self):
        self._check(self._L.bisbm_pair_scores_reset(self._h))

    def pair_scores(self):
        """(sum float64 [P] in the order of pair_scores_set, terms): the estimate of a pair's expected edge count is
        sum / terms."""
        out = np.zeros(getattr(self, "n_pairs", 0), dtype=np.float64)
        terms = C.c_uint64()
        self._check(self._L.bisbm_pair_scores_get(self._h, _p(out, _f64p), C.byref(terms)))
        return out, terms.value

    # -- edge probabilities (include/bisbm.h, "Edge probabilities")
    def edge_probs_set(self, pairs, kinds=None, keep_last=False):
        """The edges to weigh: an integer array [P, 2] of (type-a node, type-b node) and per pair EDGE_ADD (0; also "+") or
        EDGE_REMOVE (1; "-"), None: all ADD; replaces earlier pairs and zeroes the sums.  keep_last: keep every chain's dS of the
        last sample for edge_probs_last (n_chains x P doubles on the device).  An empty array frees everything."""
        pr = np.asarray(pairs)
        if pr.size == 0:
            pr = np.zeros((0, 2), dtype=np.uint32)
        if pr.ndim != 2 or pr.shape[1] != 2 or not np.issubdtype(pr.dtype, np.integer):
            raise ValueError("pairs must be an integer array of shape (P, 2)")
        if len(pr) and (pr.min() < 0 or pr.max() > 0xFFFFFFFF):
            raise ValueError("a node id of a pair is outside [0, 2^32)")
        u = np.ascontiguousarray(pr[:, 0], dtype=np.uint32)
        v = np.ascontiguousarray(pr[:, 1], dtype=np.uint32)
        kd = None
        if kinds is not None:
            kd = np.array([{"+": EDGE_ADD, "-": EDGE_REMOVE}.get(k, k) for k in kinds] if len(kinds) else [], dtype=np.int64)
            if kd.shape != (len(u),) or (len(kd) and (kd.min() < 0 or kd.max() > 255)):
                raise ValueError("kinds must hold one of EDGE_ADD / EDGE_REMOVE per pair")
            kd = np.ascontiguousarray(kd, dtype=np.uint8)
        self._check(self._L.bisbm_edge_probs_set(self._h, len(u), _p(u, _u32p), _p(v, _u32p), _p(kd, _u8p) if kd is not None else None,
                                                 EDGE_KEEP_LAST if keep_last else 0))
        self.n_edge_pairs = len(u)

    def edge_probs_accumulate(self):
        """One sample: every counted chain's dS and exp(-dS) are added to every pair's sums (with replica exchange on, the
        chains on rung 0 only)."""
        self._check(self._L.bisbm_edge_probs_accumulate(self._h))

    def edge_probs_reset(self):
        self._check(self._L.bisbm_edge_probs_reset(self._h))

    def edge_probs(self):
        """A dict, arrays [P] in the order of edge_probs_set: dS_sum, w_sum (float64), mult (uint32: the present multiplicity),
        terms, and the estimates mean_dS = dS_sum / terms and log_prob = ln(w_sum / terms), the log posterior-predictive odds of
        the edited graph (NaN before the first sample, -inf where every counted chain's exp(-dS) is 0)."""
        P = getattr(self, "n_edge_pairs", 0)
        ds, w, mult = np.zeros(P, dtype=np.float64), np.zeros(P, dtype=np.float64), np.zeros(P, dtype=np.uint32)
        terms = C.c_uint64()
        self._check(self._L.bisbm_edge_probs_get(self._h, _p(ds, _f64p), _p(w, _f64p), _p(mult, _u32p), C.byref(terms)))
        if not terms.value:
            mean = logp = np.full(P, np.nan)
        else:  # (math.log: the C library's logarithm, the one the command line prints)
            import math
            t = float(terms.value)
            mean = ds / t
            logp = np.array([math.log(x) if x > 0 else (-math.inf if x == 0 else math.nan) for x in (w / t).tolist()], dtype=np.float64)
        return {"dS_sum": ds, "w_sum": w, "mult": mult, "terms": terms.value, "mean_dS": mean, "log_prob": logp}

    def edge_probs_last(self, i):
        """float64 [n_chains]: dS of pair i (in the order of edge_probs_set) in every chain at the last sample, NaN where the
        chain was not counted; needs keep_last."""
        out = np.zeros(self.n_chains, dtype=np.float64)
        self._check(self._L.bisbm_edge_probs_get_last(self._h, int(i), _p(out, _f64p)))
        return out

    # -- query scores (include/bisbm.h, "Query scores")
    def query_scores_set(self, queries):
        """The nodes to rank candidates for: an integer array [Q] of node ids of either type (they may repeat); replaces earlier
        queries and zeroes the sums.  Every query gets a row of one f64 per node of the other type on the device.  An empty
        array frees everything."""
        q = np.asarray(queries)
        if q.size == 0:
            q = np.zeros(0, dtype=np.uint32)
        if q.ndim != 1 or not np.issubdtype(q.dtype, np.integer):
            raise ValueError("queries must be a one-dimensional integer array")
        if len(q) and (q.min() < 0 or q.max() > 0xFFFFFFFF):
            raise ValueError("a query is outside [0, 2^32)")
        q = np.ascontiguousarray(q, dtype=np.uint32)
        self._check(self._L.bisbm_query_scores_set(self._h, len(q), _p(q, _u32p)))
        self.queries = q.copy()

    def query_scores_accumulate(self):
        """One sample: every counted chain's term is added to the sum of every (query, candidate), chain by chain in ascending
        order (with replica exchange on, the chains on rung 0 only)."""
        self._check(self._L.bisbm_query_scores_accumulate(self._h))

    def query_scores_reset(self):
        self._check(self._L.bisbm_query_scores_reset(self._h))

    def query_scores(self, i):
        """(row float64 [n_other], terms) of the i-th query: the sums of its candidates in id order (candidate j of a type-a
        query is node na + j, of a type-b query node j)."""
        queries = getattr(self, "queries", np.zeros(0, dtype=np.uint32))
        i = int(i)
        if not 0 <= i < len(queries):
            raise IndexError("query index %d: %d queries are set" % (i, len(queries)))
        out = np.zeros(self.n - self.na if queries[i] < self.na else self.na, dtype=np.float64)
        terms = C.c_uint64()
        self._check(self._L.bisbm_query_scores_get_row(self._h, i, _p(out, _f64p), C.byref(terms)))
        return out, terms.value

    def query_topk(self, k, exclude_edges=True):
        """(nodes uint32 [Q, k], sums float64 [Q, k], terms): every query's k best candidates by pooled sum, descending, ties to
        the lowest node id, selected on the device.  exclude_edges: the query's neighbours are not eligible.  Entries past the
        eligible candidates are 0xffffffff / 0.0."""
        Q = len(getattr(self, "queries", ()))
        nodes = np.zeros((Q, int(k)), dtype=np.uint32)
        sums = np.zeros((Q, int(k)), dtype=np.float64)
        terms = C.c_uint64()
        self._check(self._L.bisbm_query_scores_topk(self._h, int(k), 1 if exclude_edges else 0, _p(nodes, _u32p), _p(sums, _f64p), C.byref(terms)))
        return nodes, sums, terms.value

    def recommend(self, k, exclude_edges=True):
        """(nodes uint32 [Q, k], scores float64 [Q, k], terms): query_topk with scores = sum / terms, the estimate of the expected
        number of edges between the query and the node."""
        nodes, sums, terms = self.query_topk(k, exclude_edges)
        return nodes, sums / terms, terms

    # -- edge queries (include/bisbm.h, "Edge queries")
    def edge_queries_set(self, queries):
        """The nodes whose candidate edges are weighed: an integer array [Q] of node ids of either type (they may repeat);
        replaces earlier queries and zeroes the sums.  Every query gets a row of one f64 per node of the other type on the
        device.  An empty array frees everything."""
        q = np.asarray(queries)
        if q.size == 0:
            q = np.zeros(0, dtype=np.uint32)
        if q.ndim != 1 or not np.issubdtype(q.dtype, np.integer):
            raise ValueError("queries must be a one-dimensional integer array")
        if len(q) and (q.min() < 0 or q.max() > 0xFFFFFFFF):
            raise ValueError("a query is outside [0, 2^32)")
        q = np.ascontiguousarray(q, dtype=np.uint32)
        self._check(self._L.bisbm_edge_queries_set(self._h, len(q), _p(q, _u32p)))
        self.edge_query_nodes = q.copy()

    def edge_queries_accumulate(self):
        """One sample: every counted chain's exp(-dS) of adding the edge is added to the sum of every (query, candidate), chain
        by chain in ascending order (with replica exchange on, the chains on rung 0 only)."""
        self._check(self._L.bisbm_edge_queries_accumulate(self._h))

    def edge_queries_reset(self):
        self._check(self._L.bisbm_edge_queries_reset(self._h))

    @staticmethod
    def _log_odds(w_sum, terms):
        """ln(w_sum / terms) with the C library's logarithm (the one the command line prints): NaN before the first sample,
        -inf where every counted chain's exp(-dS) is 0"""
        import math
        w = np.asarray(w_sum, dtype=np.float64)
        if not terms:
            return np.full(w.shape, np.nan)
        flat = [math.log(x) if x > 0 else (-math.inf if x == 0 else math.nan) for x in (w / float(terms)).ravel().tolist()]
        return np.array(flat, dtype=np.float64).reshape(w.shape)

    def edge_queries(self, i):
        """A dict for the i-th query, arrays [n_other] over its candidates in id order (candidate j of a type-a query is node
        na + j, of a type-b query node j): w_sum (float64), mult (uint32: the present multiplicity of the edge to the candidate),
        terms, and log_prob = ln(w_sum / terms), the log posterior-predictive odds of the graph with the edge added."""
        queries = getattr(self, "edge_query_nodes", np.zeros(0, dtype=np.uint32))
        i = int(i)
        if not 0 <= i < len(queries):
            raise IndexError("query index %d: %d queries are set" % (i, len(queries)))
        n_other = self.n - self.na if queries[i] < self.na else self.na
        w, mult = np.zeros(n_other, dtype=np.float64), np.zeros(n_other, dtype=np.uint32)
        terms = C.c_uint64()
        self._check(self._L.bisbm_edge_queries_get_row(self._h, i, _p(w, _f64p), _p(mult, _u32p), C.byref(terms)))
        return {"w_sum": w, "mult": mult, "terms": terms.value, "log_prob": self._log_odds(w, terms.value)}

    def edge_queries_topk(self, k, exclude_edges=True):
        """(nodes uint32 [Q, k], w_sum float64 [Q, k], terms): every query's k best candidates by pooled w_sum, descending, ties
        to the lowest node id, selected on the device.  exclude_edges: the query's neighbours are not eligible.  Entries past
        the eligible candidates are 0xffffffff / 0.0."""
        Q = len(getattr(self, "edge_query_nodes", ()))
        nodes = np.zeros((Q, int(k)), dtype=np.uint32)
        sums = np.zeros((Q, int(k)), dtype=np.float64)
        terms = C.c_uint64()
        self._check(self._L.bisbm_edge_queries_topk(self._h, int(k), 1 if exclude_edges else 0, _p(nodes, _u32p), _p(sums, _f64p), C.byref(terms)))
        return nodes, sums, terms.value

    def recommend_edges(self, k, exclude_edges=True):
        """(nodes uint32 [Q, k], w_sum float64 [Q, k], log_prob float64 [Q, k]): edge_queries_topk with log_prob =
        ln(w_sum / terms), the log odds of adding the edge between the query and the node (entries past the eligible
        candidates: node 0xffffffff, w_sum 0.0, log_prob -inf); edge_queries_topk gives the terms."""
        nodes, sums, terms = self.edge_queries_topk(k, exclude_edges)
        return nodes, sums, self._log_odds(sums, terms)

    # -- co-assignment (include/bisbm.h, "Co-assignment")
    def coassign_set(self, queries):
        """The nodes to find similar nodes for: an integer array [Q] of node ids of either type (they may repeat); replaces
        earlier queries and zeroes the counts.  Every query gets a row of one uint32 per node of its own type on the device.
        An empty array frees everything."""
        q = np.asarray(queries)
        if q.size == 0:
            q = np.zeros(0, dtype=np.uint32)
        if q.ndim != 1 or not np.issubdtype(q.dtype, np.integer):
            raise ValueError("queries must be a one-dimensional integer array")
        if len(q) and (q.min() < 0 or q.max() > 0xFFFFFFFF):
            raise ValueError("a query is outside [0, 2^32)")
        q = np.ascontiguousarray(q, dtype=np.uint32)
        self._check(self._L.bisbm_coassign_set(self._h, len(q), _p(q, _u32p)))
        self.coassign_queries = q.copy()

    def coassign_accumulate(self):
        """One sample: every counted chain adds 1 to every (query, node of its type) whose labels agree in that chain (with
        replica exchange on, the chains on rung 0 only)."""
        self._check(self._L.bisbm_coassign_accumulate(self._h))

    def coassign_reset(self):
        self._check(self._L.bisbm_coassign_reset(self._h))

    def coassignment(self, i):
        """(row uint32 [n_own], terms) of the i-th query: in how many of the `terms` counted (sample, chain) pairs every node
        of its type shared its block, in id order (candidate j of a type-a query is node j, of a type-b query node na + j)."""
        queries = getattr(self, "coassign_queries", np.zeros(0, dtype=np.uint32))
        i = int(i)
        if not 0 <= i < len(queries):
            raise IndexError("query index %d: %d queries are set" % (i, len(queries)))
        out = np.zeros(self.na if queries[i] < self.na else self.n - self.na, dtype=np.uint32)
        terms = C.c_uint64()
        self._check(self._L.bisbm_coassign_get_row(self._h, i, _p(out, _u32p), C.byref(terms)))
        return out, terms.value

    def coassign_topk(self, k):
        """(nodes uint32 [Q, k], counts uint32 [Q, k], terms): every query's k nodes of its own type with the largest counts,
        descending, ties to the lowest node id, selected on the device; the query node itself is never among them.  Entries
        past the eligible nodes are 0xffffffff / 0."""
        Q = len(getattr(self, "coassign_queries", ()))
        nodes = np.zeros((Q, int(k)), dtype=np.uint32)
        counts = np.zeros((Q, int(k)), dtype=np.uint32)
        terms = C.c_uint64()
        self._check(self._L.bisbm_coassign_topk(self._h, int(k), _p(nodes, _u32p), _p(counts, _u32p), C.byref(terms)))
        return nodes, counts, terms.value

    def similar(self, k):
        """(nodes uint32 [Q, k], probability float64 [Q, k], terms): coassign_topk with count / terms, the estimate of the
        posterior probability that the node shares the query's block."""
        nodes, counts, terms = self.coassign_topk(k)
        return nodes, counts / terms, terms

    # -- fold-in queries (include/bisbm.h, "Fold-in queries")
    def foldin_set(self, nodes, alpha=None, what=FOLDIN_RECOMMEND | FOLDIN_SIMILAR):
        """The virtual nodes to fold in: a sequence of (type, neighbours) with type "a" / "b" (or 0 / 1) and neighbours a
        non-empty sequence of ids of existing nodes of the OTHER type (they may repeat; the order is kept).  alpha: the
        smoothing constant, by default the model's epsilon.  what: the row kinds to keep.  Replaces earlier virtual nodes and
        zeroes the sums; an empty sequence frees everything."""
        types, lists = [], []
        for node in nodes:
            t, ids = node
            t = {"a": 0, "b": 1}.get(t, t)
            if isinstance(t, str) or int(t) != t or not 0 <= int(t) <= 255:
                raise ValueError("a virtual node's type must be 'a', 'b', 0 or 1")
            ids = np.asarray(ids)
            if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
                raise ValueError("a virtual node's neighbours must be a one-dimensional integer array")
            if ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF):
                raise ValueError("a neighbour is outside [0, 2^32)")
            types.append(int(t))
            lists.append(ids.astype(np.uint32))
        t = np.ascontiguousarray(types, dtype=np.uint8)
        ptr = np.zeros(len(lists) + 1, dtype=np.uint64)
        ptr[1:] = np.cumsum([len(x) for x in lists])
        flat = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), dtype=np.uint32)
        alpha = self.epsilon if alpha is None else float(alpha)
        self._check(self._L.bisbm_foldin_set(self._h, len(t), _p(t, _u8p), _p(ptr, _u64p), _p(flat, _u32p), alpha, int(what)))
        self.foldin_types, self.foldin_lists = t.copy(), lists

    def foldin_accumulate(self):
        """One sample: every counted chain's block posterior of every virtual node, and its terms added to the kept rows chain by
        chain in ascending order (with replica exchange on, the chains on rung 0 only)."""
        self._check(self._L.bisbm_foldin_accumulate(self._h))

    def foldin_reset(self):
        self._check(self._L.bisbm_foldin_reset(self._h))

    def _foldin_index(self, i):
        types = getattr(self, "foldin_types", np.zeros(0, dtype=np.uint8))
        i = int(i)
        if not 0 <= i < len(types):
            raise IndexError("virtual node %d: %d are set" % (i, len(types)))
        return i, int(types[i])

    def foldin_posteriors(self, i):
        """float64 [n_chains, K_own]: the i-th virtual node's block posterior in every chain at the last sample (row c, column =
        block within the node's type; K_own: the largest block count of that type among the chains, 0.0 past a chain's own;
        NaN rows: chains that were not counted)."""
        i, t = self._foldin_index(i)
        stride = max(self.ka_kb(c)[t] for c in range(self.n_chains)) if self.mixed_shapes else (self.KB if t else self.KA)
        out = np.zeros((self.n_chains, stride), dtype=np.float64)
        self._check(self._L.bisbm_foldin_get_posteriors(self._h, i, stride, _p(out, _f64p)))
        return out

    def foldin_scores(self, i, what):
        """(row float64, terms) of the i-th virtual node: what = FOLDIN_RECOMMEND: the sums over the nodes of the other type in id
        order; FOLDIN_SIMILAR: over the nodes of its own type (candidate j of type a is node j, of type b node na + j)."""
        i, t = self._foldin_index(i)
        cand_b = (t == 0) if what == FOLDIN_RECOMMEND else (t == 1)
        out = np.zeros(self.n - self.na if cand_b else self.na, dtype=np.float64)
        terms = C.c_uint64()
        self._check(self._L.bisbm_foldin_get_row(self._h, int(what), i, _p(out, _f64p), C.byref(terms)))
        return out, terms.value

    def foldin_topk(self, what, k, exclude_listed=False):
        """(nodes uint32 [Q, k], sums float64 [Q, k], terms): every virtual node's k best candidates of the rows of kind `what`,
        descending, ties to the lowest node id, selected on the device; 0xffffffff / 0.0 past the eligible candidates."""
        Q = len(getattr(self, "foldin_types", ()))
        nodes = np.zeros((Q, int(k)), dtype=np.uint32)
        sums = np.zeros((Q, int(k)), dtype=np.float64)
        terms = C.c_uint64()
        self._check(self._L.bisbm_foldin_topk(self._h, int(what), int(k), 1 if exclude_listed else 0, _p(nodes, _u32p), _p(sums, _f64p), C.byref(terms)))
        return nodes, sums, terms.value

    def foldin_recommend(self, k, exclude_listed=True):
        """(nodes, scores, terms): foldin_topk of the recommend rows with scores = sum / terms, the estimate of the expected number
        of edges between the virtual node and the node; exclude_listed: the nodes of its list are not eligible."""
        nodes, sums, terms = self.foldin_topk(FOLDIN_RECOMMEND, k, exclude_listed)
        return nodes, sums / terms, terms

    def foldin_similar(self, k):
        """(nodes, probability, terms): foldin_topk of the similar rows with sum / terms, the estimate of the posterior
        probability that the node shares the virtual node's block."""
        nodes, sums, terms = self.foldin_topk(FOLDIN_SIMILAR, k, False)
        return nodes, sums / terms, terms

    # -- node conditionals (include/bisbm.h, "Node conditionals")
    def conditionals_set(self, nodes=None, beta=1.0, keep_last=False):
        """The nodes whose full conditional P(b_v = s | all other labels) ~ exp(-beta dS(v -> s)) is evaluated: a sequence of
        node ids of either type (they may repeat), None: every node in id order.  keep_last: keep the dS and P rows of the last
        sample per chain (conditionals_last).  Replaces earlier queries, zeroes the sums and forgets the reference; an empty
        sequence frees everything."""
        if nodes is None:
            q, nq, ptr = np.arange(self.n, dtype=np.uint32), self.n, None
        else:
            q = np.asarray(nodes)
            if q.ndim != 1 or (q.size and not np.issubdtype(q.dtype, np.integer)):
                raise ValueError("the queries must be a one-dimensional integer array")
            if q.size and (q.min() < 0 or q.max() > 0xFFFFFFFF):
                raise ValueError("a query is outside [0, 2^32)")
            q = np.ascontiguousarray(q, dtype=np.uint32)
            nq, ptr = len(q), _p(q, _u32p)
        self._check(self._L.bisbm_conditionals_set(self._h, nq, ptr, float(beta), COND_KEEP_LAST if keep_last else 0))
        self.conditional_queries = q.copy()

    def conditionals_set_reference(self, labels):
        """The reference partition (n labels) every chain is aligned to before its conditional rows go into the soft marginals;
        None clears it.  Either way the soft marginals start afresh."""
        if labels is None:
            self._check(self._L.bisbm_conditionals_set_reference(self._h, None))
            return
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        if lab.shape != (self.n,):
            raise ValueError("the reference must hold n labels")
        self._check(self._L.bisbm_conditionals_set_reference(self._h, _p(lab, _u32p)))

    def conditionals_accumulate(self):
        """One sample: every counted chain's conditional of every query, its terms added to the kept sums chain by chain in
        ascending order (with replica exchange on, the chains on rung 0 only).  Chain state is only read."""
        self._check(self._L.bisbm_conditionals_accumulate(self._h))

    def conditionals_reset(self):
        self._check(self._L.bisbm_conditionals_reset(self._h))

    def conditionals_stats(self):
        """{"stay", "entropy", "margin": float64 [Q] sums over the counted chains, "free": uint64 [Q], "terms": int}: divide stay
        and entropy by terms, margin by free (the chains in which the node was not alone in its block)."""
        Q = len(getattr(self, "conditional_queries", ()))
        stay, ent, mar = (np.zeros(Q, dtype=np.float64) for _ in range(3))
        free = np.zeros(Q, dtype=np.uint64)
        terms = C.c_uint64()
        self._check(self._L.bisbm_conditionals_get_stats(self._h, _p(stay, _f64p), _p(ent, _f64p), _p(mar, _f64p), _p(free, _u64p), C.byref(terms)))
        return {"stay": stay, "entropy": ent, "margin": mar, "free": free, "terms": terms.value}

    def conditionals_marginals(self):
        """(prob float64 [Q, kmax], terms): the soft marginals -- every counted chain's conditional row added through its
        alignment to the reference; column = block within the query's type.  Needs conditionals_set_reference."""
        Q = len(getattr(self, "conditional_queries", ()))
        kmax, terms = C.c_uint32(), C.c_uint64()
        self._check(self._L.bisbm_conditionals_get_marginals(self._h, None, C.byref(kmax), C.byref(terms)))
        out = np.zeros((Q, kmax.value), dtype=np.float64)
        self._check(self._L.bisbm_conditionals_get_marginals(self._h, _p(out, _f64p), C.byref(kmax), C.byref(terms)))
        return out, terms.value

    def conditionals_last(self, i):
        """(dS, P) float64 [n_chains, K_own] of the i-th query at the last sample (row c, column = block within the node's type;
        K_own: the largest block count of that type among the chains, 0.0 past a chain's own; NaN rows: chains that were not
        counted).  Needs keep_last."""
        q = getattr(self, "conditional_queries", np.zeros(0, dtype=np.uint32))
        i = int(i)
        if not 0 <= i < len(q):
            raise IndexError("query %d: %d are set" % (i, len(q)))
        t = 1 if q[i] >= self.na else 0
        stride = max(self.ka_kb(c)[t] for c in range(self.n_chains)) if self.mixed_shapes else (self.KB if t else self.KA)
        dS = np.zeros((self.n_chains, stride), dtype=np.float64)
        P = np.zeros((self.n_chains, stride), dtype=np.float64)
        self._check(self._L.bisbm_conditionals_get_last(self._h, i, stride, _p(dS, _f64p), _p(P, _f64p)))
        return dS, P

    # -- held conditionals and the least settled queries (include/bisbm.h, "Held conditionals", "Least settled")
    def conditionals_held(self, on=True):
        """Switch what conditionals_accumulate evaluates: the held row -- the heat-bath kernel's row under the handle's clamp,
        block constraints and block fields as they are at each sample -- or (on=False) the model's unrestricted row.  A call that
        changes the switch zeroes the sums and the soft marginals and forgets the last rows; conditionals_set turns it off."""
        self._check(self._L.bisbm_held_conditionals_set(self._h, 1 if on else 0))

    def conditionals_is_held(self):
        on = C.c_int()
        self._check(self._L.bisbm_held_conditionals_get(self._h, C.byref(on)))
        return bool(on.value)

    def least_settled(self, k, by="entropy"):
        """(query indices uint32 [k], nodes int64 [k], values float64 [k], terms): the k queries with the largest entropy sum
        (by="entropy") or the smallest stay sum (by="stay") of conditionals_stats, selected on the device; ties in ascending query
        index.  Past the queries an index is QUERY_NONE, its node -1 and its value 0.0."""
        if by not in ("entropy", "stay"):
            raise ValueError("by = %r: \"entropy\" or \"stay\"" % (by,))
        k = int(k)
        idx = np.zeros(max(k, 0), dtype=np.uint32)
        val = np.zeros(max(k, 0), dtype=np.float64)
        terms = C.c_uint64()
        self._check(self._L.bisbm_least_settled_topk(self._h, SETTLED_BY_STAY if by == "stay" else SETTLED_BY_ENTROPY, k if k >= 0 else 0, _p(idx, _u32p),
                                                      _p(val, _f64p), C.byref(terms)))
        q = np.asarray(getattr(self, "conditional_queries", np.zeros(0, dtype=np.uint32)), dtype=np.int64)
        some = idx != QUERY_NONE
        nodes = np.full(len(idx), -1, dtype=np.int64)
        nodes[some] = q[idx[some]]
        return idx, nodes, val, terms.value

    # -- partition distances and posterior modes (include/bisbm.h, "Partition distances and posterior modes")
    def partition_distances(self, chains=None):
        """(vi float64 [m, m], H float64 [m]): the variation of information (nats) between every two of the selected chains'
        partitions and each one's partition entropy, in the order of `chains` (None: all chains).  Reads labels only."""
        if chains is None:
            sel, m, ptr = None, self.n_chains, None
        else:
            sel = np.ascontiguousarray(chains, dtype=np.uint32).ravel()
            m, ptr = len(sel), _p(sel, _u32p)
        vi = np.zeros((m, m), dtype=np.float64)
        H = np.zeros(m, dtype=np.float64)
        self._check(self._L.bisbm_partition_distances(self._h, m, ptr, _p(vi, _f64p), _p(H, _f64p)))
        return vi, H

    def partition_distances_to(self, refs, chains=None, shapes=None):
        """(vi float64 [m, R], H_ref float64 [R]): the variation of information (nats) between every selected chain's partition
        (None: all chains) and every row of `refs` [R, n], partitions of the same nodes that need not be chains, and each
        reference's partition entropy.  `shapes`: (ka, kb) for all references or one pair per reference; default: the model's
        (KA, KB).  Reads labels only."""
        r = np.ascontiguousarray(np.atleast_2d(refs), dtype=np.uint32)
        if r.ndim != 2 or r.shape[1] != self.n:
            raise ValueError("refs must have shape (n_refs, %d), got %s" % (self.n, r.shape))
        R = r.shape[0]
        sh = np.asarray((self.KA, self.KB) if shapes is None else shapes, dtype=np.int64)
        sh = np.broadcast_to(sh, (R, 2)) if sh.ndim == 1 else sh
        if sh.shape != (R, 2) or (R and (sh.min() < 0 or sh.max() > 0xFFFFFFFF)):
            raise ValueError("shapes must be one (ka, kb) or one per reference")
        rka = np.ascontiguousarray(sh[:, 0], dtype=np.uint32)
        rkb = np.ascontiguousarray(sh[:, 1], dtype=np.uint32)
        if chains is None:
            sel, m, ptr = None, self.n_chains, None
        else:
            sel = np.ascontiguousarray(chains, dtype=np.uint32).ravel()
            m, ptr = len(sel), _p(sel, _u32p)
        vi = np.zeros((m, R), dtype=np.float64)
        H = np.zeros(R, dtype=np.float64)
        self._check(self._L.bisbm_partition_distances_to(self._h, m, ptr, R, _p(r, _u32p), _p(rka, _u32p), _p(rkb, _u32p), _p(vi, _f64p), _p(H, _f64p)))
        return vi, H

    def partition_contingency(self, c, d):
        """uint32 [K_c, K_d]: how many nodes have label r in chain c and label s in chain d (global labels)."""
        c, d = int(c), int(d)
        for x in (c, d):
            if not 0 <= x < self.n_chains:
                raise BisbmError(BISBM_ERR_INVALID_ARG, "chain %d out of range: the model has %d chains" % (x, self.n_chains))
        out = np.zeros((sum(self.ka_kb(c)), sum(self.ka_kb(d))), dtype=np.uint32)
        self._check(self._L.bisbm_partition_contingency(self._h, int(c), int(d), _p(out, _u32p)))
        return out

    def partition_modes(self, threshold, chains=None):
        """The selected chains grouped into modes: single linkage over VI <= threshold (the caller's resolution: no default).
        `chains` None: all chains, or with replica exchange on the chains on rung 0.  Returns a dict: `chains` (the selection),
        `mode` (per selected chain), `medoids` (chain index per mode), `weights` (each mode's share of the selection),
        `lowest_entropy` (per mode the member chain of the least entropy()), `vi` (the matrix of the selection).
        The chains of this model only: pooling over ranks (ChainShard) is not done here."""
        if chains is None:
            sel = np.arange(self.n_chains, dtype=np.uint32)
            if self.tempering_L:
                sel = sel[self.tempering_state()[0] == 0]
        else:
            sel = np.ascontiguousarray(chains, dtype=np.uint32).ravel()
        vi, _ = self.partition_distances(sel)
        mode, med = partition_modes(vi, threshold)
        S = self.entropy()[sel]
        low = np.array([sel[mode == k][np.argmin(S[mode == k])] for k in range(len(med))], dtype=np.uint32)
        return {"chains": sel, "mode": mode, "medoids": sel[med], "weights": np.bincount(mode, minlength=len(med)) / len(sel),
                "lowest_entropy": low, "vi": vi}

    # -- chain traces (include/bisbm.h, "Chain traces")
    def trace_set(self, depth):
        """A ring of `depth` snapshots of every chain's partition on the device (0 frees it); forgets every earlier record."""
        self._check(self._L.bisbm_trace_set(self._h, int(depth)))
        self.trace_depth = int(depth)

    def trace_record(self):
        """One record: every chain's VI and unchanged-node count against each of its held snapshots, its description length and
        partition entropy appended to the series, then the current partitions pushed into the ring.  Reads state only."""
        self._check(self._L.bisbm_trace_record(self._h))

    def trace_reset(self):
        """Forgets snapshots, sums and series; the depth stays."""
        self._check(self._L.bisbm_trace_reset(self._h))

    def _trace_raw(self):
        D = int(getattr(self, "trace_depth", 0))
        vi_sum = np.zeros((self.n_chains, D), dtype=np.float64)
        agree = np.zeros((self.n_chains, D), dtype=np.uint64)
        vi_last = np.zeros((self.n_chains, D), dtype=np.float64)
        pairs = np.zeros(D, dtype=np.uint64)
        rec = C.c_uint64()
        self._check(self._L.bisbm_trace_get_lags(self._h, _p(vi_sum, _f64p), _p(agree, _u64p), _p(vi_last, _f64p), _p(pairs, _u64p), C.byref(rec)))
        return vi_sum, agree, vi_last, pairs, int(rec.value)

    def trace_lags(self):
        """The lag curves since the last set / reset, a dict of arrays [n_chains, depth] (column a - 1: age a, in records):
        `vi_mean` = vi_sum / pairs, `changed` = 1 - agree_sum / (pairs n), the share of nodes whose label differs, `vi_last` (the
        last record's VI, NaN for ages not yet held); and `vi_sum`, `agree_sum` as the library keeps them, `pairs` uint64 [depth],
        `records`.  Lags with pairs == 0 are NaN in vi_mean and changed."""
        vi_sum, agree, vi_last, pairs, rec = self._trace_raw()
        den = np.where(pairs > 0, pairs.astype(np.float64), np.nan)
        return {"vi_mean": vi_sum / den, "changed": 1.0 - agree.astype(np.float64) / (den * float(self.n)), "vi_last": vi_last,
                "vi_sum": vi_sum, "agree_sum": agree, "pairs": pairs, "records": rec}

    def trace_series(self, what="S"):
        """float64 [records, n_chains]: the description length ("S", what entropy() returned at every record) or the partition
        entropy ("H") of every chain at every record."""
        if what not in ("S", "H"):
            raise ValueError("what must be \"S\" or \"H\", not %r" % (what,))
        rec = C.c_uint64()
        self._check(self._L.bisbm_trace_get_lags(self._h, None, None, None, None, C.byref(rec)))
        out = np.zeros((int(rec.value), self.n_chains), dtype=np.float64)
        self._check(self._L.bisbm_trace_get_series(self._h, TRACE_S if what == "S" else TRACE_H, _p(out, _f64p)))
        return out

    # -- block summaries (include/bisbm.h, "Block summaries")
    def block_sums_set(self, on=True, keep_last=False):
        """Every aligned sample of marginals_accumulate also sums the counted chains' block states -- the ka x kb edge-count
        quadrant, the block sizes and the block degrees -- through the sample's permutations, per mode (mode 0: the pooled
        histogram).  `keep_last`: every counted chain's aligned tables of the last sample are kept too (block_last).  Every
        call zeroes the sums; on=False frees them."""
        what = (BLOCK_SUMS | (BLOCK_KEEP_LAST if keep_last else 0)) if on else 0
        self._check(self._L.bisbm_block_sums_set(self._h, what))

    def block_sums(self, mode=None):
        """The raw words of one mode (None: the pooled histogram's) as a dict: `terms` (chain samples), `e` uint64 [3, KA, KB],
        `n` and `d` uint64 [3, KA + KB]; plane 0 is the sum, 1 and 2 the low and high word of the sum of squares
        (sum x^2 = sq_hi * 2^32 + sq_lo)."""
        ka, kb = self.ka_kb(0)
        e = np.zeros((3, ka, kb), dtype=np.uint64)
        n = np.zeros((3, ka + kb), dtype=np.uint64)
        d = np.zeros((3, ka + kb), dtype=np.uint64)
        terms = C.c_uint64()
        self._check(self._L.bisbm_block_sums_get(self._h, 0 if mode is None else int(mode), C.byref(terms), _p(e, _u64p), _p(n, _u64p), _p(d, _u64p)))
        return {"terms": int(terms.value), "e": e, "n": n, "d": d}

    def block_summary(self, mode=None):
        """Means and standard deviations over the counted chain samples of one mode (None: the pooled histogram's), in the
        numbering of the node marginals of the same samples, as a dict: `terms`, `e_mean` / `e_sd` [KA, KB] (edges between
        type-a block R and type-b block KA + S), `n_mean` / `n_sd` and `m_r_mean` / `m_r_sd` [KA + KB] (block sizes and
        degrees), `share` = e_mean / e_mean.sum().  block_moments says how the moments are taken; terms = 0 gives NaN."""
        w = self.block_sums(mode)
        out = {"terms": w["terms"]}
        for key, name in (("e", "e"), ("n", "n"), ("d", "m_r")):
            mean, var = block_moments(w[key][0], w[key][1], w[key][2], w["terms"])
            out[name + "_mean"], out[name + "_sd"] = mean, np.sqrt(var)
        tot = out["e_mean"].sum()
        out["share"] = out["e_mean"] / tot if tot > 0 else np.full_like(out["e_mean"], np.nan)
        return out

    def block_last(self, chain):
        """(mode, e int32 [KA, KB], n_r int32 [KA + KB], m_r int32 [KA + KB]): the aligned tables of `chain` at the last sample
        and the mode it was counted into (block_sums_set(keep_last=True)); BISBM_ERR_STATE for a chain it did not count."""
        ka, kb = self.ka_kb(chain)
        e = np.zeros((ka, kb), dtype=np.int32)
        n_r = np.zeros(ka + kb, dtype=np.int32)
        m_r = np.zeros(ka + kb, dtype=np.int32)
        mode = C.c_uint32()
        self._check(self._L.bisbm_block_sums_get_last(self._h, int(chain), C.byref(mode), _p(e, _i32p), _p(n_r, _i32p), _p(m_r, _i32p)))
        return mode.value, e, n_r, m_r

    def device_layout(self):
        """(device ordinals, first chain of each device) behind this handle."""
        nd = C.c_int()
        self._check(self._L.bisbm_device_count(self._h, C.byref(nd), None, None))
        devs, first = (C.c_int * nd.value)(), np.zeros(nd.value, dtype=np.uint32)
        self._check(self._L.bisbm_device_count(self._h, C.byref(nd), devs, _p(first, _u32p)))
        return list(devs), first.tolist()

    def debug_log_q(self, n, k, fast=False):
        n = np.ascontiguousarray(n, dtype=np.int32)
        k = np.ascontiguousarray(k, dtype=np.int32)
        out = np.zeros(len(n), dtype=np.float64)
        self._check(self._L.bisbm_debug_log_q(self._h, _p(n, _i32p), _p(k, _i32p), len(n), int(bool(fast)),
                                              _p(out, _f64p)))
        return out


def align_assignment(table):
    """The alignment's assignment solver on the host (bisbm_align_assignment): table [k, k] of overlaps C[r][s] ->
    (perm uint32 [k] maximising sum_r C[r][perm[r]], that sum).  Needs no device."""
    t = np.ascontiguousarray(table, dtype=np.uint32)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or t.shape[0] == 0:
        raise ValueError("table must be a non-empty square matrix")
    perm = np.zeros(t.shape[0], dtype=np.uint32)
    tot = C.c_uint64()
    rc = lib().bisbm_align_assignment(t.shape[0], _p(t, _u32p), _p(perm, _u32p), C.byref(tot))
    if rc != BISBM_OK:
        raise BisbmError(rc, (lib().bisbm_last_error(None) or b"").decode())
    return perm, tot.value


def mode_assignment(mode_of_chain, n_chains, n_modes=None):
    """(mode_of_chain uint32 [n_chains], n_modes) from a per-chain array (MODE_NONE: not counted) or from the dict
    BlockModel.partition_modes returns (chains outside its selection become MODE_NONE).  Needs no device."""
    if isinstance(mode_of_chain, dict):
        sel = np.asarray(mode_of_chain["chains"], dtype=np.int64).ravel()
        mode = np.asarray(mode_of_chain["mode"], dtype=np.int64).ravel()
        if len(sel) != len(mode) or (len(sel) and (sel.min() < 0 or sel.max() >= n_chains)):
            raise ValueError("the grouping names chains outside the model's %d" % n_chains)
        moc = np.full(n_chains, MODE_NONE, dtype=np.uint32)
        moc[sel] = mode
        if n_modes is None:
            n_modes = len(mode_of_chain["medoids"])
    else:
        raw = np.asarray(mode_of_chain)
        if raw.ndim != 1 or len(raw) != n_chains:
            raise ValueError("mode_of_chain has %s entries, the model has %d chains" % (raw.shape, n_chains))
        if not np.issubdtype(raw.dtype, np.integer) or (len(raw) and (raw.min() < 0 or raw.max() > MODE_NONE)):
            raise ValueError("mode_of_chain must hold integers in [0, 2^32)")
        moc = np.ascontiguousarray(raw, dtype=np.uint32)
        if n_modes is None:
            counted = moc[moc != MODE_NONE]
            n_modes = int(counted.max()) + 1 if len(counted) else 0
    if int(n_modes) < 1:
        raise ValueError("no chain is given a mode")
    return moc, int(n_modes)


def numpy_block_sums(perms, quads, n_rs, m_rs, modes, n_modes, ka, kb):
    """The literal model of the block summaries (include/bisbm.h, "Block summaries"); needs no device.  For every chain c with
    modes[c] = g != MODE_NONE, pi = perms[c] (global-label form, uint [ka + kb]), quads[c] [ka, kb], n_rs[c] and m_rs[c]
    [ka + kb]:
        E[g][pi(a)][pi(ka + b) - ka] += quads[c][a][b];  N[g][pi(r)] += n_rs[c][r];  D[g][pi(r)] += m_rs[c][r];  terms[g] += 1
    where adding x to a cell adds x to its plane 0, (x * x) & 0xffffffff to plane 1 and (x * x) >> 32 to plane 2.  Returns a dict
    `terms` uint64 [n_modes], `e` uint64 [n_modes, 3, ka, kb], `n` and `d` uint64 [n_modes, 3, ka + kb]."""
    K = ka + kb
    out = {"terms": np.zeros(n_modes, dtype=np.uint64), "e": np.zeros((n_modes, 3, ka, kb), dtype=np.uint64),
           "n": np.zeros((n_modes, 3, K), dtype=np.uint64), "d": np.zeros((n_modes, 3, K), dtype=np.uint64)}

    def add(planes, index, x):
        x = int(x)
        planes[(0,) + index] += np.uint64(x)
        planes[(1,) + index] += np.uint64((x * x) & 0xFFFFFFFF)
        planes[(2,) + index] += np.uint64((x * x) >> 32)
    for c in range(len(modes)):
        g = int(modes[c])
        if g == MODE_NONE:
            continue
        pi = [int(v) for v in perms[c]]
        for a in range(ka):
            for b in range(kb):
                add(out["e"][g], (pi[a], pi[ka + b] - ka), quads[c][a][b])
        for r in range(K):
            add(out["n"][g], (pi[r],), n_rs[c][r])
            add(out["d"][g], (pi[r],), m_rs[c][r])
        out["terms"][g] += np.uint64(1)
    return out


def block_moments(sum, sq_lo, sq_hi, terms):
    """(mean, variance) float64 arrays of the cells whose three accumulators are given (arrays of one shape), over `terms`
    samples.  mean = sum / terms.  With S2 = sq_hi * 2^32 + sq_lo (the exact sum of squares), variance =
    (S2 * terms - sum^2) / terms^2: numerator and denominator are taken in Python integers and divided once, so the (population)
    variance is never negative and is exactly 0.0 when all samples agree.  terms = 0 gives NaN.  Needs no device."""
    s, lo, hi = (np.asarray(a, dtype=np.uint64) for a in (sum, sq_lo, sq_hi))
    t = int(terms)
    mean = np.full(s.shape, np.nan)
    var = np.full(s.shape, np.nan)
    if t > 0:
        for i in np.ndindex(*s.shape):
            x, s2 = int(s[i]), (int(hi[i]) << 32) + int(lo[i])
            mean[i] = x / t
            var[i] = (s2 * t - x * x) / (t * t)
    return mean, var


def partition_modes(vi, threshold):
    """Modes of a symmetric VI matrix [m, m] on the host (bisbm_partition_modes): single linkage over VI <= threshold ->
    (mode uint32 [m], numbered by lowest member; medoids uint32 [n_modes], indices into the matrix).  Needs no device."""
    v = np.ascontiguousarray(vi, dtype=np.float64)
    if v.ndim != 2 or v.shape[0] != v.shape[1]:
        raise ValueError("vi must be a square matrix")
    m = v.shape[0]
    mode = np.zeros(max(m, 1), dtype=np.uint32)
    med = np.zeros(max(m, 1), dtype=np.uint32)
    n_modes = C.c_uint32()
    rc = lib().bisbm_partition_modes(m, _p(v, _f64p), float(threshold), _p(mode, _u32p), _p(med, _u32p), C.byref(n_modes))
    if rc != BISBM_OK:
        raise BisbmError(rc, (lib().bisbm_last_error(None) or b"").decode())
    return mode[:m], med[: n_modes.value]


def trace_summary(x, window=5.0):
    """(tau float64 [C], window uint32 [C], rhat) of a series x [T, C] (one column per chain; a 1-d series is one chain) on the
    host (bisbm_trace_summary): each chain's integrated autocorrelation time with Sokal's automatic window (stop at the first
    lag M >= window * tau; window[c] == T // 2 says the series was too short, a chain that never moved has tau = inf and window
    0), and the split R-hat over the chains.  5.0 is Sokal's convention, not a measurement.  Needs no device."""
    v = np.asarray(x, dtype=np.float64)
    if v.ndim == 1:
        v = v[:, None]
    if v.ndim != 2:
        raise ValueError("x must be a series [T] or [T, C]")
    v = np.ascontiguousarray(v)
    T, Cn = v.shape
    tau = np.zeros(max(Cn, 1), dtype=np.float64)
    win = np.zeros(max(Cn, 1), dtype=np.uint32)
    rhat = C.c_double()
    rc = lib().bisbm_trace_summary(T, Cn, _p(v, _f64p), float(window), _p(tau, _f64p), _p(win, _u32p), C.byref(rhat))
    if rc != BISBM_OK:
        raise BisbmError(rc, (lib().bisbm_last_error(None) or b"").decode())
    return tau[:Cn], win[:Cn], rhat.value


def validate_ladder(ladder):
    """A replica-exchange ladder as float32 (what the library runs), or ValueError: at least 2 temperatures, each finite and
    > 0 as a float32, non-decreasing."""
    try:
        vals = [float(x) for x in ladder]
    except (TypeError, ValueError):
        raise ValueError("the temperature ladder must be a sequence of numbers")
    if len(vals) < 2:
        raise ValueError("a temperature ladder needs at least 2 rungs, got %d" % len(vals))
    with np.errstate(over="ignore"):
        lad = np.asarray(vals, dtype=np.float32)
    for i, t in enumerate(lad):
        if not (np.isfinite(t) and t > 0):
            raise ValueError("ladder[%d] = %s: every temperature must be finite and > 0" % (i, vals[i]))
        if i and t < lad[i - 1]:
            raise ValueError("ladder[%d] = %s < ladder[%d] = %s: the ladder must be non-decreasing" % (i, vals[i], i - 1, vals[i - 1]))
    return lad


RUNG_STAT_COLUMNS = ("mh_steps", "mh_accepted", "heatbath_steps", "heatbath_moves", "reshuffles", "reshuffles_accepted")


def round_recipe(mh=1, heatbath=0, reshuffles=0, scans=3):
    """The bisbm_round_recipe of a round of `mh` MH sweeps, `heatbath` heat-bath sweeps and `reshuffles` pair reshuffles of
    `scans` launch scans, or ValueError: every count an integer in [0, 2^32), not all three moves 0."""
    vals = []
    for name, v in (("mh", mh), ("heatbath", heatbath), ("reshuffles", reshuffles), ("scans", scans)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s = %r is not an integer" % (name, v))
        if not 0 <= int(v) < 1 << 32:
            raise ValueError("%s = %r is outside [0, 2^32)" % (name, v))
        vals.append(int(v))
    if vals[0] == 0 and vals[1] == 0 and vals[2] == 0:
        raise ValueError("a round of mh = 0, heatbath = 0 and reshuffles = 0 runs nothing")
    return RoundRecipe(*vals)


def rung_moves_recipe(rung_moves):
    """The keyword `rung_moves` of marginalize() and friends -- a dict with some of the keys mh (default 1), heatbath (0),
    reshuffles (0), scans (3) -- as keyword arguments of BlockModel.tempering_rounds, or ValueError."""
    if not isinstance(rung_moves, dict):
        raise ValueError("rung_moves must be a dict with the keys mh, heatbath, reshuffles, scans, not %r" % (rung_moves,))
    unknown = sorted(set(rung_moves) - {"mh", "heatbath", "reshuffles", "scans"})
    if unknown:
        raise ValueError("rung_moves has unknown keys %s (known: mh, heatbath, reshuffles, scans)" % unknown)
    kw = {"mh": 1, "heatbath": 0, "reshuffles": 0, "scans": 3}
    kw.update(rung_moves)
    round_recipe(**kw)
    return {k: int(v) for k, v in kw.items()}


def numpy_rung_tally(stats, rung, mh_steps=0, mh_accepted=0, heatbath_steps=0, heatbath_moves=0, reshuffles=0, reshuffles_accepted=0):
    """The per-rung tally of one round on the host (bisbm_tempering_rung_stats): every chain's six deltas (scalars or arrays
    [n_chains]) added to row rung[c] of `stats` (uint64 [L, 6], changed in place and returned) -- the rungs the chains held
    during the round, before its exchange."""
    rung = np.asarray(rung, dtype=np.int64)
    for col, d in enumerate((mh_steps, mh_accepted, heatbath_steps, heatbath_moves, reshuffles, reshuffles_accepted)):
        np.add.at(stats[:, col], rung, np.broadcast_to(np.asarray(d, dtype=np.uint64), rung.shape))
    return stats


def validate_population_temps(temps):
    """The temperatures of a population run as float32 (what the library runs), or ValueError: at least 2, each finite and > 0
    as a float32, non-increasing."""
    try:
        vals = [float(x) for x in temps]
    except (TypeError, ValueError):
        raise ValueError("the temperatures must be a sequence of numbers")
    if len(vals) < 2:
        raise ValueError("a population run needs at least 2 temperatures, got %d" % len(vals))
    with np.errstate(over="ignore"):
        T = np.asarray(vals, dtype=np.float32)
    for i, t in enumerate(T):
        if not (np.isfinite(t) and t > 0):
            raise ValueError("temps[%d] = %s: every temperature must be finite and > 0" % (i, vals[i]))
        if i and t > T[i - 1]:
            raise ValueError("temps[%d] = %s > temps[%d] = %s: the temperatures must be non-increasing" % (i, vals[i], i - 1, vals[i - 1]))
    return T


def population_offspring(S, delta_beta, u):
    """Offspring counts, parent map and log ratio of one resampling step on the host (bisbm_population_offspring): description
    lengths S [C], delta_beta >= 0, one uniform u in [0, 1) -> (offspring uint32 [C], parent uint32 [C], log_ratio).  Needs no
    device."""
    s = np.ascontiguousarray(S, dtype=np.float64).ravel()
    off = np.zeros(max(len(s), 1), dtype=np.uint32)
    parent = np.zeros(max(len(s), 1), dtype=np.uint32)
    lr = C.c_double()
    rc = lib().bisbm_population_offspring(len(s), _p(s, _f64p), float(delta_beta), float(u), _p(off, _u32p), _p(parent, _u32p), C.byref(lr))
    if rc != BISBM_OK:
        raise BisbmError(rc, (lib().bisbm_last_error(None) or b"").decode())
    return off[: len(s)], parent[: len(s)], lr.value


def population_anneal(model, temps, sweeps_per_step, burn_in_sweeps=0, rung_moves=None):
    """Population annealing of all chains of `model`: `burn_in_sweeps` sweeps at temps[0], then BlockModel.population_run.
    Returns its dict plus "entropy" (the description length of every chain at the end) and "best_chain" (its argmin, ties ->
    the lowest chain).  `rung_moves`: a dict {"mh", "heatbath", "reshuffles", "scans"} as in marginalize() -- every step then
    runs `sweeps_per_step` ROUNDS of those moves at the step's temperature (BlockModel.population_rounds)."""
    T = validate_population_temps(temps)
    recipe = rung_moves_recipe(rung_moves) if rung_moves is not None else None
    if int(burn_in_sweeps) > 0:
        model.run_sweeps(int(burn_in_sweeps), float(T[0]))
    out = model.population_run(T, sweeps_per_step) if recipe is None else model.population_rounds(T, sweeps_per_step, **recipe)
    out["entropy"] = model.entropy()
    out["best_chain"] = int(np.argmin(out["entropy"]))
    return out


def _fmt_g6(x):
    """What `std::clog << double` prints (6 significant digits, %g)."""
    return "%g" % x


# --------------------------------------------------------------------------- metropolis_hasting
class MetropolisHasting:
    """Mirror of ``metropolis_hasting`` (metropolis_hasting.hh:23-71)."""

    def anneal(self, blockmodel, cooling_schedule, cooling_schedule_kwargs, duration, steps_await, engine=None):
        """metropolis_hasting.cc:64-101.  Returns the acceptance rate: a float for one chain, an
        array for several."""
        kw = np.zeros(2, dtype=np.float32)
        vals = list(cooling_schedule_kwargs)[:2]
        kw[: len(vals)] = vals
        rates = np.zeros(blockmodel.n_chains, dtype=np.float64)
        blockmodel._check(blockmodel._L.bisbm_anneal(blockmodel._h, _schedule_id(cooling_schedule), _p(kw, _f32p),
                                                     int(duration), int(steps_await), _p(rates, _f64p)))
        return float(rates[0]) if blockmodel.n_chains == 1 else rates


metropolis_hasting = MetropolisHasting
blockmodel_t = BlockModel

from .distributed import (ChainShard, numpy_coassign, numpy_conditional_row, numpy_held_conditional_row, numpy_least_settled, numpy_foldin_posterior, numpy_foldin_rows, numpy_foldin_tables, numpy_heatbath_choice, numpy_reshuffle_accept, numpy_reshuffle_launch, numpy_reshuffle_pair, numpy_reshuffle_q, numpy_reshuffle_step, numpy_split_merge_accept, numpy_split_merge_choice, numpy_split_merge_launch, numpy_split_merge_dS, numpy_split_merge_step, numpy_split_merge_renumber, numpy_split_merge_roles, numpy_split_merge_pairs,  # noqa: E402,F401
                          numpy_edge_dS, numpy_edge_multiplicity, numpy_edge_query_rows, numpy_pair_scores, numpy_query_topk, shard_chains)
from .marginalize import marginalize, marginalize_modes  # noqa: E402,F401
