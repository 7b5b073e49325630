"""The table of tests/state_cases.py covers the ABI: every prototype of include/bspgemm.h that takes a bspgemm_context * is
named by a case, is part of how every case runs, or is exempt for a stated reason.  A new entry point fails here until it
joins the table (and with it the poisoned-memory and workspace-layout tests).  CPU only: nothing here touches a GPU.
"""
import os
import re

import state_cases
from abi_kit import ROOT


# what every case goes through on its way in and out (state_cases.Ops.upload, _matrix, _result; the tests' scribble)
PLUMBING = {
    "bspgemm_matrix_upload": "every case uploads its operands through it",
    "bspgemm_matrix_download": "every case that returns an operand downloads it",
    "bspgemm_result_download": "every case that returns a result downloads it",
    "bspgemm_result_download_values": "every case that returns a counted result downloads its values",
    "bspgemm_debug_scribble": "the hook itself: the dirty-state tests call it between the runs of every case",
}
# entry points that launch no kernel and touch no workspace
EXEMPT = {
    "bspgemm_destroy": "frees the context",
    "bspgemm_set_stream": "stream setter: synchronises and swaps a handle",
    "bspgemm_synchronize": "waits for the stream",
    "bspgemm_set_flow": "option",
    "bspgemm_set_class_timing": "option",
    "bspgemm_set_option": "option",
    "bspgemm_get_option": "option",
    "bspgemm_matrix_wrap_device": "wraps the caller's arrays in a handle: no allocation, no launch",
    "bspgemm_last_stats": "reads host-side statistics",
    "bspgemm_stats_at": "reads host-side statistics",
    "bspgemm_comm_create": "communicator layer (csrc/comm.hip): hooks and tests of its own",
    "bspgemm_comm_create_host": "communicator layer (csrc/comm.hip): hooks and tests of its own",
}
# what the table must hold whatever else changes: none of these may ever be exempted
COMPUTE = """bspgemm_multiply bspgemm_multiply_masked bspgemm_multiply_masked_ex bspgemm_multiply_accumulate
bspgemm_multiply_masked_count bspgemm_multiply_masked_dot bspgemm_matrix_from_result bspgemm_matrix_from_result_where
bspgemm_matrix_select bspgemm_matrix_setop bspgemm_matrix_equal bspgemm_matrix_symmetrize bspgemm_matrix_transpose
bspgemm_matrix_extract bspgemm_matrix_extract_rows_of bspgemm_closure bspgemm_closure_ex bspgemm_triangle_count
bspgemm_triangle_count_ex bspgemm_ktruss bspgemm_ktruss_ex bspgemm_bfs bspgemm_bfs_tree bspgemm_connected_components
bspgemm_strongly_connected_components bspgemm_core_numbers bspgemm_kcore bspgemm_graph_coloring bspgemm_label_propagation
bspgemm_local_clustering bspgemm_pagerank bspgemm_betweenness bspgemm_maximal_matching bspgemm_weights_hashed bspgemm_sssp
bspgemm_row_work_prefix bspgemm_partition_rows bspgemm_lengths_to_row_ptr""".split()


def context_prototypes():
    """every function of include/bspgemm.h with a parameter of type [const] bspgemm_context *"""
    text = open(os.path.join(ROOT, "include", "bspgemm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.findall(r"\b(bspgemm_[a-zA-Z0-9_]+|SpGEMM_hip[a-zA-Z0-9_]*)\s*\(([^()]*)\)\s*;", text)
    return sorted(name for name, params in found if re.search(r"\bbspgemm_context\s*\*(?!\s*\*)", params))


def test_every_context_entry_point_is_a_case_or_exempt():
    protos = context_prototypes()
    assert len(protos) >= 55 and "bspgemm_sssp" in protos and "bspgemm_create" not in protos
    covered = state_cases.covered_entries()
    assert covered <= set(protos), "cases name what the header does not declare: %s" % sorted(covered - set(protos))
    groups = (covered, set(PLUMBING), set(EXEMPT))
    homeless = [p for p in protos if not any(p in grp for grp in groups)]
    assert not homeless, "neither a case of tests/state_cases.py nor exempt: %s" % homeless
    assert not covered & set(EXEMPT), "exempt and covered at once: %s" % sorted(covered & set(EXEMPT))
    stale = (set(PLUMBING) | set(EXEMPT)) - set(protos)
    assert not stale, "listed here, gone from the header: %s" % sorted(stale)
    assert all(reason and "\n" not in reason for reason in list(EXEMPT.values()) + list(PLUMBING.values()))


def test_no_compute_entry_point_is_exempt():
    assert len(COMPUTE) == 38 and set(COMPUTE) <= set(context_prototypes())
    assert not set(COMPUTE) & (set(EXEMPT) | set(PLUMBING))
    missing = set(COMPUTE) - state_cases.covered_entries()
    assert not missing, "compute entry points without a case: %s" % sorted(missing)


def test_the_table_is_well_formed():
    """every case names operands that exist, options that exist, and the forced-option cases run on the hub graph"""
    for name, case in state_cases.CASES.items():
        assert case.entries and case.on and callable(case.run) and callable(case.check), name
        assert all(on in state_cases._BUILDERS for on in case.on), name
        assert all(k in state_cases.bspgemm.OPTIONS for k in case.options), name
    forced = {k for c in state_cases.CASES.values() for k in c.options}
    assert {"lp_min_class", "pr_min_class", "bc_lanes", "match_lanes", "extract_lanes", "bfs_push_lanes"} <= forced
    assert {"bfs_tree", "pagerank_pull", "masked_dot", "extract", "core_numbers"} <= set(state_cases.GRAPH_CASES)
    assert len(state_cases.IDS) == len(set(state_cases.IDS))


def test_the_operands_are_what_the_cases_need():
    rp, ci, n = state_cases.operands("hub").host["A"][:3]
    assert n == 6000 and rp[1] - rp[0] > 4096 and (ci == 0).sum() > 4096      # out- and in-degree of the hub above the chunk sizes
    assert ci.size % 4 and ci.size % 4096
    rp, ci, n = state_cases.operands("gap").host["A"][:3]
    lens = rp[1:] - rp[:-1]
    assert (lens[6:n - 6] == 0).all() and n - 12 > 4096 and lens[:6].min() > 0 and lens[n - 6:].min() > 0
    for name in state_cases.GRAPHS:                                            # untidy storage: canonicalising runs inside the calls
        rp, ci, n = state_cases.operands(name).host["A"][:3]
        assert not state_cases.pagerank_ref.is_canonical(rp, ci, n), name
