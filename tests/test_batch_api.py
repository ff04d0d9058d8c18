"""Monte-Carlo batch (ipc_run_batch), the parts that need no GPU: the C ABI exports and binds the symbol and reports a NULL
handle, and -- on the CPU oracle -- the premises of the feature: over the cells themselves the matrix of a sub-list is the
sub-matrix of the union's matrix; the processing order of a sub-list with increasing members is the union's order restricted and
relabelled; and the greedy set of a sub-list is NOT the union's set restricted to it, so every run needs its own set-max."""
import ctypes
import os

import numpy as np
import pytest

import sweep_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def member_lists(N):
    """Member lists that are no prefixes of the union: every third candidate from 1, and a head with a gap behind it."""
    return [np.arange(1, N, 3), np.concatenate([np.arange(0, 16), np.arange(24, 32)])]


def test_batch_symbol_exported_and_null_handle_reported():
    import __graft_entry__ as ge
    ge.build()
    from ipc_amd import capi
    lib = capi.load()
    assert hasattr(lib, "ipc_run_batch")
    assert "ipc_run_batch" in capi.SYMBOLS
    assert lib.ipc_run_batch.argtypes is not None
    header = open(os.path.join(ROOT, "include", "ipc_amd.h")).read()
    assert "int ipc_run_batch(ipc_engine_t* h, int n_runs, const int* run_offsets, const int* members" in header
    assert "ipc_batch_report_t" in header and "STRICTLY INCREASING" in header
    # the report struct in the header's order: three ints, a 64-bit count on its natural alignment, four ints
    assert [f for f, _ in capi.BatchReport._fields_] == ["runs", "union_candidates", "cells", "cells_separate", "long_cells",
                                                         "damped_cells", "literal_cells", "chunks"]
    assert [t for _, t in capi.BatchReport._fields_] == [ctypes.c_int] * 3 + [ctypes.c_longlong] + [ctypes.c_int] * 4
    assert ctypes.sizeof(capi.BatchReport) == 40 and capi.BatchReport.cells_separate.offset == 16
    # NULL handle => -1 (IPC_ERR_ARG) + message, no crash, no GPU needed; outputs stay untouched
    rep = capi.BatchReport(7, 7, 7, 7, 7, 7, 7, 7)
    off = (ctypes.c_int * 2)(0, 1)
    mem = (ctypes.c_int * 1)(0)
    assert lib.ipc_run_batch(None, 1, off, mem, None, None, ctypes.byref(rep)) == -1
    assert b"NULL handle" in lib.ipc_last_error()
    assert rep.runs == 7 and rep.cells_separate == 7 and rep.chunks == 7


def test_python_surface():
    from ipc_amd.consensus import IPC
    assert callable(getattr(IPC, "run_batch"))


TIGHT = SC.PAIRS[3]                                           # (0.5, 1.0): pair cells do reject, so the greedy has verdicts to take


def _matrix(O, g, fast=6.251, slow=11.345):
    cfg = SC.config(g, fast, slow)
    return O.consistency_matrix(g.dim, g.odom_meas, g.odom_info, cfg.s_factor, g.loop_ids, g.loop_meas, g.loop_info,
                                cfg.fast_reject_th, cfg.fast_reject_iter_base, cfg.slow_reject_th, cfg.slow_reject_iter_base)


_full = {}


def _full_matrix(O, name):
    if name not in _full:
        _full[name] = _matrix(O, SC.graph(name))
    return _full[name]


@pytest.mark.parametrize("name", ["se2", "se3"])
def test_oracle_matrix_of_a_sub_list_is_the_sub_matrix(oracle, name):
    g = SC.graph(name)
    ok, mx = _full_matrix(oracle, name)
    for m in member_lists(g.N):
        assert m.max() < g.N and not np.array_equal(m, np.arange(len(m)))       # no prefix
        ok_s, mx_s = _matrix(oracle, SC.stub(g, sel=m))
        assert mx_s.tobytes() == np.ascontiguousarray(mx[np.ix_(m, m)]).tobytes(), (name, len(m))
        assert ok_s.tobytes() == np.ascontiguousarray(ok[np.ix_(m, m)]).tobytes(), (name, len(m))


def test_oracle_greedy_set_of_a_sub_list_is_not_the_restricted_set(oracle):
    """At the default thresholds every candidate of the small graphs whose own cell passes is accepted and the greedy has nothing
    to decide; at the tight pair of sweep_cases it does.  The union's decisions at that pair are the rule applied to the chi2
    matrix (the thresholds enter after the optimisation: tests/test_sweep_api.py), the sub-lists go through the oracle."""
    g = SC.graph("se2")
    _, mx = _full_matrix(oracle, "se2")
    ok = SC.ok_from_chi2(g, mx, *TIGHT)
    acc = oracle.set_max(ok, oracle.candidate_order(g.loop_ids))
    assert 0 < acc.sum() < np.diag(ok).sum()                  # the greedy does reject candidates whose own cell passed
    differs = []
    for m in member_lists(g.N):
        sub = SC.stub(g, sel=m)
        ok_s, _ = _matrix(oracle, sub, *TIGHT)
        assert np.array_equal(ok_s, ok[np.ix_(m, m)])
        acc_s = oracle.set_max(ok_s, oracle.candidate_order(sub.loop_ids))
        differs.append(not np.array_equal(acc_s, acc[m]))
    # ... which is why the batch runs a set-max per run: dropping a candidate frees the ones it was blocking
    assert any(differs)


def test_oracle_order_of_a_sub_list_is_the_restricted_order(oracle):
    """With increasing members the (max id, local index) order of the sub-list is the union's (max id, index) order restricted
    to the members and relabelled -- on a list with ties in max id."""
    g = SC.graph("wide")
    hi = g.loop_ids.max(axis=1)
    assert len(np.unique(hi)) < g.N                                              # ties
    order = np.asarray(oracle.candidate_order(g.loop_ids))
    for m in member_lists(g.N) + [np.arange(g.N - 65, g.N)]:
        tied = [h for h in np.unique(hi[m]) if (hi[m] == h).sum() > 1]
        assert tied, "the member list holds no tie"
        loc = -np.ones(g.N, dtype=np.int64)
        loc[m] = np.arange(len(m))
        restricted = loc[order][loc[order] >= 0]
        sub_order = np.asarray(oracle.candidate_order(SC.stub(g, sel=m).loop_ids))
        assert np.array_equal(sub_order, restricted)
