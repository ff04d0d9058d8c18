"""Threshold sweep (ipc_run_sweep / ipc_sweep_reset), the parts that need no GPU: the C ABI exports and binds the two symbols
and reports argument errors, and -- on the CPU oracle -- the premise of the feature: the thresholds enter after the
optimisation (reference src/consensus_utils.cpp:17-19), so the matrix of max chi2 is the same bytes at every threshold pair
and only the decisions change."""
import ctypes

import numpy as np
import pytest

import sweep_cases as SC

SWEEP = ("ipc_run_sweep", "ipc_sweep_reset")


def test_sweep_symbols_exported_and_argument_errors_reported():
    import __graft_entry__ as ge
    ge.build()
    from ipc_amd import capi
    lib = capi.load()
    for name in SWEEP:
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    # the report struct is eight ints, in the header's order
    assert [f for f, _ in capi.SweepReport._fields_] == ["thresholds", "cells", "long_cells", "damped_cells", "literal_cells",
                                                         "literal_held", "reused_solve", "chunks"]
    assert all(t is ctypes.c_int for _, t in capi.SweepReport._fields_)
    assert ctypes.sizeof(capi.SweepReport) == 32
    # NULL handle => -1 (IPC_ERR_ARG) + message, no crash, no GPU needed; outputs stay untouched
    rep = capi.SweepReport(7, 7, 7, 7, 7, 7, 7, 7)
    th = (ctypes.c_double * 2)(6.251, 11.345)
    assert lib.ipc_run_sweep(None, 2, th, th, None, None, ctypes.byref(rep)) == -1
    assert b"NULL handle" in lib.ipc_last_error()
    assert rep.thresholds == 7 and rep.chunks == 7
    assert lib.ipc_sweep_reset(None) == -1
    assert b"NULL handle" in lib.ipc_last_error()


def test_python_surface():
    from ipc_amd.consensus import IPC
    for name in ("run_sweep", "sweep_reset"):
        assert callable(getattr(IPC, name)), name


def _matrix(O, g, fast, slow):
    cfg = SC.config(g, fast, slow)
    return O.consistency_matrix(g.dim, g.odom_meas, g.odom_info, cfg.s_factor, g.loop_ids, g.loop_meas, g.loop_info,
                                cfg.fast_reject_th, cfg.fast_reject_iter_base, cfg.slow_reject_th, cfg.slow_reject_iter_base)


@pytest.mark.parametrize("name,pairs", [("se3", SC.PAIRS[:4]), ("se2", [SC.PAIRS[0], SC.PAIRS[3]])], ids=["se3", "se2"])
def test_oracle_chi2_does_not_depend_on_the_thresholds(oracle, name, pairs):
    """The oracle optimises a cell and compares afterwards: maxchi2 is byte-equal at every pair (NaNs included) and `ok` is the
    decision rule applied to it -- the diagonal on `fast`, overlapping pairs on `slow`, otherwise ok[i][i] & ok[j][j]."""
    g = SC.graph(name)
    assert (g.V, g.N) == ((400, 40) if name == "se2" else (128, 36))
    mx0, seen = None, set()
    for fast, slow in pairs:
        ok, mx = _matrix(oracle, g, fast, slow)
        if mx0 is None:
            mx0 = mx
        assert mx.tobytes() == mx0.tobytes(), (fast, slow)
        assert np.array_equal(ok, SC.ok_from_chi2(g, mx0, fast, slow)), (fast, slow)
        seen.add(ok.tobytes())
    assert len(seen) >= 2                                     # the decisions do change with the pair
