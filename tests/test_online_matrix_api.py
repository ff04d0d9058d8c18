"""Online matrix mode (ipc_run_online / ipc_online_covered / ipc_online_reset / ipc_reserve_candidates), the parts that need no
GPU: the C ABI exports and binds the four symbols and reports argument errors, and -- on the CPU oracle -- the two facts the
feature rests on: the consistency matrix over the first n candidates is the leading n x n block of the matrix over all of them,
and the greedy set over a prefix of the processing order is the whole run's set restricted to that prefix."""
import ctypes

import numpy as np
import pytest

ONLINE = ("ipc_run_online", "ipc_online_covered", "ipc_online_reset", "ipc_reserve_candidates")


def test_online_matrix_symbols_exported_and_argument_errors_reported():
    import __graft_entry__ as ge
    ge.build()
    from ipc_amd import capi
    lib = capi.load()
    for name in ONLINE:
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    # the report struct is eight ints, in the header's order
    assert [f for f, _ in capi.OnlineReport._fields_] == ["covered_before", "covered_after", "cells", "long_cells",
                                                          "literal_cells", "damped_cells", "set_max_resumed", "grew"]
    assert ctypes.sizeof(capi.OnlineReport) == 32
    # NULL handle => -1 (IPC_ERR_ARG) + message, no crash, no GPU needed; outputs stay untouched
    rep = capi.OnlineReport(7, 7, 7, 7, 7, 7, 7, 7)
    assert lib.ipc_run_online(None, None, None, ctypes.byref(rep)) == -1
    assert b"NULL handle" in lib.ipc_last_error()
    assert rep.cells == 7 and rep.covered_after == 7
    m = ctypes.c_int(5)
    assert lib.ipc_online_covered(None, ctypes.byref(m)) == -1
    assert b"NULL" in lib.ipc_last_error()
    assert m.value == 5
    assert lib.ipc_online_reset(None) == -1
    assert b"NULL handle" in lib.ipc_last_error()
    assert lib.ipc_reserve_candidates(None, 100) == -1
    assert b"NULL handle" in lib.ipc_last_error()


def test_python_surface():
    from ipc_amd.consensus import IPC
    for name in ("run_online", "online_reset", "reserve_candidates"):
        assert callable(getattr(IPC, name)), name
    assert isinstance(IPC.online_covered, property)


def _graphs():
    from ipc_amd import synth
    from ipc_amd.consensus import Config
    return [(synth.inject_outliers(synth.small_se2(), 6, seed=3), Config(s_factor=10.0)),
            (synth.inject_outliers(synth.small_se3(), 5, seed=4), Config(s_factor=50.0, slow_reject_th=6.251))]


def _matrix(O, g, cfg, n):
    return O.consistency_matrix(g.dim, g.odom_meas, g.odom_info, cfg.s_factor, g.loop_ids[:n], g.loop_meas[:n], g.loop_info[:n],
                                cfg.fast_reject_th, cfg.fast_reject_iter_base, cfg.slow_reject_th, cfg.slow_reject_iter_base)


@pytest.mark.parametrize("which", [0, 1], ids=["se2", "se3"])
def test_oracle_prefix_matrix_is_the_leading_block(oracle, which):
    """A cell reads its own two candidates, the chain between them and the parameters: the matrix over the first n candidates
    (file order, as ipc_append_candidate numbers them) is the leading block of the matrix over all -- decisions and max chi2,
    exactly."""
    g, cfg = _graphs()[which]
    ok, mx = _matrix(oracle, g, cfg, g.N)
    assert ok.any() and not ok.all()
    for n in (1, 2, g.N // 3, g.N // 2, g.N - 1):
        okn, mxn = _matrix(oracle, g, cfg, n)
        assert np.array_equal(okn, ok[:n, :n]), n
        assert np.array_equal(mxn, mx[:n, :n], equal_nan=True), n


@pytest.mark.parametrize("which", [0, 1], ids=["se2", "se3"])
def test_oracle_set_max_of_an_order_prefix_is_the_restricted_set(oracle, which):
    """The greedy's verdict on a candidate reads the verdicts in front of it only: over the first n candidates of the processing
    order it accepts what the whole run accepts among them."""
    g, cfg = _graphs()[which]
    ok, _ = _matrix(oracle, g, cfg, g.N)
    order = oracle.candidate_order(g.loop_ids)
    acc = oracle.set_max(ok, order)
    assert 0 < acc.sum() < g.N
    for n in (1, 3, g.N // 2, g.N - 2, g.N):
        members = np.sort(order[:n])                         # the prefix as a candidate list of its own
        local = {int(k): q for q, k in enumerate(members)}
        sub = ok[np.ix_(members, members)]
        sub_order = np.array([local[int(k)] for k in order[:n]], dtype=np.int32)
        assert np.array_equal(oracle.set_max(sub, sub_order), acc[members]), n
