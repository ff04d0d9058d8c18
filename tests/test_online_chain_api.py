"""Online mode (ipc_append_odometry / ipc_reserve_vertices / ipc_vertex_count), the parts that need no GPU: the C ABI exports
and binds the three symbols and reports argument errors, and -- on the CPU oracle -- the premise of the feature: running
agreementCheck on the graph as far as it is known gives what the run on the whole graph gives."""
import numpy as np
import pytest


def test_online_symbols_exported_and_argument_errors_reported():
    import __graft_entry__ as ge
    ge.build()
    from ipc_amd import capi
    lib = capi.load()
    for name in ("ipc_append_odometry", "ipc_reserve_vertices", "ipc_vertex_count"):
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    z = np.zeros(21)
    p = z.ctypes.data
    # NULL handle / NULL arrays / n_edges < 1 => -1 (IPC_ERR_ARG) + message, no crash, no GPU needed
    assert lib.ipc_append_odometry(None, 1, p, p) == -1
    assert b"NULL handle" in lib.ipc_last_error()
    assert lib.ipc_append_odometry(None, 0, p, p) == -1
    assert b"n_edges" in lib.ipc_last_error()
    assert lib.ipc_append_odometry(None, -3, None, None) == -1
    assert b"n_edges" in lib.ipc_last_error()
    assert lib.ipc_reserve_vertices(None, 100) == -1
    assert b"NULL handle" in lib.ipc_last_error()
    import ctypes
    n = ctypes.c_int(7)
    assert lib.ipc_vertex_count(None, ctypes.byref(n)) == -1
    assert b"NULL" in lib.ipc_last_error()
    assert n.value == 7


def _whole_and_online(O, g, cfg, cuts):
    """Records (decision, lo, hi, cluster, max_chi2) per candidate: of the oracle's run on the whole graph, and of its run on the
    graph truncated to the first Vc vertices for every Vc of `cuts` in turn -- a NEW oracle object per cut, which knows the chain
    up to vertex Vc - 1 and the candidates that end there, and takes over poses and consensus set of the one before."""
    dim = g.dim
    args = (cfg.s_factor, cfg.fast_reject_th, cfg.fast_reject_iter_base, cfg.slow_reject_th, cfg.slow_reject_iter_base)
    order = [int(k) for k in O.candidate_order(g.loop_ids)]
    hi = g.loop_ids.max(axis=1)
    whole = O.IncrementalIPC(dim, g.odom_meas, g.odom_info, *args, g.loop_ids, g.loop_meas, g.loop_info)
    ref = {k: whole.agreement_check(k) for k in order}
    got, poses, cns = {}, None, []
    assert cuts[-1] == g.V and sorted(cuts) == list(cuts)
    for Vc in cuts:
        sel = [k for k in range(g.N) if hi[k] < Vc]
        loc = {k: j for j, k in enumerate(sel)}
        inc = O.IncrementalIPC(dim, g.odom_meas[:Vc - 1], g.odom_info[:Vc - 1], *args,
                               g.loop_ids[sel].reshape(-1, 2), g.loop_meas[sel], g.loop_info[sel])
        if poses is not None:
            # the vertices met since: pure odometry on top of the last pose, composed pose by pose (propagateCurrentGuess,
            # reference src/consensus_utils.cpp:61-71; oracle/ipc_oracle.c does its tail with the same two calls)
            ext = np.zeros((Vc, poses.shape[1]))
            ext[:poses.shape[0]] = poses
            for i in range(poses.shape[0], Vc):
                ext[i] = O.pose_mul(dim, ext[i - 1], O.meas_to_pose(dim, g.odom_meas[i - 1]))
            inc.set_state(ext, [loc[k] for k in cns])
        for k in order:
            if k in loc and k not in got:
                got[k] = inc.agreement_check(loc[k])
        poses, cns = inc.poses(), [sel[j] for j in inc.consensus()]
    return order, ref, got, (whole.consensus(), cns), (whole.poses(), poses)


def _assert_same(order, ref, got, sets, poses):
    assert sorted(got) == sorted(order)
    for k in order:
        (ok_r, r), (ok_g, q) = ref[k], got[k]
        assert ok_g == ok_r, (k, r, q)
        assert (q["lo"], q["hi"], q["cluster"]) == (r["lo"], r["hi"], r["cluster"]), (k, r, q)
        assert q["max_chi2"] == r["max_chi2"], (k, r, q)           # exact: the oracle's tail is composed pose by pose
    assert list(sets[0]) == list(sets[1])
    assert np.array_equal(poses[0], poses[1])


def test_oracle_online_equals_batch_se2(oracle):
    """The premise of the online mode in the reference's own semantics, SE2: agreementCheck only reads vertices <= hi and
    re-propagates the tail, so the truncated runs and the whole run are the same algorithm -- equal decisions, (lo, hi,
    cluster), max_chi2 (exact), consensus set and final poses."""
    from ipc_amd import synth
    from ipc_amd.consensus import Config
    g = synth.inject_outliers(synth.small_se2(), 6, seed=3)
    cfg = Config(s_factor=10.0)
    cuts = [12, 25, 33, 47, 54, g.V]
    _assert_same(*_whole_and_online(oracle, g, cfg, cuts))


def test_oracle_online_equals_batch_se3(oracle):
    """The same for SE3."""
    from ipc_amd import synth
    from ipc_amd.consensus import Config
    g = synth.inject_outliers(synth.small_se3(), 5, seed=4)
    cfg = Config(s_factor=50.0, slow_reject_th=6.251)
    cuts = [9, 18, 26, 31, 37, g.V]
    _assert_same(*_whole_and_online(oracle, g, cfg, cuts))
