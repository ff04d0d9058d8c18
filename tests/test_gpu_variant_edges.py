"""Every cell-kernel variant of the default policies on inputs aimed at its layout edges (tests/edge_cells.py), one
variant per case (single-token policy, read by make_plan when the engine is created), every solved cell held against
the CPU oracle at the project's parity bar of 1e-5 relative in max chi2."""
import os

import numpy as np
import pytest

import edge_cells as EC

pytestmark = pytest.mark.gpu

REL = 1e-5
POLICY_VARS = ("IPC_SE2_POLICY", "IPC_SE3_POLICY", "IPC_SE3_LATENCY_POLICY")


def _set_policy(monkeypatch, env):
    for var in POLICY_VARS:
        if var in env:
            monkeypatch.setenv(var, env[var])
        else:
            monkeypatch.delenv(var, raising=False)


def _records(eng):
    c = eng.cell_info()
    return c[np.lexsort((c["j"], c["i"]))]


@pytest.mark.parametrize("case", EC.CASES, ids=[c.id for c in EC.CASES])
def test_variant_at_its_layout_edges(oracle, monkeypatch, case):
    from ipc_amd.consensus import IPC, unpack_bits
    O = oracle
    g = EC.case_graph(case)
    cfg = EC.case_config(case)
    tags = g.meta["tags"]
    ci, cj, ref, _ = EC.oracle_cells(case, min(16, os.cpu_count() or 1))
    _set_policy(monkeypatch, case.env)
    eng = IPC(g, cfg, device=0)
    bits, acc = eng.run()
    rep = eng.solve_report()
    cells = _records(eng)
    bits2, acc2 = eng.run()
    cells2 = _records(eng)
    eng.close()
    assert rep["long_cells"] == 0 and rep["failed_cells"] == 0 and rep["nan_cells"] == 0, rep
    # the solved set is the overlap rule on the candidate list (the oracle's cells are listed in the same order)
    assert list(zip(cells["i"].tolist(), cells["j"].tolist())) == list(zip(ci.tolist(), cj.tolist()))
    assert int(((cells["flags"] & 2) != 0).sum()) == 0
    got = cells["max_chi2"]
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-12)
    w = int(np.argmax(err))
    print("%s: %d cells, worst relative chi2 difference %.3g at cell (%s, %s)"
          % (case.id, len(cells), err[w], tags[ci[w]], tags[cj[w]]))
    th = np.where(ci == cj, cfg.fast_reject_th, cfg.slow_reject_th)
    bad = np.nonzero((got > th) != (ref > th))[0]
    assert len(bad) == 0, [(tags[ci[k]], tags[cj[k]], got[k], ref[k]) for k in bad]
    bad = np.nonzero(~(err <= REL))[0]
    assert len(bad) == 0, [(tags[ci[k]], tags[cj[k]], got[k], ref[k]) for k in bad]
    # matrix bits from the oracle's decisions, free (touching, disjoint) pairs = AND of the diagonals; the consensus set
    ok = EC.oracle_matrix(g, cfg, ci, cj, ref)
    assert np.array_equal(unpack_bits(bits, g.N), ok)
    assert np.array_equal(acc, O.set_max(ok, O.candidate_order(g.loop_ids)))
    # two runs of one engine: bit-identical records
    assert np.array_equal(bits, bits2) and np.array_equal(acc, acc2)
    for f in ("i", "j", "max_chi2", "iterations", "evals", "flags"):
        assert np.array_equal(cells[f], cells2[f]), f


def _boundary_graph(dim, cap):
    """Two candidates (0, cap) and (0, cap + 1): diagonal cells of L == cap and L == cap + 1 (and their pair cell)."""
    g = EC.edge_graph(dim, 1, (cap + 64) // 64, "lane" if dim == 2 else "slot", 0, 3)
    from ipc_amd.graphio import PoseGraph
    ids = np.array([[0, cap], [0, cap + 1]], dtype=np.int32)
    meas = np.stack([_rel_meas(dim, g, 0, cap), _rel_meas(dim, g, 0, cap + 1)])
    info = np.ascontiguousarray(g.loop_info[:2])
    return PoseGraph(dim, g.vertices, g.odom_meas, g.odom_info, ids, meas, info, {})


def _rel_meas(dim, g, a, b):
    """The measurement the odometry itself implies between vertices a and b, moved by a few centimetres."""
    from oracle import oracle as O
    from ipc_amd import synth
    poses = O.propagate(dim, g.odom_meas)
    if dim == 2:
        r = O.pose_mul(2, O.pose_inv(2, poses[a]), poses[b])
        return np.asarray(r[:3], dtype=np.float64) + np.array([0.05, -0.03, 0.01])
    Ra, ta = poses[a][:9].reshape(3, 3), poses[a][9:]
    Rb, tb = poses[b][:9].reshape(3, 3), poses[b][9:]
    return np.concatenate([Ra.T @ (tb - ta) + np.array([0.05, -0.03, 0.02]), synth._R_to_quat(Ra.T @ Rb)])


@pytest.mark.parametrize("dim,cap,tok_at,tok_above", [(2, 832, "w13", "p7"), (3, 512, "w8", "g3")])
def test_planner_boundary_between_two_bins(oracle, monkeypatch, dim, cap, tok_at, tok_above):
    """Default policy: a cell with L == cap stays in the bin of that capacity, one with L == cap + 1 goes to the next.  Each
    is bit-identical to the same cell under the single-token policy of its variant, and matches the oracle."""
    from ipc_amd.consensus import IPC, Config
    O = oracle
    g = _boundary_graph(dim, cap)
    cfg = Config() if dim == 2 else Config(s_factor=50.0, slow_reject_th=6.251)
    pvar = "IPC_SE2_POLICY" if dim == 2 else "IPC_SE3_POLICY"
    res = {}
    for name, env in (("default", {}), (tok_at, {pvar: tok_at, "IPC_SE3_LATENCY_POLICY": "none"}),
                      (tok_above, {pvar: tok_above, "IPC_SE3_LATENCY_POLICY": "none"})):
        _set_policy(monkeypatch, env)
        # (the smaller variant alone cannot hold the longer cells: it gets the L == cap candidate only)
        eng = IPC(g.subset([0]) if name == tok_at else g, cfg, device=0)
        eng.run()
        res[name] = (_records(eng), eng.solve_report())
        eng.close()
    d, rep = res["default"]
    assert rep["long_cells"] == 0 and rep["failed_cells"] == 0 and rep["nan_cells"] == 0
    assert list(zip(d["i"].tolist(), d["j"].tolist())) == [(0, 0), (0, 1), (1, 1)]
    assert list(d["hi"] - d["lo"]) == [cap, cap + 1, cap + 1]
    assert res[tok_at][1]["long_cells"] == 0 and res[tok_above][1]["long_cells"] == 0
    assert d["max_chi2"][0] == res[tok_at][0]["max_chi2"][0]
    assert d["max_chi2"][1] == res[tok_above][0]["max_chi2"][1] and d["max_chi2"][2] == res[tok_above][0]["max_chi2"][2]
    poses = O.propagate(dim, g.odom_meas)
    ref, _, _ = O.pair_cells_mt(dim, g.odom_meas, g.odom_info, cfg.s_factor, poses, g.loop_ids, g.loop_meas, g.loop_info,
                                d["i"], d["j"], cfg.fast_reject_iter_base, cfg.slow_reject_iter_base, 3)
    err = np.abs(d["max_chi2"] - ref) / np.maximum(np.abs(ref), 1e-12)
    print("planner boundary dim %d: relative chi2 differences %s" % (dim, err))
    th = np.array([cfg.fast_reject_th, cfg.slow_reject_th, cfg.fast_reject_th])
    assert np.array_equal(d["max_chi2"] > th, ref > th)
    assert np.all(err <= REL), (d["max_chi2"], ref)
