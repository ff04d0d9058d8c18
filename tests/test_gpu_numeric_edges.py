"""Every cell-kernel body and the cluster solvers on inputs aimed at the edges of the pose algebra (tests/numeric_edges.py:
all four branches of quat_from_R for poses, gauges and error rotations, error quaternions with q_w -> 0 on both sides
of the sign flip, heading errors next to +-pi, headings that wrap inside a cell), every result held against the CPU
oracle at the project's parity bar of 1e-5 relative in max chi2.  tests/test_numeric_edges_cpu.py holds
the conditions under which a disagreement here is a finding about the kernel: the oracle is right and well conditioned
on every one of these cells."""
import os

import numpy as np
import pytest

import numeric_edges as NE

pytestmark = pytest.mark.gpu

REL = 1e-5
FLOOR = 1e-12
POLICY_VARS = ("IPC_SE2_POLICY", "IPC_SE3_POLICY", "IPC_SE3_LATENCY_POLICY")
CLUSTER_VARS = ("IPC_CLUSTER_MODE", "IPC_BAND_MIN_N")
NTHREADS = min(16, os.cpu_count() or 1)


def _set_env(monkeypatch, names, env):
    for var in names:
        if var in env:
            monkeypatch.setenv(var, str(env[var]))
        else:
            monkeypatch.delenv(var, raising=False)


def _records(eng):
    c = eng.cell_info()
    return c[np.lexsort((c["j"], c["i"]))]


@pytest.mark.parametrize("case", NE.CASES, ids=[c.id for c in NE.CASES])
def test_kernel_body_at_the_edges_of_the_pose_algebra(oracle, monkeypatch, case):
    from ipc_amd.consensus import IPC, unpack_bits
    O = oracle
    g = NE.case_graph(case)
    cfg = NE.config(case.dim)
    tags = g.meta["tags"]
    ci, cj, ref, _ = NE.oracle_cells(case.dim, case.span, NTHREADS)
    _set_env(monkeypatch, POLICY_VARS, case.env)
    eng = IPC(g, cfg, device=0)
    bits, acc = eng.run()
    rep = eng.solve_report()
    cells = _records(eng)
    bits2, acc2 = eng.run()
    cells2 = _records(eng)
    eng.close()
    assert rep["long_cells"] == 0 and rep["failed_cells"] == 0 and rep["nan_cells"] == 0, rep
    # the solved set is the overlap rule on the candidate list (the oracle's cells are listed in the same order)
    assert list(zip(cells["i"].tolist(), cells["j"].tolist())) == NE.expected_cells(g.loop_ids)
    assert list(zip(cells["i"].tolist(), cells["j"].tolist())) == list(zip(ci.tolist(), cj.tolist()))
    assert int(((cells["flags"] & 2) != 0).sum()) == 0
    got = cells["max_chi2"]
    err = np.abs(got - ref) / np.maximum(np.abs(ref), FLOOR)
    w = int(np.argmax(err))
    print("%s: %d cells, worst relative chi2 difference %.3g at cell (%s, %s)"
          % (case.id, len(cells), err[w], tags[ci[w]], tags[cj[w]]))
    th = np.where(ci == cj, cfg.fast_reject_th, cfg.slow_reject_th)
    bad = np.nonzero((got > th) != (ref > th))[0]
    assert len(bad) == 0, [(tags[ci[k]], tags[cj[k]], got[k], ref[k]) for k in bad]
    bad = np.nonzero(~(err <= REL))[0]
    assert len(bad) == 0, [(tags[ci[k]], tags[cj[k]], got[k], ref[k]) for k in bad]
    # matrix bits from the oracle's decisions, free (touching, disjoint) pairs = AND of the diagonals; the consensus set
    ok = NE.oracle_matrix(g, cfg, ci, cj, ref)
    assert np.array_equal(unpack_bits(bits, g.N), ok)
    assert np.array_equal(acc, O.set_max(ok, O.candidate_order(g.loop_ids)))
    # two runs of one engine: bit-identical records
    assert np.array_equal(bits, bits2) and np.array_equal(acc, acc2)
    for f in ("i", "j", "max_chi2", "iterations", "evals", "flags"):
        assert np.array_equal(cells[f], cells2[f]), f


def _faithful(eng, order):
    eng.reset()
    rec = []
    for k in order:
        ok, info = eng.agreementCheck(int(k), with_info=True)
        rec.append((bool(ok), info.lo, info.hi, info.n_cluster_loops, info.iterations, info.tries, info.flags,
                    info.max_chi2, info.chi2_total, info.chi2_initial))
    return rec, np.array(eng.getMaxConsensusSet())


@pytest.mark.parametrize("dim", [2, 3])
def test_cluster_solvers_at_the_edges_of_the_pose_algebra(oracle, monkeypatch, dim):
    """The whole candidate list of the dimension's smallest graph through agreementCheck in candidate order, under the
    device-resident solver, the host-driven one and the banded large-cluster kernel forced onto every cluster."""
    from ipc_amd.consensus import IPC
    O = oracle
    g = NE.numeric_graph(dim, NE.SMALLEST[dim])
    cfg = NE.config(dim)
    tags = g.meta["tags"]
    order = O.candidate_order(g.loop_ids)
    inc = O.IncrementalIPC(dim, g.odom_meas, g.odom_info, cfg.s_factor, cfg.fast_reject_th, cfg.fast_reject_iter_base,
                           cfg.slow_reject_th, cfg.slow_reject_iter_base, g.loop_ids, g.loop_meas, g.loop_info)
    ref = [inc.agreement_check(int(k)) for k in order]
    ref_set = inc.consensus()
    _set_env(monkeypatch, POLICY_VARS, {})
    recs = {}
    for name, env in (("persist", {"IPC_CLUSTER_MODE": "persist"}), ("host", {"IPC_CLUSTER_MODE": "host"}),
                      ("band", {"IPC_BAND_MIN_N": 0})):
        _set_env(monkeypatch, CLUSTER_VARS, env)
        eng = IPC(g, cfg, device=0)
        assert np.array_equal(eng.candidate_order(), order)
        rec, cns = _faithful(eng, order)
        eng.close()
        recs[name] = rec
        worst, at = 0.0, None
        for k, (ok_ref, r), got in zip(order, ref, rec):
            assert (got[0], got[1], got[2], got[3]) == (ok_ref, r["lo"], r["hi"], r["cluster"]), (name, tags[k], got, r)
            assert not (got[6] & 2), (name, tags[k], got)
            e = abs(got[7] - r["max_chi2"]) / max(abs(r["max_chi2"]), FLOOR)
            if e >= worst:
                worst, at = e, tags[k]
            assert e <= REL, (name, tags[k], got[7], r["max_chi2"])
        assert np.array_equal(cns, ref_set), (name, cns, ref_set)
        print("se%d %s: %d checks, worst relative chi2 difference %.3g at %s" % (dim, name, len(order), worst, at))
    for q, (ra, rb) in enumerate(zip(recs["persist"], recs["host"])):
        assert ra[:7] == rb[:7], (q, ra, rb)
        for x, y in zip(ra[7:], rb[7:]):
            assert np.float64(x).tobytes() == np.float64(y).tobytes() or (x != x and y != y), (q, ra, rb)
