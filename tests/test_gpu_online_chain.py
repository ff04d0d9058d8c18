"""Online mode on the GPU: an engine grown pose by pose (ipc_append_odometry) must hold, BIT FOR BIT, what an engine that was
given the whole chain holds -- open-loop poses, every ipc_check_info_t of the faithful loop, consensus set, current poses,
the matrix mode's bits and the final map.  No tolerances: the tail of an accept is one rigid transform D applied to the
open-loop poses, a vertex appended later gets the same D; a tolerance would hide a stale D or a mis-strided field.

"batch"  = ipc_create with the whole chain + ipc_set_candidates, checks in ipc_candidate_order.
"online" = ipc_create with the first 2 vertices, one ipc_append_odometry per pose, every candidate appended
           (ipc_append_candidate) once its later vertex exists, ties in file order, and checked in that order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-5      # chi2 tolerance (relative) against the CPU oracle, as tests/test_gpu_incremental.py


def _cfg(dim):
    from ipc_amd.consensus import Config
    return Config(s_factor=10.0) if dim == 2 else Config(s_factor=50.0, slow_reject_th=6.251)


def _se2_graph():
    from ipc_amd import synth                      # the 3-lap graph of test_incremental_medium_clusters
    return synth.inject_outliers(synth._se2_graph(400, 24, seed=75, laps=3.0, name="inc"), 16, seed=5)


def _se3_graph():
    from ipc_amd import synth                      # the small sphere of test_incremental_se3_clusters
    g = synth.sphere_like(rings=8, per_ring=16, radius=8.0)
    keep = np.arange(0, g.N, max(1, g.N // 24))
    return synth.inject_outliers(g.subset(keep), 8, seed=6)


def _graph(dim):
    return _se2_graph() if dim == 2 else _se3_graph()


def _stub(g, V=2, sel=()):
    """The graph as far as its first V vertices, with the candidates `sel`."""
    from ipc_amd.graphio import PoseGraph
    sel = np.asarray(sel, dtype=np.int64)
    return PoseGraph(g.dim, g.vertices[:V], g.odom_meas[:V - 1], g.odom_info[:V - 1],
                     g.loop_ids[sel].reshape(-1, 2), g.loop_meas[sel], g.loop_info[sel], dict(g.meta))


def _engine(g, cfg):
    from ipc_amd.consensus import IPC
    return IPC(g, cfg, device=0)


def _batch(g, cfg):
    eng = _engine(g, cfg)
    eng.reset()
    recs = {}
    for k in eng.candidate_order():
        ok, info = eng.agreementCheck(int(k), with_info=True)
        recs[int(k)] = (ok, bytes(info))
    return eng, recs


def _online(g, cfg, reserve=None, lag=0, chunk=1):
    """Grows an engine from 2 vertices.  chunk poses are appended at a time (chunk == 1: one ipc_append_odometry per pose, else
    one call per burst), then the candidates they complete; checks run in arrival order and stay `lag` candidates behind the
    appends (lag > 0: the look-ahead pipeline has solves in flight and tentative states alive while the chain grows).
    Returns the engine, the records by FILE index and the map file index -> engine index."""
    eng = _engine(_stub(g), cfg)
    if reserve:
        eng.reserve_vertices(reserve)
    hi = g.loop_ids.max(axis=1)
    recs, index, pending = {}, {}, []

    def check(upto):
        while len(pending) > upto:
            k = pending.pop(0)
            ok, info = eng.agreementCheck(index[k], with_info=True)
            recs[k] = (ok, bytes(info))

    v = 2
    while v < g.V:
        n = min(chunk, g.V - v)
        if chunk == 1:
            assert eng.append_odometry(g.odom_meas[v - 1], g.odom_info[v - 1]) == v + 1
        else:
            assert eng.append_odometry(g.odom_meas[v - 1:v - 1 + n], g.odom_info[v - 1:v - 1 + n]) == v + n
        for w in range(v, v + n):
            for k in np.nonzero(hi == w)[0]:                 # file order
                index[int(k)] = eng.append_candidate(g.loop_ids[k], g.loop_meas[k], g.loop_info[k])
                pending.append(int(k))
        v += n
        check(lag)
    check(0)
    assert eng.n_vertices == g.V and eng.N == g.N
    return eng, recs, index


def _growths(V, start=2):
    """How often the arrays grow on the way from `start` to V vertices, one pose at a time (include/ipc_amd.h: the capacity
    doubles, in multiples of 64 vertices)."""
    cap, n = start, 0
    for need in range(start + 1, V + 1):
        if need > cap:
            cap = max(64, (2 * cap + 63) // 64 * 64)
            while cap < need:
                cap *= 2
            n += 1
    return n


def _assert_same_run(g, batch, brecs, eng, recs, index):
    for k in batch.candidate_order():
        k = int(k)
        assert recs[k][0] == brecs[k][0], (k, _fmt(brecs[k][1]), _fmt(recs[k][1]))
        assert recs[k][1] == brecs[k][1], (k, _fmt(brecs[k][1]), _fmt(recs[k][1]))
    back = {j: k for k, j in index.items()}
    assert [back[int(j)] for j in eng.getMaxConsensusSet()] == [int(k) for k in batch.getMaxConsensusSet()]
    assert eng.initial_poses().tobytes() == batch.initial_poses().tobytes()
    assert eng.current_poses().tobytes() == batch.current_poses().tobytes()


def _fmt(raw):
    from ipc_amd import capi
    info = capi.CheckInfo.from_buffer_copy(raw)
    return {f: getattr(info, f) for f, _ in capi.CheckInfo._fields_}


@pytest.fixture(scope="module", params=[2, 3], ids=["se2", "se3"])
def problem(request):
    g = _graph(request.param)
    cfg = _cfg(request.param)
    batch, brecs = _batch(g, cfg)
    assert any(ok for ok, _ in brecs.values()) and not all(ok for ok, _ in brecs.values())
    return g, cfg, batch, brecs


def test_online_run_is_bitwise_the_batch_run(problem):
    """Pose by pose, candidate by candidate: every record (agrees, lo, hi, n_cluster_loops, iterations, tries, flags, max_chi2,
    chi2_total, chi2_initial -- raw bytes), the consensus set, ipc_initial_poses and ipc_current_poses."""
    g, cfg, batch, brecs = problem
    eng, recs, index = _online(g, cfg)
    _assert_same_run(g, batch, brecs, eng, recs, index)


@pytest.mark.parametrize("reserve", [False, True], ids=["growing", "reserved"])
def test_online_run_with_solves_in_flight(problem, reserve):
    """The checks stay 6 candidates behind the appends, so the chain grows -- within the capacity and, without
    ipc_reserve_vertices, through several doublings -- while the pipeline has solves in flight and tentative states alive."""
    g, cfg, batch, brecs = problem
    eng, recs, index = _online(g, cfg, reserve=g.V if reserve else None, lag=6)
    if not reserve and g.dim == 2:
        assert _growths(g.V) >= 3 and eng.n_vertices == g.V          # 2 -> 64 -> 128 -> 256 -> 512
    _assert_same_run(g, batch, brecs, eng, recs, index)


def test_bursts_of_poses_and_their_candidates(problem):
    """Poses in bursts of 50 (one ipc_append_odometry per burst), the candidates of a burst appended together, then checked."""
    g, cfg, batch, brecs = problem
    eng, recs, index = _online(g, cfg, chunk=50)
    _assert_same_run(g, batch, brecs, eng, recs, index)


@pytest.mark.parametrize("dim", [2, 3])
def test_burst_sizes_give_the_open_loop_poses_of_create(dim):
    """Chunks of 1, 7, 64 and all the rest: ipc_initial_poses byte-equal to ipc_create with the whole chain."""
    g, cfg = _graph(dim), _cfg(dim)
    ref = _engine(_stub(g, g.V), cfg).initial_poses()
    eng = _engine(_stub(g), cfg)
    v = 2
    for n in (1, 7, 64, g.V):
        n = min(n, g.V - v)
        assert eng.append_odometry(g.odom_meas[v - 1:v - 1 + n], g.odom_info[v - 1:v - 1 + n]) == v + n
        v += n
        assert eng.initial_poses().tobytes() == ref[:v].tobytes()
    assert v == g.V and eng.n_vertices == g.V


def _grown(g, cfg, V0=2, sel=None, chunk=37):
    """An engine created with V0 vertices, the chain appended in chunks, the candidates `sel` (default: all) set at once."""
    eng = _engine(_stub(g, V0), cfg)
    v = V0
    while v < g.V:
        n = min(chunk, g.V - v)
        eng.append_odometry(g.odom_meas[v - 1:v - 1 + n], g.odom_info[v - 1:v - 1 + n])
        v += n
    sel = np.arange(g.N) if sel is None else np.asarray(sel)
    eng.set_candidates(g.loop_ids[sel], g.loop_meas[sel], g.loop_info[sel])
    return eng


@pytest.mark.parametrize("dim", [2, 3])
def test_matrix_mode_after_growth_and_with_a_cached_plan(dim):
    g, cfg = _graph(dim), _cfg(dim)
    bits_ref, acc_ref = _engine(g, cfg).run()
    eng = _grown(g, cfg)
    bits, acc = eng.run()
    assert bits.tobytes() == bits_ref.tobytes() and acc.tobytes() == acc_ref.tobytes()
    # a cached plan: run on the graph as far as vertex Vc - 1, append the rest and ONE candidate that uses it, run again
    hi = g.loop_ids.max(axis=1)
    late = int(np.argmax(hi))
    Vc = int(np.sort(hi)[len(hi) // 2]) + 1
    early = [k for k in range(g.N) if hi[k] < Vc]
    assert 2 < len(early) < g.N and hi[late] >= Vc
    part = _engine(_stub(g, Vc, early), cfg)
    b0, a0 = part.run()
    fresh0 = _engine(_stub(g, Vc, early), cfg).run()
    assert b0.tobytes() == fresh0[0].tobytes()
    v = Vc
    while v < g.V:
        n = min(29, g.V - v)
        part.append_odometry(g.odom_meas[v - 1:v - 1 + n], g.odom_info[v - 1:v - 1 + n])
        v += n
    b1, a1 = part.run()                                   # the chain alone changes no cell
    assert b1.tobytes() == b0.tobytes() and a1.tobytes() == a0.tobytes()
    part.append_candidate(g.loop_ids[late], g.loop_meas[late], g.loop_info[late])
    b2, a2 = part.run()
    bf, af = _engine(_stub(g, g.V, early + [late]), cfg).run()
    assert b2.tobytes() == bf.tobytes() and a2.tobytes() == af.tobytes()


@pytest.mark.parametrize("dim", [2, 3])
def test_final_optimize_on_a_grown_engine(dim):
    g, cfg = _graph(dim), _cfg(dim)
    batch = _engine(g, cfg)
    _, acc = batch.run()
    assert acc.sum() >= 3
    poses_ref, info_ref = batch.final_optimize(acc, iterations=100)
    eng = _grown(g, cfg)
    poses, info = eng.final_optimize(acc, iterations=100)
    assert (info.chi2_total, info.max_chi2, info.iterations) == (info_ref.chi2_total, info_ref.max_chi2, info_ref.iterations)
    assert poses.tobytes() == poses_ref.tobytes()
    # ... and with the final map's own chain records already there when the chain grows
    g2 = _stub(g, g.V - 40, [k for k in range(g.N) if g.loop_ids[k].max() < g.V - 40])
    part = _engine(g2, cfg)
    part.final_optimize(np.ones(part.N, dtype=np.uint8), iterations=3)
    part.append_odometry(g.odom_meas[g2.V - 1:], g.odom_info[g2.V - 1:])
    part.set_candidates(g.loop_ids, g.loop_meas, g.loop_info)
    poses2, info2 = part.final_optimize(acc, iterations=100)
    assert (info2.chi2_total, info2.max_chi2) == (info_ref.chi2_total, info_ref.max_chi2)
    assert poses2.tobytes() == poses_ref.tobytes()


def test_online_run_against_the_oracle(oracle):
    """The new path held against the CPU oracle directly, not only against the engine's other path."""
    from ipc_amd import synth
    g = synth.inject_outliers(synth.small_se2(), 6, seed=3)
    cfg = _cfg(2)
    inc = oracle.IncrementalIPC(2, g.odom_meas, g.odom_info, cfg.s_factor, cfg.fast_reject_th, cfg.fast_reject_iter_base,
                                cfg.slow_reject_th, cfg.slow_reject_iter_base, g.loop_ids, g.loop_meas, g.loop_info)
    from ipc_amd import capi
    eng, recs, index = _online(g, cfg, lag=2)
    for k in oracle.candidate_order(g.loop_ids):
        ok_ref, ref = inc.agreement_check(int(k))
        ok, info = recs[int(k)][0], capi.CheckInfo.from_buffer_copy(recs[int(k)][1])
        assert (info.lo, info.hi, info.n_cluster_loops) == (ref["lo"], ref["hi"], ref["cluster"]), (k, ref)
        assert ok == ok_ref, (k, ref, info.max_chi2)
        assert abs(info.max_chi2 - ref["max_chi2"]) <= REL * max(abs(ref["max_chi2"]), 1e-12), (k, ref, info.max_chi2)
    back = {j: k for k, j in index.items()}
    assert [back[int(j)] for j in eng.getMaxConsensusSet()] == [int(k) for k in inc.consensus()]
    ref_poses, got = inc.poses(), eng.current_poses()
    assert np.allclose(got[:, :2], ref_poses[:, :2], rtol=0, atol=1e-6)
    assert np.abs(np.angle(np.exp(1j * (got[:, 2] - ref_poses[:, 2])))).max() <= 1e-7


@pytest.mark.parametrize("dim", [2, 3])
def test_contract_edges(dim):
    from ipc_amd import capi
    g, cfg = _graph(dim), _cfg(dim)
    hi = g.loop_ids.max(axis=1)
    k = int(np.argmin(hi))
    V0 = int(hi[k])                                          # the candidate's later vertex is vertex V0: the first one missing
    eng = _engine(_stub(g, V0), cfg)
    assert eng.n_vertices == V0
    with pytest.raises(capi.IpcError, match="outside"):
        eng.append_candidate(g.loop_ids[k], g.loop_meas[k], g.loop_info[k])
    assert eng.append_odometry(g.odom_meas[V0 - 1], g.odom_info[V0 - 1]) == V0 + 1
    j = eng.append_candidate(g.loop_ids[k], g.loop_meas[k], g.loop_info[k])
    assert j == 0 and eng.N == 1
    eng.agreementCheck(j)
    # argument errors: status + message, never a throw from the library
    z = np.zeros(21)
    assert eng.lib.ipc_append_odometry(eng.h, 0, z.ctypes.data, z.ctypes.data) == -1
    assert eng.lib.ipc_append_odometry(eng.h, 1, None, z.ctypes.data) == -1
    assert b"NULL" in eng.lib.ipc_last_error()
    assert eng.lib.ipc_reserve_vertices(eng.h, 2 ** 31 - 1) == -1
    assert b"overflow" in eng.lib.ipc_last_error()
    eng.reserve_vertices(3)                                  # below the capacity: a no-op, not an error
    assert eng.n_vertices == V0 + 1
    # reset, then an append: current == open at the new vertex, bitwise
    eng.reset()
    eng.append_odometry(g.odom_meas[V0:V0 + 5], g.odom_info[V0:V0 + 5])
    assert eng.n_vertices == V0 + 6
    cur, init = eng.current_poses(), eng.initial_poses()
    ps = 3 if dim == 2 else 12
    assert cur.shape == (V0 + 6, ps) and cur.tobytes() == init.tobytes()
    # a state of the grown length goes in and comes out
    poses = init.copy()
    poses[:, 0 if dim == 2 else 9] += 0.25
    eng.set_state(poses, [], 0)
    back = eng.current_poses()
    assert back.shape == poses.shape
    assert np.array_equal(back, poses) if dim == 3 else np.allclose(back, poses, rtol=0, atol=1e-12)
    # ... and the vertex appended next continues it rigidly: D = poses[V-1] (+) open[V-1]^-1, here a pure shift
    eng.append_odometry(g.odom_meas[V0 + 5], g.odom_info[V0 + 5])
    cur, init = eng.current_poses(), eng.initial_poses()
    want = init[-1].copy()
    want[0 if dim == 2 else 9] += 0.25
    assert np.allclose(cur[-1], want, rtol=0, atol=1e-9)
    with pytest.raises(AssertionError):                      # (the state of the shorter chain no longer fits)
        eng.set_state(poses, [], 0)
