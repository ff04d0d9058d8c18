"""Every device buffer, pinned buffer and event the library acquires is released by the time its engine is destroyed
(ipc_debug_live_resources: the owning handles of ipc_amd/csrc/hip_owned.hpp count themselves).  One life of an engine through
every path that allocates, grows or retires -- matrix mode, online matrix, candidate and chain growth, the look-ahead
pipeline of the faithful mode, the final map -- in a FRESH child process per case, so that engines other test modules hold
cannot move the process-wide counters.  The run's bits and accepted set are held against the CPU oracle as smoke() does:
a broken engine does not pass by releasing everything."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_child_failed = []


def _live(lib):
    import ctypes
    out = (ctypes.c_int * 3)()
    assert lib.ipc_debug_live_resources(ctypes.byref(out)) == 0
    return list(out)


def _child(dim):
    sys.path.insert(0, ROOT)
    import numpy as np
    from ipc_amd import capi, synth
    from ipc_amd.consensus import IPC, Config, unpack_bits
    from ipc_amd.graphio import PoseGraph
    from oracle import oracle as O

    if dim == 2:
        g, cfg = synth.inject_outliers(synth.small_se2(), 6, seed=3), Config(s_factor=10.0)
    else:
        g, cfg = synth.inject_outliers(synth.small_se3(), 5, seed=4), Config(s_factor=50.0, slow_reject_th=6.251)
    ok, _ = O.consistency_matrix(dim, g.odom_meas, g.odom_info, cfg.s_factor, g.loop_ids, g.loop_meas, g.loop_info,
                                 cfg.fast_reject_th, cfg.fast_reject_iter_base, cfg.slow_reject_th, cfg.slow_reject_iter_base)
    n0 = g.N - 1                                   # the last candidate (file order) arrives by ipc_append_candidate
    first = PoseGraph(g.dim, g.vertices, g.odom_meas, g.odom_info, g.loop_ids[:n0], g.loop_meas[:n0], g.loop_info[:n0], dict(g.meta))
    ref0 = O.set_max(np.ascontiguousarray(ok[:n0, :n0]), O.candidate_order(first.loop_ids))   # (a cell reads its own two candidates only)
    ref1 = O.set_max(ok, O.candidate_order(g.loop_ids))

    lib = capi.load()
    assert _live(lib) == [0, 0, 0]
    eng = IPC(first, cfg, device=0)                # ipc_create, ipc_set_candidates
    bits, acc = eng.run()
    assert np.array_equal(unpack_bits(bits, n0), ok[:n0, :n0]), "consistency matrix differs from the oracle"
    assert np.array_equal(acc, ref0), "accepted set differs from the oracle"
    acc_on, _ = eng.run_online()
    assert np.array_equal(acc_on, ref0)
    assert eng.append_candidate(g.loop_ids[n0], g.loop_meas[n0], g.loop_info[n0]) == n0
    eng.reserve_candidates(64)
    eng.reserve_candidates(128)                    # crosses the capacity: candidate arrays and online matrix grow, the old ones are retired
    eng.reserve_vertices(g.V + 2)                  # the chain arrays grow (retired as well)
    assert eng.append_odometry(g.odom_meas[-2:], g.odom_info[-2:]) == g.V + 2      # a burst: the pinned staging buffer
    bits_on, acc_on, rep = eng.run_online(want_bits=True)
    assert rep["covered_after"] == g.N
    assert np.array_equal(unpack_bits(bits_on, g.N), ok), "online matrix differs from the oracle"
    assert np.array_equal(acc_on, ref1), "online accepted set differs from the oracle"
    capi.check(lib.ipc_incremental_prepare(eng.h))                                  # the pipeline's slots, states and solvers
    for k in eng.candidate_order()[:3]:
        eng.agreementCheck(int(k))
    poses, _ = eng.final_optimize(acc_on)
    assert np.isfinite(poses).all()
    alive = _live(lib)
    assert all(n > 0 for n in alive), alive       # (the counters are wired, not constants)
    eng.close()
    assert _live(lib) == [0, 0, 0], "an engine's resources outlived it"
    again = IPC(first, cfg, device=0)
    _, acc2 = again.run()
    assert np.array_equal(acc2, ref0)
    assert all(n > 0 for n in _live(lib)[::2])     # (device buffers and events at least)
    again.close()
    assert _live(lib) == [0, 0, 0], "a second engine's resources outlived it"
    print("resource balance OK: dim %d, alive %s" % (dim, alive))


@pytest.mark.parametrize("dim", [2, 3], ids=["se2", "se3"])
def test_engine_releases_everything_it_acquired(dim):
    if _child_failed:
        pytest.fail("not started: the child of case %s ended with status %d" % _child_failed[0])
    user_site = ["-s"] if sys.flags.no_user_site else []
    # (a first import of torch and the load of the code objects included)
    try:
        r = subprocess.run([sys.executable] + user_site + [os.path.abspath(__file__), str(dim)], capture_output=True, text=True,
                           timeout=300, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _child_failed.append((dim, 124))
        raise
    if r.returncode != 0:
        _child_failed.append((dim, r.returncode))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "resource balance OK" in r.stdout


if __name__ == "__main__":
    _child(int(sys.argv[1]))
