"""Online mode (ipc_append_odometry) measured on a bench workload.  One JSON line per run.

  --mode online    the engine starts with 2 vertices; one ipc_append_odometry per pose, every candidate appended
                   (ipc_append_candidate) and checked as soon as its later vertex exists.  Reports candidates/s over the whole
                   loop and the host time of the in-capacity appends (ipc_reserve_vertices up front, so none of them grows).
  --mode upfront   what a caller could do for online use before ipc_append_odometry existed: the whole chain known at
                   ipc_create, one ipc_append_candidate + check per candidate, same arrival order.  Uses nothing newer than
                   ipc_append_candidate, so with --root it measures another checkout of the project (e.g. the parent commit,
                   built in its own directory) with this very script.
  --mode bursts    poses arrive in bursts of --burst (one ipc_append_odometry per burst), the candidates of a burst are appended
                   together and then checked: the look-ahead pipeline works across in-capacity appends.
  --mode batch     ipc_create with the whole chain, ipc_set_candidates, checks in ipc_candidate_order (the README's replay).
  --mode queued    an in-capacity append of ONE edge behind a long batch of queued work on the engine's stream (a burst of
                   --burst edges: its compose is one lane walking the chain): host time of the call against the time
                   ipc_synchronize then still waits.

With IPC_SPEC_STATS=1 in the environment the engine prints the pipeline's launches / results_used / discarded to stderr when
it is destroyed (ipc_destroy), i.e. right after the JSON line.
Usage: python tools/online_bench.py --mode online [--workload C2] [--root DIR]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")   # the host program's job, before HIP initialises (include/ipc_amd.h, "environment")

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["online", "upfront", "bursts", "batch", "queued"])
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout whose ipc_amd package, library and bench.py are measured (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import bench
    from ipc_amd import capi
    from ipc_amd.consensus import IPC
    from ipc_amd.graphio import PoseGraph
    g, cfg, _ = bench.build_workload(a.workload)
    g.odom_meas, g.odom_info = np.ascontiguousarray(g.odom_meas, dtype=np.float64), np.ascontiguousarray(g.odom_info, dtype=np.float64)
    hi = g.loop_ids.max(axis=1)
    arrivals = [np.nonzero(hi == v)[0] for v in range(g.V)]           # candidates by later vertex, file order
    out = dict(mode=a.mode, workload=a.workload, V=int(g.V), N=int(g.N), root=os.path.abspath(a.root))

    def stub(V):
        z = np.zeros((0, g.loop_meas.shape[1])), np.zeros((0, g.loop_info.shape[1]))
        return PoseGraph(g.dim, g.vertices[:V], g.odom_meas[:V - 1], g.odom_info[:V - 1], np.zeros((0, 2), dtype=np.int32), z[0], z[1])

    def warm(eng):
        # allocations, streams, workspaces and the first launches are construction, not the loop (ipc_incremental_prepare)
        eng.lib.ipc_incremental_prepare(eng.h)

    acc = 0
    if a.mode == "batch":
        eng = IPC(g, cfg)
        warm(eng)
        order = eng.candidate_order()
        eng.reset()
        t0 = time.perf_counter()
        for k in order:
            acc += eng.agreementCheck(int(k))
        dt = time.perf_counter() - t0
    elif a.mode == "upfront":
        eng = IPC(stub(g.V), cfg)
        warm(eng)
        t0 = time.perf_counter()
        for v in range(2, g.V):
            for k in arrivals[v]:
                acc += eng.agreementCheck(eng.append_candidate(g.loop_ids[k], g.loop_meas[k], g.loop_info[k]))
        dt = time.perf_counter() - t0
    elif a.mode == "queued":
        eng = IPC(stub(2), cfg)
        eng.reserve_vertices(g.V)
        warm(eng)
        n = min(a.burst, g.V - 3)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.append_odometry(g.odom_meas[1:1 + n], g.odom_info[1:1 + n])
        t1 = time.perf_counter()
        eng.append_odometry(g.odom_meas[1 + n], g.odom_info[1 + n])
        t2 = time.perf_counter()
        eng.synchronize()
        t3 = time.perf_counter()
        out.update(burst_edges=int(n), burst_call_us=1e6 * (t1 - t0), single_append_call_us=1e6 * (t2 - t1),
                   synchronize_after_us=1e6 * (t3 - t2))
        print(json.dumps(out))
        eng.close()
        return
    else:
        chunk = 1 if a.mode == "online" else a.burst
        eng = IPC(stub(2), cfg)
        eng.reserve_vertices(g.V)
        warm(eng)
        app = []
        t0 = time.perf_counter()
        v = 2
        while v < g.V:
            n = min(chunk, g.V - v)
            ta = time.perf_counter()
            rc = eng.lib.ipc_append_odometry(eng.h, n, g.odom_meas[v - 1:v - 1 + n].ctypes.data, g.odom_info[v - 1:v - 1 + n].ctypes.data)
            app.append(time.perf_counter() - ta)
            capi.check(rc)
            ks = [eng.append_candidate(g.loop_ids[k], g.loop_meas[k], g.loop_info[k]) for w in range(v, v + n) for k in arrivals[w]]
            for j in ks:
                acc += eng.agreementCheck(j)
            v += n
        dt = time.perf_counter() - t0
        assert eng.n_vertices == g.V
        app = 1e6 * np.array(app)
        out.update(appends=len(app), append_call_us_median=float(np.median(app)), append_call_us_p90=float(np.percentile(app, 90)),
                   append_call_us_max=float(app.max()), appends_total_s=float(app.sum() * 1e-6), edges_per_append=chunk)
    out.update(loop_s=dt, candidates_per_s=g.N / dt, accepted=int(acc))
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
