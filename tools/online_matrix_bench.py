"""Online matrix mode (ipc_run_online) measured on a bench workload.

  --mode stream      the whole chain is there; the candidates are appended in processing order (by later vertex, ties in file
                     order), one ipc_append_candidate + ipc_run_online per candidate.  Per-update latency (host wall clock of
                     the two calls; ipc_run_online returns with the accepted set on the host), cells per update, storage
                     growths, set-max path counts, the sum of cells; at the end three whole solves of the finished list
                     (ipc_online_reset + ipc_run_online) beside ipc_run, alternating.  Every output carries the GPU_MAX_HW_QUEUES
                     its process ran with.  One JSON line; --out writes it to a file as well.
  --mode append_run  what a caller had to do before ipc_run_online: ipc_append_candidate + ipc_run, which solves the whole
                     matrix again.  Timed at --samples list lengths spread over the run (a quarter of them among the last 100
                     candidates): the engine holds the first n - 1 candidates and has run once, then candidate n arrives.  Uses
                     nothing newer than ipc_append_candidate, so with --root it measures another checkout of the project (the
                     parent commit, built in its own directory) with this very script.
  --mode compare     runs the two modes above in fresh child processes, alternating (parent, this, parent, this, ...: --rounds
                     pairs), and writes medians, the ratio over the last 100 candidates and the run-to-run spread to --out.
                     The orchestrating process never opens the GPU.

Usage: python tools/online_matrix_bench.py --mode compare --workload C2 --parent-root DIR --out profiles/r9_online_matrix_c2.json
       python tools/online_matrix_bench.py --mode stream --workload C5 --out profiles/r9_online_matrix_c5.json"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")   # the host program's job, before HIP initialises (include/ipc_amd.h, "environment")

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 100                                          # "the last 100 candidates": where the bar of DESIGN.md 3.2 is taken


def _workload(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import bench
    from ipc_amd.graphio import PoseGraph
    g, cfg, _ = bench.build_workload(a.workload)
    arr = np.argsort(g.loop_ids.max(axis=1), kind="stable")            # arrival order = processing order
    ids = np.ascontiguousarray(g.loop_ids[arr], dtype=np.int32)
    meas = np.ascontiguousarray(g.loop_meas[arr], dtype=np.float64)
    info = np.ascontiguousarray(g.loop_info[arr], dtype=np.float64)
    empty = PoseGraph(g.dim, g.vertices, g.odom_meas, g.odom_info, np.zeros((0, 2), dtype=np.int32),
                      np.zeros((0, meas.shape[1])), np.zeros((0, info.shape[1])))
    return g, cfg, empty, ids, meas, info


def _which(root):
    return "this checkout" if os.path.abspath(root) == HERE else "another checkout (--root)"


def _env():
    """The queue count the HIP runtime of this process was started with: every latency quoted from a profile is tied to it."""
    return dict(GPU_MAX_HW_QUEUES=os.environ.get("GPU_MAX_HW_QUEUES"))


def _stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return dict(median_ms=float(np.median(ms)), p95_ms=float(np.percentile(ms, 95)), max_ms=float(ms.max()), mean_ms=float(ms.mean()))


def stream(a):
    g, cfg, empty, ids, meas, info = _workload(a)
    from ipc_amd import capi
    from ipc_amd.consensus import IPC
    eng = IPC(empty, cfg)
    lib, N = eng.lib, ids.shape[0]
    if a.reserve:
        eng.reserve_candidates(N)
    acc = np.zeros(N, dtype=np.uint8)
    rep, k = capi.OnlineReport(), C.c_int(0)
    lat, cells, grew, resumed = np.zeros(N), np.zeros(N, dtype=np.int64), 0, 0
    t_all = time.perf_counter()
    for n in range(N):
        t0 = time.perf_counter()
        rc = lib.ipc_append_candidate(eng.h, ids[n].ctypes.data, meas[n].ctypes.data, info[n].ctypes.data, C.byref(k))
        rc = rc or lib.ipc_run_online(eng.h, None, acc.ctypes.data, C.byref(rep))
        lat[n] = time.perf_counter() - t0
        capi.check(rc)
        cells[n], grew, resumed = rep.cells, grew + rep.grew, resumed + rep.set_max_resumed
    total_s = time.perf_counter() - t_all
    lat *= 1e3
    most = [int(n) for n in np.argsort(-cells, kind="stable")[:5]]
    out = dict(mode="stream", workload=a.workload, V=int(g.V), N=int(N), reserved=bool(a.reserve), checkout=_which(a.root),
               updates=int(N), update=_stats(lat), loop_s=total_s,
               cells_per_update=dict(median=float(np.median(cells)), p95=float(np.percentile(cells, 95)), max=int(cells.max())),
               updates_with_most_cells=[dict(n=n + 1, cells=int(cells[n]), ms=float(lat[n])) for n in most],
               storage_growths=int(grew), set_max=dict(resumed=int(resumed), rerun=int(N - resumed)), cells_total=int(cells.sum()),
               accepted=int(acc.sum()))
    out["update_last_%d" % TAIL] = _stats(lat[-TAIL:])
    # a whole solve of the finished list (M = 0: k_plan_delta plans every column) beside ipc_run on the same engine, alternating;
    # neither finds a cached plan, each call invalidates the other's
    whole = dict(run_online_ms=[], run_ms=[])
    for _ in range(3):
        eng.online_reset()
        t0 = time.perf_counter()
        capi.check(lib.ipc_run_online(eng.h, None, acc.ctypes.data, C.byref(rep)))
        whole["run_online_ms"].append(1e3 * (time.perf_counter() - t0))
        assert rep.cells == out["cells_total"] and int(acc.sum()) == out["accepted"]
        t0 = time.perf_counter()
        capi.check(lib.ipc_run(eng.h, None, acc.ctypes.data))
        whole["run_ms"].append(1e3 * (time.perf_counter() - t0))
        assert int(acc.sum()) == out["accepted"]
    out["whole_solve"] = whole
    out["env"] = _env()
    eng.close()
    return out


def sample_positions(N, samples):
    tail = max(2, samples // 4)
    head = np.linspace(max(2, N // samples), N - TAIL - 1, samples - tail).astype(int)
    return sorted(set(int(n) for n in head) | set(int(n) for n in np.linspace(N - TAIL + 1, N, tail).astype(int)))


def append_run(a):
    g, cfg, empty, ids, meas, info = _workload(a)
    from ipc_amd import capi
    from ipc_amd.consensus import IPC
    eng = IPC(empty, cfg)
    lib, N = eng.lib, ids.shape[0]
    acc = np.zeros(N, dtype=np.uint8)
    k = C.c_int(0)
    rows = []
    for n in sample_positions(N, a.samples):
        eng.set_candidates(ids[:n - 1], meas[:n - 1], info[:n - 1])
        capi.check(lib.ipc_run(eng.h, None, acc.ctypes.data))          # the state a caller is in when candidate n arrives
        t0 = time.perf_counter()
        rc = lib.ipc_append_candidate(eng.h, ids[n - 1].ctypes.data, meas[n - 1].ctypes.data, info[n - 1].ctypes.data, C.byref(k))
        rc = rc or lib.ipc_run(eng.h, None, acc.ctypes.data)
        dt = time.perf_counter() - t0
        capi.check(rc)
        rows.append(dict(n=n, ms=1e3 * dt, cells=eng.solve_report()["cells"]))
    tail = [r["ms"] for r in rows if r["n"] > N - TAIL]
    out = dict(mode="append_run", workload=a.workload, N=int(N), checkout=_which(a.root), samples=rows,
               accepted=int(acc.sum()))
    out["append_run_last_%d" % TAIL] = _stats(tail)
    out["env"] = _env()
    eng.close()
    return out


def compare(a):
    def child(mode, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--workload", a.workload, "--root", root,
               "--samples", str(a.samples)] + (["--reserve"] if a.reserve else [])
        txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=a.child_timeout).stdout.decode()
        return json.loads([ln for ln in txt.splitlines() if ln.startswith("{")][-1])
    key_s, key_p = "update_last_%d" % TAIL, "append_run_last_%d" % TAIL
    parents, streams = [], []
    for _ in range(a.rounds):                                          # alternating, every run in a fresh process
        parents.append(child("append_run", a.parent_root))
        streams.append(child("stream", a.root))
    assert all(p["accepted"] == s["accepted"] for p, s in zip(parents, streams))
    pm = [p[key_p]["median_ms"] for p in parents]
    sm = [s[key_s]["median_ms"] for s in streams]
    out = dict(mode="compare", workload=a.workload, rounds=a.rounds, tail=TAIL,
               online_update_median_ms_last_100=float(np.median(sm)), online_update_median_ms_runs=sm,
               parent_append_plus_run_median_ms_last_100=float(np.median(pm)), parent_append_plus_run_median_ms_runs=pm,
               ratio=float(np.median(pm) / np.median(sm)), ratio_runs=[p / s for p, s in zip(pm, sm)],
               spread=dict(online=float((max(sm) - min(sm)) / np.median(sm)), parent=float((max(pm) - min(pm)) / np.median(pm))),
               stream=streams[-1], parent=parents[-1], env=_env())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["stream", "append_run", "compare"])
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--root", default=HERE, help="checkout whose ipc_amd package, library and bench.py are measured (default: this one)")
    ap.add_argument("--parent-root", default=None, help="compare: the checkout measured with --mode append_run")
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reserve", action="store_true", help="stream: ipc_reserve_candidates(N) up front")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "compare" and not a.parent_root:
        ap.error("--mode compare needs --parent-root")
    out = {"stream": stream, "append_run": append_run, "compare": compare}[a.mode](a)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
