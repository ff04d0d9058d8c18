"""The exact set in online matrix mode (ipc_run_online_exact) measured on a bench workload.

  --mode stream        the whole chain is there; the candidates are appended in processing order, --burst of them per update
                       (ipc_append_candidate x burst + ipc_run_online_exact, which returns with the proven set on the host).
                       Per update: host wall clock of those calls, cells, newcomer roots searched, steps, whether the set
                       changed; with --force-whole every update is a whole search over the stored matrix
                       (IPC_ONLINE_EXACT_RESUME=0 -- for information only).  One JSON line.
  --mode append_exact  the only route to the same answer before ipc_run_online_exact: ipc_append_candidate + ipc_run_exact, which
                       solves every cell and searches the whole graph again.  Timed at --samples list lengths spread over the run
                       (a quarter of them among the last 100 candidates), as tools/online_matrix_bench.py --mode append_run does.
                       Uses nothing newer than ipc_run_exact, so with --root it measures the parent commit with this very script.
  --mode compare       the two modes above in fresh child processes, alternating (parent, this, ...: --rounds pairs), then one
                       stream in bursts of 50 and one forced to whole searches; medians and spreads to --out.  The orchestrating
                       process never opens the GPU.

Usage: python tools/online_exact_bench.py --mode compare --workload C2 --parent-root DIR --out profiles/online_exact_C2.json"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from online_matrix_bench import TAIL, _env, _stats, _which, _workload, sample_positions


def stream(a):
    if a.force_whole:
        os.environ["IPC_ONLINE_EXACT_RESUME"] = "0"                    # read at ipc_create: the held set is never resumed from
    g, cfg, empty, ids, meas, info = _workload(a)
    from ipc_amd import capi
    from ipc_amd.consensus import IPC
    eng = IPC(empty, cfg)
    lib, N = eng.lib, ids.shape[0]
    acc = np.zeros(N, dtype=np.uint8)
    on, rep, k = capi.OnlineReport(), capi.ExactResumeReport(), C.c_int(0)
    rows, sizes = [], []
    t_all = time.perf_counter()
    for n0 in range(0, N, a.burst):
        n1 = min(N, n0 + a.burst)
        t0 = time.perf_counter()
        rc = 0
        for n in range(n0, n1):
            rc = rc or lib.ipc_append_candidate(eng.h, ids[n].ctypes.data, meas[n].ctypes.data, info[n].ctypes.data, C.byref(k))
        rc = rc or lib.ipc_run_online_exact(eng.h, None, acc.ctypes.data, None, C.byref(on), C.byref(rep))
        dt = time.perf_counter() - t0
        capi.check(rc)
        assert rep.first == (0 if a.force_whole else n0)
        rows.append(dict(n=n1, ms=1e3 * dt, cells=on.cells, newcomers=rep.newcomers, roots=rep.subproblems, steps=int(rep.steps),
                         changed=rep.changed, proven=rep.proven, size=rep.size))
        sizes.append(rep.size)
    total_s = time.perf_counter() - t_all
    lat = np.array([r["ms"] for r in rows])
    tail = np.array([r["ms"] for r in rows if r["n"] > N - TAIL])
    roots, steps = np.array([r["roots"] for r in rows]), np.array([r["steps"] for r in rows])
    out = dict(mode="stream", workload=a.workload, V=int(g.V), N=int(N), burst=a.burst, forced_whole_search=bool(a.force_whole),
               checkout=_which(a.root), updates=len(rows), update=_stats(lat), loop_s=total_s,
               roots_per_update=dict(median=float(np.median(roots)), max=int(roots.max()), total=int(roots.sum()),
                                     updates_with_a_search=int((roots > 0).sum())),
               steps_per_update=dict(median=float(np.median(steps)), max=int(steps.max()), total=int(steps.sum())),
               set_changed=int(sum(r["changed"] for r in rows)), unproven_updates=int(sum(1 - r["proven"] for r in rows)),
               sizes_never_shrink=bool(all(b >= a_ for a_, b in zip(sizes, sizes[1:]))),
               final=dict(size=int(rep.size), proven=int(rep.proven), multistart_size=int(rep.multistart_size), accepted=int(acc.sum())))
    out["update_last_%d" % TAIL] = _stats(tail)
    if not a.force_whole:
        out["slowest_updates"] = sorted(rows, key=lambda r: -r["ms"])[:5]
    out["env"] = _env()
    eng.close()
    return out


def append_exact(a):
    g, cfg, empty, ids, meas, info = _workload(a)
    from ipc_amd import capi
    from ipc_amd.consensus import IPC
    eng = IPC(empty, cfg)
    lib, N = eng.lib, ids.shape[0]
    acc = np.zeros(N, dtype=np.uint8)
    rep, k = capi.ExactReport(), C.c_int(0)
    rows = []
    for n in sample_positions(N, a.samples):
        eng.set_candidates(ids[:n - 1], meas[:n - 1], info[:n - 1])
        capi.check(lib.ipc_run_exact(eng.h, None, acc.ctypes.data, None, C.byref(rep)))     # the state a caller is in when candidate n arrives
        t0 = time.perf_counter()
        rc = lib.ipc_append_candidate(eng.h, ids[n - 1].ctypes.data, meas[n - 1].ctypes.data, info[n - 1].ctypes.data, C.byref(k))
        rc = rc or lib.ipc_run_exact(eng.h, None, acc.ctypes.data, None, C.byref(rep))
        dt = time.perf_counter() - t0
        capi.check(rc)
        rows.append(dict(n=n, ms=1e3 * dt, size=rep.size, proven=rep.proven, steps=int(rep.steps)))
    tail = [r["ms"] for r in rows if r["n"] > N - TAIL]
    out = dict(mode="append_exact", workload=a.workload, N=int(N), checkout=_which(a.root), samples=rows,
               final=dict(size=int(rep.size), proven=int(rep.proven)))
    out["append_exact_last_%d" % TAIL] = _stats(tail)
    out["append_exact_all"] = _stats([r["ms"] for r in rows])
    out["env"] = _env()
    eng.close()
    return out


def compare(a):
    def child(mode, root, extra=()):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--workload", a.workload, "--root", root,
               "--samples", str(a.samples)] + list(extra)
        txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=a.child_timeout).stdout.decode()
        return json.loads([ln for ln in txt.splitlines() if ln.startswith("{")][-1])
    key_s, key_p = "update_last_%d" % TAIL, "append_exact_last_%d" % TAIL
    parents, streams = [], []
    for _ in range(a.rounds):                                          # alternating, every run in a fresh process
        parents.append(child("append_exact", a.parent_root))
        streams.append(child("stream", a.root))
    assert all(p["final"]["size"] == s["final"]["size"] and p["final"]["proven"] == s["final"]["proven"] == 1
               for p, s in zip(parents, streams))
    # the same list lengths: the stream's updates at the parent's sample positions
    at = [r["n"] for r in parents[0]["samples"]]
    pm = [p[key_p]["median_ms"] for p in parents]
    sm = [s[key_s]["median_ms"] for s in streams]
    bursts = child("stream", a.root, ["--burst", "50"])
    whole = child("stream", a.root, ["--force-whole"])
    for s in streams:
        s.pop("slowest_updates", None)
    out = dict(mode="compare", workload=a.workload, rounds=a.rounds, tail=TAIL, parent_sample_lengths=at,
               online_exact_update_median_ms_last_100=float(np.median(sm)), online_exact_update_median_ms_runs=sm,
               online_exact_update_median_ms_all_updates_runs=[s["update"]["median_ms"] for s in streams],
               parent_append_plus_run_exact_median_ms_last_100=float(np.median(pm)), parent_append_plus_run_exact_median_ms_runs=pm,
               ratio=float(np.median(pm) / np.median(sm)), ratio_runs=[p / s for p, s in zip(pm, sm)],
               spread=dict(online_exact=float((max(sm) - min(sm)) / np.median(sm)), parent=float((max(pm) - min(pm)) / np.median(pm))),
               stream=streams[-1], parent=parents[-1], stream_bursts_of_50=bursts, stream_forced_whole_search=whole, env=_env())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["stream", "append_exact", "compare"])
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--root", default=HERE, help="checkout whose ipc_amd package, library and bench.py are measured (default: this one)")
    ap.add_argument("--parent-root", default=None, help="compare: the checkout measured with --mode append_exact")
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--burst", type=int, default=1)
    ap.add_argument("--force-whole", action="store_true", help="stream: every update a whole search (information only)")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "compare" and not a.parent_root:
        ap.error("--mode compare needs --parent-root")
    out = {"stream": stream, "append_exact": append_exact, "compare": compare}[a.mode](a)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
