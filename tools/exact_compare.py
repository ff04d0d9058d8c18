"""Greedy set (ipc_set_max), multi-start set (ipc_set_max_multistart) and exact set (ipc_set_max_exact) on a bench workload: the
consistency matrix is solved once (run_multistart), then per set the size and the precision / recall of the reference's harness
(the TP / FP / TN / FN ladder of src/simulation.cpp:70-105, the first `canonic_inliers` loops being the true ones), what the
exact call proved (proven, upper_bound, subproblems, capped, steps) and what it costs.

Timing (one process, one engine, the matrix resident on the device): ipc_set_max_exact blocks the host, so a call is timed by the
host clock around it; one untimed call, then --rounds calls; median, minimum and maximum are reported.  Every call must return
the same bytes and the same report.

--census: the census of the maximum sets as well (ipc_set_max_census), on the same engine and matrix: count,
core_size and support_size, precision and recall of the core beside those of the accepted set, and the wall clock of the whole
call, timed in the same way; the census stage is what the call takes beyond ipc_set_max_exact (both medians are reported).

Usage: python tools/exact_compare.py --workload C2        (writes profiles/exact_compare_C2.json)
       python tools/exact_compare.py --workload C2 --census      (writes profiles/census_C2.json)"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")   # the host program's job, before HIP initialises (include/ipc_amd.h, "environment")

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from multistart_compare import precision_recall, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", help="a bench.py workload name (C1, C2, C3, ..)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--census", action="store_true", help="also ipc_set_max_census: count, core, support and its wall clock")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import bench
    from ipc_amd.consensus import IPC
    from ipc_amd.dist import EngineBackend
    g, cfg, desc = bench.build_workload(a.workload)
    eng = IPC(g, cfg, device=0)
    bits, ms, greedy, sizes, ms_rep = eng.run_multistart(want_bits=True)
    N = eng.N

    b = EngineBackend(eng)
    wall, reports, sets = [], [], []
    with b.stream_ctx():
        d_bits = torch.from_numpy(bits.view(np.int64).reshape(-1)).to(b.device)
        d_acc = b.empty_bytes(N)
        b.stream.synchronize()
        for r in range(1 + a.rounds):
            t0 = time.perf_counter()
            rep = b.set_max_exact(d_bits, d_acc)
            if r:
                wall.append(1e3 * (time.perf_counter() - t0))
            reports.append(rep)
            sets.append(d_acc.cpu().numpy().copy())
        census = None
        if a.census:
            d_core, d_support = b.empty_bytes(N), b.empty_bytes(N)
            c_wall, c_reports, c_sets = [], [], []
            for r in range(1 + a.rounds):
                t0 = time.perf_counter()
                ex_rep, cs_rep = b.set_max_census(d_bits, d_acc, d_core, d_support)
                if r:
                    c_wall.append(1e3 * (time.perf_counter() - t0))
                c_reports.append((ex_rep, cs_rep))
                c_sets.append([t.cpu().numpy().copy() for t in (d_acc, d_core, d_support)])
            census = (c_wall, c_reports, c_sets)
    exact = sets[0]
    same = all(r == reports[0] for r in reports) and all(np.array_equal(s, exact) for s in sets)
    mem = np.flatnonzero(exact)
    ok = ((bits[mem][:, mem >> 6] >> (mem & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    eng.close()

    rep = reports[0]
    out = dict(workload=a.workload, description=desc, V=int(g.V), N=int(N), canonic_inliers=int(cfg.canonic_inliers),
               report=rep, multistart_report=ms_rep,
               greedy=precision_recall(greedy, cfg.canonic_inliers), multistart=precision_recall(ms, cfg.canonic_inliers),
               exact=precision_recall(exact, cfg.canonic_inliers),
               exact_set_is_a_clique=bool(ok.all()), exact_equals_multistart=bool(np.array_equal(exact, ms)),
               calls_identical=bool(same),
               timing=dict(method="host clock around the blocking call, one untimed call then %d timed" % a.rounds,
                           ipc_set_max_exact=stats(wall)),
               env=dict(GPU_MAX_HW_QUEUES=os.environ.get("GPU_MAX_HW_QUEUES"), IPC_EXACT_STEP_CAP=os.environ.get("IPC_EXACT_STEP_CAP")))
    names = ("greedy", "multistart", "exact")
    if census:
        c_wall, c_reports, c_sets = census
        ex_rep, cs_rep = c_reports[0]
        acc_c, core, support = c_sets[0]
        c_same = all(r == c_reports[0] for r in c_reports) and all(np.array_equal(x, y) for s in c_sets for x, y in zip(s, c_sets[0]))
        t_exact, t_census = out["timing"]["ipc_set_max_exact"]["median_ms"], stats(c_wall)["median_ms"]
        out.update(census_report=cs_rep, core=precision_recall(core, cfg.canonic_inliers), support=precision_recall(support, cfg.canonic_inliers),
                   ambiguous=[int(k) for k in np.flatnonzero(support & ~core & 1)][:256],
                   census_exact_stage_equals_exact=bool(ex_rep == rep and np.array_equal(acc_c, exact)), census_calls_identical=bool(c_same))
        out["timing"].update(ipc_set_max_census=stats(c_wall), census_stage_median_ms=t_census - t_exact,
                             census_stage_over_exact_stage=(t_census - t_exact) / t_exact if t_exact else float("nan"))
        names += ("core", "support")
    print("%-10s %6s %6s %6s %10s %8s" % ("set", "size", "tp", "fp", "precision", "recall"))
    for name in names:
        p = out[name]
        print("%-10s %6d %6d %6d %10.4f %8.4f" % (name, p["size"], p["tp"], p["fp"], p["precision"], p["recall"]))
    print("report: " + json.dumps(rep))
    print("ipc_set_max_exact %.3f ms (median of %d), identical calls: %s" % (out["timing"]["ipc_set_max_exact"]["median_ms"], a.rounds, same))
    if census:
        print("census: " + json.dumps(out["census_report"]))
        print("ipc_set_max_census %.3f ms (median of %d): the census stage %.3f ms, %.2f of the exact stage; identical calls: %s" % (
            out["timing"]["ipc_set_max_census"]["median_ms"], a.rounds, out["timing"]["census_stage_median_ms"],
            out["timing"]["census_stage_over_exact_stage"], out["census_calls_identical"]))
    path = a.out or os.path.join(HERE, "profiles", "%s_%s.json" % ("census" if census else "exact_compare", a.workload))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
