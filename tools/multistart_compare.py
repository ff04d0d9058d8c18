"""Greedy set (ipc_set_max) against the multi-start set (ipc_set_max_multistart) on a bench workload: the consistency matrix is
solved once (run_multistart), then per set the size and the precision / recall of the reference's harness (the TP / FP / TN / FN
ladder of src/simulation.cpp:70-105, the first `canonic_inliers` loops being the true ones), and what the maximisation costs.

Timing (one process, one engine, the matrix resident on the device): after --warmup untimed calls of each, --rounds rounds that
alternate ipc_set_max and ipc_set_max_multistart on the engine's stream, each call between two HIP events recorded on that
stream and read after a stream synchronise; median, minimum and spread over the rounds are reported.  The cell solve of the same
run is the HIP-event time of the cell kernels of the last solve (ipc_solver_time_ms), the step the wall time of a repeated
run() (host clock around a call that ends in a device synchronise), median over --rounds steps behind one warm-up step.  The
multi-start kernels' time per launch: run the tool under a kernel trace in a run of its own (the names start with k_ms_).

Usage: python tools/multistart_compare.py --workload C2        (writes profiles/multistart_compare_C2.json)"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")   # the host program's job, before HIP initialises (include/ipc_amd.h, "environment")

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def precision_recall(acc, inliers):
    """src/simulation.cpp:70-81 with gt_loops[k].first = (k < canonic_inliers); float division as there (nan for 0 / 0)."""
    acc = np.asarray(acc).astype(bool)
    truth = np.arange(acc.shape[0]) < inliers
    tp, fn = int((truth & acc).sum()), int((truth & ~acc).sum())
    fp, tn = int((~truth & acc).sum()), int((~truth & ~acc).sum())
    prec = tp / (tp + fp) if tp + fp else float("nan")
    rec = tp / (tp + fn) if tp + fn else float("nan")
    return dict(size=int(acc.sum()), tp=tp, fp=fp, tn=tn, fn=fn, precision=prec, recall=rec)


def stats(v):
    v = [float(x) for x in v]
    med = float(np.median(v))
    return dict(median_ms=med, min_ms=min(v), max_ms=max(v), spread=(max(v) - min(v)) / med if med else 0.0, rounds=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", help="a bench.py workload name (C1, C2, C3, ..)")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import bench
    from ipc_amd.consensus import IPC
    from ipc_amd.dist import EngineBackend
    g, cfg, desc = bench.build_workload(a.workload)
    eng = IPC(g, cfg, device=0)
    bits, acc, greedy, sizes, rep = eng.run_multistart(want_bits=True)
    solve_ms, launches = eng.solver_time_ms()
    N = eng.N

    b = EngineBackend(eng)
    t_set, t_ms = [], []
    with b.stream_ctx():
        d_bits = torch.from_numpy(bits.view(np.int64).reshape(-1)).to(b.device)
        d_acc, d_best = b.empty_bytes(N), b.empty_bytes(N)
        d_sizes = torch.empty(N, dtype=torch.int32, device=b.device)
        for r in range(a.warmup + a.rounds):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record(b.stream)
            b.set_max(d_bits, d_acc)
            ev[1].record(b.stream)
            b.set_max_multistart(d_bits, d_best, d_sizes)
            ev[2].record(b.stream)
            b.stream.synchronize()
            if r >= a.warmup:
                t_set.append(ev[0].elapsed_time(ev[1]))
                t_ms.append(ev[1].elapsed_time(ev[2]))
    same = bool(np.array_equal(d_acc.cpu().numpy(), greedy) and np.array_equal(d_best.cpu().numpy(), acc)
                and np.array_equal(d_sizes.cpu().numpy(), sizes))

    eng.run()
    steps = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        eng.run()
        steps.append(1e3 * (time.perf_counter() - t0))
    step_solve_ms, _ = eng.solver_time_ms()
    eng.close()

    s_set, s_ms, s_step = stats(t_set), stats(t_ms), stats(steps)
    out = dict(workload=a.workload, description=desc, V=int(g.V), N=int(N), canonic_inliers=int(cfg.canonic_inliers),
               report=rep, greedy=precision_recall(greedy, cfg.canonic_inliers),
               multistart=precision_recall(acc, cfg.canonic_inliers),
               distinct_sizes=int(len(set(sizes[sizes > 0].tolist()))),
               device_calls_equal_run_multistart=same,
               timing=dict(method="HIP events on the engine's stream around each call, the two calls alternating in one process; "
                                  "%d warm-up rounds, %d timed" % (a.warmup, a.rounds),
                           ipc_set_max=s_set, ipc_set_max_multistart=s_ms,
                           multistart_over_set_max=s_ms["median_ms"] / s_set["median_ms"],
                           cell_solve_ms_first_run=solve_ms, cell_solve_ms_repeated_step=step_solve_ms, solver_launches=launches,
                           step_wall=s_step, multistart_share_of_step=s_ms["median_ms"] / s_step["median_ms"]),
               env=dict(GPU_MAX_HW_QUEUES=os.environ.get("GPU_MAX_HW_QUEUES"),
                        IPC_MULTISTART_REG_WORDS=os.environ.get("IPC_MULTISTART_REG_WORDS")))
    print("%-10s %6s %6s %6s %10s %8s" % ("set", "size", "tp", "fp", "precision", "recall"))
    for name in ("greedy", "multistart"):
        p = out[name]
        print("%-10s %6d %6d %6d %10.4f %8.4f" % (name, p["size"], p["tp"], p["fp"], p["precision"], p["recall"]))
    print("report: " + json.dumps(rep))
    print("ipc_set_max %.3f ms, ipc_set_max_multistart %.3f ms (medians of %d), cell solve %.3f ms, step %.3f ms"
          % (s_set["median_ms"], s_ms["median_ms"], a.rounds, step_solve_ms, s_step["median_ms"]))
    path = a.out or os.path.join(HERE, "profiles", "multistart_compare_%s.json" % a.workload)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
