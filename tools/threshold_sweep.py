"""Threshold sweep (ipc_run_sweep) on a bench workload or a .g2o file: the cells are solved once, the consistent set is
produced for a list of (fast_reject_th, slow_reject_th) pairs, and per pair the accepted count and the precision / recall of the
reference's harness are printed (the TP / FP / TN / FN ladder of src/simulation.cpp:70-105, the first `canonic_inliers` loops
being the true ones), then the sweep's report.

  default pairs   the workload's own pair scaled by 16 log-spaced factors in [1/4, 4]; --pairs "f:s,f:s,..." gives others
  --check         every entry of the sweep against a fresh engine created with that pair, one run() each, bit for bit; the counts
                  of differing words and bytes go to --out (default profiles/sweep_<workload>.json)
  --time          the measurement of DESIGN.md 3.4 in fresh child processes, alternating: (a) a fresh engine's first run() at one
                  pair -- with --parent-root in another checkout of the project (the parent commit, built in its own directory) --,
                  (b) a fresh engine's run_sweep of the default pairs, (c) a second run_sweep of 16 other pairs on that engine.
                  Medians and spreads go to --out.  The orchestrating process never opens the GPU.

Usage: python tools/threshold_sweep.py --workload C2 --check
       python tools/threshold_sweep.py --workload C2 --time --parent-root DIR
       python tools/threshold_sweep.py --g2o FILE --canonic-inliers 256 --s-factor 10"""
import argparse
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")   # the host program's job, before HIP initialises (include/ipc_amd.h, "environment")

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(a):
    sys.path.insert(0, os.path.abspath(a.root))
    if a.g2o:
        from ipc_amd.consensus import Config
        from ipc_amd.graphio import read_g2o
        g = read_g2o(a.g2o)
        cfg = Config(s_factor=a.s_factor if a.s_factor else (10.0 if g.dim == 2 else 50.0), canonic_inliers=a.canonic_inliers)
        return g, cfg, os.path.splitext(os.path.basename(a.g2o))[0]
    import bench
    g, cfg, _ = bench.build_workload(a.workload)
    return g, cfg, a.workload


def default_pairs(cfg, n=16, shift=1.0):
    """The configuration's pair scaled by n log-spaced factors in [1/4, 4] (shift: another grid between the same ends)."""
    k = np.logspace(-2.0, 2.0, n, base=2.0) * shift
    return [(float(cfg.fast_reject_th * f), float(cfg.slow_reject_th * f)) for f in k]


def _pairs(a, cfg):
    if a.pairs:
        return [tuple(float(x) for x in p.split(":")) for p in a.pairs.split(",")]
    return default_pairs(cfg)


def precision_recall(acc, inliers):
    """src/simulation.cpp:70-81 with gt_loops[k].first = (k < canonic_inliers); float division as there (nan for 0 / 0)."""
    acc = np.asarray(acc).astype(bool)
    truth = np.arange(acc.shape[0]) < inliers
    tp, fn = int((truth & acc).sum()), int((truth & ~acc).sum())
    fp, tn = int((~truth & acc).sum()), int((~truth & ~acc).sum())
    prec = tp / (tp + fp) if tp + fp else float("nan")
    rec = tp / (tp + fn) if tp + fn else float("nan")
    return dict(tp=tp, fp=fp, tn=tn, fn=fn, precision=prec, recall=rec)


def _engine(g, cfg, fast=None, slow=None):
    from dataclasses import replace
    from ipc_amd.consensus import IPC
    if fast is not None:
        cfg = replace(cfg, fast_reject_th=fast, slow_reject_th=slow)
    return IPC(g, cfg, device=0)


def sweep(a):
    g, cfg, name = _load(a)
    pairs = _pairs(a, cfg)
    eng = _engine(g, cfg)
    t0 = time.perf_counter()
    bits, acc, rep = eng.run_sweep([p[0] for p in pairs], [p[1] for p in pairs], want_bits=True)
    dt = time.perf_counter() - t0
    eng.close()
    rows = []
    print("%10s %10s %9s %6s %6s %10s %8s" % ("fast_th", "slow_th", "accepted", "tp", "fp", "precision", "recall"))
    for t, (f, s) in enumerate(pairs):
        pr = precision_recall(acc[t], cfg.canonic_inliers)
        rows.append(dict(fast_th=f, slow_th=s, accepted=int(acc[t].sum()), **pr))
        print("%10.4f %10.4f %9d %6d %6d %10.4f %8.4f" % (f, s, rows[-1]["accepted"], pr["tp"], pr["fp"], pr["precision"], pr["recall"]))
    print("report: " + json.dumps(rep))
    out = dict(mode="sweep", workload=name, V=int(g.V), N=int(g.N), canonic_inliers=int(cfg.canonic_inliers), pairs=rows, report=rep,
               sweep_ms=1e3 * dt, env=dict(GPU_MAX_HW_QUEUES=os.environ.get("GPU_MAX_HW_QUEUES")))
    if a.check:
        diff = []
        for t, (f, s) in enumerate(pairs):
            ref = _engine(g, cfg, f, s)
            b_ref, a_ref = ref.run()
            ref.close()
            diff.append(dict(fast_th=f, slow_th=s, differing_words=int((bits[t] != b_ref).sum()),
                             differing_accepted_bytes=int((acc[t] != a_ref).sum())))
        out["check"] = dict(fresh_engines=len(pairs), differing_words=sum(d["differing_words"] for d in diff),
                            differing_accepted_bytes=sum(d["differing_accepted_bytes"] for d in diff), per_pair=diff)
        print("check against %d fresh engines: %d differing words, %d differing accepted bytes"
              % (len(pairs), out["check"]["differing_words"], out["check"]["differing_accepted_bytes"]))
    return out


def time_run(a):
    """(a): the first run() of a fresh engine, nothing cached; uses nothing newer than ipc_run, so --root may be another checkout."""
    g, cfg, name = _load(a)
    t0 = time.perf_counter()
    eng = _engine(g, cfg)
    t1 = time.perf_counter()
    _, acc = eng.run()
    t2 = time.perf_counter()
    eng.close()
    return dict(mode="time_run", workload=name, create_ms=1e3 * (t1 - t0), run_ms=1e3 * (t2 - t1), accepted=int(acc.sum()))


def time_sweep(a):
    """(b) a fresh engine's run_sweep of the default pairs, (c) a second run_sweep of as many other pairs on that engine."""
    g, cfg, name = _load(a)
    first, other = default_pairs(cfg), default_pairs(cfg, shift=2.0 ** (2.0 / 15.0))
    t0 = time.perf_counter()
    eng = _engine(g, cfg)
    t1 = time.perf_counter()
    acc1, rep1 = eng.run_sweep([p[0] for p in first], [p[1] for p in first])
    t2 = time.perf_counter()
    acc2, rep2 = eng.run_sweep([p[0] for p in other], [p[1] for p in other])
    t3 = time.perf_counter()
    eng.close()
    assert rep1["reused_solve"] == 0 and rep2["reused_solve"] == 1
    return dict(mode="time_sweep", workload=name, create_ms=1e3 * (t1 - t0), sweep_ms=1e3 * (t2 - t1), second_sweep_ms=1e3 * (t3 - t2),
                report=rep1, second_report=rep2, accepted=[int(x.sum()) for x in acc1])


def timing(a):
    def child(mode, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--workload", a.workload, "--root", root]
        txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=a.child_timeout).stdout.decode()
        return json.loads([ln for ln in txt.splitlines() if ln.startswith("{")][-1])
    runs, sweeps = [], []
    for _ in range(a.rounds):                                          # alternating, every run in a fresh process
        runs.append(child("time_run", a.parent_root or a.root))
        sweeps.append(child("time_sweep", a.root))
    ra = [r["run_ms"] for r in runs]
    sb, sc = [s["sweep_ms"] for s in sweeps], [s["second_sweep_ms"] for s in sweeps]
    spread = lambda v: float((max(v) - min(v)) / np.median(v))
    med_a, med_b = float(np.median(ra)), float(np.median(sb))
    return dict(mode="time", workload=a.workload, rounds=a.rounds,
                a_first_run_of_a_fresh_engine=dict(checkout="another checkout (--parent-root)" if a.parent_root else "this checkout",
                                                   median_ms=med_a, runs_ms=ra, spread=spread(ra)),
                b_sweep_of_16_pairs=dict(median_ms=med_b, runs_ms=sb, spread=spread(sb)),
                c_second_sweep_of_16_other_pairs=dict(median_ms=float(np.median(sc)), runs_ms=sc, spread=spread(sc)),
                b_over_a=med_b / med_a, bar=1.05 + spread(ra), within_bar=bool(med_b / med_a <= 1.05 + spread(ra)),
                report=sweeps[-1]["report"], second_report=sweeps[-1]["second_report"],
                env=dict(GPU_MAX_HW_QUEUES=os.environ.get("GPU_MAX_HW_QUEUES")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", help="a bench.py workload name")
    ap.add_argument("--g2o", default=None, help="a .g2o file instead of a workload (with --canonic-inliers, --s-factor)")
    ap.add_argument("--canonic-inliers", type=int, default=0)
    ap.add_argument("--s-factor", type=float, default=0.0)
    ap.add_argument("--pairs", default=None, help='"fast:slow,fast:slow,..." instead of the 16 default pairs')
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--mode", default=None, choices=["time_run", "time_sweep"], help="(the children of --time)")
    ap.add_argument("--root", default=HERE, help="checkout whose ipc_amd package, library and bench.py are used (default: this one)")
    ap.add_argument("--parent-root", default=None, help="--time: the checkout that (a) is measured in")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode:
        print(json.dumps({"time_run": time_run, "time_sweep": time_sweep}[a.mode](a)))
        return
    name = os.path.splitext(os.path.basename(a.g2o))[0] if a.g2o else a.workload
    path = a.out or os.path.join(HERE, "profiles", "sweep_%s.json" % name)
    out = {}
    if os.path.exists(path):                                           # --check and --time fill the same file, each its own part
        with open(path) as f:
            out = json.load(f)
    if a.time:
        out["time"] = timing(a)
        print(json.dumps(out["time"]))
    else:
        out["sweep"] = sweep(a)
    if a.check or a.time or a.out:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
