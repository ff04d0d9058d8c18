"""Monte-Carlo batch (ipc_run_batch) -- the reference's experiment loop on one engine.  bash/ipc_experiments_2D.sh runs one
dataset at ten outlier levels with ten draws each, ten ipc_tester_2D processes side by side; every draw shares the odometry chain
and the first `canonic_inliers` loop closures, only the injected outliers differ.  Here the draws of one level are one call: the
union list is the inliers followed by each draw's outliers, run r is the inliers plus its own outliers, and every cell among the
shared inliers is solved once.

  runs            from a base graph (--workload C1|C2: the workload's true loops; or --g2o FILE: all of its loops), R = --runs draws
                  through ipc_amd.synth.inject_outliers with the seeds --seed .. --seed + R - 1 and --outliers n each
  output          precision and recall per run (the TP / FP / TN / FN ladder of src/simulation.cpp:70-105, canonic_inliers = the base
                  graph's loop count), their mean and spread, the batch's report
  --check         every run against a fresh engine that was given the draw's own graph, one run() each, bit for bit; the counts of
                  differing words and bytes go to --out (default profiles/batch_<workload>.json)
  --time          the measurement of DESIGN.md 3.5 in fresh child processes, alternating: (a) one engine, set_candidates + run() per
                  draw -- with --parent-root in another checkout of the project (the parent commit, built in its own directory) --,
                  (b) one engine, set_candidates of the union + run_batch.  Host wall clock, outputs on the host.  One --outliers
                  level per invocation; the levels fill the same file.  The orchestrating process never opens the GPU.
  --sets exact    the three sets per draw (ipc_run_batch_exact) instead of the greedy set alone: size, precision and
                  recall of the greedy, the multi-start and the exact set, and whether the exact set is proven; the file is
                  profiles/batch_exact_<workload>.json.  With --time, in fresh child processes, alternating: (b) as above, (c) one
                  engine, set_candidates of the union + run_batch_exact, (d) one fresh engine and one run_exact() per draw -- the
                  only route to the same sets without ipc_run_batch_exact, with --parent-root in that checkout.  Two figures: the
                  added cost c / b, and d / c.

Usage: python tools/monte_carlo_batch.py --workload C2 --runs 10 --outliers 1000 --check
       python tools/monte_carlo_batch.py --workload C2 --runs 10 --outliers 256 --time --parent-root DIR
       python tools/monte_carlo_batch.py --workload C2 --sets exact [--time --parent-root DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")   # the host program's job, before HIP initialises (include/ipc_amd.h, "environment")

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _base(a):
    """(base graph: the chain and the true loops, Config with canonic_inliers = its loop count, name)."""
    from dataclasses import replace
    if a.g2o:
        from ipc_amd.consensus import Config
        from ipc_amd.graphio import read_g2o
        g = read_g2o(a.g2o)
        cfg = Config(s_factor=a.s_factor if a.s_factor else (10.0 if g.dim == 2 else 50.0), canonic_inliers=g.N)
        return g, cfg, os.path.splitext(os.path.basename(a.g2o))[0]
    import bench
    g, cfg, _ = bench.build_workload(a.workload)
    g = g.subset(np.arange(cfg.canonic_inliers))
    return g, replace(cfg, canonic_inliers=g.N), a.workload


def draws(a, base):
    """(the R draws as graphs, the union graph, the member lists): the union is the inliers followed by each draw's outliers."""
    from ipc_amd import synth
    from ipc_amd.graphio import PoseGraph
    gs = [synth.inject_outliers(base, a.outliers, seed=a.seed + r) for r in range(a.runs)]
    n0 = base.N
    ids = np.concatenate([base.loop_ids] + [g.loop_ids[n0:] for g in gs])
    meas = np.concatenate([base.loop_meas] + [g.loop_meas[n0:] for g in gs])
    info = np.concatenate([base.loop_info] + [g.loop_info[n0:] for g in gs])
    union = PoseGraph(base.dim, base.vertices, base.odom_meas, base.odom_info, ids, meas, info, dict(base.meta))
    members, at = [], n0
    for g in gs:
        k = g.N - n0
        members.append(np.concatenate([np.arange(n0), np.arange(at, at + k)]).astype(np.int32))
        at += k
    return gs, union, members


def _chain_only(g):
    from ipc_amd.graphio import PoseGraph
    return PoseGraph(g.dim, g.vertices, g.odom_meas, g.odom_info, g.loop_ids[:0], g.loop_meas[:0], g.loop_info[:0], dict(g.meta))


def precision_recall(acc, inliers):
    """src/simulation.cpp:70-81 with gt_loops[k].first = (k < canonic_inliers); float division as there (nan for 0 / 0)."""
    acc = np.asarray(acc).astype(bool)
    truth = np.arange(acc.shape[0]) < inliers
    tp, fn = int((truth & acc).sum()), int((truth & ~acc).sum())
    fp, tn = int((~truth & acc).sum()), int((~truth & ~acc).sum())
    prec = tp / (tp + fp) if tp + fp else float("nan")
    rec = tp / (tp + fn) if tp + fn else float("nan")
    return dict(tp=tp, fp=fp, tn=tn, fn=fn, precision=prec, recall=rec)


def _env():
    return dict(GPU_MAX_HW_QUEUES=os.environ.get("GPU_MAX_HW_QUEUES"))


def batch(a):
    from ipc_amd.consensus import IPC
    base, cfg, name = _base(a)
    gs, union, members = draws(a, base)
    eng = IPC(union, cfg, device=0)
    t0 = time.perf_counter()
    bits, accs, rep = eng.run_batch(members, want_bits=True)
    dt = time.perf_counter() - t0
    eng.close()
    rows = []
    print("%4s %6s %9s %6s %6s %10s %8s" % ("run", "seed", "accepted", "tp", "fp", "precision", "recall"))
    for r, acc in enumerate(accs):
        pr = precision_recall(acc, cfg.canonic_inliers)
        rows.append(dict(run=r, seed=a.seed + r, candidates=int(acc.shape[0]), accepted=int(acc.sum()), **pr))
        print("%4d %6d %9d %6d %6d %10.4f %8.4f" % (r, a.seed + r, rows[-1]["accepted"], pr["tp"], pr["fp"], pr["precision"], pr["recall"]))
    p, q = np.array([x["precision"] for x in rows]), np.array([x["recall"] for x in rows])
    summary = dict(precision_mean=float(np.nanmean(p)), precision_min=float(np.nanmin(p)), precision_max=float(np.nanmax(p)),
                   recall_mean=float(np.nanmean(q)), recall_min=float(np.nanmin(q)), recall_max=float(np.nanmax(q)))
    print("precision %.4f [%.4f, %.4f]  recall %.4f [%.4f, %.4f]" % (summary["precision_mean"], summary["precision_min"], summary["precision_max"],
                                                                      summary["recall_mean"], summary["recall_min"], summary["recall_max"]))
    print("report: " + json.dumps(rep))
    out = dict(mode="batch", workload=name, V=int(base.V), canonic_inliers=int(cfg.canonic_inliers), runs=a.runs, outliers=a.outliers,
               seed=a.seed, union_candidates=int(union.N), per_run=rows, summary=summary, report=rep,
               cell_ratio=rep["cells_separate"] / max(rep["cells"], 1), batch_ms=1e3 * dt, env=_env())
    if a.check:
        diff = []
        for r, g in enumerate(gs):
            ref = IPC(g, cfg, device=0)
            b_ref, a_ref = ref.run()
            ref.close()
            diff.append(dict(run=r, differing_words=int((bits[r] != b_ref).sum()), differing_accepted_bytes=int((accs[r] != a_ref).sum())))
        out["check"] = dict(fresh_engines=len(gs), differing_words=sum(d["differing_words"] for d in diff),
                            differing_accepted_bytes=sum(d["differing_accepted_bytes"] for d in diff), per_run=diff)
        print("check against %d fresh engines: %d differing words, %d differing accepted bytes"
              % (len(gs), out["check"]["differing_words"], out["check"]["differing_accepted_bytes"]))
    return out


def batch_exact(a):
    """--sets exact: the three sets of every draw from one run_batch_exact."""
    from ipc_amd.consensus import IPC
    base, cfg, name = _base(a)
    _, union, members = draws(a, base)
    eng = IPC(union, cfg, device=0)
    t0 = time.perf_counter()
    accs, mss, greedys, reps, rep, bx = eng.run_batch_exact(members)
    dt = time.perf_counter() - t0
    eng.close()
    rows = []
    print("%4s %6s | %6s %9s %7s | %6s %9s %7s | %6s %9s %7s %6s" % ("run", "seed", "greedy", "precision", "recall", "multi", "precision", "recall",
                                                                     "exact", "precision", "recall", "proven"))
    for r in range(len(members)):
        sets = dict(greedy=greedys[r], multistart=mss[r], exact=accs[r])
        row = dict(run=r, seed=a.seed + r, candidates=int(accs[r].shape[0]), proven=int(reps[r]["proven"]), report=reps[r])
        for k, v in sets.items():
            row[k] = dict(size=int(v.sum()), **precision_recall(v, cfg.canonic_inliers))
        rows.append(row)
        print("%4d %6d | %6d %9.4f %7.4f | %6d %9.4f %7.4f | %6d %9.4f %7.4f %6d"
              % ((r, a.seed + r) + tuple(x for k in sets for x in (row[k]["size"], row[k]["precision"], row[k]["recall"])) + (row["proven"],)))
    summary = {}
    for k in ("greedy", "multistart", "exact"):
        p, q = np.array([x[k]["precision"] for x in rows]), np.array([x[k]["recall"] for x in rows])
        summary[k] = dict(size_mean=float(np.mean([x[k]["size"] for x in rows])), precision_mean=float(np.nanmean(p)), recall_mean=float(np.nanmean(q)),
                          recall_min=float(np.nanmin(q)), recall_max=float(np.nanmax(q)))
        print("%-10s size %.1f  precision %.4f  recall %.4f [%.4f, %.4f]" % (k, summary[k]["size_mean"], summary[k]["precision_mean"],
                                                                            summary[k]["recall_mean"], summary[k]["recall_min"], summary[k]["recall_max"]))
    print("report: " + json.dumps(rep))
    print("sets:   " + json.dumps(bx))
    return dict(mode="batch_exact", workload=name, V=int(base.V), canonic_inliers=int(cfg.canonic_inliers), runs=a.runs, outliers=a.outliers,
                seed=a.seed, union_candidates=int(union.N), per_run=rows, summary=summary, report=rep, sets_report=bx, batch_exact_ms=1e3 * dt,
                env=_env())


def time_batch_exact(a):
    """(c): one engine, set_candidates of the union + run_batch_exact."""
    from ipc_amd.consensus import IPC
    base, cfg, name = _base(a)
    _, union, members = draws(a, base)
    eng = IPC(_chain_only(base), cfg, device=0)
    t0 = time.perf_counter()
    eng.set_candidates(union.loop_ids, union.loop_meas, union.loop_info)
    accs, mss, greedys, reps, rep, bx = eng.run_batch_exact(members)
    dt = time.perf_counter() - t0
    eng.close()
    return dict(mode="time_batch_exact", workload=name, ms=1e3 * dt, accepted=[int(x.sum()) for x in greedys], exact=[int(x.sum()) for x in accs],
                multistart=[int(x.sum()) for x in mss], proven=[int(r["proven"]) for r in reps], report=rep, sets_report=bx)


def time_exact_separate(a):
    """(d): one fresh engine and one run_exact() per draw; uses nothing newer than ipc_run_exact, so --root may be another checkout.
    ms: the engines' construction included; run_exact_ms: the run_exact() calls alone."""
    from ipc_amd.consensus import IPC
    base, cfg, name = _base(a)
    gs, _, _ = draws(a, base)
    exact, proven, inner = [], [], 0.0
    t0 = time.perf_counter()
    for g in gs:
        eng = IPC(g, cfg, device=0)
        t1 = time.perf_counter()
        acc, _, rep = eng.run_exact()
        inner += time.perf_counter() - t1
        eng.close()
        exact.append(int(acc.sum()))
        proven.append(int(rep["proven"]))
    dt = time.perf_counter() - t0
    return dict(mode="time_exact_separate", workload=name, ms=1e3 * dt, run_exact_ms=1e3 * inner, exact=exact, proven=proven)


def timing_exact(a):
    def child(mode, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--workload", a.workload, "--root", root, "--runs", str(a.runs),
               "--outliers", str(a.outliers), "--seed", str(a.seed)]
        if a.g2o:
            cmd += ["--g2o", a.g2o, "--s-factor", str(a.s_factor)]
        txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=a.child_timeout).stdout.decode()
        return json.loads([ln for ln in txt.splitlines() if ln.startswith("{")][-1])
    bat, bex, sep = [], [], []
    for _ in range(a.rounds):                                          # alternating, every measurement in a fresh process
        bat.append(child("time_batch", a.root))
        bex.append(child("time_batch_exact", a.root))
        sep.append(child("time_exact_separate", a.parent_root or a.root))
    assert all(x["accepted"] == y["accepted"] for x in bat for y in bex), "run_batch and run_batch_exact gave different greedy sets"
    assert all(x["exact"] == y["exact"] and x["proven"] == y["proven"] for x in sep for y in bex), "the two routes gave different exact sets"
    tb, tc, td, ti = ([x[k] for x in v] for v, k in ((bat, "ms"), (bex, "ms"), (sep, "ms"), (sep, "run_exact_ms")))
    spread = lambda v: float((max(v) - min(v)) / np.median(v))
    part = lambda v: dict(median_ms=float(np.median(v)), runs_ms=v, spread=spread(v))
    return dict(mode="time_exact", workload=a.workload, runs=a.runs, outliers=a.outliers, rounds=a.rounds,
                b_set_candidates_of_the_union_and_run_batch=part(tb), c_set_candidates_of_the_union_and_run_batch_exact=part(tc),
                d_fresh_engine_and_run_exact_per_draw=dict(checkout="another checkout (--parent-root)" if a.parent_root else "this checkout",
                                                           run_exact_calls_alone=part(ti), **part(td)),
                added_cost_c_over_b=float(np.median(tc) / np.median(tb)), added_ms_c_minus_b=float(np.median(tc) - np.median(tb)),
                separate_over_batch_d_over_c=float(np.median(td) / np.median(tc)),
                separate_run_exact_alone_over_batch=float(np.median(ti) / np.median(tc)),
                exact=bex[-1]["exact"], multistart=bex[-1]["multistart"], greedy=bex[-1]["accepted"], proven=bex[-1]["proven"],
                report=bex[-1]["report"], sets_report=bex[-1]["sets_report"], env=_env())


def time_separate(a):
    """(a): one engine, set_candidates + run() per draw; uses nothing newer than ipc_run, so --root may be another checkout."""
    from ipc_amd.consensus import IPC
    base, cfg, name = _base(a)
    gs, _, _ = draws(a, base)
    eng = IPC(_chain_only(base), cfg, device=0)
    accepted = []
    t0 = time.perf_counter()
    for g in gs:
        eng.set_candidates(g.loop_ids, g.loop_meas, g.loop_info)
        _, acc = eng.run()
        accepted.append(int(acc.sum()))
    dt = time.perf_counter() - t0
    eng.close()
    return dict(mode="time_separate", workload=name, ms=1e3 * dt, accepted=accepted)


def time_batch(a):
    """(b): one engine, set_candidates of the union + run_batch."""
    from ipc_amd.consensus import IPC
    base, cfg, name = _base(a)
    _, union, members = draws(a, base)
    eng = IPC(_chain_only(base), cfg, device=0)
    t0 = time.perf_counter()
    eng.set_candidates(union.loop_ids, union.loop_meas, union.loop_info)
    _, accs, rep = eng.run_batch(members, want_bits=True)
    dt = time.perf_counter() - t0
    eng.close()
    return dict(mode="time_batch", workload=name, ms=1e3 * dt, accepted=[int(x.sum()) for x in accs], report=rep)


def timing(a):
    def child(mode, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--workload", a.workload, "--root", root, "--runs", str(a.runs),
               "--outliers", str(a.outliers), "--seed", str(a.seed)]
        if a.g2o:
            cmd += ["--g2o", a.g2o, "--s-factor", str(a.s_factor)]
        txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=a.child_timeout).stdout.decode()
        return json.loads([ln for ln in txt.splitlines() if ln.startswith("{")][-1])
    sep, bat = [], []
    for _ in range(a.rounds):                                          # alternating, every measurement in a fresh process
        sep.append(child("time_separate", a.parent_root or a.root))
        bat.append(child("time_batch", a.root))
    assert all(s["accepted"] == b["accepted"] for s in sep for b in bat), "the two paths accepted different sets"
    ta, tb = [s["ms"] for s in sep], [b["ms"] for b in bat]
    spread = lambda v: float((max(v) - min(v)) / np.median(v))
    rep = bat[-1]["report"]
    return dict(mode="time", workload=a.workload, runs=a.runs, outliers=a.outliers, rounds=a.rounds,
                a_set_candidates_and_run_per_draw=dict(checkout="another checkout (--parent-root)" if a.parent_root else "this checkout",
                                                       median_ms=float(np.median(ta)), runs_ms=ta, spread=spread(ta)),
                b_set_candidates_of_the_union_and_run_batch=dict(median_ms=float(np.median(tb)), runs_ms=tb, spread=spread(tb)),
                a_over_b=float(np.median(ta) / np.median(tb)), cell_ratio=rep["cells_separate"] / max(rep["cells"], 1), report=rep, env=_env())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", help="a bench.py workload whose true loops are the base graph (C1, C2)")
    ap.add_argument("--g2o", default=None, help="a .g2o file as the base graph instead (with --s-factor)")
    ap.add_argument("--s-factor", type=float, default=0.0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--outliers", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--sets", default="greedy", choices=["greedy", "exact"], help="exact: the greedy, multi-start and exact set per draw")
    ap.add_argument("--mode", default=None, choices=["time_separate", "time_batch", "time_batch_exact", "time_exact_separate"],
                    help="(the children of --time)")
    ap.add_argument("--root", default=HERE, help="checkout whose ipc_amd package, library and bench.py are used (default: this one)")
    ap.add_argument("--parent-root", default=None, help="--time: the checkout that (a) is measured in")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.mode:
        print(json.dumps({"time_separate": time_separate, "time_batch": time_batch, "time_batch_exact": time_batch_exact,
                          "time_exact_separate": time_exact_separate}[a.mode](a)))
        return
    name = os.path.splitext(os.path.basename(a.g2o))[0] if a.g2o else a.workload
    exact = a.sets == "exact"
    path = a.out or os.path.join(HERE, "profiles", "batch_%s%s.json" % ("exact_" if exact else "", name))
    out = {}
    if os.path.exists(path):                                           # --check and --time fill the same file, each its own part
        with open(path) as f:
            out = json.load(f)
    if a.time:
        out.setdefault("time", {})["outliers_%d" % a.outliers] = timing_exact(a) if exact else timing(a)
        print(json.dumps(out["time"]["outliers_%d" % a.outliers]))
    elif exact:
        out["batch_exact"] = batch_exact(a)
    else:
        out["batch"] = batch(a)
    if a.check or a.time or a.out or exact:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
