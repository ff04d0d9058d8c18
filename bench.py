#!/usr/bin/env python
"""bench.py -- candidate-pairs/s of the consistency matrix + set-max (BASELINE.json metric).

A "step" is one pass of the hot path over the whole candidate set: plan + solve every cell of
the N x N consistency matrix (row-sharded over the ranks), all-gather the bit rows (N > 1 GPU),
assemble the symmetric matrix and run the set-max.  Inputs (odometry chain, candidates) are
resident in HBM before the timed region starts.

Workload (config.workload): BASELINE.json configs[1] = INTEL-like SE2 graph (V=1228, 256 true
loops) + 1000 injected outliers => N=1256, 789,396 cells (i <= j).  Synthetic stand-in -- the
INTEL file itself is not shipped with the reference and there is no network.

python bench.py --gpus N --steps K --warmup W [--workload C1|C2|C3|C4|C4m|C5|T4k|T700|T2400]
                [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints one JSON line (`ms_per_step`: one timed step).
--dump-outputs DIR writes what the last timed step computed (accepted set, consistency matrix, per-cell chi2) as .npy.
--full adds everything else: roofline, single-shot first step, CPU baseline, the literal trial loop on the GPU, the
reference's incremental metric and final map, the set-only mode.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")   # before HIP initialises: one hardware queue per solve of the incremental mode's window

import numpy as np
import torch

FP64_PEAK_TFLOPS = 78.6      # MI355X FP64: vector == dense MFMA rate (half the 157.3 TF FP32 rate)
HBM_PEAK_GBS = 8000.0

B_ODOM = 72.0                    # bytes of one odometry record (3 + 6 doubles), SURVEY.md 8d
B_ODOM3 = 224.0                  # 7 + 21 doubles
F_SURVEY = {2: 450.0, 3: 3000.0}  # SURVEY.md 8(d) placeholders: flops per pose and outer iteration


def build_workload(name):
    from ipc_amd import synth
    from ipc_amd.consensus import Config
    if name == "C2":
        g = synth.inject_outliers(synth.intel_like(), 1000, seed=1000)
        cfg = Config(6.251, 50, 11.345, 100, 10.0, canonic_inliers=256)
        desc = "INTEL-like SE2 synthetic (V=1228, 256 true loops) + 1000 injected outliers"
    elif name == "C1":
        g = synth.inject_outliers(synth.intel_like(), 100, seed=100)
        cfg = Config(6.251, 50, 11.345, 100, 10.0, canonic_inliers=256)
        desc = "INTEL-like SE2 synthetic (V=1228, 256 true loops) + 100 injected outliers"
    elif name == "C3":
        g = synth.inject_outliers(synth.mit_like(), 5000, seed=5000)
        cfg = Config(6.251, 50, 11.345, 100, 10.0, canonic_inliers=20)
        desc = "MIT-like SE2 synthetic (V=808, 20 true loops) + 5000 injected outliers"
    elif name == "C4":
        g = synth.inject_outliers(synth.sphere_like(), 2000, seed=2000)
        cfg = Config(6.251, 50, 6.251, 100, 50.0, canonic_inliers=2450)
        desc = "sphere2500-like SE3 synthetic (V=2500, 2450 true loops) + 2000 injected outliers"
    elif name == "C4m":
        g = synth.inject_outliers(synth.sphere_like(), 200, seed=200)
        g = g.subset(np.concatenate([np.arange(0, 2450, 10), np.arange(2450, g.N)]))
        cfg = Config(6.251, 50, 6.251, 100, 50.0, canonic_inliers=245)
        desc = "sphere2500-like SE3 synthetic (V=2500), every 10th true loop (245) + 200 injected outliers"
    elif name == "C4s":
        g = synth.inject_outliers(synth.sphere_like(rings=20, per_ring=25, radius=20.0), 60, seed=60)
        g2 = g.subset(np.concatenate([np.arange(0, 475, 8), np.arange(475, g.N)]))
        g = g2
        cfg = Config(6.251, 50, 6.251, 100, 50.0, canonic_inliers=60)
        desc = "small sphere SE3 synthetic (V=500, 60 true loops) + 60 injected outliers"
    elif name == "C5":        # BASELINE configs[4] on one GPU (the driver shards it over 8): bounded loop spans
        g = synth.inject_outliers(synth.chain3d(), 20000, seed=20000, local=True)
        cfg = Config(6.251, 50, 6.251, 100, 50.0, canonic_inliers=5000)
        desc = "synthetic SE3 chain (V=50000, 5000 true loops of span <= 200) + 20000 injected local outliers"
    elif name == "T700":      # every chain <= 699 poses: one kernel variant can take all cells (variant A/B timing)
        g = synth.inject_outliers(synth._se2_graph(700, 60, seed=7, laps=4.0), 300, seed=70)
        cfg = Config(6.251, 50, 11.345, 100, 10.0, canonic_inliers=60)
        desc = "SE2 synthetic (V=700, 60 true loops) + 300 injected outliers"
    elif name == "T2400":     # long trajectory: chains up to ~2400 poses, the chain no longer fits the LDS window
        g = synth.inject_outliers(synth._se2_graph(2400, 40, seed=9, laps=14.0, name="long"), 200, seed=24)
        cfg = Config(6.251, 50, 11.345, 100, 10.0, canonic_inliers=40)
        desc = "SE2 synthetic (V=2400, 40 true loops) + 200 injected outliers"
    elif name == "T4k":       # short chains only (local loop closures, as in real odometry + place recognition): SE2 w1 / w3 bins
        g0 = synth._se2_graph(4000, 3000, seed=13, laps=60.0, name="local")
        span = np.abs(g0.loop_ids[:, 1] - g0.loop_ids[:, 0])
        g0 = g0.subset(np.nonzero(span <= 140)[0])
        g = synth.inject_outliers(g0, 3000, seed=41, local=True)
        cfg = Config(6.251, 50, 11.345, 100, 10.0, canonic_inliers=g0.N)
        desc = "SE2 synthetic (V=4000, %d true loops of span <= 140) + 3000 injected local outliers" % g0.N
    elif name == "R2k":       # SE2 spiral, every pose closed onto the turn before: one growing cluster of ~2 000 loops (banded solver on 3 x 3 blocks)
        g = synth.inject_outliers(synth.ring_se2(), 300, seed=23)
        cfg = Config(6.251, 50, 11.345, 100, 10.0, canonic_inliers=1950)
        desc = "SE2 spiral synthetic (V=2000, 1950 true loops of span 50) + 300 injected outliers"
    elif name == "tiny":
        g = synth.inject_outliers(synth._se2_graph(300, 24, seed=5, laps=3.0), 40, seed=4)
        cfg = Config(6.251, 50, 11.345, 100, 10.0, canonic_inliers=24)
        desc = "tiny SE2 synthetic (V=300) + 40 outliers"
    else:
        raise SystemExit("unknown workload " + name)
    return g, cfg, desc


def effective_cores():
    """Host cores this process may really use: the smaller of the CPUs it is allowed on and its cgroup's CPU quota
    (the GPU boxes report 256 logical CPUs and grant 16 through cpu.max -- threads beyond that only get throttled)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota:
        n = max(1, min(n, int(quota + 0.5)))
    return n


def _stratified_sample(cells, n_target, seed=0):
    """Indices of an L-stratified sample of the solved cells, in random order."""
    L = (cells["hi"] - cells["lo"]).astype(np.int64)
    order = np.argsort(L, kind="stable")
    pick = order[np.linspace(0, len(order) - 1, min(n_target, len(order))).astype(np.int64)]
    rng = np.random.default_rng(seed)
    rng.shuffle(pick)                      # any prefix is an unbiased stratified sample; shards are balanced
    return pick


def cpu_baseline(g, cfg, cells, budget_s):
    """The CPU oracle (plain-C restatement of the reference path, oracle/) on the GPU box's host cores, SURVEY.md 8(d).

    All-core leg: POSIX threads drawing cells from one shared queue, longest chains first; the WHOLE set of solved cells
    when the budget allows it (configs 1-2 are timed in full), else an L-stratified sample of at least 64
    cells per thread -- one run (tens of seconds of CPU work).  1-thread leg (the reference is single-threaded): a prefix
    of a stratified sample.  The chi2 differences against the GPU are reported per class: cells both sides converged on,
    and cells that stop at the iteration cap on a still-moving trajectory (rounding-dependent end point)."""
    from oracle import oracle as O
    poses = O.propagate(g.dim, g.odom_meas)
    cores = effective_cores()
    Lall = (cells["hi"] - cells["lo"]).astype(np.int64)

    def run(idx, threads):
        idx = idx[np.argsort(-Lall[idx], kind="stable")]          # the queue hands out the long chains first
        t0 = time.perf_counter()
        mx, its, used = O.pair_cells_mt(g.dim, g.odom_meas, g.odom_info, cfg.s_factor, poses, g.loop_ids, g.loop_meas,
                                        g.loop_info, cells["i"][idx], cells["j"][idx], cfg.fast_reject_iter_base,
                                        cfg.slow_reject_iter_base, threads)
        return time.perf_counter() - t0, idx, mx, its, used

    pick = _stratified_sample(cells, 4096)
    # size the legs to the budget from a short 1-thread probe
    n_probe, t_probe = 0, 0.0
    while n_probe < min(32, len(pick)) and t_probe < 1.5:
        dtp = run(pick[n_probe:n_probe + 2], 1)[0]
        t_probe += dtp
        n_probe += 2
    rate1 = n_probe / max(t_probe, 1e-9)
    n1 = int(max(n_probe, min(len(pick), rate1 * budget_s * 0.4)))
    t1, idx1, mx1, its1, _ = run(pick[:n1], 1)
    rate1 = n1 / t1
    # all cores (warm-up discarded, median of >= 5): a short all-core probe gives the rate the box really
    # delivers (shared hosts, SMT); the sample is what ~1/8 of 0.7 x budget_s holds at that rate -- at least 64 cells per
    # thread, the WHOLE workload if that is less (C1) -- and is run 1 + 5 times: the first run is the warm-up
    nprobe_all = int(min(len(cells), 8 * cores))
    tp = run(_stratified_sample(cells, nprobe_all, seed=2), cores)[0]
    want = int(nprobe_all / max(tp, 1e-9) * budget_s * 0.7 / 6.0)
    whole = want >= len(cells)
    n_all = len(cells) if whole else int(min(len(cells), max(want, 64 * cores)))
    sel = np.arange(len(cells)) if whole else _stratified_sample(cells, n_all, seed=1)
    reps_all = []
    for rep in range(6):
        t_rep, idxa, mxa, itsa, used = run(sel, cores)
        if rep > 0:
            reps_all.append(t_rep)
    t_all = float(np.median(reps_all))
    th_all = np.where(cells["i"] == cells["j"], cfg.fast_reject_th, cfg.slow_reject_th)
    nl = np.where(cells["i"] == cells["j"], 1, 2)
    cap_all = np.where(cells["i"] == cells["j"], cfg.fast_reject_iter_base, cfg.slow_reject_iter_base) * np.where(Lall + nl > 100, 5, 1)
    mism = int(((~(mxa > th_all[idxa])) != (~(cells["max_chi2"][idxa] > th_all[idxa]))).sum())
    rel = np.abs(mxa - cells["max_chi2"][idxa]) / np.maximum(np.abs(mxa), 1e-300)
    conv = (itsa < cap_all[idxa]) & (cells["iterations"][idxa] < cap_all[idxa])
    rel_conv = float(np.nanmax(rel[conv])) if conv.any() else 0.0
    rel_cap = float(np.nanmax(rel[~conv])) if (~conv).any() else 0.0
    one = dict(value=rate1, unit="solved candidate-pairs/s", cores=1, kind="port",
               sample="%d solved cells (prefix of an L-stratified sample), %.1f s, one run" % (n1, t1))
    return dict(value=n_all / t_all, unit="solved candidate-pairs/s (compare with solved_cells_per_s, not with value)", cores=used, kind="port",
                sample="%s, one shared work queue (longest chains first) over %d POSIX threads (the host shows %d logical CPUs; affinity and the cgroup CPU quota leave %d), warm-up run "
                       "discarded, median of 5 runs = %.2f s; the CPU side is this repo's plain-C restatement (oracle/), not g2o -- the reference cannot "
                       "be built here; non-overlapping pairs are free on both sides and excluded from this rate" % (
                           ("ALL %d solved cells of the workload" % n_all) if whole else
                           ("%d solved cells, L-stratified over the chain-length order of the same workload (%d per thread)"
                            % (n_all, n_all // max(used, 1))), used, os.cpu_count() or 1, cores, t_all),
                whole_workload=bool(whole),
                run_seconds=[round(t, 3) for t in reps_all],
                scaling_over_1_thread=(n_all / t_all) / rate1,
                single_thread=one,
                decisions_differing_from_gpu=mism,
                max_rel_chi2_diff_vs_gpu={"converged": rel_conv, "at_iteration_cap": rel_cap,
                                          "cells_converged": int(conv.sum()), "cells_at_iteration_cap": int((~conv).sum()),
                                          "note": "north_star's 1e-5 holds on the converged class; a cell that stops at the "
                                                  "iteration cap stops on a still-moving trajectory whose end point depends "
                                                  "on rounding (g2o has no convergence test), decisions agree there too"})


def incremental_metric(g, cfg, eng, gpu_candidates, cpu_budget_s, workload, reps=3):
    """The reference's own metric (src/simulation.cpp:36-44,87): mean wall time per agreementCheck in the faithful
    incremental mode, as candidates/s.  GPU: ipc_agreement_check over the WHOLE candidate list (device-resident
    dog-leg, speculative window).  CPU: the oracle's IncrementalIPC (1 thread) on the prefix of the processing order
    it finishes inside the budget -- the early candidates meet small clusters, so the prefix rate flatters the CPU;
    the GPU's rate on the same prefix is reported next to it, and so is the oracle's time for the whole list as
    recorded when the committed fixture was written (another machine: the authoring container)."""
    from oracle import oracle as O
    order = eng.candidate_order()
    n_gpu = len(order) if gpu_candidates <= 0 else min(gpu_candidates, len(order))
    t_gpu, acc_gpu, stamps, runs = 1e30, None, None, []
    for _ in range(reps):                         # (a run of C1 / C2 is ~1 s and single runs spread by 15 %: one host thread feeds 16 streams)
        eng.reset()
        eng.agreementCheck(int(order[0]))        # warm-up: workspaces, streams
        eng.reset()
        eng.synchronize()
        acc_r, stamps_r = [], []
        t0 = time.perf_counter()
        for k in order[:n_gpu]:
            acc_r.append(eng.agreementCheck(int(k)))
            stamps_r.append(time.perf_counter() - t0)
        eng.synchronize()
        t_r = time.perf_counter() - t0
        runs.append(n_gpu / t_r)
        if acc_gpu is not None and acc_r != acc_gpu:
            raise RuntimeError("faithful run: decisions differ between two repetitions")
        if t_r < t_gpu:
            t_gpu, stamps = t_r, stamps_r
        acc_gpu = acc_r
    cpu = O.IncrementalIPC(g.dim, g.odom_meas, g.odom_info, cfg.s_factor, cfg.fast_reject_th, cfg.fast_reject_iter_base,
                           cfg.slow_reject_th, cfg.slow_reject_iter_base, g.loop_ids, g.loop_meas, g.loop_info)
    t0 = time.perf_counter()
    acc_cpu = []
    for k in order[:n_gpu]:
        ok, _ = cpu.agreement_check(int(k))
        acc_cpu.append(ok)
        if time.perf_counter() - t0 > cpu_budget_s:
            break
    t_cpu = time.perf_counter() - t0
    n_cpu = len(acc_cpu)
    med = float(np.median(runs))
    out = dict(unit="candidates/s", gpu=med, gpu_is="median of %d run%s" % (len(runs), "" if len(runs) == 1 else "s"), gpu_best_run=n_gpu / t_gpu,
               gpu_candidates=n_gpu, gpu_avg_time_x_test_s=1.0 / med, gpu_seconds_per_run=[round(n_gpu / r, 3) for r in runs],
               gpu_accepted=int(sum(acc_gpu)), gpu_runs=[round(r, 1) for r in runs],
               cpu_1t_prefix=n_cpu / t_cpu, cpu_prefix_candidates=n_cpu, cpu_avg_time_x_test_s_prefix=t_cpu / n_cpu,
               gpu_on_the_same_prefix=n_cpu / stamps[n_cpu - 1],
               decisions_differing_on_common_prefix=int(sum(a != b for a, b in zip(acc_gpu[:n_cpu], acc_cpu))),
               note="reference metric 'Avg Time x test' (src/simulation.cpp:87) as a rate; GPU over the whole list, "
                    "CPU = oracle IncrementalIPC (1 thread) on the prefix it finishes in the budget")
    if n_gpu == len(order):
        # the harness's final map over odometry / s + the accepted loops, optimize(1000) (src/simulation.cpp:50-65; the
        # reference times it, :62-68, and throws the figure away)
        accv = np.zeros(len(order), dtype=np.uint8)
        accv[np.asarray(order)[np.array(acc_gpu, dtype=bool)]] = 1
        eng.final_optimize(accv, iterations=1000)
        tf = []
        for _ in range(3):
            t0 = time.perf_counter()
            _, finfo = eng.final_optimize(accv, iterations=1000)
            tf.append(time.perf_counter() - t0)
        fm = dict(seconds=float(np.median(tf)), chi2_initial=finfo.chi2_initial, chi2_total=finfo.chi2_total, max_edge_chi2=finfo.max_chi2,
                  iterations=finfo.iterations, loops=int(accv.sum()), flags=finfo.flags)
        ffx = os.path.join(ROOT, "tests", "golden", "%s_final_map_expected.npz" % workload.lower())
        if os.path.exists(ffx):
            fe = np.load(ffx)
            if np.array_equal(fe["accepted"], accv):
                fm["oracle_chi2_total"] = float(fe["chi2_total"])
                fm["rel_diff_vs_oracle"] = abs(finfo.chi2_total - float(fe["chi2_total"])) / float(fe["chi2_total"])
                fm["oracle_seconds_authoring_container_1_thread"] = float(fe["oracle_seconds_authoring_container"])
        out["final_map"] = fm
    fx = os.path.join(ROOT, "tests", "golden", "%s_incremental_expected.npz" % workload.lower())
    if os.path.exists(fx) and n_gpu == len(order):
        exp = np.load(fx)
        ne = len(exp["order"])
        if np.array_equal(exp["order"], order[:ne]):
            full = ne == len(order)
            key = "oracle_full_run" if full else "oracle_prefix_run"
            out["decisions_differing_from_the_%s" % key] = int((exp["decision"].astype(bool) != np.array(acc_gpu[:ne])).sum())
            out["%s_s_authoring_container_1_thread" % key] = float(exp["oracle_seconds_authoring_container"])
            out["%s_candidates" % key] = int(ne)
            out["%s_source" % key] = os.path.relpath(fx, ROOT)
            if not full:
                out["gpu_seconds_on_the_oracle_prefix"] = stamps[ne - 1]
    return out


def faithful_run_of(workload):
    """Wall time of the faithful agreementCheck loop over ALL candidates of another bench workload (configs[0] next to the
    headline's configs[1]); decisions against the committed oracle run."""
    from ipc_amd.consensus import IPC
    g, cfg, _ = build_workload(workload)
    eng = IPC(g, cfg, device=0)
    order = eng.candidate_order()
    times, acc = [], None
    for _ in range(3):
        eng.reset()
        eng.agreementCheck(int(order[0]))
        eng.reset()
        eng.synchronize()
        t0 = time.perf_counter()
        acc = [eng.agreementCheck(int(k)) for k in order]
        eng.synchronize()
        times.append(time.perf_counter() - t0)
    eng.close()
    med = float(np.median(times))
    out = dict(workload=workload, candidates=len(order), seconds=med, seconds_is="median of 3 runs", seconds_per_run=[round(t, 3) for t in times],
               candidates_per_s=len(order) / med, accepted=int(sum(acc)))
    fx = os.path.join(ROOT, "tests", "golden", "%s_incremental_expected.npz" % workload.lower())
    if os.path.exists(fx):
        exp = np.load(fx)
        if np.array_equal(exp["order"], order):
            out["decisions_differing_from_the_oracle_full_run"] = int((exp["decision"].astype(bool) != np.array(acc)).sum())
            out["oracle_full_run_s_authoring_container_1_thread"] = float(exp["oracle_seconds_authoring_container"])
    return out


def kernel_source_digest():
    """sha256 over the cell-solver kernel sources: a committed counter pass belongs to the build it was taken on."""
    import hashlib
    hh = hashlib.sha256()
    csrc = os.path.join(ROOT, "ipc_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.startswith(("se2_", "se3_", "block_prims", "cell_kernels")):
            hh.update(open(os.path.join(csrc, f), "rb").read())
    return hh.hexdigest()[:16]


def executed_flops(workload, dim):
    """Executed FP64 flops of the cell-solver kernels of ONE solve of this workload, from the committed rocprofv3 PMC
    pass profiles/r<round>_<workload>_pmc_sq.csv (SQ_INSTS_VALU_{FMA,MUL,ADD,TRANS}_F64 are wave-level instruction
    counts: x 64 lanes, FMA = 2 flops).  `current` says whether the pass was taken on the kernel sources of this build
    (sidecar .meta.json written by tools/r4_profile.sh sq; passes without one predate the check).  None: no such file."""
    import csv
    for rnd in ("r6", "r5", "r4", "r3", "r2"):
        path = os.path.join(ROOT, "profiles", "%s_%s_pmc_sq.csv" % (rnd, workload.lower()))
        if os.path.exists(path):
            break
    else:
        return None
    c = {}
    for r in csv.DictReader(open(path)):
        if any(t in r["kernel"] for t in ("_cells_kernel", "_wave_kernel", "_group_kernel", "_lds_kernel")):
            c[r["counter"]] = c.get(r["counter"], 0.0) + float(r["sum_value"])
    if "SQ_INSTS_VALU_FMA_F64" not in c:
        return None
    meta = os.path.splitext(path)[0] + ".meta.json"
    current = None
    if os.path.exists(meta):
        current = json.load(open(meta)).get("kernel_source_digest") == kernel_source_digest()
    return dict(flops=64.0 * (2 * c["SQ_INSTS_VALU_FMA_F64"] + c.get("SQ_INSTS_VALU_MUL_F64", 0.0)
                              + c.get("SQ_INSTS_VALU_ADD_F64", 0.0) + c.get("SQ_INSTS_VALU_TRANS_F64", 0.0)),
                mfma_mops_f64=c.get("SQ_INSTS_VALU_MFMA_MOPS_F64"), source=os.path.relpath(path, ROOT), current=current)


DUMP_MATRIX_ELEMS = 4 * 1024 * 1024     # --dump-outputs: at most 16 MB of float32 matrix rows ...
DUMP_CELLS = 1024 * 1024                # ... and 20 MB of per-cell records (i, j float32, max_chi2 float64, iterations float32)


def dump_outputs(path, bits, acc, cells, N):
    """What the timed path computed in its last step, as float32 / float64 .npy files under `path` (at most ~36 MB):
    the accepted set, the symmetric consistency matrix (all rows, or a fixed seeded sample of rows when N x N exceeds
    DUMP_MATRIX_ELEMS) and the solved cells of this rank sorted by (i, j) (a fixed seeded sample beyond DUMP_CELLS).
    Every sampled array comes with the indices it was taken at."""
    from ipc_amd.consensus import unpack_bits
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "accepted.npy"), acc.astype(np.float32))
    rows = np.arange(N)
    if N * N > DUMP_MATRIX_ELEMS:
        rows = np.sort(np.random.default_rng(0).choice(N, DUMP_MATRIX_ELEMS // N, replace=False))
    np.save(os.path.join(path, "consistency_matrix.npy"), unpack_bits(bits[rows], N).astype(np.float32))
    np.save(os.path.join(path, "consistency_matrix_rows.npy"), rows.astype(np.float32))
    cells = cells[np.lexsort((cells["j"], cells["i"]))]
    if len(cells) > DUMP_CELLS:
        cells = cells[np.sort(np.random.default_rng(1).choice(len(cells), DUMP_CELLS, replace=False))]
    np.save(os.path.join(path, "cell_ij.npy"), np.stack([cells["i"], cells["j"]], axis=1).astype(np.float32))
    np.save(os.path.join(path, "cell_max_chi2.npy"), cells["max_chi2"].astype(np.float64))
    np.save(os.path.join(path, "cell_iterations.npy"), cells["iterations"].astype(np.float32))


def roofline_figures(args, g, cells, sms, launches, world):
    """Roofline of the dominant kernel (the cell solver launches of one step): FP64 and HBM, from this run's HIP-event
    kernel time and the committed counter passes under profiles/."""
    L = (cells["hi"] - cells["lo"]).astype(np.float64)
    nl = np.where(cells["i"] == cells["j"], 1, 2)
    bo = B_ODOM if g.dim == 2 else B_ODOM3
    alg_bytes = float((L * bo + nl * bo + 1.0 / 8).sum())
    # HBM traffic of the solver kernels from the committed rocprofv3 PMC passes of this same command
    # (FETCH_SIZE / WRITE_SIZE in KB, separate passes; FETCH_SIZE doubled per the gfx950 note on
    # those counters).  Per step, like `achieved`.
    traffic = None
    for rnd in ("r6_", "r5_", "r4_", ""):
        pmc_csv = os.path.join(ROOT, "profiles", "%spmc_hbm_%s.csv" % (rnd, args.workload))
        if os.path.exists(pmc_csv):
            break
    if os.path.exists(pmc_csv) and world == 1:
        import csv
        f = w = 0.0
        for r in csv.DictReader(open(pmc_csv)):
            if any(t in r["kernel"] for t in ("_cells_kernel", "_wave_kernel", "_pair_kernel", "_group_kernel", "_lds_kernel")):
                if r["counter"] == "FETCH_SIZE":
                    f += float(r["sum_value"])
                elif r["counter"] == "WRITE_SIZE":
                    w += float(r["sum_value"])
        traffic = (2.0 * f + w) * 1024.0
    pose_iters = float((L * cells["iterations"]).sum())
    survey_flops = pose_iters * F_SURVEY[g.dim]                 # 450 / 3000 flop per pose and outer iteration
    ex = executed_flops(args.workload, g.dim) if world == 1 else None
    # `achieved` / `frac`: EXECUTED FP64 flops of one step (counter pass of this workload, committed under profiles/) over
    # this run's HIP-event kernel time, when such a pass exists for the kernels of this build; otherwise SURVEY's model.
    use_ex = ex is not None and ex["current"] is not False
    ach_flops = ex["flops"] if use_ex else survey_flops
    achieved_tflops = ach_flops / (sms * 1e-3) / 1e12
    alg_tflops = survey_flops / (sms * 1e-3) / 1e12
    roofline = {"bound": "fp64-valu", "contract_bound": "mfma",
                "achieved": round(alg_tflops, 4), "peak": FP64_PEAK_TFLOPS,
                "unit": "TFLOP/s", "frac": round(alg_tflops / FP64_PEAK_TFLOPS, 5), "traffic": traffic,
                "frac_is": "ALGORITHMIC: SURVEY.md 8(d)'s K L F_d (pose_iterations_per_step x %g flop) / kernel_ms_per_step / peak; the executed "
                           "fraction of the counter pass is frac_executed" % F_SURVEY[g.dim],
                "achieved_executed": round(achieved_tflops, 4),
                "frac_executed_basis": ("executed FP64 flops (%s: SQ_INSTS_VALU_{FMA x2,MUL,ADD,TRANS}_F64 x 64 lanes of one solve of "
                               "this workload = %.4g) / kernel_ms_per_step / peak" % (ex["source"], ex["flops"])) if use_ex
                              else "SURVEY.md 8(d) model: pose_iterations_per_step x %g flop / kernel_ms_per_step / peak" % F_SURVEY[g.dim],
                "frac_survey_model": round(survey_flops / (sms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS, 5),
                "frac_executed": round(ex["flops"] / (sms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS, 5) if ex else None,
                "executed_fp64_flops_per_step": ex["flops"] if ex else None,
                "executed_pass_is_of_this_build": ex["current"] if ex else None,
                "mfma_mops_f64": ex["mfma_mops_f64"] if ex else None,
                "traffic_note": "HBM bytes per step of the solver kernels, %s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE "
                                "passes, FETCH doubled per the gfx950 note); mostly register-spill scratch, the chain itself "
                                "is L2-resident" % os.path.relpath(pmc_csv, ROOT),
                "kernel": "%s (%d launches per step, one per chain-length bin and loop count)" % (
                    "se2_wave_kernel<M,NL,STAGED> + se2_group_kernel<W,M,NL,STAGED> + se2_cells_kernel<W,M,NL>" if g.dim == 2
                    else "se3_lds_kernel<W,M,NL> (+ se3_cells_kernel<W,M,NL> beyond 2560 poses)", launches),
                "kernel_ms_per_step": round(sms, 4),
                "pose_iterations_per_step": pose_iters,
                "note": "compute-bound on the FP64 vector ALU (no MFMA-shaped products: SQ_INSTS_VALU_MFMA_MOPS_F64 = 0); "
                        "the contract's enum has no VALU entry, its 'mfma' roof for f64 is the same 78.6 TFLOP/s; the HBM "
                        "roof is far away, see roofline_hbm"}
    hbm_gbs = alg_bytes / (sms * 1e-3) / 1e9
    roofline_hbm = {"bound": "hbm", "achieved": round(hbm_gbs, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(hbm_gbs / HBM_PEAK_GBS, 6), "traffic": traffic,
                    "algorithmic_bytes_per_step": alg_bytes}
    return roofline, roofline_hbm


def full_measurements(args, out, g, cfg, eng, acc, cells, sms, launches, ms_per_step, rank, local_rank, world, barrier):
    """--full: everything beyond the headline -- roofline, single-shot first step, CPU baseline, the literal trial loop,
    the reference's own incremental metric, the set-only mode, configs[0] -- added to `out`."""
    import torch.distributed as dist
    from ipc_amd.consensus import IPC
    from ipc_amd.dist import EngineBackend, ShardedMatrix
    N = eng.N
    out["roofline"], out["roofline_hbm"] = roofline_figures(args, g, cells, sms, launches, world)
    if ms_per_step < 5000.0:
        # A SINGLE-SHOT matrix: a second engine of the same graph (kernels loaded, streams there), its FIRST step -- the two
        # planning passes with their host read-back, the buffers' hipMalloc, cells solved in list order (the repeated steps
        # above run on the cached cell lists, slow cells first, include/ipc_amd.h "stream contract").  All ranks take part.
        eng1 = IPC(g, cfg, device=local_rank)
        sm1 = ShardedMatrix(EngineBackend(eng1), rank, world)
        barrier()
        t0f = time.perf_counter()
        sm1.step()
        barrier()
        first_ms = (time.perf_counter() - t0f) * 1e3
        if world > 1:
            t = torch.tensor([first_ms], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            first_ms = float(t.item())
        _, acc1 = sm1.result()
        out["first_step_ms"] = first_ms
        out["first_step_same_accepted_set"] = bool(np.array_equal(acc1, acc))
        out["first_step_note"] = ("single-shot matrix on a fresh engine: planning passes + host read-back + buffer allocation + cells in list "
                                  "order; ms_per_step is a repeated step on the cached cell lists (slow cells first)")
        eng1.close()
    if rank == 0 and world == 1 and not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline(g, cfg, cells, args.cpu_seconds)
        gpu_solved_rate = len(cells) * 1.0 / (ms_per_step * 1e-3)
        out["cpu_baseline"]["gpu_solved_cells_per_s"] = gpu_solved_rate
        out["cpu_baseline"]["gpu_over_cpu_all_cores_on_solved_cells"] = gpu_solved_rate / out["cpu_baseline"]["value"]
        out["cpu_baseline"]["gpu_over_cpu_1_thread_on_solved_cells"] = gpu_solved_rate / out["cpu_baseline"]["single_thread"]["value"]
        if ms_per_step < 2500.0:
            # the same matrix by g2o's LITERAL trial loop (no convergence test: IPC_TERMINATE_EPS=0), i.e. the algorithm the
            # CPU baseline runs, on the GPU: the ratio on identical algorithms
            old_eps = os.environ.get("IPC_TERMINATE_EPS")
            os.environ["IPC_TERMINATE_EPS"] = "0"
            try:
                eng_lit = IPC(g, cfg, device=local_rank)
            finally:
                if old_eps is None:
                    del os.environ["IPC_TERMINATE_EPS"]
                else:
                    os.environ["IPC_TERMINATE_EPS"] = old_eps
            sm_lit = ShardedMatrix(EngineBackend(eng_lit), 0, 1)
            sm_lit.step()
            torch.cuda.synchronize()
            t0l = time.perf_counter()
            for _ in range(2):
                sm_lit.step()
            torch.cuda.synchronize()
            lit_ms = (time.perf_counter() - t0l) / 2 * 1e3
            _, acc_lit = sm_lit.result()
            eng_lit.close()
            out["cpu_baseline"]["gpu_literal_loop_ms_per_step"] = lit_ms
            out["cpu_baseline"]["gpu_literal_loop_same_accepted_set"] = bool(np.array_equal(acc_lit, acc))
            out["cpu_baseline"]["gpu_literal_loop_over_cpu_all_cores_on_solved_cells"] = (len(cells) / (lit_ms * 1e-3)) / out["cpu_baseline"]["value"]
            out["cpu_baseline"]["gpu_literal_loop_over_cpu_1_thread_on_solved_cells"] = (len(cells) / (lit_ms * 1e-3)) / out["cpu_baseline"]["single_thread"]["value"]
        n_inc = args.incremental_candidates
        if n_inc is None:
            n_inc = N if g.dim == 2 and args.workload in ("C1", "C2", "tiny", "T700") else 0
        elif n_inc < 0:
            n_inc = N
        if n_inc > 0:
            big = args.workload in ("C3", "C4", "C5")
            out["incremental"] = incremental_metric(g, cfg, eng, n_inc, args.cpu_seconds * 0.5, args.workload, reps=1 if big else 3)
    if rank == 0 and world == 1 and not args.no_set_only:
        # reported separately, never the headline: the accepted SET without the cells the set-max never reads
        # (ipc_run_set_only: diagonal cells first, then the pairs among the candidates whose own cell passed)
        eng.run_set_only()
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            acc_so, n_so = eng.run_set_only()
        eng.synchronize()
        t_so = (time.perf_counter() - t0) / 3
        out["set_only_mode"] = {"ms_per_run": t_so * 1e3, "solved_cells": int(n_so), "same_set_as_the_matrix": bool(np.array_equal(acc_so, acc)),
                                "note": "not the metric: no consistency matrix comes out of this mode, only the accepted set"}
    if rank == 0 and world == 1 and "incremental" in out and args.workload == "C2":
        # BASELINE configs[0], the reference's own CPU-runnable case (71 % accepted: a serial chain), timed last and with the
        # headline engine gone: every live engine holds streams, and beyond two dozen the runtime serialises them
        eng.close()
        out["incremental"]["configs0"] = faithful_run_of("C1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5, help="timed steps")
    ap.add_argument("--warmup", type=int, default=1, help="untimed steps before them")
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/*.npy (float32 / float64, at most ~36 MB; rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline, single-shot first step, CPU baseline, GPU "
                         "literal trial loop, the reference's incremental metric, set-only mode (minutes)")
    ap.add_argument("--cpu-seconds", type=float, default=30.0, help="(--full) CPU baseline budget")
    ap.add_argument("--no-cpu", action="store_true", help="(--full) skip the CPU baseline and the incremental metric")
    ap.add_argument("--no-set-only", action="store_true", help="(--full) skip the set-only side measurement")
    ap.add_argument("--incremental-candidates", type=int, default=None,
                    help="(--full) candidates of the faithful incremental mode to time (reference metric); -1: all of them (C4: minutes, "
                         "C5: tens of minutes -- one run instead of three); 0: none; default: all for C1 / C2 / tiny / T700 at 1 GPU, "
                         "none otherwise")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: run N ranks (one per GPU) under torch.distributed.run in a child process
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        sys.exit(subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                                  "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
                                  "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    import torch.distributed as dist
    from ipc_amd.consensus import IPC
    from ipc_amd.dist import EngineBackend, ShardedMatrix

    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world,
                                device_id=torch.device("cuda", local_rank))

    g, cfg, desc = build_workload(args.workload)
    eng = IPC(g, cfg, device=local_rank)               # chain + candidates now resident in HBM
    sm = ShardedMatrix(EngineBackend(eng), rank, world)
    N = eng.N
    n_cells_total = N * (N + 1) // 2

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        sm.step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sm.step()
    barrier()
    dt = time.perf_counter() - t0
    # per-step solver time from HIP events recorded on the launch stream (last step; --full's roofline)
    sms, launches = eng.solver_time_ms()
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt / args.steps * 1e3

    cells = eng.cell_info()                            # this rank's solved cells (of the last step)
    bits, acc = sm.result()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, bits, acc, cells, N)

    out = {
        "metric": "candidate-pairs/s (consistency matrix + set-max)",
        "value": n_cells_total * args.steps / dt,
        "unit": "candidate-pairs/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": "%s: %s; N=%d candidates, %d cells (i<=j), %d solved on rank 0, "
                               "s=%.0f, fast %.3f/%d, slow %.3f/%d" % (
                                   args.workload, desc, N, n_cells_total, len(cells), cfg.s_factor,
                                   cfg.fast_reject_th, cfg.fast_reject_iter_base, cfg.slow_reject_th,
                                   cfg.slow_reject_iter_base),
                   "parallelism": "rows%%%d + all-gather" % world if world > 1 else "1 GPU"},
        "accepted": int(acc.sum()),
    }
    out["solved_cells_rank0"] = int(len(cells))
    # cells whose intervals do not overlap cost nothing (C[i][j] = C[i][i] & C[j][j]): `value` counts them, as the metric
    # is defined over all N(N+1)/2 pairs; the rate over the cells that are actually solved is the one to compare with
    # cpu_baseline (which times solved cells only)
    out["solved_cells_per_s"] = len(cells) * 1.0 / (ms_per_step * 1e-3) if world == 1 else None
    out["free_cells_in_value"] = int(n_cells_total - len(cells)) if world == 1 else None
    if args.full:
        full_measurements(args, out, g, cfg, eng, acc, cells, sms, launches, ms_per_step, rank, local_rank, world, barrier)
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
