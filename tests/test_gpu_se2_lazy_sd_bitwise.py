"""The lazy steepest-descent SE(2) wave / pair kernels (se2_wave_kernel_lz / se2_group_kernel_lz, LAZY_SD of se2_wave_solve)
compute the same bits as the kernels whose bins they serve, cell by cell.

A lazy kernel forms b^T H b, alpha and |h_sd| only in the iterations whose trial loop reads them (the first trial is not
Gauss-Newton, or a Gauss-Newton trial was rejected and the loop goes on), through the same expressions and the same
reduction order as phases B1 / B2 of the other kernels.  IPC_SE2_LAZY_SD=0 makes every policy token launch the kernel it
names; =1 (the default) serves those of kw5 kw7 kw9 w11 w13 kp7 kp9 p11 by their lazy forms that the engine's compiled-in
list names (kLazySdWaveM / kLazySdPairM, cell_plan.hpp: the kernels through the static and the measured gate); =2 serves all
eight, listed or not, so that a kernel outside the list is held to the same bits.  All in the one library, so every case
builds the engine in this process under =0, under =1 and, where =1 leaves a kernel of the case out, under =2, and compares
EVERY solved cell -- packed matrix, accepted set, max_chi2,
chi2_total, iterations, tries, flags, evals -- with array_equal on bit patterns.  No digests of another build.

    tiny-kw5 .. tiny-p11  V = 300 under a one-variant policy: idle lanes, and an idle second wave for the pairs
    t700                  T700 under the default policy
    v1400-p               V = 1400, 10 true loops + 40 outliers, under kp9,p11: both waves hold poses and loop ends, and
                          both must enter sd_terms together
    unstaged              V = 2100 (12 true loops + 60 outliers) under the default policy: the chain constants do not fit
                          the LDS (STAGED = false)

Each case must contain what it is for: cells with tries > iterations and more trial sweeps than iterations (a rejection
made sd_terms run after a Gauss-Newton trial or between trials), cells where every iteration took its first trial (the
block may never have run), a cell at its iteration cap; and the engine's launch counter must show that the lazy kernels
ran under =2, under =1 where the list names one of the case's kernels, and not under =0.

Shown once to be able to fail, on two builds with one line changed each: one that runs sd_terms() only before the
first trial of an iteration (`if (numTries == 1)` in front of the check: none after a rejected Gauss-Newton trial) fails all
eleven cases, max_chi2 differing in 99 to 698 cells per case; one that reduces the lazy b^T H b with wave_sum instead of
wave_sum16_entry1 fails all eleven, 49 to 97 cells per case.
"""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
POLICY_VAR, LAZY_VAR = "IPC_SE2_POLICY", "IPC_SE2_LAZY_SD"
# case -> policy (None: the shipped default, variable unset)
CASES = {
    "tiny-kw5": "kw5", "tiny-kw7": "kw7", "tiny-kw9": "kw9", "tiny-kp7": "kp7", "tiny-kp9": "kp9",
    "tiny-w11": "w11", "tiny-w13": "w13", "tiny-p11": "p11",
    "t700": None,
    "v1400-p": "kp9,p11",
    "unstaged": None,
}
UNSTAGED_V = 2100
PAIR_V = 1400
# policy token -> the lazy kernel that serves it (tags of tools/isa_loop_mix.py)
LAZY_OF = {"kw5": "lw5", "kw7": "lw7", "kw9": "lw9", "w11": "lw11", "w13": "lw13", "kp7": "lp7", "kp9": "lp9", "p11": "lp11"}
FIELDS = ("i", "j", "lo", "hi", "max_chi2", "chi2_total", "iterations", "tries", "flags", "evals")


def case_graph(case):
    from bench import build_workload
    from ipc_amd import synth
    from ipc_amd.consensus import Config
    if case.startswith("tiny"):
        g, cfg, _ = build_workload("tiny")
        return g, cfg
    if case == "t700":
        g, cfg, _ = build_workload("T700")
        return g, cfg
    if case == "v1400-p":                            # the graphs of tests/test_gpu_se2_kept_trial_bitwise.py
        g = synth.inject_outliers(synth._se2_graph(PAIR_V, 10, seed=21, laps=5.0), 40, seed=22)
        return g, Config()
    g = synth.inject_outliers(synth._se2_graph(UNSTAGED_V, 12, seed=11, laps=6.0), 60, seed=12)
    return g, Config()


def compiled_in():
    """Tags of the lazy kernels the engine substitutes under IPC_SE2_LAZY_SD=1 (kLazySdWaveM / kLazySdPairM, cell_plan.hpp)."""
    src = open(os.path.join(ROOT, "ipc_amd", "csrc", "cell_plan.hpp")).read()
    tags = set()
    for name, pre in (("kLazySdWaveM", "lw"), ("kLazySdPairM", "lp")):
        m = re.search(r"static const int %s\[\] = \{([^}]*)\}" % name, src)
        tags |= {pre + x.strip() for x in m.group(1).split(",") if x.strip() and int(x) > 0}
    return tags


def solve(g, cfg, policy, lazy):
    """(packed matrix, accepted set, per-cell records sorted by (i, j), solve report, lazy launches) under a policy string
    and a setting of IPC_SE2_LAZY_SD."""
    from ipc_amd.consensus import IPC
    old = {k: os.environ.get(k) for k in (POLICY_VAR, LAZY_VAR)}
    try:
        if policy is None:
            os.environ.pop(POLICY_VAR, None)
        else:
            os.environ[POLICY_VAR] = policy
        os.environ[LAZY_VAR] = lazy
        eng = IPC(g, cfg, device=0)
        bits, acc = eng.run()
        c = eng.cell_info()
        rep = eng.solve_report()
        n_lazy = eng.lazy_sd_launches()
        eng.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return np.asarray(bits).copy(), np.asarray(acc).copy(), c[np.lexsort((c["j"], c["i"]))], rep, n_lazy


def coverage(c, cfg):
    """(cells with tries > iterations, cells with more trial sweeps than iterations: a trial was rejected and another one
    swept, cells with as many trial sweeps as iterations: every iteration took its first trial, cells at their iteration
    cap).  evals counts the initial sweep and every trial sweep; tries alone does not tell a rejection, a cell that stops
    on the convergence test books g2o's whole trial budget.  The cap is that of the kernels (consensus_utils.cpp:12-13)."""
    nl = np.where(c["i"] == c["j"], 1, 2)
    base = np.where(nl == 1, cfg.fast_reject_iter_base, cfg.slow_reject_iter_base)
    cap = np.where((c["hi"] - c["lo"]) + nl > 100, 5 * base, base)
    return (int((c["tries"] > c["iterations"]).sum()), int((c["evals"] - 1 - c["iterations"] > 0).sum()),
            int((c["evals"] - 1 == c["iterations"]).sum()), int((c["iterations"] == cap).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_lazy_sd_bit_identical_to_eager(case):
    g, cfg = case_graph(case)
    policy = CASES[case]
    bits0, acc0, c0, rep0, lazy0 = solve(g, cfg, policy, "0")
    cov = coverage(c0, cfg)
    print(case, "policy", policy, "cells", len(c0), "tries > iterations", cov[0], "a trial rejected", cov[1],
          "every first trial taken", cov[2], "at the iteration cap", cov[3], "max chain", int((c0["hi"] - c0["lo"]).max()), "lazy launches", lazy0)
    assert rep0["long_cells"] == 0                   # every cell went through a wave / pair / quad / block kernel
    assert cov[0] > 0 and cov[1] > 0 and cov[2] > 0 and cov[3] > 0, "the case does not exercise what it is for"
    if case == "v1400-p":
        assert (c0["hi"] - c0["lo"]).max() > 128 * 9     # beyond kp9: p11 runs, and its second wave holds poses
    assert lazy0 == 0, "IPC_SE2_LAZY_SD=0 launched a lazy kernel"
    tags = {LAZY_OF[t] for t in (policy.split(",") if policy else LAZY_OF)}     # the lazy kernels the case can reach
    listed = compiled_in()
    for setting in ["1"] + ([] if tags <= listed else ["2"]):
        bits1, acc1, c1, rep1, lazy1 = solve(g, cfg, policy, setting)
        print(case, "lazy launches under =%s:" % setting, lazy1)
        if setting == "2" or (tags & listed):
            assert lazy1 > 0, "IPC_SE2_LAZY_SD=%s launched no lazy kernel" % setting
        else:
            assert lazy1 == 0, "IPC_SE2_LAZY_SD=1 launched a lazy kernel outside the compiled-in list"
        assert rep1["long_cells"] == 0
        assert len(c1) == len(c0)
        assert np.array_equal(bits0, bits1), "packed consistency matrix"
        assert np.array_equal(acc0, acc1), "accepted set"
        for f in FIELDS:
            a, b = c0[f], c1[f]
            if a.dtype.kind == "f":                  # bit patterns: NaN equals NaN, -0.0 differs from 0.0
                a, b = a.astype(np.float64).view(np.uint64), b.astype(np.float64).view(np.uint64)
            bad = np.nonzero(a != b)[0]
            assert np.array_equal(a, b), "%s differs in %d of %d cells, first (i, j) = (%d, %d) under =%s" % (
                f, len(bad), len(a), c0["i"][bad[0]], c0["j"][bad[0]], setting)
