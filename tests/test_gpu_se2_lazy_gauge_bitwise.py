"""The lazy steepest-descent SE(2) kernels at M = 9 (lw9, lp9: se2_wave_kernel_lz<9, ..> / se2_group_kernel_lz<2, 9, ..>)
hold the gauge pose -- pose 0 of the cell -- in accumulator registers, parked by hand once per cell and read back at every
use (PARK_GAUGE of se2_wave_solve), and the engine serves the bins of kw9 and kp9 by them by default.  They compute the
same bits as kw9 and kp9, cell by cell.

Every case builds the engine in this process under IPC_SE2_LAZY_SD=0 (every policy token launches the kernel it names) and
under =1 (the compiled-in list, kLazySdWaveM / kLazySdPairM of cell_plan.hpp) and compares EVERY solved cell -- packed matrix,
accepted set, max_chi2, chi2_total, iterations, tries, flags, evals -- with array_equal on bit patterns.  Never =2: a kernel
that is not listed is an error here, the launch counter under =1 must be above zero.

    tiny-kw9    V = 300 under policy kw9: one wave per cell, idle lanes
    tiny-kp9    V = 300 under policy kp9: the second wave of every pair is idle
    v1400-p     V = 1400, 10 true loops + 40 outliers, under kp9,p11: both waves of a pair hold poses, and the second
                wave's predecessor pose is the mailbox value, not the gauge
    unstaged    V = 2100, 12 true loops + 60 outliers, under the default policy: the chain constants do not fit the LDS
    v1400-p7    the V = 1400 graph under kp7,kp9,p11: lp7, whose "terms formed" flag is a bit of its flags word (SD_BIT of
                se2_wave_solve), with poses in both waves; the bit must not reach the cells' flags

A parked gauge that came back as zeros would go unnoticed in a cell whose chain starts at the origin (pose 0 of the graph
is the identity).  So every case must hold solved cells with lo > 0, among them one with more trial sweeps than iterations
(sd_terms() ran and read the parked pose for lane 0's predecessor) and one at its iteration cap; and the CPU test below
shows from the graphs alone that most cells of every case start away from pose 0.

Shown once to be able to fail, on a build that is not kept: with phase B1's read of gauge.x returning the
parked gauge.y all five cases fail, max_chi2 differing in 233 to 1584 cells per case.
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
CASES = {"tiny-kw9": "kw9", "tiny-kp9": "kp9", "v1400-p": "kp9,p11", "unstaged": None, "v1400-p7": "kp7,kp9,p11"}
UNSTAGED_V = 2100
PAIR_V = 1400
FIELDS = ("i", "j", "lo", "hi", "max_chi2", "chi2_total", "iterations", "tries", "flags", "evals")


def case_graph(case):
    from bench import build_workload
    from ipc_amd import synth
    from ipc_amd.consensus import Config
    if case.startswith("tiny"):
        g, cfg, _ = build_workload("tiny")
        return g, cfg
    if case.startswith("v1400"):                     # the graphs of tests/test_gpu_se2_lazy_sd_bitwise.py
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
        assert m, name
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


def test_the_engine_lists_lw9_lp9_and_lp7():
    assert {"lw9", "lp9", "lp7"} <= compiled_in()


@pytest.mark.parametrize("case", list(CASES))
def test_most_cells_start_away_from_pose_zero(case):
    """From the graph alone: a cell (i, j) spans the poses of its two loops, so its gauge is the lowest end point of the
    two.  Pose 0 is the identity; every other pose of these trajectories is away from it in x, y or theta."""
    g, _ = case_graph(case)
    first = np.asarray(g.loop_ids).min(axis=1)
    i, j = np.triu_indices(len(first))
    lo = np.minimum(first[i], first[j])
    share = float((lo > 0).mean())
    print(case, "cells", len(lo), "with lo > 0", int((lo > 0).sum()), "share %.3f" % share)
    assert share > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_parked_gauge_bit_identical_to_eager(case):
    g, cfg = case_graph(case)
    policy = CASES[case]
    bits0, acc0, c0, rep0, lazy0 = solve(g, cfg, policy, "0")
    nl = np.where(c0["i"] == c0["j"], 1, 2)
    base = np.where(nl == 1, cfg.fast_reject_iter_base, cfg.slow_reject_iter_base)
    cap = np.where((c0["hi"] - c0["lo"]) + nl > 100, 5 * base, base)      # the kernels' cap (consensus_utils.cpp:12-13)
    away = c0["lo"] > 0
    rejected = away & (c0["evals"] - 1 - c0["iterations"] > 0)            # evals: the initial sweep and every trial sweep
    capped = away & (c0["iterations"] == cap)
    print(case, "policy", policy, "cells", len(c0), "lo > 0", int(away.sum()), "of them a trial rejected", int(rejected.sum()),
          "at the iteration cap", int(capped.sum()), "max chain", int((c0["hi"] - c0["lo"]).max()))
    assert rep0["long_cells"] == 0                   # every cell went through a wave / pair / quad / block kernel
    assert 2 * int(away.sum()) > len(c0), "most cells of the case should start away from pose 0"
    assert rejected.any() and capped.any(), "the case does not exercise what it is for"
    if case == "v1400-p":
        assert (c0["hi"] - c0["lo"]).max() > 128 * 9     # beyond kp9: p11 runs, and the second wave of kp9 cells holds poses
        assert ((c0["hi"] - c0["lo"] > 64 * 9) & (c0["hi"] - c0["lo"] <= 128 * 9) & away).any()
    if case == "v1400-p7":                           # kp7 cells with poses in the second wave
        assert ((c0["hi"] - c0["lo"] > 64 * 7) & (c0["hi"] - c0["lo"] <= 128 * 7) & away).any()
    assert lazy0 == 0, "IPC_SE2_LAZY_SD=0 launched a lazy kernel"
    bits1, acc1, c1, rep1, lazy1 = solve(g, cfg, policy, "1")
    print(case, "lazy launches under =1:", lazy1)
    assert lazy1 > 0, "IPC_SE2_LAZY_SD=1 launched no lazy kernel"
    assert rep1["long_cells"] == 0
    assert len(c1) == len(c0)
    assert np.array_equal(bits0, bits1), "packed consistency matrix"
    assert np.array_equal(acc0, acc1), "accepted set"
    for f in FIELDS:
        a, b = c0[f], c1[f]
        if a.dtype.kind == "f":                      # bit patterns: NaN equals NaN, -0.0 differs from 0.0
            a, b = a.astype(np.float64).view(np.uint64), b.astype(np.float64).view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert np.array_equal(a, b), "%s differs in %d of %d cells, first (i, j) = (%d, %d)" % (
            f, len(bad), len(a), c0["i"][bad[0]], c0["j"][bad[0]])
