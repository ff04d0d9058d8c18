"""The kept-trial SE(2) wave / pair kernels (policy tokens kwM / kpM) compute the same bits as the wave / pair kernels
of the same M (wM / pM), cell by cell.

A kept-trial kernel parks the pose every trial sweep forms in each slot (and for M <= 8 the slot's error) in accumulator
registers and commits an accepted trial by reading them back; the other kernel throws the trial's poses away and
re-sweeps an accepted trial with the same coefficients.  The parked value is what the second sweep recomputes, so no
output may move by a bit.  Both kernels are in the one library, so every case builds the engine twice in this process,
under the old token and under the k token, and compares EVERY solved cell -- packed matrix, accepted set, max_chi2,
chi2_total, iterations, tries, flags, evals -- with array_equal.  No digests of another build.

    tiny-w5 .. tiny-p11   V = 300 under a one-variant policy: idle lanes, and an idle second wave for p
    t700-w                T700 under w9,w11 against kw9,kw11: every lane of the wave holds poses
    v1400-p               V = 1400, 10 true loops + 40 outliers, under p9,p11 against kp9,kp11: both waves hold poses and
                          loop ends; the boundary pose crosses the mailbox in the trial and no longer in the commit
    unstaged              V = 2100 (12 true loops + 60 outliers) under the previous default policy against the shipped default (policy unset) and against
                          the policy with every kept-trial kernel: the chain constants do not fit the LDS (STAGED = false)

Each case must contain what it is for: cells where a rejected trial came before an accepted one (tries > iterations: the
parked pose was overwritten before it was used), cells with more evaluations than iterations, and a cell that ran to
its iteration cap.  (With the 10 and 20 outliers of tests/test_gpu_se2_keep_errors_bitwise.py the last two graphs hold no
cell at its cap under the old kernels; with 40 and 60 they hold two each.)

Shown once to be able to fail: a build whose trial sweep parks Y.th before the angle wrap fails these cases.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
POLICY_VAR = "IPC_SE2_POLICY"
# the default policy before the kept-trial kernels existed, and the same with every kept-trial kernel in place
OLD_DEFAULT = "w1,w3,w5,w7,w9,w11,w13,p7,p9,p11,q7,q9,q11,q13,16x4,16x8,16x16"
ALL_KEPT = "w1,w3,kw5,kw7,kw9,kw11,w13,kp7,kp9,kp11,q7,q9,q11,q13,16x4,16x8,16x16"
# case -> (policy of the old kernels, [policies of the kept-trial kernels]); None: the shipped default (variable unset)
CASES = {
    "tiny-w5": ("w5", ["kw5"]), "tiny-w7": ("w7", ["kw7"]), "tiny-w9": ("w9", ["kw9"]),
    "tiny-p7": ("p7", ["kp7"]), "tiny-p9": ("p9", ["kp9"]), "tiny-p11": ("p11", ["kp11"]),
    "t700-w": ("w9,w11", ["kw9,kw11"]),
    "v1400-p": ("p9,p11", ["kp9,kp11"]),
    "unstaged": (OLD_DEFAULT, [None, ALL_KEPT]),
}
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
    if case == "t700-w":
        g, cfg, _ = build_workload("T700")
        return g, cfg
    if case == "v1400-p":
        g = synth.inject_outliers(synth._se2_graph(PAIR_V, 10, seed=21, laps=5.0), 40, seed=22)
        return g, Config()
    g = synth.inject_outliers(synth._se2_graph(UNSTAGED_V, 12, seed=11, laps=6.0), 60, seed=12)
    return g, Config()


def solve(g, cfg, policy):
    """(packed matrix, accepted set, per-cell records sorted by (i, j), solve report) under a policy string."""
    from ipc_amd.consensus import IPC
    old = os.environ.get(POLICY_VAR)
    try:
        if policy is None:
            os.environ.pop(POLICY_VAR, None)
        else:
            os.environ[POLICY_VAR] = policy
        eng = IPC(g, cfg, device=0)
        bits, acc = eng.run()
        c = eng.cell_info()
        rep = eng.solve_report()
        eng.close()
    finally:
        if old is None:
            os.environ.pop(POLICY_VAR, None)
        else:
            os.environ[POLICY_VAR] = old
    return np.asarray(bits).copy(), np.asarray(acc).copy(), c[np.lexsort((c["j"], c["i"]))], rep


def coverage(c, cfg):
    """What the cells of a run exercise: (cells with tries > iterations, cells with evals - 1 - iterations > 0, cells at
    their iteration cap).  The cap is that of the kernels (consensus_utils.cpp:12-13)."""
    nl = np.where(c["i"] == c["j"], 1, 2)
    base = np.where(nl == 1, cfg.fast_reject_iter_base, cfg.slow_reject_iter_base)
    cap = np.where((c["hi"] - c["lo"]) + nl > 100, 5 * base, base)
    return (int((c["tries"] > c["iterations"]).sum()), int((c["evals"] - 1 - c["iterations"] > 0).sum()),
            int((c["iterations"] == cap).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_kept_trial_bit_identical_to_resweep(case):
    g, cfg = case_graph(case)
    old_policy, kept_policies = CASES[case]
    bits0, acc0, c0, rep0 = solve(g, cfg, old_policy)
    cov = coverage(c0, cfg)
    print(case, "old", old_policy, "cells", len(c0), "tries > iterations", cov[0], "evals - 1 - iterations > 0", cov[1],
          "at the iteration cap", cov[2], "max chain", int((c0["hi"] - c0["lo"]).max()))
    assert rep0["long_cells"] == 0                   # every cell went through a wave / pair / quad / block kernel
    assert cov[0] > 0 and cov[1] > 0 and cov[2] > 0, "the case does not exercise what it is for"
    if case == "t700-w":
        assert (c0["hi"] - c0["lo"]).max() > 64 * 9      # some cells are beyond w9: (k)w11 runs too
    if case == "v1400-p":
        assert (c0["hi"] - c0["lo"]).max() > 128 * 9     # ... beyond p9: (k)p11 runs, and its second wave holds poses
    for pol in kept_policies:
        bits1, acc1, c1, rep1 = solve(g, cfg, pol)
        print(case, "kept", pol, "cells", len(c1))
        assert rep1["long_cells"] == 0
        assert len(c1) == len(c0)
        assert np.array_equal(bits0, bits1), "packed consistency matrix"
        assert np.array_equal(acc0, acc1), "accepted set"
        for f in FIELDS:
            a, b = c0[f], c1[f]
            if a.dtype.kind == "f":                  # bit patterns: NaN equals NaN, -0.0 differs from 0.0
                a, b = a.astype(np.float64).view(np.uint64), b.astype(np.float64).view(np.uint64)
            bad = np.nonzero(a != b)[0]
            assert np.array_equal(a, b), "%s differs in %d of %d cells, first (i, j) = (%d, %d)" % (
                f, len(bad), len(a), c0["i"][bad[0]], c0["j"][bad[0]])
