"""The SE(2) wave / pair / quad kernels with 9 and 11 poses per lane compute the same bits as the build the digests
were taken from.

Those instantiations of se2_wave_cell.hpp park the odometry errors of the committed state in accumulator registers
(written by phase A of a dog-leg iteration, read by phases B1 and C) where the pinned build recomputed them from the
poses in each phase, and w11 fetches its slot constants one slot ahead.  The parked value is the recomputed one --
the same se2_error on the same poses and constants -- so no output may move by a bit.  The cases drive each
instantiation family:

    tiny-w9 .. tiny-q11   V = 300 under a one-variant policy: idle lanes, and idle second / later waves for p and q
    t700-w              T700 under w9,w11: every lane of the wave holds poses
    v1400-p             V = 1400, 10 true loops + 10 outliers, under p9,p11: both waves hold poses and loop ends
    unstaged            V = 2100 under the default policy: the chain constants do not fit the LDS (STAGED = false)

tests/golden/se2_keep_errors_digests.json holds SHA-256 digests of the packed matrix, the accepted set, max_chi2,
iterations and the per-cell flags, taken from the parent commit's library; that build gave the same digests in two
separate runs.

    python tests/test_gpu_se2_keep_errors_bitwise.py OUT.json    # digests of the library in use (IPC_AMD_LIB selects it)
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "se2_keep_errors_digests.json")
POLICY_VAR = "IPC_SE2_POLICY"
# case -> policy (None: the default policy)
CASES = {"tiny-w9": "w9", "tiny-w11": "w11", "tiny-p9": "p9", "tiny-p11": "p11", "tiny-q9": "q9", "tiny-q11": "q11",
         "t700-w": "w9,w11", "v1400-p": "p9,p11", "unstaged": None}
UNSTAGED_V = 2100
PAIR_V = 1400


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
        g = synth.inject_outliers(synth._se2_graph(PAIR_V, 10, seed=21, laps=5.0), 10, seed=22)
        return g, Config()
    g = synth.inject_outliers(synth._se2_graph(UNSTAGED_V, 12, seed=11, laps=6.0), 20, seed=12)
    return g, Config()


def digests(case):
    from ipc_amd.consensus import IPC
    g, cfg = case_graph(case)
    old = os.environ.get(POLICY_VAR)
    try:
        if CASES[case] is None:
            os.environ.pop(POLICY_VAR, None)
        else:
            os.environ[POLICY_VAR] = CASES[case]
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
    c = c[np.lexsort((c["j"], c["i"]))]

    def sha(a):
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

    return {"cells": int(len(c)), "matrix": sha(np.asarray(bits)), "accepted": sha(np.asarray(acc).astype(np.uint8)),
            "max_chi2": sha(c["max_chi2"].astype(np.float64)), "iterations": sha(c["iterations"].astype(np.int64)),
            "flags": sha(c["flags"].astype(np.int64)), "long_cells": int(rep["long_cells"]),
            "max_chain": int((c["hi"] - c["lo"]).max())}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_kept_errors_bit_identical_to_pinned_build(case):
    want = json.load(open(GOLDEN))["digests"][case]
    got = digests(case)
    for k in sorted(got):
        print(case, k, got[k], "pinned", want[k])
    assert got == want
    assert got["long_cells"] == 0                    # every cell went through a wave / pair / quad / block kernel
    if case == "t700-w":
        assert got["max_chain"] > 64 * 9             # some cells are beyond w9: w11 runs too
    if case == "v1400-p":
        assert got["max_chain"] > 128 * 9            # ... beyond p9: p11 runs, and its second wave holds poses


if __name__ == "__main__":
    out = {w: digests(w) for w in CASES}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))
