"""The capacitance solve of the SE(2) wave / pair / quad kernels computes the same bits as the build the digests were
taken from.

Phase B of se2_wave_cell.hpp (Gamma, the assembly of S, the Gauss-Jordan pivots, nu, alpha / hsdNorm) is compiled per
(NL, W, STAGED) and its data movement differs with W; tests/test_gpu_se2_bitwise.py reaches it mostly through the wave
kernels.  The cases here drive it through one variant family each:

    tiny-w1, tiny-w5   one wave per cell (w1: eight waves per CU; the chains beyond 64 poses go to w5)
    tiny-p5            two waves per cell
    tiny-q7            four waves per cell
    unstaged           V = 2100: the chain constants do not fit the LDS, the kernels run STAGED = false (default policy)
    nan-edge           one odometry edge with NaN information: the solve leaves through its non-positive / NaN pivot exit

tests/golden/se2_capsolve_digests.json holds SHA-256 digests of the packed matrix, the accepted set, max_chi2,
iterations and the per-cell flags, taken from the parent commit's library; that build gave the same digests in two
separate runs.  In the nan-edge case the parent leaves `flags2_cells` cells through `flags & 2` (the count is pinned
and asserted positive, so the exit is in the pinned set).

    python tests/test_gpu_capsolve_bitwise.py OUT.json    # digests of the library in use (IPC_AMD_LIB selects it)
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "se2_capsolve_digests.json")
POLICY_VAR = "IPC_SE2_POLICY"
# case -> policy (None: the default policy)
CASES = {"tiny-w1": "w1,w5", "tiny-w5": "w5", "tiny-p5": "p5", "tiny-q7": "q7", "unstaged": None, "nan-edge": None}
UNSTAGED_V = 2100


def case_graph(case):
    from bench import build_workload
    from ipc_amd import synth
    from ipc_amd.consensus import Config
    if case.startswith("tiny"):
        g, cfg, _ = build_workload("tiny")
        return g, cfg
    if case == "unstaged":
        g = synth.inject_outliers(synth._se2_graph(UNSTAGED_V, 12, seed=11, laps=6.0), 20, seed=12)
        return g, Config()
    g = synth.inject_outliers(synth.small_se2(), 6, seed=3)
    oi = g.odom_info.copy()
    oi[40] = np.nan
    g.odom_info = oi
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
            "flags": sha(c["flags"].astype(np.int64)), "flags2_cells": int(((c["flags"] & 2) != 0).sum()),
            "long_cells": int(rep["long_cells"])}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_capacitance_solve_bit_identical_to_pinned_build(case):
    want = json.load(open(GOLDEN))["digests"][case]
    got = digests(case)
    for k in sorted(got):
        print(case, k, got[k], "pinned", want[k])
    assert got == want
    assert got["long_cells"] == 0                    # every cell went through a wave / pair / quad / block kernel
    if case == "nan-edge":
        assert got["flags2_cells"] > 0, "no cell left through the non-positive / NaN pivot exit"


if __name__ == "__main__":
    out = {w: digests(w) for w in CASES}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))
