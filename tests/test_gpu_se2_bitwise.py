"""The SE(2) cell kernels compute the same bits as the build the digests were taken from.

Changes to the per-slot code of se2_wave_cell.hpp that do not touch the arithmetic (register residency, predicates,
address forms) must leave the packed consistency matrix, the accepted set and the per-cell chi2 bit-identical.
tests/golden/se2_bitwise_digests.json holds SHA-256 digests of the three arrays on two small workloads (`tiny`,
`T700`: wave, pair and quad kernels, one and two loops), taken from the commit before the dog-leg loop's address
and predicate forms were changed; that build gave the same digests in two separate runs.

    python tests/test_gpu_se2_bitwise.py OUT.json      # digests of the library in use (IPC_AMD_LIB selects it)
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "se2_bitwise_digests.json")
WORKLOADS = ("tiny", "T700")


def digests(workload):
    from bench import build_workload
    from ipc_amd.consensus import IPC
    g, cfg, _ = build_workload(workload)
    eng = IPC(g, cfg, device=0)
    bits, acc = eng.run()
    c = eng.cell_info()
    c = c[np.lexsort((c["j"], c["i"]))]

    def sha(a):
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

    return {"cells": int(len(c)), "matrix": sha(np.asarray(bits)), "accepted": sha(np.asarray(acc).astype(np.uint8)),
            "max_chi2": sha(c["max_chi2"].astype(np.float64)), "iterations": sha(c["iterations"].astype(np.int64))}


@pytest.mark.gpu
@pytest.mark.parametrize("workload", WORKLOADS)
def test_se2_outputs_bit_identical_to_pinned_build(workload):
    want = json.load(open(GOLDEN))["digests"][workload]
    got = digests(workload)
    for k in ("cells", "matrix", "accepted", "max_chi2", "iterations"):
        print(workload, k, got[k], "pinned", want[k])
    assert got == want


if __name__ == "__main__":
    out = {w: digests(w) for w in WORKLOADS}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))
