"""Static instruction mix of the dog-leg loop of the p9 pair kernels (tools/isa_loop_mix.py) against the tables that
were committed with the change that keeps their committed odometry errors parked in accumulator registers
(profiles/se2_keep_errors_loop_mix_{before,after}.txt).

Against the "after" table, by the rules of tests/test_se2_loop_mix.py: the FP64 instruction count of the loop body is
the arithmetic and must not move by one instruction; spill counts, scratch size and the register shuffling (AGPR
copies + lane reads / writes, the hand-written parking copies among them) must not be above it.  Against the "before"
table: what the stored errors are for -- fewer FP64 instructions and fewer VALU instructions in the loop body than the
build that recomputed them, and no more scratch."""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_loop_mix  # noqa: E402

BEFORE = os.path.join(ROOT, "profiles", "se2_keep_errors_loop_mix_before.txt")
AFTER = os.path.join(ROOT, "profiles", "se2_keep_errors_loop_mix_after.txt")
KEYS = ("f64_all", "valu", "copy_lane", "sgpr_spill_count", "vgpr_spill_count", "scratch_bytes")


def test_committed_tables_hold_the_same_kernels():
    before, after = isa_loop_mix.parse_report(BEFORE), isa_loop_mix.parse_report(AFTER)
    assert set(before) == set(after) and len(after) == 24      # six units, NL = 1 / 2, staged / unstaged
    for k in sorted(after):
        a, b = after[k], before[k]
        if a["f64_all"] != b["f64_all"]:                       # an instantiation that keeps its errors
            assert k.split("/")[0] in ("w9", "p9", "w11", "p11"), k
            assert a["f64_all"] < b["f64_all"] and a["valu"] < b["valu"] and a["scratch_bytes"] <= b["scratch_bytes"], k
        else:                                                   # every other one: untouched
            assert a == b, k
    assert all(after[k]["f64_all"] < before[k]["f64_all"] for k in after if k.startswith("p9/"))


@pytest.mark.skipif(not os.path.exists(isa_loop_mix.hipcc()), reason="hipcc is not installed: no assembly to count")
def test_p9_loop_body_against_the_committed_tables():
    before, after = isa_loop_mix.parse_report(BEFORE), isa_loop_mix.parse_report(AFTER)
    with tempfile.TemporaryDirectory() as d:
        rows = {r["kernel"]: r for r in isa_loop_mix.analyse(isa_loop_mix.build_asm("p9", d))}
    assert set(rows) == {k for k in after if k.startswith("p9/")}
    for k, r in sorted(rows.items()):
        a, b = after[k], before[k]
        print(k, {x: r[x] for x in KEYS}, "after", a, "before", b)
        assert r["f64_all"] == a["f64_all"], "the FP64 instruction count of the loop body moved: the arithmetic was touched"
        assert r["vgpr_spill_count"] <= a["vgpr_spill_count"]
        assert r["sgpr_spill_count"] <= a["sgpr_spill_count"]
        assert r["scratch_bytes"] <= a["scratch_bytes"]
        assert r["copy_lane"] <= a["copy_lane"]
        assert r["f64_all"] < b["f64_all"] and r["valu"] < b["valu"] and r["scratch_bytes"] <= b["scratch_bytes"]
