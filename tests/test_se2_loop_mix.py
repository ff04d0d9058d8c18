"""Static instruction mix of the dog-leg loop of one SE(2) pair kernel (tools/isa_loop_mix.py) against the table that
was committed before the loop's address and predicate forms were changed (profiles/r7_se2_loop_mix_before.txt):
the FP64 instruction count of the loop body is the arithmetic -- it must not move by one instruction -- and the
spill counts, the scratch size and the register-shuffling (AGPR copies + lane reads / writes) must not be above it."""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_loop_mix  # noqa: E402

BEFORE = os.path.join(ROOT, "profiles", "r7_se2_loop_mix_before.txt")


def test_classes():
    c = isa_loop_mix.classify
    assert c("\tv_fma_f64 v[0:1], v[2:3], v[4:5], v[6:7]") == "f64"
    assert c("\tv_cmp_lt_f64_e32 vcc, v[0:1], v[2:3]") == "f64_cmp"
    assert c("\tv_cvt_f64_i32_e32 v[0:1], v2") == "f64_cvt"
    assert c("\tv_accvgpr_read_b32 v1, a3") == "accvgpr"
    assert c("\tv_readlane_b32 s0, v255, 3") == "lane"
    assert c("\tv_mov_b32_dpp v1, v2 row_shr:1 row_mask:0xf bank_mask:0xf") == "dpp_mov"
    assert c("\tv_add_u32_e32 v1, 8, v2") == "v_int"
    assert c("\ts_and_saveexec_b64 s[0:1], vcc") == "salu"
    assert c("\tscratch_load_dword v1, off, off offset:4") == "scratch"
    assert c(".LBB0_1:") is None and c("\t; sched_barrier mask(0x00000000)") is None


@pytest.mark.skipif(not os.path.exists(isa_loop_mix.hipcc()), reason="hipcc is not installed: no assembly to count")
def test_p7_loop_body_against_the_committed_table():
    before = isa_loop_mix.parse_report(BEFORE)
    with tempfile.TemporaryDirectory() as d:
        rows = {r["kernel"]: r for r in isa_loop_mix.analyse(isa_loop_mix.build_asm("p7", d))}
    assert set(rows) == {k for k in before if k.startswith("p7/")}
    for k, r in sorted(rows.items()):
        b = before[k]
        print(k, {x: r[x] for x in ("f64_all", "valu", "copy_lane", "sgpr_spill_count", "vgpr_spill_count", "scratch_bytes")},
              "before", b)
        assert r["f64_all"] == b["f64_all"], "the FP64 instruction count of the loop body moved: the arithmetic was touched"
        assert r["vgpr_spill_count"] <= b["vgpr_spill_count"]
        assert r["sgpr_spill_count"] <= b["sgpr_spill_count"]
        assert r["scratch_bytes"] <= b["scratch_bytes"]
        assert r["copy_lane"] <= b["copy_lane"]
