"""Static gate of the kept-trial SE(2) kernels (se2_wave_kernel_kt / se2_group_kernel_kt, policy tokens kwM / kpM), from
gfx950 assembly (tools/isa_loop_mix.py) and the committed table profiles/se2_kept_trial_loop_mix.txt.

A kept-trial kernel parks the trial's poses in accumulator registers and reads an accepted trial back instead of
sweeping the chain a second time.  Against its counterpart (w9 for kw9, p9 for kp9 ...) IN THE SAME BUILD, for every
NL / staged combination:
    * no scratch;
    * no more spilled vector registers than the counterpart;
    * fewer FP64 instructions in the dog-leg loop body -- and the same number fewer in all four combinations, a multiple
      of M: one commit-sweep slot (both its small-rotation and its full-sincos branch) times M, nothing left of it
      (68 per slot where the commit also re-evaluated the error, M = 5 and 7; 51 per slot at M = 9 and 11).
The default policy (kDefaultPolicy, cell_plan.hpp) names a kept-trial kernel only where the table shows all four of its
combinations through this gate.  The translation units of the old kernels must emit the old kernels only, and the new
units the new kernels only; tests/test_se2_loop_mix.py and tests/test_se2_keep_errors_loop_mix.py hold the old kernels'
loop bodies to their own tables."""
import os
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_loop_mix  # noqa: E402

TABLE = os.path.join(ROOT, "profiles", "se2_kept_trial_loop_mix.txt")
COMBOS = ("nl1/staged", "nl1/unstaged", "nl2/staged", "nl2/unstaged")
KEPT = ("kw5", "kw7", "kw9", "kw11", "kp7", "kp9", "kp11")


def gate(kept, old):
    """Why a kept-trial kernel fails the static gate against its counterpart ([]: it passes)."""
    why = []
    if kept["scratch_bytes"] != 0:
        why.append("scratch %d B" % kept["scratch_bytes"])
    if kept["vgpr_spill_count"] > old["vgpr_spill_count"]:
        why.append("vgpr_spill %d > %d" % (kept["vgpr_spill_count"], old["vgpr_spill_count"]))
    if not kept["f64_all"] < old["f64_all"]:
        why.append("FP64 %d >= %d" % (kept["f64_all"], old["f64_all"]))
    return why


def default_policy():
    src = open(os.path.join(ROOT, "ipc_amd", "csrc", "cell_plan.hpp")).read()
    return re.search(r'kDefaultPolicy = "([^"]+)"', src).group(1).split(",")


def test_committed_table_and_default_policy():
    t = isa_loop_mix.parse_report(TABLE)
    assert len(t) == 4 * 2 * len(KEPT)               # every kept-trial unit and its counterpart, four combinations each
    passes = {}
    for tag in KEPT:
        m = int(tag[2:])
        why = {c: gate(t["%s/%s" % (tag, c)], t["%s/%s" % (tag[1:], c)]) for c in COMBOS}
        passes[tag] = not any(why.values())
        print(tag, "passes" if passes[tag] else "fails: %s" % {c: w for c, w in why.items() if w})
        # the second sweep is gone without residue, in every combination, whether or not the kernel passes
        drop = {t["%s/%s" % (tag[1:], c)]["f64_all"] - t["%s/%s" % (tag, c)]["f64_all"] for c in COMBOS}
        assert len(drop) == 1 and min(drop) > 0 and min(drop) % m == 0, (tag, drop)
        print(tag, "FP64 instructions fewer than", tag[1:], min(drop), "=", min(drop) // m, "x", m)
    pol = default_policy()
    for tag in KEPT:
        assert (tag in pol) != (tag[1:] in pol), tag             # one of the two serves the bin
        if tag in pol:
            assert passes[tag], "%s is in the default policy and fails its static gate" % tag
    assert [p for p in pol if p.startswith("k")], "no kept-trial kernel in the default policy"
    for tag in ("kw5", "kw7", "kw9", "kp7", "kp9"):
        assert passes[tag], tag


@pytest.mark.skipif(not os.path.exists(isa_loop_mix.hipcc()), reason="hipcc is not installed: no assembly to count")
def test_kw9_kp9_kp7_against_their_counterparts_in_one_build():
    t = isa_loop_mix.parse_report(TABLE)
    tags = ("w9", "p9", "p7", "kw9", "kp9", "kp7")
    with tempfile.TemporaryDirectory() as d:
        with ThreadPoolExecutor(max_workers=min(len(tags), os.cpu_count() or 4)) as ex:
            rows = dict(zip(tags, ex.map(lambda g: {r["kernel"]: r for r in isa_loop_mix.analyse(isa_loop_mix.build_asm(g, d))}, tags)))
    for tag in tags:                                 # each unit emits its own kernels and no others
        assert set(rows[tag]) == {"%s/%s" % (tag, c) for c in COMBOS}, tag
    for tag in ("kw9", "kp9", "kp7"):
        m = int(tag[2:])
        for c in COMBOS:
            kept, old = rows[tag]["%s/%s" % (tag, c)], rows[tag[1:]]["%s/%s" % (tag[1:], c)]
            print(tag, c, {x: (kept[x], old[x]) for x in ("f64_all", "valu", "copy_lane", "vgpr_spill_count", "scratch_bytes")})
            assert gate(kept, old) == [], (tag, c)
            assert (old["f64_all"] - kept["f64_all"]) % m == 0, (tag, c)
            assert kept["f64_all"] == t["%s/%s" % (tag, c)]["f64_all"], "the table is not this build's"
            assert kept["valu"] < old["valu"]
