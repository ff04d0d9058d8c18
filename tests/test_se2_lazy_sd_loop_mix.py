"""Static gate of the lazy steepest-descent SE(2) kernels (se2_wave_kernel_lz / se2_group_kernel_lz, tags lwM / lpM), from
gfx950 assembly (tools/isa_loop_mix.py) and the committed table profiles/se2_lazy_sd_loop_mix.txt.

A lazy kernel leaves b^T H b, alpha and |h_sd| out of phases B1 / B2 and forms them in one block, sd_terms(), inside the
trial loop, which runs only in the iterations that read them.  The block is delimited in the assembly by two marker
comments (";ipc_sd_terms_begin" / ";ipc_sd_terms_end", each behind a scheduling barrier), so its instructions can be
counted apart.  Against its counterpart -- the kernel the default policy names for that M: kw5 kw7 kw9 w11 w13, kp7 kp9
p11 -- IN THE SAME BUILD, for every NL / staged combination:
    * no scratch;
    * no more spilled vector registers and no more spilled scalar registers than the counterpart;
    * fewer VALU instructions in the dog-leg loop body outside the sd_terms() block.
The static FP64 count of the whole body is no gate: the block moves, it does not vanish.

The engine substitutes a lazy kernel (kLazySdWaveM / kLazySdPairM, cell_plan.hpp) only where the table shows all four of
its combinations through this gate."""
import os
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_loop_mix  # noqa: E402

TABLE = os.path.join(ROOT, "profiles", "se2_lazy_sd_loop_mix.txt")
COMBOS = ("nl1/staged", "nl1/unstaged", "nl2/staged", "nl2/unstaged")
COUNTERPART = {"lw5": "kw5", "lw7": "kw7", "lw9": "kw9", "lw11": "w11", "lw13": "w13",
               "lp7": "kp7", "lp9": "kp9", "lp11": "p11"}


def gate(lazy, old):
    """Why a lazy kernel fails the static gate against its counterpart ([]: it passes)."""
    why = []
    if lazy["scratch_bytes"] != 0:
        why.append("scratch %d B" % lazy["scratch_bytes"])
    if lazy["vgpr_spill_count"] > old["vgpr_spill_count"]:
        why.append("vgpr_spill %d > %d" % (lazy["vgpr_spill_count"], old["vgpr_spill_count"]))
    if lazy["sgpr_spill_count"] > old["sgpr_spill_count"]:
        why.append("sgpr_spill %d > %d" % (lazy["sgpr_spill_count"], old["sgpr_spill_count"]))
    if lazy.get("sd_block_valu") is None:
        why.append("the sd_terms block is not delimited")
    elif not lazy["valu"] - lazy["sd_block_valu"] < old["valu"]:
        why.append("VALU outside sd_terms %d >= %d" % (lazy["valu"] - lazy["sd_block_valu"], old["valu"]))
    return why


def compiled_in():
    """Tags of the kernels the engine substitutes (kLazySdWaveM / kLazySdPairM of cell_plan.hpp)."""
    src = open(os.path.join(ROOT, "ipc_amd", "csrc", "cell_plan.hpp")).read()
    tags = []
    for name, pre in (("kLazySdWaveM", "lw"), ("kLazySdPairM", "lp")):
        m = re.search(r"static const int %s\[\] = \{([^}]*)\}" % name, src)
        assert m, name
        tags += [pre + x.strip() for x in m.group(1).split(",") if x.strip() and int(x) > 0]
    return tags


def test_committed_table_and_compiled_in_list():
    t = isa_loop_mix.parse_report(TABLE)
    assert len(t) == 4 * 2 * len(COUNTERPART)        # every lazy unit and its counterpart, four combinations each
    passes = {}
    for tag, old in COUNTERPART.items():
        why = {c: gate(t["%s/%s" % (tag, c)], t["%s/%s" % (old, c)]) for c in COMBOS}
        passes[tag] = not any(why.values())
        for c in COMBOS:
            a, b = t["%s/%s" % (tag, c)], t["%s/%s" % (old, c)]
            print(tag, c, "VALU", a["valu"], "of which sd_terms", a.get("sd_block_valu"), "counterpart", b["valu"],
                  "spills v/s", (a["vgpr_spill_count"], a["sgpr_spill_count"]), "counterpart",
                  (b["vgpr_spill_count"], b["sgpr_spill_count"]), "scratch", a["scratch_bytes"])
        print(tag, "passes" if passes[tag] else "fails: %s" % {c: w for c, w in why.items() if w})
    for tag in compiled_in():
        assert tag in COUNTERPART, tag
        assert passes[tag], "%s is substituted by the engine and fails its static gate" % tag


def test_the_lazy_getter_is_declared_and_listed():
    """include/ipc_amd_lazy_sd.h declares what ipc_amd.capi lists in SYMBOLS_LAZY_SD, and ipc_amd.h includes it."""
    sys.path.insert(0, ROOT)
    from ipc_amd import capi
    src = open(os.path.join(ROOT, "include", "ipc_amd_lazy_sd.h")).read()
    assert sorted(re.findall(r"^int (ipc_\w+)\(", src, re.M)) == sorted(capi.SYMBOLS_LAZY_SD)
    assert '#include "ipc_amd_lazy_sd.h"' in open(os.path.join(ROOT, "include", "ipc_amd.h")).read()


@pytest.mark.skipif(not os.path.exists(isa_loop_mix.hipcc()), reason="hipcc is not installed: no assembly to count")
def test_substituted_kernels_against_their_counterparts_in_one_build():
    """Every kernel the engine substitutes, and the kernel it serves, compiled here: the committed table is this build's and
    the gate holds on the build, not on the table alone."""
    t = isa_loop_mix.parse_report(TABLE)
    subst = compiled_in()
    assert subst, "the compiled-in list is empty"
    tags = tuple(subst) + tuple(COUNTERPART[g] for g in subst)
    with tempfile.TemporaryDirectory() as d:
        with ThreadPoolExecutor(max_workers=min(len(tags), os.cpu_count() or 4)) as ex:
            rows = dict(zip(tags, ex.map(lambda g: {r["kernel"]: r for r in isa_loop_mix.analyse(isa_loop_mix.build_asm(g, d))}, tags)))
    for tag in tags:                                 # each unit emits its own kernels and no others
        assert set(rows[tag]) == {"%s/%s" % (tag, c) for c in COMBOS}, tag
    for tag in subst:
        for c in COMBOS:
            lazy, old = rows[tag]["%s/%s" % (tag, c)], rows[COUNTERPART[tag]]["%s/%s" % (COUNTERPART[tag], c)]
            print(tag, c, {x: (lazy[x], old[x]) for x in ("valu", "f64_all", "copy_lane", "vgpr_spill_count",
                                                         "sgpr_spill_count", "scratch_bytes")}, "sd_terms", lazy["sd_block_valu"])
            for x in ("valu", "f64_all", "sd_block_valu", "vgpr_spill_count", "sgpr_spill_count", "scratch_bytes"):
                assert lazy[x] == t["%s/%s" % (tag, c)][x], "the table is not this build's (%s %s %s)" % (tag, c, x)
            for x in ("valu", "vgpr_spill_count", "sgpr_spill_count", "scratch_bytes"):
                assert old[x] == t["%s/%s" % (COUNTERPART[tag], c)][x], "the table is not this build's (%s %s %s)" % (COUNTERPART[tag], c, x)
            assert lazy["sd_block_valu"] is not None and lazy["sd_block_valu"] > 0      # the block is there, and delimited
            assert old["sd_block_valu"] is None                                       # ... and in no other kernel
            assert gate(lazy, old) == [], (tag, c)
