#!/usr/bin/env python
"""Instruction mix of the dog-leg loop body of the SE(2) wave / pair kernels, from gfx950 assembly (static: one pass
through the loop body, every unrolled slot counted once; a once-per-iteration block weighs like a per-slot one).

  python tools/isa_loop_mix.py FILE.s [FILE.s ...] [--match REGEX] [--json]
  python tools/isa_loop_mix.py --build [--only p7,p9,...] [--match nl2/staged] [--out FILE]    # the recipe, see hot_units()

A kernel is the text between its global label and its .Lfunc_end.  Loops are the backward branches to a .LBB label
of the kernel; the widest one is taken as the dog-leg loop (`for (int it ...)` of se2_wave_solve), which is > 90 % of
the kernel's text.  Registers, spill counts and scratch come from the kernel's metadata note in the same file.

The classes are those of tools/isa_mix.py, with the memory classes split (scratch traffic inside the loop is what a
VGPR spill costs) and FP64 compares / conversions kept apart from FP64 arithmetic:
  f64       v_*_f64 arithmetic (add, mul, fma, rcp, rsq, sqrt, min, max, ldexp, frexp, trig_preop, div_*), DPP forms too
  f64_cmp   v_cmp*_f64, v_cmp_class_f64          f64_cvt   conversions from / to f64, v_rndne / floor / fract ...
  accvgpr   v_accvgpr_read / write (AGPR <-> VGPR copies)
  lane      v_readlane / v_writelane / v_readfirstlane (SGPR spill traffic, wave-uniform broadcasts)
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VALU_CLASSES = ("f64", "f64_cmp", "f64_cvt", "accvgpr", "v_mov", "v_int", "cndmask", "lane", "dpp_mov", "v_other")
ALL_CLASSES = VALU_CLASSES + ("salu", "s_nop", "s_waitcnt", "lds", "scratch", "vmem", "smem")
_F64_ROUND = ("v_rndne_f64", "v_floor_f64", "v_ceil_f64", "v_trunc_f64", "v_fract_f64")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)(?:\s|$)")
SD_BEGIN, SD_END = ";ipc_sd_terms_begin", ";ipc_sd_terms_end"     # marker comments of se2_wave_solve's sd_terms()


def classify(line):
    """Class of one assembly line, or None if it is not an instruction."""
    m = _INSN.match(line)
    if not m:
        return None
    op = m.group(1)
    if op.startswith("v_"):
        if op.startswith("v_accvgpr"):
            return "accvgpr"
        if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            return "lane"
        if "_f64" in op:
            if op.startswith("v_cmp"):
                return "f64_cmp"
            if op.startswith("v_cvt") or op.startswith(_F64_ROUND):
                return "f64_cvt"
            return "f64"
        if op.startswith("v_mov"):
            return "dpp_mov" if ("dpp" in line or "row_" in line or "quad_perm" in line) else "v_mov"
        if op.startswith("v_cndmask"):
            return "cndmask"
        if re.search(r"_(u|i|b)(16|32|64)(_|$)", op) or op.startswith(("v_and", "v_or", "v_xor", "v_not", "v_bfe",
                                                                      "v_lshl", "v_lshr", "v_ashr", "v_mbcnt")):
            return "v_int"
        return "v_other"
    if op.startswith("s_"):
        if op.startswith("s_nop"):
            return "s_nop"
        if op.startswith("s_waitcnt"):
            return "s_waitcnt"
        if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
            return "smem"
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    return None


def _demangle(names):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def short_name(demangled):
    """se2_wave_kernel<9, 2, true> -> w9/nl2/staged; se2_group_kernel<2, 9, 2, true> -> p9/nl2/staged (W = 4: q);
    the kept-trial kernels se2_wave_kernel_kt / se2_group_kernel_kt -> kw9/..., kp9/...; the lazy steepest-descent
    kernels se2_wave_kernel_lz / se2_group_kernel_lz -> lw9/..., lp9/..."""
    m = re.search(r"se2_wave_kernel_lz<(\d+), (\d+), (true|false)>", demangled)
    if m:
        return "lw%s/nl%s/%s" % (m.group(1), m.group(2), "staged" if m.group(3) == "true" else "unstaged")
    m = re.search(r"se2_group_kernel_lz<(\d+), (\d+), (\d+), (true|false)>", demangled)
    if m:
        return "l%s%s/nl%s/%s" % ({"2": "p", "4": "q"}.get(m.group(1), "g" + m.group(1)), m.group(2), m.group(3),
                                  "staged" if m.group(4) == "true" else "unstaged")
    m = re.search(r"se2_wave_kernel_kt<(\d+), (\d+), (true|false)>", demangled)
    if m:
        return "kw%s/nl%s/%s" % (m.group(1), m.group(2), "staged" if m.group(3) == "true" else "unstaged")
    m = re.search(r"se2_group_kernel_kt<(\d+), (\d+), (\d+), (true|false)>", demangled)
    if m:
        return "k%s%s/nl%s/%s" % ({"2": "p", "4": "q"}.get(m.group(1), "g" + m.group(1)), m.group(2), m.group(3),
                                  "staged" if m.group(4) == "true" else "unstaged")
    m = re.search(r"se2_wave_kernel<(\d+), (\d+), (true|false)>", demangled)
    if m:
        return "w%s/nl%s/%s" % (m.group(1), m.group(2), "staged" if m.group(3) == "true" else "unstaged")
    m = re.search(r"se2_group_kernel<(\d+), (\d+), (\d+), (true|false)>", demangled)
    if m:
        return "%s%s/nl%s/%s" % ({"2": "p", "4": "q"}.get(m.group(1), "g" + m.group(1)), m.group(2), m.group(3),
                                 "staged" if m.group(4) == "true" else "unstaged")
    return re.sub(r"\(.*", "", demangled).replace("void ", "")


def _metadata(lines):
    """{mangled kernel name: {key: value}} from the amdhsa.kernels note of the file."""
    meta, cur = {}, None
    keys = ("name", "vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
            "private_segment_fixed_size", "group_segment_fixed_size")
    in_kernels = False
    for l in lines:
        if l.startswith("amdhsa.kernels:"):
            in_kernels = True
            continue
        if not in_kernels:
            continue
        if l.startswith("amdhsa.") or l.startswith("..."):
            in_kernels = False
            continue
        m = re.match(r"^  (-| ) \.(\w+):\s*(.*)$", l)
        if not m:
            continue
        if m.group(1) == "-":
            cur = {}
        k, v = m.group(2), m.group(3).strip().strip("'\"")
        if cur is not None and k in keys:
            cur[k] = v if k == "name" else int(v)
            if k == "name":
                meta[v] = cur
    return meta


def kernels_of(path):
    """[(mangled name, body lines)] of every kernel (function with a .Lfunc_end) in an assembly file, + metadata."""
    lines = open(path).read().split("\n")
    meta = _metadata(lines)
    out, name, start = [], None, 0
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            name, start = m.group(1), i
        elif name and l.startswith(".Lfunc_end"):
            if name in meta:
                out.append((name, lines[start:i]))
            name = None
    return out, meta


def loops_of(body):
    """Backward branches of a kernel body as (first line, branch line), widest first."""
    lab = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            lab[m.group(1)] = i
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in lab and lab[m.group(1)] < i:
            loops.append((lab[m.group(1)], i))
    loops.sort(key=lambda t: (t[0] - t[1], t[0]))
    return loops


def dogleg_loop(body):
    """The widest backward branch of the kernel.  (The block layout is not nested: the persistent cell loop's own back
    edges start further down -- behind the loop-constant set-up that is laid out after the dog-leg header -- and are
    narrower; the dog-leg loop is > 90 % of the kernel's text, so the widest span is it.)"""
    loops = loops_of(body)
    return loops[0] if loops else None


def count(seg):
    c, ops = collections.Counter(), collections.Counter()
    for l in seg:
        k = classify(l)
        if k:
            c[k] += 1
            ops[_INSN.match(l).group(1)] += 1
    return c, ops


def analyse(path, match=None):
    rows = []
    kernels, meta = kernels_of(path)
    dem = _demangle([n for n, _ in kernels])
    for name, body in kernels:
        d = dem.get(name, name)
        if match and not re.search(match, d) and not re.search(match, short_name(d)):
            continue
        loop = dogleg_loop(body)
        if loop is None:
            continue
        c, ops = count(body[loop[0]:loop[1] + 1])
        valu = sum(c[k] for k in VALU_CLASSES)
        md = meta[name]
        # the sd_terms() block of a lazy steepest-descent kernel, between its two marker comments (once each, in order,
        # inside the loop: else the block counts as not delimited)
        seg = body[loop[0]:loop[1] + 1]
        mb = [i for i, l in enumerate(seg) if SD_BEGIN in l]
        me = [i for i, l in enumerate(seg) if SD_END in l]
        sd_valu = None
        if len(mb) == 1 and len(me) == 1 and mb[0] < me[0]:
            sc, _ = count(seg[mb[0]:me[0]])
            sd_valu = sum(sc[k] for k in VALU_CLASSES)
        rows.append({
            "kernel": short_name(d), "loop_lines": loop[1] - loop[0] + 1,
            "counts": {k: c[k] for k in ALL_CLASSES}, "valu": valu,
            "f64_all": c["f64"] + c["f64_cmp"] + c["f64_cvt"],
            "f64_share": (c["f64"] + c["f64_cmp"] + c["f64_cvt"]) / valu if valu else 0.0,
            "sd_block_valu": sd_valu,
            "copy_lane": c["accvgpr"] + c["lane"],
            "execz": ops["s_cbranch_execz"] + ops["s_cbranch_execnz"],
            "saveexec": sum(v for k, v in ops.items() if "saveexec" in k),
            "v_add_u32": ops["v_add_u32_e32"] + ops["v_add_u32_e64"],
            "vgpr_count": md.get("vgpr_count"), "agpr_count": md.get("agpr_count"), "sgpr_count": md.get("sgpr_count"),
            "sgpr_spill_count": md.get("sgpr_spill_count"), "vgpr_spill_count": md.get("vgpr_spill_count"),
            "scratch_bytes": md.get("private_segment_fixed_size"),
            "top_int_salu": [[k, v] for k, v in ops.most_common() if classify("\t" + k + " ") in ("v_int", "v_other", "salu")][:12],
        })
    rows.sort(key=lambda r: r["kernel"])
    return rows


def render(rows, out=sys.stdout):
    for r in rows:
        c = r["counts"]
        out.write("%s   loop body %d lines; registers %s (agpr %s), sgpr %s, sgpr_spill %s, vgpr_spill %s, scratch %s B\n" % (
            r["kernel"], r["loop_lines"], r["vgpr_count"], r["agpr_count"], r["sgpr_count"], r["sgpr_spill_count"],
            r["vgpr_spill_count"], r["scratch_bytes"]))
        for k in VALU_CLASSES:
            if c[k]:
                out.write("    %-10s %6d  %.3f of VALU\n" % (k, c[k], c[k] / r["valu"]))
        out.write("    %-10s %6d  %.3f of VALU   (f64 + f64_cmp + f64_cvt: every v_*_f64)\n" % ("FP64 all", r["f64_all"], r["f64_share"]))
        out.write("    %-10s %6d\n" % ("all VALU", r["valu"]))
        if r.get("sd_block_valu") is not None:
            out.write("    %-10s %6d   (VALU of the sd_terms block, between its markers)\n" % ("sd_terms", r["sd_block_valu"]))
        for k in ALL_CLASSES[len(VALU_CLASSES):]:
            if c[k]:
                out.write("    %-10s %6d\n" % (k, c[k]))
        out.write("    accvgpr+lane %d, execz branches %d, saveexec %d, v_add_u32 %d\n" % (
            r["copy_lane"], r["execz"], r["saveexec"], r["v_add_u32"]))
        out.write("    most frequent integer / other VALU and SALU: %s\n\n" % ", ".join("%s %d" % (k, v) for k, v in r["top_int_salu"]))


def parse_report(path):
    """{kernel: {f64_all, valu, copy_lane, sgpr_spill_count, vgpr_spill_count, scratch_bytes}} of a text report written
    by render() (the committed profiles/r7_se2_loop_mix_*.txt)."""
    out = {}
    for blk in open(path).read().split("\n\n"):
        m = re.match(r"^(\S+)   loop body", blk.strip())
        if not m:
            continue
        g = lambda pat: int(re.search(pat, blk).group(1))
        sd = re.search(r"^    sd_terms\s+(\d+)", blk, re.M)
        out[m.group(1)] = {"sd_block_valu": int(sd.group(1)) if sd else None, "f64_all": g(r"FP64 all\s+(\d+)"), "valu": g(r"all VALU\s+(\d+)"),
                           "copy_lane": g(r"accvgpr\+lane (\d+)"), "sgpr_spill_count": g(r"sgpr_spill (\d+)"),
                           "vgpr_spill_count": g(r"vgpr_spill (\d+)"), "scratch_bytes": g(r"scratch (\d+) B")}
    return out


# ---- the recipe: assembly of the hot instantiations, one per compile (shipped flags, device side only) ----
def hot_units():
    """{tag: (translation unit, [-D...])}: w9 w11 w13 of se2_wave.hip, p7 p9 p11 of se2_pair.hip, and the kept-trial
    kernels kw5 .. kw11 of se2_wave_kt.hip and kp7 kp9 kp11 of se2_pair_kt.hip (with w5 and w7, their counterparts); the
    lazy steepest-descent kernels lw5 .. lw13 of se2_wave_lz.hip and lp7 lp9 lp11 of se2_pair_lz.hip (counterparts: what the
    default policy names for that M, kw5 kw7 kw9 w11 w13 and kp7 kp9 p11)."""
    u = {}
    for m in (9, 11, 13):
        u["w%d" % m] = ("se2_wave.hip", ["-DIPC_WAVE_ONLY_M=%d" % m])
    for m in (7, 9, 11):
        u["p%d" % m] = ("se2_pair.hip", ["-DIPC_PAIR_ONLY_M=%d" % m])
    for m in (5, 7):
        u["w%d" % m] = ("se2_wave.hip", ["-DIPC_WAVE_ONLY_M=%d" % m])
    for m in (5, 7, 9, 11):
        u["kw%d" % m] = ("se2_wave_kt.hip", ["-DIPC_WAVE_KT_ONLY_M=%d" % m])
    for m in (7, 9, 11):
        u["kp%d" % m] = ("se2_pair_kt.hip", ["-DIPC_PAIR_KT_ONLY_M=%d" % m])
    for m in (5, 7, 9, 11, 13):
        u["lw%d" % m] = ("se2_wave_lz.hip", ["-DIPC_WAVE_LZ_ONLY_M=%d" % m])
    for m in (7, 9, 11):
        u["lp%d" % m] = ("se2_pair_lz.hip", ["-DIPC_PAIR_LZ_ONLY_M=%d" % m])
    return u


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_asm(tag, outdir, extra=()):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    unit, defs = hot_units()[tag]
    dst = os.path.join(outdir, tag + ".s")
    subprocess.check_call([hipcc()] + list(ge.HIP_FLAGS) + defs + list(extra) +
                          ["-S", "--cuda-device-only", os.path.join(ge.CSRC, unit), "-o", dst])
    return dst


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*")
    ap.add_argument("--match", default=None, help="regex on the demangled or short kernel name (e.g. 'nl2/staged')")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--build", action="store_true", help="compile the hot instantiations to assembly first")
    ap.add_argument("--only", default=None, help="with --build: comma-separated tags out of " + ",".join(hot_units()))
    ap.add_argument("--asm-dir", default=None, help="with --build: where the .s files go (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    files = list(a.files)
    tmp = None
    if a.build:
        from concurrent.futures import ThreadPoolExecutor
        tags = a.only.split(",") if a.only else list(hot_units())
        outdir = a.asm_dir
        if outdir is None:
            tmp = tempfile.TemporaryDirectory()
            outdir = tmp.name
        os.makedirs(outdir, exist_ok=True)
        with ThreadPoolExecutor(max_workers=min(len(tags), 8, os.cpu_count() or 4)) as ex:
            files += list(ex.map(lambda t: build_asm(t, outdir), tags))
    rows = []
    for f in files:
        rows += analyse(f, a.match)
    out = open(a.out, "w") if a.out else sys.stdout
    if a.json:
        json.dump(rows, out, indent=1)
        out.write("\n")
    else:
        render(rows, out)
    if a.out:
        out.close()
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
