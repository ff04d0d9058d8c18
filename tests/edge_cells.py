"""Aimed inputs for the cell kernels: small pose graphs whose candidates sit on the layout edges of one kernel variant.

Plain module (no GPU use, no fixtures): tests/test_edge_cells_cpu.py checks that the positions land where their tags
say and that the oracle alone is well conditioned on these inputs; tests/test_gpu_variant_edges.py runs every variant
of the default policies on them and holds every solved cell against the oracle.

A cell of L poses is laid over a variant of W waves x 64 lanes x M slots (capacity cap = 64 W M); pose j = 1 .. L is
counted from the gauge (pose 0, the first vertex of the cell).  Two layouts exist (restated in owner() / pose_at()):

  "lane"  SE2 wave / pair / quad kernels (se2_wave_cell.hpp): consecutive poses in one lane,
          cell-lane gl = (j-1) / M, slot (j-1) % M, wave gl / 64 = (j-1) / (64 M), lane gl % 64
  "slot"  SE2 block (se2_cell.hpp), SE3 block (se3_cell.hpp) and SE3 LDS kernels (se3_lds_cell.hpp): consecutive poses
          in consecutive lanes, j = wave 64 M + slot 64 + lane + 1,
          wave (j-1) / (64 M), slot ((j-1) % (64 M)) / 64, lane (j-1) % 64
"""
import functools
import math
from collections import namedtuple

import numpy as np

from ipc_amd import synth
from ipc_amd.graphio import PoseGraph

Cand = namedtuple("Cand", "tag f t claims dup_of")     # f, t relative to the offset; claims: checked by tests/test_edge_cells_cpu.py

SE2_SHIFT, SE3_SHIFT = 4.0, 3.0                       # outliers: metres added to the measured translation


def owner(family, W, M, j):
    """(wave, lane, slot) of pose j >= 1."""
    if family == "lane":
        gl = (j - 1) // M
        return gl // 64, gl % 64, (j - 1) % M
    r = (j - 1) % (64 * M)
    return (j - 1) // (64 * M), r % 64, r // 64


def pose_at(family, W, M, wave, lane, slot):
    if family == "lane":
        return (wave * 64 + lane) * M + slot + 1
    return wave * 64 * M + slot * 64 + lane + 1


def last_fill(family, M, L):
    """Poses in the last occupied lane (lane layout) / in the last occupied 64-pose block (slot layout)."""
    return (L - 1) % (M if family == "lane" else 64) + 1


def _lane_list(W, M):
    C = 64 * W * M
    P = functools.partial(pose_at, "lane", W, M)
    s1, s2 = min(1, M - 1), min(2, M - 1)
    out = [
        # whole capacity: from at the gauge (lf == 0 path), to in the last slot of the last lane of the last wave
        Cand("whole", 0, C, [("f", "gauge"), ("t", "owner", (W - 1, 63, M - 1)), ("L", C)], None),
        Cand("whole-reversed", C, 0, [("t", "gauge"), ("f", "owner", (W - 1, 63, M - 1))], None),
        # (1, cap) + (0, cap-1): a two-loop cell of exactly cap poses that neither loop spans
        Cand("cap-pair-a", 1, C, [("f", "owner", (0, 0, 0))], None),
        Cand("cap-pair-b", 0, C - 1, [("fill", (M - 1) or 1)], None),          # last lane holds M-1 poses
        Cand("fill-1", C - M + 1, 0, [("fill", 1)], None),                     # last lane holds one pose
        Cand("short-2", 0, 2, [("L", 2)], None),                               # all but one or two lanes idle
        Cand("short-M+1", M + 1, 0, [("L", M + 1), ("f", "owner", (0, 1, 0))], None),
        # slot 0 and slot M-1 of a lane; starts where short-M+1 ends (touching: a free cell)
        Cand("slot0-slotM-1", P(0, 1, 0), P(0, 20, M - 1), [("f", "slot", 0), ("t", "slot", M - 1)], None),
        Cand("duplicate", P(0, 1, 0), P(0, 20, M - 1), [], 7),
        # two loops with end points in the same slot index of different lanes (one ownSlots bit), staggered, one reversed
        Cand("share-slot-a", P(0, 3, s1), P(0, 29, M - 1), [("f", "owner", (0, 3, s1))], None),
        Cand("share-slot-b", P(0, 49, M - 1), P(0, 9, s1), [("t", "owner", (0, 9, s1))], None),
        # two loops that start at one interior pose
        Cand("share-start", P(0, 3, s1), P(0, 45, s2), [("f", "owner", (0, 3, s1))], None),
    ]
    if W <= 2:                                            # ... and two that end at one interior pose
        out.append(Cand("share-end", 5, P(0, 29, M - 1), [("t", "owner", (0, 29, M - 1))], None))
    if M >= 3:                                            # ends on the last vertex (tail = 0), last lane holds one pose:
        out.append(Cand("pad-read", M - 1, C, [("fill", 1), ("t", "last")], None))   # M-1 records read past the chain
    if W == 2:                                            # both sides of the wave boundary 64 M | 64 M + 1
        out.append(Cand("wave0-last", 7, 64 * M, [("t", "owner", (0, 63, M - 1))], None))
        out.append(Cand("wave1-first", C - 5, 64 * M + 1, [("t", "owner", (1, 0, 0))], None))
    if W == 4:                                            # both sides of 64 M k | 64 M k + 1, k = 1, 2, 3
        out.append(Cand("wave0-last/wave2-first", 64 * M, 128 * M + 1,
                        [("f", "owner", (0, 63, M - 1)), ("t", "owner", (2, 0, 0))], None))
        out.append(Cand("wave2-last/wave1-first", 192 * M, 64 * M + 1,
                        [("f", "owner", (2, 63, M - 1)), ("t", "owner", (1, 0, 0))], None))
        out.append(Cand("wave1-last/wave3-first", 128 * M, 192 * M + 1,
                        [("f", "owner", (1, 63, M - 1)), ("t", "owner", (3, 0, 0))], None))
    return out


def _slot_list(W, M, small):
    C = 64 * W * M
    P = functools.partial(pose_at, "slot", W, M)
    x_in, y_in = P(0, 19, 0), C - 7                       # inside a 64-pose block
    x_blk, y_blk = 64, C - 64                             # M >= 2: last pose of a block that does not end a wave
    x_wav, y_wav = 64 * M, C - 64 * M                     # W >= 2: last pose of a wave
    whole = [
        Cand("whole", 0, C, [("f", "gauge"), ("t", "owner", (W - 1, 63, M - 1)), ("L", C)], None),
        Cand("whole-reversed", C, 0, [("t", "gauge"), ("f", "owner", (W - 1, 63, M - 1))], None),
        Cand("cap-pair-a", 1, C, [("f", "owner", (0, 0, 0))], None),
        Cand("cap-pair-b", 0, C - 1, [("fill", 63)], None),
        Cand("short-2", 2, 0, [("L", 2)], None),
        # in-block class changes, nested in the whole-capacity loops; starts where short-2 ends (touching: a free cell)
        Cand("inner-in", 2, C - 9, [("f", "place", "in"), ("t", "place", "in")], None),
    ]
    tail_wav = Cand("tail-wave", C, x_wav, [("t", "owner", (0, 63, M - 1)), ("t", "place", "wave")], None)
    inner_blk = Cand("inner-block", 65, y_blk, [("f", "owner", (0, 0, 1)), ("t", "place", "block")], None)
    if small:                                             # the 16x8 / 16x16 cases: eight candidates, both sides of 64 | 65 and
        return whole[:5] + [                              # of 64 M | 64 M + 1; the second touches tail-wave (a free cell)
            tail_wav,
            Cand("block0-last/wave0-last", 64, x_wav, [("f", "owner", (0, 63, 0)), ("t", "owner", (0, 63, M - 1))], None),
            Cand("block1-first/wave1-first", 65, x_wav + 1, [("f", "owner", (0, 0, 1)), ("t", "owner", (1, 0, 0))], None)]
    out = whole
    if W >= 2:                                            # the last wave of the team holds a single pose
        out.append(Cand("last-wave-1", C - 64 * M + 1, 0, [("f", "owner", (W - 1, 0, 0)), ("fill", 1)], None))
    elif M >= 2:
        out.append(Cand("last-block-1", C - 63, 0, [("f", "owner", (0, 0, M - 1)), ("fill", 1)], None))
    # heads (0, p) and tails (q, cap): with the whole-capacity loops they are the same-start (AB|A) and same-end (A|AB)
    # cells, with each other the staggered ones (A|AB|B); the class changes at p and q fall inside a block, on a block
    # boundary and on a wave boundary
    out.append(Cand("head-in", y_in, 0, [("f", "place", "in")], None))
    out.append(Cand("tail-in", x_in, C, [("f", "place", "in")], None))
    if M >= 2:
        out.append(Cand("head-block", 0, y_blk, [("t", "place", "block")], None))
        out.append(Cand("tail-block", C, x_blk, [("t", "place", "block"), ("t", "owner", (0, 63, 0))], None))
        if y_blk - 65 >= 2:
            out.append(inner_blk)                         # other side of the slot boundary 64 | 65
    if W >= 2:
        out.append(Cand("head-wave", 0, y_wav, [("t", "place", "wave"), ("t", "owner", (W - 2, 63, M - 1))], None))
        out.append(tail_wav)
        # other side of the wave boundary 64 M | 64 M + 1; W >= 4: nested class changes on wave boundaries
        out.append(Cand("inner-wave", y_wav if W >= 4 else C - 3, 64 * M + 1, [("t", "owner", (1, 0, 0))], None))
    out.append(Cand("duplicate", 2, C - 9, [], 5))
    fillers = [Cand("filler-a", C // 6, C // 2, [], None), Cand("filler-b", C // 2, 5 * C // 6, [], None),
               Cand("filler-c", 2 * C // 3 + 1, C // 4, [], None)]
    for f in fillers:
        if len(out) < 12:
            out.append(f)
    return out


def edge_candidates(family, W, M, small=False):
    cands = _lane_list(W, M) if family == "lane" else _slot_list(W, M, small)
    C = 64 * W * M
    for c in cands:
        assert 0 <= c.f <= C and 0 <= c.t <= C and abs(c.f - c.t) >= 2, c
    assert len(cands) <= 16
    return cands


def is_outlier(k, tag):
    """About one candidate in four; the four whole-capacity loops at the head of the lists stay inliers."""
    return tag == "short-2" or (k >= 5 and k % 4 == 1)


def outlier_shift(dim, L):
    """Metres added to the measured translation of an outlier.  A long chain absorbs such a shift in its accumulated
    odometry uncertainty (its cells are accepted all the same; a shift that grows with L runs the dog-leg into its
    iteration cap): the rejected cells of a case are those of its short and medium loops."""
    return SE2_SHIFT if dim == 2 else SE3_SHIFT


def place_of(W, M, p):
    """Where a class change behind pose p falls in the slot layout (poses <= p keep their class)."""
    if p % (64 * M) == 0:
        return "wave"
    return "block" if p % 64 == 0 else "in"


def pair_shape(a, b):
    """Shape of the two ranges a = (lo, hi), b = (lo, hi) of a two-loop cell; None when they do not overlap."""
    (la, ha), (lb, hb) = a, b
    if min(ha, hb) - max(la, lb) <= 0:
        return "touching" if min(ha, hb) == max(la, lb) else None
    if (la, ha) == (lb, hb):
        return "identical"
    if la == lb:
        return "same-start"
    if ha == hb:
        return "same-end"
    if (la < lb and hb < ha) or (lb < la and ha < hb):
        return "nested"
    return "staggered"


def expected_cells(loop_ids):
    """The cells the engine solves: every diagonal cell, and a pair cell where the two ranges overlap with positive
    length (reference src/consensus.cpp:157-159).  Sorted list of (i, j), i <= j."""
    lo, hi = loop_ids.min(1), loop_ids.max(1)
    N = len(lo)
    return [(i, j) for i in range(N) for j in range(i, N)
            if i == j or min(hi[i], hi[j]) - max(lo[i], lo[j]) > 0]


# ---- trajectories and measurements, drawn the way ipc_amd.synth draws them ---------------------------------------------
def _se2_chain(V, rng, sig_o=(0.03, 0.012), odom_trust=10.0):
    """Ground truth, odometry and open-loop vertices of synth._se2_graph (same tour, same noise model) without its
    all-pairs distance table, which is quadratic in V."""
    laps = max(2.5, V / 200.0)
    t = np.linspace(0.0, 2 * np.pi * laps, V)
    gx = 12.0 * np.sin(t * 1.0 + 0.3) + 3.0 * np.sin(t * 0.11) + np.cumsum(rng.normal(0, 0.01, V))
    gy = 8.0 * np.sin(t * 2.0) + 2.0 * np.cos(t * 0.07) + np.cumsum(rng.normal(0, 0.01, V))
    gth = np.arctan2(np.gradient(gy), np.gradient(gx))
    gt = np.stack([gx, gy, gth], axis=1)
    odom_meas = np.zeros((V - 1, 3))
    odom_info = np.zeros((V - 1, 6))
    for j in range(V - 1):
        cov, inf = synth._se2_info(rng, sig_o[0], sig_o[1])
        z = synth._se2_between(gt[j], gt[j + 1]) + rng.multivariate_normal(np.zeros(3), cov / odom_trust)
        z[2] = synth._wrap(z[2])
        odom_meas[j] = z
        odom_info[j] = synth._upper(inf)
    verts = np.zeros((V, 3))
    for j in range(V - 1):
        a, z = verts[j], odom_meas[j]
        c, s = math.cos(a[2]), math.sin(a[2])
        verts[j + 1] = [a[0] + c * z[0] - s * z[1], a[1] + s * z[0] + c * z[1], synth._wrap(a[2] + z[2])]
    return gt, odom_meas, odom_info, verts


@functools.lru_cache(maxsize=8)
def edge_graph(dim, W, M, family, offset=0, tail=3, seed=None, small=False):
    """PoseGraph of offset + 64 W M + 1 + tail vertices with the aimed candidates of (family, W, M) shifted by `offset`;
    meta["tags"] names the edge each candidate aims at.  Cached: callers must not modify it."""
    C = 64 * W * M
    V = offset + C + 1 + tail
    cands = edge_candidates(family, W, M, small)
    if seed is None:
        seed = default_seed(dim, W, M, family, offset)
    pairs = [(offset + c.f, offset + c.t) for c in cands]
    if dim == 2:
        rng = np.random.default_rng(seed)
        gt, odom_meas, odom_info, verts = _se2_chain(V, rng)
        loop_meas = np.zeros((len(pairs), 3))
        loop_info = np.zeros((len(pairs), 6))
        for k, (a, b) in enumerate(pairs):
            cov, inf = synth._se2_info(rng, 0.05, 0.02)
            z = synth._se2_between(gt[a], gt[b]) + rng.multivariate_normal(np.zeros(3), cov)
            z[2] = synth._wrap(z[2])
            loop_meas[k] = z
            loop_info[k] = synth._upper(inf)
        g = PoseGraph(2, verts, odom_meas, odom_info, np.array(pairs, dtype=np.int32), loop_meas, loop_info, {})
    else:
        rng = np.random.default_rng(seed)
        s = np.arange(V) * 0.05
        pos = np.stack([20 * np.cos(s) + 0.002 * np.arange(V), 20 * np.sin(s),
                        0.01 * np.arange(V) % 7.0 + np.cumsum(rng.normal(0, 0.01, V))], axis=1)
        Rs = synth._look_frames(pos + np.array([0, 0, 100.0]))
        g = synth._se3_graph(Rs, pos, pairs, seed, name="edge-se3")
    for k, c in enumerate(cands):
        if c.dup_of is not None:
            g.loop_meas[k] = g.loop_meas[c.dup_of]
            g.loop_info[k] = g.loop_info[c.dup_of]
        elif is_outlier(k, c.tag):
            g.loop_meas[k, 0] += outlier_shift(dim, abs(c.f - c.t))
    g.meta = dict(name="edge-%s-%dx%d" % (family, W, M), seed=seed, tags=[c.tag for c in cands], offset=offset,
                  cands=cands, family=family, W=W, M=M)
    for a in (g.vertices, g.odom_meas, g.odom_info, g.loop_ids, g.loop_meas, g.loop_info):
        a.setflags(write=False)
    return g


# Seeds are part of the inputs: tests/test_edge_cells_cpu.py holds the oracle's margins on them.  A case whose default
# seed leaves a cell of the oracle within 1 % of its threshold gets another one here.
SEED_OVERRIDES = {                                       # key: (dim, family, W, M, offset)
    (2, 'lane', 4, 13, 37): 113372,
    (3, 'slot', 1, 3, 37): 115229,
    (3, 'slot', 4, 3, 37): 115805,
    (3, 'slot', 4, 10, 37): 117597,
}


def default_seed(dim, W, M, family, offset):
    key = (dim, family, W, M, offset)
    return SEED_OVERRIDES.get(key, 5000 * dim + 64 * W * M + (7 if family == "lane" else 0) + offset)


# ---- the cases of tests/test_gpu_variant_edges.py ------------------------------------------------------------------------
Case = namedtuple("Case", "id dim token family W M offset tail small env")
UNSTAGED_OFFSET = 1100 + 37
UNSTAGED_MIN_V = 2100       # 88 bytes x (V - 1 + 32) records alone exceed the 160 KB of LDS from V = 1831 on


def _tok(dim, tok):
    """(family, W, M) of a policy token."""
    if "x" in tok:
        w, m = tok.split("x")
        return "slot", int(w), int(m)
    m = int(tok[1:])
    if dim == 2:
        return "lane", {"w": 1, "p": 2, "q": 4}[tok[0]], m
    return "slot", {"w": 1, "g": 4}[tok[0]], m


SE2_TOKENS = "w1 w3 w5 w7 w9 w11 w13 p5 p7 p9 p11 q7 q9 q11 q13 16x4 16x8 16x16".split()
SE3_TOKENS = "w1 w2 w3 w4 w6 w8 g3 g4 g5 g6 g7 g8 g9 g10 16x4".split()
SE3_BLOCK_TOKENS = "1x1 1x2 1x3 2x2 2x3 4x2 4x4 8x4 8x5".split()


def _cases():
    out = []
    for tok in SE2_TOKENS:
        fam, W, M = _tok(2, tok)
        out.append(Case("se2-" + tok, 2, tok, fam, W, M, 37, 0, tok in ("16x8", "16x16"), {"IPC_SE2_POLICY": tok}))
    for tok in SE2_TOKENS:
        fam, W, M = _tok(2, tok)
        if tok[0] in "wp":                                # the wave and pair variants once more, constants from L2
            tail = max(0, UNSTAGED_MIN_V - (UNSTAGED_OFFSET + 64 * W * M + 1))
            out.append(Case("se2-" + tok + "-unstaged", 2, tok, fam, W, M, UNSTAGED_OFFSET, tail, False,
                            {"IPC_SE2_POLICY": tok}))
    for tok in SE3_TOKENS + SE3_BLOCK_TOKENS:
        fam, W, M = _tok(3, tok)
        out.append(Case("se3-" + tok, 3, tok, fam, W, M, 37, 0, False,
                        {"IPC_SE3_POLICY": tok, "IPC_SE3_LATENCY_POLICY": "none"}))
    # each family's graph once under the default policy (offset 0: lo_abs == 0 on the cells that start at the gauge)
    out.append(Case("se2-default-lane", 2, None, "lane", 4, 13, 0, 3, False, {}))
    out.append(Case("se2-default-slot", 2, None, "slot", 16, 4, 0, 3, False, {}))
    out.append(Case("se3-default-lds", 3, None, "slot", 4, 10, 0, 3, False, {}))
    out.append(Case("se3-default-block", 3, None, "slot", 8, 5, 0, 3, False, {}))
    return out


CASES = _cases()


def case_graph(case):
    return edge_graph(case.dim, case.W, case.M, case.family, case.offset, case.tail, None, case.small)


def case_config(case):
    from ipc_amd.consensus import Config
    return Config() if case.dim == 2 else Config(s_factor=50.0, slow_reject_th=6.251)


@functools.lru_cache(maxsize=4)
def _oracle_cells_cached(dim, W, M, family, offset, tail, small, nthreads):
    from oracle import oracle as O
    from ipc_amd.consensus import Config
    g = edge_graph(dim, W, M, family, offset, tail, None, small)
    cfg = Config() if dim == 2 else Config(s_factor=50.0, slow_reject_th=6.251)
    cells = expected_cells(g.loop_ids)
    ci = np.array([c[0] for c in cells], dtype=np.int32)
    cj = np.array([c[1] for c in cells], dtype=np.int32)
    poses = O.propagate(dim, g.odom_meas)
    mx, its, _ = O.pair_cells_mt(dim, g.odom_meas, g.odom_info, cfg.s_factor, poses, g.loop_ids, g.loop_meas, g.loop_info,
                                 ci, cj, cfg.fast_reject_iter_base, cfg.slow_reject_iter_base, nthreads)
    for a in (ci, cj, mx, its):
        a.setflags(write=False)
    return ci, cj, mx, its


def oracle_cells(case, nthreads):
    """(i, j, max chi2, iterations) of the oracle on every expected cell of the case; computed once per graph."""
    return _oracle_cells_cached(case.dim, case.W, case.M, case.family, case.offset, case.tail, case.small, nthreads)


def iteration_cap(cfg, L, nl):
    base = cfg.fast_reject_iter_base if nl == 1 else cfg.slow_reject_iter_base
    return base * 5 if L + nl > 100 else base              # reference src/consensus_utils.cpp:12-13


def oracle_matrix(g, cfg, ci, cj, mx):
    """Consistency matrix assembled from the oracle's decisions; free cells are the AND of the diagonals."""
    N = g.N
    ok = np.zeros((N, N), dtype=np.uint8)
    solved = np.zeros((N, N), dtype=bool)
    for i, j, m in zip(ci, cj, mx):
        th = cfg.fast_reject_th if i == j else cfg.slow_reject_th
        ok[i, j] = ok[j, i] = 0 if m > th else 1
        solved[i, j] = solved[j, i] = True
    d = np.diag(ok).copy()
    free = ~solved
    ok[free] = (d[:, None] & d[None, :])[free]
    return ok
