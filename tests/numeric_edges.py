"""Aimed inputs for the pose algebra of the cell kernels and the cluster solvers: small pose graphs whose poses and loop
measurements sit on the numerical edges of SE2 / SE3 -- every branch of quat_from_R (se3_cell.hpp) for the poses, the
gauges and the error rotations, error quaternions with q_w -> 0 on both sides of the q_w >= 0 sign flip, heading errors
of +-pi, headings that cross +-pi inside a cell and at its gauge.

Plain module (no GPU use, no fixtures), the numerical counterpart of tests/edge_cells.py (which owns the layout edges):
tests/test_numeric_edges_cpu.py checks that every input lands on the edge its tag names and that the oracle alone is
right and well conditioned there; tests/test_gpu_numeric_edges.py runs one case per kernel body and the cluster solvers
on them and holds every result against the oracle.

Every loop measurement that is not an inlier is built from the oracle's propagated (open-loop) poses as
Z = X_ab * Rot(axis, angle), translation unchanged, so the error rotation at the start of the solve is Rot^-1 to
rounding.  The aimed SE3 loops of length 2 carry an information matrix with translation-rotation cross terms
(coupled_information): without them no output depends on the q_w >= 0 flip.  Positions are relative to the case's offset;
the longest cell of a case spans `span` poses.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from ipc_amd import synth
from ipc_amd.graphio import PoseGraph

from edge_cells import (SE2_SHIFT, SE3_SHIFT, _se2_chain, _tok, expected_cells, iteration_cap,     # noqa: F401
                        oracle_matrix, pair_shape)

Cand = namedtuple("Cand", "tag f t kind arg dup_of")   # kind: inlier | rot | quirk | shift | zero | dup; arg: (axis, angle) | metres

OFFSET = 37
TAIL = 3
PI = math.pi


# ---- the branch rule of quat_from_R, restated ----------------------------------------------------------------------------
def quat_branch(R):
    """Branch quat_from_R takes on the 3x3 rotation R: 'w' (positive trace), else the largest diagonal entry, ties to the
    lower index between 0 and 1 / 2, and to 1 between 1 and 2."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return "w"
    if R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        return "i0"
    if R[1, 1] > R[0, 0] and R[1, 1] >= R[2, 2]:
        return "i1"
    return "i2"


def quat_before_flip(R):
    """(x, y, z, w) as the taken branch of quat_from_R forms it, before the normalisation to q_w >= 0."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    b = quat_branch(R)
    q = np.zeros(4)
    if b == "w":
        t = math.sqrt(R[0, 0] + R[1, 1] + R[2, 2] + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[:3] = [(R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t]
    else:
        i = int(b[1])
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q / np.linalg.norm(q)


def quat_mul(a, b):
    """Hamilton product of two quaternions (x, y, z, w)."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def axis_angle_quat(axis, angle):
    """(x, y, z, w) of Rot(axis, angle); an angle of exactly pi gives w == 0 exactly."""
    n = np.asarray(axis, dtype=np.float64)
    n = n / np.linalg.norm(n)
    if angle == PI:
        return np.concatenate([n, [0.0]])
    return np.concatenate([n * math.sin(0.5 * angle), [math.cos(0.5 * angle)]])


# ---- the candidate lists -------------------------------------------------------------------------------------------------
SE3_ROT = {                                             # tag -> (axis, angle)
    "rot-x-pi-1e-3": ((1, 0, 0), PI - 1e-3),
    "rot-y-pi-1e-6": ((0, 1, 0), PI - 1e-6),
    "rot-z-pi": ((0, 0, 1), PI),
    "rot-111-pi-1e-9": ((1, 1, 1), PI - 1e-9),
    "rot-z-pi+1e-6": ((0, 0, 1), PI + 1e-6),           # the other side of the q_w sign flip
    "rot-123-120deg": ((1, 2, 3), 2 * PI / 3),         # trace == 0: the boundary between 'w' and the other branches
    "rot-skew-90deg": ((2, -1, 0.5), PI / 2),
    "rot-skew-30deg": ((-0.3, 1, 2), PI / 6),
    "rot-skew-5deg": ((1, -2, 0.7), PI / 36),
}
# A heading error of exactly pi sits on the cut of the angle: +pi and -pi are two different starts of the descent, one ulp
# of the measurement decides between them, and the max chi2 of the cells that hold such a loop moves by 7e-5 .. 4e-2
# relative (measured with the oracle) -- no parity bar can be held there.  1e-12 rad is the nearest the error comes to the
# cut while a rounding-level difference (a few thousand ulps of pi) still cannot carry it across.  In SE3 the error is
# the vector part of a quaternion, continuous through a half turn up to its sign, and exactly pi stays in the list.
SE2_ROT = {
    "head-pi-1e-12": PI - 1e-12,
    "head-pi-1e-9": PI - 1e-9,
    "head--pi+1e-9": -PI + 1e-9,
    "head-pi/2": PI / 2,
    "head-0.3": 0.3,
    "head-0.05": 0.05,
}


# Metres between the near-zero-residual loop and the composition of the propagated poses.  The positions reach 40 m, one
# ulp of which is 7e-15 m: a residual of 1e-6 m is known to 1e-8 relative at best, and its chi2 then moves by 1e-7 under
# one ulp of the measurement and differs by up to 4e-8 between two correct evaluations of the edge error, which is more
# than the conditions of tests/test_numeric_edges_cpu.py allow (1e-7, 1e-9).  1e-3 m keeps both two decades inside.
NEAR_ZERO = 1e-3


def _mid_len(span):
    return 36 if span < 100 else 48


def _mid_start(span, frac):
    return 2 + int(round(frac * (span - _mid_len(span) - 4)))


def se3_candidates(span, short):
    """short: start positions of the five loops of length 2 -- three whose gauge pose lies in branch i0, i1, i2, and a
    touching pair (u, u + 2), (u + 2, u + 4)."""
    S, Lm = span, _mid_len(span)
    p0, p1, p2, u = short
    m1 = _mid_start(S, 0.05)
    R = lambda tag, f, t: Cand(tag, f, t, "rot", SE3_ROT[tag], None)
    out = [
        Cand("inlier-long", 0, S, "inlier", None, None),
        Cand("inlier-mid", m1, m1 + Lm, "inlier", None, None),
        R("rot-x-pi-1e-3", p0, p0 + 2),
        # nested in inlier-long, staggered with inlier-mid: cells rejected only because of their second loop
        R("rot-y-pi-1e-6", m1 + Lm // 2, m1 + Lm // 2 + Lm),
        R("rot-z-pi", 1, S),
        R("rot-111-pi-1e-9", p1, p1 + 2),
        R("rot-z-pi+1e-6", _mid_start(S, 0.35) + Lm, _mid_start(S, 0.35)),         # reversed
        R("rot-123-120deg", p2, p2 + 2),
        R("rot-skew-90deg", _mid_start(S, 0.95), _mid_start(S, 0.95) + Lm),
        R("rot-skew-30deg", 0, S - 1),
        R("rot-skew-5deg", _mid_start(S, 0.2), _mid_start(S, 0.2) + Lm),
        # as the reference's injector emits it; short, like its local outliers: its translation is drawn about zero, and
        # tens of metres of translation error run the dog-leg into its iteration cap
        Cand("quirk-wxyz", u, u + 2, "quirk", None, None),
        Cand("shift", u + 2, u + 4, "shift", SE3_SHIFT, None),                     # touches quirk-wxyz: a free cell
        Cand("zero-residual", _mid_start(S, 0.6), _mid_start(S, 0.6) + Lm, "zero", 0.0, None),
        Cand("near-zero-residual", S, 0, "zero", NEAR_ZERO, None),                 # reversed
        Cand("duplicate", m1 + Lm // 2, m1 + Lm // 2 + Lm, "dup", None, 3),
    ]
    return out


def se2_candidates(span, short):
    """short: (pg, u) -- the loop (pg, pg + 2) starts at the pose whose heading is nearest to +-pi; (u, u + 2) and
    (u + 2, u + 4) touch."""
    S, Lm = span, _mid_len(span)
    pg, u = short
    m1 = _mid_start(S, 0.05)
    R = lambda tag, f, t: Cand(tag, f, t, "rot", SE2_ROT[tag], None)
    out = [
        Cand("inlier-long", 0, S, "inlier", None, None),
        Cand("inlier-mid", m1, m1 + Lm, "inlier", None, None),
        R("head-pi-1e-12", pg, pg + 2),
        R("head-pi-1e-9", m1 + Lm // 2, m1 + Lm // 2 + Lm),                        # nested / staggered with the inliers
        R("head--pi+1e-9", 1, S),
        R("head-pi/2", _mid_start(S, 0.5), _mid_start(S, 0.5) + 2),
        R("head-0.3", _mid_start(S, 0.35) + Lm, _mid_start(S, 0.35)),              # reversed
        R("head-0.05", 0, S - 1),
        Cand("shift", u + 2, u + 4, "shift", SE2_SHIFT, None),
        Cand("zero-residual", _mid_start(S, 0.6), _mid_start(S, 0.6) + Lm, "zero", 0.0, None),
        Cand("near-zero-residual", S, 0, "zero", NEAR_ZERO, None),                 # reversed
        Cand("duplicate", m1 + Lm // 2, m1 + Lm // 2 + Lm, "dup", None, 3),
        Cand("inlier-short", u, u + 2, "inlier", None, None),                      # touches shift: a free cell
        Cand("inlier-mid-b", _mid_start(S, 0.95), _mid_start(S, 0.95) + Lm, "inlier", None, None),
    ]
    return out


# ---- trajectories --------------------------------------------------------------------------------------------------------
def tumble_frames(V):
    """Orientations R_j = Rot(n_j, th_j) with R_0 = I: after a ramp over the first 24 poses the angle swings by 1.25 rad
    about pi with a period of 17 poses (trace > 0 beyond 60 degrees from pi: about a third of the poses), the axis
    precesses with a period of 41 poses on a cone about (1, 1, 1), so that each coordinate in turn is its largest.  Any
    64 consecutive poses hold all four branches of quat_from_R; consecutive poses differ by 28 degrees at the most."""
    j = np.arange(V)
    th = np.minimum(1.0, j / 24.0) * (PI + 1.25 * np.sin(2 * PI * j / 17.0))
    phase = 2 * PI * j / 41.0
    c = np.array([1.0, 1.0, 1.0]) / math.sqrt(3.0)
    e1 = np.array([1.0, -1.0, 0.0]) / math.sqrt(2.0)
    e2 = np.cross(c, e1)
    ax = c[None, :] + 0.6 * (np.cos(phase)[:, None] * e1[None, :] + np.sin(phase)[:, None] * e2[None, :])
    ax /= np.linalg.norm(ax, axis=1)[:, None]
    return np.stack([synth._rotvec_to_R(ax[k] * th[k]) for k in range(V)])


def coupled_information(upper, rng):
    """The 6 x 6 information `upper` (21 numbers) with its translation and rotation blocks coupled: covariance T C T^T,
    T = [[I, G], [0, I]], G uniform in +-0.4 times the ratio of the two blocks' standard deviations (correlations up to
    ~0.5).  synth._se3_info draws block-diagonal matrices; under those e^T Omega e does not change when the rotation part of
    e changes its sign, the Jacobians change theirs with it, and a quat_from_R without its q_w >= 0 flip solves every cell
    to the same bits -- the flip is observable only through the cross terms (found by the mutation check)."""
    Om = np.zeros((6, 6))
    Om[np.triu_indices(6)] = upper
    Om = Om + Om.T - np.diag(np.diag(Om))
    cov = np.linalg.inv(Om)
    T = np.eye(6)
    T[:3, 3:] = rng.uniform(-0.4, 0.4, (3, 3)) * math.sqrt(np.trace(cov[:3, :3]) / np.trace(cov[3:, 3:]))
    cov = T @ cov @ T.T
    return synth._upper(np.linalg.inv(0.5 * (cov + cov.T)))


def _first(pred, lo, hi, taken, width=2):
    for p in range(lo, hi):
        if pred(p) and all(abs(p - q) >= width + 1 for q in taken):
            return p
    raise RuntimeError("no pose with the wanted property in [%d, %d)" % (lo, hi))


# Seeds are part of the inputs: tests/test_numeric_edges_cpu.py holds the conditions on them.  A graph whose default
# seed misses one gets another one here.
SEED_OVERRIDES = {                                       # key: (dim, span)
    # SE2, default seeds 14192 / 14640 / 14768: the max chi2 of an inlier cell (chi2 0.04 .. 0.2, nothing aimed in it) moves
    # by 0.8e-7 / 1.5e-7 / 2.5e-7 relative when every loop measurement moves by one ulp; the condition is 1e-7
    (2, 192): 14193,
    (2, 640): 14644,
    (2, 768): 14771,
}


def default_seed(dim, span):
    return SEED_OVERRIDES.get((dim, span), 7000 * dim + span)


@functools.lru_cache(maxsize=16)
def numeric_graph(dim, span, seed=None):
    """PoseGraph of OFFSET + span + 1 + TAIL vertices with the aimed candidates; meta["tags"] names them, meta["cands"]
    holds the list.  Cached: callers must not modify it."""
    from oracle import oracle as O
    if seed is None:
        seed = default_seed(dim, span)
    V = OFFSET + span + 1 + TAIL
    off = OFFSET
    if dim == 2:
        rng = np.random.default_rng(seed)
        gt, odom_meas, odom_info, verts = _se2_chain(V, rng)
        P = O.propagate(2, odom_meas)
        dist = np.abs(np.abs(P[:, 2]) - PI)
        pg = int(np.argmin(dist[off + 2:off + span - 3])) + 2
        u = _first(lambda p: True, span // 3, span - 5, [pg], width=4)
        cands = se2_candidates(span, (pg, u))
        pairs = [(off + c.f, off + c.t) for c in cands]
        loop_meas = np.zeros((len(pairs), 3))
        loop_info = np.zeros((len(pairs), 6))
        for k, (a, b) in enumerate(pairs):
            cov, inf = synth._se2_info(rng, 0.05, 0.02)
            z = synth._se2_between(gt[a], gt[b]) + rng.multivariate_normal(np.zeros(3), cov)
            z[2] = synth._wrap(z[2])
            loop_meas[k] = z
            loop_info[k] = synth._upper(inf)
        g = PoseGraph(2, verts, odom_meas, odom_info, np.array(pairs, dtype=np.int32), loop_meas, loop_info, {})
        for k, (c, (a, b)) in enumerate(zip(cands, pairs)):
            if c.kind in ("inlier", "dup"):
                continue
            r = np.asarray(O.pose_mul(2, O.pose_inv(2, P[a]), P[b])[:3], dtype=np.float64)
            if c.kind == "rot":
                r[2] = O.normalize_theta(r[2] + c.arg)
            else:                                          # shift, zero, near-zero: metres added to the translation
                r[0] += c.arg
            g.loop_meas[k] = r
    else:
        rng = np.random.default_rng(seed)
        s = np.arange(V) * 0.05
        pos = np.stack([20 * np.cos(s) + 0.002 * np.arange(V), 20 * np.sin(s),
                        0.01 * np.arange(V) % 7.0 + np.cumsum(rng.normal(0, 0.01, V))], axis=1)
        Rs = tumble_frames(V)
        g0 = synth._se3_graph(Rs, pos, [], seed, name="tumble")        # the odometry does not depend on the loop list
        P = O.propagate(3, g0.odom_meas)
        br = [quat_branch(p[:9]) for p in P]
        taken = []
        for want in ("i0", "i1", "i2"):
            taken.append(_first(lambda p: br[off + p] == want, 2, span - 3, taken))
        taken.append(_first(lambda p: True, span // 3, span - 5, taken, width=4))
        cands = se3_candidates(span, tuple(taken))
        pairs = [(off + c.f, off + c.t) for c in cands]
        g = synth._se3_graph(Rs, pos, pairs, seed, name="tumble")
        assert np.array_equal(g.odom_meas, g0.odom_meas)
        quirk = synth.sample_outliers(3, V, 1, seed)[1][0]
        rng_c = np.random.default_rng(seed + 1000003)
        for k, (c, (a, b)) in enumerate(zip(cands, pairs)):
            if c.kind in ("inlier", "dup"):
                continue
            if abs(c.f - c.t) == 2:                       # (on the longer chains the coupled half turns run into the iteration
                g.loop_info[k] = coupled_information(g.loop_info[k], rng_c)     # cap, and exactly pi becomes a cut as in SE2)
            if c.kind == "quirk":
                g.loop_meas[k] = quirk
                continue
            X = O.pose_mul(3, O.pose_inv(3, P[a]), P[b])
            t, q = np.array(X[9:12]), synth._R_to_quat(X[:9].reshape(3, 3))
            if c.kind == "rot":
                q = quat_mul(q, axis_angle_quat(*c.arg))
            else:
                t[0] += c.arg
            g.loop_meas[k] = np.concatenate([t, q])
    for k, c in enumerate(cands):
        if c.dup_of is not None:
            g.loop_meas[k] = g.loop_meas[c.dup_of]
            g.loop_info[k] = g.loop_info[c.dup_of]
    g.meta = dict(name="numeric-se%d-%d" % (dim, span), seed=seed, tags=[c.tag for c in cands], offset=off, cands=cands,
                  span=span)
    for a in (g.vertices, g.odom_meas, g.odom_info, g.loop_ids, g.loop_meas, g.loop_info):
        a.setflags(write=False)
    return g


# ---- the cases of tests/test_gpu_numeric_edges.py: one per code body -----------------------------------------------------
Case = namedtuple("Case", "id dim token span env")
MAX_SPAN = 768


def _cases():
    out = []
    for tok in ("w3", "p5", "q7", "16x4", None):
        cap = MAX_SPAN if tok is None else 64 * _tok(2, tok)[1] * _tok(2, tok)[2]
        span = cap if tok is not None and tok[0] == "w" else min(cap, MAX_SPAN)
        out.append(Case("se2-" + (tok or "default"), 2, tok, span, {"IPC_SE2_POLICY": tok} if tok else {}))
    for tok in ("w1", "w3", "g3", "1x1", "2x2", "16x4", None):
        cap = MAX_SPAN if tok is None else 64 * _tok(3, tok)[1] * _tok(3, tok)[2]
        span = cap if tok is not None and tok[0] == "w" else min(cap, MAX_SPAN)
        out.append(Case("se3-" + (tok or "default"), 3, tok, span,
                        {"IPC_SE3_POLICY": tok, "IPC_SE3_LATENCY_POLICY": "none"} if tok else {}))
    return out


CASES = _cases()
GRAPHS = sorted({(c.dim, c.span) for c in CASES})        # several cases share one graph
SMALLEST = {dim: min(s for d, s in GRAPHS if d == dim) for dim in (2, 3)}


def case_graph(case):
    return numeric_graph(case.dim, case.span)


def config(dim):
    from ipc_amd.consensus import Config
    return Config() if dim == 2 else Config(s_factor=50.0, slow_reject_th=6.251)


def solve_cells(g, cfg, nthreads, loop_meas=None):
    """(i, j, max chi2, iterations) of the oracle on every expected cell of g (optionally with other measurements)."""
    from oracle import oracle as O
    cells = expected_cells(g.loop_ids)
    ci = np.array([c[0] for c in cells], dtype=np.int32)
    cj = np.array([c[1] for c in cells], dtype=np.int32)
    poses = O.propagate(g.dim, g.odom_meas)
    mx, its, _ = O.pair_cells_mt(g.dim, g.odom_meas, g.odom_info, cfg.s_factor, poses, g.loop_ids,
                                 g.loop_meas if loop_meas is None else loop_meas, g.loop_info, ci, cj,
                                 cfg.fast_reject_iter_base, cfg.slow_reject_iter_base, nthreads)
    return ci, cj, mx, its


@functools.lru_cache(maxsize=16)
def oracle_cells(dim, span, nthreads):
    """The oracle's plain run on a graph; computed once and shared by the tests, read-only."""
    g = numeric_graph(dim, span)
    out = solve_cells(g, config(dim), nthreads)
    for a in out:
        a.setflags(write=False)
    return out
