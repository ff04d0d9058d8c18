"""Conditions on the aimed inputs of tests/numeric_edges.py, checked without a GPU: every input lands on the numerical
edge its tag names (by a restatement of quat_from_R's branch rule and by scipy's Rotation class), the oracle's edge
errors there are those of the independent algebra of tests/test_oracle_independent.py, and the oracle alone is well
away from every threshold and iteration cap and insensitive to rounding -- so that a disagreement of a kernel or a
cluster solver in tests/test_gpu_numeric_edges.py is a disagreement about the pose algebra, not about a borderline or
ill-conditioned cell.  Conditions, not measurements: an input that misses one is re-aimed in numeric_edges.py."""
import math
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import numeric_edges as NE
import test_oracle_independent as TI

GRAPH_IDS = ["se%d-%d" % gs for gs in NE.GRAPHS]
SE3_GRAPHS = [gs for gs in NE.GRAPHS if gs[0] == 3]
SE2_GRAPHS = [gs for gs in NE.GRAPHS if gs[0] == 2]
NTHREADS = min(16, os.cpu_count() or 1)
BRANCHES = ("w", "i0", "i1", "i2")


def _ranges(g):
    return [(int(min(a, b)), int(max(a, b))) for a, b in g.loop_ids]


def _rel_diff(a, b, floor=1e-12):
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def _start_error_rotation(g, P, k):
    """Z^-1 X_a^-1 X_b of loop k at the propagated poses, with scipy's Rotation."""
    a, b = g.loop_ids[k]
    Ra = Rotation.from_matrix(P[a][:9].reshape(3, 3))
    Rb = Rotation.from_matrix(P[b][:9].reshape(3, 3))
    q = np.asarray(g.loop_meas[k][3:7])
    return Rotation.from_quat(q / np.linalg.norm(q)).inv() * Ra.inv() * Rb


def test_the_cases_cover_every_code_body_at_the_stated_sizes():
    want = {"se2-w3": 192, "se2-p5": 640, "se2-q7": 768, "se2-16x4": 768, "se2-default": 768,
            "se3-w1": 64, "se3-w3": 192, "se3-g3": 768, "se3-1x1": 64, "se3-2x2": 256, "se3-16x4": 768, "se3-default": 768}
    assert {c.id: c.span for c in NE.CASES} == want
    for c in NE.CASES:
        if c.token is None:
            assert c.env == {}
        elif c.dim == 2:
            assert c.env == {"IPC_SE2_POLICY": c.token}
        else:
            assert c.env == {"IPC_SE3_POLICY": c.token, "IPC_SE3_LATENCY_POLICY": "none"}
        if c.token is not None:
            fam, W, M = NE._tok(c.dim, c.token)
            cap = 64 * W * M
            assert c.span == (cap if W == 1 else min(cap, 768))
            # both layouts put 64 M consecutive poses into one wave: every wave of p5 and g3 holds poses of the longest
            # cell, at least two waves of the other multi-wave variants do
            waves = -(-c.span // (64 * M))
            assert waves == W if c.token in ("w1", "w3", "p5", "g3", "1x1", "2x2") else 2 <= waves < W, (c.id, waves)
    assert NE.SMALLEST == {2: 192, 3: 64}


@pytest.mark.parametrize("dim,span", NE.GRAPHS, ids=GRAPH_IDS)
def test_the_lists_hold_the_required_candidates_and_shapes(dim, span):
    g = NE.numeric_graph(dim, span)
    cands, tags, off = g.meta["cands"], g.meta["tags"], g.meta["offset"]
    rng = _ranges(g)
    assert g.V == off + span + 1 + NE.TAIL and g.V <= 830 and off % 64 != 0
    assert 12 <= len(cands) <= 16 and len(set(tags)) == len(tags)
    assert len(NE.expected_cells(g.loop_ids)) <= 136
    for k, c in enumerate(cands):
        assert tuple(g.loop_ids[k]) == (off + c.f, off + c.t) and 0 <= min(c.f, c.t) and max(c.f, c.t) <= span, c
    assert max(hi - lo for lo, hi in rng) == span and min(lo for lo, _ in rng) == off
    want = set(NE.SE3_ROT if dim == 3 else NE.SE2_ROT) | {"shift", "zero-residual", "near-zero-residual", "duplicate"}
    want |= {"quirk-wxyz"} if dim == 3 else set()
    assert want <= set(tags) and sum(c.kind == "inlier" for c in cands) >= 2
    kinds = {}
    for c in cands:
        kinds.setdefault(c.kind, []).append(abs(c.f - c.t))
    for kind in ("inlier", "rot"):                           # chain lengths: 2, one of 30 - 60, near the longest cell
        L = kinds[kind]
        assert (dim == 3 and kind == "inlier") or 2 in L
        assert any(30 <= x <= 60 for x in L) and any(x >= span - 1 for x in L), (kind, L)
    assert 2 in kinds["shift"] + kinds["inlier"]
    dup = tags.index("duplicate")
    src = cands[dup].dup_of
    assert cands[src].kind == "rot" and rng[dup] == rng[src]
    assert np.array_equal(g.loop_meas[dup], g.loop_meas[src]) and np.array_equal(g.loop_info[dup], g.loop_info[src])
    if dim == 3:
        from ipc_amd import synth
        q = tags.index("quirk-wxyz")
        m = synth.sample_outliers(3, g.V, 1, g.meta["seed"])[1][0]
        assert np.array_equal(g.loop_meas[q], m) and abs(m[3]) > 0.9        # "w" sits in the slot read as qx
    # pair shapes: inlier x rotation outlier nested and staggered (inlier first: the cell is rejected only because of its
    # second loop), two rotation outliers about different axes, a touching pair
    shapes = set()
    two_rot = False
    for i in range(len(cands)):
        for j in range(i + 1, len(cands)):
            sh = NE.pair_shape(rng[i], rng[j])
            if cands[i].kind == "inlier" and cands[j].kind == "rot" and abs(cands[j].f - cands[j].t) >= 30:
                shapes.add(sh)
            if sh == "touching":
                shapes.add("touching")
            if cands[i].kind == cands[j].kind == "rot" and sh in ("nested", "staggered"):
                two_rot |= dim == 2 or not np.allclose(np.cross(cands[i].arg[0], cands[j].arg[0]), 0)
    assert {"nested", "staggered", "touching"} <= shapes and two_rot


@pytest.mark.parametrize("dim,span", SE3_GRAPHS, ids=["se3-%d" % s for _, s in SE3_GRAPHS])
def test_se3_tags_land_on_every_branch(oracle, dim, span):
    O = oracle
    g = NE.numeric_graph(dim, span)
    cands, tags, off = g.meta["cands"], g.meta["tags"], g.meta["offset"]
    P = O.propagate(3, g.odom_meas)
    br = [NE.quat_branch(p[:9]) for p in P]
    # scipy agrees with the restated rule on which component is the largest (its own conversion picks it the same way)
    count = {b: br[off:off + span + 1].count(b) for b in BRANCHES}
    assert all(count[b] >= 8 for b in BRANCHES), count
    ci, cj = zip(*NE.expected_cells(g.loop_ids))
    lo = g.loop_ids.min(1)
    gauges = {br[min(lo[i], lo[j])] for i, j in zip(ci, cj)}
    assert {"i0", "i1", "i2"} <= gauges, gauges
    ebr, qw = {}, {}
    for k, c in enumerate(cands):
        E = _start_error_rotation(g, P, k)
        ebr[c.tag] = NE.quat_branch(E.as_matrix())
        qw[c.tag] = abs(E.as_quat()[3])
        if c.kind == "rot":
            stated = c.arg[1] if c.arg[1] <= math.pi else 2 * math.pi - c.arg[1]
            assert abs(E.magnitude() - stated) <= 1e-6, (c.tag, E.magnitude(), stated)
            # the axis is the stated one (the error is Rot^-1), up to the sign that a half turn leaves open
            n = np.asarray(c.arg[0], dtype=np.float64)
            rv = E.as_rotvec()
            assert abs(abs(rv @ n) / (np.linalg.norm(rv) * np.linalg.norm(n)) - 1.0) <= 1e-6, c.tag
    assert set(ebr.values()) == set(BRANCHES), ebr
    assert ebr["rot-x-pi-1e-3"] == "i0" and ebr["rot-y-pi-1e-6"] == "i1" and ebr["rot-z-pi"] == "i2"
    assert ebr["rot-skew-5deg"] == ebr["inlier-long"] == "w"
    assert min(qw.values()) < 1e-8 and qw["rot-z-pi"] < 1e-12 and qw["rot-111-pi-1e-9"] < 1e-8
    # pi - 1e-6 and pi + 1e-6 about z: the same |q_w|, opposite signs before the q_w >= 0 flip
    Em = _start_error_rotation(g, P, tags.index("rot-y-pi-1e-6")).as_quat()
    Ep = _start_error_rotation(g, P, tags.index("rot-z-pi+1e-6")).as_quat()
    assert abs(abs(Em[3]) - 5e-7) < 1e-9 and abs(abs(Ep[3]) - 5e-7) < 1e-9
    assert (Em[3] * Em[1] > 0) != (Ep[3] * Ep[2] > 0)
    # the q_w >= 0 flip is observable: under a block-diagonal information e^T Omega e keeps its value when the rotation part
    # of e changes sign (and so does every cell: a quat_from_R without the flip gives the same bits), so the aimed loops
    # of length 2 carry translation-rotation cross terms, and some of their errors have q_w < 0 before the flip
    flipped = clearly = 0
    for k, c in enumerate(cands):
        Om = _sym(g.loop_info[k], 6)
        cross = np.linalg.norm(Om[:3, 3:]) / math.sqrt(np.linalg.norm(Om[:3, :3]) * np.linalg.norm(Om[3:, 3:]))
        E = _start_error_rotation(g, P, k).as_matrix()
        assert np.allclose(Rotation.from_quat(NE.quat_before_flip(E)).as_matrix(), E, atol=1e-12), c.tag
        if c.kind not in ("inlier", "dup") and abs(c.f - c.t) == 2:
            assert cross > 0.05, (c.tag, cross)
            flipped += NE.quat_before_flip(E)[3] < 0
            clearly += NE.quat_before_flip(E)[3] < -1e-4
        else:
            assert cross < 1e-9, (c.tag, cross)
    assert flipped >= 2 and clearly >= 1, (flipped, clearly)
    # the trace of the 120 degree error is zero to rounding: the branch boundary
    assert abs(np.trace(_start_error_rotation(g, P, tags.index("rot-123-120deg")).as_matrix())) < 1e-12
    print("se3-%d: pose branches %s, gauges %s, error branches %s, smallest error q_w %.3g"
          % (span, count, sorted(gauges), ebr, min(qw.values())))


@pytest.mark.parametrize("dim,span", SE2_GRAPHS, ids=["se2-%d" % s for _, s in SE2_GRAPHS])
def test_se2_tags_land_on_the_heading_edges(oracle, dim, span):
    O = oracle
    g = NE.numeric_graph(dim, span)
    cands = g.meta["cands"]
    P = O.propagate(2, g.odom_meas)
    for k, c in enumerate(cands):
        a, b = g.loop_ids[k]
        e = TI.se2_err(g.loop_meas[k], P[a], P[b])
        if c.kind == "rot":                                  # Z = X_ab Rot(d): the error is -d, and +-pi are one angle
            assert abs(TI.wrap(e[2] + c.arg)) <= 1e-14, (c.tag, e[2])
            assert abs(abs(e[2]) - abs(c.arg)) <= 1e-14 and abs(e[0]) < 1e-9 and abs(e[1]) < 1e-9, (c.tag, e)
            assert abs(e[2]) < math.pi - 0.5 * (math.pi - abs(c.arg)) or abs(c.arg) < 3, (c.tag, e[2])   # its side of the cut
        elif c.kind in ("zero", "shift"):
            assert abs(e[2]) <= 1e-12 and abs(math.hypot(e[0], e[1]) - c.arg) <= 1e-9, (c.tag, e)
    th = P[:, 2]
    cross = np.nonzero(np.abs(np.diff(th)) > math.pi)[0]    # the heading wraps between vertex q and q + 1
    lo, hi = g.loop_ids.min(1), g.loop_ids.max(1)
    cells = NE.expected_cells(g.loop_ids)
    with_cross = [(i, j) for i, j in cells
                  if np.any((cross >= min(lo[i], lo[j])) & (cross < max(hi[i], hi[j])))]
    assert len(with_cross) >= 3
    gauge = min(abs(abs(th[min(lo[i], lo[j])]) - math.pi) for i, j in cells)
    assert gauge <= 0.02, gauge
    print("se2-%d: %d crossings of +-pi, %d of %d cells hold one, nearest gauge heading %.3g rad from +-pi, "
          "largest heading error at the start %.6f rad"
          % (span, len(cross), len(with_cross), len(cells), gauge,
             max(abs(TI.se2_err(g.loop_meas[k], P[g.loop_ids[k][0]], P[g.loop_ids[k][1]])[2]) for k in range(g.N))))


def _sym(up, d):
    return TI._sym(np.asarray(up), d)


@pytest.mark.parametrize("dim,span", NE.GRAPHS, ids=GRAPH_IDS)
def test_oracle_edge_errors_are_those_of_the_independent_algebra(oracle, dim, span):
    """chi2 = e^T Omega e of every aimed loop at the starting poses; chi2, not e: at exactly pi both e and -e are right."""
    O = oracle
    g = NE.numeric_graph(dim, span)
    P = O.propagate(dim, g.odom_meas)
    worst = 0.0
    for k, c in enumerate(g.meta["cands"]):
        a, b = g.loop_ids[k]
        Om = _sym(g.loop_info[k], 3 if dim == 2 else 6)
        e = O.edge_error(dim, O.meas_to_pose(dim, g.loop_meas[k]), P[a], P[b])
        if dim == 2:
            ei = TI.se2_err(g.loop_meas[k], P[a], P[b])
        else:
            X = [TI.P3(Rotation.from_matrix(P[v][:9].reshape(3, 3)), P[v][9:]) for v in (a, b)]
            ei = TI.se3_err(TI.P3.from_meas(g.loop_meas[k]), X[0], X[1])
        chi, chi_i = float(e @ Om @ e), float(ei @ Om @ ei)
        rel = abs(chi - chi_i) / max(abs(chi_i), 1e-12)
        worst = max(worst, rel)
        assert rel <= 1e-9, (c.tag, chi, chi_i)
    print("se%d-%d: worst relative difference of the starting chi2 %.3g" % (dim, span, worst))


def _moved_by_one_ulp(meas):
    return np.nextafter(meas, np.inf)


@pytest.mark.parametrize("dim,span", NE.GRAPHS, ids=GRAPH_IDS)
def test_oracle_alone_is_well_conditioned(oracle, dim, span):
    O = oracle
    g = NE.numeric_graph(dim, span)
    cfg = NE.config(dim)
    tags = g.meta["tags"]
    ci, cj, mx, its = NE.oracle_cells(dim, span, NTHREADS)
    cells = NE.expected_cells(g.loop_ids)
    assert cells == list(zip(ci.tolist(), cj.tolist())) and not np.isnan(mx).any()
    lo, hi = g.loop_ids.min(1), g.loop_ids.max(1)
    N = g.N
    rng = _ranges(g)
    free = [(i, j) for i in range(N) for j in range(i + 1, N) if (i, j) not in set(cells)]
    assert any(NE.pair_shape(rng[i], rng[j]) == "touching" for i, j in free)      # touching loops: a free cell
    diag_ok = {}
    n_acc = n_rej = second = 0
    for i, j, m, it in zip(ci.tolist(), cj.tolist(), mx.tolist(), its.tolist()):
        nl = 1 if i == j else 2
        th = cfg.fast_reject_th if i == j else cfg.slow_reject_th
        L = max(hi[i], hi[j]) - min(lo[i], lo[j])
        assert abs(m - th) > 0.01 * th, ("within 1 % of the threshold", tags[i], tags[j], m)
        assert it < NE.iteration_cap(cfg, L, nl), ("iteration cap", tags[i], tags[j], it)
        if i == j:
            diag_ok[i] = not (m > th)
        n_acc += not (m > th)
        n_rej += bool(m > th)
    for i, j, m in zip(ci.tolist(), cj.tolist(), mx.tolist()):
        if i != j and m > cfg.slow_reject_th and diag_ok[i] and not diag_ok[j]:
            second += 1
    assert n_acc >= 3 and n_rej >= 3, (n_acc, n_rej)
    assert second >= 1                                      # rejected only because of its second loop
    # rounding: other summation order in the factorisation; every loop measurement one ulp up
    O.set_wide_dots(True)
    try:
        _, _, mx_wide, _ = NE.solve_cells(g, cfg, NTHREADS)
    finally:
        O.set_wide_dots(False)
    _, _, mx_ulp, _ = NE.solve_cells(g, cfg, NTHREADS, loop_meas=_moved_by_one_ulp(g.loop_meas))
    worst = 0.0
    for other, what in ((mx_wide, "wide dots"), (mx_ulp, "one ulp")):
        rel = _rel_diff(other, mx)
        w = int(np.argmax(rel))
        worst = max(worst, rel[w])
        assert rel[w] <= 1e-7, (what, tags[ci[w]], tags[cj[w]], mx[w], other[w])
    print("se%d-%d: %d cells, %d accepted, %d rejected, max iterations %d, worst move under rounding %.3g"
          % (dim, span, len(cells), n_acc, n_rej, int(its.max()), worst))


@pytest.mark.parametrize("dim", [2, 3])
def test_faithful_run_on_the_smallest_graph_is_well_conditioned(oracle, dim):
    O = oracle
    g = NE.numeric_graph(dim, NE.SMALLEST[dim])
    cfg = NE.config(dim)
    tags = g.meta["tags"]
    inc = O.IncrementalIPC(dim, g.odom_meas, g.odom_info, cfg.s_factor, cfg.fast_reject_th, cfg.fast_reject_iter_base,
                           cfg.slow_reject_th, cfg.slow_reject_iter_base, g.loop_ids, g.loop_meas, g.loop_info)
    n_acc = n_cluster = 0
    for k in O.candidate_order(g.loop_ids):
        ok, ref = inc.agreement_check(int(k))
        th = cfg.slow_reject_th if ref["cluster"] else cfg.fast_reject_th
        m = ref["max_chi2"]
        assert m == m and abs(m - th) > 0.01 * th, ("within 1 % of the threshold", tags[k], m)
        assert ok == (not (m > th))
        assert ref["iterations"] < NE.iteration_cap(cfg, ref["hi"] - ref["lo"], ref["cluster"] + 1), (tags[k], ref)
        n_acc += ok
        n_cluster += ref["cluster"] > 0
    assert n_acc >= 3 and g.N - n_acc >= 3 and n_cluster >= 3
    assert len(inc.consensus()) == n_acc
