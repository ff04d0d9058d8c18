"""Conditions on the aimed inputs of tests/edge_cells.py, checked without a GPU: the tagged positions land where the
tags say (by a restatement of each kernel family's index formula), the expected cell set is the overlap rule, and the
oracle alone is well away from every threshold and iteration cap -- so that a disagreement of a kernel in
tests/test_gpu_variant_edges.py is a disagreement about the layout, not about a borderline cell."""
import os

import numpy as np
import pytest

import edge_cells as EC

IDS = [c.id for c in EC.CASES]


def _ranges(g):
    off = g.meta["offset"]
    return [(min(c.f, c.t), max(c.f, c.t)) for c in g.meta["cands"]], off


@pytest.mark.parametrize("case", EC.CASES, ids=IDS)
def test_tags_land_where_they_say(case):
    g = EC.case_graph(case)
    cands, fam, W, M = g.meta["cands"], case.family, case.W, case.M
    C = 64 * W * M
    assert g.V == case.offset + C + 1 + case.tail
    assert 8 >= len(cands) if case.small else 12 <= len(cands) <= 16
    assert len(EC.expected_cells(g.loop_ids)) <= 136
    for k, c in enumerate(cands):
        assert tuple(g.loop_ids[k]) == (case.offset + c.f, case.offset + c.t), c.tag
        L = abs(c.f - c.t)
        for claim in c.claims:
            if claim[0] == "L":
                assert L == claim[1], c
            elif claim[0] == "fill":
                # the kernel's own view: lane layout -- lanes gl with gl * M < L are busy, the last holds L - gl * M poses
                if fam == "lane":
                    gl = (L - 1) // M
                    assert gl * M < L <= (gl + 1) * M and L - gl * M == claim[1], c
                else:
                    assert (L - 1) % 64 + 1 == claim[1], c
            else:
                p = c.f if claim[0] == "f" else c.t
                rel = p - min(c.f, c.t)                        # pose index inside the candidate's own (diagonal) cell
                if claim[1] == "gauge":
                    assert rel == 0, c
                elif claim[1] == "last":
                    assert p == C and (case.tail != 0 or case.offset + p == g.V - 1), c
                elif claim[1] == "place":
                    assert EC.place_of(W, M, p) == claim[2], c
                else:
                    # owners are stated for the cell that starts at the offset (lo == 0): the whole-capacity pairs
                    wave, lane, slot = EC.owner(fam, W, M, p)
                    if fam == "lane":
                        assert (p - 1) // M == wave * 64 + lane and (p - 1) % M == slot, c
                    else:
                        assert p == wave * 64 * M + slot * 64 + lane + 1, c
                    assert 0 <= wave < W and 0 <= lane < 64 and 0 <= slot < M, c
                    if claim[1] == "owner":
                        assert (wave, lane, slot) == claim[2], c
                    else:
                        assert slot == claim[2], c
    # unstaged runs: the staged window alone (88 bytes per record, V - 1 + 32 records) is beyond the 160 KB of LDS
    if case.id.endswith("-unstaged"):
        assert g.V >= EC.UNSTAGED_MIN_V and 88 * (g.V - 1 + 32) > 160 * 1024 and case.offset % 64 != 0
    elif case.token is not None:
        assert case.offset % 64 != 0 and case.tail == 0      # lo_abs != 0; the last candidate vertex ends the chain


@pytest.mark.parametrize("case", EC.CASES, ids=IDS)
def test_required_shapes_are_present(case):
    g = EC.case_graph(case)
    rng, _ = _ranges(g)
    cands, W, M = g.meta["cands"], case.W, case.M
    C = 64 * W * M
    shapes = {}
    for i in range(len(cands)):
        for j in range(i + 1, len(cands)):
            sh = EC.pair_shape(rng[i], rng[j])
            if sh is None:
                continue
            rev = (cands[i].f > cands[i].t) != (cands[j].f > cands[j].t)
            lo, hi = min(rng[i][0], rng[j][0]), max(rng[i][1], rng[j][1])
            cuts = [p for p in rng[i] + rng[j] if lo < p < hi] if sh != "touching" else []
            shapes.setdefault(sh, []).append((rev, (lo, hi), tuple(cuts), i, j))
    for sh in ("staggered", "nested", "same-start", "same-end", "identical", "touching"):
        assert sh in shapes, sh
        assert any(r[0] for r in shapes[sh]), sh + ": no instance with one loop reversed"
    dup = [k for k, c in enumerate(cands) if c.dup_of is not None]
    if not case.small:
        assert dup and all(np.array_equal(g.loop_meas[k], g.loop_meas[cands[k].dup_of]) for k in dup)
    # a two-loop cell of exactly cap poses that neither loop spans alone
    assert any(max(rng[i][1], rng[j][1]) - min(rng[i][0], rng[j][0]) == C and rng[i][1] - rng[i][0] < C
               and rng[j][1] - rng[j][0] < C and EC.pair_shape(rng[i], rng[j]) == "staggered"
               for i in range(len(cands)) for j in range(i + 1, len(cands)))
    ends = {p for c in cands for p in (c.f, c.t)}
    assert {0, C} <= ends
    if case.family == "lane":
        slots = {EC.owner("lane", W, M, p)[2] for p in ends if p > 0}
        assert {0, M - 1} <= slots
        for k in range(1, W):
            assert {64 * M * k, 64 * M * k + 1} <= ends, k
    else:
        if M >= 2 and W * M >= 3:
            assert {64, 65} <= ends
        if W >= 2:
            assert {64 * M, 64 * M + 1} <= ends
        if case.dim == 3 and not case.small:
            # class changes of the SE3 LDS kernels (poses <= p keep their class, later ones change): for every shape with
            # a change, one inside a 64-pose block, one on a block boundary (M >= 2), one on a wave boundary (W >= 2; the
            # nested shape needs two interior wave boundaries, W >= 4)
            for sh in ("staggered", "nested", "same-start", "same-end"):
                places = set()
                for _, cell, cuts, i, j in shapes[sh]:
                    places |= {EC.place_of(W, M, p - cell[0]) for p in cuts if cell[0] == 0}
                want = {"in"} | ({"block"} if M >= 2 and W * M >= 3 else set())
                if W >= 4 or (W >= 2 and sh != "nested"):
                    want.add("wave")
                assert want <= places, (sh, want, places)


@pytest.mark.parametrize("case", EC.CASES, ids=IDS)
def test_oracle_alone_is_well_conditioned(oracle, case):
    g = EC.case_graph(case)
    cfg = EC.case_config(case)
    ci, cj, mx, its = EC.oracle_cells(case, min(16, os.cpu_count() or 1))
    # the expected set is the overlap rule, and the oracle agrees that exactly these cells exist (NaN: no overlap)
    cells = EC.expected_cells(g.loop_ids)
    assert cells == list(zip(ci.tolist(), cj.tolist())) and not np.isnan(mx).any()
    lo, hi = g.loop_ids.min(1), g.loop_ids.max(1)
    N = g.N
    assert all((i, i) in cells for i in range(N))
    free = [(i, j) for i in range(N) for j in range(i + 1, N) if (i, j) not in set(cells)]
    assert all(hi[i] <= lo[j] or hi[j] <= lo[i] for i, j in free)
    rng, _ = _ranges(g)
    assert any(EC.pair_shape(rng[i], rng[j]) == "touching" for i, j in free)      # touching loops: a free cell
    diag_ok = {}
    n_acc = n_rej = second = 0
    for i, j, m, it in zip(ci.tolist(), cj.tolist(), mx.tolist(), its.tolist()):
        nl = 1 if i == j else 2
        th = cfg.fast_reject_th if i == j else cfg.slow_reject_th
        L = max(hi[i], hi[j]) - min(lo[i], lo[j])
        assert abs(m - th) > 0.01 * th, ("within 1 % of the threshold", i, j, m)
        assert it < EC.iteration_cap(cfg, L, nl), ("iteration cap", i, j, it)
        if i == j:
            diag_ok[i] = not (m > th)
        n_acc += not (m > th)
        n_rej += bool(m > th)
    for i, j, m in zip(ci.tolist(), cj.tolist(), mx.tolist()):
        if i != j and m > cfg.slow_reject_th and diag_ok[i] and not diag_ok[j]:
            second += 1
    assert n_acc >= 3 and n_rej >= 3, (n_acc, n_rej)
    assert second >= 1                                      # rejected only because of its second loop
    print("%s: %d cells, %d accepted, %d rejected, max iterations %d" % (case.id, len(cells), n_acc, n_rej, int(its.max())))
