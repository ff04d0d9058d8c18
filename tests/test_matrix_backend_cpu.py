"""Conditions on the injected inputs of tests/matrix_cases.py, checked without a GPU: the two plain references agree
with the oracle's, and by the references alone the inputs decide something where the kernels' own structure sits
(inside a round of 64 live candidates, across rounds, on both select paths of the assembly) -- so that
tests/test_gpu_matrix_backend.py cannot pass trivially."""
import functools

import numpy as np
import pytest

import edge_cells as EC
import matrix_cases as MC

SET_IDS = [c.id for c in MC.SET_CASES]


@functools.lru_cache(maxsize=None)
def _diagnostics(case):
    order = MC.set_order(case.N)
    ok = MC.set_matrix(case)
    return MC.ref_set_max(ok, order), MC.round_mate_rejects(ok, order), MC.joins_past_rejected_mate(ok, order)


@pytest.mark.parametrize("case", MC.SET_CASES, ids=SET_IDS)
def test_set_max_references_agree(oracle, case):
    order = MC.set_order(case.N)
    ok = MC.set_matrix(case)
    assert ok.shape == (case.N, case.N) and np.array_equal(ok, ok.T)
    g = MC.graph_for(order)
    assert np.array_equal(oracle.candidate_order(g.loop_ids), order)
    acc = _diagnostics(case)[0]
    assert np.array_equal(acc, oracle.set_max(ok.astype(np.uint8), order))
    exp = MC.set_expected(case, ok, order)
    if exp is not None:
        assert np.array_equal(acc, exp)
    if case.gen == "nlive_exact":
        assert int(np.diag(ok).sum()) == case.arg
    if case.gen == "late_live":
        assert not ok[order[:1024], order[:1024]].any()


def test_order_exercises_the_tie_rule():
    for N in MC.SET_SIZES:
        order = MC.set_order(N)
        hi = MC.graph_for(order).loop_ids.max(1)
        if N >= 63:
            assert len(set(hi.tolist())) <= N // 4             # many candidates share a key
            assert (np.diff(order) < 0).sum() >= 4             # ... and the order is not the identity


@pytest.mark.parametrize("N", [n for n in MC.SET_SIZES if n >= 63])
def test_planted_cases_decide_inside_a_round(N):
    case = next(c for c in MC.SET_CASES if c.id == "planted-%d" % N)
    acc, rejects, _ = _diagnostics(case)
    assert 4 <= int(acc.sum()) <= N - 4
    assert sum(rejects) >= 1


def test_case_list_decides_across_rounds_and_past_rejected_mates():
    later, past = 0, 0
    for case in MC.SET_CASES:
        if case.gen in ("planted", "late_live", "nlive_exact"):
            _, rejects, joins = _diagnostics(case)
            later += sum(rejects[1:])
            past += joins
    assert later >= 1
    assert past >= 1


def test_ref_assemble_is_the_oracle_matrix_rule():
    """EC.oracle_matrix builds the matrix from per-cell verdicts the way the oracle-checked tests do: solved cells
    from their max chi2, free cells as the AND of the diagonals."""
    from ipc_amd.consensus import Config
    case = MC.assemble_case(65)
    g, cfg = MC.graph_for(intervals=case.ids), Config()
    cells = MC.expected_cells(case.ids)
    assert cells == EC.expected_cells(g.loop_ids)
    ci = np.array([c[0] for c in cells])
    cj = np.array([c[1] for c in cells])
    mx = np.where(case.U[ci, cj], 0.0, 1e9)                    # a verdict per solved cell: far below / far above
    assert np.array_equal(EC.oracle_matrix(g, cfg, ci, cj, mx).astype(bool), case.C)
    assert np.array_equal(case.C, case.C.T)


@pytest.mark.parametrize("N", [n for n in MC.ASSEMBLE_SIZES if n >= 64])
def test_interval_sets_hold_every_kind_and_both_select_paths(N):
    ids = MC.assemble_case(N).ids
    assert MC.interval_kinds(ids) == MC.ALL_KINDS
    fast, slow = MC.select_paths(ids)
    assert fast >= 1 and slow >= 1


@pytest.mark.parametrize("N", [n for n in MC.PLAN_SIZES if n >= 64])
def test_plan_graph_intervals_hold_every_kind(N):
    g = MC.plan_graph(N)
    assert g.V == MC.PLAN_V
    assert MC.interval_kinds(g.loop_ids) == MC.ALL_KINDS
    lo, hi = g.loop_ids.min(1), g.loop_ids.max(1)
    assert (hi - lo).max() <= MC.PLAN_MAX_LEN


def test_plan_graph_diagonal_verdicts_by_the_oracle(oracle):
    """The loops measure what the odometry measures (max chi2 = 0), the shifted ones 30 m more: the oracle's diagonal
    is the design, far from the threshold on both sides."""
    from ipc_amd.consensus import Config
    N = 63
    g, cfg = MC.plan_graph(N), Config()
    poses = oracle.propagate(2, g.odom_meas)
    shifted = set(MC.plan_shifted(N))
    for k in range(N):
        solved, mx, _ = oracle.pair_cell(2, g.odom_meas, g.odom_info, cfg.s_factor, poses, g.loop_ids, g.loop_meas,
                                         g.loop_info, k, k, cfg.fast_reject_iter_base, cfg.slow_reject_iter_base)
        assert solved
        if k in shifted:
            assert mx > 10 * cfg.fast_reject_th, (k, mx)
        else:
            assert mx < 1e-6, (k, mx)


def test_gathered_rows_keep_the_read_bits_and_poison_the_rest():
    case = MC.assemble_case(65)
    N, words = 65, 2
    slot = np.arange(N)[::-1].copy()
    a, b = MC.gathered_rows(case.U, slot, N + 3, 1), MC.gathered_rows(case.U, slot, N + 3, 2)
    from ipc_amd.consensus import unpack_bits
    ua, ub = unpack_bits(a, words * 64).astype(bool), unpack_bits(b, words * 64).astype(bool)
    upper = np.triu(np.ones((N, N), dtype=bool))
    for u in (ua, ub):
        assert np.array_equal(u[slot][:, :N][upper], case.U[upper])
    unread = np.ones_like(ua)
    unread[slot[:, None], np.arange(N)[None, :]] = ~upper
    assert (ua[unread] != ub[unread]).mean() > 0.3
    assert (ua[unread]).mean() > 0.3 and (~ua[unread]).mean() > 0.3
