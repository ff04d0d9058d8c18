"""The references of tests/multistart_cases.py against each other and against the definition, and the conditions that make
its inputs adversarial -- by the references alone, no GPU."""
import numpy as np
import pytest

import matrix_cases as MC
import multistart_cases as MS

SMALL = [c.id for c in MS.CASES if c.N <= 129]


def _positions(case_id):
    """position in L of every candidate (-1: dead)"""
    N = MS.BY_ID[case_id].N
    pos = np.full(N, -1)
    for q, k in enumerate(MS.reference(case_id).live):
        pos[k] = q
    return pos


def test_the_case_list_is_the_one_the_issue_names():
    ids = set(MS.CASE_IDS)
    assert len(ids) == len(MS.CASE_IDS) == 6 * 8 + 5 + 7 + 3 + 3
    for must in ("planted-4097", "planted-4161", "late_live-2049", "late_live-4161", "far_conflict-4161", "nlive_exact-1025-128",
                 "nlive_exact-4161-64", "planted_all_live-4161", "two_cliques-131-65", "all_ones-1025", "dead-1"):
        assert must in ids
    assert "all_ones-4161" not in ids


@pytest.mark.parametrize("case_id", SMALL)
def test_plain_reference_equals_bitset_reference(case_id):
    ok, order = MS.matrix(case_id), MC.set_order(MS.BY_ID[case_id].N)
    plain, fast = MS.ref_multistart_plain(ok, order), MS.reference(case_id)
    assert np.array_equal(plain.accepted, fast.accepted)
    assert np.array_equal(plain.sizes, fast.sizes)
    assert plain.best_q == fast.best_q and plain.live == fast.live


@pytest.mark.parametrize("case_id", MS.CASE_IDS)
def test_result_is_a_maximal_clique_no_smaller_than_the_greedy(case_id):
    N = MS.BY_ID[case_id].N
    ok, order, r = MS.matrix(case_id), MC.set_order(N), MS.reference(case_id)
    greedy = MC.ref_set_max(ok, order)
    mem = np.flatnonzero(r.accepted)
    n = len(r.live)
    assert (r.sizes > 0).sum() == n and all(r.sizes[k] > 0 for k in r.live)
    if n == 0:
        assert mem.size == 0 and r.best_q == -1 and greedy.sum() == 0
        return
    # S_0 is the greedy set
    assert r.sizes[r.live[0]] == greedy.sum()
    if r.best_q == 0:
        assert np.array_equal(r.accepted, greedy)
    assert mem.size == r.sizes.max() == r.sizes[r.live[r.best_q]] >= greedy.sum()
    assert r.best_q == min(q for q, k in enumerate(r.live) if r.sizes[k] == r.sizes.max())
    assert r.accepted[r.live[r.best_q]] == 1
    assert ok[np.ix_(mem, mem)].all()                                  # pairwise consistent, all live
    covers = ok[:, mem].all(axis=1) & np.diag(ok)                      # live candidates that agree with every member
    assert set(np.flatnonzero(covers)) == set(mem)                     # ... are the members: maximal


def test_s0_is_the_greedy_set_member_for_member():
    for case_id in ("planted-129", "planted_all_live-129", "nlive_exact-1025-128", "two_cliques-129-64"):
        N = MS.BY_ID[case_id].N
        ok, order = MS.matrix(case_id), MC.set_order(N)
        live = [int(k) for k in order if ok[k][k]]
        members = [live[0]]
        for k in live[1:]:
            if all(ok[k][m] for m in members):
                members.append(k)
        assert sorted(members) == np.flatnonzero(MC.ref_set_max(ok, order)).tolist()
        assert MS.reference(case_id).sizes[live[0]] == len(members)


def test_planted_all_live_4161_collapses_under_the_greedy():
    r = MS.reference("planted_all_live-4161")
    ok, order = MS.matrix("planted_all_live-4161"), MC.set_order(4161)
    assert len(r.live) == 4161
    assert int(MC.ref_set_max(ok, order).sum()) == 4
    assert int(r.accepted.sum()) == 432 and r.best_q == 3267
    assert (_positions("planted_all_live-4161")[np.flatnonzero(r.accepted)] >= 4096).any()
    assert (4161 + 63) // 64 == 66                                     # compact words: past the 64-word lane loop


def test_nlive_exact_1025_128_nine_against_forty_eight():
    r = MS.reference("nlive_exact-1025-128")
    assert len(r.live) == 128
    assert int(MC.ref_set_max(MS.matrix("nlive_exact-1025-128"), MC.set_order(1025)).sum()) == 9
    assert int(r.accepted.sum()) == 48 and r.best_q == 20


@pytest.mark.parametrize("case_id", ["planted-1025", "planted-4161"])
def test_planted_cases_have_a_later_winner_and_many_sizes(case_id):
    N = MS.BY_ID[case_id].N
    r = MS.reference(case_id)
    greedy = int(MC.ref_set_max(MS.matrix(case_id), MC.set_order(N)).sum())
    assert int(r.accepted.sum()) > greedy and r.best_q != 0
    assert len(set(r.sizes[r.sizes > 0].tolist())) >= 50


@pytest.mark.parametrize("N,k", [(129, 64), (131, 65), (1025, 300)])
def test_two_cliques_gives_the_first_clique(N, k):
    r = MS.reference("two_cliques-%d-%d" % (N, k))
    order = MC.set_order(N)
    assert len(r.live) == N
    assert sorted(np.flatnonzero(r.accepted).tolist()) == sorted(order[1:k + 1].tolist())
    assert r.best_q == 1
    assert r.sizes[order[0]] == 1 and r.sizes[order[k + 1]] == k       # the tie: the later clique is as large


@pytest.mark.parametrize("N", MS.SMALL_SIZES)
def test_all_ones_wins_at_position_zero(N):
    r = MS.reference("all_ones-%d" % N)
    assert r.best_q == 0 and (r.sizes == N).all() and r.accepted.all()
