"""The references of tests/exact_cases.py against networkx and against the definition, the conditions that make its inputs
adversarial -- by the references alone -- and the shape of the new C ABI.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import exact_cases as EX
import matrix_cases as MC
import multistart_cases as MS

SMALL = [c.id for c in EX.CASES if len(EX.multistart(c.id).live) <= 129]
ENUM_LIMIT = 20000
BEATS_MULTISTART =("nlive_exact-1025-128", "hidden_c-1025", "decoys-129-40", "decoys-1025-300", "decoys-4161-70")


def test_the_case_list_is_the_one_the_issue_names():
    ids = set(EX.CASE_IDS)
    assert len(ids) == len(EX.CASE_IDS)
    assert {c.id for c in MS.CASES if c.N <= 129} <= ids
    for N in (63, 64, 65, 128, 129):
        assert "planted-%d" % N in ids
    for must in ("nlive_exact-1025-1", "nlive_exact-1025-63", "nlive_exact-1025-64", "nlive_exact-1025-65", "nlive_exact-1025-128",
                 "nlive_exact-4161-64", "nlive_exact-4161-65", "all_ones-1025", "identity-1025", "dead-1025", "chain_conflict-1025",
                 "far_conflict-1025", "two_cliques-1025-300", "decoys-129-40", "decoys-1025-300", "decoys-4161-70", "hidden-1025",
                 "hidden-4161", "hidden_c-1025"):
        assert must in ids
    for cap_only in EX.CAP_ONLY:
        assert cap_only not in ids and cap_only in EX.BY_ID
    assert (4161 + 63) // 64 == 66 and len(EX.multistart("hidden-4161").live) == 4161      # two words per lane
    assert len(EX.multistart("decoys-4161-70").live) == 4161


@pytest.mark.parametrize("case_id", SMALL)
def test_reference_agrees_with_networkx(case_id):
    nx = pytest.importorskip("networkx")
    ok, order = EX.matrix(case_id), MC.set_order(EX.BY_ID[case_id].N)
    live = [int(k) for k in order if ok[k][k]]
    g = nx.Graph()
    g.add_nodes_from(live)
    g.add_edges_from((a, b) for i, a in enumerate(live) for b in live[i + 1:] if ok[a][b])
    omega = EX.reference(case_id).omega
    # networkx's own exact search, and its enumeration of the maximal cliques.  chain_conflict and far_conflict have some
    # 1.3^n and 2^64 maximal cliques at n >= 63 / 128 and the random graphs of 128 more than ENUM_LIMIT: there the
    # enumeration is cut and can only show that none of those is larger; wherever it ends by itself its maximum must be omega.
    assert nx.max_weight_clique(g, weight=None)[1] == omega
    seen = [len(c) for c in itertools.islice(nx.find_cliques(g), ENUM_LIMIT + 1)]
    if len(seen) <= ENUM_LIMIT:
        assert max(seen, default=0) == omega
    else:
        assert max(seen) <= omega


@pytest.mark.parametrize("case_id", SMALL)
def test_colour_bound_on_bit_sets_equals_the_plain_one(case_id):
    ok, order = EX.matrix(case_id), MC.set_order(EX.BY_ID[case_id].N)
    assert EX.colour_bound(case_id) == EX.ref_colour_bound_plain(ok, order)


@pytest.mark.parametrize("case_id", EX.CASE_IDS)
def test_reference_clique_and_the_bracket(case_id):
    N = EX.BY_ID[case_id].N
    ok, r, ms = EX.matrix(case_id), EX.reference(case_id), EX.multistart(case_id)
    acc = np.zeros(N, dtype=np.uint8)
    acc[r.clique] = 1
    assert len(set(r.clique)) == len(r.clique) == r.omega == int(acc.sum())
    assert EX.is_clique_of_live(ok, acc)
    lb = int(ms.accepted.sum())
    assert lb <= r.omega <= EX.colour_bound(case_id)
    assert (r.omega == 0) == (len(ms.live) == 0)


def test_a_capped_reference_says_so():
    r = EX.ref_exact(EX.matrix("nlive_exact-1025-128"), MC.set_order(1025), cap=100)
    assert not r.finished and r.steps > 100 and r.omega <= EX.reference("nlive_exact-1025-128").omega


@pytest.mark.parametrize("case_id", BEATS_MULTISTART)
def test_the_optimum_beats_the_multistart(case_id):
    assert EX.reference(case_id).omega > int(EX.multistart(case_id).accepted.sum())


def test_the_figures_of_the_adversarial_cases():
    assert (EX.reference("nlive_exact-1025-128").omega, int(EX.multistart("nlive_exact-1025-128").accepted.sum())) == (51, 48)
    assert (EX.reference("hidden_c-1025").omega, int(EX.multistart("hidden_c-1025").accepted.sum())) == (140, 139)
    assert len(EX.multistart("hidden_c-1025").live) == 931
    for N, m in EX.DECOYS:
        cid = "decoys-%d-%d" % (N, m)
        ms = EX.multistart(cid)
        assert len(ms.live) == N and int(ms.accepted.sum()) == 2 and EX.reference(cid).omega == m
        assert sorted(EX.reference(cid).clique) == sorted(MC.set_order(N)[N - m:].tolist())
        assert EX.colour_bound(cid) == m + 1


@pytest.mark.parametrize("case_id", ["hidden-1025", "two_cliques-1025-300", "hidden-4161", "all_ones-1025"])
def test_the_multistart_is_already_optimal(case_id):
    assert EX.reference(case_id).omega == int(EX.multistart(case_id).accepted.sum()) > 0


def test_struct_and_symbols_of_the_new_abi():
    from ipc_amd import capi
    assert ctypes.sizeof(capi.ExactReport) == 40
    assert [f for f, _ in capi.ExactReport._fields_] == ["live", "multistart_size", "size", "upper_bound", "proven", "subproblems",
                                                         "capped", "steps"]
    assert capi.ExactReport.steps.offset == 32 and capi.ExactReport.steps.size == 8
    assert len(capi.SYMBOLS) == len(set(capi.SYMBOLS)) == 50
    assert "ipc_set_max_exact" in capi.SYMBOLS and "ipc_run_exact" in capi.SYMBOLS
    lib = capi.load()
    assert hasattr(lib, "ipc_set_max_exact") and hasattr(lib, "ipc_run_exact")


def test_null_handle_errors_need_no_gpu():
    from ipc_amd import capi
    lib = capi.load()
    assert lib.ipc_set_max_exact(None, None, None, None, None) == -1
    assert b"ipc_set_max_exact: NULL" in lib.ipc_last_error()
    assert lib.ipc_run_exact(None, None, None, None, None) == -1
    assert b"ipc_run_exact: NULL" in lib.ipc_last_error()
