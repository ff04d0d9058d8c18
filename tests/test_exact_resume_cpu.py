"""The reference of tests/exact_resume_cases.py against EX.reference on every (case, split), chains of resumed calls, the
conditions that make the pairs cover every outcome -- by the references alone -- and the shape of the new C ABI.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import exact_cases as EX
import exact_resume_cases as ER
import matrix_cases as MC
import multistart_cases as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_split_list_is_the_one_the_issue_names():
    assert len(set(ER.SPLITS)) == len(ER.SPLITS)
    small = [c for c in EX.CASES if c.N <= 129]
    for c in small:
        want = {min(max(f, 0), c.N) for f in (0, 1, 63, 64, 65, c.N // 2, c.N - 1, c.N)}
        assert {f for cid, f in ER.SPLITS if cid == c.id} == want
    for cid in ER.LARGE:
        N = EX.BY_ID[cid].N
        assert [f for c, f in ER.SPLITS if c == cid] == [N // 2, N - 64, N - 1]
    assert {cid for cid, _ in ER.SPLITS} == {c.id for c in small} | set(ER.LARGE)
    assert "decoys-129-40" in ER.CHAIN_CASES and all(EX.BY_ID[c].N == 129 for c in ER.CHAIN_CASES)


# ---- 1. every (case, split) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id,first", ER.SPLITS, ids=ER.SPLIT_IDS)
def test_reference_reaches_omega_from_every_split(case_id, first):
    ok, held, r = EX.matrix(case_id), ER.held_set(case_id, first), ER.reference(case_id, first)
    omega = EX.reference(case_id).omega
    assert held[first:].sum() == 0 and EX.is_clique_of_live(ok, held)
    assert r.size == omega == int(r.accepted.sum()) and r.proven == 1
    assert EX.is_clique_of_live(ok, r.accepted)
    assert r.w0 == int(held.sum()) <= omega and r.lb <= omega <= r.upper_bound
    if omega == r.w0:
        assert r.accepted.tobytes() == held.tobytes() and r.changed == 0
    else:
        assert r.changed == 1


# ---- 2. chains ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("burst", ER.CHAIN_BURSTS)
@pytest.mark.parametrize("case_id", ER.CHAIN_CASES)
def test_chains_of_resumed_calls_end_at_omega(case_id, burst):
    N = EX.BY_ID[case_id].N
    ok, order = EX.matrix(case_id), MC.set_order(N)
    held, first, size = np.zeros(N, dtype=np.uint8), 0, 0
    for length in ER.chain_firsts(N, burst):
        r = ER.ref_exact_resume(ER.prefix(ok, length), order, first, held)
        assert r.w0 == size and r.size >= size and (r.changed == 0 or r.size > size)      # it changes only to grow
        assert EX.is_clique_of_live(ER.prefix(ok, length), r.accepted)
        held, first, size = r.accepted, length, r.size
    assert size == EX.reference(case_id).omega


# ---- 3. conditions on the inputs ------------------------------------------------------------------------------------------
def test_every_outcome_occurs_among_the_pairs():
    search_wins = multistart_wins = unchanged = no_newcomer = first_zero = 0
    for cid, first in ER.SPLITS:
        r = ER.reference(cid, first)
        b0 = max(r.w0, r.lb)
        search_wins += r.size > b0
        multistart_wins += r.size == r.lb > r.w0
        unchanged += r.changed == 0 and r.newcomers > 0
        no_newcomer += r.newcomers == 0
        first_zero += first == 0
    assert min(search_wins, multistart_wins, unchanged, no_newcomer, first_zero) >= 1, \
        (search_wins, multistart_wins, unchanged, no_newcomer, first_zero)


@pytest.mark.parametrize("case_id,first,w0,lb,omega", [("nlive_exact-1025-128", 961, 50, 48, 51), ("hidden_c-1025", 961, 135, 139, 140),
                                                       ("decoys-1025-300", 1024, 299, 2, 300), ("decoys-4161-70", 2080, 34, 2, 70)])
def test_the_figures_of_the_large_pairs(case_id, first, w0, lb, omega):
    assert (case_id, first) in ER.SPLITS
    r = ER.reference(case_id, first)
    assert (r.w0, r.lb, r.size, EX.reference(case_id).omega) == (w0, lb, omega, omega)
    assert r.size > max(r.w0, r.lb) and r.searched and r.roots > 0          # the search wins, not the multi-start


def test_two_cliques_is_closed_by_the_multistart_and_one_newcomer_changes_nothing():
    for cid, first in ER.SPLITS:
        r = ER.reference(cid, first)
        if cid == "two_cliques-1025-300":
            assert r.size == r.lb and r.roots == 0
        elif cid in ER.LARGE and first == EX.BY_ID[cid].N - 1 and cid != "decoys-1025-300":
            assert r.newcomers <= 1 and r.changed == 0


# ---- 4. the ABI -------------------------------------------------------------------------------------------------------------
def test_struct_and_symbols_of_the_resume_abi():
    from ipc_amd import capi
    assert ctypes.sizeof(capi.ExactResumeReport) == 56
    assert [f for f, _ in capi.ExactResumeReport._fields_] == ["first", "live", "newcomers", "size_before", "multistart_size", "size",
                                                               "upper_bound", "proven", "changed", "subproblems", "capped", "steps"]
    assert capi.ExactResumeReport.steps.offset == 48 and capi.ExactResumeReport.steps.size == 8
    lib = capi.load()
    # the three entry points are declared in a header of their own, which ipc_amd.h includes; the list against that header
    src = open(os.path.join(ROOT, "include", "ipc_amd_online_exact.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(ipc_[a-z_0-9]+)\s*\(", src))) == sorted(capi.SYMBOLS_ONLINE_EXACT)
    assert sorted(capi.SYMBOLS_ONLINE_EXACT) == ["ipc_online_exact_state", "ipc_run_online_exact", "ipc_set_max_exact_resume"]
    assert not set(capi.SYMBOLS_ONLINE_EXACT) & set(capi.SYMBOLS)
    assert '#include "ipc_amd_online_exact.h"' in open(os.path.join(ROOT, "include", "ipc_amd.h")).read()
    for name in capi.SYMBOLS_ONLINE_EXACT:
        assert hasattr(lib, name)


def test_null_handle_errors_need_no_gpu():
    from ipc_amd import capi
    lib = capi.load()
    assert lib.ipc_set_max_exact_resume(None, None, 0, None, None, None) == -1
    assert b"ipc_set_max_exact_resume: NULL" in lib.ipc_last_error()
    assert lib.ipc_run_online_exact(None, None, None, None, None, None) == -1
    assert b"ipc_run_online_exact: NULL" in lib.ipc_last_error()
    assert lib.ipc_online_exact_state(None, None, None) == -1
    assert b"ipc_online_exact_state: NULL" in lib.ipc_last_error()
