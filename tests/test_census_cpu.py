"""The references of tests/census_cases.py against the table of the issue, against each other and against the invariants of
the definition -- the adversarial properties of the cases are shown by the references alone -- and the shape of the new C ABI
(include/ipc_amd_census.h).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import census_cases as CS
import exact_cases as EX
import matrix_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the complement of a chain of 63 and more has beyond NX_LIMIT maximal cliques (some 1.3^n): networkx's enumeration is cut there
NX_IDS = [i for i in CS.SMALL_IDS if not (i.startswith("chain_conflict") and EX.BY_ID[i].N >= 63)]


# ---- 1. the case list and the table ----------------------------------------------------------------------------------------
def test_the_case_list_is_the_one_the_issue_names():
    ids = set(CS.CASE_IDS)
    assert len(ids) == len(CS.CASE_IDS) and set(CS.TABLE) <= ids
    small = {c.id for c in EX.CASES if c.N <= 129}
    assert small - ids == {"far_conflict-128", "far_conflict-129"} and ids <= set(EX.CASE_IDS)
    assert CS.CAP_CASE in EX.BY_ID and CS.CAP_CASE not in ids
    assert len(NX_IDS) >= len(CS.SMALL_IDS) - 5
    for i in ("nlive_exact-4161-64", "nlive_exact-4161-65", "hidden-4161", "decoys-4161-70"):       # two words of a row per lane
        assert (EX.BY_ID[i].N + 63) // 64 > 64 and i in ids


@pytest.mark.parametrize("case_id", sorted(CS.TABLE))
def test_the_reference_reproduces_the_table(case_id):
    omega, count, core, support, sub = CS.reference(case_id)
    print(case_id, omega, count, int(core.sum()), int(support.sum()), "subproblems", sub)
    assert (omega, count, int(core.sum()), int(support.sum())) == CS.TABLE[case_id]


def test_what_the_table_makes_of_the_cases():
    """More than one maximum set in one subproblem, ties that share nothing, an optimum that fills its root's candidate set,
    omega = 1 roots and n = 0."""
    for i in ("nlive_exact-1025-64", "nlive_exact-1025-128", "nlive_exact-4161-65"):
        omega, count, _, _, sub = CS.reference(i)
        assert count > sub >= 1                                       # some subproblem holds several members of MAX
    for i in ("two_cliques-129-64", "chain_conflict-64"):
        assert CS.reference(i)[1] > 1 and not CS.reference(i)[2].any()
    for i in ("all_ones-129", "decoys-129-40", "decoys-4161-70"):
        omega, count, core, support, sub = CS.reference(i)
        assert count == 1 and sub == 1 and int(core.sum()) == omega   # the one root not pruned: 1 + |candidates| == omega
    omega, count, core, support, sub = CS.reference("identity-129")
    assert (omega, count, sub) == (1, 129, 129) and support.all() and not core.any()
    assert CS.reference("dead-129")[1] == 1 and CS.reference("dead-129")[4] == 0


# ---- 2. the two references -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", NX_IDS)
def test_the_two_references_agree(case_id):
    pytest.importorskip("networkx")
    omega, count, core, support, _ = CS.reference(case_id)
    got = CS.nx_census(EX.matrix(case_id), MC.set_order(EX.BY_ID[case_id].N), omega, CS.NX_LIMIT)
    assert got is not None, "networkx's enumeration was cut"
    assert got[0] == count and np.array_equal(got[1], core) and np.array_equal(got[2], support)


# ---- 3. the invariants -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", CS.CASE_IDS)
def test_invariants_of_the_reference(case_id):
    N = EX.BY_ID[case_id].N
    omega, count, core, support, sub = CS.reference(case_id)
    acc = np.zeros(N, dtype=np.uint8)
    acc[EX.reference(case_id).clique] = 1                         # one maximum set, from another search
    CS.check_invariants(EX.matrix(case_id), acc, core, support, count, omega)
    n = len(EX.multistart(case_id).live)
    assert 0 <= sub <= n and (sub >= 1) == (n > 0)
    # every member of the support lies in a clique of omega: it has omega - 1 neighbours inside the support
    ok = EX.matrix(case_id)
    mem = np.flatnonzero(support)
    if len(mem):
        assert (ok[np.ix_(mem, mem)].sum(axis=1) >= omega).all()
    cm = np.flatnonzero(core)
    assert ok[np.ix_(cm, mem)].all()                              # a core member agrees with the whole support


def test_the_cap_case_is_closed_by_the_bracket_alone():
    """far_conflict-128: LB = UB0 = 64, so the exact stage proves omega without a search, whatever the step cap; and its 2^64
    maximum sets are 64 free choices out of 64 conflicting pairs."""
    lb = int(EX.multistart(CS.CAP_CASE).accepted.sum())
    assert lb == EX.colour_bound(CS.CAP_CASE) == 64 and len(EX.multistart(CS.CAP_CASE).live) == 128
    ok = EX.matrix(CS.CAP_CASE)
    conflicts = np.argwhere(~ok & ~np.eye(128, dtype=bool))
    assert len(conflicts) == 128 and len(set(conflicts.ravel().tolist())) == 128      # 64 disjoint pairs, both directions
    # decoys-129-40 under 64 steps: LB = 2 < UB0 = 41, the exact stage has to search
    assert int(EX.multistart(CS.EXACT_CAPPED_CASE).accepted.sum()) == 2 and EX.colour_bound(CS.EXACT_CAPPED_CASE) == 41


# ---- 4. the ABI ------------------------------------------------------------------------------------------------------------
def test_struct_and_symbols_of_the_census_abi():
    from ipc_amd import capi
    assert ctypes.sizeof(capi.CensusReport) == 48
    assert [f for f, _ in capi.CensusReport._fields_] == ["live", "size", "exact_proven", "proven", "count", "core_size", "support_size",
                                                          "subproblems", "capped", "steps"]
    assert capi.CensusReport.count.offset == 16 and capi.CensusReport.count.size == 8
    assert capi.CensusReport.steps.offset == 40 and capi.CensusReport.steps.size == 8
    src = open(os.path.join(ROOT, "include", "ipc_amd_census.h")).read()
    assert "#ifndef IPC_AMD_H" in src and "#error" in src and "Not a header to include by itself" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(ipc_[a-z_0-9]+)\s*\(", src))) == sorted(capi.SYMBOLS_CENSUS)
    assert sorted(capi.SYMBOLS_CENSUS) == ["ipc_run_census", "ipc_set_max_census"]
    others = set(capi.SYMBOLS) | set(capi.SYMBOLS_ONLINE_EXACT) | set(capi.SYMBOLS_LAZY_SD) | set(capi.SYMBOLS_BATCH_EXACT)
    assert not set(capi.SYMBOLS_CENSUS) & others
    assert len(capi.SYMBOLS) == len(set(capi.SYMBOLS)) == 50
    assert '#include "ipc_amd_census.h"' in open(os.path.join(ROOT, "include", "ipc_amd.h")).read()
    lib = capi.load()
    for name in capi.SYMBOLS_CENSUS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry.count('"ipc_amd_census.h"') == 2                 # a change of the header rebuilds the library
    assert os.path.exists(os.path.join(ROOT, "ipc_amd", "csrc", "census_kernels.hpp"))


def test_null_arguments_need_no_gpu():
    from ipc_amd import capi
    lib = capi.load()
    assert lib.ipc_set_max_census(None, None, None, None, None, None, None, None) == -1
    assert b"ipc_set_max_census: NULL" in lib.ipc_last_error()
    assert lib.ipc_run_census(None, None, None, None, None, None, None) == -1
    assert b"ipc_run_census: NULL" in lib.ipc_last_error()
