"""The batches of tests/batch_exact_cases.py are worth running -- by the references alone -- and the shape of the new C ABI
(include/ipc_amd_batch_exact.h).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import batch_exact_cases as BX
import exact_cases as EX
import matrix_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the batches --------------------------------------------------------------------------------------------------------
def test_batch_a_is_every_small_case_once():
    small = [c.id for c in EX.CASES if c.N <= 129]
    assert sorted(BX.BATCHES["A"]) == sorted(small) and len(set(small)) == len(small)
    assert {BX.size(i) for i in BX.BATCHES["A"]} == {1, 2, 63, 64, 65, 128, 129}


def test_batch_b_mixes_the_widths_the_issue_names():
    B = BX.BATCHES["B"]
    for i in ("decoys-4161-70", "decoys-1025-300", "hidden_c-1025", "nlive_exact-1025-128", BX.ZEROS, "all_ones-1"):
        assert i in B
    assert any(i.startswith("all_ones-") and BX.size(i) > 1 for i in B) and any(i.startswith("hidden-") for i in B)
    assert max(BX.size(i) for i in B) == 4161                     # two words of a row per lane: the chunk runs the R = 2 kernels
    assert {(BX.size(i) + 63) // 64 for i in B} >= {66, 17, 2, 1}
    assert not BX.matrix(BX.ZEROS).any() and len(BX.multistart(BX.ZEROS).live) == 0
    assert BX.size("all_ones-1") == 1 and BX.matrix("all_ones-1").all()
    for i in B:
        if i.startswith(("all_ones-", "hidden-")):
            assert not BX.searched(i) and int(BX.multistart(i).accepted.sum()) == BX.colour_bound(i) == BX.omega(i)
    assert not set(B) & set(EX.CAP_ONLY) and not set(BX.BATCHES["A"]) & set(EX.CAP_ONLY)
    assert EX.CAP_ONLY[0] in BX.CAP_BATCH and not BX.searched(BX.CAP_BATCH[-1])


@pytest.mark.parametrize("name", sorted(BX.BATCHES))
def test_searched_and_closed_runs_are_neighbours(name):
    ids = BX.BATCHES[name]
    s = [BX.searched(i) for i in ids]
    live = [len(BX.multistart(i).live) for i in ids]
    print(name, [(i, "searched" if f else "closed") for i, f in zip(ids, s)])
    assert any(s) and not all(s)
    assert any(a != b for a, b in zip(s, s[1:]))                   # a searched run beside a closed one
    assert any(a and b for a, b in zip(s, s[1:]))                  # two searched runs side by side
    assert any(s[k - 1] and live[k] == 0 and s[k + 1] for k in range(1, len(ids) - 1))     # n = 0 between two searched runs
    for i, f in zip(ids, s):
        lb = int(BX.multistart(i).accepted.sum())
        assert lb <= BX.omega(i) <= BX.colour_bound(i)
        if f:
            assert len(BX.multistart(i).live) >= 2


def test_the_search_wins_in_some_run_and_the_multistart_in_another():
    for name, ids in BX.BATCHES.items():
        open_runs = [i for i in ids if BX.searched(i)]
        assert any(BX.omega(i) > int(BX.multistart(i).accepted.sum()) for i in open_runs), name
    # neighbours of different LB: a search that pruned against its neighbour's LB would explore another tree
    for ids in (BX.BATCHES["B"], BX.BATCHES["B"][::-1]):
        lbs = [int(BX.multistart(i).accepted.sum()) for i in ids]
        assert all(a != b for a, b, i, j in zip(lbs, lbs[1:], ids, ids[1:]) if BX.searched(i) or BX.searched(j))


# ---- 2. offsets ------------------------------------------------------------------------------------------------------------
def test_offsets_and_packing():
    vec, mat = BX.offsets([1, 63, 64, 65, 129])
    assert vec.tolist() == [0, 1, 64, 128, 193, 322]
    assert mat.tolist() == [0, 1, 64, 128, 128 + 130, 128 + 130 + 387]
    ids = ["all_ones-65", "dead-2", "planted-129"]
    run_n, order, words = BX.packed(ids)
    vec, mat = BX.offsets(run_n)
    assert run_n.tolist() == [65, 2, 129] and order.dtype == np.int32 and words.dtype == np.uint64
    assert len(order) == vec[-1] and len(words) == mat[-1]
    for r, i in enumerate(ids):
        n = int(run_n[r])
        assert np.array_equal(order[vec[r]:vec[r + 1]], MC.set_order(n))
        assert np.array_equal(words[mat[r]:mat[r + 1]].reshape(n, -1), MC.pack_rows(BX.matrix(i)))


# ---- 3. the ABI ------------------------------------------------------------------------------------------------------------
def test_struct_and_symbols_of_the_batch_exact_abi():
    from ipc_amd import capi
    assert ctypes.sizeof(capi.BatchExactReport) == 24
    assert [f for f, _ in capi.BatchExactReport._fields_] == ["runs", "chunks", "searched_runs", "proven_runs", "set_launches",
                                                              "set_host_waits"]
    assert ctypes.sizeof(capi.ExactReport) == 40                  # reports [n_runs]: the stride of the array
    lib = capi.load()
    src = open(os.path.join(ROOT, "include", "ipc_amd_batch_exact.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(ipc_[a-z_0-9]+)\s*\(", src))) == sorted(capi.SYMBOLS_BATCH_EXACT)
    assert sorted(capi.SYMBOLS_BATCH_EXACT) == ["ipc_run_batch_exact", "ipc_set_max_batch_exact"]
    assert not set(capi.SYMBOLS_BATCH_EXACT) & (set(capi.SYMBOLS) | set(capi.SYMBOLS_ONLINE_EXACT) | set(capi.SYMBOLS_LAZY_SD))
    assert len(capi.SYMBOLS) == 50
    assert '#include "ipc_amd_batch_exact.h"' in open(os.path.join(ROOT, "include", "ipc_amd.h")).read()
    for name in capi.SYMBOLS_BATCH_EXACT:
        assert hasattr(lib, name)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert entry.count('"ipc_amd_batch_exact.h"') == 2            # a change of the header rebuilds the library
    assert os.path.exists(os.path.join(ROOT, "ipc_amd", "csrc", "batch_exact_kernels.hpp"))


def test_null_arguments_need_no_gpu():
    from ipc_amd import capi
    lib = capi.load()
    assert lib.ipc_set_max_batch_exact(None, 1, None, None, None, None, None, None, None, None, None) == -1
    assert b"ipc_set_max_batch_exact: NULL" in lib.ipc_last_error()
    assert lib.ipc_run_batch_exact(None, 1, None, None, None, None, None, None, None, None, None) == -1
    assert b"ipc_run_batch_exact: NULL" in lib.ipc_last_error()
    assert lib.ipc_run_batch(None, 1, None, None, None, None, None) == -1
    assert b"ipc_run_batch: NULL" in lib.ipc_last_error()
