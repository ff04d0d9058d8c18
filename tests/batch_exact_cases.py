"""Batches of matrices for the sets of a batch (ipc_set_max_batch_exact, ipc_run_batch_exact).

Plain module (no GPU use, no fixtures).  A run is a matrix of tests/exact_cases.py under its processing order MC.set_order(N) --
or one of the two extra matrices below -- and every reference is that module's (or the same functions on the extra matrices):
the multi-start set and LB, UB0, the clique number.  tests/test_batch_exact_cpu.py holds the conditions that make the batches
worth running, by the references alone; tests/test_gpu_batch_exact.py runs the kernels on them.

The layout of a batch is the one ipc_run_batch documents for its outputs: matrices back to back, run r [N_r][ceil(N_r/64)] words;
orders and byte outputs back to back, run r at sum of N_q, q < r."""
import functools

import numpy as np

import exact_cases as EX
import matrix_cases as MC
import multistart_cases as MS

ZEROS = "zeros-70"                                # an all-zero matrix: no live candidate, n = 0
EXTRA = {ZEROS: 70}


def _small():
    """Batch A: every case with N <= 129 -- the word edges 1, 63, 64, 65, 128, 129 -- in one call.  The list order of
    tests/exact_cases.py, but for two runs moved to the end so that a run without a live candidate (dead-129) sits between two
    searched ones (decoys-129-40 and planted-64); planted-128 and planted-129 are searched neighbours as they stand."""
    ids = [c.id for c in EX.CASES if c.N <= 129]
    moved = ["dead-129", "planted-64"]
    return [i for i in ids if i not in moved] + moved


# Batch B mixes widths: 66 words (two per lane, so the whole chunk runs the R = 2 kernels), 17 words, 2 words, 1 word.
# No two neighbours have the same LB, in this order or reversed: a prune against the neighbour's LB explores another tree.
BATCH_B = ["decoys-4161-70", "hidden_c-1025", ZEROS, "decoys-1025-300", "nlive_exact-1025-128", "all_ones-1", "all_ones-1025",
           "hidden-1025"]
BATCHES = {"A": _small(), "B": BATCH_B}
CAP_BATCH = ["planted-1025", "decoys-129-40", "hidden-1025"]     # the cap test: two runs that hit the cap and one closed by LB = UB0
CAP = 64


def size(run_id):
    return EXTRA[run_id] if run_id in EXTRA else EX.BY_ID[run_id].N


@functools.lru_cache(maxsize=None)
def matrix(run_id):
    if run_id not in EXTRA:
        return EX.matrix(run_id)
    ok = np.zeros((EXTRA[run_id],) * 2, dtype=bool)
    ok.setflags(write=False)
    return ok


@functools.lru_cache(maxsize=None)
def multistart(run_id):
    """The multi-start reference (its set, the live list); shared, not to be modified."""
    if run_id not in EXTRA:
        return EX.multistart(run_id)
    r = MS.ref_multistart_bitset(matrix(run_id), MC.set_order(size(run_id)))
    r.accepted.setflags(write=False), r.sizes.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def colour_bound(run_id):
    return EX.colour_bound(run_id) if run_id not in EXTRA else EX.ref_colour_bound(matrix(run_id), MC.set_order(size(run_id)))


@functools.lru_cache(maxsize=None)
def omega(run_id):
    if run_id not in EXTRA:
        return EX.reference(run_id).omega
    r = EX.ref_exact(matrix(run_id), MC.set_order(size(run_id)))
    assert r.finished
    return r.omega


def searched(run_id):
    """The bracket is open behind the multi-start and UB0: the search has to run."""
    return int(multistart(run_id).accepted.sum()) < colour_bound(run_id)


def offsets(sizes):
    """(vector offsets [R + 1], matrix offsets in words [R + 1]) of runs with these candidate counts."""
    sizes = [int(n) for n in sizes]
    vec = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    mat = np.concatenate([[0], np.cumsum([n * ((n + 63) // 64) for n in sizes])]).astype(np.int64)
    return vec, mat


def packed(run_ids):
    """(run_n int32 [R], orders back to back int32, matrices back to back uint64) of a batch."""
    run_n = np.array([size(i) for i in run_ids], dtype=np.int32)
    order = np.concatenate([MC.set_order(int(n)) for n in run_n]).astype(np.int32)
    words = np.concatenate([MC.pack_rows(matrix(i)).reshape(-1) for i in run_ids]).astype(np.uint64)
    return run_n, order, words
