"""Inputs and the reference for the resumed exact set (ipc_set_max_exact_resume, ipc_run_online_exact).

Plain module (no GPU use, no fixtures), in the manner of tests/exact_cases.py, whose matrices, orders and references it uses.
tests/test_exact_resume_cpu.py holds the reference against EX.reference; tests/test_gpu_exact_resume.py runs the kernels.

The definition (include/ipc_amd_online_exact.h): A = the set handed in, a maximum clique of the graph on the live candidates < first;
NEW = the positions of L whose candidate is >= first; w0 = |A|; LB = the multi-start size of the whole matrix; b0 = max(w0, LB);
c = the colours of the greedy colouring of NEW alone; UB = min(n, w0 + c).  Root r = the r-th position p of NEW with the
candidate set row(p) minus the newcomers in front of p."""
import functools
import sys
from collections import namedtuple

import numpy as np

import exact_cases as EX
import matrix_cases as MC
import multistart_cases as MS

Resume = namedtuple("Resume", "size accepted proven changed live newcomers w0 lb colours upper_bound searched roots")

LARGE = ("nlive_exact-1025-128", "hidden_c-1025", "decoys-1025-300", "two_cliques-1025-300", "decoys-4161-70")
CHAIN_BURSTS = (1, 7, 64)


def prefix(ok, first):
    """The matrix with the diagonal of the candidates >= first cleared: they are dead, the graph is that of the prefix."""
    out = np.array(ok, dtype=bool, copy=True)
    idx = np.arange(first, out.shape[0])
    out[idx, idx] = False
    return out


def colours_of(rows, mask):
    """The number of colours of the sequential greedy colouring of the positions in `mask`, in position order."""
    uncoloured, k = mask, 0
    while uncoloured:
        k += 1
        sweep = uncoloured
        while sweep:
            low = sweep & -sweep
            sweep &= ~(rows[low.bit_length() - 1] | low)
            uncoloured ^= low
    return k


def _search(rows, root, cand, b0):
    """The largest clique root + (members of cand) with more than b0 members, by plain recursion with a colouring bound; the
    first of its size wins.  Returns the positions ([] where none beats b0)."""
    best, path = [], [root]
    bound = [b0]

    def expand(S, size):
        verts, cols = [], []
        Q, k = S, 0
        while Q:
            k += 1
            U = Q
            while U:
                low = U & -U
                v = low.bit_length() - 1
                U &= ~(rows[v] | low)
                Q ^= low
                verts.append(v)
                cols.append(k)
        for i in range(len(verts) - 1, -1, -1):
            if size + cols[i] <= bound[0]:
                return
            v = verts[i]
            path.append(v)
            child = S & rows[v]
            if child:
                expand(child, size + 1)
            elif size + 1 > bound[0]:
                bound[0] = size + 1
                best[:] = path
            path.pop()
            S &= ~(1 << v)

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, len(rows) + 200))
    try:
        expand(cand, 1)
    finally:
        sys.setrecursionlimit(old)
    return list(best)


def ref_exact_resume(ok, order, first, held, ms=None):
    """The definition on Python integers.  held: [N] uint8, the set handed in; ms: the multi-start reference of (ok, order), computed
    here unless given.  No cap: every root finishes, proven = 1."""
    ok = np.asarray(ok, dtype=bool)
    N = ok.shape[0]
    held = np.asarray(held, dtype=np.uint8)
    live, rows = EX._rows(ok, order)
    n = len(live)
    if ms is None:
        ms = MS.ref_multistart_bitset(ok, order)
    lb, w0 = int(np.asarray(ms.accepted).sum()), int(held.sum())
    new = 0
    for a, cand in enumerate(live):
        if cand >= first:
            new |= 1 << a
    roots = [a for a in range(n) if (new >> a) & 1]
    m = len(roots)
    b0 = max(w0, lb)
    c = colours_of(rows, new)
    ub = min(n, w0 + c)
    incumbent = held.copy() if w0 >= lb else np.array(ms.accepted, dtype=np.uint8)
    searched = m > 0 and b0 < ub
    best_size, best, ran = b0, None, 0
    if searched:
        for p in roots:
            cand = rows[p] & ~(new & ((1 << p) - 1))
            if 1 + bin(cand).count("1") <= b0:
                continue
            ran += 1
            got = _search(rows, p, cand, b0)
            if len(got) > best_size:                              # (ascending r: the smallest r that attains the size stays)
                best_size, best = len(got), got
    if best is None:
        acc = incumbent
    else:
        acc = np.zeros(N, dtype=np.uint8)
        acc[[live[a] for a in best]] = 1
    changed = int(not np.array_equal(acc, held))
    return Resume(best_size, acc, 1, changed, n, m, w0, lb, c, ub, searched, ran)


# ---- the (case, split) pairs ---------------------------------------------------------------------------------------------
def _splits():
    out = []
    for c in EX.CASES:
        if c.N <= 129:
            firsts = sorted({min(max(f, 0), c.N) for f in (0, 1, 63, 64, 65, c.N // 2, c.N - 1, c.N)})
            out += [(c.id, f) for f in firsts]
    for cid in LARGE:
        N = EX.BY_ID[cid].N
        out += [(cid, f) for f in (N // 2, N - 64, N - 1)]
    return out


SPLITS = _splits()
SPLIT_IDS = ["%s@%d" % s for s in SPLITS]
CHAIN_CASES = [c.id for c in EX.CASES if c.N == 129]              # (decoys-129-40 is one of them)


@functools.lru_cache(maxsize=None)
def held_set(case_id, first):
    """The set handed in: EX.ref_exact's clique of the prefix, as bytes.  Computed once and shared; read-only."""
    N = EX.BY_ID[case_id].N
    acc = np.zeros(N, dtype=np.uint8)
    if first > 0:
        r = EX.ref_exact(prefix(EX.matrix(case_id), first), MC.set_order(N))
        assert r.finished
        acc[r.clique] = 1
    acc.setflags(write=False)
    return acc


@functools.lru_cache(maxsize=None)
def reference(case_id, first):
    """ref_exact_resume of a pair, computed once and shared."""
    N = EX.BY_ID[case_id].N
    r = ref_exact_resume(EX.matrix(case_id), MC.set_order(N), first, held_set(case_id, first), ms=EX.multistart(case_id))
    r.accepted.setflags(write=False)
    return r


def chain_firsts(N, burst):
    """The list lengths of a chain: burst, 2 burst, .., N."""
    out = list(range(burst, N, burst))
    return out + [N]
