"""Inputs and references for the census of the maximum consistent sets (ipc_set_max_census).

Plain module (no GPU use, no fixtures), in the manner of tests/exact_cases.py, whose matrices, orders and references it uses.
tests/test_census_cpu.py holds the two references against each other and against the table of the issue;
tests/test_gpu_census.py runs the kernels on the same cases.

The definition (include/ipc_amd_census.h), restated: L, positions and G as in tests/exact_cases.py; omega = the clique number of
G; MAX = the cliques of G with exactly omega members; count = |MAX|; core = the candidates in every member of MAX; support =
the candidates in some member.  No live candidate: MAX = {the empty set}, count = 1, core and support empty.  Subproblem q holds
the members of MAX whose smallest position is q; its candidate set is row(q) restricted to the positions > q; it is pruned at
once where 1 + |candidates| < omega, and `subproblems` counts the roots that are not."""
import functools
import sys

import numpy as np

import exact_cases as EX
import matrix_cases as MC


# ---- references --------------------------------------------------------------------------------------------------------
def ref_census(ok, order, omega):
    """(count, core [N] uint8, support [N] uint8, subproblems) by plain recursion on Python integers, one subproblem per
    position: a clique grows by its members in ascending position, so each is met once, at the subproblem of its smallest
    position; a branch ends where the members so far and the candidates left -- by their number, and on entry by the classes of
    a greedy colouring -- cannot make omega.  Members are taken in ascending position, not in the kernels' colour order: counts,
    AND and OR do not depend on it."""
    live, rows = EX._rows(ok, order)
    N = np.asarray(ok).shape[0]
    core_out, support_out = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8)
    n = len(live)
    if n == 0:
        return 1, core_out, support_out, 0
    assert omega >= 1
    found = [0, -1, 0]                                            # count, AND, OR over the cliques met

    def colours(S):
        """Classes of the sequential greedy colouring of S (tests/exact_cases.py, ref_colour_bound): a clique takes at most one
        member of a class, so no clique inside S has more members than this."""
        k = 0
        while S:
            k += 1
            sweep = S
            while sweep:
                low = sweep & -sweep
                sweep &= ~(rows[low.bit_length() - 1] | low)
                S ^= low
        return k

    def grow(members, size, cand):
        if size == omega:
            found[0] += 1
            found[1] &= members
            found[2] |= members
            return
        while cand and size + bin(cand).count("1") >= omega and size + colours(cand) >= omega:
            low = cand & -cand
            cand ^= low
            grow(members | low, size + 1, cand & rows[low.bit_length() - 1])      # (cand holds the positions behind `low` only)

    subproblems = 0
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, omega + 200))
    try:
        for q in range(n):
            cand = (rows[q] >> (q + 1)) << (q + 1)
            if 1 + bin(cand).count("1") < omega:
                continue
            subproblems += 1
            grow(1 << q, 1, cand)
    finally:
        sys.setrecursionlimit(old)
    for a in range(n):
        core_out[live[a]] = (found[1] >> a) & 1
        support_out[live[a]] = (found[2] >> a) & 1
    return found[0], core_out, support_out, subproblems


def nx_census(ok, order, omega, limit):
    """The same from networkx's enumeration of the maximal cliques, filtered to omega members: (count, core, support), or None
    where the graph has more than `limit` maximal cliques (the enumeration is cut there)."""
    import itertools

    import networkx as nx
    ok = np.asarray(ok, dtype=bool)
    N = ok.shape[0]
    live = [int(k) for k in order if ok[k][k]]
    core, support = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8)
    if not live:
        return 1, core, support
    g = nx.Graph()
    g.add_nodes_from(live)
    g.add_edges_from((a, b) for i, a in enumerate(live) for b in live[i + 1:] if ok[a][b])
    cliques = list(itertools.islice(nx.find_cliques(g), limit + 1))
    if len(cliques) > limit:
        return None
    top = [c for c in cliques if len(c) == omega]
    assert top and max(len(c) for c in cliques) == omega
    core[live] = 1
    for c in top:
        mark = np.zeros(N, dtype=np.uint8)
        mark[c] = 1
        core &= mark
        support |= mark
    return len(top), core, support


# ---- case list ---------------------------------------------------------------------------------------------------------
# far_conflict-128, -129 and -1025 hold 64 disjoint conflicting pairs: 2^64, 2^63 and many maximum cliques, which no reference
# enumerates -- the cap cases
CAP_CASE, CAP = "far_conflict-128", 4096
EXACT_CAPPED_CASE, EXACT_CAP = "decoys-129-40", 64                # (tests/test_gpu_exact.py: the exact stage itself is capped)
NOT_ENUMERABLE = ("far_conflict-128", "far_conflict-129")

# (omega, count, core size, support size): the table of the issue, from a scratch run of a reference on a CPU
TABLE = {
    "planted-63": (38, 8, 35, 41), "planted-64": (36, 4, 34, 38), "planted-65": (31, 2, 30, 32),
    "planted-128": (73, 8, 70, 76), "planted-129": (64, 16, 60, 68),
    "identity-129": (1, 129, 0, 129), "dead-129": (0, 1, 0, 0), "all_ones-129": (129, 1, 129, 129),
    "chain_conflict-64": (32, 33, 0, 64), "chain_conflict-128": (64, 65, 0, 128), "chain_conflict-129": (65, 1, 65, 65),
    "far_conflict-65": (64, 2, 63, 65),
    "two_cliques-129-64": (64, 2, 0, 128), "two_cliques-1025-300": (300, 2, 0, 600),
    "decoys-129-40": (40, 1, 40, 40), "decoys-1025-300": (300, 1, 300, 300), "decoys-4161-70": (70, 1, 70, 70),
    "nlive_exact-1025-64": (36, 288, 27, 45), "nlive_exact-1025-128": (51, 1728, 40, 64),
    "nlive_exact-4161-64": (25, 6, 22, 28), "nlive_exact-4161-65": (30, 96, 23, 37),
    "hidden-4161": (612, 1, 612, 612), "hidden_c-1025": (140, 4, 138, 142),
}
SMALL_IDS = [c.id for c in EX.CASES if c.N <= 129 and c.id not in NOT_ENUMERABLE]
CASE_IDS = SMALL_IDS + [i for i in TABLE if i not in SMALL_IDS]
NX_LIMIT = 20000


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """(omega, count, core, support, subproblems) of a case: omega from tests/exact_cases.py, the rest from ref_census; computed
    once and shared, callers must not modify it."""
    omega = EX.reference(case_id).omega
    count, core, support, sub = ref_census(EX.matrix(case_id), MC.set_order(EX.BY_ID[case_id].N), omega)
    core.setflags(write=False), support.setflags(write=False)
    return omega, count, core, support, sub


def check_invariants(ok, accepted, core, support, count, size):
    """What holds of a proven census: core <= accepted <= support, count == 1 exactly where the three are one set, the sizes in
    that order, and a support of live candidates."""
    accepted, core, support = (np.asarray(a, dtype=np.uint8) for a in (accepted, core, support))
    assert set(np.unique(np.concatenate([core, support])).tolist()) <= {0, 1}
    assert (core <= accepted).all() and (accepted <= support).all()
    assert (count == 1) == (core.tobytes() == support.tobytes() == accepted.tobytes())
    assert int(core.sum()) <= size == int(accepted.sum()) <= int(support.sum())
    assert np.asarray(ok, dtype=bool).diagonal()[np.flatnonzero(support)].all()
    assert count >= 1
