"""Inputs and references for the exact maximum consistent set (ipc_set_max_exact).

Plain module (no GPU use, no fixtures), in the manner of tests/multistart_cases.py, whose matrices, orders and references it
uses.  tests/test_exact_cpu.py holds the references against networkx and shows that the inputs are adversarial by the references
alone; tests/test_gpu_exact.py runs the kernels on them.

The definition (include/ipc_amd.h): L = the processing order restricted to the live candidates (ok[k][k]); G = the graph on L
whose edges are the set off-diagonal bits; omega = its clique number; LB = the size of the multi-start set; UB0 = the number of
colours of the sequential greedy colouring of L in position order."""
import functools
import sys
from collections import namedtuple

import numpy as np

import matrix_cases as MC
import multistart_cases as MS

Exact = namedtuple("Exact", "omega clique steps finished")      # clique: candidate indices (a maximum one when finished)


def _rows(ok, order):
    """(live list, rows): rows[a] = the neighbours of l_a as a bit set over the positions of L, the diagonal cleared."""
    ok = np.asarray(ok, dtype=bool)
    live = [int(k) for k in order if ok[k][k]]
    n = len(live)
    if n == 0:
        return live, []
    sub = ok[np.ix_(live, live)].copy()
    np.fill_diagonal(sub, False)
    packed = np.packbits(sub, axis=1, bitorder="little")
    return live, [int.from_bytes(packed[a].tobytes(), "little") for a in range(n)]


# ---- references --------------------------------------------------------------------------------------------------------
class _OutOfSteps(Exception):
    pass


def ref_exact(ok, order, cap=None):
    """Maximum clique of G by plain recursion: colour the candidates greedily (a clique takes at most one vertex of a colour
    class), branch from the last colour down, stop where size + colour cannot beat the best clique so far.  No lower bound
    from outside, one incumbent.  A step is one coloured vertex; with `cap`, gives up after that many (finished = False, the
    best clique so far)."""
    live, rows = _rows(ok, order)
    best, path = [], []
    steps = [0]

    def expand(P, size):
        verts, colours = [], []
        Q, k = P, 0
        while Q:
            k += 1
            U = Q
            while U:
                low = U & -U
                v = low.bit_length() - 1
                U &= ~(rows[v] | low)
                Q ^= low
                verts.append(v)
                colours.append(k)
        steps[0] += len(verts)
        if cap is not None and steps[0] > cap:
            raise _OutOfSteps
        for i in range(len(verts) - 1, -1, -1):
            if size + colours[i] <= len(best):
                return
            v = verts[i]
            path.append(v)
            child = P & rows[v]
            if child:
                expand(child, size + 1)
            elif size + 1 > len(best):
                best[:] = path
            path.pop()
            P &= ~(1 << v)

    finished = True
    if rows:
        old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old, len(rows) + 200))
        try:
            expand((1 << len(rows)) - 1, 0)
        except _OutOfSteps:
            finished = False
        finally:
            sys.setrecursionlimit(old)
    return Exact(len(best), sorted(live[v] for v in best), steps[0], finished)


def ref_colour_bound(ok, order):
    """UB0: repeat -- open a colour class, sweep the uncoloured positions of L in ascending order, take a position if it is
    adjacent to no member of the class.  The number of classes.  On bit sets over the positions: a position the sweep takes
    strikes its neighbours from the rest of the sweep."""
    _, rows = _rows(ok, order)
    uncoloured, k = (1 << len(rows)) - 1, 0
    while uncoloured:
        k += 1
        sweep = uncoloured
        while sweep:
            low = sweep & -sweep
            sweep &= ~(rows[low.bit_length() - 1] | low)
            uncoloured ^= low
    return k


def ref_colour_bound_plain(ok, order):
    """The same as loops over the bool array, for the small cases."""
    ok = np.asarray(ok, dtype=bool)
    live = [int(k) for k in order if ok[k][k]]
    colour = {}
    k = 0
    while len(colour) < len(live):
        k += 1
        members = []
        for a, cand in enumerate(live):
            if a in colour:
                continue
            if not any(ok[cand][live[m]] for m in members):
                members.append(a)
                colour[a] = k
    return k


def is_clique_of_live(ok, acc):
    """acc [N] uint8: every member is live and every two members agree."""
    mem = np.flatnonzero(acc)
    return bool(np.asarray(ok, dtype=bool)[np.ix_(mem, mem)].all())


# ---- generators --------------------------------------------------------------------------------------------------------
def decoys(N, order, m):
    """Positions N-m .. N-1 form a clique K; positions 0 .. m-1 are decoys, the i-th adjacent to the i-th member of K only;
    nobody else agrees with anybody; everyone is live.  Every greedy chain ends after two members (a decoy and its partner, or
    a member of K and its decoy, who comes first in the order); the clique number is m."""
    assert 2 * m <= N and m >= 2
    ok = np.eye(N, dtype=bool)
    K = np.asarray(order[N - m:])
    ok[np.ix_(K, K)] = True
    for i in range(m):
        ok[order[i], K[i]] = ok[K[i], order[i]] = True
    return ok


def hidden(N):
    return MC.planted(N, 9000 + N, clique=0.15, p_diag=1.0, p_conflict=0.0, p_out=0.05)


def hidden_c(N):
    return MC.planted(N, 9000 + N, clique=0.15, p_diag=0.9, p_conflict=0.0005, p_out=0.3)


# ---- case list ---------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id N make")            # make() -> ok [N, N] bool; the order is MC.set_order(N)

DECOYS = ((129, 40), (1025, 300), (4161, 70))
CAP_ONLY = ("planted-1025", "late_live-2049", "planted_all_live-4161")     # no reference finished these: the cap test only
KNOB = "IPC_EXACT_STEP_CAP"                       # read at ipc_create: steps after which a subproblem gives up


def _cases():
    out = [Case(c.id, c.N, c.make) for c in MS.CASES if c.N <= 129]
    ids = ["nlive_exact-1025-%d" % n for n in (1, 63, 64, 65, 128)] + ["nlive_exact-4161-%d" % n for n in (64, 65)]
    ids += ["%s-1025" % gen for gen in ("all_ones", "identity", "dead", "chain_conflict", "far_conflict")]
    ids += ["two_cliques-1025-300"]
    out += [Case(i, MS.BY_ID[i].N, MS.BY_ID[i].make) for i in ids]
    out += [Case("decoys-%d-%d" % (N, m), N, functools.partial(lambda N, m: decoys(N, MC.set_order(N), m), N, m)) for N, m in DECOYS]
    out += [Case("hidden-%d" % N, N, functools.partial(hidden, N)) for N in (1025, 4161)]
    out += [Case("hidden_c-1025", 1025, functools.partial(hidden_c, 1025))]
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}
BY_ID.update({i: Case(i, MS.BY_ID[i].N, MS.BY_ID[i].make) for i in CAP_ONLY})


@functools.lru_cache(maxsize=None)
def matrix(case_id):
    ok = np.asarray(BY_ID[case_id].make(), dtype=bool)
    ok.setflags(write=False)
    return ok


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """ref_exact of a case, computed once and shared."""
    r = ref_exact(matrix(case_id), MC.set_order(BY_ID[case_id].N))
    assert r.finished
    return r


@functools.lru_cache(maxsize=None)
def multistart(case_id):
    """The multi-start reference (LB and its set) of a case, computed once and shared; callers must not modify it."""
    r = MS.ref_multistart_bitset(matrix(case_id), MC.set_order(BY_ID[case_id].N))
    r.accepted.setflags(write=False), r.sizes.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def colour_bound(case_id):
    return ref_colour_bound(matrix(case_id), MC.set_order(BY_ID[case_id].N))
