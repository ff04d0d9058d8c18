"""Injected inputs for the matrix back end: what happens to a cell's verdict after it is solved.

Plain module (no GPU use, no fixtures).  ipc_assemble_matrix and ipc_set_max take device arrays from the caller, so
the symmetric assembly (k_assemble) and the greedy consistent set (k_set_max) can be fed bit patterns the dog-leg
never produces and held against the plain references below; tests/test_matrix_backend_cpu.py checks the references
against each other and that the inputs are adversarial by the references alone, tests/test_gpu_matrix_backend.py
runs the kernels on them.

The graphs only carry the candidates' end vertices (which fix the processing order and the overlap rule); their
measurements are those of the odometry itself and are solved by one test only (the cell plan).

References are Python loops over numpy bool arrays: no 64-bit words, no rounds of 64, no compaction.
"""
import functools
from collections import namedtuple

import numpy as np

from ipc_amd.graphio import PoseGraph

SET_SIZES = (1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2049, 4097, 4161)
ASSEMBLE_SIZES = (1, 63, 64, 65, 129, 257, 1025)
CHAIN_SIZES = (129, 1025)
PLAN_SIZES = (63, 64, 65, 257)
ROUND = 64                                    # live candidates the set-max takes per round (diagnostics only)


# ---- processing order ------------------------------------------------------------------------------------------------
def order_with_ties(N, seed):
    """A permutation of 0 .. N-1 made of ascending runs of ~8 candidates: what sorting by (key, index) gives when
    many candidates share a key."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, max(1, N // 8), N)
    return np.lexsort((np.arange(N), keys)).astype(np.int32)


def sort_order(ids):
    """The processing order: by the greater end vertex, ties to the lower index (restated, not imported)."""
    hi = np.asarray(ids).reshape(-1, 2).max(1)
    return np.array(sorted(range(len(hi)), key=lambda k: (int(hi[k]), k)), dtype=np.int32)


def graph_for(order=None, intervals=None, V=None, shifted=()):
    """SE2 PoseGraph on a straight unit-step line with unit information.

    `order` (a permutation): the greater end vertex of every loop is chosen so that the processing order is `order` --
    the key grows by one wherever the permutation descends, so an ascending run shares one key and is ordered by the
    tie rule alone.  `intervals` [N, 2] (from, to) instead gives the end vertices directly.  Loop measurements are
    the odometry's own (from -> to along the line); the candidates in `shifted` get 30 m more and fail any cell."""
    if intervals is None:
        order = np.asarray(order, dtype=np.int32)
        N = len(order)
        assert sorted(order.tolist()) == list(range(N))
        key = np.zeros(N, dtype=np.int64)
        cur = 2
        for p in range(N):
            if p and order[p] < order[p - 1]:
                cur += 1
            key[order[p]] = cur
        lo = np.maximum(0, key - 2 - np.arange(N) % 5)
        ids = np.stack([lo, key], axis=1)
        ids[1::2] = ids[1::2, ::-1]                          # every second loop reversed (from > to)
    else:
        ids = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
        N = len(ids)
    ids = ids.astype(np.int32)
    assert (np.abs(ids[:, 0] - ids[:, 1]) >= 2).all() and ids.min() >= 0
    if order is not None:
        assert np.array_equal(sort_order(ids), order)
    nV = int(ids.max()) + 2 if V is None else V
    assert ids.max() < nV
    verts = np.zeros((nV, 3))
    verts[:, 0] = np.arange(nV)
    odom_meas = np.tile([1.0, 0.0, 0.0], (nV - 1, 1))
    odom_info = np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (nV - 1, 1))
    loop_meas = np.zeros((N, 3))
    loop_meas[:, 0] = ids[:, 1] - ids[:, 0]
    for k in shifted:
        loop_meas[k, 0] += 30.0
    loop_info = np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (N, 1))
    return PoseGraph(2, verts, odom_meas, odom_info, ids, loop_meas, loop_info, dict(name="matrix-case"))


# ---- plain references ------------------------------------------------------------------------------------------------
def ref_assemble(U, lo, hi):
    """C[i][i] = U[i][i]; i != j: the solved bit U[min][max] where the intervals overlap with positive length, else
    U[i][i] & U[j][j] (reference src/consensus.cpp:157-159).  Only the upper triangle of U is read."""
    N = len(lo)
    C = np.zeros((N, N), dtype=bool)
    for i in range(N):
        C[i][i] = U[i][i]
        for j in range(i + 1, N):
            if min(hi[i], hi[j]) - max(lo[i], lo[j]) > 0:
                C[i][j] = C[j][i] = U[i][j]
            else:
                C[i][j] = C[j][i] = U[i][i] and U[j][j]
    return C


def ref_set_max(ok, order):
    """Greedy consistent set: in processing order, a candidate whose own cell passed joins if it agrees with every
    member so far."""
    N = len(order)
    acc = np.zeros(N, dtype=bool)
    for k in order:
        if not ok[k][k]:
            continue
        if ok[k][acc].all():
            acc[k] = True
    return acc.astype(np.uint8)


def _blocks(ok, order):
    """Per block of ROUND live candidates: (members in order, the set as it stood at the block's start)."""
    acc = ref_set_max(ok, order).astype(bool)
    live = [int(k) for k in order if ok[k][k]]
    pos = {k: p for p, k in enumerate(live)}
    out = []
    for b in range(0, len(live), ROUND):
        before = np.array([acc[k] and pos[k] < b for k in range(len(order))], dtype=bool)
        out.append((live[b:b + ROUND], before))
    return out, acc


def round_mate_rejects(ok, order):
    """Diagnostic: per block of 64 live candidates, how many agree with the set as it stood at the block's start but
    are turned down (by a member of their own block)."""
    blocks, acc = _blocks(ok, order)
    return [sum(1 for k in mem if ok[k][before].all() and not acc[k]) for mem, before in blocks]


def joins_past_rejected_mate(ok, order):
    """Diagnostic: accepted candidates that conflict with an earlier member of their own block which agreed with the
    set at the block's start and was turned down all the same."""
    blocks, acc = _blocks(ok, order)
    n = 0
    for mem, before in blocks:
        for q, k in enumerate(mem):
            if acc[k] and any(not ok[k][m] and not acc[m] and ok[m][before].all() for m in mem[:q]):
                n += 1
    return n


# ---- matrix generators (all symmetric) ---------------------------------------------------------------------------------
def _sym(rng, N, p):
    a = np.triu(rng.random((N, N)) < p, 1)
    return a | a.T


def planted(N, seed, clique=0.6, p_diag=0.9, p_conflict=0.002, p_out=0.3):
    rng = np.random.default_rng(seed)
    inc = rng.random(N) < clique
    both = inc[:, None] & inc[None, :]
    ok = np.where(both, ~_sym(rng, N, p_conflict), _sym(rng, N, p_out))
    np.fill_diagonal(ok, rng.random(N) < p_diag)
    return ok


def all_ones(N):
    return np.ones((N, N), dtype=bool)


def identity(N):
    return np.eye(N, dtype=bool)


def dead(N):
    ok = _sym(np.random.default_rng(N), N, 0.5)
    np.fill_diagonal(ok, False)
    return ok


def chain_conflict(N, order):
    ok = np.ones((N, N), dtype=bool)
    for p in range(1, N):
        ok[order[p], order[p - 1]] = ok[order[p - 1], order[p]] = False
    return ok


def far_conflict(N, order):
    """Position p conflicts with position p - 64 only, everyone is live: round-mates never conflict, every verdict
    comes from the accepted mask of the round before -- at 65 and 66 words through the second trip of the lane loop
    for the members whose index is 4096 or more.  The even rounds join."""
    ok = np.ones((N, N), dtype=bool)
    for p in range(ROUND, N):
        ok[order[p], order[p - ROUND]] = ok[order[p - ROUND], order[p]] = False
    return ok


def late_live(N, order, seed):
    assert N > 1024
    ok = np.zeros((N, N), dtype=bool)
    tail = np.asarray(order[1024:])
    ok[np.ix_(tail, tail)] = planted(N - 1024, seed)
    # the dead candidates' other bits are set: a kernel that let one through would be taken with everything
    head = np.asarray(order[:1024])
    ok[head, :] = True
    ok[:, head] = True
    ok[head, head] = False
    return ok


def nlive_exact(N, n, seed):
    rng = np.random.default_rng(seed)
    alive = np.sort(rng.choice(N, n, replace=False))
    ok = _sym(rng, N, 0.5)
    ok[np.ix_(alive, alive)] = planted(n, seed + 1, p_diag=1.0, p_conflict=0.02)
    np.fill_diagonal(ok, False)
    ok[alive, alive] = True
    return ok


SetCase = namedtuple("SetCase", "id gen N arg")


def _set_cases():
    out = [SetCase("planted-%d" % N, "planted", N, None) for N in SET_SIZES]
    for gen in ("all_ones", "identity", "dead", "chain_conflict", "far_conflict"):
        out += [SetCase("%s-%d" % (gen, N), gen, N, None) for N in SET_SIZES]
    out += [SetCase("late_live-%d" % N, "late_live", N, None) for N in (1025, 2049, 4161)]
    out += [SetCase("nlive_exact-1025-%d" % n, "nlive_exact", 1025, n) for n in (1, 63, 64, 65, 128)]
    out += [SetCase("nlive_exact-4161-%d" % n, "nlive_exact", 4161, n) for n in (64, 65)]
    return out


SET_CASES = _set_cases()


# Seeds are part of the inputs (tests/test_matrix_backend_cpu.py holds the conditions on them).  Where an outsider at the
# head of the order wins and the default seed leaves a set of a handful, another seed gives one of a few hundred.
PLANTED_SEEDS = {63: 7363, 128: 7228, 129: 7429, 4097: 11397, 4161: 11261}


def set_order(N):
    """One processing order per size: the cases of one size share an engine."""
    return order_with_ties(N, 100 + N)


def set_matrix(case):
    N, order, seed = case.N, set_order(case.N), 7000 + case.N
    if case.gen == "planted":
        return planted(N, PLANTED_SEEDS.get(N, seed))
    if case.gen == "chain_conflict":
        return chain_conflict(N, order)
    if case.gen == "far_conflict":
        return far_conflict(N, order)
    if case.gen == "late_live":
        return late_live(N, order, seed)
    if case.gen == "nlive_exact":
        return nlive_exact(N, case.arg, seed + case.arg)
    return {"all_ones": all_ones, "identity": identity, "dead": dead}[case.gen](N)


def set_expected(case, ok, order):
    """What the case is built to give, where that is known without running a reference (else None)."""
    N = case.N
    acc = np.zeros(N, dtype=np.uint8)
    if case.gen == "all_ones":
        acc[:] = 1
    elif case.gen == "identity":
        acc[order[0]] = 1
    elif case.gen == "dead":
        pass
    elif case.gen == "chain_conflict":
        acc[order[0::2]] = 1
    elif case.gen == "far_conflict":
        acc[[order[p] for p in range(N) if (p // ROUND) % 2 == 0]] = 1
    else:
        return None
    return acc


def pack_rows(ok):
    """[R, N] bool -> [R, words] uint64, bit j of a row = ok[., j]; bits >= N are zero."""
    R, N = ok.shape
    words = (N + 63) // 64
    pad = np.zeros((R, words * 64), dtype=np.uint8)
    pad[:, :N] = ok
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint64).reshape(R, words)


# ---- intervals for the assembly ------------------------------------------------------------------------------------------
def intervals_for(N, seed, max_len=30, V=None):
    """[N, 2] (from, to): anchors at random places, followers nested in / equal to / touching / overlapping by one
    edge a random anchor, two candidates at the head of the line that overlap nobody (they touch each other), about
    four in ten reversed; indices shuffled.  The line is ~N / 2 vertices long, so a 64-candidate word often holds
    nobody that overlaps a given row."""
    rng = np.random.default_rng(seed)
    if N == 1:
        return np.array([[2, 0]], dtype=np.int32)
    span = max(2 * max_len + 8, N // 2) if V is None else V - 1
    iv = [(0, 2), (2, 4)][:N]
    anchors = []
    while len(iv) < N:
        kind = len(iv) % 6 if anchors else 0
        if kind in (0, 5):                                 # an anchor (5: a short one, 2 .. 5 edges)
            ln = int(rng.integers(4, max_len + 1)) if kind == 0 else int(rng.integers(2, 6))
            lo = int(rng.integers(5, span - ln + 1))
            anchors.append((lo, lo + ln))
            iv.append((lo, lo + ln))
            continue
        a_lo, a_hi = anchors[int(rng.integers(len(anchors)))]
        if kind == 1 and a_hi - a_lo >= 4:                 # strictly nested
            c = (a_lo + 1, a_hi - 1)
        elif kind == 2:                                    # equal
            c = (a_lo, a_hi)
        elif kind == 3:                                    # touching: starts where the anchor ends
            c = (a_hi, min(span, a_hi + int(rng.integers(2, max_len + 1))))
        else:                                              # overlaps the anchor's last edge only
            c = (a_hi - 1, min(span, a_hi - 1 + int(rng.integers(2, max_len + 1))))
        if c[1] - c[0] < 2:
            c = (a_lo, a_hi)
        iv.append(c)
    iv = np.array(iv, dtype=np.int32)[rng.permutation(N)]
    rev = rng.random(N) < 0.4
    iv[rev] = iv[rev, ::-1]
    return iv


def interval_kinds(ids):
    """Which kinds of pairs (and reversed loops) a candidate list holds."""
    ids = np.asarray(ids)
    lo, hi = ids.min(1), ids.max(1)
    ov = np.minimum(hi[:, None], hi[None, :]) - np.maximum(lo[:, None], lo[None, :])
    off = ~np.eye(len(lo), dtype=bool)
    kinds = set()
    if (ids[:, 0] > ids[:, 1]).any():
        kinds.add("reversed")
    if ((lo[:, None] < lo[None, :]) & (hi[None, :] < hi[:, None])).any():
        kinds.add("nested")
    if ((lo[:, None] == lo[None, :]) & (hi[:, None] == hi[None, :]) & off).any():
        kinds.add("equal")
    if (ov < 0).any():
        kinds.add("disjoint")
    if (hi[:, None] == lo[None, :]).any():
        kinds.add("touching")
    if ((ov == 1) & off).any():
        kinds.add("one-edge")
    return kinds


ALL_KINDS = {"reversed", "nested", "equal", "disjoint", "touching", "one-edge"}


def select_paths(ids):
    """(row, word) pairs in which no other candidate of the word overlaps the row / in which some do."""
    ids = np.asarray(ids)
    lo, hi = ids.min(1), ids.max(1)
    N = len(lo)
    words = (N + 63) // 64
    ov = np.zeros((N, words * 64), dtype=bool)
    ov[:, :N] = (np.minimum(hi[:, None], hi[None, :]) - np.maximum(lo[:, None], lo[None, :])) > 0
    ov[np.arange(N), np.arange(N)] = False
    some = ov.reshape(N, words, 64).any(2)
    return int((~some).sum()), int(some.sum())


def expected_cells(ids, alive=None):
    """Sorted (i, j), i <= j: every diagonal cell, a pair cell where the intervals overlap with positive length.  With
    `alive`: the diagonal cells of everyone, the pair cells among the alive only (the set-only mode)."""
    ids = np.asarray(ids)
    lo, hi = ids.min(1), ids.max(1)
    out = []
    for i in range(len(lo)):
        out.append((i, i))
        for j in range(i + 1, len(lo)):
            if alive is not None and not (alive[i] and alive[j]):
                continue
            if min(hi[i], hi[j]) - max(lo[i], lo[j]) > 0:
                out.append((i, j))
    return out


AssembleCase = namedtuple("AssembleCase", "N ids U C")


@functools.lru_cache(maxsize=None)
def assemble_case(N):
    """Intervals, solved bits (density 0.5 above the diagonal, 0.8 on it) and the reference matrix; computed once per
    size, callers must not modify it."""
    ids = intervals_for(N, 300 + N)
    rng = np.random.default_rng(900 + N)
    U = np.triu(rng.random((N, N)) < 0.5, 1)
    np.fill_diagonal(U, rng.random(N) < 0.8)
    C = ref_assemble(U, ids.min(1), ids.max(1))
    for a in (ids, U, C):
        a.setflags(write=False)
    return AssembleCase(N, ids, U, C)


def gathered_rows(U, slot, nrows, poison_seed):
    """[nrows, words] uint64 as the all-gather leaves them: row i of U at row slot[i], bits i .. N-1.  Everything the
    rule does not read -- the bits below the diagonal, the bits >= N of the last word, the rows no candidate owns -- is
    random, drawn from `poison_seed`."""
    N = U.shape[0]
    words = (N + 63) // 64
    rng = np.random.default_rng(poison_seed)
    rows = rng.random((N, words * 64)) < 0.5
    upper = np.triu(np.ones((N, N), dtype=bool))
    rows[:, :N] = np.where(upper, U, rows[:, :N])
    out = rng.integers(0, 2 ** 64, (nrows, words), dtype=np.uint64)
    out[np.asarray(slot)] = np.packbits(rows, axis=1, bitorder="little").view(np.uint64).reshape(N, words)
    return out


# ---- the cell plan -------------------------------------------------------------------------------------------------------
PLAN_V, PLAN_MAX_LEN = 200, 24                             # two overlapping loops span at most 47 edges: one-wave cells


def plan_shifted(N):
    return [k for k in range(N) if k % 5 == 2]


@functools.lru_cache(maxsize=None)
def plan_graph(N):
    ids = intervals_for(N, 500 + N, max_len=PLAN_MAX_LEN, V=PLAN_V)
    return graph_for(intervals=ids, V=PLAN_V, shifted=plan_shifted(N))
