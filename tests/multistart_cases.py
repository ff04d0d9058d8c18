"""Inputs and references for the multi-start set maximisation (ipc_set_max_multistart).

Plain module (no GPU use, no fixtures), in the manner of tests/matrix_cases.py, whose matrices, orders and packing it uses.
tests/test_multistart_cpu.py holds the two references against each other and shows that the inputs are adversarial by the
references alone; tests/test_gpu_multistart.py runs the kernels on them.

The definition (include/ipc_amd.h): L = the processing order restricted to the live candidates (ok[k][k]); S_q = the greedy set
over l_q, l_0, l_1, .., l_{q-1}, l_{q+1}, ..; the result is the S_q of greatest cardinality, ties to the smallest q;
sizes[k] = |S_q| for k = l_q and 0 for a dead candidate."""
import functools
from collections import namedtuple

import numpy as np

import matrix_cases as MC

Result = namedtuple("Result", "accepted sizes best_q live")      # uint8 [N], int32 [N], position in L or -1, candidates of L


# ---- references --------------------------------------------------------------------------------------------------------
def ref_multistart_plain(ok, order):
    """Loops over bool arrays, exactly the definition: no words, no compaction, no bit tricks."""
    N = len(order)
    live = [int(k) for k in order if ok[k][k]]
    sizes = np.zeros(N, dtype=np.int32)
    best, best_q = None, -1
    for q, seed in enumerate(live):
        members = [seed]
        for k in live[:q] + live[q + 1:]:
            if all(ok[k][m] for m in members):
                members.append(k)
        sizes[seed] = len(members)
        if best is None or len(members) > len(best):
            best, best_q = members, q
    acc = np.zeros(N, dtype=np.uint8)
    if best is not None:
        acc[best] = 1
    return Result(acc, sizes, best_q, live)


def ref_multistart_bitset(ok, order):
    """The same on Python integers as bit sets over the positions of L: cand = row(l_q) minus l_q; the lowest set bit joins,
    cand &= its row.  For the large cases."""
    ok = np.asarray(ok, dtype=bool)
    N = len(order)
    live = [int(k) for k in order if ok[k][k]]
    n = len(live)
    sizes = np.zeros(N, dtype=np.int32)
    acc = np.zeros(N, dtype=np.uint8)
    if n == 0:
        return Result(acc, sizes, -1, live)
    sub = ok[np.ix_(live, live)].copy()
    np.fill_diagonal(sub, False)
    packed = np.packbits(sub, axis=1, bitorder="little")
    rows = [int.from_bytes(packed[a].tobytes(), "little") for a in range(n)]

    def chain(q):
        cand, members = rows[q], [q]
        while cand:
            c = (cand & -cand).bit_length() - 1
            members.append(c)
            cand &= rows[c]
        return members

    best_q, best_len = -1, 0
    for q in range(n):
        s = len(chain(q))
        sizes[live[q]] = s
        if s > best_len:
            best_q, best_len = q, s
    acc[[live[c] for c in chain(best_q)]] = 1
    return Result(acc, sizes, best_q, live)


# ---- generators --------------------------------------------------------------------------------------------------------
def planted_all_live(N, seed):
    """Everyone is live, a clique of ~15 % hidden among outsiders that agree with 5 %: the head of the order is an outsider."""
    return MC.planted(N, seed, clique=0.15, p_diag=1.0, p_out=0.05)


def two_cliques(N, order, k):
    """Position 0 agrees with nobody, positions 1 .. k form a clique, positions k+1 .. 2k a second one; no other agreements.
    The result is exactly the positions 1 .. k: a tie at equal size that neither position 0 nor the later seed wins."""
    assert 2 * k < N
    ok = np.eye(N, dtype=bool)
    a, b = np.asarray(order[1:k + 1]), np.asarray(order[k + 1:2 * k + 1])
    ok[np.ix_(a, a)] = True
    ok[np.ix_(b, b)] = True
    return ok


# ---- case list ---------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id N make")            # make() -> ok [N, N] bool; the order is MC.set_order(N)

SMALL_SIZES = (1, 2, 63, 64, 65, 128, 129, 1025)


def _cases():
    by_id = {c.id: c for c in MC.SET_CASES}
    ids = ["%s-%d" % (gen, N) for gen in ("planted", "all_ones", "identity", "dead", "chain_conflict", "far_conflict")
           for N in SMALL_SIZES]
    ids += ["planted-4097", "planted-4161", "late_live-2049", "late_live-4161", "far_conflict-4161"]
    ids += [c.id for c in MC.SET_CASES if c.gen == "nlive_exact"]
    out = [Case(i, by_id[i].N, functools.partial(MC.set_matrix, by_id[i])) for i in ids]
    out += [Case("planted_all_live-%d" % N, N, functools.partial(planted_all_live, N, 7000 + N)) for N in (65, 129, 4161)]
    out += [Case("two_cliques-%d-%d" % (N, k), N, functools.partial(lambda N, k: two_cliques(N, MC.set_order(N), k), N, k))
            for N, k in ((129, 64), (131, 65), (1025, 300))]
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}
KNOB = "IPC_MULTISTART_REG_WORDS"                  # read at ipc_create: 0 sends every N to the LDS kernel, 1 / 2 cap the register kernel


@functools.lru_cache(maxsize=None)
def matrix(case_id):
    ok = np.asarray(BY_ID[case_id].make(), dtype=bool)
    ok.setflags(write=False)
    return ok


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The bitset reference of a case, computed once and shared; callers must not modify it."""
    c = BY_ID[case_id]
    r = ref_multistart_bitset(matrix(case_id), MC.set_order(c.N))
    r.accepted.setflags(write=False), r.sizes.setflags(write=False)
    return r
