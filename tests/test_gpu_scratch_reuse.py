"""One engine through shrinking and growing candidate lists: the set-maximisation workspaces hold more than the N of the moment.

Every other injected-matrix test makes one engine per size, so a workspace's capacity equals N wherever its sub-arrays (live, pos,
sizes; flag, size, steps) are cut -- a slice cut at N instead of the capacity, or the other way round, shows only when the two
differ.  Here one engine, on a chain long enough for the largest list, has its candidate list replaced through
4161 -> 129 -> 1025 -> 129 -> 4161 and at every size runs, on the decoys matrix of that size (tests/exact_cases.py: the multi-start
ends at 2, below the colour bound, so the search runs; one word per lane up to 4096 candidates, two at 4161), in this order:
the multi-start with sizes, the exact set, the exact set resumed at a split of tests/exact_resume_cases.py, the greedy.  Each result
against the plain references those tests already hold (the multi-start's through EX.multistart: MS.ref_multistart_bitset on the
case's matrix, the decoys being exact cases), poisoned guard bytes behind every output, and the second visit to a size byte for byte
the first.  No tolerances: the outputs are integers and bytes."""
import numpy as np
import pytest

import exact_cases as EX
import exact_resume_cases as ER
import matrix_cases as MC
import multistart_cases as MS
import sweep_cases as SC

pytestmark = pytest.mark.gpu

POISON, POISON32 = 0xAA, 0x5A5A5A5A
VISITS = (4161, 129, 1025, 129, 4161)
CASE = {4161: ("decoys-4161-70", 2080), 129: ("decoys-129-40", 64), 1025: ("decoys-1025-300", 512)}     # size -> (case, split)


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in SC.ENV_KEYS + (MS.KNOB, EX.KNOB):
        monkeypatch.delenv(k, raising=False)


def _guarded(b, N, dtype, poison, head=None):
    import torch
    buf = np.full(N + 64, poison, dtype=dtype)
    if head is not None:
        buf[:N] = head
    return torch.from_numpy(buf).to(b.device)


def _out(t, N, poison, what):
    a = t.cpu().numpy()
    assert (a[N:] == poison).all(), "wrote behind %s[N]" % what
    return a[:N].copy()


def _visit(eng, b, N):
    """The four calls at the list of N candidates; every output as bytes, every report as a dict."""
    import torch
    case_id, first = CASE[N]
    assert (case_id, first) in ER.SPLITS and EX.BY_ID[case_id].N == N
    order = MC.set_order(N)
    g = MC.graph_for(order, V=eng.graph.V)
    eng.set_candidates(g.loop_ids, g.loop_meas, g.loop_info)
    assert eng.N == N and np.array_equal(eng.candidate_order(), order)
    ok, packed = EX.matrix(case_id), MC.pack_rows(EX.matrix(case_id))
    ms, ex, held, er = EX.multistart(case_id), EX.reference(case_id), ER.held_set(case_id, first), ER.reference(case_id, first)
    lb = int(ms.accepted.sum())
    assert lb == 2 < ex.omega, "the case no longer forces a search"               # (LB below omega, so below the colour bound too)
    with b.stream_ctx():
        bits = torch.from_numpy(np.ascontiguousarray(packed).view(np.int64).reshape(-1)).to(b.device)
        # the multi-start with sizes
        acc, sizes = _guarded(b, N, np.uint8, POISON), _guarded(b, N, np.int32, POISON32)
        b.set_max_multistart(bits, acc, sizes)
        b.stream.synchronize()
        ms_acc, ms_sizes = _out(acc, N, POISON, "accepted"), _out(sizes, N, POISON32, "sizes")
        assert np.array_equal(ms_acc, ms.accepted) and np.array_equal(ms_sizes, ms.sizes)
        # the exact set (as _check_proven of tests/test_gpu_exact.py)
        acc = _guarded(b, N, np.uint8, POISON)
        ex_rep = b.set_max_exact(bits, acc)
        b.stream.synchronize()
        ex_acc = _out(acc, N, POISON, "accepted")
        print(N, case_id, ex_rep)
        assert ex_rep["proven"] == 1 and ex_rep["capped"] == 0 and ex_rep["size"] == ex_rep["upper_bound"] == ex.omega
        assert ex_rep["multistart_size"] == lb and ex_rep["live"] == len(ms.live)
        assert int(ex_acc.sum()) == ex.omega and EX.is_clique_of_live(ok, ex_acc) and set(np.unique(ex_acc).tolist()) <= {0, 1}
        assert 0 < ex_rep["subproblems"] <= ex_rep["live"] and ex_rep["steps"] >= ex_rep["subproblems"]
        # the exact set resumed from the held set of the prefix (as _check of tests/test_gpu_exact_resume.py)
        acc = _guarded(b, N, np.uint8, POISON, head=held)
        er_rep = b.set_max_exact_resume(bits, first, acc)
        b.stream.synchronize()
        er_acc = _out(acc, N, POISON, "accepted")
        print(N, case_id, first, er_rep)
        assert er_rep["proven"] == 1 and er_rep["capped"] == 0
        assert er_rep["size"] == er_rep["upper_bound"] == ex.omega == er.size == int(er_acc.sum()) and EX.is_clique_of_live(ok, er_acc)
        assert er_rep["first"] == first and er_rep["size_before"] == er.w0 == int(held.sum())
        assert er_rep["live"] == er.live and er_rep["newcomers"] == er.newcomers and er_rep["multistart_size"] == er.lb
        assert er_rep["changed"] == int(ex.omega > er.w0) == int(er_acc.tobytes() != held.tobytes())
        assert er_rep["subproblems"] == er.roots and er_rep["steps"] >= er_rep["subproblems"]
        if ex.omega > max(er.w0, er.lb):
            assert er_rep["subproblems"] > 0
        elif ex.omega > er.w0:
            assert np.array_equal(er_acc, er.accepted)
        # the greedy, and the input
        acc = _guarded(b, N, np.uint8, POISON)
        b.set_max(bits, acc)
        b.stream.synchronize()
        greedy = _out(acc, N, POISON, "accepted")
        assert np.array_equal(greedy, MC.ref_set_max(ok, order))
        assert np.array_equal(bits.cpu().numpy().view(np.uint64).reshape(packed.shape), packed), "the input bits changed"
    return (ms_acc.tobytes(), ms_sizes.tobytes(), ex_acc.tobytes(), ex_rep, er_acc.tobytes(), er_rep, greedy.tobytes())


def test_workspaces_larger_than_the_list_of_the_moment():
    from ipc_amd.consensus import IPC, Config
    from ipc_amd.dist import EngineBackend
    V = max(int(MC.graph_for(MC.set_order(N)).loop_ids.max()) + 2 for N in set(VISITS))
    eng = IPC(MC.graph_for(MC.set_order(VISITS[0]), V=V), Config(), device=0)
    b = EngineBackend(eng)
    seen = {}
    try:
        for N in VISITS:
            got = _visit(eng, b, N)
            if N in seen:
                assert got == seen[N], "the second visit to N=%d differs from the first" % N
            seen[N] = got
    finally:
        eng.close()
