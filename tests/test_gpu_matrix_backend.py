"""The matrix back end on injected inputs: ipc_set_max and ipc_assemble_matrix are handed device arrays made by
tests/matrix_cases.py -- bit patterns the dog-leg never produces -- and held bit for bit against that module's plain
references; one test solves cells and holds the cell plan (k_plan) against the overlap rule.

Measured on an MI355X: the 158 cases of this file take 5 s together (7 s of wall time with the interpreter's start);
what they hold and what they do not is in DESIGN.md 4.2."""
import numpy as np
import pytest

import matrix_cases as MC

pytestmark = pytest.mark.gpu

POISON = 0xAA
SET_IDS = [c.id for c in MC.SET_CASES]


class _Engines:
    """One engine per (graph, row policy): the cases of one size share it, so a case also runs behind other
    matrices on the same engine."""

    def __init__(self):
        self.d = {}

    def get(self, key, make_graph, policy=None):
        import os
        from ipc_amd.consensus import IPC, Config
        from ipc_amd.dist import EngineBackend
        if (key, policy) not in self.d:
            old = os.environ.get("IPC_ROW_BALANCE")
            if policy is not None:
                os.environ["IPC_ROW_BALANCE"] = policy
            try:
                g = make_graph()
                eng = IPC(g, Config(), device=0)
            finally:
                if policy is not None:
                    if old is None:
                        del os.environ["IPC_ROW_BALANCE"]
                    else:
                        os.environ["IPC_ROW_BALANCE"] = old
            self.d[(key, policy)] = (g, eng, EngineBackend(eng))
        return self.d[(key, policy)]

    def close(self):
        for _, eng, _ in self.d.values():
            eng.close()
        self.d.clear()


@pytest.fixture(scope="module")
def engines():
    e = _Engines()
    yield e
    e.close()


def _to_device(b, words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64).reshape(-1)).to(b.device)


def _set_max(b, ok):
    """ipc_set_max on the packed matrix; accepted has 64 poisoned bytes behind N.  Returns (accepted [N], tail [64])."""
    import torch
    N = ok.shape[0]
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(ok))
        acc = torch.full((N + 64,), POISON, dtype=torch.uint8, device=b.device)
        b.set_max(bits, acc)
    b.stream.synchronize()
    out = acc.cpu().numpy()
    return out[:N].copy(), out[N:].copy()


@pytest.mark.parametrize("case", MC.SET_CASES, ids=SET_IDS)
def test_set_max_on_injected_matrices(oracle, engines, case):
    N = case.N
    order = MC.set_order(N)
    g, eng, b = engines.get(("set", N), lambda: MC.graph_for(order))
    assert np.array_equal(eng.candidate_order(), oracle.candidate_order(g.loop_ids))
    assert np.array_equal(eng.candidate_order(), order)
    ok = MC.set_matrix(case)
    ref = MC.ref_set_max(ok, order)
    exp = MC.set_expected(case, ok, order)
    if exp is not None:
        assert np.array_equal(ref, exp)
    other = MC.identity(N) if case.gen == "all_ones" else MC.all_ones(N)
    runs = [_set_max(b, ok), _set_max(b, ok), _set_max(b, other), _set_max(b, ok)]
    for k in (0, 1, 3):
        acc, tail = runs[k]
        wrong = np.flatnonzero(acc != ref)
        assert wrong.size == 0, ("run %d" % k, "candidates", wrong[:10], "positions",
                                 [int(np.flatnonzero(order == w)[0]) for w in wrong[:10]])
        assert (tail == POISON).all(), "run %d wrote behind accepted[N]" % k
    assert np.array_equal(runs[2][0], MC.ref_set_max(other, order))


def _slot_map(ids, world, policy):
    import ctypes as C
    from ipc_amd import capi
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    slot = np.zeros(len(ids), dtype=np.int32)
    capi.check(capi.load().ipc_row_assignment(len(ids), ids.ctypes.data_as(C.c_void_p), world,
                                              {"cyclic": 0, "cost": 1}[policy], slot.ctypes.data_as(C.c_void_p)))
    return slot


def _assemble(b, gathered, world, N, fill_seed):
    """ipc_assemble_matrix into a buffer pre-filled with random words; returns [N, words] uint64."""
    words = (N + 63) // 64
    fill = np.random.default_rng(fill_seed).integers(0, 2 ** 64, (N, words), dtype=np.uint64)
    with b.stream_ctx():
        d_g = _to_device(b, gathered)
        d_bits = _to_device(b, fill)
        b.assemble(d_g, world, d_bits)
    b.stream.synchronize()
    return d_bits, d_bits.cpu().numpy().view(np.uint64).reshape(N, words)


@pytest.mark.parametrize("policy", ["cyclic", "cost"])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("N", MC.ASSEMBLE_SIZES)
def test_assemble_on_injected_rows(oracle, engines, N, world, policy):
    case = MC.assemble_case(N)
    g, eng, b = engines.get(("asm", N), lambda: MC.graph_for(intervals=case.ids), policy)
    assert np.array_equal(eng.candidate_order(), oracle.candidate_order(g.loop_ids))
    slot = _slot_map(case.ids, world, policy)
    rpr = eng.rows_per_rank(world)
    assert rpr == (N + world - 1) // world
    assert len(set(slot.tolist())) == N and slot.min() >= 0 and slot.max() < world * rpr
    ref =MC.pack_rows(case.C)                                   # bits >= N of every row are zero
    outs = []
    for poison_seed in (11, 12):
        gathered = MC.gathered_rows(case.U, slot, world * rpr, poison_seed)
        _, got = _assemble(b, gathered, world, N, 20 + poison_seed)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, ("poison %d" % poison_seed, "first (row, word)", bad[:5].tolist())
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("N", MC.CHAIN_SIZES)
def test_assemble_then_set_max_equals_the_reference_chain(oracle, engines, N):
    import torch
    case = MC.assemble_case(N)
    g, eng, b = engines.get(("asm", N), lambda: MC.graph_for(intervals=case.ids), "cost")
    order = oracle.candidate_order(g.loop_ids)
    assert np.array_equal(eng.candidate_order(), order)
    ref = MC.ref_set_max(case.C, order)
    assert 2 <= int(ref.sum()) <= N - 2
    for world in (1, 3):
        slot = _slot_map(case.ids, world, "cost")
        gathered = MC.gathered_rows(case.U, slot, world * eng.rows_per_rank(world), 31)
        d_bits, _ = _assemble(b, gathered, world, N, 32)
        with b.stream_ctx():
            acc = torch.full((N + 64,), POISON, dtype=torch.uint8, device=b.device)
            b.set_max(d_bits, acc)
        b.stream.synchronize()
        out = acc.cpu().numpy()
        assert np.array_equal(out[:N], ref)
        assert (out[N:] == POISON).all()


def _cell_pairs(eng):
    c = eng.cell_info()
    return sorted(zip(c["i"].tolist(), c["j"].tolist()))


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("N", MC.PLAN_SIZES)
def test_plan_lists_every_cell_exactly_once(oracle, engines, N, world):
    from ipc_amd.consensus import unpack_bits
    g, eng, b = engines.get(("plan", N), lambda: MC.plan_graph(N))
    assert np.array_equal(eng.candidate_order(), oracle.candidate_order(g.loop_ids))
    expected = MC.expected_cells(g.loop_ids)
    if world == 1:
        bits, _ = eng.run()
        assert _cell_pairs(eng) == expected                      # (sorted lists: a cell listed twice would show)
        alive = np.diag(unpack_bits(bits, N)).astype(bool)
        shifted = np.zeros(N, dtype=bool)
        shifted[MC.plan_shifted(N)] = True
        assert np.array_equal(alive, ~shifted)
        _, n_set = eng.run_set_only()
        assert n_set == len(MC.expected_cells(g.loop_ids, alive))
        assert n_set < len(expected)
        return
    slot = _slot_map(g.loop_ids, world, "cost")
    rpr = eng.rows_per_rank(world)
    union = []
    for r in range(world):
        with b.stream_ctx():
            upper = b.empty_words(rpr * eng.words)
            b.solve_rows(r, world, upper)
        b.stream.synchronize()
        cells = _cell_pairs(eng)
        assert all(slot[i] // rpr == r for i, _ in cells)        # a row's cells are solved by the rank that owns the row
        union += cells
    assert sorted(union) == expected
