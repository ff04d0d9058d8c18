"""The multi-start and the exact set of every run of a batch on the GPU (ipc_set_max_batch_exact, ipc_run_batch_exact;
DESIGN.md 3.9).

1. The kernels on the injected batches of tests/batch_exact_cases.py: per run the references of tests/exact_cases.py AND, byte
   for byte and field for field, the single-matrix calls (ipc_set_max_exact, ipc_set_max) on an engine of that size; poison
   behind every output, the input unchanged, a second call, the runs in reversed order.
2. The step cap.  3. End to end against fresh engines' run_exact().  4. One launch sequence per chunk.  5. Errors and resources.
Every reference is a Python definition or an existing single-matrix call, never the new code.  No tolerances: the outputs are
integers and bytes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                        # (the child of the resource test: the case modules import the package)
    sys.path.insert(0, ROOT)

import batch_exact_cases as BX
import exact_cases as EX
import matrix_cases as MC
import multistart_cases as MS
import sweep_cases as SC

pytestmark = pytest.mark.gpu

POISON = 0xAA
DEFAULT = SC.PAIRS[0]
TIGHT = SC.PAIRS[3]                                               # (0.5, 1.0): pair cells reject, the sets differ
BATCH_ENV = ("IPC_BATCH_CHUNK", "IPC_BATCH_BUDGET")
vp = ctypes.c_void_p


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in SC.ENV_KEYS + BATCH_ENV + (MS.KNOB, EX.KNOB):
        monkeypatch.delenv(k, raising=False)


class _Engines:
    """One engine per (size, cap), as in tests/test_gpu_exact.py: the single-matrix references of one size share it."""

    def __init__(self):
        self.d = {}

    def get(self, N, cap=None):
        from ipc_amd.consensus import IPC, Config
        from ipc_amd.dist import EngineBackend
        if (N, cap) not in self.d:
            old = os.environ.get(EX.KNOB)
            if cap is not None:
                os.environ[EX.KNOB] = str(cap)
            try:
                eng = IPC(MC.graph_for(MC.set_order(N)), Config(), device=0)
            finally:
                if cap is not None:
                    if old is None:
                        del os.environ[EX.KNOB]
                    else:
                        os.environ[EX.KNOB] = old
            assert np.array_equal(eng.candidate_order(), MC.set_order(N))
            self.d[(N, cap)] = (eng, EngineBackend(eng))
        return self.d[(N, cap)]

    def close(self):
        for eng, _ in self.d.values():
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


_single = {}


def _single_matrix(engines, run_id, cap=None):
    """(accepted, report, greedy) of ipc_set_max_exact and ipc_set_max on an engine of the run's size: computed once, shared."""
    import torch
    if (run_id, cap) not in _single:
        N = BX.size(run_id)
        eng, b = engines.get(N, cap)
        with b.stream_ctx():
            bits = _to_device(b, MC.pack_rows(BX.matrix(run_id)))
            acc = torch.full((N + 64,), POISON, dtype=torch.uint8, device=b.device)
            greedy = torch.full((N + 64,), POISON, dtype=torch.uint8, device=b.device)
            rep = b.set_max_exact(bits, acc)
            b.set_max(bits, greedy)
        b.stream.synchronize()
        a, g = acc.cpu().numpy()[:N].copy(), greedy.cpu().numpy()[:N].copy()
        a.setflags(write=False), g.setflags(write=False)
        _single[(run_id, cap)] = (a, rep, g)
    return _single[(run_id, cap)]


def _batch(b, run_ids, greedy=True, multistart=True):
    """ipc_set_max_batch_exact on the batch, 64 poisoned bytes behind every output, the input compared afterwards.  Returns
    (per-run accepted, multistart, greedy, reports, batch-exact report)."""
    import torch
    run_n, order, words = BX.packed(run_ids)
    vec, _ = BX.offsets(run_n)
    total = int(vec[-1])
    with b.stream_ctx():
        bits = _to_device(b, words)
        outs = [torch.full((total + 64,), POISON, dtype=torch.uint8, device=b.device) for _ in range(3)]
        reps, bx = b.set_max_batch_exact(run_n, order, bits, outs[0], outs[1] if multistart else None, outs[2] if greedy else None)
    b.stream.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for k, used in enumerate((True, multistart, greedy)):
        assert (host[k][total:] == POISON).all(), "wrote behind output %d" % k
        if used:
            assert set(np.unique(host[k][:total]).tolist()) <= {0, 1}
        else:
            assert (host[k] == POISON).all()
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), words), "the input bits changed"
    cut = lambda a: [a[vec[r]:vec[r + 1]].copy() for r in range(len(run_ids))]
    return cut(host[0]), cut(host[1]), cut(host[2]), reps, bx


# ---- 1. injected batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_injected_batch_equals_references_and_single_matrix_calls(engines, name):
    ids = BX.BATCHES[name]
    _, b = engines.get(65)                                        # any engine serves: its own candidate list is not read
    acc, ms, greedy, reps, bx = _batch(b, ids)
    print(name, bx)
    for r, i in enumerate(ids):
        ok, ref_ms = BX.matrix(i), BX.multistart(i)
        print(i, reps[r])
        assert np.array_equal(ms[r], ref_ms.accepted), i
        assert int(acc[r].sum()) == BX.omega(i) and EX.is_clique_of_live(ok, acc[r]), i
        assert reps[r]["proven"] == 1 and reps[r]["size"] == reps[r]["upper_bound"] == BX.omega(i), i
        assert reps[r]["live"] == len(ref_ms.live) and reps[r]["multistart_size"] == int(ref_ms.accepted.sum()), i
        assert (reps[r]["subproblems"] > 0 or reps[r]["steps"] == 0) and (reps[r]["steps"] > 0) <= BX.searched(i), i
        a1, rep1, g1 = _single_matrix(engines, i)
        assert acc[r].tobytes() == a1.tobytes() and reps[r] == rep1, (i, reps[r], rep1)
        assert greedy[r].tobytes() == g1.tobytes(), i
        assert np.array_equal(greedy[r], MC.ref_set_max(ok, MC.set_order(BX.size(i)))), i
    n_searched = sum(BX.searched(i) for i in ids)
    assert bx == dict(runs=len(ids), chunks=1, searched_runs=n_searched, proven_runs=len(ids), set_launches=bx["set_launches"],
                      set_host_waits=2)
    # once more: identical
    acc2, ms2, greedy2, reps2, bx2 = _batch(b, ids)
    assert reps2 == reps and bx2 == bx
    assert all(x.tobytes() == y.tobytes() for x, y in zip(acc + ms + greedy, acc2 + ms2 + greedy2))
    # the runs in reversed order: a run's results depend neither on its neighbours nor on its offsets
    acc3, ms3, greedy3, reps3, bx3 = _batch(b, ids[::-1])
    assert reps3[::-1] == reps and bx3 == bx
    assert all(x.tobytes() == y.tobytes() for x, y in zip(acc + ms + greedy, acc3[::-1] + ms3[::-1] + greedy3[::-1]))


# ---- 2. the cap ------------------------------------------------------------------------------------------------------------
def test_step_cap_brackets_of_a_batch(engines):
    ids = BX.CAP_BATCH
    _, b = engines.get(65, cap=BX.CAP)                            # the cap is the serving engine's
    acc, ms, greedy, reps, bx = _batch(b, ids)
    by = dict(zip(ids, range(len(ids))))
    for i in ids:
        print(i, reps[by[i]])
    for i, sub, capped, lo, hi in (("planted-1025", 247, 247, 371, 414), ("decoys-129-40", 38, 30, 2, 41)):
        r = reps[by[i]]
        assert (r["subproblems"], r["capped"], r["size"], r["upper_bound"], r["proven"]) == (sub, capped, lo, hi, 0), (i, r)
        assert r["multistart_size"] == lo and hi == EX.colour_bound(i)
        assert BX.CAP * r["capped"] <= r["steps"] <= BX.CAP * r["subproblems"]
        assert np.array_equal(acc[by[i]], BX.multistart(i).accepted) and np.array_equal(ms[by[i]], BX.multistart(i).accepted)
    closed = ids[-1]
    r = reps[by[closed]]
    assert r["proven"] == 1 and r["steps"] == 0 and r["subproblems"] == 0 and r["size"] == r["upper_bound"] == BX.omega(closed)
    assert np.array_equal(acc[by[closed]], BX.multistart(closed).accepted)
    for i in ids:
        a1, rep1, g1 = _single_matrix(engines, i, cap=BX.CAP)
        assert acc[by[i]].tobytes() == a1.tobytes() and reps[by[i]] == rep1 and greedy[by[i]].tobytes() == g1.tobytes(), (i, rep1)
    assert bx["searched_runs"] == 2 and bx["proven_runs"] == 1


# ---- 3. end to end -------------------------------------------------------------------------------------------------------
def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def standard_runs(N):
    """The runs of tests/test_gpu_batch.py, restated: a shared head with each of three disjoint tails, the whole list, one single
    candidate, a stride-3 selection that starts at 1, and the first run once more."""
    head = np.arange(16)
    cut = [16, 16 + (N - 16) // 3, 16 + 2 * (N - 16) // 3, N]
    runs = [np.concatenate([head, np.arange(cut[q], cut[q + 1])]) for q in range(3)]
    runs += [np.arange(N), np.array([5]), np.arange(1, N, 3)]
    runs.append(runs[0].copy())
    return [_i32(r) for r in runs]


_fresh_exact = {}


def fresh_run_exact(name, g, members, pair):
    """(bits, accepted, multistart, report) of a fresh engine's run_exact() on the candidates `members` of g, in that order."""
    key = (name, tuple(int(k) for k in members), pair)
    if key not in _fresh_exact:
        eng = SC.engine(SC.stub(g, sel=_i32(members)), *pair)
        _fresh_exact[key] = eng.run_exact(want_bits=True)
        eng.close()
    return _fresh_exact[key]


@pytest.mark.parametrize("pair", [DEFAULT, TIGHT], ids=["default", "tight"])
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_run_batch_exact_end_to_end(monkeypatch, name, pair):
    g = SC.graph(name)
    assert g.N == (40 if name == "se2" else 36)
    runs = standard_runs(g.N)
    f, s = [p[0] for p in SC.PAIRS[:3]], [p[1] for p in SC.PAIRS[:3]]
    eng = SC.engine(g, *pair)
    r_bits, r_acc = eng.run()
    cns = eng.getMaxConsensusSet().copy()
    on_bits, on_acc, _ = eng.run_online(want_bits=True)
    sw_bits, sw_acc, sw_rep = eng.run_sweep(f, s, want_bits=True)
    assert sw_rep["reused_solve"] == 0
    bits, acc, ms, greedy, reps, brep, bx = eng.run_batch_exact(runs, want_bits=True)
    print(name, pair, brep, bx)
    for r, m in enumerate(runs):
        b_ref, a_ref, m_ref, rep_ref = fresh_run_exact(name, g, m, pair)
        assert bits[r].shape == b_ref.shape and bits[r].tobytes() == b_ref.tobytes(), r
        assert ms[r].tobytes() == m_ref.tobytes() and acc[r].tobytes() == a_ref.tobytes() and reps[r] == rep_ref, (r, reps[r], rep_ref)
    assert acc[6].tobytes() == acc[0].tobytes() and reps[6] == reps[0]                  # the repeated run
    assert bx["runs"] == brep["runs"] == len(runs) and bx["chunks"] == brep["chunks"] == 1
    assert bx["proven_runs"] == sum(r["proven"] for r in reps) and bx["set_host_waits"] <= 2 * bx["chunks"]
    assert bx["searched_runs"] >= sum(r["subproblems"] > 0 for r in reps)
    # the other calls around it: the consensus set, the online matrix, the held sweep, run()
    assert np.array_equal(eng.getMaxConsensusSet(), cns)
    sw_bits2, sw_acc2, sw_rep2 = eng.run_sweep(f, s, want_bits=True)
    assert sw_rep2["reused_solve"] == 1 and sw_bits2.tobytes() == sw_bits.tobytes() and sw_acc2.tobytes() == sw_acc.tobytes()
    on_bits2, on_acc2, on_rep2 = eng.run_online(want_bits=True)
    assert on_rep2["cells"] == 0 and on_bits2.tobytes() == on_bits.tobytes() and on_acc2.tobytes() == on_acc.tobytes()
    r_bits2, r_acc2 = eng.run()
    assert r_bits2.tobytes() == r_bits.tobytes() and r_acc2.tobytes() == r_acc.tobytes()
    # greedy and bits are run_batch()'s, on this engine and afterwards unchanged
    b_bits, b_acc, b_rep = eng.run_batch(runs, want_bits=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(bits + greedy, b_bits + b_acc))
    assert {k: brep[k] for k in brep if k != "chunks"} == {k: b_rep[k] for k in b_rep if k != "chunks"}
    eng.close()
    # chunks of two runs: the same outputs
    monkeypatch.setenv("IPC_BATCH_CHUNK", "2")
    eng = SC.engine(g, *pair)
    bits_c, acc_c, ms_c, greedy_c, reps_c, brep_c, bx_c = eng.run_batch_exact(runs, want_bits=True)
    eng.close()
    assert bx_c["chunks"] == brep_c["chunks"] >= 2 and bx_c["set_host_waits"] <= 2 * bx_c["chunks"]
    assert reps_c == reps and (bx_c["searched_runs"], bx_c["proven_runs"]) == (bx["searched_runs"], bx["proven_runs"])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(bits + acc + ms + greedy, bits_c + acc_c + ms_c + greedy_c))


def test_run_batch_exact_with_open_runs_in_several_chunks(monkeypatch):
    """The "wide" graph (200 candidates) at the (2.0, 4.0) pair: by the fresh engines' own reports three of these runs need the
    search and it beats the multi-start set in two -- in one chunk, and with the open runs spread over three chunks."""
    g = SC.graph("wide")
    pair = SC.PAIRS[2]
    N = g.N
    runs = [_i32(r) for r in (np.arange(N), np.arange(0, N, 2), np.arange(1, N, 3), np.arange(N // 2), np.arange(N // 3, N))]
    refs = [fresh_run_exact("wide", g, m, pair) for m in runs]
    open_runs = [r for r, ref in enumerate(refs) if ref[3]["subproblems"] > 0]
    assert len(open_runs) >= 3 and sum(ref[3]["size"] > ref[3]["multistart_size"] for ref in refs) >= 2, [ref[3] for ref in refs]
    assert len({r // 2 for r in open_runs}) >= 3                  # chunks of two runs: an open run in three of them
    for chunk in (None, "2"):
        if chunk:
            monkeypatch.setenv("IPC_BATCH_CHUNK", chunk)
        eng = SC.engine(g, *pair)
        bits, acc, ms, greedy, reps, brep, bx = eng.run_batch_exact(runs, want_bits=True)
        b_bits, b_acc, _ = eng.run_batch(runs, want_bits=True)
        eng.close()
        print(chunk, bx, reps)
        for r, (b_ref, a_ref, m_ref, rep_ref) in enumerate(refs):
            assert bits[r].tobytes() == b_ref.tobytes() and ms[r].tobytes() == m_ref.tobytes() and acc[r].tobytes() == a_ref.tobytes(), r
            assert reps[r] == rep_ref, (r, reps[r], rep_ref)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(bits + greedy, b_bits + b_acc))
        assert bx["chunks"] == (3 if chunk else 1) and bx["searched_runs"] >= len(open_runs) and bx["proven_runs"] == len(runs)
        assert bx["set_host_waits"] <= 2 * bx["chunks"]


# ---- 4. structure ----------------------------------------------------------------------------------------------------------
def test_one_launch_sequence_and_two_waits_per_chunk(engines):
    _, b = engines.get(65)
    seven = ["planted-64", "all_ones-65", "dead-2", "planted-128", "identity-63", "decoys-129-40", "far_conflict-129"]
    one = ["planted-128"]
    assert sum(BX.searched(i) for i in seven) == 3 and BX.searched(one[0])
    *_, bx7 = _batch(b, seven)
    *_, bx1 = _batch(b, one)
    print(bx7, bx1)
    assert bx7["chunks"] == bx1["chunks"] == 1
    assert bx7["set_launches"] == bx1["set_launches"] > 0         # not a sequence per run
    assert bx7["set_host_waits"] == bx1["set_host_waits"] == 2
    *_, bx0 = _batch(b, ["all_ones-65", "dead-2"])                # nothing to search: one wait, the search is not launched
    assert bx0["set_host_waits"] == 1 and bx0["set_launches"] < bx1["set_launches"] and bx0["searched_runs"] == 0
    *_, bxn = _batch(b, seven, greedy=False, multistart=False)    # the optional device outputs left out
    assert bxn["set_host_waits"] == 2 and bxn["set_launches"] <= bx7["set_launches"]


# ---- 5. errors and resources -------------------------------------------------------------------------------------------------
def _live(lib):
    out = (ctypes.c_int * 3)()
    assert lib.ipc_debug_live_resources(ctypes.byref(out)) == 0
    return list(out)


def test_argument_state_and_limit_errors(engines):
    import torch
    from ipc_amd import capi
    from ipc_amd.consensus import IPC, Config
    lib = capi.load()
    eng, b = engines.get(65)
    ids = ["all_ones-65", "planted-64"]
    run_n, order, words = BX.packed(ids)
    with b.stream_ctx():
        bits = _to_device(b, words)
        acc = torch.full((129 + 64,), POISON, dtype=torch.uint8, device=b.device)
    b.stream.synchronize()
    st = vp(b.stream.cuda_stream)

    def call(h, n, rn, od, bt, ac):
        p = lambda a: None if a is None else a.ctypes.data_as(vp)
        return lib.ipc_set_max_batch_exact(h, n, p(rn), p(od), None if bt is None else vp(bt.data_ptr()), None, None,
                                           None if ac is None else vp(ac.data_ptr()), None, None, st)

    assert call(None, 2, run_n, order, bits, acc) == -1 and b"NULL" in lib.ipc_last_error()              # IPC_ERR_ARG
    assert call(eng.h, 2, None, order, bits, acc) == -1 and b"NULL" in lib.ipc_last_error()
    assert call(eng.h, 2, run_n, None, bits, acc) == -1 and b"NULL" in lib.ipc_last_error()
    assert call(eng.h, 2, run_n, order, None, acc) == -1 and b"NULL" in lib.ipc_last_error()
    assert call(eng.h, 2, run_n, order, bits, None) == -1 and b"NULL" in lib.ipc_last_error()            # NULL d_accepted
    assert call(eng.h, 0, run_n, order, bits, acc) == -1 and b"runs" in lib.ipc_last_error()
    assert call(eng.h, 2, _i32([65, 0]), order, bits, acc) == -1 and b"candidates" in lib.ipc_last_error()
    bad = order.copy()
    bad[65 + 7] = bad[65 + 3]                                     # a repeated entry in the second slice
    assert call(eng.h, 2, run_n, bad, bits, acc) == -1 and b"permutation" in lib.ipc_last_error()
    bad = order.copy()
    bad[64] = 65                                                  # an entry outside 0 .. N_r - 1
    assert call(eng.h, 2, run_n, bad, bits, acc) == -1 and b"permutation" in lib.ipc_last_error()
    b.stream.synchronize()
    assert (acc.cpu().numpy() == POISON).all()                    # a refused call wrote nothing
    # a run of 8193: refused before anything is allocated
    before = _live(lib)
    big_order = np.arange(8193, dtype=np.int32)
    assert call(eng.h, 1, _i32([8193]), big_order, bits, acc) == -4 and b"8193" in lib.ipc_last_error()  # IPC_ERR_LIMIT
    assert call(eng.h, 2, _i32([65, 8193]), np.concatenate([order[:65], big_order]), bits, acc) == -4
    assert _live(lib) == before
    # every optional output NULL
    assert call(eng.h, 2, run_n, order, bits, acc) == 0
    b.stream.synchronize()
    out = acc.cpu().numpy()
    assert out[:65].all() and int(out[65:129].sum()) == BX.omega("planted-64") and (out[129:] == POISON).all()
    # ipc_run_batch_exact: the errors of ipc_run_batch, the limit, every output NULL
    g = SC.graph("se2")

    def run(e, n_runs, offsets, members):
        off, mem = _i32(offsets), _i32(members)
        return lib.ipc_run_batch_exact(e.h, n_runs, off.ctypes.data_as(vp), mem.ctypes.data_as(vp), None, None, None, None, None, None, None)

    empty = SC.engine(SC.stub(g, sel=[]))
    assert run(empty, 1, [0, 1], [0]) == -3 and b"no candidates" in lib.ipc_last_error()                # IPC_ERR_STATE
    empty.close()
    small = SC.engine(SC.stub(g, sel=SC.arrival(g)[:20]))
    assert run(small, 0, [0], [0]) == -1 and b"runs" in lib.ipc_last_error()
    assert run(small, 2, [0, 2, 2], [0, 1]) == -1 and b"empty" in lib.ipc_last_error()
    assert run(small, 1, [0, 3], [1, 4, 4]) == -1 and b"increasing" in lib.ipc_last_error()
    assert b"ipc_run_batch_exact" in lib.ipc_last_error()
    assert run(small, 2, [0, 2, 4], [1, 4, 2, 7]) == 0            # every output NULL
    small.close()
    big = IPC(MC.graph_for(np.arange(8193, dtype=np.int32)), Config(), device=0)
    before = _live(lib)
    assert run(big, 2, [0, 2, 8195], np.concatenate([[0, 1], np.arange(8193)])) == -4 and b"8193" in lib.ipc_last_error()
    assert _live(lib) == before
    big.close()


def _balance_child():
    """The device call twice, run_batch_exact twice, close: the second call at equal shapes allocates nothing and nothing stays
    behind.  In a process of its own, so that engines other test modules hold cannot move the process-wide counters."""
    sys.path.insert(0, ROOT)
    from ipc_amd import capi
    from ipc_amd.consensus import IPC, Config
    from ipc_amd.dist import EngineBackend
    lib = capi.load()
    assert _live(lib) == [0, 0, 0]
    eng = IPC(MC.graph_for(MC.set_order(65)), Config(), device=0)
    b = EngineBackend(eng)
    ids = ["decoys-129-40", "dead-2", "planted-64"]               # (two runs whose search runs: the stacks are allocated)
    mine = _live(lib)
    first = _batch(b, ids)
    held = _live(lib)
    assert held[0] > mine[0] and held[1] > mine[1], (mine, held)  # (the workspace and the pinned staging are counted)
    assert first[4]["searched_runs"] == 2 and first[3][0]["size"] == 40
    second = _batch(b, ids)
    assert _live(lib) == held, "the second call at equal shapes allocated"
    assert second[3] == first[3] and all(x.tobytes() == y.tobytes() for x, y in zip(first[0], second[0]))
    eng.close()
    del b
    import torch
    torch.cuda.synchronize()
    g = SC.graph("se2")
    eng = SC.engine(g)
    runs = standard_runs(g.N)
    one = eng.run_batch_exact(runs)
    after = _live(lib)
    two = eng.run_batch_exact(runs)
    assert _live(lib) == after, "the second run_batch_exact at equal shapes allocated"
    assert one[3] == two[3] and all(x.tobytes() == y.tobytes() for x, y in zip(one[0], two[0]))
    eng.close()
    assert _live(lib) == [0, 0, 0], "an engine's resources outlived it"
    print("batch exact resource balance OK: held %s" % held)


def test_batch_exact_releases_everything_it_acquired():
    user_site = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + user_site + [os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "batch exact resource balance OK" in r.stdout


if __name__ == "__main__":
    _balance_child()
