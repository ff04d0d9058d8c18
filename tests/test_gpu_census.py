"""Census of the maximum consistent sets on the GPU (ipc_set_max_census, ipc_run_census).

1. The kernels on injected matrices (the rig of tests/test_gpu_exact.py, restated): count, core, support and subproblems against
   the references of tests/census_cases.py, accepted and the exact report against ipc_set_max_exact on the same engine, poison
   behind the three outputs, the input bits unchanged, a second call behind another matrix.
2. The step cap: a capped census gives the trivial bounds and a deterministic lower count; a capped exact stage gives no census.
3. End to end on solved matrices; the other calls are not disturbed.
4. Errors and resources.  5. Both register variants.
No tolerances anywhere: the outputs are integers."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                        # (the child of the resource test: the case modules import the package)
    sys.path.insert(0, ROOT)

import census_cases as CS
import exact_cases as EX
import matrix_cases as MC
import multistart_cases as MS
import sweep_cases as SC

pytestmark = pytest.mark.gpu

POISON = 0xAA
vp = ctypes.c_void_p


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in SC.ENV_KEYS + (MS.KNOB, EX.KNOB):
        monkeypatch.delenv(k, raising=False)


class _Engines:
    """One engine per (size, cap): the cases of one size share it, so a case also runs behind other matrices."""

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


def _poisoned(b, N):
    import torch
    return torch.full((N + 64,), POISON, dtype=torch.uint8, device=b.device)


def _bytes(t, N, what):
    a = t.cpu().numpy()
    assert (a[N:] == POISON).all(), "wrote behind %s[N]" % what
    assert set(np.unique(a[:N]).tolist()) <= {0, 1}, what
    return a[:N].copy()


def _census(b, bits, N):
    """ipc_set_max_census on a device matrix, 64 poisoned bytes behind each output.  Returns (accepted, core, support, exact
    report, census report)."""
    with b.stream_ctx():
        acc, core, support = _poisoned(b, N), _poisoned(b, N), _poisoned(b, N)
        ex, cs = b.set_max_census(bits, acc, core, support)
    b.stream.synchronize()
    return _bytes(acc, N, "accepted"), _bytes(core, N, "core"), _bytes(support, N, "support"), ex, cs


def _exact(b, bits, N):
    with b.stream_ctx():
        acc = _poisoned(b, N)
        rep = b.set_max_exact(bits, acc)
    b.stream.synchronize()
    return _bytes(acc, N, "accepted"), rep


def _same(x, y):
    return all(p.tobytes() == q.tobytes() for p, q in zip(x[:3], y[:3])) and x[3] == y[3] and x[4] == y[4]


def _check_proven(case_id, got):
    acc, core, support, ex, cs = got
    ok = EX.matrix(case_id)
    omega, count, core_ref, support_ref, sub = CS.reference(case_id)
    n = len(EX.multistart(case_id).live)
    print(case_id, ex, cs, "reference", omega, count, int(core_ref.sum()), int(support_ref.sum()), sub)
    assert ex["proven"] == 1 and cs["exact_proven"] == 1 and cs["proven"] == 1 and cs["capped"] == 0
    assert cs["live"] == ex["live"] == n and cs["size"] == ex["size"] == omega == int(acc.sum())
    assert cs["count"] == count and cs["subproblems"] == sub
    assert np.array_equal(core, core_ref) and np.array_equal(support, support_ref)
    assert cs["core_size"] == int(core.sum()) and cs["support_size"] == int(support.sum())
    assert EX.is_clique_of_live(ok, acc)
    CS.check_invariants(ok, acc, core, support, cs["count"], cs["size"])
    assert cs["steps"] >= 0 and (cs["steps"] == 0) == (omega <= 1)
    assert cs["count"] <= max(cs["steps"], cs["subproblems"], 1)


def _check_trivial_bounds(case_id, got):
    acc, core, support, ex, cs = got
    ok = EX.matrix(case_id)
    assert not core.any() and np.array_equal(support.astype(bool), ok.diagonal())
    assert cs["core_size"] == 0 and cs["support_size"] == cs["live"] == int(ok.diagonal().sum())


# ---- 1. injected bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", CS.CASE_IDS)
def test_census_on_injected_matrices(engines, case_id):
    N = EX.BY_ID[case_id].N
    eng, b = engines.get(N)
    ok = EX.matrix(case_id)
    packed = MC.pack_rows(ok)
    # another matrix in between, known by hand: all_ones (one maximum set: everybody), or identity (N maximum sets of one) behind
    # all_ones itself and at N = 4161, where the one root of all_ones would take N^2 / 2 steps, beyond the default cap
    lonely = case_id.startswith("all_ones") or N > 1025
    other = MC.identity(N) if lonely else MC.all_ones(N)
    with b.stream_ctx():
        bits, bits_other = _to_device(b, packed), _to_device(b, MC.pack_rows(other))
    first = _census(b, bits, N)
    _check_proven(case_id, first)
    acc_x, rep_x = _exact(b, bits, N)                             # the exact call on the same engine and matrix: steps included
    assert acc_x.tobytes() == first[0].tobytes() and rep_x == first[3], (rep_x, first[3])
    o = _census(b, bits_other, N)
    assert o[4]["proven"] == 1 and o[4]["count"] == (N if lonely else 1) and o[4]["size"] == (1 if lonely else N), o[4]
    assert o[2].all() and bool(o[1].all()) == (not lonely or N == 1)
    second = _census(b, bits, N)
    assert _same(first, second), (first[3:], second[3:])
    assert np.array_equal(bits.cpu().numpy().view(np.uint64).reshape(packed.shape), packed), "the input bits changed"


# ---- 2. the cap ----------------------------------------------------------------------------------------------------------
def test_a_capped_census_gives_the_trivial_bounds_and_a_deterministic_count(engines):
    N, case_id = EX.BY_ID[CS.CAP_CASE].N, CS.CAP_CASE
    eng, b = engines.get(N, cap=CS.CAP)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(EX.matrix(case_id)))
    got = _census(b, bits, N)
    acc, core, support, ex, cs = got
    print(case_id, ex, cs)
    assert ex["proven"] == 1 and ex["subproblems"] == 0 and ex["size"] == 64          # closed by LB = UB0: no search, whatever the cap
    assert cs["exact_proven"] == 1 and cs["size"] == 64 and int(acc.sum()) == 64
    assert cs["proven"] == 0 and 1 <= cs["capped"] <= cs["subproblems"] <= cs["live"] == 128
    assert 0 <= cs["count"] <= cs["steps"] and CS.CAP * cs["capped"] <= cs["steps"] <= CS.CAP * cs["subproblems"]
    _check_trivial_bounds(case_id, got)
    again = _census(b, bits, N)
    assert _same(got, again), (got[3:], again[3:])


def test_a_capped_exact_stage_gives_no_census(engines):
    N, case_id = EX.BY_ID[CS.EXACT_CAPPED_CASE].N, CS.EXACT_CAPPED_CASE
    eng, b = engines.get(N, cap=CS.EXACT_CAP)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(EX.matrix(case_id)))
    got = _census(b, bits, N)
    acc, core, support, ex, cs = got
    print(case_id, ex, cs)
    acc_x, rep_x = _exact(b, bits, N)
    assert acc_x.tobytes() == acc.tobytes() and rep_x == ex
    assert ex["proven"] == 0 and cs["exact_proven"] == 0 and cs["proven"] == 0
    assert cs["size"] == ex["size"] == ex["multistart_size"] == int(acc.sum())
    assert cs["count"] == 0 and cs["steps"] == 0 and cs["subproblems"] == 0 and cs["capped"] == 0
    _check_trivial_bounds(case_id, got)


# ---- 3. end to end -----------------------------------------------------------------------------------------------------
_fresh_exact = {}


def _fresh_run_exact(name, g, pair):
    if (name, pair) not in _fresh_exact:
        eng = SC.engine(g, *pair)
        _fresh_exact[(name, pair)] = eng.run_exact(want_bits=True)
        eng.close()
    return _fresh_exact[(name, pair)]


@pytest.mark.parametrize("name,pair", [("se2", SC.PAIRS[0]), ("se2", SC.PAIRS[3]), ("se3", SC.PAIRS[0]), ("se3", SC.PAIRS[3]),
                                       ("wide", SC.PAIRS[2])], ids=["se2-default", "se2-tight", "se3-default", "se3-tight", "wide"])
def test_run_census_end_to_end(name, pair):
    from ipc_amd.consensus import unpack_bits
    g = SC.graph(name)
    f, s = [p[0] for p in SC.PAIRS[:3]], [p[1] for p in SC.PAIRS[:3]]
    b_ref, a_ref, _, rep_ref = _fresh_run_exact(name, g, pair)
    if name == "wide":
        assert rep_ref["subproblems"] > 0                         # the exact stage needs its search here
    eng = SC.engine(g, *pair)
    order = eng.candidate_order()
    bits, acc, core, support, ex, cs = eng.run_census(want_bits=True)          # a fresh engine: run_census first
    assert eng.getMaxConsensusSet().size == 0
    assert bits.tobytes() == b_ref.tobytes() and acc.tobytes() == a_ref.tobytes() and ex == rep_ref, (ex, rep_ref)
    ok = unpack_bits(bits, g.N).astype(bool)
    assert ex["proven"] == 1 and cs["exact_proven"] == 1 and cs["proven"] == 1 and cs["size"] == ex["size"]
    count, core_ref, support_ref, sub = CS.ref_census(ok, order, ex["size"])
    print(name, pair, ex, cs, "reference", count, int(core_ref.sum()), int(support_ref.sum()), sub)
    assert cs["count"] == count and cs["subproblems"] == sub
    assert np.array_equal(core, core_ref) and np.array_equal(support, support_ref)
    assert cs["core_size"] == int(core.sum()) and cs["support_size"] == int(support.sum()) and cs["live"] == int(ok.diagonal().sum())
    CS.check_invariants(ok, acc, core, support, cs["count"], cs["size"])
    # the other matrix calls, then run_census again, then the other calls again
    r_bits, r_acc = eng.run()
    cns = eng.getMaxConsensusSet().copy()
    on_bits, on_acc, _ = eng.run_online(want_bits=True)
    sw_bits, sw_acc, sw_rep = eng.run_sweep(f, s, want_bits=True)
    assert sw_rep["reused_solve"] == 0
    again = eng.run_census()
    assert again[0].tobytes() == acc.tobytes() and again[1].tobytes() == core.tobytes() and again[2].tobytes() == support.tobytes()
    assert again[3] == ex and again[4] == cs
    assert np.array_equal(eng.getMaxConsensusSet(), cns)
    sw_bits2, sw_acc2, sw_rep2 = eng.run_sweep(f, s, want_bits=True)
    assert sw_rep2["reused_solve"] == 1
    assert sw_bits2.tobytes() == sw_bits.tobytes() and sw_acc2.tobytes() == sw_acc.tobytes()
    on_bits2, on_acc2, on_rep2 = eng.run_online(want_bits=True)
    assert on_rep2["cells"] == 0                                   # the online matrix still covers every candidate
    assert on_bits2.tobytes() == on_bits.tobytes() and on_acc2.tobytes() == on_acc.tobytes()
    r_bits2, r_acc2 = eng.run()
    assert r_bits2.tobytes() == r_bits.tobytes() and r_acc2.tobytes() == r_acc.tobytes()
    eng.close()


# ---- 4. errors and resources -------------------------------------------------------------------------------------------
def _live(lib):
    out = (ctypes.c_int * 3)()
    assert lib.ipc_debug_live_resources(ctypes.byref(out)) == 0
    return list(out)


def test_argument_state_and_limit_errors(engines):
    from ipc_amd import capi
    from ipc_amd.consensus import IPC, Config
    lib = capi.load()
    N = 65
    eng, b = engines.get(N)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(MC.all_ones(N)))
        outs = [_poisoned(b, N) for _ in range(3)]
    b.stream.synchronize()
    st = vp(b.stream.cuda_stream)
    good = [eng.h, vp(bits.data_ptr())] + [vp(t.data_ptr()) for t in outs]
    for k in range(5):                                            # each NULL pointer: IPC_ERR_ARG, nothing written
        args = list(good)
        args[k] = None
        assert lib.ipc_set_max_census(*args, None, None, st) == -1
        assert b"ipc_set_max_census: NULL" in lib.ipc_last_error()
    assert lib.ipc_run_census(None, None, None, None, None, None, None) == -1
    assert b"NULL" in lib.ipc_last_error()
    b.stream.synchronize()
    for t in outs:
        assert (t.cpu().numpy() == POISON).all()                  # a refused call wrote nothing
    empty = SC.engine(SC.stub(SC.graph("se2"), sel=[]))
    assert lib.ipc_set_max_census(empty.h, *good[1:], None, None, None) == -3                              # IPC_ERR_STATE
    assert b"no candidates" in lib.ipc_last_error()
    assert lib.ipc_run_census(empty.h, None, None, None, None, None, None) == -3
    assert b"no candidates" in lib.ipc_last_error()
    empty.close()
    assert lib.ipc_run_census(eng.h, None, None, None, None, None, None) == 0        # every output may be NULL
    assert lib.ipc_set_max_census(*good, None, None, st) == 0                         # both reports NULL
    b.stream.synchronize()
    for t in outs:
        a = t.cpu().numpy()
        assert a[:N].all() and (a[N:] == POISON).all()            # all ones: one maximum set, everybody
    big = IPC(MC.graph_for(np.arange(8193, dtype=np.int32)), Config(), device=0)     # N = 8193: refused before anything is allocated
    before = _live(lib)
    assert lib.ipc_set_max_census(big.h, *good[1:], None, None, None) == -4                                # IPC_ERR_LIMIT
    assert b"8193" in lib.ipc_last_error()
    assert lib.ipc_run_census(big.h, None, None, None, None, None, None) == -4
    assert _live(lib) == before
    big.close()


def _balance_child():
    """The device call twice, run_census three times, close: the second call at equal N allocates nothing and nothing stays
    behind.  In a process of its own, so that engines other test modules hold cannot move the process-wide counters."""
    sys.path.insert(0, ROOT)
    from ipc_amd import capi
    from ipc_amd.consensus import IPC, Config
    from ipc_amd.dist import EngineBackend
    lib = capi.load()
    assert _live(lib) == [0, 0, 0]
    N, case_id = 129, "planted-129"                               # (a case whose census search runs: the stacks are allocated)
    eng = IPC(MC.graph_for(MC.set_order(N)), Config(), device=0)
    b = EngineBackend(eng)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(EX.matrix(case_id)))
        acc, core, support = b.empty_bytes(N), b.empty_bytes(N), b.empty_bytes(N)
    b.stream.synchronize()
    mine = _live(lib)
    with b.stream_ctx():
        first = b.set_max_census(bits, acc, core, support)
    out1 = [t.cpu().numpy().copy() for t in (acc, core, support)]
    held = _live(lib)
    assert held[0] > mine[0], (mine, held)                        # (the workspace is counted)
    assert first[1]["subproblems"] > 0 and first[1]["count"] == 16 and first[1]["proven"] == 1
    with b.stream_ctx():
        second = b.set_max_census(bits, acc, core, support)
    assert _live(lib) == held, "the second call at equal N allocated"
    assert second == first and all(np.array_equal(t.cpu().numpy(), o) for t, o in zip((acc, core, support), out1))
    eng.run_census()
    eng.run_census()
    after = _live(lib)
    eng.run_census()
    assert _live(lib) == after
    del bits, acc, core, support
    eng.close()
    assert _live(lib) == [0, 0, 0], "an engine's resources outlived it"
    print("census resource balance OK: held %s" % held)


def test_census_releases_everything_it_acquired():
    user_site = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + user_site + [os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "census resource balance OK" in r.stdout


# ---- 5. both register variants -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id,per_lane", [("planted-129", 1), ("nlive_exact-4161-65", 2), ("hidden-4161", 2)])
def test_both_register_variants_run(engines, case_id, per_lane):
    """One word per lane up to N = 4096, two beyond: N = 129 runs k_cs_search<1>, N = 4161 (66 words) k_cs_search<2>.  Each of
    these cases makes the census search itself run, and the first two meet several maximum sets."""
    N = EX.BY_ID[case_id].N
    assert ((N + 63) // 64 + 63) // 64 == per_lane
    eng, b = engines.get(N)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(EX.matrix(case_id)))
    got = _census(b, bits, N)
    _check_proven(case_id, got)
    assert got[4]["subproblems"] > 0 and got[4]["steps"] > 0
    if not case_id.startswith("hidden"):
        assert got[4]["count"] > 1


if __name__ == "__main__":
    _balance_child()
