"""Exact maximum consistent set on the GPU (ipc_set_max_exact, ipc_run_exact).

1. The kernels on injected matrices (the rig of tests/test_gpu_multistart.py, restated): proven, size and upper bound against
   the references of tests/exact_cases.py, the set a clique of live candidates, poison behind accepted, repeated runs on one
   engine with another matrix in between, and ipc_set_max on the same device buffer afterwards.
2. The step cap (IPC_EXACT_STEP_CAP=64): the bracket, the multi-start set, identical reports.
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


def _exact(b, bits, N):
    """ipc_set_max_exact on a device matrix, 64 poisoned bytes behind accepted[N].  Returns (accepted [N], report)."""
    import torch
    with b.stream_ctx():
        acc = torch.full((N + 64,), POISON, dtype=torch.uint8, device=b.device)
        rep = b.set_max_exact(bits, acc)
    b.stream.synchronize()
    a = acc.cpu().numpy()
    assert (a[N:] == POISON).all(), "wrote behind accepted[N]"
    assert set(np.unique(a[:N]).tolist()) <= {0, 1}
    return a[:N].copy(), rep


def _check_proven(case_id, got):
    acc, rep = got
    ok, ref, ms = EX.matrix(case_id), EX.reference(case_id), EX.multistart(case_id)
    lb = int(ms.accepted.sum())
    print(case_id, rep, "reference omega", ref.omega, "LB", lb)
    assert rep["proven"] == 1 and rep["capped"] == 0
    assert rep["size"] == rep["upper_bound"] == ref.omega
    assert rep["multistart_size"] == lb and rep["live"] == len(ms.live)
    assert int(acc.sum()) == ref.omega and EX.is_clique_of_live(ok, acc)
    assert 0 <= rep["subproblems"] <= rep["live"] and rep["steps"] >= rep["subproblems"]
    if ref.omega == lb:
        assert np.array_equal(acc, ms.accepted)


# ---- 1. injected bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", EX.CASE_IDS)
def test_exact_on_injected_matrices(engines, case_id):
    import torch
    N = EX.BY_ID[case_id].N
    order = MC.set_order(N)
    eng, b = engines.get(N)
    ok = EX.matrix(case_id)
    packed = MC.pack_rows(ok)
    all_ones = case_id.startswith("all_ones")
    other = MC.identity(N) if all_ones else MC.all_ones(N)
    with b.stream_ctx():
        bits, bits_other = _to_device(b, packed), _to_device(b, MC.pack_rows(other))
    first = _exact(b, bits, N)
    _check_proven(case_id, first)
    acc_o, rep_o = _exact(b, bits_other, N)                       # another matrix in between: all_ones / identity, known by hand
    want = 1 if all_ones else N
    assert rep_o["proven"] == 1 and rep_o["size"] == rep_o["upper_bound"] == rep_o["multistart_size"] == want
    assert (acc_o.sum() == 1 and acc_o[order[0]] == 1) if all_ones else acc_o.all()
    second = _exact(b, bits, N)
    assert second[0].tobytes() == first[0].tobytes() and second[1] == first[1], (first[1], second[1])
    # the greedy on the same device buffer, and the buffer itself
    with b.stream_ctx():
        acc = torch.full((N + 64,), POISON, dtype=torch.uint8, device=b.device)
        b.set_max(bits, acc)
    b.stream.synchronize()
    out = acc.cpu().numpy()
    assert np.array_equal(out[:N], MC.ref_set_max(ok, order)) and (out[N:] == POISON).all()
    assert np.array_equal(bits.cpu().numpy().view(np.uint64).reshape(packed.shape), packed), "the input bits changed"


# ---- 2. the cap ----------------------------------------------------------------------------------------------------------
def test_the_step_cap_gives_a_deterministic_bracket(engines):
    N, case_id = 1025, "planted-1025"
    eng, b = engines.get(N, cap=64)
    ok, ms = EX.matrix(case_id), EX.multistart(case_id)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(ok))
    acc, rep = _exact(b, bits, N)
    print(case_id, rep)
    lb = int(ms.accepted.sum())
    assert rep["proven"] == 0 and rep["capped"] > 0
    assert np.array_equal(acc, ms.accepted)
    assert rep["size"] == rep["multistart_size"] == lb
    assert rep["upper_bound"] == EX.colour_bound(case_id) > lb
    assert rep["capped"] <= rep["subproblems"] and 64 * rep["capped"] <= rep["steps"] <= 64 * rep["subproblems"]
    acc2, rep2 = _exact(b, bits, N)
    assert rep2 == rep and acc2.tobytes() == acc.tobytes()


def test_decoys_under_the_cap_is_proven_or_bracketed(engines):
    N, case_id = 129, "decoys-129-40"
    eng, b = engines.get(N, cap=64)
    ok = EX.matrix(case_id)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(ok))
    acc, rep = _exact(b, bits, N)
    print(case_id, rep)
    assert EX.is_clique_of_live(ok, acc) and int(acc.sum()) == rep["size"]
    assert (rep["proven"], rep["size"]) in ((1, 40), (0, 2))
    assert rep["size"] <= 40 <= rep["upper_bound"]
    if not rep["proven"]:
        assert rep["capped"] > 0 and rep["upper_bound"] == EX.colour_bound(case_id)
        assert np.array_equal(acc, EX.multistart(case_id).accepted)


# ---- 3. end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_run_exact_end_to_end(name):
    from ipc_amd.consensus import unpack_bits
    g = SC.graph(name)
    pairs = SC.PAIRS[:3]
    f, s = [p[0] for p in pairs], [p[1] for p in pairs]
    b_ref, a_ref, _ = SC.fresh(("exact", name), g, 6.251, 11.345)
    eng = SC.engine(g)
    order = eng.candidate_order()
    bits, acc, ms, rep = eng.run_exact(want_bits=True)            # a fresh engine: run_exact first
    assert eng.getMaxConsensusSet().size == 0
    assert bits.tobytes() == b_ref.tobytes()
    ok = unpack_bits(bits, g.N).astype(bool)
    ref = EX.ref_exact(ok, order, cap=5_000_000)
    assert ref.finished
    print(name, rep, "reference omega", ref.omega)
    assert rep["proven"] == 1 and rep["size"] == rep["upper_bound"] == ref.omega == int(acc.sum())
    assert EX.is_clique_of_live(ok, acc)
    ms_ref = MS.ref_multistart_plain(ok, order)
    assert np.array_equal(ms, ms_ref.accepted) and rep["multistart_size"] == int(ms.sum()) and rep["live"] == len(ms_ref.live)
    if ref.omega == rep["multistart_size"]:
        assert np.array_equal(acc, ms)
    # the other matrix calls, then run_exact again, then the other calls again
    r_bits, r_acc = eng.run()
    cns = eng.getMaxConsensusSet().copy()
    m_acc = eng.run_multistart()[0]
    assert m_acc.tobytes() == ms.tobytes()
    on_bits, on_acc, _ = eng.run_online(want_bits=True)
    sw_bits, sw_acc, sw_rep = eng.run_sweep(f, s, want_bits=True)
    assert sw_rep["reused_solve"] == 0
    assert r_bits.tobytes() == b_ref.tobytes() and r_acc.tobytes() == a_ref.tobytes()
    acc2, ms2, rep2 = eng.run_exact()
    assert acc2.tobytes() == acc.tobytes() and ms2.tobytes() == ms.tobytes() and rep2 == rep
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
    import torch
    from ipc_amd import capi
    from ipc_amd.consensus import IPC, Config
    lib = capi.load()
    eng, b = engines.get(65)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(MC.all_ones(65)))
        acc = torch.full((65 + 64,), POISON, dtype=torch.uint8, device=b.device)
    b.stream.synchronize()
    st = vp(b.stream.cuda_stream)
    assert lib.ipc_set_max_exact(None, vp(bits.data_ptr()), vp(acc.data_ptr()), None, st) == -1            # IPC_ERR_ARG
    assert b"NULL" in lib.ipc_last_error()
    assert lib.ipc_set_max_exact(eng.h, None, vp(acc.data_ptr()), None, st) == -1
    assert b"NULL" in lib.ipc_last_error()
    assert lib.ipc_set_max_exact(eng.h, vp(bits.data_ptr()), None, None, st) == -1
    assert b"NULL" in lib.ipc_last_error()
    assert lib.ipc_run_exact(None, None, None, None, None) == -1
    assert b"NULL" in lib.ipc_last_error()
    b.stream.synchronize()
    assert (acc.cpu().numpy() == POISON).all()                    # a refused call wrote nothing
    empty = SC.engine(SC.stub(SC.graph("se2"), sel=[]))
    assert lib.ipc_set_max_exact(empty.h, vp(bits.data_ptr()), vp(acc.data_ptr()), None, None) == -3       # IPC_ERR_STATE
    assert b"no candidates" in lib.ipc_last_error()
    assert lib.ipc_run_exact(empty.h, None, None, None, None) == -3
    assert b"no candidates" in lib.ipc_last_error()
    empty.close()
    assert lib.ipc_run_exact(eng.h, None, None, None, None) == 0                     # every output may be NULL
    assert lib.ipc_set_max_exact(eng.h, vp(bits.data_ptr()), vp(acc.data_ptr()), None, st) == 0            # report = NULL
    b.stream.synchronize()
    assert acc.cpu().numpy()[:65].all()
    # N = 8193: refused before anything is allocated
    big = IPC(MC.graph_for(np.arange(8193, dtype=np.int32)), Config(), device=0)
    before = _live(lib)
    assert lib.ipc_set_max_exact(big.h, vp(bits.data_ptr()), vp(acc.data_ptr()), None, None) == -4         # IPC_ERR_LIMIT
    assert b"8193" in lib.ipc_last_error()
    assert lib.ipc_run_exact(big.h, None, None, None, None) == -4
    assert _live(lib) == before
    big.close()


def _balance_child():
    """run_exact twice, the device call twice, close: the second call at equal N allocates nothing and nothing stays behind.
    In a process of its own, so that engines other test modules hold cannot move the process-wide counters."""
    sys.path.insert(0, ROOT)
    from ipc_amd import capi
    from ipc_amd.consensus import IPC, Config
    from ipc_amd.dist import EngineBackend
    lib = capi.load()
    assert _live(lib) == [0, 0, 0]
    N, case_id = 129, "decoys-129-40"                             # (a case whose search runs: the stacks are allocated)
    eng = IPC(MC.graph_for(MC.set_order(N)), Config(), device=0)
    b = EngineBackend(eng)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(EX.matrix(case_id)))
        acc = b.empty_bytes(N)
    b.stream.synchronize()
    mine = _live(lib)
    with b.stream_ctx():
        first = b.set_max_exact(bits, acc)
    a1 = acc.cpu().numpy().copy()
    held = _live(lib)
    assert held[0] > mine[0], (mine, held)                        # (the workspace is counted)
    assert first["subproblems"] > 0 and first["size"] == 40
    with b.stream_ctx():
        second = b.set_max_exact(bits, acc)
    assert _live(lib) == held, "the second call at equal N allocated"
    assert second == first and np.array_equal(acc.cpu().numpy(), a1)
    eng.run_exact()
    eng.run_exact()
    after = _live(lib)
    eng.run_exact()
    assert _live(lib) == after
    del bits, acc
    eng.close()
    assert _live(lib) == [0, 0, 0], "an engine's resources outlived it"
    print("exact resource balance OK: held %s" % held)


def test_exact_releases_everything_it_acquired():
    user_site = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + user_site + [os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "exact resource balance OK" in r.stdout


# ---- 5. both register variants -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id,per_lane", [("decoys-129-40", 1), ("hidden-4161", 2), ("decoys-4161-70", 2)])
def test_both_register_variants_run(engines, case_id, per_lane):
    """One word per lane up to N = 4096, two beyond: N = 129 runs k_ex_bound<1> / k_ex_search<1>, N = 4161 (66 words) the <2>
    kernels.  hidden-4161 is closed by the bound alone (LB = UB0); the decoys make the search itself run."""
    N = EX.BY_ID[case_id].N
    assert ((N + 63) // 64 + 63) // 64 == per_lane
    eng, b = engines.get(N)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(EX.matrix(case_id)))
    got = _exact(b, bits, N)
    _check_proven(case_id, got)
    if case_id.startswith("decoys"):
        assert got[1]["subproblems"] > 0 and got[1]["steps"] > 0


if __name__ == "__main__":
    _balance_child()
