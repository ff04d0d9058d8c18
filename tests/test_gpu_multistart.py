"""Multi-start set maximisation on the GPU (ipc_set_max_multistart, ipc_run_multistart).

1. The kernels on injected matrices (the rig of tests/test_gpu_matrix_backend.py, restated): accepted and sizes bit for bit
   against the references of tests/multistart_cases.py, poison behind both outputs, repeated runs on one engine with another
   matrix in between, d_sizes = NULL, and ipc_set_max on the same device buffer afterwards.
2. Every kernel variant (IPC_MULTISTART_REG_WORDS) on the N = 129 and N = 4161 cases.
3. End to end on solved matrices: bits and the greedy set are run()'s, the other calls are not disturbed.
4. Errors and resources.
No tolerances anywhere: the outputs are integers.  IPC_ERR_LIMIT needs N > 491 520 and is not exercised."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                        # (the child of the resource test: the case modules import the package)
    sys.path.insert(0, ROOT)

import matrix_cases as MC
import multistart_cases as MS
import sweep_cases as SC

pytestmark = pytest.mark.gpu

POISON, POISON32 = 0xAA, 0x5A5A5A5A
vp = ctypes.c_void_p


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in SC.ENV_KEYS + (MS.KNOB,):
        monkeypatch.delenv(k, raising=False)


class _Engines:
    """One engine per (size, knob): the cases of one size share it, so a case also runs behind other matrices."""

    def __init__(self):
        self.d = {}

    def get(self, N, knob=None):
        from ipc_amd.consensus import IPC, Config
        from ipc_amd.dist import EngineBackend
        if (N, knob) not in self.d:
            old = os.environ.get(MS.KNOB)
            if knob is not None:
                os.environ[MS.KNOB] = str(knob)
            try:
                eng = IPC(MC.graph_for(MC.set_order(N)), Config(), device=0)
            finally:
                if knob is not None:
                    if old is None:
                        del os.environ[MS.KNOB]
                    else:
                        os.environ[MS.KNOB] = old
            assert np.array_equal(eng.candidate_order(), MC.set_order(N))
            self.d[(N, knob)] = (eng, EngineBackend(eng))
        return self.d[(N, knob)]

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


def _multistart(b, bits, N, want_sizes=True):
    """ipc_set_max_multistart on a device matrix; 64 poisoned bytes behind accepted[N], 64 poisoned int32 behind sizes[N].
    Returns (accepted [N], sizes [N] or None); asserts that the poison is intact."""
    import torch
    with b.stream_ctx():
        acc = torch.full((N + 64,), POISON, dtype=torch.uint8, device=b.device)
        sizes = torch.full((N + 64,), POISON32, dtype=torch.int32, device=b.device)
        b.set_max_multistart(bits, acc, sizes if want_sizes else None)
    b.stream.synchronize()
    a, s = acc.cpu().numpy(), sizes.cpu().numpy()
    assert (a[N:] == POISON).all(), "wrote behind accepted[N]"
    assert (s[N:] == POISON32).all(), "wrote behind sizes[N]"
    if not want_sizes:
        assert (s == POISON32).all(), "d_sizes = NULL, yet sizes were written"
    return a[:N].copy(), (s[:N].copy() if want_sizes else None)


def _check(case_id, got, order):
    acc, sizes = got
    ref = MS.reference(case_id)
    wrong = np.flatnonzero(acc != ref.accepted)
    assert wrong.size == 0, (case_id, "accepted differs at candidates", wrong[:10], "positions",
                             [int(np.flatnonzero(order == w)[0]) for w in wrong[:10]])
    if sizes is not None:
        wrong = np.flatnonzero(sizes != ref.sizes)
        assert wrong.size == 0, (case_id, "sizes differ at candidates", wrong[:10], sizes[wrong[:10]], ref.sizes[wrong[:10]])


# ---- 1. injected bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", MS.CASE_IDS)
def test_multistart_on_injected_matrices(engines, case_id):
    import torch
    N = MS.BY_ID[case_id].N
    order = MC.set_order(N)
    eng, b = engines.get(N)
    ok = MS.matrix(case_id)
    packed = MC.pack_rows(ok)
    other = MC.identity(N) if case_id.startswith("all_ones") else MC.all_ones(N)
    with b.stream_ctx():
        bits, bits_other = _to_device(b, packed), _to_device(b, MC.pack_rows(other))
    _check(case_id, _multistart(b, bits, N), order)
    _check(case_id, _multistart(b, bits, N), order)
    acc_o, sizes_o = _multistart(b, bits_other, N)               # another matrix in between: all_ones / identity, known by hand
    if case_id.startswith("all_ones"):
        assert acc_o.sum() == 1 and acc_o[order[0]] == 1 and (sizes_o == 1).all()
    else:
        assert acc_o.all() and (sizes_o == N).all()
    _check(case_id, _multistart(b, bits, N), order)
    _check(case_id, _multistart(b, bits, N, want_sizes=False), order)
    # the greedy on the same device buffer, and the buffer itself
    with b.stream_ctx():
        acc = torch.full((N + 64,), POISON, dtype=torch.uint8, device=b.device)
        b.set_max(bits, acc)
    b.stream.synchronize()
    out = acc.cpu().numpy()
    assert np.array_equal(out[:N], MC.ref_set_max(ok, order)) and (out[N:] == POISON).all()
    assert np.array_equal(bits.cpu().numpy().view(np.uint64).reshape(packed.shape), packed), "the input bits changed"


# ---- 2. every kernel variant -------------------------------------------------------------------------------------------
# words per lane: N = 129 -> 1, N = 4161 -> 2.  Knob 0: the LDS kernel at both; 1: registers (R = 1) at 129, LDS at 4161;
# 2 (the default): registers at both (R = 1, R = 2).
@pytest.mark.parametrize("N", [129, 4161])
@pytest.mark.parametrize("knob", [0, 1, 2])
def test_every_kernel_variant_gives_the_same_outputs(engines, knob, N):
    eng, b = engines.get(N, knob)
    order = MC.set_order(N)
    ids = [c.id for c in MS.CASES if c.N == N]
    assert len(ids) >= 6
    for case_id in ids:
        with b.stream_ctx():
            bits = _to_device(b, MC.pack_rows(MS.matrix(case_id)))
        _check(case_id, _multistart(b, bits, N), order)


# ---- 3. end to end -----------------------------------------------------------------------------------------------------
def _expected_report(ok, acc, greedy, ref):
    q = ref.best_q
    return dict(live=int(np.diag(ok).sum()), greedy_size=int(greedy.sum()), best_size=int(acc.sum()),
                best_seed=ref.live[q] if q >= 0 else -1, best_seed_position=q)


@pytest.mark.parametrize("name", ["se2", "se3"])
def test_run_multistart_end_to_end(name):
    from ipc_amd.consensus import unpack_bits
    g = SC.graph(name)
    pairs = SC.PAIRS[:3]
    f, s = [p[0] for p in pairs], [p[1] for p in pairs]
    b_ref, a_ref, _ = SC.fresh(("multistart", name), g, 6.251, 11.345)
    eng = SC.engine(g)
    order = eng.candidate_order()
    # a fresh engine: run_multistart first
    bits, acc, greedy, sizes, rep = eng.run_multistart(want_bits=True)
    assert eng.getMaxConsensusSet().size == 0
    assert bits.tobytes() == b_ref.tobytes() and greedy.tobytes() == a_ref.tobytes()
    ok = unpack_bits(bits, g.N).astype(bool)
    ref = MS.ref_multistart_plain(ok, order)
    assert np.array_equal(acc, ref.accepted) and np.array_equal(sizes, ref.sizes)
    assert sizes.dtype == np.int32 and acc.sum() >= greedy.sum() > 0
    assert rep == _expected_report(ok, acc, greedy, ref)
    # the other matrix calls, then run_multistart again, then the other calls again
    r_bits, r_acc = eng.run()
    cns = eng.getMaxConsensusSet().copy()
    on_bits, on_acc, _ = eng.run_online(want_bits=True)
    sw_bits, sw_acc, sw_rep = eng.run_sweep(f, s, want_bits=True)
    assert sw_rep["reused_solve"] == 0
    assert r_bits.tobytes() == b_ref.tobytes() and r_acc.tobytes() == a_ref.tobytes()
    acc2, greedy2, sizes2, rep2 = eng.run_multistart()
    assert acc2.tobytes() == acc.tobytes() and greedy2.tobytes() == r_acc.tobytes() and sizes2.tobytes() == sizes.tobytes()
    assert rep2 == rep
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


def test_argument_and_state_errors(engines):
    import torch
    from ipc_amd import capi
    lib = capi.load()
    eng, b = engines.get(65)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(MC.all_ones(65)))
        acc = torch.full((65 + 64,), POISON, dtype=torch.uint8, device=b.device)
    b.stream.synchronize()
    st = vp(b.stream.cuda_stream)
    assert lib.ipc_set_max_multistart(None, vp(bits.data_ptr()), vp(acc.data_ptr()), None, st) == -1       # IPC_ERR_ARG
    assert b"NULL" in lib.ipc_last_error()
    assert lib.ipc_set_max_multistart(eng.h, None, vp(acc.data_ptr()), None, st) == -1
    assert b"NULL" in lib.ipc_last_error()
    assert lib.ipc_set_max_multistart(eng.h, vp(bits.data_ptr()), None, None, st) == -1
    assert b"NULL" in lib.ipc_last_error()
    assert lib.ipc_run_multistart(None, None, None, None, None, None) == -1
    assert b"NULL" in lib.ipc_last_error()
    b.stream.synchronize()
    assert (acc.cpu().numpy() == POISON).all()                    # a refused call wrote nothing
    empty = SC.engine(SC.stub(SC.graph("se2"), sel=[]))
    assert lib.ipc_set_max_multistart(empty.h, vp(bits.data_ptr()), vp(acc.data_ptr()), None, None) == -3  # IPC_ERR_STATE
    assert b"no candidates" in lib.ipc_last_error()
    assert lib.ipc_run_multistart(empty.h, None, None, None, None, None) == -3
    assert b"no candidates" in lib.ipc_last_error()
    empty.close()
    assert lib.ipc_run_multistart(eng.h, None, None, None, None, None) == 0          # every output may be NULL


def _balance_child():
    """run_multistart twice, the device call twice, close: the second call at equal N allocates nothing and nothing stays
    behind.  In a process of its own, so that engines other test modules hold cannot move the process-wide counters."""
    sys.path.insert(0, ROOT)
    import torch
    from ipc_amd import capi
    from ipc_amd.dist import EngineBackend
    lib = capi.load()
    g = SC.graph("se2")
    assert _live(lib) == [0, 0, 0]
    eng = SC.engine(g)
    eng.run()
    eng.run()                                                     # (whatever the solve path acquires lazily is there now)
    before = _live(lib)
    first = eng.run_multistart()
    held = _live(lib)
    assert held[0] > before[0], (before, held)                    # (the workspace is counted)
    second = eng.run_multistart()
    assert _live(lib) == held, "the second call at equal N allocated"
    assert all(np.array_equal(x, y) for x, y in zip(first[:3], second[:3])) and first[3] == second[3]
    b = EngineBackend(eng)
    bits = np.zeros((g.N, eng.words), dtype=np.uint64)
    capi.check(lib.ipc_run(eng.h, bits.ctypes.data_as(vp), None))
    for _ in range(2):
        with b.stream_ctx():
            d_bits = torch.from_numpy(bits.view(np.int64).reshape(-1)).to(b.device)
            acc = b.empty_bytes(g.N)
            b.set_max_multistart(d_bits, acc)
        b.stream.synchronize()
        assert np.array_equal(acc.cpu().numpy(), first[0])
        assert _live(lib) == held
    eng.close()
    assert _live(lib) == [0, 0, 0], "an engine's resources outlived it"
    print("multistart resource balance OK: held %s" % held)


def test_multistart_releases_everything_it_acquired():
    user_site = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + user_site + [os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "multistart resource balance OK" in r.stdout


if __name__ == "__main__":
    _balance_child()
