"""Resumed exact set on the GPU (ipc_set_max_exact_resume, ipc_run_online_exact).

(a) every (case, split) of tests/exact_resume_cases.py on injected matrices (the rig of tests/test_gpu_exact.py, restated);
(b) chains of resumed calls; (c) the step cap; (d) invalid held sets and the N limit; (e) end to end in online matrix mode;
(f) resources; (g) both register variants.  No tolerances anywhere: the outputs are integers and bytes."""
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
import exact_resume_cases as ER
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


def _resume(b, bits, N, first, held):
    """ipc_set_max_exact_resume on a device matrix: accepted preloaded with `held` and 64 poisoned bytes behind it.  Returns
    (accepted [N], report)."""
    import torch
    buf = np.full(N + 64, POISON, dtype=np.uint8)
    buf[:N] = held
    with b.stream_ctx():
        acc = torch.from_numpy(buf).to(b.device)
        rep = b.set_max_exact_resume(bits, first, acc)
    b.stream.synchronize()
    a = acc.cpu().numpy()
    assert (a[N:] == POISON).all(), "wrote behind accepted[N]"
    assert set(np.unique(a[:N]).tolist()) <= {0, 1}
    return a[:N].copy(), rep


def _check(ok, ref, omega, held, got, first):
    acc, rep = got
    assert rep["proven"] == 1 and rep["capped"] == 0
    assert rep["size"] == rep["upper_bound"] == omega == int(acc.sum())
    assert EX.is_clique_of_live(ok, acc)
    assert rep["first"] == first and rep["size_before"] == ref.w0 == int(held.sum())
    assert rep["live"] == ref.live and rep["newcomers"] == ref.newcomers and rep["multistart_size"] == ref.lb
    assert rep["changed"] == int(omega > ref.w0) == int(acc.tobytes() != held.tobytes())
    if omega == ref.w0:
        assert acc.tobytes() == held.tobytes()
    assert rep["subproblems"] == ref.roots and rep["steps"] >= rep["subproblems"]
    if omega > max(ref.w0, ref.lb):
        assert rep["subproblems"] > 0
    elif omega > ref.w0:
        assert np.array_equal(acc, ref.accepted)                  # the multi-start set, byte for byte


# ---- (a) every (case, split) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id,first", ER.SPLITS, ids=ER.SPLIT_IDS)
def test_resume_on_injected_matrices(engines, case_id, first):
    N = EX.BY_ID[case_id].N
    eng, b = engines.get(N)
    ok, held, ref = EX.matrix(case_id), ER.held_set(case_id, first), ER.reference(case_id, first)
    packed = MC.pack_rows(ok)
    all_ones = case_id.startswith("all_ones")
    other = MC.identity(N) if all_ones else MC.all_ones(N)
    with b.stream_ctx():
        bits, bits_other = _to_device(b, packed), _to_device(b, MC.pack_rows(other))
    one = _resume(b, bits, N, first, held)
    print(case_id, first, one[1], "reference", ref.size, ref.w0, ref.lb)
    _check(ok, ref, EX.reference(case_id).omega, held, one, first)
    # another matrix in between (all_ones / identity, known by hand), resumed from nothing
    acc_o, rep_o = _resume(b, bits_other, N, 0, np.zeros(N, dtype=np.uint8))
    want = 1 if all_ones else N
    assert rep_o["proven"] == 1 and rep_o["size"] == rep_o["upper_bound"] == want == int(acc_o.sum())
    two = _resume(b, bits, N, first, held)
    assert two[0].tobytes() == one[0].tobytes() and two[1] == one[1], (one[1], two[1])
    assert np.array_equal(bits.cpu().numpy().view(np.uint64).reshape(packed.shape), packed), "the input bits changed"


# ---- (b) chains -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("burst", ER.CHAIN_BURSTS)
@pytest.mark.parametrize("case_id", ER.CHAIN_CASES)
def test_chains_on_the_device(engines, case_id, burst):
    N = EX.BY_ID[case_id].N
    eng, b = engines.get(N)
    ok, order = EX.matrix(case_id), MC.set_order(N)
    held, first, size = np.zeros(N, dtype=np.uint8), 0, 0
    for length in ER.chain_firsts(N, burst):
        sub = ER.prefix(ok, length)
        with b.stream_ctx():
            bits = _to_device(b, MC.pack_rows(sub))
        acc, rep = _resume(b, bits, N, first, held)
        assert rep["proven"] == 1 and rep["size"] == int(acc.sum()) and EX.is_clique_of_live(sub, acc)
        assert rep["size_before"] == size and rep["size"] >= size
        assert rep["changed"] == int(acc.tobytes() != held.tobytes()) and (rep["changed"] == 0 or rep["size"] > size)
        held, first, size = acc, length, rep["size"]
    assert size == EX.reference(case_id).omega


# ---- (c) the cap ----------------------------------------------------------------------------------------------------------
def test_the_step_cap_returns_the_incumbent_and_the_bracket(engines):
    N, case_id, first = 1025, "decoys-1025-300", 512
    eng, b = engines.get(N, cap=64)
    ok, held, ref = EX.matrix(case_id), ER.held_set(case_id, first), ER.reference(case_id, first)
    _, rows = EX._rows(ok, MC.set_order(N))
    live = [int(k) for k in MC.set_order(N) if ok[k][k]]
    new = sum(1 << a for a, k in enumerate(live) if k >= first)
    c = ER.colours_of(rows, new)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(ok))
    acc, rep = _resume(b, bits, N, first, held)
    print(case_id, first, rep)
    assert rep["proven"] == 0 and rep["capped"] > 0
    incumbent = held if ref.w0 >= ref.lb else EX.multistart(case_id).accepted
    assert acc.tobytes() == np.asarray(incumbent).tobytes()
    assert rep["size"] == max(ref.w0, ref.lb) and rep["upper_bound"] == min(len(live), ref.w0 + c)
    assert rep["size_before"] == ref.w0 and rep["multistart_size"] == ref.lb and rep["changed"] == int(ref.w0 < ref.lb)
    assert rep["capped"] <= rep["subproblems"] and 64 * rep["capped"] <= rep["steps"] <= 64 * rep["subproblems"]
    acc2, rep2 = _resume(b, bits, N, first, held)
    assert rep2 == rep and acc2.tobytes() == acc.tobytes()


# ---- (d) invalid held sets, the limit ---------------------------------------------------------------------------------------
def _live(lib):
    out = (ctypes.c_int * 3)()
    assert lib.ipc_debug_live_resources(ctypes.byref(out)) == 0
    return list(out)


def test_invalid_held_sets_and_the_limit(engines):
    import torch
    from ipc_amd import capi
    from ipc_amd.consensus import IPC, Config
    lib = capi.load()
    N, first = 129, 100
    eng, b = engines.get(N)
    ok = np.array(MC.all_ones(N), dtype=bool)
    ok[5, 5] = False                                              # a dead candidate
    ok[3, 4] = ok[4, 3] = False                                   # two live candidates that disagree
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(ok))
    st = vp(b.stream.cuda_stream)

    def call(members, byte=1):
        buf = np.full(N + 64, POISON, dtype=np.uint8)
        buf[:N] = 0
        buf[list(members)] = byte
        with b.stream_ctx():
            acc = torch.from_numpy(buf).to(b.device)
        b.stream.synchronize()
        rc = lib.ipc_set_max_exact_resume(eng.h, vp(bits.data_ptr()), first, vp(acc.data_ptr()), None, st)
        b.stream.synchronize()
        return rc, acc.cpu().numpy(), buf

    for members, byte in (((10, 120), 1), ((5, 10), 1), ((3, 4, 10), 1), ((10,), 2)):
        rc, after, before = call(members, byte)
        assert rc == -1 and b"ipc_set_max_exact_resume" in lib.ipc_last_error(), (members, byte)                # IPC_ERR_ARG
        assert after.tobytes() == before.tobytes(), "a refused call wrote"
    rc, after, before = call((3, 10, 20))                         # a valid clique of the prefix (not a maximum one: the claim is the caller's)
    assert rc == 0 and (after[N:] == POISON).all() and int(after[:N].sum()) == N - 2
    assert lib.ipc_set_max_exact_resume(eng.h, vp(bits.data_ptr()), -1, vp(bits.data_ptr()), None, st) == -1
    assert lib.ipc_set_max_exact_resume(eng.h, vp(bits.data_ptr()), N + 1, vp(bits.data_ptr()), None, st) == -1
    assert lib.ipc_set_max_exact_resume(eng.h, None, 0, vp(bits.data_ptr()), None, st) == -1
    assert lib.ipc_set_max_exact_resume(eng.h, vp(bits.data_ptr()), 0, None, None, st) == -1
    empty = SC.engine(SC.stub(SC.graph("se2"), sel=[]))
    assert lib.ipc_set_max_exact_resume(empty.h, vp(bits.data_ptr()), 0, vp(bits.data_ptr()), None, None) == -3   # IPC_ERR_STATE
    assert lib.ipc_run_online_exact(empty.h, None, None, None, None, None) == -3
    empty.close()
    # N = 8193: refused before anything is allocated, and before the update is made
    big = IPC(MC.graph_for(np.arange(8193, dtype=np.int32)), Config(), device=0)
    before = _live(lib)
    assert lib.ipc_set_max_exact_resume(big.h, vp(bits.data_ptr()), 0, vp(bits.data_ptr()), None, None) == -4     # IPC_ERR_LIMIT
    assert b"8193" in lib.ipc_last_error()
    assert lib.ipc_run_online_exact(big.h, None, None, None, None, None) == -4
    assert _live(lib) == before and big.online_covered == 0
    big.close()


# ---- (e) end to end in online matrix mode -----------------------------------------------------------------------------------
def _append(eng, g, ks):
    return [eng.append_candidate(g.loop_ids[k], g.loop_meas[k], g.loop_info[k]) for k in ks]


def _fresh_exact(g, sel):
    eng = SC.engine(SC.stub(g, sel=sel))
    acc, _, rep = eng.run_exact()
    eng.close()
    assert rep["proven"] == 1 and rep["size"] == int(acc.sum())
    return rep["size"]


@pytest.mark.parametrize("burst", [1, 7])
@pytest.mark.parametrize("name", ["se2", "se3", "wide"])
def test_online_exact_end_to_end(name, burst):
    from ipc_amd.consensus import unpack_bits
    g = SC.graph(name)
    arr = SC.arrival(g)
    eng, plain = SC.engine(SC.stub(g, sel=[])), SC.engine(SC.stub(g, sel=[]))
    assert eng.online_exact_state == (0, 0)
    held, size, n_resumed = np.zeros(0, dtype=np.uint8), 0, 0
    for q in range(0, len(arr), burst):
        ks = arr[q:q + burst]
        _append(eng, g, ks), _append(plain, g, ks)
        N = q + len(ks)
        bits, acc, greedy, on, rep = eng.run_online_exact(want_bits=True)
        p_bits, p_acc, p_on = plain.run_online(want_bits=True)
        assert bits.tobytes() == p_bits.tobytes() and greedy.tobytes() == p_acc.tobytes() and on == p_on
        assert rep["proven"] == 1 and rep["first"] == q and eng.online_exact_state == (N, 1)
        assert rep["size"] == int(acc.sum()) == _fresh_exact(g, arr[:N])
        assert EX.is_clique_of_live(unpack_bits(bits, N).astype(bool), acc)
        before = np.concatenate([held, np.zeros(N - held.shape[0], dtype=np.uint8)])
        grew = rep["size"] > size
        assert (acc.tobytes() != before.tobytes()) == grew, "the set changed without growing"
        if q:
            assert rep["changed"] == int(grew) and rep["size_before"] == size
            n_resumed += 1
        held, size = acc, rep["size"]
    assert n_resumed == (len(arr) - 1) // burst
    eng.close(), plain.close()


def test_online_exact_state_across_the_other_calls():
    """Plain run_online() calls in between keep the state and are caught up; append_odometry changes nothing; online_reset makes
    the next call a whole search."""
    full = SC.graph("se2")
    V0 = full.V - 3
    g = SC.stub(full, V=V0, sel=[k for k in range(full.N) if full.loop_ids[k].max() < V0])
    arr = SC.arrival(g)
    eng = SC.engine(SC.stub(g, sel=[]))
    covered, size, last = 0, 0, None
    for q, k in enumerate(arr):
        _append(eng, g, [k])
        if q % 3 != 2 and q != len(arr) - 1:
            eng.run_online()
            assert eng.online_exact_state == (covered, 1 if covered else 0)
            continue
        acc, greedy, on, rep = eng.run_online_exact()
        assert rep["first"] == covered and rep["proven"] == 1
        assert (on["covered_before"], on["covered_after"]) == (q, q + 1)                   # (run_online made the updates in between)
        assert rep["size"] == _fresh_exact(g, arr[:q + 1]) >= size
        covered, size, last = q + 1, rep["size"], (acc, rep)
        assert eng.online_exact_state == (covered, 1)
    assert eng.append_odometry(full.odom_meas[V0 - 1:], full.odom_info[V0 - 1:]) == full.V
    assert eng.online_exact_state == (covered, 1)
    acc, greedy, on, rep = eng.run_online_exact()
    assert acc.tobytes() == last[0].tobytes() and rep["first"] == covered and rep["newcomers"] == 0 and rep["changed"] == 0
    assert rep["size"] == rep["size_before"] == size and rep["steps"] == 0
    eng.online_reset()
    assert eng.online_exact_state == (0, 0)
    acc2, greedy2, on2, rep2 = eng.run_online_exact()
    assert rep2["first"] == 0 and rep2["proven"] == 1 and rep2["size"] == size and on2["covered_before"] == 0
    assert greedy2.tobytes() == greedy.tobytes() and EX.is_clique_of_live(_stored_matrix(eng), acc2)
    eng.set_candidates(g.loop_ids[arr[:5]], g.loop_meas[arr[:5]], g.loop_info[arr[:5]])
    assert eng.online_exact_state == (0, 0)
    acc3, _, _, rep3 = eng.run_online_exact()
    assert rep3["first"] == 0 and rep3["size"] == _fresh_exact(g, arr[:5]) == int(acc3.sum())
    eng.close()


def _stored_matrix(eng):
    from ipc_amd.consensus import unpack_bits
    bits, _, _ = eng.run_online(want_bits=True)                   # (nothing new: the stored matrix)
    return unpack_bits(bits, eng.N).astype(bool)


def test_an_unproven_call_is_followed_by_a_whole_search(monkeypatch):
    """IPC_EXACT_STEP_CAP=1: whenever a call returns proven = 0 the next one has first = 0.  (Whether any call is capped on these
    graphs is recorded in DESIGN.md 3.8; none is forced.)"""
    monkeypatch.setenv(EX.KNOB, "1")
    capped = 0
    for name in ("se2", "se3", "wide"):
        g = SC.graph(name)
        arr = SC.arrival(g)
        eng = SC.engine(SC.stub(g, sel=[]))
        proven, covered = 0, 0
        for q in range(0, len(arr), 7):
            _append(eng, g, arr[q:q + 7])
            acc, greedy, on, rep = eng.run_online_exact()
            assert rep["first"] == (covered if proven else 0)
            assert rep["proven"] == (1 if rep["capped"] == 0 else 0) and rep["size"] == int(acc.sum()) <= rep["upper_bound"]
            proven, covered = rep["proven"], eng.N
            assert eng.online_exact_state == (covered, proven)
            capped += rep["proven"] == 0
        eng.close()
    print("calls capped under IPC_EXACT_STEP_CAP=1:", capped)


# ---- (f) resources ----------------------------------------------------------------------------------------------------------
def _balance_child():
    """The device call twice, a stream of run_online_exact calls across a growth of the online storage, close: a second call at
    equal N allocates nothing and nothing stays behind.  In a process of its own (the counters are process-wide)."""
    sys.path.insert(0, ROOT)
    from ipc_amd import capi
    from ipc_amd.consensus import IPC, Config
    from ipc_amd.dist import EngineBackend
    lib = capi.load()
    assert _live(lib) == [0, 0, 0]
    N, case_id, first = 129, "decoys-129-40", 64                  # (a pair whose search runs: the stacks are allocated)
    eng = IPC(MC.graph_for(MC.set_order(N)), Config(), device=0)
    b = EngineBackend(eng)
    held = ER.held_set(case_id, first)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(EX.matrix(case_id)))
    b.stream.synchronize()
    mine = _live(lib)
    a1, r1 = _resume(b, bits, N, first, held)
    held_res = _live(lib)
    assert held_res[0] > mine[0] and r1["subproblems"] > 0 and r1["size"] == 40
    a2, r2 = _resume(b, bits, N, first, held)
    assert _live(lib) == held_res, "the second call at equal N allocated"
    assert r2 == r1 and a2.tobytes() == a1.tobytes()
    del bits
    eng.close()
    g = SC.graph("wide")
    arr = SC.arrival(g)
    on = SC.engine(SC.stub(g, sel=[]))
    grew = 0
    for q in range(0, 140, 10):
        _append(on, g, arr[q:q + 10])
        _, _, rep_on, rep = on.run_online_exact()
        grew += rep_on["grew"]
        assert rep["proven"] == 1
    assert grew >= 2                                              # (64 -> 128 -> 256: the held set moved with the matrix)
    after = _live(lib)
    on.run_online_exact()
    assert _live(lib) == after
    on.close()
    assert _live(lib) == [0, 0, 0], "an engine's resources outlived it"
    print("exact resume resource balance OK: held %s" % held_res)


def test_resume_releases_everything_it_acquired():
    user_site = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + user_site + [os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "exact resume resource balance OK" in r.stdout


# ---- (g) both register variants -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id,first,per_lane", [("decoys-129-40", 64, 1), ("decoys-4161-70", 2080, 2)])
def test_both_register_variants_run(engines, case_id, first, per_lane):
    """One word per lane up to N = 4096, two beyond: N = 129 runs the <1> kernels, N = 4161 (66 words) the <2> kernels; on both
    pairs the search itself runs and wins."""
    N = EX.BY_ID[case_id].N
    assert ((N + 63) // 64 + 63) // 64 == per_lane and (case_id, first) in ER.SPLITS
    eng, b = engines.get(N)
    ok, held, ref = EX.matrix(case_id), ER.held_set(case_id, first), ER.reference(case_id, first)
    with b.stream_ctx():
        bits = _to_device(b, MC.pack_rows(ok))
    got = _resume(b, bits, N, first, held)
    _check(ok, ref, EX.reference(case_id).omega, held, got, first)
    assert got[1]["subproblems"] > 0 and got[1]["steps"] > 0 and got[1]["size"] > max(ref.w0, ref.lb)


if __name__ == "__main__":
    _balance_child()
