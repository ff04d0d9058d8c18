"""Monte-Carlo batch on the GPU (ipc_run_batch): the cells that some run needs are solved once, in the indices of the union list,
and assembled into every run's own matrix and consistent set; every run must be, BIT FOR BIT, what run() gives on a fresh engine
that was handed the run's members as its candidate list.  No tolerances: one would hide a bit at the union's index instead of
the local one, a stride of another run, or a set-max that read a neighbour's matrix.

Every reference is a fresh engine and the existing run() (tests/sweep_cases.py), never the batch itself."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import sweep_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = SC.PAIRS[0]
TIGHT = SC.PAIRS[3]                                           # (0.5, 1.0): pair cells reject, the greedy has verdicts to take
BATCH_ENV = ("IPC_BATCH_CHUNK", "IPC_BATCH_BUDGET")
vp = ctypes.c_void_p


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in SC.ENV_KEYS + BATCH_ENV:
        monkeypatch.delenv(k, raising=False)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def fresh_run(key, g, members, pair=DEFAULT):
    """(bits, accepted, solve report) of a fresh engine's run() on the candidates `members` of g, in that order."""
    m = _i32(members)
    return SC.fresh((key, tuple(int(k) for k in m)), SC.stub(g, sel=m), *pair)


def assert_batch_equals_fresh(key, g, runs, bits, accs, pair=DEFAULT):
    assert len(accs) == len(runs)
    for r, m in enumerate(runs):
        b_ref, a_ref, _ = fresh_run(key, g, m, pair)
        assert accs[r].shape == (len(m),) and accs[r].tobytes() == a_ref.tobytes(), (key, r)
        if bits is not None:
            assert bits[r].shape == b_ref.shape and bits[r].tobytes() == b_ref.tobytes(), (key, r)


def standard_runs(N):
    """A shared head with each of three disjoint tails, the whole list, one single candidate, a stride-3 selection that starts
    at 1, and the first run once more."""
    head = np.arange(16)
    cut = [16, 16 + (N - 16) // 3, 16 + 2 * (N - 16) // 3, N]
    runs = [np.concatenate([head, np.arange(cut[q], cut[q + 1])]) for q in range(3)]
    runs += [np.arange(N), np.array([5]), np.arange(1, N, 3)]
    runs.append(runs[0].copy())
    return [_i32(r) for r in runs]


def together(N, runs):
    """[N, N] bool: some run holds both candidates."""
    memb = np.zeros((len(runs), N), dtype=bool)
    for r, m in enumerate(runs):
        memb[r, m] = True
    return (memb.astype(np.int64).T @ memb.astype(np.int64)) > 0, memb


def overlap(g):
    """[N, N] bool: the id intervals overlap with positive length (reference src/consensus.cpp:157-159)."""
    lo, hi = g.loop_ids.min(axis=1), g.loop_ids.max(axis=1)
    return (np.minimum(hi[:, None], hi[None, :]) - np.maximum(lo[:, None], lo[None, :])) > 0


# ---- 1. equality, both dimensions, with and without the literal loop on shared cells ------------------------------------
def _aimed_pair(name, g):
    """A threshold pair that puts SHARED cells inside a borderline band of 0.05: the median max chi2 of the diagonal cells and of
    the pair cells among the head 0..15 (which three of the standard runs hold), each divided by 1.03.  The chi2 are those of a
    fresh engine's run() with the band off."""
    os.environ["IPC_BORDERLINE_BAND"] = "0"
    try:
        eng = SC.engine(g)
        eng.run()
        cells = eng.cell_info().copy()
        eng.close()
    finally:
        del os.environ["IPC_BORDERLINE_BAND"]
    x = cells["max_chi2"]
    usable = np.isfinite(x) & (x > 1e-3) & ((cells["flags"] & 2) == 0) & (cells["i"] < 16) & (cells["j"] < 16)
    xd, xp = np.sort(x[usable & (cells["i"] == cells["j"])]), np.sort(x[usable & (cells["i"] != cells["j"])])
    assert len(xd) >= 3 and len(xp) >= 3, name
    return float(xd[len(xd) // 2]) / 1.03, float(xp[len(xp) // 2]) / 1.03


@pytest.mark.parametrize("name,pair,band", [("se2", DEFAULT, None), ("se3", DEFAULT, None), ("se2", TIGHT, None),
                                            ("se2", "aimed", "0.05"), ("se3", "aimed", "0.05")],
                         ids=["se2", "se3", "se2-tight", "se2-band-0.05", "se3-band-0.05"])
def test_every_run_is_the_fresh_engines_run(monkeypatch, name, pair, band):
    g = SC.graph(name)
    assert g.N == (40 if name == "se2" else 36)
    if pair == "aimed":
        pair = _aimed_pair(name, g)
    if band is not None:
        monkeypatch.setenv("IPC_BORDERLINE_BAND", band)
    runs = standard_runs(g.N)
    eng = SC.engine(g, *pair)
    bits, accs, rep = eng.run_batch(runs, want_bits=True)
    print("report", name, pair, band, rep)
    assert_batch_equals_fresh(name, g, runs, bits, accs, pair)
    full = np.zeros((len(runs), g.N), dtype=np.uint8)         # the accepted sets in union indices
    for r, m in enumerate(runs):
        full[r, m] = accs[r]
    assert len({f.tobytes() for f in full}) >= 3              # not vacuous: the set does change with the run
    assert accs[6].tobytes() == accs[0].tobytes() and bits[6].tobytes() == bits[0].tobytes()      # the repeated run
    assert rep["runs"] == len(runs) and rep["union_candidates"] == g.N and rep["chunks"] == 1
    whole = fresh_run(name, g, runs[3], pair)[2]              # the whole list is a run: every cell is needed
    assert rep["cells"] == whole["cells"] and rep["literal_cells"] == whole["literal_cells"]
    if band is not None:
        assert rep["literal_cells"] >= 2                      # shared cells did go through the literal loop (the two aimed at, at least)
    if pair == TIGHT:
        # the greedy binds: some run's set is not the whole list's set restricted to the run
        assert any(accs[r].tobytes() != accs[3][m].tobytes() for r, m in enumerate(runs))
    assert len(eng.getMaxConsensusSet()) == 0                 # a batch has no single set
    eng.close()


# ---- 2. counts: only pairs that occur together in some run are solved ----------------------------------------------------
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_cells_are_those_some_run_needs(name):
    g = SC.graph(name)
    N = g.N
    tail = np.arange(16, N)
    # two tails that interleave along the chain, a run without the head, and the head's neighbours alone
    runs = [_i32(np.concatenate([np.arange(16), tail[0::2]])), _i32(np.concatenate([np.arange(16), tail[1::2]])),
            _i32(tail[1::3]), _i32(np.arange(2, 12))]
    tog, memb = together(N, runs)
    ov = overlap(g)
    iu = np.triu(np.ones((N, N), dtype=bool), 1)
    assert (ov & iu & ~tog & memb.any(axis=0)[:, None] & memb.any(axis=0)[None, :]).any()    # overlapping pairs that share no run exist
    want = int(memb.any(axis=0).sum() + (ov & iu & tog).sum())
    eng = SC.engine(g)
    bits, accs, rep = eng.run_batch(runs, want_bits=True)
    assert_batch_equals_fresh(name, g, runs, bits, accs)
    assert rep["cells"] == want
    assert rep["cells_separate"] == sum(fresh_run(name, g, m)[2]["cells"] for m in runs)
    assert rep["cells_separate"] > rep["cells"]
    cells = eng.cell_info()
    assert len(cells) == want == eng.solve_report()["cells"]
    seen = {(int(c["i"]), int(c["j"])) for c in cells}
    assert len(seen) == want                                  # distinct
    assert all(i <= j and tog[i, j] and (i == j or ov[i, j]) for i, j in seen)
    eng.close()


# ---- 3. word and round edges with per-run strides ------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 129, 200]


def test_word_edges_per_run_strides_and_output_bounds():
    """Runs of N_r around the 64-bit word and the 64-candidate round of the set-max in ONE call, so that neighbours have
    different strides: arrival-order prefixes (local = union index) and the same sizes from the tail of the list (local !=
    union index).  The bytes behind both outputs stay untouched."""
    from ipc_amd import capi
    wide = SC.graph("wide")
    assert wide.N == 200
    U = SC.stub(wide, sel=SC.arrival(wide))                   # the union in arrival order: a prefix of it is a prefix of the order
    runs = [_i32(np.arange(n)) for n in SIZES] + [_i32(np.arange(200 - n, 200)) for n in SIZES]
    refs = [SC.fresh(("wide", n), SC.stub(U, sel=np.arange(n)), *DEFAULT) for n in SIZES]          # (shared with the sweep's tests)
    refs += [fresh_run("wide-arrival", U, m) for m in runs[len(SIZES):]]
    sizes = [len(m) for m in runs]
    offsets = _i32(np.concatenate([[0], np.cumsum(sizes)]))
    members = _i32(np.concatenate(runs))
    mats = [n * ((n + 63) // 64) for n in sizes]
    mo = np.concatenate([[0], np.cumsum(mats)])
    nb, na = 8 * int(mo[-1]), int(offsets[-1])
    eng = SC.engine(U)
    for want_bits in (True, False):
        bbuf = np.full(nb + 64, 0xA5, dtype=np.uint8)
        abuf = np.full(na + 64, 0xA5, dtype=np.uint8)
        rep = capi.BatchReport()
        capi.check(eng.lib.ipc_run_batch(eng.h, len(runs), offsets.ctypes.data_as(vp), members.ctypes.data_as(vp),
                                         bbuf.ctypes.data_as(vp) if want_bits else None, abuf.ctypes.data_as(vp), ctypes.byref(rep)))
        assert (abuf[na:] == 0xA5).all()
        assert (bbuf[nb:] == 0xA5).all()
        if not want_bits:
            assert (bbuf == 0xA5).all()
        words = bbuf[:nb].view(np.uint64)
        for r, n in enumerate(sizes):
            b_ref, a_ref, _ = refs[r]
            assert abuf[offsets[r]:offsets[r + 1]].tobytes() == a_ref.tobytes(), (r, n)
            if want_bits:
                assert words[mo[r]:mo[r + 1]].tobytes() == b_ref.tobytes(), (r, n)
        assert rep.runs == len(runs) and rep.chunks == 1
    eng.close()


# ---- 4. more than 64 runs: membership word 1 -----------------------------------------------------------------------------
def test_more_than_64_runs():
    g = SC.graph("se2")
    rng = np.random.default_rng(11)
    runs = [_i32(np.sort(rng.choice(30, size=3 + (q & 1), replace=False))) for q in range(64)]       # triples and quadruples below 30
    runs += [_i32([q, 10 + q, 30 + q, 34 + q]) for q in range(6)]                                     # runs 64 .. 69 reach past 30
    assert len(runs) == 70 and all((np.diff(m) > 0).all() for m in runs)
    tog_low, _ = together(g.N, runs[:64])
    tog_all, _ = together(g.N, runs)
    ov = overlap(g)
    iu = np.triu(np.ones((g.N, g.N), dtype=bool), 1)
    only_high = ov & iu & tog_all & ~tog_low
    assert only_high.any()                                    # an overlapping pair that occurs together only in a run >= 64
    eng = SC.engine(g)
    bits, accs, rep = eng.run_batch(runs, want_bits=True)
    assert_batch_equals_fresh("se2", g, runs, bits, accs)
    memb_any = np.zeros(g.N, dtype=bool)
    memb_any[np.concatenate(runs)] = True
    assert rep["cells"] == int(memb_any.sum() + (ov & iu & tog_all).sum())
    seen = {(int(c["i"]), int(c["j"])) for c in eng.cell_info()}
    assert all((int(i), int(j)) in seen for i, j in zip(*np.nonzero(only_high)))
    assert rep["cells_separate"] == sum(fresh_run("se2", g, m)[2]["cells"] for m in runs)
    eng.close()


# ---- 5. chunks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_chunked_batch_equals_the_unchunked_call(monkeypatch, name):
    g = SC.graph(name)
    runs = standard_runs(g.N)
    eng = SC.engine(g)
    bits0, accs0, rep0 = eng.run_batch(runs, want_bits=True)
    assert rep0["chunks"] == 1
    eng.close()
    for chunk, want in ((1, 7), (2, 4)):
        monkeypatch.setenv("IPC_BATCH_CHUNK", str(chunk))
        eng = SC.engine(g)
        bits, accs, rep = eng.run_batch(runs, want_bits=True)
        assert rep["chunks"] == want
        assert all(a.tobytes() == b.tobytes() for a, b in zip(bits, bits0))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(accs, accs0))
        eng.close()
    monkeypatch.delenv("IPC_BATCH_CHUNK")
    assert_batch_equals_fresh(name, g, runs, bits0, accs0)


# ---- 6. long cells -------------------------------------------------------------------------------------------------------
def test_long_cells_are_shared_too(monkeypatch):
    """Chains beyond the one kernel of the policy go through the host-driven cluster solver, once per shared cell."""
    monkeypatch.setenv("IPC_SE2_POLICY", "w1")
    g = SC.graph("long")
    assert g.V <= 200 and g.N == 12
    runs = [_i32(np.arange(12)), _i32(np.arange(0, 12, 2)), _i32(np.arange(1, 12, 3)), _i32([0, 1, 2, 3, 8, 9, 10, 11]), _i32([7])]
    eng = SC.engine(g)
    bits, accs, rep = eng.run_batch(runs, want_bits=True)
    ref = fresh_run("long", g, runs[0])[2]
    assert rep["long_cells"] == ref["long_cells"] > 0 and rep["cells"] == ref["cells"]
    assert sum(fresh_run("long", g, m)[2]["long_cells"] for m in runs[1:]) > 0       # sub-lists hold long cells as well
    assert_batch_equals_fresh("long", g, runs, bits, accs)
    eng.close()


# ---- 7. neighbours -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_other_calls_and_the_batch_do_not_disturb_each_other(name):
    full = SC.graph(name)
    arr = SC.arrival(full)
    sel, last = arr[:-1], arr[-1]
    g = SC.stub(full, sel=sel)
    key = (name, "less-one")
    n = g.N
    runs = [_i32(np.arange(1, n, 2)), _i32(np.arange(0, n, 3)), _i32(np.arange(n - 9, n))]
    b_ref, a_ref, rep_ref = SC.fresh(key, g, *DEFAULT)
    eng = SC.engine(g)
    b, a = eng.run()
    assert b.tobytes() == b_ref.tobytes() and a.tobytes() == a_ref.tobytes()
    cns = eng.getMaxConsensusSet().copy()
    acc_on, rep_on = eng.run_online()
    assert rep_on["cells"] == rep_ref["cells"] and acc_on.tobytes() == a_ref.tobytes()
    _, rep_sw = eng.run_sweep([DEFAULT[0]], [DEFAULT[1]])
    assert rep_sw["reused_solve"] == 0
    bits, accs, rep = eng.run_batch(runs, want_bits=True)
    assert_batch_equals_fresh(key, g, runs, bits, accs)
    assert np.array_equal(eng.getMaxConsensusSet(), cns)
    assert len(eng.cell_info()) == rep["cells"] < rep_ref["cells"]             # this call's cells, fewer than the whole matrix
    b, a = eng.run()                                          # the same bytes after the batch
    assert b.tobytes() == b_ref.tobytes() and a.tobytes() == a_ref.tobytes()
    eng.run_batch(runs)
    acc_sw, rep_sw = eng.run_sweep([DEFAULT[0]], [DEFAULT[1]])
    assert rep_sw["reused_solve"] == 1 and acc_sw[0].tobytes() == a_ref.tobytes()   # the held sweep pass survived
    acc_on, rep_on = eng.run_online()
    assert rep_on["cells"] == 0 and acc_on.tobytes() == a_ref.tobytes()             # the online matrix was neither read nor changed
    # one more candidate, then a batch that uses the new index
    k = eng.append_candidate(full.loop_ids[last], full.loop_meas[last], full.loop_info[last])
    assert k == n
    g1 = SC.stub(full, sel=arr)
    runs1 = [_i32(np.concatenate([np.arange(0, n, 2), [n]])), _i32([n]), _i32(np.arange(n + 1))]
    bits, accs, rep = eng.run_batch(runs1, want_bits=True)
    assert rep["union_candidates"] == n + 1
    assert_batch_equals_fresh((name, "arrival"), g1, runs1, bits, accs)
    eng.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------
def _live(lib):
    out = (ctypes.c_int * 3)()
    assert lib.ipc_debug_live_resources(ctypes.byref(out)) == 0
    return list(out)


def test_argument_state_and_limit_errors(monkeypatch):
    from ipc_amd import capi
    g = SC.graph("se2")
    lib = capi.load()

    def call(eng, n_runs, offsets, members, acc=None):
        off = None if offsets is None else _i32(offsets)
        mem = None if members is None else _i32(members)
        return lib.ipc_run_batch(eng.h, n_runs, None if off is None else off.ctypes.data_as(vp),
                                 None if mem is None else mem.ctypes.data_as(vp), None,
                                 None if acc is None else acc.ctypes.data_as(vp), None)

    empty = SC.engine(SC.stub(g, sel=[]))
    assert call(empty, 1, [0, 1], [0]) == -3                  # IPC_ERR_STATE
    assert b"no candidates" in lib.ipc_last_error()
    empty.close()
    eng = SC.engine(SC.stub(g, sel=SC.arrival(g)[:20]))
    acc = np.zeros(64, dtype=np.uint8)
    assert call(eng, 0, [0], [0], acc) == -1
    assert b"runs" in lib.ipc_last_error()
    assert call(eng, 1, None, [0], acc) == -1
    assert b"NULL" in lib.ipc_last_error()
    assert call(eng, 1, [0, 1], None, acc) == -1
    assert b"NULL" in lib.ipc_last_error()
    assert call(eng, 2, [0, 2, 2], [0, 1], acc) == -1         # an empty run
    assert b"empty" in lib.ipc_last_error()
    assert call(eng, 1, [0, 2], [3, 20], acc) == -1           # an index outside [0, N_u)
    assert b"outside" in lib.ipc_last_error()
    assert call(eng, 1, [0, 2], [-1, 3], acc) == -1
    assert b"outside" in lib.ipc_last_error()
    assert call(eng, 1, [0, 3], [1, 4, 4], acc) == -1         # not strictly increasing: a repeat, a step back
    assert b"increasing" in lib.ipc_last_error()
    assert call(eng, 2, [0, 2, 4], [1, 4, 7, 2], acc) == -1
    assert b"increasing" in lib.ipc_last_error()
    assert not acc.any()
    assert call(eng, 2, [0, 2, 4], [1, 4, 2, 7], acc) == 0    # (the same numbers in order are a valid call)
    eng.close()
    # IPC_ERR_LIMIT: a chunk budget that holds no run, refused before anything is allocated
    monkeypatch.setenv("IPC_BATCH_BUDGET", "64")
    eng = SC.engine(SC.stub(g, sel=SC.arrival(g)[:20]))
    before = _live(lib)
    assert call(eng, 1, [0, 3], [1, 4, 7], acc) == -4
    assert b"budget" in lib.ipc_last_error()
    assert _live(lib) == before
    eng.close()


# ---- 9. resource balance -------------------------------------------------------------------------------------------------
def _balance_child():
    """Batches of growing size (every scratch array grows, some twice), an append in between, close: nothing stays behind.  In
    a process of its own, so that engines other test modules hold cannot move the process-wide counters."""
    sys.path.insert(0, ROOT)
    from ipc_amd import capi
    lib = capi.load()
    g = SC.graph("se2")
    arr = SC.arrival(g)
    assert _live(lib) == [0, 0, 0]
    eng = SC.engine(SC.stub(g, sel=arr[:20]))
    eng.run_batch([_i32([0, 3, 5])])
    held = _live(lib)
    eng.run_batch([_i32(np.arange(0, 20, 2)), _i32(np.arange(20))])
    eng.run_batch([_i32(np.arange(q % 5, 20, 2 + q % 3)) for q in range(70)])        # two membership words, 70 descriptors
    k = arr[20]
    eng.append_candidate(g.loop_ids[k], g.loop_meas[k], g.loop_info[k])
    runs = [_i32(np.arange(21)), _i32([4, 20])]
    bits, accs, rep = eng.run_batch(runs, want_bits=True)
    alive = _live(lib)
    assert alive[0] >= held[0] > 0 and alive[1] > 0 and alive[2] > 0, alive      # (the counters are wired, not constants)
    eng.close()
    assert _live(lib) == [0, 0, 0], "an engine's resources outlived it"
    assert_batch_equals_fresh(("se2", "first-21"), SC.stub(g, sel=arr[:21]), runs, bits, accs)
    assert _live(lib) == [0, 0, 0]
    print("batch resource balance OK: alive %s" % alive)


def test_batch_releases_everything_it_acquired():
    user_site = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + user_site + [os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "batch resource balance OK" in r.stdout


if __name__ == "__main__":
    _balance_child()
