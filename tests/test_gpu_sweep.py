"""Threshold sweep on the GPU (ipc_run_sweep): the cells are solved once and decided at many (fast_reject_th, slow_reject_th)
pairs; every entry must be, BIT FOR BIT, what run() gives on a fresh engine created with that pair.  No tolerances: one would hide
a first-pass / literal chi2 mix-up, a set-max mask shared between thresholds or a bit at the wrong stride.

Every reference is a fresh engine and the existing run() (tests/sweep_cases.py), never the sweep itself."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import sweep_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RECORD = ("max_chi2", "chi2_total", "iterations", "tries", "flags")
MIXED = [4, 0, 1, 3, 1, 5, 2]                                 # the six pairs unsorted, (10.64, 10.64) twice


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in SC.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


def _records(cells):
    """(i, j) -> the raw bytes of max_chi2, chi2_total, iterations, tries, flags."""
    return {(int(c["i"]), int(c["j"])): b"".join(np.asarray(c[f]).tobytes() for f in RECORD) for c in cells}


def _sweep(eng, pairs, want_bits=True):
    f, s = [p[0] for p in pairs], [p[1] for p in pairs]
    if want_bits:
        return eng.run_sweep(f, s, want_bits=True)
    acc, rep = eng.run_sweep(f, s)
    return None, acc, rep


def _cells_under(g, env, fast=6.251, slow=11.345):
    """Cell records of a fresh engine's run() at (fast, slow) with `env` on top of the environment of the moment."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = SC.engine(g, fast, slow)
        eng.run()
        cells = eng.cell_info().copy()
        eng.close()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return cells


def _first_pass_chi2(g):
    """Cell records of a fresh run() with the borderline band off: the first pass (and the Levenberg retry) alone."""
    return _cells_under(g, {"IPC_BORDERLINE_BAND": "0"})


def _retried(g, cells):
    """Per record of `cells`: the first pass ended with flags & 2, so the cell is retried with damping and never band-tested.
    The retry overwrites the flag; a run without the retry (IPC_LM_RETRY=0) still shows it."""
    raw = _cells_under(g, {"IPC_BORDERLINE_BAND": "0", "IPC_LM_RETRY": "0"})
    failed = {(int(c["i"]), int(c["j"])) for c in raw if int(c["flags"]) & 2}
    return np.array([(int(c["i"]), int(c["j"])) in failed for c in cells], dtype=bool)


def _borderline(cells, fast, slow, band, retried):
    """Cells a fresh engine at (fast, slow) sends to the literal loop: the expression of k_collect_failed in float64."""
    x = cells["max_chi2"]
    th = np.where(cells["i"] == cells["j"], fast, slow)
    with np.errstate(invalid="ignore"):
        return (np.abs(x - th) <= band * th) & ~retried


def _bit(bits, i, j):
    return int((int(bits[i, j >> 6]) >> (j & 63)) & 1)


# ---- 1. equality, both dimensions -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_every_entry_is_the_fresh_engines_run(name):
    g = SC.graph(name)
    pairs = [SC.PAIRS[q] for q in MIXED]
    eng = SC.engine(g, 123.0, 0.001)                          # (the engine's own thresholds are not consulted)
    bits, acc, rep = _sweep(eng, pairs)
    assert bits.shape == (len(pairs), g.N, (g.N + 63) // 64) and bits.dtype == np.uint64
    SC.assert_sweep_equals_fresh(name, g, pairs, bits, acc)
    assert len({a.tobytes() for a in acc}) >= 3               # not vacuous: the set does change with the pair
    assert acc[2].tobytes() == acc[4].tobytes()               # the repeated pair
    ref_cells = SC.fresh(name, g, *pairs[0])[2]["cells"]
    assert rep["thresholds"] == len(pairs) and rep["cells"] == ref_cells and rep["reused_solve"] == 0 and rep["chunks"] == 1
    assert len(eng.getMaxConsensusSet()) == 0                 # a sweep has no single set
    eng.close()


# ---- 2. oracle-held ------------------------------------------------------------------------------------------------------
_oracle_sweeps = {}


@pytest.mark.parametrize("t", range(len(SC.ORACLE_PAIRS)))
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_sweep_against_the_cpu_oracle(oracle, name, t):
    from ipc_amd.consensus import unpack_bits
    g = SC.graph(name)
    if name not in _oracle_sweeps:
        eng = SC.engine(g)
        _oracle_sweeps[name] = _sweep(eng, SC.ORACLE_PAIRS)[:2]
        eng.close()
    bits, acc = _oracle_sweeps[name]
    fast, slow = SC.ORACLE_PAIRS[t]
    cfg = SC.config(g, fast, slow)
    ok, _ = oracle.consistency_matrix(g.dim, g.odom_meas, g.odom_info, cfg.s_factor, g.loop_ids, g.loop_meas, g.loop_info,
                                      fast, cfg.fast_reject_iter_base, slow, cfg.slow_reject_iter_base)
    assert np.array_equal(unpack_bits(bits[t], g.N), ok)
    assert np.array_equal(acc[t], oracle.set_max(ok, oracle.candidate_order(g.loop_ids)))


# ---- 3. word and round edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 200])
def test_word_edges_and_output_bounds(N):
    """N around the 64-bit word and the 64-candidate round of the set-max; the bytes behind both outputs stay untouched."""
    from ipc_amd import capi
    wide = SC.graph("wide")
    assert wide.N == 200
    g = SC.stub(wide, sel=SC.arrival(wide)[:N])
    key = ("wide", N)
    pairs = [SC.PAIRS[0], SC.PAIRS[2], SC.PAIRS[4]]
    T, words = len(pairs), (N + 63) // 64
    eng = SC.engine(g)
    fast = np.array([p[0] for p in pairs]); slow = np.array([p[1] for p in pairs])
    for want_bits in (True, False):
        nb, na = T * N * words * 8, T * N
        bbuf = np.full(nb + 64, 0xA5, dtype=np.uint8)
        abuf = np.full(na + 64, 0x5A, dtype=np.uint8)
        rep = capi.SweepReport()
        capi.check(eng.lib.ipc_run_sweep(eng.h, T, fast.ctypes.data_as(ctypes.c_void_p), slow.ctypes.data_as(ctypes.c_void_p),
                                         bbuf.ctypes.data_as(ctypes.c_void_p) if want_bits else None,
                                         abuf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rep)))
        assert (abuf[na:] == 0x5A).all()
        assert (bbuf[nb:] == 0xA5).all()
        if not want_bits:
            assert (bbuf == 0xA5).all()
        bits = bbuf[:nb].view(np.uint64).reshape(T, N, words) if want_bits else None
        SC.assert_sweep_equals_fresh(key, g, pairs, bits, abuf[:na].reshape(T, N))
        assert rep.reused_solve == (0 if want_bits else 1)
    eng.close()


# ---- 4. the band ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_borderline_band_keeps_first_pass_and_literal_apart(monkeypatch, name):
    g = SC.graph(name)
    band = 0.05
    cells = _first_pass_chi2(g)
    retried = _retried(g, cells)
    usable = np.isfinite(cells["max_chi2"]) & (cells["max_chi2"] > 1e-3) & ~retried
    diag = np.sort(cells["max_chi2"][usable & (cells["i"] == cells["j"])])
    pair = np.sort(cells["max_chi2"][usable & (cells["i"] != cells["j"])])
    assert len(diag) >= 3 and len(pair) >= 3
    xs = [(diag[len(diag) // 3], pair[len(pair) // 3]), (diag[2 * len(diag) // 3], pair[2 * len(pair) // 3])]
    pairs = []
    for xd, xp in xs:                                         # inside the band of x / 1.03, outside that of 1.2 x
        pairs += [(xd / 1.03, xp / 1.03), (1.2 * xd, 1.2 * xp)]
    border = [_borderline(cells, f, s, band, retried) for f, s in pairs]
    union = np.logical_or.reduce(border)
    assert any((border[a] & ~border[b]).any() for a in range(len(pairs)) for b in range(len(pairs)))   # borderline at one pair, not at another
    monkeypatch.setenv("IPC_BORDERLINE_BAND", str(band))
    eng = SC.engine(g)
    bits, acc, rep = _sweep(eng, pairs)
    SC.assert_sweep_equals_fresh(name, g, pairs, bits, acc)
    lit = [SC.fresh(name, g, f, s)[2]["literal_cells"] for f, s in pairs]
    assert rep["literal_cells"] > 0 and max(lit) <= rep["literal_cells"] <= sum(lit)
    assert rep["literal_held"] == rep["literal_cells"]
    assert lit == [int(b.sum()) for b in border]              # (retried cells are no borderline cells: left out of `border`)
    assert rep["literal_cells"] == int(union.sum())
    eng.close()
    # g2o's literal loop everywhere (IPC_TERMINATE_EPS=0): the band is 0, nothing is solved again
    monkeypatch.setenv("IPC_TERMINATE_EPS", "0")
    eng = SC.engine(g)
    bits, acc, rep = _sweep(eng, pairs)
    assert rep["literal_cells"] == 0 and rep["literal_held"] == 0
    SC.assert_sweep_equals_fresh(name, g, pairs, bits, acc)
    eng.close()


@pytest.mark.parametrize("name", ["se2", "se3"])
def test_held_literal_is_not_used_outside_the_band(monkeypatch, name):
    """A literal record is observable through bits only, and it lies within 2 sqrt(term_eps) of the first pass: far inside a band
    of 0.05.  So this case takes the band from the data: the cell whose literal chi2 y is farthest (relatively) from its first
    pass x, a band of an eighth of that distance, pair A with the cell's threshold AT x (borderline: the literal record is
    solved and held) and pair B with it half way between x and y -- four band widths from x, not borderline, and x and y lie on
    opposite sides of it.  At B a fresh engine decides on x; a sweep that used the literal wherever it is held would decide on y."""
    g = SC.graph(name)
    cells = _first_pass_chi2(g)
    literal = _cells_under(g, {"IPC_TERMINATE_EPS": "0"})     # g2o's literal loop on every cell: only used to aim the thresholds
    y_of = {(int(c["i"]), int(c["j"])): float(c["max_chi2"]) for c in literal}
    x = cells["max_chi2"]
    y = np.array([y_of[(int(c["i"]), int(c["j"]))] for c in cells])
    usable = np.isfinite(x) & np.isfinite(y) & (x > 1e-3) & ~_retried(g, cells)
    rel = np.where(usable, np.abs(y - x) / np.where(usable, x, 1.0), 0.0)
    c = int(np.argmax(rel))
    assert rel[c] > 1e-12                                     # the two loops do end at different values somewhere
    i, j, xc = int(cells["i"][c]), int(cells["j"][c]), float(x[c])
    band = float(rel[c]) / 8.0
    monkeypatch.setenv("IPC_BORDERLINE_BAND", repr(band))
    th_a = xc
    pair_a = (th_a, SC.PAIRS[0][1]) if i == j else (SC.PAIRS[0][0], th_a)
    lit_c = [float(r["max_chi2"]) for r in _cells_under(g, {}, *pair_a) if (int(r["i"]), int(r["j"])) == (i, j)][0]
    assert lit_c != xc                                        # the fresh engine at A did replace the cell's chi2 by its literal record
    th_b = 0.5 * (xc + lit_c)
    pair_b = (th_b, SC.PAIRS[0][1]) if i == j else (SC.PAIRS[0][0], th_b)
    assert abs(xc - th_a) <= band * th_a and not abs(xc - th_b) <= band * th_b
    assert (xc > th_b) != (lit_c > th_b)                      # first pass and literal straddle the threshold of B
    pairs = [pair_a, pair_b]
    eng = SC.engine(g)
    bits, acc, rep = _sweep(eng, pairs)
    assert rep["literal_cells"] >= 1
    assert _bit(bits[1], i, j) == (0 if xc > th_b else 1)
    SC.assert_sweep_equals_fresh(name, g, pairs, bits, acc)
    eng.close()
    # ... and when the record was left behind by an earlier call
    eng = SC.engine(g)
    _sweep(eng, [pair_a])
    bits, acc, rep = _sweep(eng, [pair_b])
    assert rep["reused_solve"] == 1 and rep["literal_held"] >= 1
    assert _bit(bits[0], i, j) == (0 if xc > th_b else 1)
    SC.assert_sweep_equals_fresh(name, g, [pair_b], bits, acc)
    eng.close()


# ---- 5. long and borderline cells ----------------------------------------------------------------------------------------
def test_long_cells_inside_the_band(monkeypatch):
    """Chains beyond the one kernel of the policy go through the host-driven cluster solver, in the first pass and -- with the
    convergence test off -- when a requested pair makes them borderline."""
    g = SC.graph("long")
    assert g.V <= 200 and g.N <= 16
    band, cap = 0.05, 64
    monkeypatch.setenv("IPC_SE2_POLICY", "w1")
    cells = _first_pass_chi2(g)
    span = cells["hi"] - cells["lo"]
    assert span.max() > cap
    is_long = span > cap
    retried = _retried(g, cells)
    usable = is_long & np.isfinite(cells["max_chi2"]) & (cells["max_chi2"] > 1e-3) & ~retried
    xd = cells["max_chi2"][usable & (cells["i"] == cells["j"])]
    xp = cells["max_chi2"][usable & (cells["i"] != cells["j"])]
    assert len(xd) >= 1 and len(xp) >= 1
    xd, xp = float(np.sort(xd)[len(xd) // 2]), float(np.sort(xp)[len(xp) // 2])
    pairs = [SC.PAIRS[0], (xd / 1.03, xp / 1.03), (1.2 * xd, 1.2 * xp)]
    assert (_borderline(cells, *pairs[1], band, retried) & is_long).any()
    monkeypatch.setenv("IPC_BORDERLINE_BAND", str(band))
    eng = SC.engine(g)
    bits, acc, rep = _sweep(eng, pairs)
    assert rep["long_cells"] == int(is_long.sum()) >= 2
    assert rep["literal_cells"] >= 1
    SC.assert_sweep_equals_fresh("long", g, pairs, bits, acc)
    eng.close()


# ---- 6. the held pass, first checks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_held_pass_is_reused_and_survives_other_calls(name):
    g = SC.graph(name)
    eng = SC.engine(g)
    bits, acc, rep = _sweep(eng, SC.PAIRS[:2])
    assert rep["reused_solve"] == 0 and rep["cells"] > 0
    SC.assert_sweep_equals_fresh(name, g, SC.PAIRS[:2], bits, acc)
    # the cell records after a sweep: the first pass, i.e. those of a fresh run() without the band
    assert _records(eng.cell_info()) == _records(_first_pass_chi2(g))
    assert eng.solve_report()["cells"] == rep["cells"]
    bits, acc, rep2 = _sweep(eng, SC.PAIRS[2:5])
    assert rep2["reused_solve"] == 1 and rep2["cells"] == 0 and rep2["thresholds"] == 3
    SC.assert_sweep_equals_fresh(name, g, SC.PAIRS[2:5], bits, acc)
    # a run() and a run_online() in between: neither disturbs the held pass, nor the sweep them
    b_ref, a_ref, _ = SC.fresh(name, g, *SC.PAIRS[0])
    b, a = eng.run()
    assert b.tobytes() == b_ref.tobytes() and a.tobytes() == a_ref.tobytes()
    b, a, _ = eng.run_online(want_bits=True)
    assert b.tobytes() == b_ref.tobytes() and a.tobytes() == a_ref.tobytes()
    bits, acc, rep3 = _sweep(eng, [SC.PAIRS[5], SC.PAIRS[3]])
    assert rep3["reused_solve"] == 1 and rep3["cells"] == 0
    SC.assert_sweep_equals_fresh(name, g, [SC.PAIRS[5], SC.PAIRS[3]], bits, acc)
    b, a = eng.run()
    assert b.tobytes() == b_ref.tobytes() and a.tobytes() == a_ref.tobytes()
    acc_on, rep_on = eng.run_online()
    assert rep_on["cells"] == 0 and acc_on.tobytes() == a_ref.tobytes()      # the online matrix was neither read nor changed
    eng.close()


# ---- 7. the held pass, invalidation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_held_pass_invalidation(name):
    full = SC.graph(name)
    V0 = full.V - 3
    arr = [k for k in SC.arrival(full) if full.loop_ids[k].max() < V0]
    assert len(arr) >= 8
    sel, last = arr[:-1], arr[-1]
    pairs = [SC.PAIRS[0], SC.PAIRS[2]]
    eng = SC.engine(SC.stub(full, V0, sel))
    bits, acc, rep = _sweep(eng, pairs)
    assert rep["reused_solve"] == 0
    SC.assert_sweep_equals_fresh((name, "short", V0), SC.stub(full, V0, sel), pairs, bits, acc)
    # three more odometry edges: no existing cell reads a later vertex, the held pass stays
    assert eng.append_odometry(full.odom_meas[V0 - 1:V0 + 2], full.odom_info[V0 - 1:V0 + 2]) == full.V
    bits, acc, rep = _sweep(eng, pairs)
    assert rep["reused_solve"] == 1 and rep["cells"] == 0
    SC.assert_sweep_equals_fresh((name, "short", full.V), SC.stub(full, full.V, sel), pairs, bits, acc)
    # one more candidate: the held pass is that of the shorter list
    eng.append_candidate(full.loop_ids[last], full.loop_meas[last], full.loop_info[last])
    bits, acc, rep = _sweep(eng, pairs)
    g_long = SC.stub(full, full.V, arr)
    assert rep["reused_solve"] == 0 and rep["cells"] == SC.fresh((name, "longer"), g_long, *pairs[0])[2]["cells"]
    SC.assert_sweep_equals_fresh((name, "longer"), g_long, pairs, bits, acc)
    bits, acc, rep = _sweep(eng, pairs)
    assert rep["reused_solve"] == 1
    eng.sweep_reset()
    assert len(eng.cell_info()) == 0
    bits, acc, rep = _sweep(eng, pairs)
    assert rep["reused_solve"] == 0 and rep["cells"] > 0
    SC.assert_sweep_equals_fresh((name, "longer"), g_long, pairs, bits, acc)
    eng.close()


# ---- 8. chunks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se2", "se3"])
def test_chunked_sweep_equals_the_unchunked_call(monkeypatch, name):
    g = SC.graph(name)
    pairs = SC.PAIRS[:5]
    eng = SC.engine(g)
    bits0, acc0, rep0 = _sweep(eng, pairs)
    assert rep0["chunks"] == 1
    eng.close()
    for chunk, want in ((1, 5), (2, 3)):
        monkeypatch.setenv("IPC_SWEEP_CHUNK", str(chunk))
        eng = SC.engine(g)
        bits, acc, rep = _sweep(eng, pairs)
        assert rep["chunks"] == want
        assert bits.tobytes() == bits0.tobytes() and acc.tobytes() == acc0.tobytes()
        eng.close()
    monkeypatch.delenv("IPC_SWEEP_CHUNK")
    SC.assert_sweep_equals_fresh(name, g, pairs, bits0, acc0)


# ---- 9. errors and balance -----------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    from ipc_amd import capi
    g = SC.graph("se2")
    lib = capi.load()
    vp = ctypes.c_void_p
    two = np.array([6.251, 11.345])
    nan = np.array([6.251, np.nan])
    empty = SC.engine(SC.stub(g, sel=[]))
    assert lib.ipc_run_sweep(empty.h, 2, two.ctypes.data_as(vp), two.ctypes.data_as(vp), None, None, None) == -3      # IPC_ERR_STATE
    assert b"no candidates" in lib.ipc_last_error()
    empty.close()
    eng = SC.engine(SC.stub(g, sel=SC.arrival(g)[:20]))
    acc = np.zeros(2 * eng.N, dtype=np.uint8)
    assert lib.ipc_run_sweep(eng.h, 0, two.ctypes.data_as(vp), two.ctypes.data_as(vp), None, acc.ctypes.data_as(vp), None) == -1
    assert b"thresholds" in lib.ipc_last_error()
    assert lib.ipc_run_sweep(eng.h, 2, None, two.ctypes.data_as(vp), None, acc.ctypes.data_as(vp), None) == -1
    assert b"NULL" in lib.ipc_last_error()
    assert lib.ipc_run_sweep(eng.h, 2, two.ctypes.data_as(vp), nan.ctypes.data_as(vp), None, acc.ctypes.data_as(vp), None) == -1
    assert b"NaN" in lib.ipc_last_error()
    assert not acc.any()
    eng.close()


def _live(lib):
    out = (ctypes.c_int * 3)()
    assert lib.ipc_debug_live_resources(ctypes.byref(out)) == 0
    return list(out)


def _balance_child():
    """sweep (the scratch grows), sweep (reuse, grows again), append_candidate, sweep, close: nothing stays behind.  In a process
    of its own, so that engines other test modules hold cannot move the process-wide counters."""
    sys.path.insert(0, ROOT)
    from ipc_amd import capi
    lib = capi.load()
    g = SC.graph("se2")
    arr = SC.arrival(g)
    assert _live(lib) == [0, 0, 0]
    eng = SC.engine(SC.stub(g, sel=arr[:20]))
    _, _, rep = _sweep(eng, SC.PAIRS[:2])
    assert rep["reused_solve"] == 0
    _, _, rep = _sweep(eng, SC.PAIRS)                         # more thresholds than the scratch holds: it grows again
    assert rep["reused_solve"] == 1 and rep["chunks"] == 1
    k = arr[20]
    eng.append_candidate(g.loop_ids[k], g.loop_meas[k], g.loop_info[k])
    bits, acc, rep = _sweep(eng, SC.PAIRS[:2])
    assert rep["reused_solve"] == 0
    alive = _live(lib)
    assert alive[0] > 0 and alive[2] > 0, alive               # (the counters are wired, not constants)
    eng.close()
    assert _live(lib) == [0, 0, 0], "an engine's resources outlived it"
    g21 = SC.stub(g, sel=arr[:21])
    SC.assert_sweep_equals_fresh(("se2", 21), g21, SC.PAIRS[:2], bits, acc)
    assert _live(lib) == [0, 0, 0]
    print("sweep resource balance OK: alive %s" % alive)


def test_sweep_releases_everything_it_acquired():
    user_site = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + user_site + [os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sweep resource balance OK" in r.stdout


if __name__ == "__main__":
    _balance_child()
