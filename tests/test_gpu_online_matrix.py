"""Online matrix mode on the GPU (ipc_run_online): an engine whose candidates arrive a few at a time must hold, BIT FOR BIT, what
ipc_run gives on the same list -- the consistency matrix, the accepted set, and every cell's record.  No tolerances: one would
hide a lost bit of the boundary word (coverage M not a multiple of 64), a stale accepted mask or a row at the wrong stride.

"batch"  = a fresh engine with the whole chain and the candidate list of the moment, one run().
"online" = candidates appended (ipc_append_candidate) in arrival order -- by later vertex, ties in file order, which is the
           processing order -- with a run_online() after every burst.  Batch engines get their candidates in arrival order too,
           so candidate q is candidate q on both sides."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-5      # chi2 tolerance (relative) of the project, used only for a bin whose kernel variant depends on the list length
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = ("max_chi2", "chi2_total", "iterations", "tries", "flags")


def _cfg(dim):
    from ipc_amd.consensus import Config
    return Config(s_factor=10.0) if dim == 2 else Config(s_factor=50.0, slow_reject_th=6.251)


def _se2_graph():
    from ipc_amd import synth                      # the 3-lap graph of the online-chain tests
    return synth.inject_outliers(synth._se2_graph(400, 24, seed=75, laps=3.0, name="inc"), 16, seed=5)


def _se3_graph():
    from ipc_amd import synth                      # the small sphere of the online-chain tests
    g = synth.sphere_like(rings=8, per_ring=16, radius=8.0)
    keep = np.arange(0, g.N, max(1, g.N // 24))
    return synth.inject_outliers(g.subset(keep), 8, seed=6)


def _wide_graph(dim):
    """A few hundred candidates: bursts of 64 and 65, coverage beyond two doublings of the 64-candidate capacity."""
    from ipc_amd import synth
    if dim == 2:
        return synth.inject_outliers(synth._se2_graph(400, 150, seed=76, laps=3.0, name="wide"), 50, seed=7)
    g = synth.sphere_like(rings=8, per_ring=16, radius=8.0)
    keep = np.arange(0, g.N, max(1, g.N // 110))
    return synth.inject_outliers(g.subset(keep), 40, seed=8)


def _graph(dim):
    return _se2_graph() if dim == 2 else _se3_graph()


def _stub(g, V=None, sel=()):
    """The graph as far as its first V vertices (default: all), with the candidates `sel` in that order."""
    from ipc_amd.graphio import PoseGraph
    V = g.V if V is None else V
    sel = np.asarray(sel, dtype=np.int64)
    return PoseGraph(g.dim, g.vertices[:V], g.odom_meas[:V - 1], g.odom_info[:V - 1],
                     g.loop_ids[sel].reshape(-1, 2), g.loop_meas[sel], g.loop_info[sel], dict(g.meta))


def _engine(g, cfg):
    from ipc_amd.consensus import IPC
    return IPC(g, cfg, device=0)


def _arrival(g):
    """File indices in arrival order: by later vertex, ties in file order (the engine's processing order)."""
    return [int(k) for k in np.argsort(g.loop_ids.max(axis=1), kind="stable")]


def _batch(g, cfg, sel, want_cells=False):
    """bits, accepted (and the cell records, the cell count) of a fresh engine's run() on the candidates `sel`."""
    eng = _engine(_stub(g, g.V, sel), cfg)
    bits, acc = eng.run()
    out = (bits, acc, _records(eng.cell_info()), eng.solve_report()["cells"]) if want_cells else (bits, acc)
    eng.close()
    return out


def _records(cells):
    """(i, j) -> the raw bytes of max_chi2, chi2_total, iterations, tries, flags."""
    return {(int(c["i"]), int(c["j"])): b"".join(np.asarray(c[f]).tobytes() for f in RECORD) for c in cells}


def _append(eng, g, ks):
    return [eng.append_candidate(g.loop_ids[k], g.loop_meas[k], g.loop_info[k]) for k in ks]


def _latency_bins_in_play(dim=3):
    """Bins whose kernel variant depends on the NUMBER of cells in the launch (the latency variants of thin bins), from the
    engine's default policies: [(shortest chain, longest chain)] of each such bin.  A cell of such a bin may be solved by another
    kernel in an online update (few cells) than in the batch step; every other cell's kernel depends on its bin alone.
    choose_kernel takes the latency variant of a bin from the plan for either dimension, so SE2 is checked too: the plan
    (make_plan, cell_plan.hpp) gives a bin a latency variant in one place only, and that place is reached for SE3 alone (there
    is no SE2 latency policy)."""
    assert not os.environ.get("IPC_SE3_POLICY") and not os.environ.get("IPC_SE3_LATENCY_POLICY") and not os.environ.get("IPC_SE2_POLICY")
    src = open(os.path.join(ROOT, "ipc_amd", "csrc", "cell_plan.hpp")).read()
    if dim == 2:
        sets = [m.start() for m in re.finditer(r"latency\[b\] = (?!nullptr;)", src)]
        guard = src.index("if (dim == 3) {")
        assert len(sets) == 1 and guard < sets[0] < src.index("return true;", guard)
        assert "SE2_LATENCY_POLICY" not in src
        return []
    pol = re.search(r'kDefaultPolicy3 = "([^"]+)"', src).group(1).split(",")
    lat = re.search(r'kDefaultLatencyPolicy3 = "([^"]+)"', src).group(1).split(",")
    bins = []                                                 # (capacity, waves per cell or None for the LDS-pose kernels)
    for tok in pol:
        if tok[0] in "wg":
            bins.append((64 * (1 if tok[0] == "w" else 4) * int(tok[1:]), None))
        else:
            w, m = map(int, tok.split("x"))
            bins.append((64 * w * m, w))
    bins.sort()
    lats = sorted((64 * w * m, w) for w, m in (map(int, t.split("x")) for t in lat))
    play, prev = [], 0
    for cap, w in bins:
        if w is not None:                                     # block variants only (make_plan)
            first = next(((c, lw) for c, lw in lats if c >= cap), None)
            if first is not None and first[1] > w:
                play.append((prev + 1, cap))
        prev = cap
    return play


def _assert_records_equal(g_dim, online, batch, spans):
    assert sorted(online) == sorted(batch)
    loose = _latency_bins_in_play(g_dim)
    for key in batch:
        if any(a <= spans[key] <= b for a, b in loose):       # (not with the default policies: asserted by the caller)
            o = np.frombuffer(online[key][:16], dtype=np.float64)
            b = np.frombuffer(batch[key][:16], dtype=np.float64)
            assert abs(o[0] - b[0]) <= REL * max(abs(b[0]), 1e-12), key
        else:
            assert online[key] == batch[key], key


@pytest.mark.parametrize("dim", [2, 3], ids=["se2", "se3"])
def test_one_by_one_is_bitwise_the_batch_run(dim):
    """Candidates one at a time: after every update the accepted set of a fresh batch engine on the same prefix; at the end the
    matrix word for word, the union of the per-update cell records = the batch records, the sum of report.cells = the batch
    cell count; an update with nothing new solves nothing and returns the same outputs."""
    g, cfg = _graph(dim), _cfg(dim)
    arr = _arrival(g)
    assert _latency_bins_in_play(dim) == []                   # the premise of the bitwise records: a cell's kernel depends on its bin alone
    eng = _engine(_stub(g), cfg)
    assert eng.N == 0 and eng.online_covered == 0
    recs, cells, spans = {}, 0, {}
    for q, k in enumerate(arr):
        assert _append(eng, g, [k]) == [q]
        acc, rep = eng.run_online()
        assert (rep["covered_before"], rep["covered_after"]) == (q, q + 1) and eng.online_covered == q + 1
        assert 1 <= rep["cells"] <= q + 1                     # its own cell and at most one per covered candidate
        assert rep["set_max_resumed"] == (1 if q else 0)      # in-order arrival: the greedy resumes on every update after the first
        info = eng.cell_info()
        assert len(info) == rep["cells"] == eng.solve_report()["cells"]
        assert all(int(c["j"]) == q and int(c["i"]) <= q for c in info)
        new = _records(info)
        assert not set(new) & set(recs)
        recs.update(new)
        spans.update({(int(c["i"]), int(c["j"])): int(c["hi"]) - int(c["lo"]) for c in info})
        cells += rep["cells"]
        _, acc_ref = _batch(g, cfg, arr[:q + 1])
        assert acc.tobytes() == acc_ref.tobytes(), q
    bits_ref, acc_ref, recs_ref, cells_ref = _batch(g, cfg, arr, want_cells=True)
    bits, acc, rep = eng.run_online(want_bits=True)           # nothing new
    assert rep["cells"] == 0 and rep["covered_before"] == rep["covered_after"] == g.N and rep["grew"] == 0
    assert len(eng.cell_info()) == 0
    assert bits.tobytes() == bits_ref.tobytes() and acc.tobytes() == acc_ref.tobytes()
    bits2, acc2, rep2 = eng.run_online(want_bits=True)
    assert rep2["cells"] == 0 and bits2.tobytes() == bits.tobytes() and acc2.tobytes() == acc.tobytes()
    assert cells == cells_ref
    _assert_records_equal(dim, recs, recs_ref, spans)
    assert [int(k) for k in eng.getMaxConsensusSet()] == [q for q in range(g.N) if acc_ref[q]]   # (arrival order = processing order)


@pytest.mark.parametrize("reserve", [False, True], ids=["growing", "reserved"])
@pytest.mark.parametrize("dim", [2, 3], ids=["se2", "se3"])
def test_bursts_and_boundaries(dim, reserve):
    """Updates of 1, 7, 64 and 65 candidates: coverage crosses multiples of 64 mid-word (M = 8 -> 72: the boundary word holds
    old columns beside new ones) and N crosses the capacity twice (64 -> 128 -> 256), reported in `grew`; with
    ipc_reserve_candidates up front nothing ever grows.  Matrix and accepted set after every update."""
    g, cfg = _wide_graph(dim), _cfg(dim)
    arr = _arrival(g)
    assert g.N >= 1 + 7 + 64 + 65 + 1
    eng = _engine(_stub(g), cfg)
    if reserve:
        eng.reserve_candidates(g.N)
    done, cap, sizes, grown, cells, crossed = 0, 0, [1, 7, 64, 65], 0, 0, 0
    step = 0
    while done < g.N:
        n = min(sizes[step % 4], g.N - done)
        step += 1
        _append(eng, g, arr[done:done + n])
        bits, acc, rep = eng.run_online(want_bits=True)
        N = done + n
        if done % 64 and done // 64 != (N - 1) // 64:
            crossed += 1
        expect_grew = 0
        if not reserve and N > cap:
            cap = max(64, cap)
            while cap < N:
                cap *= 2
            expect_grew = 1
        assert rep["grew"] == expect_grew, (done, N)
        grown += rep["grew"]
        assert (rep["covered_before"], rep["covered_after"]) == (done, N)
        assert rep["set_max_resumed"] == (1 if done else 0)
        cells += rep["cells"]
        bits_ref, acc_ref = _batch(g, cfg, arr[:N])
        assert bits.shape == bits_ref.shape == (N, (N + 63) // 64)
        assert acc.tobytes() == acc_ref.tobytes(), (done, N)
        assert bits.tobytes() == bits_ref.tobytes(), (done, N)
        done = N
    assert crossed >= 2
    assert grown == 0 if reserve else grown >= 3              # 0 -> 64 -> 128 -> 256 (-> 512)
    _, _, _, cells_ref = _batch(g, cfg, arr, want_cells=True)
    assert cells == cells_ref


@pytest.mark.parametrize("dim", [2, 3], ids=["se2", "se3"])
def test_chain_and_candidates_grow_together(dim):
    """The engine starts at 2 vertices; a pose is appended, then the candidates it completes, then the matrix is brought up to
    date: at the end the matrix and the accepted set of the batch engine on the whole graph."""
    g, cfg = _graph(dim), _cfg(dim)
    arr = _arrival(g)
    hi = g.loop_ids.max(axis=1)
    eng = _engine(_stub(g, 2), cfg)
    acc = None
    for v in range(2, g.V):
        assert eng.append_odometry(g.odom_meas[v - 1], g.odom_info[v - 1]) == v + 1
        ks = [k for k in arr if hi[k] == v]
        if ks:
            _append(eng, g, ks)
            acc, rep = eng.run_online()
            assert rep["covered_after"] == eng.N and rep["cells"] >= len(ks)
    assert eng.n_vertices == g.V and eng.N == g.N
    bits_ref, acc_ref = _batch(g, cfg, arr)
    bits, acc2, rep = eng.run_online(want_bits=True)
    assert rep["cells"] == 0
    assert acc.tobytes() == acc2.tobytes() == acc_ref.tobytes()
    assert bits.tobytes() == bits_ref.tobytes()


@pytest.mark.parametrize("dim", [2, 3], ids=["se2", "se3"])
def test_out_of_order_arrival_reruns_the_greedy(dim):
    """A candidate whose later vertex precedes covered candidates sorts in front of them: the greedy is rerun from the start
    (set_max_resumed == 0) and gives the batch set; in-order arrivals resume."""
    g, cfg = _graph(dim), _cfg(dim)
    arr = _arrival(g)
    late = arr[2]                                             # an early candidate, held back to the end
    assert g.loop_ids[late].max() < g.loop_ids[arr[-1]].max()
    rest = [k for k in arr if k != late]
    eng = _engine(_stub(g), cfg)
    for q, k in enumerate(rest):
        _append(eng, g, [k])
        _, rep = eng.run_online()
        assert rep["set_max_resumed"] == (1 if q else 0)
    _append(eng, g, [late])
    assert int(eng.candidate_order()[-1]) != g.N - 1          # it does not sort last
    bits, acc, rep = eng.run_online(want_bits=True)
    assert rep["set_max_resumed"] == 0 and rep["cells"] >= 1
    bits_ref, acc_ref = _batch(g, cfg, rest + [late])
    assert acc.tobytes() == acc_ref.tobytes() and bits.tobytes() == bits_ref.tobytes()


@pytest.mark.parametrize("dim", [2, 3], ids=["se2", "se3"])
def test_mode_interplay(dim):
    g, cfg = _graph(dim), _cfg(dim)
    arr = _arrival(g)
    full = _stub(g, g.V, arr)
    bits_ref, acc_ref = _batch(g, cfg, arr)
    # run_online between agreementCheck calls: the faithful records of an undisturbed run, bitwise
    plain, mixed = _engine(full, cfg), _engine(full, cfg)
    order = [int(k) for k in plain.candidate_order()]
    plain.reset(), mixed.reset()
    want = []
    for k in order:
        ok, info = plain.agreementCheck(k, with_info=True)
        want.append((ok, bytes(info)))
    got = []
    for q, k in enumerate(order):
        if q % 5 == 2:
            acc, _ = mixed.run_online()
            assert acc.tobytes() == acc_ref.tobytes()
        ok, info = mixed.agreementCheck(k, with_info=True)
        got.append((ok, bytes(info)))
    assert got == want
    assert [int(k) for k in mixed.getMaxConsensusSet()] == [int(k) for k in plain.getMaxConsensusSet()]
    plain.close(), mixed.close()
    # run() after run_online, and run_online after run(): both the batch result, whichever came first
    eng = _engine(_stub(g, g.V, arr[:g.N // 2]), cfg)
    eng.run_online()
    _append(eng, g, arr[g.N // 2:])
    b, a = eng.run()                                          # (the online call left no stale plan behind)
    assert b.tobytes() == bits_ref.tobytes() and a.tobytes() == acc_ref.tobytes()
    assert eng.online_covered == g.N // 2                     # run() neither reads nor moves the online matrix
    b, a, rep = eng.run_online(want_bits=True)
    assert rep["covered_before"] == g.N // 2 and b.tobytes() == bits_ref.tobytes() and a.tobytes() == acc_ref.tobytes()
    b, a = eng.run()
    assert b.tobytes() == bits_ref.tobytes() and a.tobytes() == acc_ref.tobytes()
    acc_set, _ = eng.run_set_only()
    assert acc_set.tobytes() == acc_ref.tobytes()
    # ipc_online_reset: a whole solve again; ipc_set_candidates resets the coverage implicitly
    eng.online_reset()
    assert eng.online_covered == 0
    b, a, rep = eng.run_online(want_bits=True)
    assert rep["covered_before"] == 0 and rep["set_max_resumed"] == 0
    assert b.tobytes() == bits_ref.tobytes() and a.tobytes() == acc_ref.tobytes()
    sel = arr[:g.N // 3]
    eng.set_candidates(g.loop_ids[sel], g.loop_meas[sel], g.loop_info[sel])
    assert eng.online_covered == 0
    b, a, rep = eng.run_online(want_bits=True)
    b3, a3 = _batch(g, cfg, sel)
    assert rep["covered_before"] == 0 and rep["covered_after"] == len(sel)
    assert b.tobytes() == b3.tobytes() and a.tobytes() == a3.tobytes()


@pytest.mark.parametrize("dim", [2, 3], ids=["se2", "se3"])
def test_reserve_on_a_list_in_use(dim):
    """ipc_reserve_candidates on an engine that holds candidates and has run: the candidate arrays move to a larger capacity.
    Every matrix call after it plans from the moved records (row order rebuilt, no cached plan of the old arrays), the faithful
    pipeline's streams wait for the copies, and appends within the reserved capacity grow nothing."""
    g, cfg = _graph(dim), _cfg(dim)
    arr = _arrival(g)
    half = g.N // 2
    assert half <= 64 < 300                                   # the first list fits the smallest capacity; the reserve outgrows it
    b_half, a_half = _batch(g, cfg, arr[:half])
    b_full, a_full = _batch(g, cfg, arr)

    def same(out, bits_ref, acc_ref):
        return out[0].tobytes() == bits_ref.tobytes() and out[1].tobytes() == acc_ref.tobytes()

    # run, reserve, then each matrix entry point on an engine of its own (none leans on what another one rebuilt)
    eng = _engine(_stub(g, g.V, arr[:half]), cfg)
    assert same(eng.run(), b_half, a_half)
    eng.reserve_candidates(300)
    assert same(eng.run(), b_half, a_half)
    eng.close()
    eng = _engine(_stub(g, g.V, arr[:half]), cfg)
    assert same(eng.run(), b_half, a_half)
    eng.reserve_candidates(300)
    acc_set, _ = eng.run_set_only()
    assert acc_set.tobytes() == a_half.tobytes()
    eng.close()
    # run, reserve, run_online (which drops the batch plan), run; then appends within the capacity: nothing grows
    eng = _engine(_stub(g, g.V, arr[:half]), cfg)
    assert same(eng.run(), b_half, a_half)
    eng.reserve_candidates(300)
    b, a, rep = eng.run_online(want_bits=True)
    assert same((b, a), b_half, a_half) and rep["grew"] == 0 and rep["covered_after"] == half
    assert same(eng.run(), b_half, a_half)
    eng.reserve_candidates(600)                               # ... and with an online matrix that covers candidates
    _append(eng, g, arr[half:])
    b, a, rep = eng.run_online(want_bits=True)
    assert same((b, a), b_full, a_full) and rep["grew"] == 0 and rep["covered_before"] == half and rep["set_max_resumed"] == 1
    assert same(eng.run(), b_full, a_full)
    acc_set, _ = eng.run_set_only()
    assert acc_set.tobytes() == a_full.tobytes()
    eng.close()
    # the faithful mode: a reserve in the middle of the checks leaves the records of an undisturbed run, bitwise
    full = _stub(g, g.V, arr)
    plain, moved = _engine(full, cfg), _engine(full, cfg)
    order = [int(k) for k in plain.candidate_order()]
    plain.reset(), moved.reset()
    want = [plain.agreementCheck(k, with_info=True) for k in order]
    got = []
    for q, k in enumerate(order):
        if q == len(order) // 3:
            moved.reserve_candidates(300)
        got.append(moved.agreementCheck(k, with_info=True))
    assert [(ok, bytes(info)) for ok, info in got] == [(ok, bytes(info)) for ok, info in want]
    assert same(moved.run(), b_full, a_full)
    plain.close(), moved.close()


def test_c2_streamed_in_bursts():
    """Full size: the C2 bench workload (1 256 candidates), streamed in processing order in bursts of 50."""
    import bench
    g, cfg, _ = bench.build_workload("C2")
    arr = _arrival(g)
    batch = _engine(_stub(g, g.V, arr), cfg)
    bits_ref, acc_ref = batch.run()
    cells_ref = batch.solve_report()["cells"]
    batch.close()
    eng = _engine(_stub(g), cfg)
    cells, grown = 0, 0
    for done in range(0, g.N, 50):
        _append(eng, g, arr[done:done + 50])
        acc, rep = eng.run_online()
        assert rep["set_max_resumed"] == (1 if done else 0)
        cells += rep["cells"]
        grown += rep["grew"]
    bits, acc2, rep = eng.run_online(want_bits=True)
    assert rep["cells"] == 0 and eng.online_covered == g.N == 1256
    print("C2 streamed: %d cells in %d updates, %d storage growths" % (cells, (g.N + 49) // 50, grown))
    assert cells == cells_ref
    assert acc.tobytes() == acc2.tobytes() == acc_ref.tobytes()
    assert bits.tobytes() == bits_ref.tobytes()
