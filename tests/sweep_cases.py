"""Graphs, threshold pairs and reference runs shared by tests/test_sweep_api.py and tests/test_gpu_sweep.py.

A reference result is ALWAYS a fresh engine created with the pair in its Config and one run() -- never the sweep itself.  The
references are computed once per (graph, candidate selection, environment, pair) and shared between the tests; nothing changes
them afterwards."""
import os

import numpy as np

# (fast_reject_th, slow_reject_th): the reference's default, its experiment scripts' override, two tight pairs, a loose one and the
# default swapped (fast > slow)
PAIRS = [(6.251, 11.345), (10.64, 10.64), (2.0, 4.0), (0.5, 1.0), (30.0, 60.0), (11.345, 6.251)]
# the pairs at which the oracle's chi2 stays >= 1.3 % clear of every threshold on both small graphs
ORACLE_PAIRS = [(6.251, 11.345), (10.64, 10.64), (0.5, 1.0), (30.0, 60.0)]
ENV_KEYS = ("IPC_TERMINATE_EPS", "IPC_BORDERLINE_BAND", "IPC_LM_RETRY", "IPC_SE2_POLICY", "IPC_SE3_POLICY", "IPC_SE3_LATENCY_POLICY",
            "IPC_SWEEP_CHUNK")

_graphs = {}
_fresh = {}


def graph(name):
    """"se2": 400 vertices, 40 candidates, 557 pair cells; "se3": the 128-vertex, 36-candidate sphere subset; "wide": 200 SE2
    candidates; "long": 120 SE2 vertices, 12 candidates, spans beyond the one-wave kernel of 64 poses."""
    if name not in _graphs:
        from ipc_amd import synth
        if name == "se2":
            g = synth.inject_outliers(synth._se2_graph(400, 24, seed=75, laps=3.0, name="inc"), 16, seed=5)
        elif name == "se3":
            s = synth.sphere_like(rings=8, per_ring=16, radius=8.0)
            g = synth.inject_outliers(s.subset(np.arange(0, s.N, max(1, s.N // 24))), 8, seed=6)
        elif name == "wide":
            g = synth.inject_outliers(synth._se2_graph(400, 150, seed=76, laps=3.0, name="wide"), 50, seed=7)
        elif name == "long":
            g = synth.inject_outliers(synth._se2_graph(120, 8, seed=78, laps=2.0, name="long"), 4, seed=9)
        else:
            raise KeyError(name)
        _graphs[name] = g
    return _graphs[name]


def config(g, fast=6.251, slow=11.345):
    from ipc_amd.consensus import Config
    return Config(s_factor=10.0 if g.dim == 2 else 50.0, fast_reject_th=float(fast), slow_reject_th=float(slow))


def arrival(g):
    """File indices by later vertex, ties in file order (the engine's processing order)."""
    return [int(k) for k in np.argsort(g.loop_ids.max(axis=1), kind="stable")]


def stub(g, V=None, sel=None):
    """The graph as far as its first V vertices (default: all), with the candidates `sel` (default: all) in that order."""
    from ipc_amd.graphio import PoseGraph
    V = g.V if V is None else V
    sel = np.arange(g.N) if sel is None else np.asarray(sel, dtype=np.int64)
    return PoseGraph(g.dim, g.vertices[:V], g.odom_meas[:V - 1], g.odom_info[:V - 1],
                     g.loop_ids[sel].reshape(-1, 2), g.loop_meas[sel], g.loop_info[sel], dict(g.meta))


def engine(g, fast=6.251, slow=11.345):
    from ipc_amd.consensus import IPC
    return IPC(g, config(g, fast, slow), device=0)


def _env_key():
    return tuple(os.environ.get(k, "") for k in ENV_KEYS)


def fresh(key, g, fast, slow):
    """(bits, accepted, solve report) of a fresh engine's run() at the pair, under the environment of the moment.  `key` names
    the graph and the candidate selection `g` was made from."""
    k = (key, _env_key(), float(fast), float(slow))
    if k not in _fresh:
        eng = engine(g, fast, slow)
        bits, acc = eng.run()
        rep = eng.solve_report()
        eng.close()
        bits.setflags(write=False), acc.setflags(write=False)
        _fresh[k] = (bits, acc, rep)
    return _fresh[k]


def assert_sweep_equals_fresh(key, g, pairs, bits, acc):
    """Every entry of a sweep's output against the fresh engine of its pair, byte for byte."""
    assert acc.shape == (len(pairs), g.N)
    for t, (f, s) in enumerate(pairs):
        b_ref, a_ref, _ = fresh(key, g, f, s)
        assert acc[t].tobytes() == a_ref.tobytes(), (key, t, f, s)
        if bits is not None:
            assert bits[t].tobytes() == b_ref.tobytes(), (key, t, f, s)


def ok_from_chi2(g, mx, fast, slow):
    """The decision rule on a matrix of max chi2: the diagonal against `fast`, overlapping pairs against `slow` (NaN agrees,
    reference src/consensus_utils.cpp:18), any other pair ok[i][i] & ok[j][j] (src/consensus.cpp:157-159)."""
    lo, hi = g.loop_ids.min(axis=1), g.loop_ids.max(axis=1)
    N = g.N
    ok = np.zeros((N, N), dtype=np.uint8)
    d = ~(np.diag(mx) > fast)
    for i in range(N):
        for j in range(N):
            if i == j:
                ok[i, j] = d[i]
            elif min(hi[i], hi[j]) - max(lo[i], lo[j]) > 0:
                ok[i, j] = not (mx[i, j] > slow)
            else:
                ok[i, j] = d[i] and d[j]
    return ok
