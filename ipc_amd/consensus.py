"""Host-side mirror of the reference's consensus interface over the C ABI.

`IPC` follows the surface of the reference's `template<class EDGE, class VERTEX> class IPC`
(reference include/ipc/consensus.hpp:5-33): constructed from the open-loop problem and a
Config, it owns the consensus set.  The batched entry points (`consistency_matrix`,
`max_consensus_set`) are the MI355X re-formulation of the per-candidate `agreementCheck` loop
(reference src/simulation.cpp:34-47): all cells of the N x N consistency matrix are solved in
one pass on the GPU, then the consistent set is grown in the reference's candidate order.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi
from .graphio import PoseGraph


@dataclass
class Config:
    """The hot-path fields of the reference's struct Config (include/ipc/utils.hpp:22-38)."""
    fast_reject_th: float = 6.251
    fast_reject_iter_base: int = 50
    slow_reject_th: float = 11.345
    slow_reject_iter_base: int = 100
    s_factor: float = 10.0
    canonic_inliers: int = 0


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class IPC:
    def __init__(self, graph: PoseGraph, cfg: Config, device: int = 0):
        self.lib = capi.load()
        self.graph, self.cfg, self.device = graph, cfg, device
        self.dim = graph.dim
        prm = capi.Params(cfg.fast_reject_th, cfg.fast_reject_iter_base, cfg.slow_reject_th,
                          cfg.slow_reject_iter_base, cfg.s_factor)
        om, oi = _d(graph.odom_meas), _d(graph.odom_info)
        h = C.c_void_p()
        capi.check(self.lib.ipc_create(graph.dim, graph.V, _p(om), _p(oi), C.byref(prm), device, C.byref(h)))
        self.h = h
        self.N = 0
        self._max_consensus_set = np.zeros(0, dtype=np.int32)
        if graph.N:
            self.set_candidates(graph.loop_ids, graph.loop_meas, graph.loop_info)

    # ---- candidates ---------------------------------------------------------------------
    def set_candidates(self, ids, meas, info):
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1, 2)
        meas, info = _d(meas), _d(info)
        capi.check(self.lib.ipc_set_candidates(self.h, ids.shape[0], _p(ids), _p(meas), _p(info)))
        self.N = ids.shape[0]
        self.ids = ids

    def append_candidate(self, ids, meas, info):
        """One more candidate at the end of the list (ipc_append_candidate: the harness hands agreementCheck an edge
        nobody announced, reference src/simulation.cpp:34-47); returns its index.  State and solves in flight stay."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(2)
        meas, info = _d(meas), _d(info)
        k = C.c_int(-1)
        capi.check(self.lib.ipc_append_candidate(self.h, _p(ids), _p(meas), _p(info), C.byref(k)))
        self.N = k.value + 1
        self.ids = np.vstack([self.ids, ids.reshape(1, 2)]) if self.N > 1 else ids.reshape(1, 2).copy()
        return k.value

    # ---- online mode: the chain grows in place ---------------------------------------------
    @property
    def n_vertices(self):
        """Vertex count of the moment (ipc_vertex_count): graph.V plus what append_odometry added."""
        n = C.c_int(0)
        capi.check(self.lib.ipc_vertex_count(self.h, C.byref(n)))
        return n.value

    def append_odometry(self, meas, info):
        """Odometry edges V-1 -> V, V -> V+1, ... appended in place (ipc_append_odometry): meas [n, 3|7] (or one record),
        info [n, 6|21].  Poses, consensus set and the solves in flight stay; returns the new vertex count."""
        ms, ns = (3, 6) if self.dim == 2 else (7, 21)
        meas, info = _d(meas).reshape(-1, ms), _d(info).reshape(-1, ns)
        assert meas.shape[0] == info.shape[0]
        capi.check(self.lib.ipc_append_odometry(self.h, int(meas.shape[0]), _p(meas), _p(info)))
        return self.n_vertices

    def reserve_vertices(self, n):
        """Room for n vertices up front (ipc_reserve_vertices): appends up to there never grow the arrays."""
        capi.check(self.lib.ipc_reserve_vertices(self.h, int(n)))

    def candidate_order(self):
        order = np.zeros(self.N, dtype=np.int32)
        capi.check(self.lib.ipc_candidate_order(self.h, _p(order)))
        return order

    def initial_poses(self):
        ps = 3 if self.dim == 2 else 12
        out = np.zeros((self.n_vertices, ps))
        capi.check(self.lib.ipc_initial_poses(self.h, _p(out)))
        return out

    @property
    def words(self):
        return (self.N + 63) // 64

    # ---- single-GPU batch path ------------------------------------------------------------
    def run(self):
        """Solve the matrix and grow the consensus set; returns (bits [N, words] uint64,
        accepted [N] uint8)."""
        bits = np.zeros((self.N, self.words), dtype=np.uint64)
        acc = np.zeros(self.N, dtype=np.uint8)
        capi.check(self.lib.ipc_run(self.h, _p(bits), _p(acc)))
        order = self.candidate_order()
        self._max_consensus_set = order[acc[order] == 1]
        return bits, acc

    def run_set_only(self):
        """The accepted set of run() without the cells the set-max never reads (diagonal first, then the pairs among the
        candidates whose own cell passed); returns (accepted [N] uint8, cells actually solved)."""
        acc = np.zeros(self.N, dtype=np.uint8)
        n = C.c_int(0)
        capi.check(self.lib.ipc_run_set_only(self.h, _p(acc), C.byref(n)))
        order = self.candidate_order()
        self._max_consensus_set = order[acc[order] == 1]
        return acc, n.value

    # ---- online matrix mode: the matrix stays on the device, an update solves the new columns ----
    def run_online(self, want_bits=False):
        """ipc_run_online: solve the cells of the candidates appended since the last call, extend the stored matrix and the
        accepted set.  Returns (accepted [N] uint8, report dict), or (bits [N, words] uint64, accepted, report) with
        want_bits; the results are those of run() on the same list."""
        acc = np.zeros(self.N, dtype=np.uint8)
        bits = np.zeros((self.N, self.words), dtype=np.uint64) if want_bits else None
        r = capi.OnlineReport()
        capi.check(self.lib.ipc_run_online(self.h, _p(bits) if want_bits else None, _p(acc), C.byref(r)))
        order = self.candidate_order()
        self._max_consensus_set = order[acc[order] == 1]
        report = {k: getattr(r, k) for k, _ in capi.OnlineReport._fields_}
        return (bits, acc, report) if want_bits else (acc, report)

    @property
    def online_covered(self):
        """How many candidates the online matrix covers (ipc_online_covered)."""
        m = C.c_int(0)
        capi.check(self.lib.ipc_online_covered(self.h, C.byref(m)))
        return m.value

    def online_reset(self):
        """Forget the online matrix (ipc_online_reset): the next run_online solves every cell."""
        capi.check(self.lib.ipc_online_reset(self.h))

    def run_online_exact(self, want_bits=False):
        """ipc_run_online_exact: the update of run_online(), then the exact set of the stored matrix, resumed from the proven set
        the engine holds where it has one.  Returns (accepted [N] uint8, greedy [N] uint8, online report dict, report dict), with
        want_bits (bits [N, words] uint64, accepted, greedy, online report, report); bits, greedy and the online report are
        those of run_online().  report["proven"] = 1: accepted is a maximum consistent set of report["size"] members.
        getMaxConsensusSet() is left as it was."""
        acc = np.zeros(self.N, dtype=np.uint8)
        greedy = np.zeros(self.N, dtype=np.uint8)
        bits = np.zeros((self.N, self.words), dtype=np.uint64) if want_bits else None
        o, r = capi.OnlineReport(), capi.ExactResumeReport()
        capi.check(self.lib.ipc_run_online_exact(self.h, _p(bits) if want_bits else None, _p(acc), _p(greedy), C.byref(o), C.byref(r)))
        online = {k: getattr(o, k) for k, _ in capi.OnlineReport._fields_}
        report = {k: getattr(r, k) for k, _ in capi.ExactResumeReport._fields_}
        return (bits, acc, greedy, online, report) if want_bits else (acc, greedy, online, report)

    @property
    def online_exact_state(self):
        """(covered, proven) of the exact set the engine holds for run_online_exact (ipc_online_exact_state); (0, 0): none."""
        c, p = C.c_int(0), C.c_int(0)
        capi.check(self.lib.ipc_online_exact_state(self.h, C.byref(c), C.byref(p)))
        return c.value, p.value

    def reserve_candidates(self, n):
        """Room for n candidates up front, in the candidate arrays and the online matrix (ipc_reserve_candidates)."""
        capi.check(self.lib.ipc_reserve_candidates(self.h, int(n)))

    # ---- threshold sweep: the cells solved once, decided at many (fast_reject_th, slow_reject_th) pairs ----
    def run_sweep(self, fast_ths, slow_ths, want_bits=False):
        """ipc_run_sweep: entry t is what run() returns on an engine created with fast_reject_th = fast_ths[t] and
        slow_reject_th = slow_ths[t] (everything else this engine's).  Returns (accepted [T, N] uint8, report dict), or
        (bits [T, N, words] uint64, accepted, report) with want_bits.  A sweep has no single set: getMaxConsensusSet()
        is left as it was."""
        fast, slow = _d(fast_ths).reshape(-1), _d(slow_ths).reshape(-1)
        assert fast.shape == slow.shape
        T = int(fast.shape[0])
        acc = np.zeros((T, self.N), dtype=np.uint8)
        bits = np.zeros((T, self.N, self.words), dtype=np.uint64) if want_bits else None
        r = capi.SweepReport()
        capi.check(self.lib.ipc_run_sweep(self.h, T, _p(fast), _p(slow), _p(bits) if want_bits else None, _p(acc), C.byref(r)))
        report = {k: getattr(r, k) for k, _ in capi.SweepReport._fields_}
        return (bits, acc, report) if want_bits else (acc, report)

    def sweep_reset(self):
        """Forget the sweep's held first pass (ipc_sweep_reset): the next run_sweep solves every cell."""
        capi.check(self.lib.ipc_sweep_reset(self.h))

    # ---- Monte-Carlo batch: the cells solved once, assembled into many candidate lists ----
    def run_batch(self, runs, want_bits=False):
        """ipc_run_batch: `runs` is a list of int arrays, each a strictly increasing selection of this engine's candidates (the
        union list); entry r is what run() returns on a fresh engine given those candidates in that order.  Returns (list of
        accepted [N_r] uint8, report dict), or (list of bits [N_r, words_r] uint64, list of accepted, report) with want_bits.
        A batch has no single set: getMaxConsensusSet() is left as it was."""
        runs = [np.ascontiguousarray(r, dtype=np.int32).reshape(-1) for r in runs]
        sizes = [int(r.shape[0]) for r in runs]
        offsets = np.zeros(len(runs) + 1, dtype=np.int32)
        offsets[1:] = np.cumsum(sizes)
        members = np.ascontiguousarray(np.concatenate(runs) if runs else np.zeros(0), dtype=np.int32)
        mats = [n * ((n + 63) // 64) for n in sizes]
        acc = np.zeros(max(int(offsets[-1]), 1), dtype=np.uint8)
        bits = np.zeros(max(sum(mats), 1), dtype=np.uint64) if want_bits else None
        r = capi.BatchReport()
        capi.check(self.lib.ipc_run_batch(self.h, len(runs), _p(offsets), _p(members), _p(bits) if want_bits else None, _p(acc),
                                          C.byref(r)))
        report = {k: getattr(r, k) for k, _ in capi.BatchReport._fields_}
        accs = [acc[offsets[q]:offsets[q + 1]] for q in range(len(runs))]
        if not want_bits:
            return accs, report
        mo = np.concatenate([[0], np.cumsum(mats)])
        return [bits[mo[q]:mo[q + 1]].reshape(sizes[q], -1) for q in range(len(runs))], accs, report

    def run_batch_exact(self, runs, want_bits=False):
        """ipc_run_batch_exact: run_batch(), and per run the multi-start and the exact set as well: entry r is what run_exact()
        returns on a fresh engine given those candidates in that order.  Returns (list of accepted [N_r] uint8, list of
        multistart, list of greedy -- run_batch()'s sets --, list of exact report dicts, batch report dict, batch-exact report
        dict), with want_bits the list of bits [N_r, words_r] uint64 in front.  getMaxConsensusSet() is left as it was."""
        runs = [np.ascontiguousarray(r, dtype=np.int32).reshape(-1) for r in runs]
        sizes = [int(r.shape[0]) for r in runs]
        offsets = np.zeros(len(runs) + 1, dtype=np.int32)
        offsets[1:] = np.cumsum(sizes)
        members = np.ascontiguousarray(np.concatenate(runs) if runs else np.zeros(0), dtype=np.int32)
        mats = [n * ((n + 63) // 64) for n in sizes]
        acc, ms, greedy = (np.zeros(max(int(offsets[-1]), 1), dtype=np.uint8) for _ in range(3))
        bits = np.zeros(max(sum(mats), 1), dtype=np.uint64) if want_bits else None
        reps = (capi.ExactReport * max(len(runs), 1))()
        r, x = capi.BatchReport(), capi.BatchExactReport()
        capi.check(self.lib.ipc_run_batch_exact(self.h, len(runs), _p(offsets), _p(members), _p(bits) if want_bits else None, _p(greedy),
                                                _p(ms), _p(acc), C.byref(r), C.cast(reps, C.c_void_p), C.byref(x)))
        cut = lambda a: [a[offsets[q]:offsets[q + 1]] for q in range(len(runs))]
        reports = [{k: getattr(reps[q], k) for k, _ in capi.ExactReport._fields_} for q in range(len(runs))]
        out = (cut(acc), cut(ms), cut(greedy), reports, {k: getattr(r, k) for k, _ in capi.BatchReport._fields_},
               {k: getattr(x, k) for k, _ in capi.BatchExactReport._fields_})
        if not want_bits:
            return out
        mo = np.concatenate([[0], np.cumsum(mats)])
        return ([bits[mo[q]:mo[q + 1]].reshape(sizes[q], -1) for q in range(len(runs))],) + out

    # ---- multi-start set maximisation: the greedy from every live seed, the largest set ----
    def run_multistart(self, want_bits=False):
        """ipc_run_multistart: solve and assemble as run(), then the greedy set of run() AND the multi-start set from the one
        matrix.  Returns (accepted [N] uint8, greedy [N] uint8, sizes [N] int32, report dict), with want_bits
        (bits [N, words] uint64, accepted, greedy, sizes, report); bits and greedy are those of run().  getMaxConsensusSet() is
        left as it was."""
        acc = np.zeros(self.N, dtype=np.uint8)
        greedy = np.zeros(self.N, dtype=np.uint8)
        sizes = np.zeros(self.N, dtype=np.int32)
        bits = np.zeros((self.N, self.words), dtype=np.uint64) if want_bits else None
        r = capi.MultistartReport()
        capi.check(self.lib.ipc_run_multistart(self.h, _p(bits) if want_bits else None, _p(acc), _p(greedy), _p(sizes), C.byref(r)))
        report = {k: getattr(r, k) for k, _ in capi.MultistartReport._fields_}
        return (bits, acc, greedy, sizes, report) if want_bits else (acc, greedy, sizes, report)

    # ---- exact maximum consistent set: branch-and-bound with the multi-start set as the lower bound ----
    def run_exact(self, want_bits=False):
        """ipc_run_exact: solve and assemble as run(), then the multi-start set AND the exact set from the one matrix.  Returns
        (accepted [N] uint8, multistart [N] uint8, report dict), with want_bits (bits [N, words] uint64, accepted, multistart,
        report).  report["proven"] = 1: accepted is a maximum consistent set of report["size"] members; 0: accepted is the
        multi-start set and the optimum lies in [size, upper_bound].  getMaxConsensusSet() is left as it was."""
        acc = np.zeros(self.N, dtype=np.uint8)
        ms = np.zeros(self.N, dtype=np.uint8)
        bits = np.zeros((self.N, self.words), dtype=np.uint64) if want_bits else None
        r = capi.ExactReport()
        capi.check(self.lib.ipc_run_exact(self.h, _p(bits) if want_bits else None, _p(acc), _p(ms), C.byref(r)))
        report = {k: getattr(r, k) for k, _ in capi.ExactReport._fields_}
        return (bits, acc, ms, report) if want_bits else (acc, ms, report)

    # ---- census of the maximum consistent sets: how many there are, what they share, what any of them holds ----
    def run_census(self, want_bits=False):
        """ipc_run_census: run_exact()'s matrix and exact set, then the census of the maximum consistent sets.  Returns (accepted
        [N] uint8, core [N] uint8, support [N] uint8, exact report dict, census report dict), with want_bits the bits [N, words]
        uint64 in front; bits, accepted and the exact report are those of run_exact().  census["proven"] = 1: there are
        census["count"] maximum sets, core marks the candidates in all of them and support those in any; 0: count is a lower
        bound (0 where the exact stage proved nothing), core is empty and support is the live candidates.
        getMaxConsensusSet() is left as it was."""
        acc, core, support = (np.zeros(self.N, dtype=np.uint8) for _ in range(3))
        bits = np.zeros((self.N, self.words), dtype=np.uint64) if want_bits else None
        r, c = capi.ExactReport(), capi.CensusReport()
        capi.check(self.lib.ipc_run_census(self.h, _p(bits) if want_bits else None, _p(acc), _p(core), _p(support), C.byref(r), C.byref(c)))
        exact = {k: getattr(r, k) for k, _ in capi.ExactReport._fields_}
        census = {k: getattr(c, k) for k, _ in capi.CensusReport._fields_}
        return (bits, acc, core, support, exact, census) if want_bits else (acc, core, support, exact, census)

    def consistency_matrix(self):
        bits, _ = self.run()
        return unpack_bits(bits, self.N)

    def getMaxConsensusSet(self):
        """Candidate indices in acceptance order (reference consensus.hpp:16)."""
        return self._max_consensus_set

    # ---- the reference's own per-candidate interface (faithful incremental mode) -------------
    def reset(self):
        """State right after the constructor (reference src/consensus.cpp:23-27)."""
        capi.check(self.lib.ipc_incremental_reset(self.h))
        self._max_consensus_set = np.zeros(0, dtype=np.int32)

    def agreementCheck(self, k, with_info=False):
        """IPC::agreementCheck (reference src/consensus.cpp:43-75) for candidate k (file index):
        cluster solve from the current state on the GPU; True when every edge passes."""
        ok, info = C.c_int(0), capi.CheckInfo()
        capi.check(self.lib.ipc_agreement_check(self.h, int(k), C.byref(ok), C.byref(info)))
        self._max_consensus_set = self._consensus()
        return (bool(ok.value), info) if with_info else bool(ok.value)

    def _consensus(self):
        n = C.c_int(0)
        capi.check(self.lib.ipc_consensus_size(self.h, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int32)
        capi.check(self.lib.ipc_consensus_set(self.h, _p(out)))
        return out[:n.value]

    def removeEdgeFromCnS(self, k):
        """IPC::removeEdgeFromCnS (reference src/consensus.cpp:77-96)."""
        r = C.c_int(0)
        capi.check(self.lib.ipc_remove_from_consensus(self.h, int(k), C.byref(r)))
        self._max_consensus_set = self._consensus()
        return bool(r.value)

    def addEdgeToCnS(self, k):
        """IPC::addEdgeToCnS (reference src/consensus.cpp:98-119)."""
        capi.check(self.lib.ipc_add_to_consensus(self.h, int(k)))
        self._max_consensus_set = self._consensus()

    def current_poses(self):
        out = np.zeros((self.n_vertices, 3 if self.dim == 2 else 12))
        capi.check(self.lib.ipc_current_poses(self.h, _p(out)))
        return out

    def set_state(self, poses, consensus, resume_position=0):
        """Resume the agreementCheck loop from a saved (current_poses(), getMaxConsensusSet()) pair
        (ipc_incremental_set_state; the two are all the state of reference include/ipc/consensus.hpp:23-32)."""
        poses = _d(poses)
        assert poses.shape == (self.n_vertices, 3 if self.dim == 2 else 12)
        cns = np.ascontiguousarray(consensus, dtype=np.int32)
        capi.check(self.lib.ipc_incremental_set_state(self.h, _p(poses), _p(cns), int(cns.shape[0]), int(resume_position)))
        self._max_consensus_set = cns.copy()

    def incremental_counters(self):
        """dict(host_solver_fallbacks, lost_launches, relaunches, literal_band_solves) -- ipc_incremental_counters."""
        c = capi.IncrementalCounters()
        capi.check(self.lib.ipc_incremental_counters(self.h, C.byref(c)))
        return {k: getattr(c, k) for k, _ in capi.IncrementalCounters._fields_}

    def final_optimize(self, accepted, iterations=1000):
        """The harness's final map (reference src/simulation.cpp:50-65): returns (poses [V,3] or
        [V,12] (R row-major, t), CheckInfo with chi2_total)."""
        acc = np.ascontiguousarray(accepted, dtype=np.uint8)
        out = np.zeros((self.n_vertices, 3 if self.dim == 2 else 12))
        info = capi.CheckInfo()
        capi.check(self.lib.ipc_final_optimize(self.h, _p(acc), int(iterations), _p(out), C.byref(info)))
        return out, info

    # ---- device-pointer stages (multi-GPU plumbing lives in ipc_amd.dist) -------------------
    def rows_per_rank(self, world):
        return self.lib.ipc_rows_per_rank(self.N, world)

    def solve_rows(self, rank, world, d_upper_ptr, stream=0):
        capi.check(self.lib.ipc_solve_rows(self.h, rank, world, C.c_void_p(d_upper_ptr), C.c_void_p(stream)))

    def assemble_matrix(self, d_gathered_ptr, world, d_bits_ptr, stream=0):
        capi.check(self.lib.ipc_assemble_matrix(self.h, C.c_void_p(d_gathered_ptr), world,
                                                C.c_void_p(d_bits_ptr), C.c_void_p(stream)))

    def set_max(self, d_bits_ptr, d_accepted_ptr, stream=0):
        capi.check(self.lib.ipc_set_max(self.h, C.c_void_p(d_bits_ptr), C.c_void_p(d_accepted_ptr),
                                        C.c_void_p(stream)))

    def set_max_multistart(self, d_bits_ptr, d_accepted_ptr, d_sizes_ptr=0, stream=0):
        capi.check(self.lib.ipc_set_max_multistart(self.h, C.c_void_p(d_bits_ptr), C.c_void_p(d_accepted_ptr),
                                                   C.c_void_p(d_sizes_ptr) if d_sizes_ptr else None, C.c_void_p(stream)))

    def set_max_exact(self, d_bits_ptr, d_accepted_ptr, stream=0):
        """ipc_set_max_exact on device pointers; blocks until the search is over and returns the report as a dict."""
        r = capi.ExactReport()
        capi.check(self.lib.ipc_set_max_exact(self.h, C.c_void_p(d_bits_ptr), C.c_void_p(d_accepted_ptr), C.byref(r), C.c_void_p(stream)))
        return {k: getattr(r, k) for k, _ in capi.ExactReport._fields_}

    def set_max_census(self, d_bits_ptr, d_accepted_ptr, d_core_ptr, d_support_ptr, stream=0):
        """ipc_set_max_census on device pointers; blocks until the census is over and returns (exact report dict, census report
        dict)."""
        r, c = capi.ExactReport(), capi.CensusReport()
        capi.check(self.lib.ipc_set_max_census(self.h, C.c_void_p(d_bits_ptr), C.c_void_p(d_accepted_ptr), C.c_void_p(d_core_ptr),
                                               C.c_void_p(d_support_ptr), C.byref(r), C.byref(c), C.c_void_p(stream)))
        return ({k: getattr(r, k) for k, _ in capi.ExactReport._fields_}, {k: getattr(c, k) for k, _ in capi.CensusReport._fields_})

    def set_max_batch_exact(self, run_n, order, d_bits_ptr, d_accepted_ptr, d_multistart_ptr=0, d_greedy_ptr=0, stream=0):
        """ipc_set_max_batch_exact on device pointers: run_n [R] and order (the runs' processing orders back to back) are host
        arrays.  Blocks until the search is over; returns (list of exact report dicts, batch-exact report dict)."""
        run_n = np.ascontiguousarray(run_n, dtype=np.int32).reshape(-1)
        order = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
        reps = (capi.ExactReport * max(len(run_n), 1))()
        x = capi.BatchExactReport()
        opt = lambda p: C.c_void_p(p) if p else None
        capi.check(self.lib.ipc_set_max_batch_exact(self.h, len(run_n), _p(run_n), _p(order), C.c_void_p(d_bits_ptr), opt(d_greedy_ptr),
                                                    opt(d_multistart_ptr), C.c_void_p(d_accepted_ptr), C.cast(reps, C.c_void_p), C.byref(x),
                                                    C.c_void_p(stream)))
        return ([{k: getattr(reps[q], k) for k, _ in capi.ExactReport._fields_} for q in range(len(run_n))],
                {k: getattr(x, k) for k, _ in capi.BatchExactReport._fields_})

    def set_max_exact_resume(self, d_bits_ptr, first, d_accepted_ptr, stream=0):
        """ipc_set_max_exact_resume on device pointers; blocks until the search is over and returns the report as a dict."""
        r = capi.ExactResumeReport()
        capi.check(self.lib.ipc_set_max_exact_resume(self.h, C.c_void_p(d_bits_ptr), int(first), C.c_void_p(d_accepted_ptr), C.byref(r),
                                                     C.c_void_p(stream)))
        return {k: getattr(r, k) for k, _ in capi.ExactResumeReport._fields_}

    # ---- diagnostics ----------------------------------------------------------------------
    def cell_info(self):
        n = C.c_int(0)
        capi.check(self.lib.ipc_cell_count(self.h, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=capi.CELL_DTYPE)
        capi.check(self.lib.ipc_cell_info(self.h, _p(out), n.value))
        return out[:n.value]

    def solve_report(self):
        """Counts over the cells of the last solve: dict(cells, long_cells, failed_cells, capped_cells, nan_cells)."""
        r = capi.SolveReport()
        capi.check(self.lib.ipc_solve_report(self.h, C.byref(r)))
        return {k: getattr(r, k) for k, _ in capi.SolveReport._fields_}

    def lazy_sd_launches(self):
        """Launches of a lazy steepest-descent SE2 cell kernel since this engine was created (0 with IPC_SE2_LAZY_SD=0)."""
        n = C.c_longlong(0)
        capi.check(self.lib.ipc_se2_lazy_sd_launches(self.h, C.byref(n)))
        return n.value

    def solver_time_ms(self):
        ms, nl = C.c_double(0), C.c_int(0)
        capi.check(self.lib.ipc_solver_time_ms(self.h, C.byref(ms), C.byref(nl)))
        return ms.value, nl.value

    def synchronize(self):
        capi.check(self.lib.ipc_synchronize(self.h))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.ipc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def unpack_bits(bits, N):
    """[N, words] uint64 -> [N, N] uint8."""
    b = np.ascontiguousarray(bits, dtype=np.uint64)
    u8 = b.view(np.uint8).reshape(b.shape[0], -1)
    return np.unpackbits(u8, axis=1, bitorder="little")[:, :N].astype(np.uint8)
