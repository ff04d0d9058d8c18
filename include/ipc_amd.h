/*
 * ipc_amd.h -- C ABI of the MI355X-native IPC consistency engine (libipc_amd.so).
 *
 * Drop-in boundary for the hot path of EmilioOlivastri/IPC: everything the reference does
 * between "here is the odometry chain + the loop-closure candidates" and "this candidate set
 * is consistent".  Each entry point names the reference interface it replaces (file:line in
 * the reference tree).  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - every function returns 0 on success and a negative ipc_status on failure, never throws,
 *     never aborts; ipc_last_error() returns a human-readable message for the calling thread.
 *   - measurements / information matrices use the g2o text-file layout the reference loads
 *     (src/utils.cpp:114): SE2 "x y theta" + 6 upper-triangular information values;
 *     SE3 "x y z qx qy qz qw" + 21 upper-triangular values in (x y z qx qy qz) order.
 *   - vertex ids are 0..V-1 and odometry edge j joins vertex j -> j+1 (the reference's own
 *     contract, src/consensus.cpp:13-23).
 *   - pointers named d_* are DEVICE pointers (HBM of the engine's GPU), everything else is
 *     host memory.  `stream` is a hipStream_t passed as void* (NULL = the engine's own
 *     NON-BLOCKING stream, which is not ordered with the legacy default stream: pass an explicit
 *     stream when other work, e.g. a collective, must be ordered with the call).
 *   - a handle is bound to one GPU and must not be used from two threads at once (the
 *     reference's IPC object is not re-entrant either).
 *   - environment: the faithful mode keeps up to 16 solves in flight, one per HIP stream; streams that share a hardware
 *     queue run one after the other and the runtime's default is 4 queues.  The HOST PROGRAM exports
 *     GPU_MAX_HW_QUEUES=24 before its first HIP call for full speed (the library does not touch the environment: round 5;
 *     ipc_tester_2D/3D and bench.py do it in their main, INTEGRATION.md shows the line for the reference's testers).
 *     Without it the window is 4 solves and a probe measures how many streams really run abreast.  IPC_SPEC_STATS=1 prints how many
 *     of the engine's streams were measured to run side by side.  The order in which the pipeline starts its solves
 *     follows a prediction of each verdict (the candidate's own chi2 at the poses it starts from; IPC_SPEC_PREDICT,
 *     INTEGRATION.md): predictions schedule, no result depends on them.
 */
#ifndef IPC_AMD_H
#define IPC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ipc_engine ipc_engine_t;

typedef enum {
    IPC_OK = 0,
    IPC_ERR_ARG = -1,        /* bad argument / out-of-contract graph        */
    IPC_ERR_HIP = -2,        /* HIP runtime failure (message has the detail) */
    IPC_ERR_STATE = -3,      /* call order (e.g. no candidates set)          */
    IPC_ERR_LIMIT = -4       /* a size the engine cannot hold (ipc_set_max: N beyond the LDS-resident mask);
                                chains of any length are solved -- see ipc_solve_rows */
} ipc_status;

/* The knobs the path reads: struct Config fields used by IPC::IPC
 * (reference include/ipc/utils.hpp:22-38, src/consensus.cpp:18-32). */
typedef struct {
    double fast_reject_th;
    int    fast_reject_iter_base;
    double slow_reject_th;
    int    slow_reject_iter_base;
    double s_factor;
} ipc_params_t;

/* Per-cell diagnostics of the last ipc_solve_rows() (parity tests, profiling). */
typedef struct {
    int    i, j;             /* candidate indices (i == j: diagonal cell)   */
    int    lo, hi;           /* vertex-id span of the sub-problem           */
    double max_chi2;         /* max over the cell's edges of chi2           */
    double chi2_total;       /* sum of chi2 at exit                          */
    int    iterations;       /* dog-leg outer iterations executed            */
    int    tries;            /* total trial steps                            */
    int    flags;            /* bit0 Terminate, bit1 Fail                    */
    int    evals;            /* residual evaluations actually executed        */
} ipc_cell_info_t;

const char* ipc_last_error(void);

/* Replaces IPC<EDGE,VERTEX>::IPC (reference src/consensus.cpp:9-33): takes the odometry chain
 * (getProblemOdom + sort, :13-15), scales its information by s_factor (robustifyVoters, :21,
 * src/consensus_utils.cpp:124-130) and propagates the open-loop guess from vertex 0
 * (propagateGuess, :23, src/consensus_utils.cpp:99-116) -- all on the GPU `device`.
 * dim = 2 (SE2) or 3 (SE3). odom_meas [V-1][3|7], odom_info [V-1][6|21]. */
int ipc_create(int dim, int n_vertices, const double* odom_meas, const double* odom_info,
               const ipc_params_t* params, int device, ipc_engine_t** out);

/* Replaces IPC<EDGE,VERTEX>::~IPC (src/consensus.cpp:35-40). */
int ipc_destroy(ipc_engine_t* h);

/* The candidate list the harness feeds to agreementCheck one by one
 * (reference src/simulation.cpp:24-26,34-47): ids [N][2] (from,to), meas [N][3|7],
 * info [N][6|21], in FILE order; the engine applies the cmpTime processing order
 * (src/utils.cpp:379-390) with the (max id, index) tie-break. */
int ipc_set_candidates(ipc_engine_t* h, int n, const int* ids, const double* meas,
                       const double* info);

/* One more candidate at the END of the list (index N), without touching the incremental state: the consensus set
 * (candidate indices), the current poses and the solves the engine has in flight stay what they are.  For a harness that
 * meets its loop closures one by one (reference src/simulation.cpp:34-47 hands IPC::agreementCheck edges it has never
 * announced).  Cost: one record written in place by a one-thread kernel that carries it in its arguments -- no
 * re-upload, no allocation (the arrays grow geometrically, log2 N times over a run), no hipFree, no host
 * synchronisation.  *index_out = the new candidate's index. */
int ipc_append_candidate(ipc_engine_t* h, const int* ids, const double* meas, const double* info, int* index_out);

/* ---- online mode: the odometry chain grows in place -------------------------------------------------------------------
 * The reference's constructor takes a loaded graph (src/consensus.cpp:13-23); nothing in IPC::agreementCheck needs the whole
 * chain -- it reads the vertices up to the candidate's later one and re-propagates the tail.  A back end that meets its graph
 * one pose at a time extends the engine instead of rebuilding it.
 *
 * ipc_append_odometry appends n_edges >= 1 odometry edges V-1 -> V, V -> V+1, ... (meas [n][3|7], info [n][6|21], as
 * ipc_create).  For every new vertex: the chain record with its information scaled by s_factor (robustifyVoters,
 * src/consensus_utils.cpp:124-130) in every copy the engine keeps; the open-loop pose open[V] = open[V-1] (+) z[V-1]
 * (propagateGuess resumed, src/consensus_utils.cpp:99-116); and the current pose D (+) open[V] in the committed state and in every
 * tentative state of the look-ahead pipeline, D being the rigid transform the last accept applied to that state's tail
 * (propagateCurrentGuess, consensus_utils.cpp:61-71; a bit copy of open[V] before any accept and after ipc_incremental_reset).
 * All of it is bit for bit what an engine created with the whole chain holds -- records, poses, and every ipc_check_info_t
 * of the checks that follow.  After ipc_incremental_set_state there is no accept to take D from: D is then DEFINED from the
 * handed-over poses the same way, T = poses[V-1], P = open[V-1], D = T (+) P^-1; the bitwise claim is for runs without a state
 * injection after the last accept (the difference is rounding).
 * Cost within the capacity, one edge: one small kernel that carries the record in its arguments, one over the pose states, an
 * event the engine's other streams wait for before their next launch -- no allocation, no hipFree, no host synchronisation, the
 * solves in flight and the cached plan of the matrix mode stay.  Several edges go through a pinned buffer of the engine.
 * Beyond the capacity the arrays double (multiples of 64 vertices; the old ones are retired, not freed); a growth gives the
 * look-ahead up and waits for the device, log2 V times over a run.
 * ipc_reserve_vertices grows up front to `capacity` vertices (a caller that knows its mission length pays nothing later);
 * a capacity below the current one is a no-op.  ipc_vertex_count: the vertex count of the moment -- what ipc_initial_poses,
 * ipc_current_poses, ipc_incremental_set_state and ipc_final_optimize size their arrays by, and the bound on candidate ids.
 * ipc_run_sharded keeps demanding engines of equal vertex count. */
int ipc_append_odometry(ipc_engine_t* h, int n_edges, const double* meas, const double* info);
int ipc_reserve_vertices(ipc_engine_t* h, int capacity);
int ipc_vertex_count(ipc_engine_t* h, int* n_vertices);

/* cmpTime processing order (host copy, N ints). */
int ipc_candidate_order(ipc_engine_t* h, int* order_out);

/* Open-loop poses after propagateGuess: SE2 [V][3] (x y theta), SE3 [V][12] (R row-major, t). */
int ipc_initial_poses(ipc_engine_t* h, double* poses_out);

/* ---- consistency matrix (the batched form of
 *      isAgreeingWithCurrentState, reference src/consensus_utils.cpp:7-22) ------------------ */

/* rows per rank of a shard: ceil(N / world). */
int ipc_rows_per_rank(int n, int world);

/* Which rank solves which row of the matrix and where the row sits in that rank's shard: slot_out[i] = owner * rpr +
 * index, rpr = ipc_rows_per_rank(n, world).  ids [n][2] as in ipc_set_candidates.  policy 0: row-cyclic (i % world);
 * policy 1 (the engine's default, IPC_ROW_BALANCE=cost): balanced by cost -- a row's cost is the number of poses its
 * cells sweep (sum over the overlapping pairs (i, j > i) of the union chain length + its own chain), rows go,
 * costliest first, to the least loaded rank with a free slot.  Pure host code (no GPU): every rank of a distributed
 * run computes the same map. */
int ipc_row_assignment(int n, const int* ids, int world, int policy, int* slot_out);

/* Solve every cell (i, j >= i) of the rows this rank owns (ipc_row_assignment with the engine's policy).  d_upper is a
 * device buffer of ipc_rows_per_rank(N, world) * ceil(N/64) uint64 words; the row of candidate i sits at index
 * slot[i] % rpr: bit j (j > i) = pair cell solved and consistent, bit i = diagonal cell consistent.  Non-overlapping
 * pairs are not solved (their bit stays 0; see ipc_assemble_matrix). */
int ipc_solve_rows(ipc_engine_t* h, int rank, int world, uint64_t* d_upper, void* stream);
/* Stream contract of ipc_solve_rows: the call enqueues on `stream` and on streams of the engine that
 * fork from / join back into it, and it blocks the HOST ONCE: behind the cell kernels, for the counts of the
 * cells to solve again (failed factorisations, IPC_LM_RETRY, and cells within IPC_BORDERLINE_BAND of their
 * threshold; skipped when both are off).  The borderline cells are then solved again on the device by the cell
 * kernels themselves (g2o's literal trial loop, compact per-bin lists built on the device, no copies through the
 * host); only cells whose linear solve failed -- degenerate information matrices -- go one by one through the
 * host-driven Levenberg solver.  The FIRST call after the candidates, the rank or the world changed blocks once
 * more, before the cell kernels: the planning pass's cell counts come back and buffers grow with hipMalloc; the
 * cell lists are then kept (round 5).  Whatever the faithful mode has in flight is given up first (it restarts with
 * the next ipc_agreement_check).  Cells whose chain
 * is longer than the largest cell kernel (SE3: 4096 poses, SE2: 16384 with the default policies) are
 * solved one at a time by the cluster solver of ipc_agreement_check -- correct for any length, host
 * driven and slow (reference cfg/3D/GRID_params.yaml: 8000 poses); ipc_solve_report() counts them. */

/* Counts over the cells of the last ipc_solve_rows() (blocks until the device is idle). */
typedef struct {
    int cells;               /* solved cells                                                   */
    int long_cells;          /* of those, solved by the cluster-solver fallback                */
    int failed_cells;        /* the optimisation ended in g2o's Fail state (flags & 2): the linear solve kept meeting
                                non-positive pivots up to the largest Levenberg damping (or the sub-problem has more than
                                24 000 unknowns AND no band structure, ipc_incremental_counters); the cell's chi2 is that
                                of the last good state                                                              */
    int capped_cells;        /* ran to the iteration cap without the dog-leg terminating       */
    int nan_cells;           /* max chi2 is NaN (counts as "agrees", like chi2 > th does in
                                the reference, src/consensus_utils.cpp:18)                     */
    int damped_cells;        /* cells whose linear solve met a non-positive pivot and were solved again with g2o's
                                Levenberg retry (lambda 1e-7 x 10 per failure up to 1e3, sticky for the rest of the
                                optimisation) on the literal normal equations                                      */
    int literal_cells;       /* cells whose max chi2 ended within IPC_BORDERLINE_BAND (default 4 sqrt(IPC_TERMINATE_EPS),
                                relative) of their threshold and were solved again by g2o's literal trial loop, so the
                                convergence test cannot have changed their decision                                 */
} ipc_solve_report_t;
int ipc_solve_report(ipc_engine_t* h, ipc_solve_report_t* out);

/* Build the full symmetric N x N bit matrix (row-major, ceil(N/64) words per row) from the
 * all-gathered shards d_gathered[world][rows_per_rank][words] (row i at gathered row slot[i]):  C[i][j] = solved bit when the
 * id intervals overlap with positive length (reference src/consensus.cpp:157-159), else
 * C[i][i] & C[j][j]. */
int ipc_assemble_matrix(ipc_engine_t* h, const uint64_t* d_gathered, int world,
                        uint64_t* d_bits, void* stream);

/* Greedy consistent-set maximisation over the matrix in cmpTime order (SURVEY.md 8a row P2;
 * plays the role of computeIndependentSubgraph + accept/reject, reference
 * src/consensus.cpp:43-75,124-171).  d_accepted: N bytes (1 = in the consensus set). */
int ipc_set_max(ipc_engine_t* h, const uint64_t* d_bits, uint8_t* d_accepted, void* stream);

/* Single-GPU convenience: solve + assemble + set-max, host outputs (any may be NULL):
 * bits_out [N][ceil(N/64)], accepted_out [N]. */
int ipc_run(ipc_engine_t* h, uint64_t* bits_out, uint8_t* accepted_out);

/* Set-only mode (one GPU): the accepted set of ipc_run without the cells the set-max never reads -- the diagonal cells
 * first, then the pair cells among the candidates whose own cell passed (SURVEY.md 8a row P2 only ever tests those).
 * Same accepted set as ipc_run by construction; no consistency matrix comes out of it (reported separately from the
 * candidate-pairs/s metric, which is defined over the full matrix).  *solved_cells_out: cells actually solved. */
int ipc_run_set_only(ipc_engine_t* h, uint8_t* accepted_out, int* solved_cells_out);

/* Matrix mode over several GPUs of one node from ONE process (what the reference's single-process testers need to use
 * more than one GPU; a multi-process run gathers with RCCL instead, ipc_amd/dist.py).  engines[r], r < n_engines, were
 * created on different devices with the same chain and given the same candidate list; engines[r] acts as rank r of
 * world n_engines: all solve their rows concurrently, the shards are gathered onto engines[0]'s device by peer copies
 * over xGMI, which assembles the matrix and runs the set-max.  Outputs as ipc_run.
 * Peer access: the shards move with hipMemcpyPeerAsync, which works whether or not the devices have peer access to each
 * other -- with access (hipDeviceEnablePeerAccess, the CALLER's decision: it is a process-wide setting the library does not
 * touch) the copy goes GPU to GPU over xGMI; without it, or where the platform denies it (IOMMU / container restrictions:
 * hipDeviceCanAccessPeer = 0), the runtime stages the copy through host memory: the same bytes arrive, at PCIe speed
 * (78 MB for C5: ~5 ms instead of < 1 ms).  Engines that share a device (tests) copy device to device. */
int ipc_run_sharded(ipc_engine_t** engines, int n_engines, uint64_t* bits_out, uint8_t* accepted_out);

/* ---- online matrix mode: the matrix stays on the device, an update solves only the cells of new candidates -----------------
 * The matrix form is this project's re-formulation of src/consensus.cpp:43-75,124-171 (agreementCheck +
 * computeIndependentSubgraph).  A cell (i, j) reads the chain records and open-loop poses of [min lo, max hi], the two candidate
 * records and the parameters -- no other candidate, not N, no vertex appended later (ipc_append_odometry never rewrites an
 * existing pose).  So the matrix over candidates 0..N-1 is the matrix over 0..M-1 plus the cells of the columns M..N-1, and the
 * greedy set (processing order (max id, index)) of a prefix of the order is the whole run's set restricted to it.
 *
 * ipc_run_online: with M = the number of candidates the engine's online matrix covers (ipc_online_covered), solves every cell
 * (i, j >= i) with j >= M and no other, extends the stored symmetric matrix by the new rows and columns, updates the accepted
 * set and sets M = N.  M = 0: a whole solve.  M = N: nothing is solved, the stored result is returned.  Outputs as ipc_run,
 * sized by the N of the moment, any may be NULL: bits_out [N][ceil(N/64)] (78 MB at N = 25 000: an online caller passes NULL and
 * reads accepted_out [N]).  Bit for bit the outputs of ipc_run on the same list.  The greedy continues from the stored accepted
 * mask when every new candidate sits behind every covered one in the processing order (a candidate that arrives with the newest
 * vertex does), otherwise it is rerun from the start over the stored matrix; report->set_max_resumed says which.  The N limit
 * of ipc_set_max applies (IPC_ERR_LIMIT).  One engine, world 1.
 * The call enters matrix mode like every other matrix call (the faithful pipeline's solves in flight are given up) and shares the
 * cell buffers of ipc_solve_rows: afterwards ipc_cell_count, ipc_cell_info and ipc_solve_report describe the cells of THIS call
 * (none after a call with M = N), and the next ipc_solve_rows / ipc_run plans its lists again.  ipc_run, ipc_run_set_only,
 * ipc_solve_rows and ipc_run_sharded neither read nor change the online matrix.
 * Storage: solved upper-triangle bits and the symmetric matrix as [capacity][capacity / 64] words, capacity a multiple of 64 that
 * doubles (the old arrays are retired, not freed, as ipc_append_candidate's are); within the capacity an update allocates and
 * frees nothing.  ipc_reserve_candidates gives room for `capacity` candidates up front, in the candidate arrays and in the online
 * matrix (no-op below the current capacity; the counterpart of ipc_reserve_vertices; kept across ipc_set_candidates).  It may be
 * called on a list in use: the records move on the engine's stream and the next matrix call plans its lists again.  The matrix
 * is quadratic in the capacity (2 x capacity^2 / 8 bytes): a capacity the device has no room for is IPC_ERR_LIMIT before anything
 * is allocated (so is the growth inside ipc_run_online), and beyond the N limit above only the candidate arrays are reserved.
 * ipc_online_reset forgets the matrix (M = 0); ipc_set_candidates does so implicitly, as for the incremental state. */
typedef struct {
    int covered_before, covered_after;   /* M before and after the call (after: N)                                   */
    int cells;                           /* cells solved by this call                                                */
    int long_cells, literal_cells, damped_cells;   /* as in ipc_solve_report_t, for this call                        */
    int set_max_resumed;                 /* 1: the greedy continued from the stored mask, 0: rerun from the start (or nothing to do) */
    int grew;                            /* 1: the matrix storage was re-laid out to a larger capacity               */
} ipc_online_report_t;
int ipc_run_online(ipc_engine_t* h, uint64_t* bits_out, uint8_t* accepted_out, ipc_online_report_t* report);
int ipc_online_covered(ipc_engine_t* h, int* m);
int ipc_online_reset(ipc_engine_t* h);
int ipc_reserve_candidates(ipc_engine_t* h, int capacity);

/* ---- threshold sweep --------------------------------------------------------------------------------
 * The reference optimises a cell first and compares afterwards (isAgreeingWithCurrentState, src/consensus_utils.cpp:7-22: the
 * thresholds enter in :17-19 alone), and its harness reports precision / recall per threshold pair (src/simulation.cpp:70-105):
 * every new (fast_reject_th, slow_reject_th) costs it a whole run.  ipc_run_sweep stands in for n_th such runs: every cell is
 * solved ONCE, then the matrix and the consistent set are produced for each pair -- device resident, in chunks of as many
 * pairs as fit a quarter of the free device memory (IPC_SWEEP_CHUNK=<n>, read at ipc_create, caps the chunk).
 *
 * Contract: entry t of bits_out ([n_th][N][ceil(N/64)]) / accepted_out ([n_th][N]) equals, bit for bit, the output of ipc_run
 * on an engine of the same graph and candidate list whose ipc_params_t differs from this engine's only in fast_reject_th =
 * fast_th[t] and slow_reject_th = slow_th[t], under the same environment (IPC_TERMINATE_EPS, IPC_BORDERLINE_BAND,
 * IPC_LM_RETRY, the default kernel policies).  The iteration bases and s_factor are the engine's own (they change the solve:
 * not sweepable); the engine's own thresholds are not consulted.  Pairs may be unsorted, may repeat, fast > slow is allowed;
 * any non-NaN double is taken as ipc_create takes it.  One engine, world 1; the N limit of ipc_set_max applies
 * (IPC_ERR_LIMIT).  The bit-for-bit claim rests on one fact: with the default policies a cell's kernel variant depends on its
 * bin alone, so a cell's record does not depend on which call solved it.
 *
 * The rule per cell (i, j) and pair t, th = (i == j) ? fast_th[t] : slow_th[t], exactly a fresh engine's: a cell whose first
 * pass ended with flags & 2 takes the Levenberg retry's chi2 (IPC_LM_RETRY on; no band test); else a cell within the
 * borderline band of th (fabs(chi2 - th) <= band * th, band = 0 with IPC_TERMINATE_EPS=0) takes the chi2 of g2o's literal
 * loop; else the first pass's chi2; the bit is !(chi2 > th).  The engine keeps the first pass AND the literal records (a cell
 * can be borderline at one pair and not at another), apart from the arrays ipc_run / ipc_solve_rows / ipc_run_online share:
 * those calls and the sweep do not disturb each other.  The literal loop runs once more only for the cells that some pair of
 * the call makes borderline and whose record is not held yet.
 *
 * The first pass is held: another ipc_run_sweep on the same candidate list skips it (reused_solve).  ipc_set_candidates,
 * ipc_append_candidate and ipc_sweep_reset drop it; ipc_append_odometry does not (no existing cell reads a later vertex).
 * After a sweep ipc_cell_count / ipc_cell_info / ipc_solve_report describe the FIRST-PASS records; literal re-solves appear
 * only as counts in the report.  The online matrix is neither read nor changed.  bits_out, accepted_out, report may be NULL.
 * Errors: n_th < 1, fast_th or slow_th NULL, a NaN threshold: IPC_ERR_ARG; no candidates set: IPC_ERR_STATE. */
typedef struct {
    int thresholds;        /* T of this call                                                                             */
    int cells;             /* cells of the first pass (0 when reused_solve)                                              */
    int long_cells, damped_cells;   /* as in ipc_solve_report_t, of the held first pass                                  */
    int literal_cells;     /* cells solved again by the literal loop in THIS call (the union over the T pairs, minus those an earlier sweep already holds) */
    int literal_held;      /* cells whose literal record the engine holds after the call                                 */
    int reused_solve;      /* 1: the first pass of an earlier ipc_run_sweep on the same candidate list was used          */
    int chunks;            /* groups of thresholds that went through assemble / set-max together                         */
} ipc_sweep_report_t;
int ipc_run_sweep(ipc_engine_t* h, int n_th, const double* fast_th, const double* slow_th, uint64_t* bits_out,
                  uint8_t* accepted_out, ipc_sweep_report_t* report);
int ipc_sweep_reset(ipc_engine_t* h);      /* forget the held first pass */

/* ---- Monte-Carlo batch ------------------------------------------------------------------------------
 * The reference is run as Monte-Carlo experiments (bash/ipc_experiments_2D.sh: one dataset, ten outlier levels, ten draws each,
 * ten ipc_tester_2D processes side by side): every draw shares the odometry chain and the first canonic_inliers loop closures,
 * only the injected outliers differ (src/simulation.cpp:24-25, scripts/generateDataset.py).  ipc_run_batch stands in for n_runs
 * such runs on one chain: the engine's candidate list (ipc_set_candidates / ipc_append_candidate) is the UNION U of all draws,
 * N_u entries; run r is members[run_offsets[r] .. run_offsets[r+1]), indices into U, STRICTLY INCREASING, N_r >= 1 of them
 * (run_offsets[0] = 0), and a candidate's local index in run r is its position in that list.  Every cell that some run needs --
 * the diagonal cells of the members and the overlapping pairs that occur together in some run, no others -- is solved ONCE;
 * each run then gets its own matrix and its own greedy set (the set of a sub-list is NOT the union's set restricted to it).
 *
 * Contract: run r's outputs equal, bit for bit, what ipc_run returns on an engine with the same chain, parameters and
 * environment whose ipc_set_candidates was given the records of run r's members in that order.  With increasing members the
 * processing order of the run's own list, (max id, local index), is the engine's order (ipc_candidate_order) restricted to the
 * members.  As for ipc_run_sweep the claim rests on one fact: with the default policies a cell's kernel variant depends on its
 * bin alone, so a cell's record does not depend on which list it was solved in.
 * bits_out holds the runs back to back: run r is [N_r][ceil(N_r/64)] words in local indices, at word offset
 * sum over q < r of N_q * ceil(N_q/64); accepted_out holds run r's N_r bytes at byte offset run_offsets[r].  bits_out,
 * accepted_out and report may be NULL.
 * The runs go through scatter / assemble / set-max device resident, in chunks of as many consecutive runs as fit a quarter of
 * the free device memory (IPC_BATCH_CHUNK=<runs> and IPC_BATCH_BUDGET=<bytes>, read at ipc_create, cap a chunk).
 * Errors: n_runs < 1, run_offsets or members NULL, an empty run, an index outside [0, N_u), members not strictly increasing:
 * IPC_ERR_ARG; no candidates set: IPC_ERR_STATE; a run beyond the N limit of ipc_set_max, or a run that fits no chunk:
 * IPC_ERR_LIMIT, before anything is allocated.  N_u itself is not bound by that limit: nothing runs a set-max over the union.
 * The call enters matrix mode like every other matrix call and shares the cell buffers of ipc_solve_rows: afterwards
 * ipc_cell_count, ipc_cell_info and ipc_solve_report describe the cells of THIS call, in union indices, and the next
 * ipc_solve_rows / ipc_run plans its lists again.  The online matrix, the sweep's held first pass, the faithful state and the
 * consensus set are neither read nor changed. */
typedef struct {
    int runs;                 /* R of this call                                                            */
    int union_candidates;     /* N of the engine's list                                                    */
    int cells;                /* cells solved: the distinct cells that some run needs                      */
    long long cells_separate; /* sum over the runs of the cells a separate ipc_run on that list would solve */
    int long_cells, damped_cells, literal_cells;   /* as in ipc_solve_report_t, over the solved cells       */
    int chunks;               /* groups of runs that went through scatter / assemble / set-max together    */
} ipc_batch_report_t;
int ipc_run_batch(ipc_engine_t* h, int n_runs, const int* run_offsets, const int* members, uint64_t* bits_out,
                  uint8_t* accepted_out, ipc_batch_report_t* report);

/* ---- multi-start set maximisation -------------------------------------------------------------------
 * ipc_set_max makes ONE greedy pass: the first live candidate of the processing order always joins, and an outlier whose own
 * cell happens to pass vetoes every inlier it disagrees with.  ipc_set_max_multistart makes that pass from every live candidate
 * and keeps the largest set.  Definition, over a matrix laid out as ipc_assemble_matrix writes it:
 *   L = (l_0 .. l_{n-1}): the processing order (ipc_candidate_order) restricted to the live candidates, C[k][k] = 1.
 *   S_q, for a seed position q: the greedy set over the sequence l_q, l_0, l_1, .., l_{q-1}, l_{q+1}, ..  -- a candidate joins
 *     if it agrees with every member so far.  S_0 is exactly the set of ipc_set_max.
 *   The result is the S_q of greatest cardinality, ties to the smallest q: never smaller than ipc_set_max's, pairwise
 *     consistent, maximal (nobody outside agrees with every member), deterministic.  n = 0: the empty set.
 *   sizes[k] = |S_q| for k = l_q, 0 for a candidate that is not live.
 * Every live candidate is a seed (no pruning); this is not an exact maximum clique.
 *
 * ipc_set_max_multistart: device in, device out, enqueued on `stream`, no host synchronisation (as ipc_set_max).  Writes exactly
 * d_accepted[0 .. N) (1 = in the set) and, unless NULL, d_sizes[0 .. N); reads d_bits only.  Errors as ipc_set_max: NULL h, d_bits
 * or d_accepted: IPC_ERR_ARG; no candidates set: IPC_ERR_STATE; N beyond the LDS-resident mask: IPC_ERR_LIMIT -- the same N.
 * The running intersection of a seed lives in registers while ceil(N/64) words are at most 64 x IPC_MULTISTART_REG_WORDS
 * (<k> = 0, 1 or 2, default 2, read at ipc_create; 0 sends every N to the LDS kernel), in shared memory beyond; the outputs do
 * not depend on the kernel.  The workspace (a compact copy of the matrix and four int vectors) belongs to the engine: a second
 * call at the same N allocates nothing.
 *
 * ipc_run_multistart (one GPU): solve + assemble as ipc_run, then BOTH sets from the one matrix.  Host outputs, any may be NULL:
 * bits_out [N][ceil(N/64)] and greedy_out [N] are bit for bit those of ipc_run on the same engine, accepted_out [N] and
 * sizes_out [N] those of ipc_set_max_multistart.  The call enters matrix mode like every other matrix call and shares the cell
 * buffers of ipc_solve_rows (ipc_cell_info describes its cells); the online matrix, the sweep's held first pass, the faithful
 * state and the consensus set are neither read nor changed. */
typedef struct {
    int live;                 /* n: candidates whose own cell passed                                        */
    int greedy_size;          /* |S_0|, the set of ipc_set_max                                              */
    int best_size;            /* the multi-start set                                                        */
    int best_seed;            /* its seed as a FILE index (-1: no live candidate)                           */
    int best_seed_position;   /* ... and as a position q in L (-1: none)                                    */
} ipc_multistart_report_t;
int ipc_set_max_multistart(ipc_engine_t* h, const uint64_t* d_bits, uint8_t* d_accepted, int32_t* d_sizes, void* stream);
int ipc_run_multistart(ipc_engine_t* h, uint64_t* bits_out, uint8_t* accepted_out, uint8_t* greedy_out, int32_t* sizes_out,
                       ipc_multistart_report_t* report);

/* ---- exact maximum consistent set ---------------------------------------------------------------------
 * ipc_set_max and ipc_set_max_multistart return consistent sets without saying how far they are from the largest one.
 * ipc_set_max_exact searches for it, within a budget, and says what it proved.  Definition, over a matrix laid out as
 * ipc_assemble_matrix writes it:
 *   L = (l_0 .. l_{n-1}): the processing order (ipc_candidate_order) restricted to the live candidates, C[k][k] = 1.
 *   G: the graph on L whose edges are the set off-diagonal bits.  omega: its clique number.
 *   LB: the size of the set of ipc_set_max_multistart on the same matrix.
 *   UB0: the number of colours of the sequential greedy colouring of L in position order -- repeat: open a colour class, sweep
 *     the uncoloured positions in ascending order, take a position if it is adjacent to no member of the class.
 *   The work is split into independent subproblems, one per position q: the cliques whose smallest position is q, with the
 *     candidate set N(l_q) restricted to the positions > q.  A subproblem whose 1 + |candidate set| <= LB is pruned at once;
 *     every other one is a depth-first branch-and-bound with a greedy colouring bound at every node, pruned against LB and
 *     against its OWN finds only (size + colour <= best).  A step is one row of the compact matrix fetched and combined; a
 *     subproblem gives up after IPC_EXACT_STEP_CAP steps (read at ipc_create, default 2^20, clamped to [1, 2^30]).
 *   Every subproblem finishes (or LB = UB0 and none is needed): proven = 1, size = upper_bound = omega and the set is a maximum
 *     clique -- the multi-start set, byte for byte, if omega = LB, else the clique of the smallest q that attains omega, and
 *     within that subproblem the first clique of that size in the search's own fixed order (NOT the lexicographically first
 *     maximum clique).  Some subproblem hits the cap: proven = 0, the set is the multi-start set, size = LB, upper_bound = UB0.
 *     n = 0: the empty set, proven = 1, size = upper_bound = 0.
 *   No subproblem reads another one's progress, so which subproblems are capped, steps, size, proven and the set are pure
 *     functions of the matrix, the order and the cap: identical from run to run, whatever wave runs what.
 *
 * ipc_set_max_exact: device in, device out, on `stream` -- but it BLOCKS THE HOST: it reads n, LB and UB0 back to size its
 * workspace, waits for the search and returns with the report filled.  Writes exactly d_accepted[0 .. N) (1 = in the set), reads
 * d_bits only; `report` may be NULL.  Errors as ipc_set_max_multistart: NULL h, d_bits or d_accepted: IPC_ERR_ARG; no candidates
 * set: IPC_ERR_STATE; N > 8192 (a row of the compact matrix is at most two words per lane): IPC_ERR_LIMIT, before anything is
 * allocated.  The depth-first stacks (min(UB0, n) levels for each wave of a pool) belong to the engine and are reused at the
 * same size; a call whose stacks would exceed a quarter of the free device memory returns IPC_ERR_LIMIT before allocating them.
 *
 * ipc_run_exact (one GPU): solve + assemble as ipc_run, then the multi-start and the exact set from the one matrix.  Host
 * outputs, any may be NULL: bits_out [N][ceil(N/64)] is bit for bit that of ipc_run, multistart_out [N] the accepted_out of
 * ipc_run_multistart, accepted_out [N] the set of ipc_set_max_exact.  The call enters matrix mode like every other matrix call
 * and shares the cell buffers of ipc_solve_rows; the online matrix, the sweep's held first pass, the faithful state and the
 * consensus set are neither read nor changed. */
typedef struct {
    int live, multistart_size, size, upper_bound, proven;
    int subproblems;          /* subproblems whose root was not pruned at once */
    int capped;               /* subproblems that hit the step cap */
    long long steps;          /* row loads over all subproblems */
} ipc_exact_report_t;
int ipc_set_max_exact(ipc_engine_t* h, const uint64_t* d_bits, uint8_t* d_accepted, ipc_exact_report_t* report, void* stream);
int ipc_run_exact(ipc_engine_t* h, uint64_t* bits_out, uint8_t* accepted_out, uint8_t* multistart_out, ipc_exact_report_t* report);

/* ---- resumed exact set, and the exact set in online matrix mode ---------------------------------------
 * Three further entry points of the library, declared in a header of their own beside this one, which it needs for the
 * handle and the online report and which includes it here (inside the extern "C" block, where there is one). */
#include "ipc_amd_online_exact.h"
#include "ipc_amd_lazy_sd.h"
/* ... and the sets of every run of a Monte-Carlo batch, likewise. */
#include "ipc_amd_batch_exact.h"
/* ... and the census of the maximum consistent sets -- count, core and support, likewise. */
#include "ipc_amd_census.h"

/* Diagnostics of the last ipc_solve_rows(), ipc_run_online(), ipc_run_sweep() or ipc_run_batch(): number of solved cells, and their records. */
int ipc_cell_count(ipc_engine_t* h, int* n_cells);
int ipc_cell_info(ipc_engine_t* h, ipc_cell_info_t* out, int capacity);

/* HIP-event time (ms) spent in the cell-solver kernels of the last ipc_solve_rows(), the
 * number of solver launches and the pose-iterations... (bench.py roofline).  Blocks until the
 * stream has drained. */
int ipc_solver_time_ms(ipc_engine_t* h, double* ms, int* launches);

int ipc_synchronize(ipc_engine_t* h);

/* ---- faithful incremental mode and final map -------------------
 * The reference's own sequential algorithm on the GPU: state = current pose estimates + the
 * consensus set, one cluster solve per candidate.  Poses are SE2 [V][3] (x y theta) or SE3
 * [V][12] (R row-major, t), as in ipc_initial_poses(). */

/* Outcome of one cluster solve. */
typedef struct {
    int    lo, hi;           /* vertex-id span of the cluster                           */
    int    n_cluster_loops;  /* accepted edges absorbed into the cluster (0: fast path) */
    int    iterations, tries, flags;   /* as in ipc_cell_info_t                         */
    double max_chi2;         /* max edge chi2 after the optimisation                    */
    double chi2_total;       /* sum of chi2 after the optimisation                      */
    double chi2_initial;     /* sum of chi2 before it                                   */
} ipc_check_info_t;

/* Back to the state right after IPC::IPC (src/consensus.cpp:23-27): current poses = open-loop
 * propagation, empty consensus set.  Implicit in ipc_set_candidates(). */
int ipc_incremental_reset(ipc_engine_t* h);

/* Everything the first ipc_agreement_check would otherwise set up inside the caller's timed loop (src/simulation.cpp:36-38
 * times every call): the pose buffers, the streams and workspaces of the solves in flight, the stream-concurrency probe.
 * Belongs to construction (IPC::IPC, src/consensus.cpp:9-33, is not timed by the harness either); optional. */
int ipc_incremental_prepare(ipc_engine_t* h);

/* Replaces IPC<EDGE,VERTEX>::agreementCheck (src/consensus.cpp:43-75) for candidate k (FILE
 * index): computeIndependentSubgraph (:124-171), fast/slow threshold and iteration base
 * (:50-52), isAgreeingWithCurrentState on chain [lo,hi] + cluster loops + candidate from the
 * current poses (consensus_utils.cpp:7-22); on agreement the poses are kept, k joins the
 * consensus set and the tail is re-propagated (propagateCurrentGuess, consensus_utils.cpp:61-71);
 * otherwise the state is untouched.  *agrees = 1 / 0.  info may be NULL.
 * Called in the processing order (ipc_candidate_order) the call finds most results waiting: the library solves ahead of
 * the caller, several candidates at a time (IPC_SPEC_WINDOW, IPC_SPEC_AHEAD), from the current state and from the states
 * finished accepts leave behind, and uses a result only if the state it started from is the committed one when its turn
 * comes -- decisions, iteration counts and chi2 are those of the one-at-a-time loop, bit for bit.  Any other order is
 * served correctly as well: the candidate asked for moves to the head of the engine's prediction and the solves behind
 * it stay valid (they assumed rejects in front of them); an edit of the set throws the work done ahead away. */
int ipc_agreement_check(ipc_engine_t* h, int k, int* agrees, ipc_check_info_t* info);

/* What the faithful mode had to do besides the plain device-resident solve since the engine was created (diagnostics; the
 * decisions are the same either way):
 *   lost_launches          persistent launches whose grid barrier gave up (a workgroup never became resident: foreign work on
 *                          the GPU).  In the look-ahead pipeline the check is redone alone when its turn comes; a check that runs
 *                          alone is launched again, twice (relaunches), before the host-driven kernels take over
 *   host_solver_fallbacks  checks redone by the host-driven solver: lost three times, or the capacitance factorisation met a
 *                          non-positive pivot -- g2o's Levenberg retry (src/utils.cpp:104-105, "dl_var") on the literal normal
 *                          equations follows
 *   literal_band_solves    damped solves that factored the literal normal equations in the banded + bordered layout (round 6:
 *                          any cluster size; dense store below IPC_LITERAL_BAND_MIN_N = 3 072 unknowns or without a band,
 *                          and then only up to 24 000 unknowns -- beyond that the optimisation ends in Fail and the candidate
 *                          is rejected) */
typedef struct {
    long host_solver_fallbacks, lost_launches, relaunches, literal_band_solves;
} ipc_incremental_counters_t;
int ipc_incremental_counters(ipc_engine_t* h, ipc_incremental_counters_t* out);

/* IPC::getMaxConsensusSet (include/ipc/consensus.hpp:16): candidate FILE indices in set order. */
int ipc_consensus_size(ipc_engine_t* h, int* n);
int ipc_consensus_set(ipc_engine_t* h, int* out);

/* IPC::removeEdgeFromCnS (src/consensus.cpp:77-96): drops the first member joining the same
 * vertex pair as candidate k; *removed = 1 if one was found. */
int ipc_remove_from_consensus(ipc_engine_t* h, int k, int* removed);
/* IPC::addEdgeToCnS (src/consensus.cpp:98-119): appends k unless a member joins the same vertex
 * pair, then re-sorts the set by cmpEdgesTime (stable). */
int ipc_add_to_consensus(ipc_engine_t* h, int k);

/* Current pose estimates (the g2o vertex estimates the reference mutates). */
int ipc_current_poses(ipc_engine_t* h, double* poses_out);

/* Resume the loop of src/simulation.cpp:34-47 from a saved state.  Everything IPC::agreementCheck reads and writes is the
 * vertex estimates of the borrowed optimizer and _max_consensus_set (include/ipc/consensus.hpp:23-32), so a pair
 * (ipc_current_poses, ipc_consensus_set) taken at any point of a run, handed back here, continues that run -- on this engine
 * or on another engine of the same graph and candidate list (round 6: how the tests put the engine into late states of
 * BASELINE configs[3] / [4] whose checks the CPU oracle was given hours for).  poses as ipc_current_poses() returns them
 * (SE3: bit for bit the state; SE2: cos / sin of theta are recomputed, a rounding-level difference); cns = candidate FILE
 * indices in set order; resume_position = how many candidates of the processing order (ipc_candidate_order) count as
 * already handed out -- it only tells the look-ahead pipeline where the caller will continue, any value 0..N is correct. */
int ipc_incremental_set_state(ipc_engine_t* h, const double* poses, const int* cns, int n_cns, int resume_position);

/* Final map (src/simulation.cpp:50-65): open-loop guess, odometry information back to
 * (info * s) / s, every candidate with accepted[k] != 0, optimize(iterations) with vertex 0
 * fixed (the harness uses 1000).  poses_out and info may be NULL. */
int ipc_final_optimize(ipc_engine_t* h, const uint8_t* accepted, int iterations, double* poses_out,
                       ipc_check_info_t* info);

/* ---- diagnostics of the incremental mode's dense solver (tests only) ---------------------------------
 * Solves the SPD system the cluster solve factors per dog-leg iteration (the capacitance matrix of the accepted
 * loops).  system: (n+1) x n column major, lower triangle of S in rows 0..n-1, right-hand side in row n.
 * mode 0: one launch per block column (host-driven solver); mode 1: the orchestration inside the persistent
 * cluster kernel, on `workgroups` workgroups.  Both must return the same bits.  info: 0, or 1 + the first block
 * column with a non-positive pivot. */
int ipc_debug_dense_solve(int n, const double* system, int mode, int workgroups, double* x_out, int* info_out);

/* The same for the BANDED capacitance system of large clusters (round 5: the faithful mode on BASELINE configs[3] / [4];
 * the reference factors whatever computeIndependentSubgraph, src/consensus.cpp:124-171, grows the cluster to with g2o's
 * sparse solver, src/utils.cpp:104-105).  system: nb + m - 1 columns of W + m doubles -- column j holds rows j .. j+W-1
 * (band; W >= 64) and then the m dense rows (the wide loops' unknowns, right-hand side last); nb band columns. */
int ipc_debug_band_solve(int nb, int m, int W, const double* system, int workgroups, double* x_out, int* info_out);
/* computeIndependentSubgraph (src/consensus.cpp:124-171) on bare intervals (host code, no GPU): the accepted edges -- positions
 * into lo / hi -- a candidate [klo, khi] absorbs, and the hull.  sweep 0: the reference's fixed-point re-scan; sweep 1: one pass
 * over the intervals sorted by first vertex (what the engine uses for sets of 512 and more).  Same set, same hull. */
int ipc_debug_absorbed_edges(int klo, int khi, int n, const int* lo, const int* hi, int sweep, int* members_out, int* n_members_out,
                             int* lo_out, int* hi_out);
/* The band structure found for a set of loops (host code, no GPU): a / b = first / last vertex per loop, d = 3 (SE2) or
 * 6 (SE3) unknowns per loop, min_n = smallest system that is banded at all (0: always).  *use_out = 0: the dense solver
 * takes the cluster and nlb_out / bwb_out / order_out are NOT written; *use_out = 1: nlb_out = loops in the band,
 * bwb_out = half-bandwidth in blocks, order_out[nl] = the loops in band order, the border's wide loops last. */
int ipc_debug_band_plan(int d, int nl, const int* a, const int* b, int min_n, int* use_out, int* nlb_out, int* bwb_out,
                        int* order_out);
/* Device buffers, pinned host buffers and events the library's owning handles hold at this moment, in the whole process
 * (out[0], out[1], out[2]; host code, no GPU): all zero once every engine is destroyed.  The per-device stream pool is not
 * counted -- it lives as long as the process. */
int ipc_debug_live_resources(int out[3]);

#ifdef __cplusplus
}
#endif
#endif /* IPC_AMD_H */
