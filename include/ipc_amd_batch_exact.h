/* Batch sets: the C ABI of libipc_amd.so for the multi-start and the exact maximum consistent set of every run of a
 * Monte-Carlo batch.
 *
 * Not a header to include by itself: include/ipc_amd.h includes it, behind ipc_engine_t, ipc_batch_report_t, ipc_exact_report_t
 * and the definitions of ipc_run_batch, ipc_set_max, ipc_set_max_multistart and ipc_set_max_exact that the text below refers
 * to.  ipc_amd.capi lists these names in SYMBOLS_BATCH_EXACT (tests/test_batch_exact_cpu.py compares that list with this
 * file, as tests/test_capi_symbols.py compares SYMBOLS with ipc_amd.h). */
#ifndef IPC_AMD_BATCH_EXACT_H
#define IPC_AMD_BATCH_EXACT_H
#ifndef IPC_AMD_H
#error "include ipc_amd.h, which includes this header"
#endif

/* ---- the multi-start and the exact set of every run of a batch --------------------------------------------
 * ipc_run_batch gives every run its own matrix and the ONE-PASS greedy set.  These two calls give every run the three sets the
 * library knows -- greedy, multi-start, exact with its proof -- in one launch sequence over all the runs of a chunk and two
 * host waits per chunk, not one sequence per run.
 *
 * ipc_set_max_batch_exact: n_runs matrices in, their sets out.
 *   d_bits (device) holds the matrices back to back in the layout ipc_run_batch documents for bits_out: run r is
 *     [N_r][ceil(N_r/64)] words at word offset sum over q < r of N_q * ceil(N_q/64), each laid out as ipc_assemble_matrix writes
 *     it.  run_n (host) [n_runs] holds the N_r.  order (host) holds the runs' processing orders back to back: run r is a
 *     permutation of 0 .. N_r-1 at offset sum of N_q, q < r.  d_greedy, d_multistart (either may be NULL) and d_accepted are
 *     device buffers of sum N_r bytes with the offsets of `order`.  reports [n_runs] and report may be NULL.
 *   The engine's candidate list and its N are not read: the engine lends its device, the stream given (NULL: its own), its
 *     workspace and the knobs read at ipc_create (IPC_EXACT_STEP_CAP).
 *   Contract: for every run r, d_multistart, d_accepted and reports[r] are, byte for byte and field for field (steps,
 *     subproblems and capped included), what ipc_set_max_exact writes and reports on an engine whose candidate count is N_r and
 *     whose ipc_candidate_order is run r's order, given matrix r, under the same IPC_EXACT_STEP_CAP; d_greedy is ipc_set_max's
 *     set there.  No run reads anything of another run: a run's outputs do not depend on its neighbours or on its offsets.
 *   The call blocks the host (at most twice: once to read every run's n, LB and UB0 and size one workspace for the runs the
 *     bracket leaves open, once for the reports), writes exactly sum N_r bytes per output and reads d_bits only.
 *   Errors: NULL h, run_n, order, d_bits or d_accepted, n_runs < 1, some N_r < 1, an order slice that is not a permutation:
 *     IPC_ERR_ARG; some N_r > 8192 (the limit of ipc_set_max_exact) or more than 65535 runs: IPC_ERR_LIMIT -- all before
 *     anything is allocated or launched.  The search's stacks obey ipc_set_max_exact's pool rule, over the subproblems of all
 *     open runs together, a slice as deep and as wide as the largest open run needs; what they lack beyond a quarter of the free
 *     device memory is IPC_ERR_LIMIT before it is allocated.
 *
 * ipc_run_batch_exact: ipc_run_batch's arguments, validation, errors, plan, solve, scatter and assemble; per chunk the set stage
 *   above then runs on the chunk's device matrices.  Host outputs, any may be NULL: bits_out and greedy_out are bit for bit
 *   ipc_run_batch's bits_out and accepted_out on the same arguments; multistart_out and accepted_out (ipc_run_batch's offsets)
 *   and reports[r] are, for run r, those of ipc_run_exact on a fresh engine with the same chain, parameters and environment
 *   that was given run r's members in that order.  A run of more than 8192 members: IPC_ERR_LIMIT before anything is
 *   allocated (the union is not bound by that).  A chunk also holds the compact matrices, the vectors of the search and room
 *   for its cliques, so the chunk boundaries and batch_report->chunks may differ from ipc_run_batch's; no output depends on
 *   them.  IPC_BATCH_CHUNK and IPC_BATCH_BUDGET cap a chunk as they do there.  ipc_run_batch itself is unchanged.
 *
 * Both calls enter matrix mode like every other matrix call; the online matrix, the sweep's held first pass, the faithful
 * state and the consensus set are neither read nor changed.  The workspace belongs to the engine: a second call at the same
 * shapes allocates nothing. */
typedef struct {
    int runs;              /* runs of this call                                                            */
    int chunks;            /* groups of runs whose set stage ran as one launch sequence                    */
    int searched_runs;     /* runs whose bracket the multi-start and UB0 did not close (LB < UB0)          */
    int proven_runs;       /* runs with proven = 1                                                         */
    int set_launches;      /* kernel launches of the set stage over the call                               */
    int set_host_waits;    /* host synchronisations of the set stage over the call                         */
} ipc_batch_exact_report_t;
int ipc_set_max_batch_exact(ipc_engine_t* h, int n_runs, const int* run_n, const int* order, const uint64_t* d_bits,
                            uint8_t* d_greedy, uint8_t* d_multistart, uint8_t* d_accepted, ipc_exact_report_t* reports,
                            ipc_batch_exact_report_t* report, void* stream);
int ipc_run_batch_exact(ipc_engine_t* h, int n_runs, const int* run_offsets, const int* members, uint64_t* bits_out,
                        uint8_t* greedy_out, uint8_t* multistart_out, uint8_t* accepted_out, ipc_batch_report_t* batch_report,
                        ipc_exact_report_t* reports, ipc_batch_exact_report_t* report);

#endif
