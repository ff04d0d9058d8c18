/* Online exact set: the C ABI of libipc_amd.so for the resumed exact maximum consistent set.
 *
 * Not a header to include by itself: include/ipc_amd.h includes it, behind ipc_engine_t, ipc_online_report_t and the
 * definitions of ipc_set_max_exact that the text below refers to.  ipc_amd.capi lists these names in SYMBOLS_ONLINE_EXACT
 * (tests/test_exact_resume_cpu.py compares that list with this file, as tests/test_capi_symbols.py compares SYMBOLS with
 * ipc_amd.h). */
#ifndef IPC_AMD_ONLINE_EXACT_H
#define IPC_AMD_ONLINE_EXACT_H
#ifndef IPC_AMD_H
#error "include ipc_amd.h, which includes this header"
#endif

/* ---- resumed exact set, and the exact set in online matrix mode ---------------------------------------
 * Old cells never change when candidates are appended, so the graph over the candidates 0 .. first-1 is an induced subgraph of
 * the graph over 0 .. N-1: a clique of the latter contains no newcomer (file index >= first) -- then it is no larger than a
 * maximum clique of the former -- or it contains one.  ipc_set_max_exact_resume searches the second kind only.
 *   On entry d_accepted[0 .. N) holds a set A: the caller's claim is that A is a maximum clique of the graph on the live
 *     candidates < first.  Checked: bytes 0 or 1, every member live, < first, every two members adjacent; a violation is
 *     IPC_ERR_ARG and d_accepted is left untouched.  first = 0 with A empty is allowed (every live candidate is a newcomer).
 *   L, positions, P, LB as for ipc_set_max_exact (LB: the multi-start set of the WHOLE matrix).  NEW = the positions a of L with
 *     l_a >= first, ascending, m of them; w0 = |A|; b0 = max(w0, LB); the incumbent is A if w0 >= LB (a tie keeps A), else the
 *     multi-start set; c = the colours of the sequential greedy colouring of NEW alone, in position order; UB = min(n, w0 + c).
 *   Root r = the r-th position p_r of NEW: the cliques that contain p_r and no newcomer at a smaller position; candidate set
 *     row(p_r) minus { p_s : s < r } -- covered candidates stay in, in front of p_r as well as behind it.  Pruned at once where
 *     1 + |candidate set| <= b0, else the depth-first branch-and-bound of ipc_set_max_exact, pruned against b0 and the root's
 *     own finds only, one step per row of P, IPC_EXACT_STEP_CAP steps at the most.
 *   m = 0 or b0 >= UB: no search, the incumbent, proven = 1, size = upper_bound = b0.  Every root finishes: proven = 1,
 *     size = upper_bound = the best size; the set is the clique of the smallest r that attains it if it exceeds b0, else the
 *     incumbent.  Some root is capped: proven = 0, the incumbent, size = b0, upper_bound = UB.
 *   proven = 1 means "maximum over all N candidates, given the claim".  No root reads another's progress: the set and every
 *     report field are pure functions of (matrix, order, first, A, cap).
 * The call blocks the host like ipc_set_max_exact (one read-back to size the stacks, one for the report), writes exactly
 * d_accepted[0 .. N), reads d_bits only, and shares ipc_set_max_exact's workspace, N limit (IPC_ERR_LIMIT beyond 8192, before
 * anything is allocated) and quarter-of-free-memory refusal.  first outside [0, N]: IPC_ERR_ARG.
 *
 * ipc_run_online_exact: the update of ipc_run_online, made by that very function -- bits_out, greedy_out (its accepted_out) and
 * online_report are bit for bit its outputs -- then the exact set of the stored matrix into accepted_out [N].  The engine holds
 * the set on the device beside the online matrix, with `covered` (the list length it was computed for) and `proven`
 * (ipc_online_exact_state).  A proven set with 0 < covered <= N is resumed from (first = covered); otherwise the call is the
 * whole search of ipc_set_max_exact over the stored matrix (report->first = 0, newcomers = live, size_before = 0, changed =
 * size > 0).  The state becomes (N, proven of this call): after an unproven call the next one searches the whole graph again.
 * ipc_online_reset and ipc_set_candidates drop the state; ipc_run_online in between neither reads nor changes it (the next
 * exact call catches up from its own `covered`); ipc_append_odometry does not touch it.  N > 8192: IPC_ERR_LIMIT before the
 * update is made.  Every output may be NULL.  IPC_ONLINE_EXACT_RESUME=0 (read at ipc_create; for A/B measurements): the held
 * set is never resumed from, every call is the whole search. */
typedef struct {
    int first;             /* candidates with file index >= first were the newcomers of this call */
    int live, newcomers;   /* n, and the live candidates among the newcomers (m) */
    int size_before;       /* w0: members of the set handed in */
    int multistart_size;   /* LB of ipc_set_max_multistart on the whole matrix */
    int size, upper_bound, proven;
    int changed;           /* 1: d_accepted differs from what was handed in */
    int subproblems;       /* newcomer roots not pruned at once */
    int capped;            /* roots that hit IPC_EXACT_STEP_CAP */
    long long steps;
} ipc_exact_resume_report_t;
int ipc_set_max_exact_resume(ipc_engine_t* h, const uint64_t* d_bits, int first, uint8_t* d_accepted,
                             ipc_exact_resume_report_t* report, void* stream);
int ipc_run_online_exact(ipc_engine_t* h, uint64_t* bits_out, uint8_t* accepted_out, uint8_t* greedy_out,
                         ipc_online_report_t* online_report, ipc_exact_resume_report_t* report);
int ipc_online_exact_state(ipc_engine_t* h, int* covered, int* proven);

#endif
