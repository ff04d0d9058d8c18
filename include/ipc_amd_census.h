/* Census of the maximum consistent sets: the C ABI of libipc_amd.so for the count, the core and the support of the maximum
 * cliques of the consistency graph.
 *
 * Not a header to include by itself: include/ipc_amd.h includes it, behind ipc_engine_t, ipc_exact_report_t and the
 * definitions of ipc_set_max_exact and ipc_run_exact that the text below refers to.  ipc_amd.capi lists these names in
 * SYMBOLS_CENSUS (tests/test_census_cpu.py compares that list with this file, as tests/test_capi_symbols.py compares SYMBOLS
 * with ipc_amd.h). */
#ifndef IPC_AMD_CENSUS_H
#define IPC_AMD_CENSUS_H
#ifndef IPC_AMD_H
#error "include ipc_amd.h, which includes this header"
#endif

/* ---- count, core and support of the maximum consistent sets --------------------------------------------
 * ipc_set_max_exact returns ONE set and, with proven = 1, the knowledge that no larger one exists -- not whether it is the only
 * one of its size.  The census says how many there are and which candidates they agree on.
 *   L, positions, P, G, omega, LB and UB0 as for ipc_set_max_exact.
 *   MAX = the set of cliques of G with exactly omega members.  count = |MAX|.  core = the candidates in every member of MAX;
 *     support = the candidates in some member of MAX.  n = 0 (no live candidate): MAX = { {} }, count = 1, core and support
 *     are empty.  support \ core is the list of the candidates on which the maximum sets disagree.
 *   1. The exact stage: exactly what ipc_set_max_exact does -- d_accepted and *exact_report are byte for byte and field for
 *     field what that call gives, steps included.  Where it ends with proven = 0, omega is unknown and no census is attempted:
 *     exact_proven = 0, proven = 0, count = 0, subproblems = capped = 0, steps = 0, core all zeros, support = the live
 *     candidates -- the trivial sound bounds (the true core contains what is written, the true support is contained in it).
 *   2. One census subproblem per position q: the members of MAX whose smallest position is q.  Candidate set row(q) restricted
 *     to the positions > q; pruned at once where 1 + |candidates| < omega; else the depth-first search of ipc_set_max_exact with
 *     the bound frozen at omega - 1: a node colours its set, lists the vertices of colour > (omega - 1) - (d + 1) and is left
 *     where nothing is listed or d + 1 + colours < omega; the bound never moves.  Every leaf (child set empty) of d + 2 = omega
 *     members is a member of MAX: the subproblem's counter goes up by one, the clique's positions are ANDed into its core and
 *     ORed into its support.  A smaller leaf is not maximum and is ignored.  omega = 1 (no edges): a root with an empty
 *     candidate set is itself the clique {q}.  A step is one row of P fetched and combined; a subproblem gives up after
 *     IPC_EXACT_STEP_CAP steps (the knob of ipc_set_max_exact, clamped as there).
 *   3. Every subproblem finished: proven = 1, count = the sum of the counters, core = the AND over the subproblems that found
 *     something, support = the OR.  Some subproblem capped: proven = 0, count = the members found before giving up -- a lower
 *     bound, and a deterministic one, every subproblem's search order being fixed --, core all zeros, support = the live
 *     candidates.  core_size and support_size are the popcounts of what is written; subproblems = the roots not pruned at
 *     once; capped and steps as in ipc_exact_report_t, for the census search alone.
 *   No subproblem reads another one's progress; AND, OR and integer sums do not depend on the order: every output is a pure
 *     function of (matrix, order, cap), identical from run to run.  count <= steps < 2^30 * 8192 cannot overflow.
 *   With proven = 1: core is a subset of accepted, accepted of support; count == 1 exactly where core == support == accepted;
 *     core_size <= size <= support_size; every member of the support is live.
 *
 * ipc_set_max_census: device in, device out, on `stream` (NULL: the engine's own); BLOCKS THE HOST: the exact stage's one or
 * two waits and one behind the census.  Writes exactly d_accepted[0 .. N), d_core[0 .. N) and d_support[0 .. N) (1 = member),
 * reads d_bits only; either report may be NULL.  Errors as ipc_set_max_exact: NULL h, d_bits, d_accepted, d_core or d_support:
 * IPC_ERR_ARG; no candidates set: IPC_ERR_STATE; N > 8192: IPC_ERR_LIMIT before anything is allocated; stacks (omega levels for
 * each wave of the pool, the pool rule of ipc_set_max_exact) beyond a quarter of the free device memory: IPC_ERR_LIMIT before they
 * are allocated.  The workspace is the exact stage's and belongs to the engine: a second call at the same N allocates nothing.
 *
 * ipc_run_census (one GPU): solve + assemble as ipc_run_exact, then the call above on the one matrix.  Host outputs, any may be
 * NULL: bits_out and accepted_out are bit for bit those of ipc_run_exact; core_out [N], support_out [N].  The call enters matrix
 * mode like every other matrix call; the online matrix, the sweep's held first pass, the faithful state and the consensus set are
 * neither read nor changed. */
typedef struct {
    int live;              /* n                                                             */
    int size;              /* omega when exact_proven, else LB                              */
    int exact_proven;      /* proven of the exact stage; 0: no census was attempted         */
    int proven;            /* 1: count, core and support are exact                          */
    long long count;       /* |MAX| (proven), else the members found before the cap         */
    int core_size, support_size;
    int subproblems, capped;
    long long steps;       /* census search only */
} ipc_census_report_t;     /* 48 bytes */

int ipc_set_max_census(ipc_engine_t* h, const uint64_t* d_bits, uint8_t* d_accepted, uint8_t* d_core, uint8_t* d_support,
                       ipc_exact_report_t* exact_report, ipc_census_report_t* report, void* stream);
int ipc_run_census(ipc_engine_t* h, uint64_t* bits_out, uint8_t* accepted_out, uint8_t* core_out, uint8_t* support_out,
                   ipc_exact_report_t* exact_report, ipc_census_report_t* report);

#endif
