// Census of the maximum consistent sets (ipc_set_max_census): how many maximum cliques the consistency graph
// has, the candidates all of them share (the core) and the candidates any of them holds (the support).  Runs behind the exact
// stage (exact_kernels.hpp), on the same compact matrix P, with omega -- the size that stage proved -- read back by the host.
// Included by engine.hip behind exact_kernels.hpp, whose ex_colour, ex_first, ex_clear and ex_fence it calls as they are; no
// existing kernel is touched.
//
//   k_cs_search<R>   the pool of k_ex_search: four independent waves per workgroup, no barrier, a wave takes the next subproblem
//                    q from a counter until none is left.  Subproblem q = the maximum cliques whose smallest position is q:
//                    candidate set row(q) restricted to the positions > q, pruned at once where 1 + |candidates| < omega; else
//                    the depth-first search of ex_subproblem with the bound FROZEN at omega - 1 -- a clique that ties omega is
//                    what is looked for, so `best` never moves and a leaf of omega members is counted, not kept.  Nothing a
//                    subproblem explores, finds or counts depends on which wave runs it or on any other subproblem.
//   k_cs_pick        one workgroup: the sums over the subproblems in k_ex_pick's fixed order, the capped fallback, the bytes.
// The clique so far (root, path[0 .. d)) is kept as a bit set K in the lane layout of the candidate sets -- a bit goes in where
// the search descends and out where it backs up, so a leaf costs R words per lane, not a walk over the path -- and a leaf of
// omega members ANDs K + v into the wave's `core` registers and ORs it into its `support` registers.  A subproblem that found
// something folds the two into ONE [2][words] accumulator with 64-bit vector atomicAnd / atomicOr (AND and OR do not depend on
// the order; the launch sequence sets the core half to ones and the support half to zero).
// Steps, the cap and the stack slice are those of ex_subproblem; a subproblem that has made `cap` steps records "capped" and
// leaves.
#pragma once

constexpr int kCsInfo = 9;                              // info words: subproblem counter, subproblems, capped, steps (two words), count
                                                        // (two words), core size, support size

template <int R>
__device__ __forceinline__ void cs_set(unsigned long long (&w)[R], int lane, int v)
{
#pragma unroll
    for (int r = 0; r < R; ++r) { if (lane + 64 * r == (v >> 6)) w[r] |= 1ull << (v & 63); }
}

// ex_subproblem's loop with the bound frozen at omega - 1: the cliques of exactly omega members that contain `root` and members
// of S.  Returns the steps made; `go` false: the cap was hit; `found`: the cliques met (before the cap, if it was hit); their
// AND in `core`, their OR in `support` (all ones / zero where found == 0).  levels = omega; slice, path as in ex_subproblem.
template <int R>
__device__ __forceinline__ unsigned ex_census_subproblem(unsigned long long (&S)[R], int lane, int root, int omega, int nw, int words,
                                                         int levels, int level_words, unsigned cap, const unsigned long long* P,
                                                         unsigned long long* slice, int* path, unsigned long long (&core)[R],
                                                         unsigned long long (&support)[R], unsigned& found, bool& go)
{
    unsigned long long C[R], K[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { K[r] = 0ull; core[r] = ~0ull; support[r] = 0ull; }
    cs_set<R>(K, lane, root);
    const int bound = omega - 1;
    // level d: the clique so far is root, path[0 .. d) -- K; S = its candidates still to branch on or to keep for the children
    int d = 0, cnt = 0, k = 0;
    unsigned steps = 0;
    bool entering = true;
    go = true; found = 0u;
    for (;;) {
        unsigned long long* level = slice + (size_t)d * level_words;
        unsigned short* list = (unsigned short*)(level + 64 * R);
        int* counters = (int*)(level + level_words - 1);
        if (entering) {
            k = ex_colour<R>(S, lane, nw, words, P, bound - (d + 1), list, cnt, steps, cap, go);
            if (!go) break;
            entering = false;
        }
        if (cnt == 0 || d + 1 + k < omega) {                     // nothing left here that could reach omega: back up
            if (d == 0) break;
            --d;
            ex_fence();
            level = slice + (size_t)d * level_words;
            counters = (int*)(level + level_words - 1);
#pragma unroll
            for (int r = 0; r < R; ++r) S[r] = level[lane + 64 * r];
            cnt = counters[0];
            k = counters[1];
            ex_clear<R>(K, lane, path[d]);
            continue;
        }
        ex_fence();
        const unsigned short e = list[cnt - 1];
        const int v = e & 0x7fff;
        --cnt;
        const int k_next = k - (e >> 15);
        if (steps >= cap) { go = false; break; }
        ++steps;
        ex_clear<R>(S, lane, v);
        {
            const unsigned long long* row = P + (size_t)v * words;
#pragma unroll
            for (int r = 0; r < R; ++r) C[r] = lane + 64 * r < nw ? S[r] & row[lane + 64 * r] : 0ull;
        }
        bool empty = true;
#pragma unroll
        for (int r = 0; r < R; ++r) empty = empty && __ballot(C[r] != 0ull) == 0ull;
        if (empty) {                                             // a maximal clique of d + 2: a member of MAX if that is omega
            if (d + 2 == omega) {
                ++found;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const unsigned long long m = K[r] | (lane + 64 * r == (v >> 6) ? 1ull << (v & 63) : 0ull);
                    core[r] &= m;
                    support[r] |= m;
                }
            }
            k = k_next;
            continue;
        }
        if (d + 1 >= levels) { go = false; break; }              // (cannot happen: the child of a clique of omega is empty)
#pragma unroll
        for (int r = 0; r < R; ++r) level[lane + 64 * r] = S[r];
        if (lane == 0) { counters[0] = cnt; counters[1] = k_next; path[d] = v; }
        cs_set<R>(K, lane, v);
        ++d;
#pragma unroll
        for (int r = 0; r < R; ++r) S[r] = C[r];
        entering = true;
    }
    return steps;
}

// slice_words: levels x level_words + the path.  acc: [2][words], core then support; info[0]: the subproblem counter.
template <int R>
__global__ __launch_bounds__(64 * kExWaves) void k_cs_search(int words, int levels, int level_words, size_t slice_words, unsigned cap,
                                                             int omega, const unsigned long long* P, const int* ms_info, int* info,
                                                             unsigned long long* ws, int* sub_flag, int* sub_count, unsigned* sub_steps,
                                                             unsigned long long* acc)
{
    const int lane = threadIdx.x & 63;
    const int n = ms_info[0], nw = (n + 63) >> 6;
    unsigned long long* slice = ws + (size_t)(blockIdx.x * kExWaves + (threadIdx.x >> 6)) * slice_words;
    int* path = (int*)(slice + (size_t)levels * level_words);
    for (;;) {
        int q = 0;
        if (lane == 0) q = atomicAdd(&info[0], 1);
        q = __builtin_amdgcn_readfirstlane(q);
        if (q >= n) return;
        unsigned long long S[R], core[R], support[R];
        int size0 = 0;
        {
            const unsigned long long* row = P + (size_t)q * words;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int w = lane + 64 * r;
                const unsigned long long behind = w > (q >> 6) ? ~0ull : (w == (q >> 6) ? (~0ull << (q & 63)) << 1 : 0ull);
                S[r] = w < nw ? row[w] & behind : 0ull;
                size0 += __popcll(S[r]);
            }
        }
        for (int off = 32; off > 0; off >>= 1) size0 += __shfl_xor(size0, off);
        if (1 + size0 < omega) {
            if (lane == 0) { sub_flag[q] = 0; sub_count[q] = 0; sub_steps[q] = 0u; }
            continue;
        }
        unsigned found = 0u, steps = 0u;
        bool go = true;
        if (size0 == 0) {                                        // omega = 1, no edges: the root is the clique {q}
            found = 1u;
#pragma unroll
            for (int r = 0; r < R; ++r) core[r] = 0ull;
            cs_set<R>(core, lane, q);
#pragma unroll
            for (int r = 0; r < R; ++r) support[r] = core[r];
        } else {
            steps = ex_census_subproblem<R>(S, lane, q, omega, nw, words, levels, level_words, cap, P, slice, path, core, support, found, go);
        }
        if (lane == 0) { sub_flag[q] = go ? 1 : 2; sub_count[q] = (int)found; sub_steps[q] = steps; }
        if (found) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int w = lane + 64 * r;
                if (w < nw) { atomicAnd(&acc[w], core[r]); atomicOr(&acc[words + w], support[r]); }
            }
        }
    }
}

// The results of the subproblems in k_ex_pick's fixed order (integer sums: any order gives the same), then the bytes: core and
// support by candidate for all N, zeroed first.  searched = 0 (the exact stage proved nothing, or n = 0: no search ran) and a
// capped subproblem give the trivial bounds: core empty, support = the live candidates.
__global__ __launch_bounds__(1024) void k_cs_pick(int N, int words, int searched, const int* live, const int* ms_info, const int* sub_flag,
                                                  const int* sub_count, const unsigned* sub_steps, const unsigned long long* acc, int* info,
                                                  unsigned char* core, unsigned char* support)
{
    __shared__ int wave_sub[16], wave_cap[16];
    __shared__ unsigned long long wave_steps[16], wave_count[16];
    __shared__ int exact, core_size, support_size;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = ms_info[0];
    int sub = 0, capped = 0;
    unsigned long long steps = 0ull, count = 0ull;
    if (searched) {
        for (int q = tid; q < n; q += 1024) {
            const int f = sub_flag[q];
            sub += f != 0;
            capped += f == 2;
            steps += sub_steps[q];
            count += (unsigned long long)sub_count[q];
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sub += __shfl_down(sub, off);
        capped += __shfl_down(capped, off);
        steps += __shfl_down(steps, off);
        count += __shfl_down(count, off);
    }
    if (lane == 0) { wave_sub[tid >> 6] = sub; wave_cap[tid >> 6] = capped; wave_steps[tid >> 6] = steps; wave_count[tid >> 6] = count; }
    if (tid == 0) { core_size = 0; support_size = 0; }
    __syncthreads();
    if (tid == 0) {
        sub = 0; capped = 0; steps = 0ull; count = 0ull;
        for (int v = 0; v < 16; ++v) { sub += wave_sub[v]; capped += wave_cap[v]; steps += wave_steps[v]; count += wave_count[v]; }
        exact = searched && capped == 0;
        info[1] = sub; info[2] = capped;
        info[3] = (int)(steps & 0xffffffffull); info[4] = (int)(steps >> 32);
        info[5] = (int)(count & 0xffffffffull); info[6] = (int)(count >> 32);
    }
    for (int c = tid; c < N; c += 1024) { core[c] = 0; support[c] = 0; }
    __syncthreads();
    int in_core = 0, in_support = 0;
    for (int a = tid; a < n; a += 1024) {
        const bool c = exact && ((acc[a >> 6] >> (a & 63)) & 1ull);
        const bool s = !exact || ((acc[words + (a >> 6)] >> (a & 63)) & 1ull);
        if (c) core[live[a]] = 1;
        if (s) support[live[a]] = 1;
        in_core += c; in_support += s;
    }
    for (int off = 32; off > 0; off >>= 1) { in_core += __shfl_down(in_core, off); in_support += __shfl_down(in_support, off); }
    if (lane == 0) { atomicAdd(&core_size, in_core); atomicAdd(&support_size, in_support); }
    __syncthreads();
    if (tid == 0) { info[7] = core_size; info[8] = support_size; }
}
