// Exact maximum consistent set (ipc_set_max_exact): a budgeted branch-and-bound for the maximum clique of the
// consistency graph, over the compact matrix P of the multi-start (multistart_kernels.hpp), whose set is the lower bound LB.
// Included by engine.hip behind multistart_kernels.hpp; no existing kernel is touched.
//
// Positions are those of L, the live candidates in processing order; row a of P holds the neighbours of l_a, diagonal cleared.
//   k_ex_bound<R>    one wave: UB0, the colours of the sequential greedy colouring of all of L; clears the subproblem counter
//   k_ex_search<R>   a pool of waves, four independent waves per workgroup, no barrier, nobody waits for anybody: a wave
//                    takes the next subproblem q from a counter until none is left.  Subproblem q = the cliques whose smallest
//                    position is q: candidate set row(q) restricted to the positions > q.  It is pruned at once where
//                    1 + |candidates| <= LB; else a depth-first search with a colouring bound at every node, pruned against
//                    LB and the subproblem's OWN finds only -- what a subproblem explores, finds and counts does not depend
//                    on which wave runs it, on the size of the pool or on any other subproblem.
//   k_ex_pick        one workgroup: (max size, min q) over the subproblems in a fixed order, their counts, the outputs
// The search of one subproblem is ex_subproblem<R>, which k_exr_search (exact_resume_kernels.hpp) calls as well.
// A candidate set is a bit set spread over the lanes as in k_ms_greedy_reg: lane l holds the words l, l + 64, .. (R of them).
// A node colours its set (repeat: open a class, take the lowest position left, strike its neighbours from the sweep), lists the
// vertices whose colour could still beat the best clique, in colour order, and branches from the end of that list; a child
// whose size + colour cannot beat the best ends the node.  A step is one row of P fetched and combined: one coloured vertex or
// one child set.  Every loop makes a step per trip or ends, and a subproblem that has made `cap` steps records "capped" and
// leaves.  The depth-first stack is a slice of a global workspace that belongs to the wave: per level the candidate set, the
// list (16 bits per vertex: the position, bit 15 on the first vertex of a colour class) and two counters; then the path.
#pragma once

constexpr int kExWaves = 4;                             // waves per workgroup of k_ex_search
constexpr int kExInfo = 8;                              // info words: UB0, subproblem counter, size, position q of the winner (-1: the
                                                        // multi-start set stands), subproblems, capped, steps (two words)
constexpr unsigned short kExClassStart = 0x8000;

template <int R>
__device__ __forceinline__ int ex_first(const unsigned long long (&w)[R], int lane)
{
    int c = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (c < 0) {
            const unsigned long long m = __ballot(w[r] != 0ull);
            if (m) c = ms_first_of(m, lane + 64 * r, w[r]);
        }
    }
    return c;
}

template <int R>
__device__ __forceinline__ void ex_clear(unsigned long long (&w)[R], int lane, int v)
{
#pragma unroll
    for (int r = 0; r < R; ++r) { if (lane + 64 * r == (v >> 6)) w[r] &= ~(1ull << (v & 63)); }
}

// Stores of one lane that another lane of the same wave reads back (list, counters, path): ordered by a fence of workgroup scope.
__device__ __forceinline__ void ex_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Colours the set S; returns the number of colours.  With `list`, the vertices of colour > min_colour go to list[0 .. count) in
// colour order (64 entries parked one per lane, then one coalesced store).  One step per vertex; false in `go` once the cap is hit.
template <int R>
__device__ __forceinline__ int ex_colour(const unsigned long long (&S)[R], int lane, int nw, int words, const unsigned long long* P,
                                         int min_colour, unsigned short* list, int& count, unsigned& steps, unsigned cap, bool& go)
{
    unsigned long long Q[R], U[R];
#pragma unroll
    for (int r = 0; r < R; ++r) Q[r] = S[r];
    int k = 0, i = 0;
    unsigned short mine = 0;
    for (;;) {
#pragma unroll
        for (int r = 0; r < R; ++r) U[r] = Q[r];
        int v = ex_first<R>(U, lane);
        if (v < 0) break;
        ++k;
        bool first = true;
        do {
            if (steps >= cap) { go = false; count = 0; return k; }
            ++steps;
            const unsigned long long* row = P + (size_t)v * words;
#pragma unroll
            for (int r = 0; r < R; ++r) { if (lane + 64 * r < nw) U[r] &= ~row[lane + 64 * r]; }
            ex_clear<R>(U, lane, v);
            ex_clear<R>(Q, lane, v);
            if (list && k > min_colour) {
                if (lane == (i & 63)) mine = (unsigned short)(v | (first ? kExClassStart : 0));
                if ((i & 63) == 63) list[(i & ~63) + lane] = mine;
                ++i;
            }
            first = false;
            v = ex_first<R>(U, lane);
        } while (v >= 0);
    }
    if (list && lane < (i & 63)) list[(i & ~63) + lane] = mine;
    count = i;
    return k;
}

template <int R>
__global__ __launch_bounds__(64) void k_ex_bound(int words, const unsigned long long* P, const int* ms_info, int* ex_info)
{
    const int lane = threadIdx.x;
    const int n = ms_info[0], nw = (n + 63) >> 6;
    unsigned long long S[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int w = lane + 64 * r;
        S[r] = w < (n >> 6) ? ~0ull : (w == (n >> 6) ? (1ull << (n & 63)) - 1ull : 0ull);
    }
    int count = 0;
    unsigned steps = 0;
    bool go = true;
    const int k = ex_colour<R>(S, lane, nw, words, P, 0, nullptr, count, steps, 0xffffffffu, go);
    if (lane == 0) { ex_info[0] = k; ex_info[1] = 0; }
}

// The depth-first search of one subproblem, shared by k_ex_search and k_exr_search (exact_resume_kernels.hpp): the cliques that
// contain `root` and members of S (the root's candidate set, as the caller restricted it), looking for more than `lb` members.
// Returns the steps made; `go` false: the cap was hit; `found`: a clique of `best` > lb members went to out[0 .. best).
// levels: the depth of a wave's stack; level_words: 64 R + ceil(n / 4) + 1 words of 8 bytes; the path lies behind the levels.
template <int R>
__device__ __forceinline__ unsigned ex_subproblem(unsigned long long (&S)[R], int lane, int root, int lb, int nw, int words, int levels,
                                                  int level_words, unsigned cap, const unsigned long long* P, unsigned long long* slice,
                                                  int* path, unsigned short* out, int& best, bool& found, bool& go)
{
    unsigned long long C[R];
    // level d: the clique so far is root, path[0 .. d); S = its candidates still to branch on or to keep for the children
    int d = 0, cnt = 0, k = 0;
    unsigned steps = 0;
    bool entering = true;
    best = lb; go = true; found = false;
    for (;;) {
        unsigned long long* level = slice + (size_t)d * level_words;
        unsigned short* list = (unsigned short*)(level + 64 * R);
        int* counters = (int*)(level + level_words - 1);
        if (entering) {
            k = ex_colour<R>(S, lane, nw, words, P, best - (d + 1), list, cnt, steps, cap, go);
            if (!go) break;
            entering = false;
        }
        if (cnt == 0 || d + 1 + k <= best) {                     // nothing left here that could beat the best: back up
            if (d == 0) break;
            --d;
            ex_fence();
            level = slice + (size_t)d * level_words;
            counters = (int*)(level + level_words - 1);
#pragma unroll
            for (int r = 0; r < R; ++r) S[r] = level[lane + 64 * r];
            cnt = counters[0];
            k = counters[1];
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
        if (empty) {                                             // a maximal clique of d + 2: the first of its size wins
            if (d + 2 > best && d + 2 <= levels) {
                best = d + 2;
                found = true;
                for (int j = lane; j < d; j += 64) out[1 + j] = (unsigned short)path[j];
                if (lane == 0) { out[0] = (unsigned short)root; out[d + 1] = (unsigned short)v; }
            }
            k = k_next;
            continue;
        }
        if (d + 1 >= levels) { go = false; break; }              // (cannot happen while the bound on the clique number holds)
#pragma unroll
        for (int r = 0; r < R; ++r) level[lane + 64 * r] = S[r];
        if (lane == 0) { counters[0] = cnt; counters[1] = k_next; path[d] = v; }
        ++d;
#pragma unroll
        for (int r = 0; r < R; ++r) S[r] = C[r];
        entering = true;
    }
    return steps;
}

// slice_words: levels x level_words + the path
template <int R>
__global__ __launch_bounds__(64 * kExWaves) void k_ex_search(int words, int levels, int level_words, size_t slice_words, unsigned cap,
                                                             const unsigned long long* P, const int* ms_info, int* ex_info,
                                                             unsigned long long* ws, int* sub_flag, int* sub_size, unsigned* sub_steps,
                                                             unsigned short* cliques)
{
    const int lane = threadIdx.x & 63;
    const int n = ms_info[0], lb = ms_info[1], nw = (n + 63) >> 6;
    unsigned long long* slice = ws + (size_t)(blockIdx.x * kExWaves + (threadIdx.x >> 6)) * slice_words;
    int* path = (int*)(slice + (size_t)levels * level_words);
    for (;;) {
        int q = 0;
        if (lane == 0) q = atomicAdd(&ex_info[1], 1);
        q = __builtin_amdgcn_readfirstlane(q);
        if (q >= n) return;
        unsigned long long S[R];
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
        if (1 + size0 <= lb) {
            if (lane == 0) { sub_flag[q] = 0; sub_size[q] = 0; sub_steps[q] = 0u; }
            continue;
        }
        int best;
        bool go, found;
        const unsigned steps = ex_subproblem<R>(S, lane, q, lb, nw, words, levels, level_words, cap, P, slice, path,
                                                cliques + (size_t)q * levels, best, found, go);
        if (lane == 0) { sub_flag[q] = go ? 1 : 2; sub_size[q] = found ? best : 0; sub_steps[q] = steps; }
    }
}

// The results of the subproblems in a fixed order, as k_ms_pick reduces the seeds: greatest size, at equal size the lower q; the
// counts by sums (integers: any order gives the same).  Where every subproblem finished and one found more than LB, accepted --
// which holds the multi-start set -- is rewritten with that subproblem's clique.
__global__ __launch_bounds__(1024) void k_ex_pick(int N, int levels, const int* live, const int* ms_info, const int* sub_flag,
                                                  const int* sub_size, const unsigned* sub_steps, const unsigned short* cliques,
                                                  int* ex_info, unsigned char* accepted)
{
    __shared__ int wave_s[16], wave_q[16], wave_sub[16], wave_cap[16];
    __shared__ unsigned long long wave_steps[16];
    __shared__ int win_s, win_q;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = ms_info[0], lb = ms_info[1];
    int bs = 0, bq = -1, sub = 0, capped = 0;
    unsigned long long steps = 0ull;
    for (int q = tid; q < n; q += 1024) {
        const int f = sub_flag[q];
        ms_better(bs, bq, sub_size[q], q);
        sub += f != 0;
        capped += f == 2;
        steps += sub_steps[q];
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int s = __shfl_down(bs, off), q = __shfl_down(bq, off);
        ms_better(bs, bq, s, q);
        sub += __shfl_down(sub, off);
        capped += __shfl_down(capped, off);
        steps += __shfl_down(steps, off);
    }
    if (lane == 0) { wave_s[tid >> 6] = bs; wave_q[tid >> 6] = bq; wave_sub[tid >> 6] = sub; wave_cap[tid >> 6] = capped; wave_steps[tid >> 6] = steps; }
    __syncthreads();
    if (tid == 0) {
        bs = 0; bq = -1; sub = 0; capped = 0; steps = 0ull;
        for (int v = 0; v < 16; ++v) {
            ms_better(bs, bq, wave_s[v], wave_q[v]);
            sub += wave_sub[v]; capped += wave_cap[v]; steps += wave_steps[v];
        }
        const bool better = capped == 0 && bs > lb;
        win_s = better ? bs : lb;
        win_q = better ? bq : -1;
        ex_info[2] = win_s; ex_info[3] = win_q; ex_info[4] = sub; ex_info[5] = capped;
        ex_info[6] = (int)(steps & 0xffffffffull); ex_info[7] = (int)(steps >> 32);
    }
    __syncthreads();
    if (win_q < 0) return;
    for (int c = tid; c < N; c += 1024) accepted[c] = 0;
    __syncthreads();
    const unsigned short* clique = cliques + (size_t)win_q * levels;
    for (int j = tid; j < win_s; j += 1024) accepted[live[clique[j]]] = 1;
}
