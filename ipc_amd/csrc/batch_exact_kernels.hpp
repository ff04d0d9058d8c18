// The multi-start and the exact set of every run of a batch (ipc_set_max_batch_exact, ipc_run_batch_exact): the
// stages of multistart_kernels.hpp and exact_kernels.hpp with the run as one more grid dimension, one launch sequence for all
// the runs of a chunk.  Included by engine.hip behind exact_resume_kernels.hpp; ex_subproblem, ex_colour, ex_first, ex_clear,
// ex_fence, ms_first_of, ms_better, ms_chain_lds and set_max_rounds are used as they are, no existing kernel is touched.
//
// A run is described as in batch_kernels.hpp: its matrix [n][words] at mat_off of the chunk's matrices, its compact matrix P at
// p_off of the chunk's compact matrices, its vectors (order, live, pos, sz, flag, size, steps, the byte outputs) at vec_off, its
// info words at info_off.  Every definition -- L, positions, P, S_q, LB, UB0, subproblem q, the pick -- is that of the
// single-matrix kernels, per run; nothing of a run reads anything of another run.
//   k_bx_set_max      one workgroup per run: ipc_set_max's greedy set (set_max_rounds)
//   k_bx_live         one workgroup per run: live list, position map, n                           (k_ms_live)
//   k_bx_compact      one wave per (run, row): P_r                                                (k_ms_compact)
//   k_bx_greedy<R>    one wave per (run, seed), cand in registers: |S_q|                          (k_ms_greedy_reg)
//   k_bx_ms_pick      one workgroup per run: (max size, min q), the multi-start set, LB           (k_ms_pick)
//   k_bx_bound<R>     one wave per run: UB0; presets the exact info words to "the multi-start set stands"  (k_ex_bound)
//   k_bx_search<R>    a pool of waves over the concatenated subproblems (run, q) of the OPEN runs (LB < UB0), run-major with
//                     ascending q, one atomic counter, no barrier                                 (k_ex_search)
//   k_bx_pick         one workgroup per open run                                                  (k_ex_pick)
// The grids of the first six are sized by the chunk's largest run and its number of runs, those of the last two by what the host
// read back (the open runs and their n); surplus waves leave on the device-side n.  R is the chunk's: 1 while every run has at
// most 4096 candidates, else 2 -- a run narrower than R is served by the `lane + 64 r < nw` guards, and no output depends on R.
#pragma once

struct BxRun { int n, words, vec_off, info_off; long long mat_off, p_off; };
// an open run: its descriptor, the number of its first subproblem in the concatenation, the depth of its stacks and cliques
struct BxOpen { int run, first, levels, pad; long long clq_off; };

constexpr int kBxInfo = 12;     // info words per run: n, LB, best position, best candidate, UB0, then kExInfo's [2 .. 8) at [5 .. 11)
constexpr int kBxEx = 3;        // info[kBxEx + j] = the word j of kExInfo, j = 2 .. 7 (size, winner, subproblems, capped, steps lo / hi)

__global__ __launch_bounds__(1024) void k_bx_set_max(const BxRun* runs, const int* order, const unsigned long long* bits,
                                                     unsigned char* accepted, int* live)
{
    const BxRun d = runs[blockIdx.x];
    set_max_rounds(d.n, d.words, d.words, order + d.vec_off, bits + d.mat_off, accepted + d.vec_off, live + d.vec_off, 0, nullptr, nullptr);
}

__global__ __launch_bounds__(1024) void k_bx_live(const BxRun* runs, const int* order_v, const unsigned long long* bits_m, int* live_v,
                                                  int* pos_v, int* info_v)
{
    __shared__ int wcount[16];
    __shared__ int nlive_s;
    const BxRun d = runs[blockIdx.x];
    const int N = d.n, stride = d.words;
    const int* order = order_v + d.vec_off;
    const unsigned long long* bits = bits_m + d.mat_off;
    int* live = live_v + d.vec_off;
    int* pos = pos_v + d.vec_off;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int k = tid; k < N; k += 1024) pos[k] = -1;
    if (tid == 0) nlive_s = 0;
    __syncthreads();
    for (int base = 0; base < N; base += 1024) {
        const int p = base + tid;
        const int k = p < N ? order[p] : -1;
        const bool keep = k >= 0 && ((bits[(size_t)k * stride + (k >> 6)] >> (k & 63)) & 1ull);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcount[wave] = __popcll(m);
        __syncthreads();
        int off = nlive_s;
        for (int v = 0; v < wave; ++v) off += wcount[v];
        if (keep) {
            const int a = off + __popcll(m & ((1ull << lane) - 1ull));
            live[a] = k;
            pos[k] = a;
        }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int v = 0; v < 16; ++v) t += wcount[v]; nlive_s += t; }
        __syncthreads();
    }
    if (tid == 0) info_v[d.info_off] = nlive_s;
}

// run = blockIdx.y, row = the wave's number along x
__global__ __launch_bounds__(64 * kMsWaves) void k_bx_compact(const BxRun* runs, const unsigned long long* bits_m, const int* live_v,
                                                              const int* info_v, unsigned long long* P_m)
{
    const BxRun d = runs[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * kMsWaves + (threadIdx.x >> 6);
    const int n = info_v[d.info_off];
    if (a >= n) return;
    const int nw = (n + 63) >> 6;
    const int* live = live_v + d.vec_off;
    const unsigned long long* row = bits_m + d.mat_off + (size_t)live[a] * d.words;
    unsigned long long* out = P_m + d.p_off + (size_t)a * d.words;
    unsigned long long mine = 0ull;
    for (int wb = 0; wb < nw; ++wb) {
        const int b = wb * 64 + lane;
        const int c = b < n ? live[b] : -1;
        const bool bit = c >= 0 && b != a && ((row[c >> 6] >> (c & 63)) & 1ull);
        const unsigned long long word = __ballot(bit);
        if (lane == (wb & 63)) mine = word;
        if ((wb & 63) == 63 || wb == nw - 1) {
            const int w = (wb & ~63) + lane;
            if (w <= wb) out[w] = mine;
        }
    }
}

// run = blockIdx.y, seed = the wave's number along x
template <int R>
__global__ __launch_bounds__(64 * kMsWaves) void k_bx_greedy(const BxRun* runs, const unsigned long long* P_m, const int* info_v, int* sz_v)
{
    const BxRun d = runs[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * kMsWaves + (threadIdx.x >> 6);
    const int n = info_v[d.info_off];
    if (q >= n) return;
    const int nw = (n + 63) >> 6, words = d.words;
    const unsigned long long* P = P_m + d.p_off;
    unsigned long long cand[R];
    {
        const unsigned long long* row = P + (size_t)q * words;
#pragma unroll
        for (int r = 0; r < R; ++r) cand[r] = lane + 64 * r < nw ? row[lane + 64 * r] : 0ull;
    }
    int size = 1;
    for (;;) {
        const int c = ex_first<R>(cand, lane);
        if (c < 0) break;
        ++size;
        const unsigned long long* row = P + (size_t)c * words;
#pragma unroll
        for (int r = 0; r < R; ++r) { if (lane + 64 * r < nw) cand[r] &= row[lane + 64 * r]; }
    }
    if (lane == 0) sz_v[d.vec_off + q] = size;
}

// dynamic LDS: the words of the chunk's widest run
__global__ __launch_bounds__(1024) void k_bx_ms_pick(const BxRun* runs, const unsigned long long* P_m, const int* live_v, const int* sz_v,
                                                     int* info_v, unsigned char* accepted_v)
{
    extern __shared__ unsigned long long ms_cand[];     // [words]
    __shared__ int wave_s[16], wave_q[16];
    const BxRun d = runs[blockIdx.x];
    const int* live = live_v + d.vec_off;
    const int* sz = sz_v + d.vec_off;
    int* info = info_v + d.info_off;
    unsigned char* accepted = accepted_v + d.vec_off;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = info[0];
    int bs = 0, bq = -1;
    for (int q = tid; q < n; q += 1024) ms_better(bs, bq, sz[q], q);
    for (int off = 32; off > 0; off >>= 1) {
        const int s = __shfl_down(bs, off), q = __shfl_down(bq, off);
        ms_better(bs, bq, s, q);
    }
    if (lane == 0) { wave_s[tid >> 6] = bs; wave_q[tid >> 6] = bq; }
    for (int k = tid; k < d.n; k += 1024) accepted[k] = 0;
    __syncthreads();
    bs = 0; bq = -1;
    for (int v = 0; v < 16; ++v) ms_better(bs, bq, wave_s[v], wave_q[v]);
    if (tid == 0) { info[1] = bs; info[2] = bq; info[3] = bq >= 0 ? live[bq] : -1; }
    if (bq < 0 || tid >= 64) return;
    ms_chain_lds(bq, (n + 63) >> 6, d.words, P_m + d.p_off, ms_cand, live, accepted);
}

template <int R>
__global__ __launch_bounds__(64) void k_bx_bound(const BxRun* runs, const unsigned long long* P_m, int* info_v)
{
    const BxRun d = runs[blockIdx.x];
    int* info = info_v + d.info_off;
    const int lane = threadIdx.x;
    const int n = info[0], nw = (n + 63) >> 6;
    unsigned long long S[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int w = lane + 64 * r;
        S[r] = w < (n >> 6) ? ~0ull : (w == (n >> 6) ? (1ull << (n & 63)) - 1ull : 0ull);
    }
    int count = 0;
    unsigned steps = 0;
    bool go = true;
    const int k = ex_colour<R>(S, lane, nw, d.words, P_m + d.p_off, 0, nullptr, count, steps, 0xffffffffu, go);
    if (lane == 0) {
        info[4] = k;
        info[kBxEx + 2] = info[1]; info[kBxEx + 3] = -1;
        info[kBxEx + 4] = 0; info[kBxEx + 5] = 0; info[kBxEx + 6] = 0; info[kBxEx + 7] = 0;
    }
}

// The open run of item i: the last one whose first subproblem is <= i (an open run has n >= 2 subproblems, so no two share a first).
__device__ __forceinline__ int bx_open_of(const BxOpen* open, int n_open, int item)
{
    int lo = 0, hi = n_open;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (open[mid].first <= item) lo = mid; else hi = mid; }
    return lo;
}

// `total` = the subproblems of all open runs; level_words and slice_words are those of the widest and deepest open run, the
// bounds (`levels`) and the clique stride a run's own.
template <int R>
__global__ __launch_bounds__(64 * kExWaves) void k_bx_search(int n_open, int total, int level_words, size_t slice_words, unsigned cap,
                                                             const BxRun* runs, const BxOpen* open, const unsigned long long* P_m,
                                                             const int* info_v, int* counter, unsigned long long* ws, int* flag_v,
                                                             int* size_v, unsigned* steps_v, unsigned short* cliques)
{
    const int lane = threadIdx.x & 63;
    unsigned long long* slice = ws + (size_t)(blockIdx.x * kExWaves + (threadIdx.x >> 6)) * slice_words;
    for (;;) {
        int item = 0;
        if (lane == 0) item = atomicAdd(counter, 1);
        item = __builtin_amdgcn_readfirstlane(item);
        if (item >= total) return;
        const BxOpen o = open[bx_open_of(open, n_open, item)];
        const BxRun d = runs[o.run];
        const int q = item - o.first;
        const int n = info_v[d.info_off], lb = info_v[d.info_off + 1], nw = (n + 63) >> 6, words = d.words;
        if (q >= n) continue;                                    // (the host counted n subproblems for this run: never taken)
        const unsigned long long* P = P_m + d.p_off;
        int* sub_flag = flag_v + d.vec_off;
        int* sub_size = size_v + d.vec_off;
        unsigned* sub_steps = steps_v + d.vec_off;
        int* path = (int*)(slice + (size_t)o.levels * level_words);
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
        const unsigned steps = ex_subproblem<R>(S, lane, q, lb, nw, words, o.levels, level_words, cap, P, slice, path,
                                                cliques + o.clq_off + (size_t)q * o.levels, best, found, go);
        if (lane == 0) { sub_flag[q] = go ? 1 : 2; sub_size[q] = found ? best : 0; sub_steps[q] = steps; }
    }
}

// k_ex_pick for the open run blockIdx.x
__global__ __launch_bounds__(1024) void k_bx_pick(const BxRun* runs, const BxOpen* open, const int* live_v, const int* flag_v,
                                                  const int* size_v, const unsigned* steps_v, const unsigned short* cliques, int* info_v,
                                                  unsigned char* accepted_v)
{
    __shared__ int wave_s[16], wave_q[16], wave_sub[16], wave_cap[16];
    __shared__ unsigned long long wave_steps[16];
    __shared__ int win_s, win_q;
    const BxOpen o = open[blockIdx.x];
    const BxRun d = runs[o.run];
    const int* live = live_v + d.vec_off;
    const int* sub_flag = flag_v + d.vec_off;
    const int* sub_size = size_v + d.vec_off;
    const unsigned* sub_steps = steps_v + d.vec_off;
    int* info = info_v + d.info_off;
    unsigned char* accepted = accepted_v + d.vec_off;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = info[0], lb = info[1];
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
        info[kBxEx + 2] = win_s; info[kBxEx + 3] = win_q; info[kBxEx + 4] = sub; info[kBxEx + 5] = capped;
        info[kBxEx + 6] = (int)(steps & 0xffffffffull); info[kBxEx + 7] = (int)(steps >> 32);
    }
    __syncthreads();
    if (win_q < 0) return;
    for (int c = tid; c < d.n; c += 1024) accepted[c] = 0;
    __syncthreads();
    const unsigned short* clique = cliques + o.clq_off + (size_t)win_q * o.levels;
    for (int j = tid; j < win_s; j += 1024) accepted[live[clique[j]]] = 1;
}
