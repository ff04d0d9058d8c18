// Resumed exact maximum consistent set (ipc_set_max_exact_resume): the caller hands in a set A that is a maximum
// clique of the graph on the candidates with file index < first; only the cliques that contain a newcomer (file index >= first)
// are searched, with max(|A|, LB) as the incumbent.  Included by engine.hip behind exact_kernels.hpp, whose ex_first, ex_clear,
// ex_colour, ex_fence and ex_subproblem it uses, over the compact matrix P of the multi-start (positions of L, diagonal cleared).
//   k_exr_prepare<R>  one workgroup: checks A (0/1 bytes, members live, < first, pairwise adjacent), w0 = |A|, the mask NEW of the
//                     newcomers' positions, the root list (NEW in ascending position, ordered compaction as k_ms_live), m, and c,
//                     the colours of the sequential greedy colouring of NEW alone; clears the root counter
//   k_exr_search<R>   the pool of k_ex_search: a wave takes the next root rank r from a counter.  Root r = the r-th position p of
//                     NEW: the cliques that contain p and no newcomer at a smaller position -- candidate set row(p) minus the
//                     newcomers in front of p; covered candidates stay in on BOTH sides of p.  Pruned at once where
//                     1 + |candidates| <= b0 = max(w0, LB); else ex_subproblem, pruned against b0 and the root's own finds only
//   k_exr_pick        one workgroup: (max size, min r) in the fixed order of k_ex_pick, the counts, then the set: the winning
//                     clique, or the multi-start bytes where LB > w0, or accepted left as handed in
#pragma once

constexpr int kExrInfo = 12;                            // info words: valid, w0, m, c, root counter, size, winner (rank r; -1: the set
                                                        // handed in stands; -2: the multi-start set), roots searched, capped, steps
                                                        // (two words), changed

template <int R>
__global__ __launch_bounds__(1024) void k_exr_prepare(int N, int first, int words, const unsigned long long* P, const int* live,
                                                      const int* pos, const int* ms_info, const unsigned char* accepted,
                                                      unsigned long long* new_mask, int* roots, int* info)
{
    __shared__ unsigned long long A_s[64 * R], new_s[64 * R];
    __shared__ int wcount[16];
    __shared__ int bad_s, w0_s, m_s;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = ms_info[0], nw = (n + 63) >> 6;
    if (tid == 0) { bad_s = 0; w0_s = 0; m_s = 0; }
    for (int w = tid; w < 64 * R; w += 1024) { A_s[w] = 0ull; new_s[w] = 0ull; }
    __syncthreads();
    // the bytes: 0 or 1, a member is live and in front of `first`
    {
        int mine = 0;
        bool bad = false;
        for (int k = tid; k < N; k += 1024) {
            const unsigned char b = accepted[k];
            if (b > 1) bad = true;
            else if (b) { ++mine; bad = bad || pos[k] < 0 || k >= first; }
        }
        if (mine) atomicAdd(&w0_s, mine);
        if (bad) atomicOr(&bad_s, 1);
    }
    // A and NEW over the positions (a wave's ballot is one word), the roots by ordered compaction
    for (int base = 0; base < n; base += 1024) {
        const int a = base + tid;
        const int k = a < n ? live[a] : -1;
        const bool in_a = k >= 0 && accepted[k] == 1, is_new = k >= first && k >= 0;
        const unsigned long long ma = __ballot(in_a), mn = __ballot(is_new);
        const int wi = (base >> 6) + wave;
        if (lane == 0) {
            wcount[wave] = __popcll(mn);
            if (wi < 64 * R) { A_s[wi] = ma; new_s[wi] = mn; }
        }
        __syncthreads();
        int off = m_s;
        for (int v = 0; v < wave; ++v) off += wcount[v];
        if (is_new) roots[off + __popcll(mn & ((1ull << lane) - 1ull))] = a;
        __syncthreads();
        if (tid == 0) { int t = 0; for (int v = 0; v < 16; ++v) t += wcount[v]; m_s += t; }
        __syncthreads();
    }
    __syncthreads();
    // pairwise adjacent, one member per wave trip: the member's row of P must contain A minus the member itself
    if (!bad_s) {
        bool bad = false;
        for (int wi = wave; wi < nw; wi += 16) {
            unsigned long long word = A_s[wi];
            while (word) {
                const int a = wi * 64 + __builtin_ctzll(word);
                word &= word - 1ull;
                const unsigned long long* row = P + (size_t)a * words;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int w = lane + 64 * r;
                    if (w < nw) {
                        unsigned long long need = A_s[w];
                        if (w == wi) need &= ~(1ull << (a & 63));
                        bad = bad || (need & ~row[w]) != 0ull;
                    }
                }
            }
        }
        if (bad) atomicOr(&bad_s, 1);
    }
    __syncthreads();
    for (int w = tid; w < nw; w += 1024) new_mask[w] = new_s[w];
    if (tid >= 64) return;
    int c = 0;
    if (!bad_s) {
        unsigned long long S[R];
#pragma unroll
        for (int r = 0; r < R; ++r) S[r] = lane + 64 * r < nw ? new_s[lane + 64 * r] : 0ull;
        int count = 0;
        unsigned steps = 0;
        bool go = true;
        c = ex_colour<R>(S, lane, nw, words, P, 0, nullptr, count, steps, 0xffffffffu, go);
    }
    if (lane == 0) { info[0] = bad_s ? 0 : 1; info[1] = w0_s; info[2] = m_s; info[3] = c; info[4] = 0; }
}

// levels, level_words, slice_words: those of k_ex_search, with levels = UB = min(n, w0 + c)
template <int R>
__global__ __launch_bounds__(64 * kExWaves) void k_exr_search(int words, int levels, int level_words, size_t slice_words, unsigned cap,
                                                              const unsigned long long* P, const int* ms_info, int* info,
                                                              const unsigned long long* new_mask, const int* roots,
                                                              unsigned long long* ws, int* root_flag, int* root_size,
                                                              unsigned* root_steps, unsigned short* cliques)
{
    const int lane = threadIdx.x & 63;
    const int n = ms_info[0], lb = ms_info[1], nw = (n + 63) >> 6;
    const int w0 = info[1], m = info[2];
    const int b0 = w0 > lb ? w0 : lb;
    unsigned long long* slice = ws + (size_t)(blockIdx.x * kExWaves + (threadIdx.x >> 6)) * slice_words;
    int* path = (int*)(slice + (size_t)levels * level_words);
    unsigned long long NEW[R];
#pragma unroll
    for (int r = 0; r < R; ++r) NEW[r] = lane + 64 * r < nw ? new_mask[lane + 64 * r] : 0ull;
    for (;;) {
        int rk = 0;
        if (lane == 0) rk = atomicAdd(&info[4], 1);
        rk = __builtin_amdgcn_readfirstlane(rk);
        if (rk >= m) return;
        const int p = roots[rk];
        unsigned long long S[R];
        int size0 = 0;
        {
            const unsigned long long* row = P + (size_t)p * words;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int w = lane + 64 * r;
                const unsigned long long front = w < (p >> 6) ? ~0ull : (w == (p >> 6) ? (1ull << (p & 63)) - 1ull : 0ull);
                S[r] = w < nw ? row[w] & ~(NEW[r] & front) : 0ull;
                size0 += __popcll(S[r]);
            }
        }
        for (int off = 32; off > 0; off >>= 1) size0 += __shfl_xor(size0, off);
        if (1 + size0 <= b0) {
            if (lane == 0) { root_flag[rk] = 0; root_size[rk] = 0; root_steps[rk] = 0u; }
            continue;
        }
        int best;
        bool go, found;
        const unsigned steps = ex_subproblem<R>(S, lane, p, b0, nw, words, levels, level_words, cap, P, slice, path,
                                                cliques + (size_t)rk * levels, best, found, go);
        if (lane == 0) { root_flag[rk] = go ? 1 : 2; root_size[rk] = found ? best : 0; root_steps[rk] = steps; }
    }
}

// The roots in the fixed order of k_ex_pick; `searched` = 0: no root ran (m = 0 or b0 >= UB), the incumbent stands.  accepted
// holds the set handed in: it is rewritten with the winning clique, or with the multi-start bytes where they are the incumbent
// (LB > w0), and left alone otherwise.
__global__ __launch_bounds__(1024) void k_exr_pick(int N, int levels, int searched, const int* live, const int* ms_info,
                                                   const int* root_flag, const int* root_size, const unsigned* root_steps,
                                                   const unsigned short* cliques, const unsigned char* ms_accepted, int* info,
                                                   unsigned char* accepted)
{
    __shared__ int wave_s[16], wave_q[16], wave_sub[16], wave_cap[16];
    __shared__ unsigned long long wave_steps[16];
    __shared__ int win_s, win_r;
    const int tid = threadIdx.x, lane = tid & 63;
    const int lb = ms_info[1], w0 = info[1], m = searched ? info[2] : 0;
    int bs = 0, bq = -1, sub = 0, capped = 0;
    unsigned long long steps = 0ull;
    for (int r = tid; r < m; r += 1024) {
        const int f = root_flag[r];
        ms_better(bs, bq, root_size[r], r);
        sub += f != 0;
        capped += f == 2;
        steps += root_steps[r];
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
        const int b0 = w0 > lb ? w0 : lb;
        const bool better = capped == 0 && bs > b0;
        win_s = better ? bs : b0;
        win_r = better ? bq : (w0 >= lb ? -1 : -2);
        info[5] = win_s; info[6] = win_r; info[7] = sub; info[8] = capped;
        info[9] = (int)(steps & 0xffffffffull); info[10] = (int)(steps >> 32);
        info[11] = win_r != -1;
    }
    __syncthreads();
    if (win_r == -1) return;
    if (win_r == -2) {
        for (int c = tid; c < N; c += 1024) accepted[c] = ms_accepted[c];
        return;
    }
    for (int c = tid; c < N; c += 1024) accepted[c] = 0;
    __syncthreads();
    const unsigned short* clique = cliques + (size_t)win_r * levels;
    for (int j = tid; j < win_s; j += 1024) accepted[live[clique[j]]] = 1;
}
