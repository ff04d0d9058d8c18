// Multi-start set maximisation (ipc_set_max_multistart): the greedy of k_set_max started once from every live
// candidate, the largest set kept.  Included by engine.hip behind batch_kernels.hpp; no existing kernel is touched.
//
// With L = (l_0 .. l_{n-1}) the processing order restricted to the candidates whose diagonal bit is set, the set S_q of seed
// position q is the greedy over l_q, l_0, l_1, .., l_{q-1}, l_{q+1}, ..: cand = row(l_q) restricted to L minus l_q; repeat: the
// first position c still in cand joins, cand &= row(c).  S_0 is k_set_max's set; the result is the S_q of greatest cardinality,
// ties to the smallest q.  Three stages, n known on the device only (every grid is sized by N, surplus waves leave):
//   k_ms_live      one workgroup: the live list, the position map, n
//   k_ms_compact   one wave per row: P[n][stride], bit b of row a = C[l_a][l_b], diagonal cleared
//   k_ms_greedy    one wave per seed, four independent waves per workgroup, no barrier: |S_q| -- cand in registers
//                  (k_ms_greedy_reg<R>, R words per lane) or in a per-wave LDS slice (k_ms_greedy_lds)
//   k_ms_pick      one workgroup: (max size, min q) by a fixed-order reduction, the winning chain once more, the outputs
// P is in positions, so "the first candidate in processing order" is the lowest set bit and a step of the chain is a ballot of
// the non-empty words, the first lane, its first bit, one broadcast, one coalesced row load, one AND.
#pragma once

constexpr int kMsWaves = 4;                             // waves (seeds / rows) per workgroup of the grid kernels
constexpr int kMsInfo = 4;                              // info words: n, best size, best position, best candidate (-1: none)

// The live list in processing order (k_set_max's ordered compaction), pos[k] = position of candidate k in it or -1, info[0] = n.
// `stride` = words per stored row of the matrix.
__global__ __launch_bounds__(1024) void k_ms_live(int N, int stride, const int* order, const unsigned long long* bits, int* live,
                                                  int* pos, int* info)
{
    __shared__ int wcount[16];
    __shared__ int nlive_s;
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
    if (tid == 0) info[0] = nlive_s;
}

// Row a of P: lane b of trip wb asks for C[l_a][l_{64 wb + b}], the ballot is the word; the words of 64 trips are parked one per
// lane and leave in one coalesced store.  Words at and beyond ceil(n/64) are never written and never read.  `stride` = words per
// stored row of the input matrix (ipc_set_max_multistart: words; the online matrix: its capacity stride), as in k_set_max.
__global__ __launch_bounds__(64 * kMsWaves) void k_ms_compact(int words, int stride, const unsigned long long* bits, const int* live,
                                                              const int* info, unsigned long long* P)
{
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * kMsWaves + (threadIdx.x >> 6);
    const int n = info[0];
    if (a >= n) return;
    const int nw = (n + 63) >> 6;
    const unsigned long long* row = bits + (size_t)live[a] * stride;
    unsigned long long* out = P + (size_t)a * words;
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

// One lane's candidate for "first position still in cand" (its word non-empty): the position, broadcast from the first such lane.
__device__ __forceinline__ int ms_first_of(unsigned long long m, int w, unsigned long long word)
{
    const int fl = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
    const int mine = w * 64 + (word ? __builtin_ctzll(word) : 0);
    return __builtin_amdgcn_readlane(mine, fl);
}

// |S_q| with cand in registers: lane l holds the words l, l + 64, .. l + 64 (R - 1) of the nw = ceil(n/64) <= 64 R words.
template <int R>
__global__ __launch_bounds__(64 * kMsWaves) void k_ms_greedy_reg(int words, const unsigned long long* P, const int* info, int* sz)
{
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * kMsWaves + (threadIdx.x >> 6);
    const int n = info[0];
    if (q >= n) return;
    const int nw = (n + 63) >> 6;
    unsigned long long cand[R];
    {
        const unsigned long long* row = P + (size_t)q * words;
#pragma unroll
        for (int r = 0; r < R; ++r) cand[r] = lane + 64 * r < nw ? row[lane + 64 * r] : 0ull;
    }
    int size = 1;
    for (;;) {
        int c = -1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (c < 0) {
                const unsigned long long m = __ballot(cand[r] != 0ull);
                if (m) c = ms_first_of(m, lane + 64 * r, cand[r]);
            }
        }
        if (c < 0) break;
        ++size;
        const unsigned long long* row = P + (size_t)c * words;
#pragma unroll
        for (int r = 0; r < R; ++r) { if (lane + 64 * r < nw) cand[r] &= row[lane + 64 * r]; }
    }
    if (lane == 0) sz[q] = size;
}

// The chain with cand in an LDS slice of nw words that belongs to this wave alone; lane l reads and writes the words l, l + 64, ..
// and no other, so nothing orders LDS accesses between lanes.  The AND pass of a step also finds the first position left (the
// next member); trips in front of t0 are empty for good (cand only shrinks).  `member`, when given, gets every member's byte.
__device__ __forceinline__ int ms_chain_lds(int q, int nw, int words, const unsigned long long* P, unsigned long long* cand,
                                            const int* live, unsigned char* member)
{
    const int lane = threadIdx.x & 63;
    const int trips = (nw + 63) >> 6;
    int c = q, size = 0, t0 = 0;
    bool first = true;
    while (c >= 0) {
        ++size;
        if (member && lane == 0) member[live[c]] = 1;
        const unsigned long long* row = P + (size_t)c * words;
        int next = -1;
        for (int t = t0; t < trips; ++t) {
            const int w = lane + 64 * t;
            unsigned long long word = 0ull;
            if (w < nw) {
                word = first ? row[w] : (cand[w] & row[w]);
                cand[w] = word;
            }
            if (next < 0) {
                const unsigned long long m = __ballot(word != 0ull);
                if (m) next = ms_first_of(m, w, word);
                else t0 = t + 1;
            }
        }
        first = false;
        c = next;
    }
    return size;
}

__global__ __launch_bounds__(64 * kMsWaves) void k_ms_greedy_lds(int words, int wpb, const unsigned long long* P, const int* info, int* sz)
{
    extern __shared__ unsigned long long ms_cand[];     // [wpb][words]
    const int wave = threadIdx.x >> 6;             // (the block is wpb waves)
    const int q = blockIdx.x * wpb + wave;
    const int n = info[0];
    if (q >= n) return;
    const int size = ms_chain_lds(q, (n + 63) >> 6, words, P, ms_cand + (size_t)wave * words, nullptr, nullptr);
    if ((threadIdx.x & 63) == 0) sz[q] = size;
}

// (max size, min q): every thread over its positions in ascending order, then the lanes of a wave, then the sixteen waves in turn;
// at every comparison the greater size wins and, at equal size, the lower position -- the order of the comparisons is fixed and
// nothing depends on which wave runs first.  Then accepted and sizes are cleared / filled, and wave 0 walks the winning chain
// once more and sets its members.
__device__ __forceinline__ void ms_better(int& bs, int& bq, int s, int q)
{
    if (q >= 0 && (s > bs || (s == bs && q < bq))) { bs = s; bq = q; }
}
__global__ __launch_bounds__(1024) void k_ms_pick(int N, int words, const unsigned long long* P, const int* live, const int* pos,
                                                  const int* sz, int* info, unsigned char* accepted, int* sizes)
{
    extern __shared__ unsigned long long ms_cand[];     // [words]
    __shared__ int wave_s[16], wave_q[16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = info[0];
    int bs = 0, bq = -1;
    for (int q = tid; q < n; q += 1024) ms_better(bs, bq, sz[q], q);
    for (int off = 32; off > 0; off >>= 1) {
        const int s = __shfl_down(bs, off), q = __shfl_down(bq, off);
        ms_better(bs, bq, s, q);
    }
    if (lane == 0) { wave_s[tid >> 6] = bs; wave_q[tid >> 6] = bq; }
    for (int k = tid; k < N; k += 1024) {
        accepted[k] = 0;
        if (sizes) { const int a = pos[k]; sizes[k] = a >= 0 ? sz[a] : 0; }
    }
    __syncthreads();
    bs = 0; bq = -1;
    for (int v = 0; v < 16; ++v) ms_better(bs, bq, wave_s[v], wave_q[v]);
    if (tid == 0) { info[1] = bs; info[2] = bq; info[3] = bq >= 0 ? live[bq] : -1; }
    if (bq < 0 || tid >= 64) return;
    ms_chain_lds(bq, (n + 63) >> 6, words, P, ms_cand, live, accepted);
}
