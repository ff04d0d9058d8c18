// Monte-Carlo batch (ipc_run_batch): R candidate lists ("runs") drawn from the engine's list, the union U.  The
// cells that some run needs are solved once, in union indices, by the engine's own planner rule and cell kernels; these kernels
// plan them and turn their records into every run's own matrix and consistent set.  Included by engine.hip behind BinCaps (cell_plan.hpp),
// k_plan's constants, assemble_tiles and set_max_rounds, whose tile scheme and round logic the per-run kernels share with
// k_assemble_delta, k_set_max and the k_sweep_* kernels.
//
// memb [N_u][mw], mw = ceil(R / 64): bit r of candidate u's words = u is a member of run r.  A cell (i, j >= i) is needed iff the
// words of i and j intersect.  Per chunk of runs (the runs c0 .. c0 + n - 1 of the call) the host uploads a descriptor per run
// and loc [n][N_u]: the local index of a union candidate in the run, -1 for a non-member.  A run's vectors (accepted, live,
// lo, hi, order, members) sit at vec_off in the chunk's areas, its upper triangle and matrix ([N_r][words_r] words) at mat_off.
#pragma once

struct BatchRun { int n, words, vec_off, pad; long long mat_off; };

// k_plan (phase 0, world 1) with one more condition: the cell exists only if some run holds both candidates.  Same rule, same
// counter layout [slot][kPlanSub], same row order (`rowperm`: a bin's list ends up sorted by chain position, see k_plan) and the
// same wave-aggregated append.  The count pass (fill = 0) also adds, per cell, the number of runs that hold both candidates to
// *sep -- the cells R separate ipc_run calls would solve -- reduced over the wave, one atomic per wave.
__global__ void k_plan_batch(int N, const int* lo, const int* hi, const int* rowperm, int nrows, BinCaps bc, unsigned* counters,
                             const unsigned* offsets, int2* cells, int fill, const unsigned long long* memb, int mw,
                             unsigned long long* sep)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;          // this thread's candidate, its interval read once
    const int loj = j < N ? lo[j] : 0, hij = j < N ? hi[j] : 0;
    const int lane = threadIdx.x & 63;
    const int chunk = (nrows + kPlanSub - 1) / kPlanSub;
    for (int u = blockIdx.y; u < chunk * kPlanSub; u += gridDim.y) {
        const int sub = u & (kPlanSub - 1);
        const int q = sub * chunk + (u / kPlanSub);               // position in the row order
        if (q >= nrows || (u / kPlanSub) >= chunk) continue;
        const int i = rowperm[q];
        if ((int)((blockIdx.x + 1) * blockDim.x) <= i) continue;  // this block's candidates all precede row i (j < i)
        int slot = -1;
        if (j < N && j >= i) {
            const int loi = lo[i], hii = hi[i];
            if (j == i) slot = bin_of(bc, hii - loi);
            else if (min(hii, hij) - max(loi, loj) > 0)           // reference src/consensus.cpp:157-159
                slot = (kMaxBins + 1) + bin_of(bc, max(hii, hij) - min(loi, loj));
        }
        int shared = 0;                                           // runs that hold both i and j
        if (slot >= 0) {
            const unsigned long long* mi = memb + (size_t)i * mw;
            const unsigned long long* mj = memb + (size_t)j * mw;
            for (int w = 0; w < mw; ++w) shared += __popcll(mi[w] & mj[w]);
            if (!shared) slot = -1;
        }
        if (!fill && __ballot(shared > 0)) {                      // (wave-uniform: every lane or none)
            int s = shared;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
            if (lane == 0) atomicAdd(sep, (unsigned long long)s);
        }
        // wave-aggregated append: one atomic per (wave, slot present)
        unsigned long long todo = __ballot(slot >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int sl = __shfl(slot, leader, 64);
            const unsigned long long same = __ballot(slot == sl);
            const int nsame = __popcll(same);
            unsigned base = 0;
            const int sc = sl * kPlanSub + sub;
            if (lane == leader) base = atomicAdd(&counters[sc], (unsigned)nsame);
            base = __shfl(base, leader, 64);
            if (slot == sl && fill) {
                const int rnk = __popcll(same & ((1ull << lane) - 1ull));
                cells[offsets[sc] + base + rnk] = make_int2(i, j);
            }
            todo &= ~same;
        }
    }
}

// The intervals of each run's members in local order: lo_r[k] = lo[member[k]], hi_r likewise.  Run = blockIdx.y.
__global__ void k_batch_gather(const BatchRun* runs, const int* members, const int* lo, const int* hi, int* lo_r, int* hi_r)
{
    const BatchRun d = runs[blockIdx.y];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d.n) return;
    const int m = members[d.vec_off + k];
    lo_r[d.vec_off + k] = lo[m];
    hi_r[d.vec_off + k] = hi[m];
}

// Cell results -> the upper-triangle bits of the chunk's runs.  One thread per solved cell, the rule of k_scatter_bits; the
// bit goes to every run c0 .. c0 + n - 1 that holds both candidates, at the run's local indices (members are increasing, so
// i <= j gives loc i <= loc j) and the run's own stride.
__global__ void k_batch_scatter(int ncells, const int2* cells, const double* chi, double fast_th, double slow_th,
                                const unsigned long long* memb, int mw, int c0, int n, int N, const BatchRun* runs, const int* loc,
                                unsigned long long* upper)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    const int2 cc = cells[c];
    const double th = cc.x == cc.y ? fast_th : slow_th;
    if (chi[c] > th) return;                                      // consensus_utils.cpp:18 (NaN agrees, as there)
    const int c1 = c0 + n - 1;
    for (int w = c0 >> 6; w <= (c1 >> 6); ++w) {
        unsigned long long both = memb[(size_t)cc.x * mw + w] & memb[(size_t)cc.y * mw + w];
        if (w == (c0 >> 6)) both &= ~0ull << (c0 & 63);           // the runs of this chunk only
        if (w == (c1 >> 6) && (c1 & 63) != 63) both &= (1ull << ((c1 & 63) + 1)) - 1ull;
        while (both) {
            const int r = (w << 6) + __ffsll((long long)both) - 1 - c0;
            both &= both - 1ull;
            const BatchRun d = runs[r];
            const int li = loc[(size_t)r * N + cc.x], lj = loc[(size_t)r * N + cc.y];
            atomicOr(upper + d.mat_off + (size_t)li * d.words + (lj >> 6), 1ull << (lj & 63));
        }
    }
}

// k_assemble's tile scheme, the run as the third grid dimension.  The grid is that of the chunk's largest run: a block beyond
// this run's words or row tiles leaves before any ballot (both tests are uniform over the block).
__global__ __launch_bounds__(256) void k_batch_assemble(const BatchRun* runs, const int* lo_r, const int* hi_r,
                                                        const unsigned long long* upper, unsigned long long* bits)
{
    const BatchRun d = runs[blockIdx.z];
    if ((int)blockIdx.x >= d.words || (int)(blockIdx.y * 4) > ((d.n - 1) >> 6)) return;
    assemble_tiles(d.n, 0, d.words, lo_r + d.vec_off, hi_r + d.vec_off, upper + d.mat_off, bits + d.mat_off);
}

// One 1 024-thread workgroup per run, side by side: its own LDS mask (dynamic LDS for the chunk's largest words_r), live list
// and accepted bytes; the rounds are those of k_set_max(first = 0) over the run's own order.
__global__ __launch_bounds__(1024) void k_batch_set_max(const BatchRun* runs, const int* order_r, const unsigned long long* bits,
                                                        unsigned char* accepted, int* live)
{
    const BatchRun d = runs[blockIdx.x];
    set_max_rounds(d.n, d.words, d.words, order_r + d.vec_off, bits + d.mat_off, accepted + d.vec_off, live + d.vec_off, 0, nullptr,
                   nullptr);
}
