// Threshold sweep (ipc_run_sweep): the cells are solved once, these kernels decide them at many
// (fast_reject_th, slow_reject_th) pairs.  Included by engine.hip behind slot_of_cell, assemble_tiles and set_max_rounds,
// whose tile scheme and round logic the batched kernels share with k_assemble_delta and k_set_max.
//
// Per cell the sweep holds chi0 (the first pass; for a cell whose linear solve failed, the Levenberg retry's value), a literal
// chi2 and a flag word: bit 0 = the literal record is held, bit 1 = the first pass ended with flags & 2 and was retried (no
// band test, k_collect_failed's `failed` branch).  The rule at a threshold th -- fast on the diagonal, slow elsewhere -- is the
// one k_collect_failed and k_scatter_bits apply on a fresh engine:
//     chi2 = (not retried && band > 0 && fabs(chi0 - th) <= band * th) ? literal : chi0;      bit = !(chi2 > th)
// The thresholds of a call sit in one small device array [fast 0 .. T-1][slow 0 .. T-1]; the index is wave-uniform.
#pragma once

constexpr int kSweepHeld = 1, kSweepRetried = 2;

__device__ __forceinline__ bool sweep_borderline(double chi0, double th, double band)
{
    return fabs(chi0 - th) <= band * th;                          // (NaN: no) -- the expression of k_collect_failed
}

// Before the Levenberg retry overwrites the records: which cells it will replace.  Nothing is held yet.
__global__ void k_sweep_init_flags(int ncells, const int4* meta, bool want_failed, int* flags)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < ncells) flags[c] = (want_failed && (meta[c].z & 2)) ? kSweepRetried : 0;
}

// Cells that some pair of the call makes borderline and whose literal record is not held yet -> the compact list of their slot
// (lit_cells / lit_idx at the slot's own offset, counted in recount[0 .. nslots)); those of the long slots, which no cell
// kernel re-solves, -> the host list, counted in recount[nslots] (k_collect_failed's bookkeeping).
__global__ void k_sweep_collect(int ncells, const int* flags, const double* chi0, const int2* cells, int n_th, const double* fast_th,
                                const double* slow_th, double band, int cap, int* list, int* recount, const unsigned* slot_off,
                                int nslots, int2* lit_cells, int* lit_idx, int long_bin)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    if (flags[c]) return;                                         // retried (rule 1: no band test) or held already
    const int2 cc = cells[c];
    const double x = chi0[c];
    const double* th = cc.x == cc.y ? fast_th : slow_th;
    bool border = false;
    for (int t = 0; t < n_th && !border; ++t) border = sweep_borderline(x, th[t], band);
    if (!border) return;
    const int sl = slot_of_cell(slot_off, nslots, c);
    if (sl == long_bin || sl == (nslots >> 1) + long_bin) {
        const int q = atomicAdd(recount + nslots, 1);
        if (q < cap) list[q] = c;
        return;
    }
    const int q = atomicAdd(recount + sl, 1);
    lit_cells[slot_off[sl] + q] = cc;
    lit_idx[slot_off[sl] + q] = c;
}

// The literal re-solves of this call into the held records (k_scatter_literal's addressing; only chi2 is kept: the cell
// records ipc_cell_info shows after a sweep are the first pass's).
__global__ void k_sweep_keep_literal(int ncells, const unsigned* slot_off, int nslots, const int* recount, const int* lit_idx,
                                     const double* lit_chi, double* literal, int* flags)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncells) return;
    const int sl = slot_of_cell(slot_off, nslots, t);
    if ((int)(t - slot_off[sl]) >= recount[sl]) return;
    const int c = lit_idx[t];
    literal[c] = lit_chi[t];
    flags[c] |= kSweepHeld;
}

// Cell results -> the upper-triangle bits of the chunk's TC matrices ([t][N][words], rows by the identity map).  A cell's
// record is read once; the rule is applied per pair.
__global__ void k_sweep_scatter(int ncells, const int2* cells, const double* chi0, const double* literal, const int* flags, int tc,
                                const double* fast_th, const double* slow_th, double band, int words, size_t mat,
                                unsigned long long* upper)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    const int2 cc = cells[c];
    const double x = chi0[c], lit = literal[c];
    const int f = flags[c];
    const bool banded = band > 0.0 && !(f & kSweepRetried);
    const double* th = cc.x == cc.y ? fast_th : slow_th;
    unsigned long long* dst = upper + (size_t)cc.x * words + (cc.y >> 6);
    const unsigned long long bit = 1ull << (cc.y & 63);
    for (int t = 0; t < tc; ++t) {
        const double tht = th[t];
        const double chi = (banded && sweep_borderline(x, tht, band)) ? lit : x;     // (borderline => held: k_sweep_collect saw every pair of the call)
        if (!(chi > tht)) atomicOr(dst + (size_t)t * mat, bit);                       // consensus_utils.cpp:18 (NaN agrees, as there)
    }
}

// k_assemble's tile scheme, the threshold as the third grid dimension: matrix t of the chunk from upper triangle t.
__global__ __launch_bounds__(256) void k_sweep_assemble(int N, int words, size_t mat, const int* lo, const int* hi,
                                                        const unsigned long long* upper, unsigned long long* bits)
{
    const size_t off = (size_t)blockIdx.z * mat;
    assemble_tiles(N, 0, words, lo, hi, upper + off, bits + off);
}

// One 1 024-thread workgroup per threshold, side by side: its own LDS mask, live list [t][N] and accepted bytes [t][N]; the
// rounds are those of k_set_max(first = 0).
__global__ __launch_bounds__(1024) void k_sweep_set_max(int N, int words, size_t mat, const int* order, const unsigned long long* bits,
                                                        unsigned char* accepted, int* live)
{
    const size_t t = blockIdx.x;
    set_max_rounds(N, words, words, order, bits + t * mat, accepted + t * (size_t)N, live + t * (size_t)N, 0, nullptr, nullptr);
}
