// Definition of ONE wave kernel template of the SE(2) cell solver; se2_wave_kernel.hpp includes this file once per
// kernel, with
//   IPC_WAVE_KERNEL_NAME   name of the __global__ template
//   IPC_WAVE_KEEP_TRIAL    KEEP_TRIAL of se2_wave_solve: false, an accepted trial is re-swept to commit; true, it is
//                          read back from the accumulator registers where the trial sweep parked it
//   IPC_WAVE_LAZY_SD       LAZY_SD of se2_wave_solve: true, the steepest-descent terms are formed only where a trial reads them
// (no include guard; one text for all kernels and no function between the kernel and se2_wave_solve, for the reason
// given in se2_group_kernel_def.hpp).
template <int M, int NL, bool STAGED>
__global__ __launch_bounds__((64 * se2_waves<M>()), 1) void IPC_WAVE_KERNEL_NAME(Se2View P, const int2* cells, int ncells,
                                                                               unsigned* counter, SolveParams prm,
                                                                               CellOut out, int wlo, int wlen, int wstride)
{
    extern __shared__ double dyn_lds[];
    constexpr int kWavesPerGroup = se2_waves<M>();
    constexpr int kScratchDoubles = (sizeof(WaveScratch<NL>) + 7) / 8;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    WaveScratch<NL>& sh = *reinterpret_cast<WaveScratch<NL>*>(dyn_lds + wave * kScratchDoubles);
    double* cst = dyn_lds + kWavesPerGroup * kScratchDoubles;
    if (STAGED) {
        // residual-pass constants of the whole window, once per workgroup (rows padded with zeros)
        for (int f = 0; f < (int)F_SG; ++f)
            for (int i = threadIdx.x; i < wstride; i += 64 * kWavesPerGroup)
                cst[i * (int)F_SG + f] = i < wlen ? P.chain[(size_t)f * P.estride + wlo + i] : 0.0;
    }
    __syncthreads();
    for (;;) {
        unsigned c = 0;
        if (lane == 0) c = atomicAdd(counter, 1u);
        c = (unsigned)__builtin_amdgcn_readfirstlane((int)c);
        if (c >= (unsigned)ncells) break;
        const int2 cc = cells[c];
        int cand[2] = {cc.x, cc.y};
        int lo = min(P.cand_from[cc.x], P.cand_to[cc.x]), hi = max(P.cand_from[cc.x], P.cand_to[cc.x]);
        if (NL == 2) {
            lo = min(lo, min(P.cand_from[cc.y], P.cand_to[cc.y]));
            hi = max(hi, max(P.cand_from[cc.y], P.cand_to[cc.y]));
        }
        const int L = hi - lo;
        const int base = NL == 1 ? prm.fast_iter : prm.slow_iter;
        const int iterations = (L + NL > 100) ? base * 5 : base;       // consensus_utils.cpp:12-13
        CellResult r;
        se2_wave_solve<M, NL, STAGED, 1, se2_err_store<M>(), IPC_WAVE_KEEP_TRIAL, IPC_WAVE_LAZY_SD>(P, lo, L, cand, iterations, sh, cst,
                                                                                                    wlo, wstride, r);
        if (lane == 0) {
            out.max_chi2[c] = r.max_chi2;
            out.chi2_total[c] = r.chi2_total;
            out.meta[c] = make_int4(r.iterations, r.tries, r.flags, r.evals);
        }
        wave_sync();                                  // the scratch is reused by the next cell
    }
}
