// Definition of ONE group kernel template of the SE(2) cell solver; se2_group_kernel.hpp includes this file once per
// kernel, with
//   IPC_GROUP_KERNEL_NAME   name of the __global__ template
//   IPC_GROUP_KEEP_TRIAL    KEEP_TRIAL of se2_wave_solve: false, an accepted trial is re-swept to commit; true, it is
//                           read back from the accumulator registers where the trial sweep parked it
//   IPC_GROUP_LAZY_SD       LAZY_SD of se2_wave_solve: true, the steepest-descent terms are formed only where a trial reads them
// (no include guard).  One text for all kernels, and no function between the kernel and se2_wave_solve: routed through
// a shared, force-inlined body the instantiations of se2_group_kernel compile to different code (registers, spills, loop
// layout) than they did as a kernel of their own, and their loop bodies are held to committed tables instruction by
// instruction (tests/test_se2_loop_mix.py, tests/test_se2_keep_errors_loop_mix.py).
//
// The four waves of a workgroup form 4 / W teams, each team solves one cell together (wave w of the
// team owns poses 64 M w + 1 .. 64 M (w + 1)); the teams are independent and share the staged chain
// constants.
template <int W, int M, int NL, bool STAGED>
__global__ __launch_bounds__(64 * kWavesPerGroup, 1) void IPC_GROUP_KERNEL_NAME(Se2View P, const int2* cells, int ncells,
                                                                                unsigned* counter, SolveParams prm,
                                                                                CellOut out, int wlo, int wlen, int wstride)
{
    extern __shared__ double dyn_lds[];
    constexpr int kPairs = kWavesPerGroup / W;
    constexpr int kScratchDoubles = (sizeof(WaveScratch<NL>) + 7) / 8;
    constexpr int kBoxDoubles = (sizeof(PairBox) + 7) / 8;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, pair = wave / W, wsub = wave & (W - 1);
    WaveScratch<NL>& sh = *reinterpret_cast<WaveScratch<NL>*>(dyn_lds + pair * kScratchDoubles);
    PairBox* box = reinterpret_cast<PairBox*>(dyn_lds + kPairs * kScratchDoubles + pair * kBoxDoubles);
    double* cst = dyn_lds + kPairs * (kScratchDoubles + kBoxDoubles);
    if (STAGED) {
        for (int f = 0; f < (int)F_SG; ++f)
            for (int i = threadIdx.x; i < wstride; i += 64 * kWavesPerGroup)
                cst[i * (int)F_SG + f] = i < wlen ? P.chain[(size_t)f * P.estride + wlo + i] : 0.0;
    }
    if (lane == 0) box->flag[wsub] = 0;
    __syncthreads();
    int seq = 0;
    for (;;) {
        // the team's first wave takes a cell from the queue and tells the others
        ++seq;
        unsigned c = 0;
        if (wsub == 0 && lane == 0) {
            c = atomicAdd(counter, 1u);
            mb_store(&box->data[0][seq & 1][0], (double)c);
        }
        wave_sync();
        if (lane == 0) __hip_atomic_store(&box->flag[wsub], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
        for (int o = 0; o < W; ++o) {
            if (o == wsub) continue;
            while (__hip_atomic_load(&box->flag[o], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - seq < 0)
                IPC_SPIN_WAIT();
        }
        wave_sync();
        c = (unsigned)mb_load(&box->data[0][seq & 1][0]);
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
        se2_wave_solve<M, NL, STAGED, W, se2_err_store<M>(), IPC_GROUP_KEEP_TRIAL, IPC_GROUP_LAZY_SD>(P, lo, L, cand, iterations, sh, cst,
                                                                                                      wlo, wstride, r, box, seq, &seq);
        if (wsub == 0 && lane == 0) {
            out.max_chi2[c] = r.max_chi2;
            out.chi2_total[c] = r.chi2_total;
            out.meta[c] = make_int4(r.iterations, r.tries, r.flags, r.evals);
        }
        wave_sync();
    }
}
