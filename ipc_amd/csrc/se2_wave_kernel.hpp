// Wave kernels of the SE(2) cell solver (se2_wave_cell.hpp): persistent workgroups of four
// independent waves, each solving one cell at a time from a shared work queue.
//
// Three kernel templates, one text (se2_wave_kernel_def.hpp): se2_wave_kernel re-sweeps an accepted trial to commit it;
// se2_wave_kernel_kt (kept trial) reads it back from the accumulator registers where the trial sweep parked it;
// se2_wave_kernel_lz (LAZY_SD of se2_wave_solve) forms the steepest-descent terms only where a trial reads them and
// commits as the default policy's kernel of that M does (kept trial up to M = 9, re-sweep beyond).
// se2_wave.hip instantiates the first, se2_wave_kt.hip the second, se2_wave_lz.hip the third.
#pragma once
#include "cell_kernels.hpp"
#include "se2_wave_cell.hpp"

using namespace ipc;

// Waves per workgroup: four (one per SIMD, up to 512 registers each); the shortest chains (M <= IPC_SE2_DENSE_MAXM
// poses per lane) fit 256 registers, so eight of their waves share a CU -- two per SIMD, each hiding the other's
// latencies -- and the staged chain constants.
#ifndef IPC_SE2_DENSE_MAXM
#define IPC_SE2_DENSE_MAXM 1
#endif
template <int M>
constexpr int se2_waves() { return M <= IPC_SE2_DENSE_MAXM ? 8 : 4; }

#define IPC_WAVE_KERNEL_NAME se2_wave_kernel
#define IPC_WAVE_KEEP_TRIAL false
#define IPC_WAVE_LAZY_SD false
#include "se2_wave_kernel_def.hpp"
#undef IPC_WAVE_KERNEL_NAME
#undef IPC_WAVE_KEEP_TRIAL
#define IPC_WAVE_KERNEL_NAME se2_wave_kernel_kt
#define IPC_WAVE_KEEP_TRIAL true
#include "se2_wave_kernel_def.hpp"
#undef IPC_WAVE_KERNEL_NAME
#undef IPC_WAVE_KEEP_TRIAL
#undef IPC_WAVE_LAZY_SD
#define IPC_WAVE_KERNEL_NAME se2_wave_kernel_lz
#define IPC_WAVE_KEEP_TRIAL (M <= kLazyKeepTrialMaxM)
#define IPC_WAVE_LAZY_SD true
#include "se2_wave_kernel_def.hpp"
#undef IPC_WAVE_KERNEL_NAME
#undef IPC_WAVE_KEEP_TRIAL
#undef IPC_WAVE_LAZY_SD

// (only the chosen template is instantiated: a translation unit emits the kernels it launches and no others)
template <int M, int NL, bool STAGED, bool KEEP_TRIAL, bool LAZY_SD>
constexpr auto se2_wave_kernel_of()
{
    if constexpr (LAZY_SD) return &se2_wave_kernel_lz<M, NL, STAGED>;
    else if constexpr (KEEP_TRIAL) return &se2_wave_kernel_kt<M, NL, STAGED>;
    else return &se2_wave_kernel<M, NL, STAGED>;
}

#ifndef IPC_LDS_BUDGET
#define IPC_LDS_BUDGET (160 * 1024)
#endif
constexpr int kLdsBudget = IPC_LDS_BUDGET;

template <int M, int NL, bool KEEP_TRIAL, bool LAZY_SD = false>
static hipError_t launch_wave_one(int n, hipStream_t st, const Se2View& P, const int2* cells, SolveParams prm, CellOut out,
                                  unsigned* counter, int n_cu)
{
    constexpr int kWavesPerGroup = se2_waves<M>();
    const int E = P.V - 1;
    const int wstride = E + 32;                       // padding: a partially filled lane reads up to M-1 records past the end
    const size_t scratch = kWavesPerGroup * ((sizeof(WaveScratch<NL>) + 7) / 8) * sizeof(double);
    const size_t staged = scratch + sizeof(double) * (size_t)F_SG * wstride;
    const int groups = std::max(1, std::min(n_cu, (n + kWavesPerGroup - 1) / kWavesPerGroup));
    if (staged <= (size_t)kLdsBudget) {
        auto k = se2_wave_kernel_of<M, NL, true, KEEP_TRIAL, LAZY_SD>();
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)staged);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k, dim3(groups), dim3(64 * kWavesPerGroup), staged, st, P, cells, n, counter, prm, out, 0, E, wstride);
    } else {
        auto k = se2_wave_kernel_of<M, NL, false, KEEP_TRIAL, LAZY_SD>();
        hipLaunchKernelGGL(k, dim3(groups), dim3(64 * kWavesPerGroup), scratch, st, P, cells, n, counter, prm, out, 0, E, wstride);
    }
    return hipGetLastError();
}
