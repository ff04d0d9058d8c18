// Group kernels of the SE(2) cell solver (se2_wave_cell.hpp with W = 2 or 4): persistent
// workgroups of four waves; W cooperating waves solve one cell at a time from a shared work queue
// (W = 2: two independent pairs per workgroup; W = 4: the whole workgroup on one cell).
#pragma once
#include "cell_kernels.hpp"
#include "se2_wave_cell.hpp"

namespace ipc {

constexpr int kWavesPerGroup = 4;
#ifndef IPC_LDS_BUDGET
#define IPC_LDS_BUDGET (160 * 1024)
#endif
constexpr int kLdsBudget = IPC_LDS_BUDGET;

// Three kernel templates, one text (se2_group_kernel_def.hpp): se2_group_kernel re-sweeps an accepted trial to commit it;
// se2_group_kernel_kt (kept trial) reads it back from the accumulator registers where the trial sweep parked it;
// se2_group_kernel_lz (LAZY_SD of se2_wave_solve) forms the steepest-descent terms only where a trial reads them and
// commits as the default policy's kernel of that M does (kept trial up to M = 9, re-sweep beyond).
#define IPC_GROUP_KERNEL_NAME se2_group_kernel
#define IPC_GROUP_KEEP_TRIAL false
#define IPC_GROUP_LAZY_SD false
#include "se2_group_kernel_def.hpp"
#undef IPC_GROUP_KERNEL_NAME
#undef IPC_GROUP_KEEP_TRIAL
#define IPC_GROUP_KERNEL_NAME se2_group_kernel_kt
#define IPC_GROUP_KEEP_TRIAL true
#include "se2_group_kernel_def.hpp"
#undef IPC_GROUP_KERNEL_NAME
#undef IPC_GROUP_KEEP_TRIAL
#undef IPC_GROUP_LAZY_SD
#define IPC_GROUP_KERNEL_NAME se2_group_kernel_lz
#define IPC_GROUP_KEEP_TRIAL (M <= kLazyKeepTrialMaxM)
#define IPC_GROUP_LAZY_SD true
#include "se2_group_kernel_def.hpp"
#undef IPC_GROUP_KERNEL_NAME
#undef IPC_GROUP_KEEP_TRIAL
#undef IPC_GROUP_LAZY_SD

// (only the chosen template is instantiated: a translation unit emits the kernels it launches and no others)
template <int W, int M, int NL, bool STAGED, bool KEEP_TRIAL, bool LAZY_SD>
constexpr auto se2_group_kernel_of()
{
    if constexpr (LAZY_SD) return &se2_group_kernel_lz<W, M, NL, STAGED>;
    else if constexpr (KEEP_TRIAL) return &se2_group_kernel_kt<W, M, NL, STAGED>;
    else return &se2_group_kernel<W, M, NL, STAGED>;
}

template <int W, int M, int NL, bool KEEP_TRIAL = false, bool LAZY_SD = false>
static hipError_t launch_group(int n, hipStream_t st, const Se2View& P, const int2* cells, SolveParams prm, CellOut out,
                              unsigned* counter, int n_cu)
{
    const int E = P.V - 1;
    const int wstride = E + 32;
    constexpr int kPairs = kWavesPerGroup / W;
    const size_t scratch = kPairs * (((sizeof(WaveScratch<NL>) + 7) / 8) + ((sizeof(PairBox) + 7) / 8)) * sizeof(double);
    const size_t staged = scratch + sizeof(double) * (size_t)F_SG * wstride;
    const int groups = std::max(1, std::min(n_cu, (n + kPairs - 1) / kPairs));
    if (staged <= (size_t)kLdsBudget) {
        auto k = se2_group_kernel_of<W, M, NL, true, KEEP_TRIAL, LAZY_SD>();
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)staged);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k, dim3(groups), dim3(64 * kWavesPerGroup), staged, st, P, cells, n, counter, prm, out, 0, E, wstride);
    } else {
        auto k = se2_group_kernel_of<W, M, NL, false, KEEP_TRIAL, LAZY_SD>();
        hipLaunchKernelGGL(k, dim3(groups), dim3(64 * kWavesPerGroup), scratch, st, P, cells, n, counter, prm, out, 0, E, wstride);
    }
    return hipGetLastError();
}

}  // namespace ipc
