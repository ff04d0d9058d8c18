// Block kernels of the SE(2) cell solver (se2_cell.hpp): one workgroup per cell.
#include "cell_kernels.hpp"
#include "se2_cell.hpp"

using namespace ipc;

// ------------------------------------------------------------------------------------------
// the hot kernel
// ------------------------------------------------------------------------------------------
// M == 1 variants are held to 128 VGPRs (4 waves per SIMD => 16 waves per CU: two 8-wave cells
// or four 4-wave cells in flight per CU, so one cell's barrier waits hide behind another's work)
#ifndef IPC_MINW
#define IPC_MINW 1
#endif
template <int W, int M, int NL>
__global__ __launch_bounds__(64 * W, (M == 1 ? IPC_MINW : (W == 2 ? 2 : 1))) void se2_cells_kernel(Se2View P, const int2* cells, int ncells,
                                                           SolveParams prm, CellOut out)
{
    __shared__ Se2Shared<W, M, NL> sh;
    const int cell = blockIdx.x;
    if (cell >= ncells) return;
    const int2 cc = cells[cell];
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
    se2_solve_cell<W, M, NL>(P, lo, L, cand, iterations, sh, r);
    if (threadIdx.x == 0) {
        out.max_chi2[cell] = r.max_chi2;
        out.chi2_total[cell] = r.chi2_total;
        out.meta[cell] = make_int4(r.iterations, r.tries, r.flags, r.evals);
    }
}

template <int NL>
static hipError_t launch_se2(int W, int M, int n, hipStream_t st, const Se2View& P, const int2* cells,
                             SolveParams prm, CellOut out)
{
#define IPC_CASE(WW, MM)                                                                          \
    case cell_wm(WW, MM):                                                                         \
        hipLaunchKernelGGL((se2_cells_kernel<WW, MM, NL>), dim3(n), dim3(64 * WW), 0, st, P, cells, n, prm, out); \
        break;
    switch (cell_wm(W, M)) {
        IPC_SE2_BLOCK_WM(IPC_CASE)
        default: return hipErrorInvalidValue;
    }
#undef IPC_CASE
    return hipGetLastError();
}


namespace ipc {
IPC_CELL_LAUNCHER(launch_se2_block, Se2View)
{
    return nl == 1 ? launch_se2<1>(W, M, n, st, P, cells, prm, out) : launch_se2<2>(W, M, n, st, P, cells, prm, out);
}
}  // namespace ipc
