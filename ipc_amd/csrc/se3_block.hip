// Block kernels of the SE(3) cell solver (se3_cell.hpp): one workgroup per cell.
#include "cell_kernels.hpp"
#include "se2_cell.hpp"                              // SolveParams
#include "se3_cell.hpp"

using namespace ipc;

// ---- SE3 cell kernel: same contract; variants kept few (the code is large) ----
template <int W, int M, int NL>
__global__ __launch_bounds__(64 * W) void se3_cells_kernel(Se3View P, const int2* cells, int ncells,
                                                           SolveParams prm, CellOut out)
{
    __shared__ Se3Shared<W, M, NL> sh;
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
    CellResult3 r;
    se3_solve_cell<W, M, NL>(P, lo, L, cand, iterations, sh, r);
    if (threadIdx.x == 0) {
        out.max_chi2[cell] = r.max_chi2;
        out.chi2_total[cell] = r.chi2_total;
        out.meta[cell] = make_int4(r.iterations, r.tries, r.flags, r.evals);
    }
}

template <int NL>
static hipError_t launch_se3(int W, int M, int n, hipStream_t st, const Se3View& P, const int2* cells,
                             SolveParams prm, CellOut out)
{
#define IPC_CASE3(WW, MM)                                                                         \
    case cell_wm(WW, MM):                                                                         \
        hipLaunchKernelGGL((se3_cells_kernel<WW, MM, NL>), dim3(n), dim3(64 * WW), 0, st, P, cells, n, prm, out); \
        break;
    switch (cell_wm(W, M)) {
        IPC_SE3_BLOCK_WM(IPC_CASE3)
        default: return hipErrorInvalidValue;
    }
#undef IPC_CASE3
    return hipGetLastError();
}


namespace ipc {
IPC_CELL_LAUNCHER(launch_se3_block, Se3View)
{
    return nl == 1 ? launch_se3<1>(W, M, n, st, P, cells, prm, out) : launch_se3<2>(W, M, n, st, P, cells, prm, out);
}
}  // namespace ipc
