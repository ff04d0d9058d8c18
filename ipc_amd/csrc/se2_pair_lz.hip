// Lazy steepest-descent pair kernels of the SE(2) cell solver: two waves per cell (se2_group_kernel.hpp with W = 2), the
// instantiations of se2_group_kernel_lz, which form b^T H b, alpha and |h_sd| only in the iterations whose trial loop
// reads them (LAZY_SD of se2_wave_solve) and otherwise are the kernel the default policy names for that M: kept trial at
// M = 7, 9 (kpM), re-sweep at M = 11 (p11).  No policy token: the plan serves those bins with these kernels
// (IPC_SE2_LAZY_SD, cell_plan.hpp).
#include "se2_group_kernel.hpp"

namespace ipc {
IPC_CELL_LAUNCHER(launch_se2_pair_lz, Se2View)
{
#define IPC_PCASE(MM)                                                                                                  \
    case MM:                                                                                                           \
        return nl == 1 ? launch_group<2, MM, 1, (MM <= kLazyKeepTrialMaxM), true>(n, st, P, cells, prm, out, counter, n_cu)    \
                       : launch_group<2, MM, 2, (MM <= kLazyKeepTrialMaxM), true>(n, st, P, cells, prm, out, counter, n_cu);
    switch (M) {
#ifdef IPC_PAIR_LZ_ONLY_M                              // (tools/isa_loop_mix.py: one instantiation, seconds to compile)
        IPC_PCASE(IPC_PAIR_LZ_ONLY_M)
#else
        IPC_SE2_PAIR_LZ_M(IPC_PCASE)
#endif
        default: return hipErrorInvalidValue;
    }
#undef IPC_PCASE
}
}  // namespace ipc
