// Lazy steepest-descent wave kernels of the SE(2) cell solver (se2_wave_kernel.hpp): the instantiations of
// se2_wave_kernel_lz, which form b^T H b, alpha and |h_sd| only in the iterations whose trial loop reads them (LAZY_SD of
// se2_wave_solve) and otherwise are the kernel the default policy names for that M: kept trial at M = 5, 7, 9 (kwM),
// re-sweep at M = 11, 13 (wM).  No policy token: the plan serves those bins with these kernels (IPC_SE2_LAZY_SD, cell_plan.hpp).
#include "se2_wave_kernel.hpp"

namespace ipc {
IPC_CELL_LAUNCHER(launch_se2_wave_lz, Se2View)
{
#define IPC_WCASE(MM)                                                                                                  \
    case MM:                                                                                                           \
        return nl == 1 ? launch_wave_one<MM, 1, (MM <= kLazyKeepTrialMaxM), true>(n, st, P, cells, prm, out, counter, n_cu)    \
                       : launch_wave_one<MM, 2, (MM <= kLazyKeepTrialMaxM), true>(n, st, P, cells, prm, out, counter, n_cu);
    switch (M) {
#ifdef IPC_WAVE_LZ_ONLY_M                              // (tools/isa_loop_mix.py: one instantiation, seconds to compile)
        IPC_WCASE(IPC_WAVE_LZ_ONLY_M)
#else
        IPC_SE2_WAVE_LZ_M(IPC_WCASE)
#endif
        default: return hipErrorInvalidValue;
    }
#undef IPC_WCASE
}

}  // namespace ipc
