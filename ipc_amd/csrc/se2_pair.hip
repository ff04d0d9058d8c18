// Pair kernels of the SE(2) cell solver: two waves per cell (se2_group_kernel.hpp with W = 2).
#include "se2_group_kernel.hpp"

namespace ipc {
IPC_CELL_LAUNCHER(launch_se2_pair, Se2View)
{
#define IPC_PCASE(MM)                                                                              \
    case MM:                                                                                       \
        return nl == 1 ? launch_group<2, MM, 1>(n, st, P, cells, prm, out, counter, n_cu)          \
                       : launch_group<2, MM, 2>(n, st, P, cells, prm, out, counter, n_cu);
    switch (M) {
#ifdef IPC_PAIR_ONLY_M                                 // (tools/maxilp_repro.py: one instantiation, seconds to compile)
        IPC_PCASE(IPC_PAIR_ONLY_M)
#else
        IPC_SE2_PAIR_M(IPC_PCASE)
#endif
        default: return hipErrorInvalidValue;
    }
#undef IPC_PCASE
}
}  // namespace ipc
