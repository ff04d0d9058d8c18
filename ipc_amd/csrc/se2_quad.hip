// Quad kernels of the SE(2) cell solver: the four waves of a workgroup on one cell
// (se2_group_kernel.hpp with W = 4), for chains beyond what a wave pair holds in registers.
#include "se2_group_kernel.hpp"

namespace ipc {
IPC_CELL_LAUNCHER(launch_se2_quad, Se2View)
{
#define IPC_PCASE(MM)                                                                              \
    case MM:                                                                                       \
        return nl == 1 ? launch_group<4, MM, 1>(n, st, P, cells, prm, out, counter, n_cu)          \
                       : launch_group<4, MM, 2>(n, st, P, cells, prm, out, counter, n_cu);
    switch (M) {
        IPC_SE2_QUAD_M(IPC_PCASE)
        default: return hipErrorInvalidValue;
    }
#undef IPC_PCASE
}
}  // namespace ipc
