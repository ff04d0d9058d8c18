// Kept-trial pair kernels of the SE(2) cell solver: two waves per cell (se2_group_kernel.hpp with W = 2), the
// instantiations of se2_group_kernel_kt, which commit an accepted trial from the poses its sweep parked in accumulator
// registers.  Policy tokens "kpM".
#include "se2_group_kernel.hpp"

namespace ipc {
IPC_CELL_LAUNCHER(launch_se2_pair_kt, Se2View)
{
#define IPC_PCASE(MM)                                                                              \
    case MM:                                                                                       \
        return nl == 1 ? launch_group<2, MM, 1, true>(n, st, P, cells, prm, out, counter, n_cu)    \
                       : launch_group<2, MM, 2, true>(n, st, P, cells, prm, out, counter, n_cu);
    switch (M) {
#ifdef IPC_PAIR_KT_ONLY_M                              // (tools/isa_loop_mix.py: one instantiation, seconds to compile)
        IPC_PCASE(IPC_PAIR_KT_ONLY_M)
#else
        IPC_SE2_PAIR_KT_M(IPC_PCASE)
#endif
        default: return hipErrorInvalidValue;
    }
#undef IPC_PCASE
}
}  // namespace ipc
