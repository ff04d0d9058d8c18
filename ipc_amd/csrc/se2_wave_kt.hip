// Kept-trial wave kernels of the SE(2) cell solver (se2_wave_kernel.hpp): the instantiations of se2_wave_kernel_kt,
// which commit an accepted trial from the poses its sweep parked in accumulator registers.  Policy tokens "kwM".
#include "se2_wave_kernel.hpp"

namespace ipc {
IPC_CELL_LAUNCHER(launch_se2_wave_kt, Se2View)
{
#define IPC_WCASE(MM)                                                                              \
    case MM:                                                                                       \
        return nl == 1 ? launch_wave_one<MM, 1, true>(n, st, P, cells, prm, out, counter, n_cu)    \
                       : launch_wave_one<MM, 2, true>(n, st, P, cells, prm, out, counter, n_cu);
    switch (M) {
#ifdef IPC_WAVE_KT_ONLY_M                              // (tools/isa_loop_mix.py: one instantiation, seconds to compile)
        IPC_WCASE(IPC_WAVE_KT_ONLY_M)
#else
        IPC_SE2_WAVE_KT_M(IPC_WCASE)
#endif
        default: return hipErrorInvalidValue;
    }
#undef IPC_WCASE
}

}  // namespace ipc
