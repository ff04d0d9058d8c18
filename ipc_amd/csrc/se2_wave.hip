// Wave kernels of the SE(2) cell solver (se2_wave_kernel.hpp): the instantiations of se2_wave_kernel, whose accepted
// trials are re-swept to commit.  (The kept-trial kernels are in se2_wave_kt.hip.)
#include "se2_wave_kernel.hpp"

namespace ipc {
IPC_CELL_LAUNCHER(launch_se2_wave, Se2View)
{
#define IPC_WCASE(MM)                                                                              \
    case MM:                                                                                       \
        return nl == 1 ? launch_wave_one<MM, 1, false>(n, st, P, cells, prm, out, counter, n_cu)   \
                       : launch_wave_one<MM, 2, false>(n, st, P, cells, prm, out, counter, n_cu);
    switch (M) {
#ifdef IPC_WAVE_ONLY_M
        IPC_WCASE(IPC_WAVE_ONLY_M)
#else
        IPC_SE2_WAVE_M(IPC_WCASE)
#endif
        default: return hipErrorInvalidValue;
    }
#undef IPC_WCASE
}

}  // namespace ipc
