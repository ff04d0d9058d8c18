// LDS-pose SE(3) cell kernels (se3_lds_kernel.hpp): one translation unit per group of (W, M) variants
#include "se3_lds_kernel.hpp"

IPC_SE3_LDS_UNIT(1, 1)
IPC_SE3_LDS_UNIT(1, 2)
IPC_SE3_LDS_UNIT(4, 10)

// the family's launcher, over the instantiations of all five units
namespace ipc {
IPC_CELL_LAUNCHER(launch_se3_lds, Se3View)
{
#define IPC_LCASE(WW, MM) case cell_wm(WW, MM): return launch_se3_lds_##WW##_##MM(nl, n, st, P, cells, prm, out, counter, n_cu);
    switch (cell_wm(W, M)) {
        IPC_SE3_LDS_WM(IPC_LCASE)
        default: return hipErrorInvalidValue;
    }
#undef IPC_LCASE
}
}  // namespace ipc
