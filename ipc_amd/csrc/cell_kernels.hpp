// The cell-solver kernels that exist, and their launch interface.  The kernels are heavily templated, so they live
// in their own translation units (se2_block.hip, se2_wave.hip, se2_wave_kt.hip, se2_wave_lz.hip, se2_pair.hip, se2_pair_kt.hip, se2_pair_lz.hip, se2_quad.hip, se3_block.hip, se3_lds_a..e.hip) that are compiled
// in parallel and linked into libipc_amd.so; engine.hip only sees these prototypes.
//
// Each family's instantiations are written down ONCE, as a list macro IPC_..._WM(X) / IPC_..._M(X) that applies X to
// every (W, M) or M.  The family's launch switch (its .hip unit) and the descriptor tables that policy parsing, plan and
// launch read (cell_plan.hpp) are expansions of these lists: a kernel is added by adding it to its list.
// Host-clean: the view and parameter types are names only here, so that cell_plan.hpp compiles in a plain host program.
#pragma once
#include <hip/hip_runtime.h>

namespace ipc {

struct Se2View;                                        // se2_cell.hpp
struct Se3View;                                        // se3_cell.hpp
struct SolveParams;                                    // se2_cell.hpp
struct CellOut {
    double* max_chi2;
    double* chi2_total;
    int4* meta;               // iterations, tries, flags, error evaluations
};

// One signature for the launcher of every family: the kernel <W, M> of the family on the n cells of a slot.
// counter: one zeroed unsigned in HBM (work queue of the launch); n_cu: workgroups to launch (the block kernels, one
// workgroup per cell, ignore both).  hipErrorInvalidValue for a (W, M) that is not in the family's list.
#define IPC_CELL_LAUNCHER(name, View)                                                                                   \
    hipError_t name(int nl, int W, int M, int n, hipStream_t st, const View& P, const int2* cells, SolveParams prm,     \
                    CellOut out, unsigned* counter, int n_cu)
// The (W, M) of a launch as one switch value
constexpr int cell_wm(int W, int M) { return W * 256 + M; }

// ---- block kernels: one workgroup of W waves per cell, M poses per lane; capacity 64*W*M.  Policy tokens "WxM" ----
#define IPC_SE2_BLOCK_WM(X)                                                                                      \
    /* M = 1 */                                                                                                  \
    X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(5, 1) X(6, 1) X(7, 1) X(8, 1) X(10, 1) X(12, 1) X(14, 1) X(16, 1)          \
    /* M = 2 */                                                                                                  \
    X(4, 2) X(5, 2) X(6, 2) X(7, 2) X(8, 2) X(10, 2) X(12, 2) X(16, 2)                                           \
    /* M = 3 */                                                                                                  \
    X(5, 3) X(6, 3) X(7, 3) X(8, 3)                                                                              \
    /* M = 4 and longer chains */                                                                                \
    X(4, 4) X(6, 4) X(8, 4) X(16, 4) X(16, 8) X(16, 16)                                                          \
    /* two waves per cell, two cells per CU */                                                                   \
    X(2, 3) X(2, 4) X(2, 5) X(2, 6)                                                                              \
    /* three / four fat waves per cell */                                                                        \
    X(3, 4) X(3, 5) X(3, 6) X(4, 3) X(4, 5)
#define IPC_SE3_BLOCK_WM(X)                                                                                      \
    X(1, 1) X(2, 1) X(4, 1) X(8, 1) X(16, 1) X(16, 2) X(16, 4) X(4, 2) X(4, 4) X(8, 2) X(8, 4) X(4, 8) X(8, 5)   \
    X(1, 2) X(2, 2) X(1, 4) X(2, 4) X(1, 3) X(2, 3)
IPC_CELL_LAUNCHER(launch_se2_block, Se2View);
IPC_CELL_LAUNCHER(launch_se3_block, Se3View);

// ---- LDS-pose kernels (SE3, se3_lds_cell.hpp): teams of W = 1 or 4 waves per cell, M poses per lane;
// capacity 64*W*M.  Policy tokens "wM" (W = 1) and "gM" (W = 4).  One function per instantiation, so that the units
// se3_lds_a..e.hip can share the compile time between them; launch_se3_lds (se3_lds_a.hip) selects among them ----
#define IPC_SE3_LDS_WM(X)                                                                                        \
    X(1, 1) X(1, 2) X(1, 3) X(1, 4) X(1, 6) X(1, 8)                                                              \
    X(4, 2) X(4, 3) X(4, 4) X(4, 5) X(4, 6) X(4, 7) X(4, 8) X(4, 9) X(4, 10)
#define IPC_SE3_LDS_DECL(WW, MM)                                                                                \
    hipError_t launch_se3_lds_##WW##_##MM(int nl, int n, hipStream_t st, const Se3View& P, const int2* cells,   \
                                          SolveParams prm, CellOut out, unsigned* counter, int n_cu);
IPC_SE3_LDS_WM(IPC_SE3_LDS_DECL)
#undef IPC_SE3_LDS_DECL
IPC_CELL_LAUNCHER(launch_se3_lds, Se3View);

// ---- wave kernels (SE2): one wave per cell, M consecutive poses per lane; capacity 64*M.  Policy tokens "wM".
// The chain window [0, V-1) is staged in LDS when it fits, else the constants are read from L2 ----
#define IPC_SE2_WAVE_M(X) X(1) X(3) X(5) X(7) X(9) X(11) X(13)
IPC_CELL_LAUNCHER(launch_se2_wave, Se2View);

// ---- pair kernels (SE2): two waves per cell, M consecutive poses per lane; capacity 128*M.  Policy tokens "pM" ----
#define IPC_SE2_PAIR_M(X) X(5) X(7) X(9) X(11)
IPC_CELL_LAUNCHER(launch_se2_pair, Se2View);

// ---- quad kernels (SE2): the four waves of a workgroup on one cell; capacity 256*M.  Policy tokens "qM" ----
#define IPC_SE2_QUAD_M(X) X(7) X(9) X(11) X(13)
IPC_CELL_LAUNCHER(launch_se2_quad, Se2View);

// ---- kept-trial wave and pair kernels (SE2, se2_wave_kt.hip / se2_pair_kt.hip): the same cells, capacities and
// results as the wave / pair kernel of the same M; an accepted trial is committed from the poses its sweep parked in
// accumulator registers instead of by a second sweep (KEEP_TRIAL of se2_wave_solve).  Policy tokens "kwM" / "kpM" ----
#define IPC_SE2_WAVE_KT_M(X) X(5) X(7) X(9) X(11)
IPC_CELL_LAUNCHER(launch_se2_wave_kt, Se2View);
#define IPC_SE2_PAIR_KT_M(X) X(7) X(9) X(11)
IPC_CELL_LAUNCHER(launch_se2_pair_kt, Se2View);

// ---- lazy steepest-descent wave and pair kernels (SE2, se2_wave_lz.hip / se2_pair_lz.hip; LAZY_SD of se2_wave_solve):
// the same cells, capacities and results, bit for bit, as the kernel the default policy names for that M (kept trial up to
// M = kLazyKeepTrialMaxM, re-sweep beyond); b^T H b, alpha and |h_sd| are formed only in the iterations whose trial
// loop reads them.  No policy token: the plan serves a bin of that kernel with this one (IPC_SE2_LAZY_SD, cell_plan.hpp) ----
constexpr int kLazyKeepTrialMaxM = 9;
#define IPC_SE2_WAVE_LZ_M(X) X(5) X(7) X(9) X(11) X(13)
IPC_CELL_LAUNCHER(launch_se2_wave_lz, Se2View);
#define IPC_SE2_PAIR_LZ_M(X) X(7) X(9) X(11)
IPC_CELL_LAUNCHER(launch_se2_pair_lz, Se2View);

}  // namespace ipc
