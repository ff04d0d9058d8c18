// The cell plan of ipc_amd/csrc/cell_plan.hpp on the host alone: every family's launcher is a stub that records its call.
// For a list of settings of IPC_SE2_POLICY / IPC_SE2_LAZY_SD and IPC_SE3_POLICY / IPC_SE3_LATENCY_POLICY the program prints
// the plan (one line per bin) and, at 256 CUs, the kernel chosen for each bin with one cell and with a cell count on either
// side of the bin's latency threshold -- through the chosen descriptor's launcher, so that the line shows the function that
// ran and the (W, M) it was given.  tests/test_cell_plan_cpu.py holds the output against tests/golden/cell_plans.txt.
// Needs the ROCm headers for the types of the launchers' signature only; nothing of the runtime is linked.
#include "../../ipc_amd/csrc/cell_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>

namespace ipc {
struct Se2View {};
struct Se3View {};
struct SolveParams {};

static struct { const char* fn; int nl, W, M; } g_call;
#define IPC_STUB(name, View) IPC_CELL_LAUNCHER(name, View) { g_call = {#name, nl, W, M}; return hipSuccess; }
IPC_STUB(launch_se2_block, Se2View) IPC_STUB(launch_se2_wave, Se2View) IPC_STUB(launch_se2_pair, Se2View)
IPC_STUB(launch_se2_quad, Se2View) IPC_STUB(launch_se2_wave_kt, Se2View) IPC_STUB(launch_se2_pair_kt, Se2View)
IPC_STUB(launch_se2_wave_lz, Se2View) IPC_STUB(launch_se2_pair_lz, Se2View)
IPC_STUB(launch_se3_block, Se3View) IPC_STUB(launch_se3_lds, Se3View)
}  // namespace ipc

using namespace ipc;

constexpr int kCu = 256;

static void set(const char* name, const char* value)
{
    if (value) setenv(name, value, 1);
    else unsetenv(name);
}

// aux: IPC_SE2_LAZY_SD (dim 2) / IPC_SE3_LATENCY_POLICY (dim 3); null: unset
static void show(int dim, const char* policy, const char* aux)
{
    set(dim == 2 ? "IPC_SE2_POLICY" : "IPC_SE3_POLICY", policy);
    set(dim == 2 ? "IPC_SE2_LAZY_SD" : "IPC_SE3_LATENCY_POLICY", aux);
    printf("== SE%d policy %s %s %s\n", dim, policy ? policy : "(unset)", dim == 2 ? "lazy_sd" : "latency", aux ? aux : "(unset)");
    BinPlan bp{};
    std::string err;
    if (!make_plan(bp, dim, err)) { printf("error: %s\n", err.c_str()); return; }
    for (int b = 0; b < bp.caps.n; ++b)
        printf("bin %d cap %d %s served by %s latency %s below %d\n", b, bp.caps.cap[b], bp.kernel[b]->token,
               (bp.lazy[b] ? bp.lazy[b] : bp.kernel[b])->token, bp.latency[b] ? bp.latency[b]->token : "-", bp.latency_below[b]);
    long long lazy = 0;
    for (int b = 0; b < bp.caps.n; ++b)
        for (int nl = 1; nl <= 2; ++nl)
            for (int n : {1, bp.latency_below[b] * kCu - 1, bp.latency_below[b] * kCu}) {
                if (n != 1 && !bp.latency_below[b]) continue;                              // (no threshold: one cell only)
                const CellKernel& k = choose_kernel(bp, b, n, kCu);
                if (is_lazy_sd(k)) ++lazy;
                if (dim == 2) (void)k.se2(nl, k.W, k.M, n, nullptr, Se2View{}, nullptr, SolveParams{}, CellOut{}, nullptr, kCu);
                else (void)k.se3(nl, k.W, k.M, n, nullptr, Se3View{}, nullptr, SolveParams{}, CellOut{}, nullptr, kCu);
                printf("  bin %d nl %d n %d -> %s by %s(nl %d, W %d, M %d)\n", b, nl, n, k.token, g_call.fn, g_call.nl, g_call.W, g_call.M);
            }
    printf("lazy launches %lld\n", lazy);
}

int main()
{
    for (const char* v : {"IPC_SE2_POLICY", "IPC_SE2_LAZY_SD", "IPC_SE3_POLICY", "IPC_SE3_LATENCY_POLICY"}) unsetenv(v);
    // ---- SE2 ----
    show(2, nullptr, nullptr);
    for (const char* lz : {"0", "1", "2", "3"}) show(2, nullptr, lz);
    for (const CellKernel& k : kSe2Kernels)                       // every compiled token alone
        if (!is_lazy_sd(k)) { show(2, k.token, nullptr); show(2, k.token, "2"); }
    for (const char* pol : {"kw7,w7", "w7,kw7", "14x1,kp7,p7", "w7,w7"}) show(2, pol, nullptr);      // equal capacities
    std::string many = "w1";
    for (int k = 1; k < 33; ++k) many += ",w1";
    show(2, many.c_str(), nullptr);
    for (const char* pol : {"w2", "kw13", "kp5", "3x3", "w", "x", "7"}) show(2, pol, nullptr);       // not compiled / no token
    // ---- SE3 ----
    show(3, nullptr, nullptr);
    show(3, "block", nullptr);
    for (const CellKernel& k : kSe3Kernels) show(3, k.token, nullptr);
    for (const char* lat : {"none", "8x1,4x2", "8x", "3x3"}) show(3, "block", lat);                  // off / equal capacities / no token / not compiled
    return 0;
}
