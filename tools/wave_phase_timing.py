"""Phase split of the SE2 wave / pair / quad kernels (debug build with -DIPC_PHASE_TIMING:
  python -c "import __graft_entry__ as g; g._build_lib('ipc_amd/libipc_dbg_timing.so', ['-DIPC_PHASE_TIMING'], 'build/dbg')"
then   python tools/wave_phase_timing.py C2   on the GPU box; IPC_TIMING_LIB names another such library).  Ticks are
s_memtime counts of lane 0 / wave 0 of every cell, summed per kernel variant.  s_memtime counts SHADER-CLOCK cycles on
gfx950 (it is s_memrealtime that runs at the constant 100 MHz): the last line divides the summed ticks by the cells that
run abreast (4 per CU for the wave kernels, 2 for the pair, 1 for the quad kernels) and by the solver time of the run --
the quotient is the clock the ticks would need.  On C2 it comes to 2.31 - 2.32 GHz (profiles/capsolve_phase_*.txt), the
MI355X's shader clock; 100 MHz ticks would have to give 0.1 GHz."""
import sys, os, ctypes as C
sys.path.insert(0, os.getcwd())
import numpy as np
from ipc_amd import capi
capi.LIB_PATH = os.environ.get("IPC_TIMING_LIB") or os.path.join(os.getcwd(), "ipc_amd", "libipc_dbg_timing.so")
from bench import build_workload
from ipc_amd.consensus import IPC
g, cfg, desc = build_workload(sys.argv[1] if len(sys.argv) > 1 else "C2")
eng = IPC(g, cfg, device=0)
eng.run()
solver_ms, _ = eng.solver_time_ms()
out = np.zeros(4096, dtype=np.uint64)
eng.lib.ipc_dbg_read(eng.h, out.ctypes.data_as(C.c_void_p), 4096)
print("variant   cells   iters   %A   %B1(partials)  %B2(solve)  %C   %trials  %commit  wait%(of all)   ticks/iter  ticks/(iter*pose)*1e3  rejected-trials/iter  GN-trials/iter  GN-rejected/iter  big-sweeps/eval  ticks/big-sweep  ticks/small-sweep  B2-ticks/iter")
abreast_ticks = 0.0
for W in (1, 2, 4):
    for M in range(1, 16):
        d = out[64 + 16 * (M + 16 * (W - 1)):][:16].astype(np.float64)
        if d[9] == 0:
            continue
        tot = d[0] + d[1] + d[2] + d[3] + d[4] + d[10]
        abreast_ticks += tot * W / 4.0
        print("%s%-3d %8d %9d  %5.1f %5.1f %5.1f %5.1f %5.1f %5.1f   %5.1f   %8.1f  %8.2f  %6.3f  %6.3f  %6.3f  %6.3f  %8.0f %8.0f  %8.1f" % (
            {1: "w", 2: "p", 4: "q"}[W], M, d[9], d[6], 100 * d[0] / tot, 100 * d[1] / tot, 100 * d[2] / tot,
            100 * d[3] / tot, 100 * d[4] / tot, 100 * d[10] / tot, 100 * d[5] / tot, tot / d[6], 1e3 * tot / d[8], d[11] / d[6], d[12] / d[6], d[13] / d[6], d[14] / max(d[7] - d[9], 1), d[15] / max(d[14], 1), float(out[64 + 16 * (M + 16 * (W - 1)) + 1024]) / max(d[7] - d[9] - d[14], 1),
            d[2] / d[6]))
n_cu = 256
print("solver time %.2f ms; summed ticks / (cells abreast on %d CUs) = %.4g; as a clock: %.3f GHz" % (
    solver_ms, n_cu, abreast_ticks / n_cu, abreast_ticks / n_cu / (solver_ms * 1e-3) / 1e9))
