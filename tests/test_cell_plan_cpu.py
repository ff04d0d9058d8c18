"""The cell plan of ipc_amd/csrc/cell_plan.hpp on the host alone: policy parsing, the order of equal capacities, the lazy
and latency substitutions and the kernel chosen for a launch, for every compiled token and the settings listed in
tests/host/cell_plan_main.cpp.  That program -- the header over stub launchers that record their call -- is built with plain
g++ and the address / undefined-behaviour sanitizers against the ROCm headers, nothing of the runtime linked, and run as a
child process; its output is held byte for byte against tests/golden/cell_plans.txt.

The fixture was not written by the code under test: it is the output of the same settings through the plan code of the
commit before the descriptor tables (BinPlan ... make_plan and SlotLauncher of engine.hip as they stood, with numeric
variant ids, compiled in a host program over stubs of the old launchers, ids translated to tokens for printing)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICY_VARS = ("IPC_SE2_POLICY", "IPC_SE2_LAZY_SD", "IPC_SE3_POLICY", "IPC_SE3_LATENCY_POLICY")


def test_plans_and_launch_choices_are_the_recorded_ones(tmp_path):
    exe = str(tmp_path / "cell_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",      # (no runtime library to load: nothing depends on the load order)
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "host", "cell_plan_main.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if k not in POLICY_VARS}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    want = open(os.path.join(ROOT, "tests", "golden", "cell_plans.txt")).read()
    if r.stdout != want:
        got, exp = r.stdout.splitlines(), want.splitlines()
        k = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        head = next((line for line in reversed(exp[:k + 1]) if line.startswith("==")), "")
        raise AssertionError("line %d under %r:\n  got      %r\n  recorded %r\n(%d lines, %d recorded)" % (
            k + 1, head, got[k] if k < len(got) else None, exp[k] if k < len(exp) else None, len(got), len(exp)))
