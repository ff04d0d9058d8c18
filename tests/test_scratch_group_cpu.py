"""ScratchCap of ipc_amd/csrc/hip_owned.hpp, the scratch group that owns its capacity, on the host alone:
tests/host/scratch_group_main.cpp is a program of its own over a fake buffer type that counts its live allocations and can
fail its k-th alloc().  Built with plain g++ against the ROCm headers, nothing of the runtime linked, and run as a child
process: no growth within the capacity, release of every member before the first allocation, the capacity at 0 after a failure
at any member with a clean growth behind it, and views cut at the capacity."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_group_grows_together_and_survives_a_failed_member(tmp_path):
    exe = str(tmp_path / "scratch_group_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "host", "scratch_group_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scratch_group OK" in r.stdout
