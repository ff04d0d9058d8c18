"""The owning handles of ipc_amd/csrc/hip_owned.hpp, on the host alone: tests/host/hip_owned_main.cpp is a program of its own,
built with AddressSanitizer and UBSan and run as a child process (nothing loaded into Python is sanitised).  It exercises
the handle template over malloc'd memory with a counting release function -- release exactly once, early returns, moves,
release(), self-move, alloc() over a held value, vectors that reallocate -- and DevBuf::alloc where no device answers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handles_release_exactly_once_under_sanitizers(tmp_path):
    exe = str(tmp_path / "hip_owned_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "host", "hip_owned_main.cpp"), "-o", exe,
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    no_device = [] if os.path.exists("/dev/kfd") else ["--no-device"]
    r = subprocess.run([exe] + no_device, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hip_owned OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
