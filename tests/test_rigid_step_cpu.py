"""The pose update and the loop rules of the device-resident rigid pre-alignment (dynfu_amd/csrc/rigid_step.hpp) driven by a
stand-alone C++ program on the CPU, tests/cpp/test_rigid_step.cpp: the known answers of kfusion::cuda::icp_update
(tests/golden/icp_update_kat.json) at test_host_icp.cpp's bar, the refused cases included; then the same program built
with -fsanitize=address,undefined and run (a stand-alone program: the sanitizer's runtime is linked into it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "icp_update_kat.json")
SRC = os.path.join(ROOT, "tests", "cpp", "test_rigid_step.cpp")


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, DFA_ICP_UPDATE_KAT=KAT, **(env or {})))
    assert r.returncode == 0 and "5 tests, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_rigid_step_known_answers_and_loop_rules(tmp_path):
    exe = str(tmp_path / "test_rigid_step")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    _run(exe)


def test_rigid_step_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "test_rigid_step_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = _run(exe, env=dict(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
