"""The one-loop walk of a lane over its nine row ranges (dynfu_amd/csrc/knn_walk.hpp: the plan, its trip count and the step
that knn_grid_query runs) driven by a stand-alone C++ program on the CPU, tests/cpp/test_knn_walk.cpp; then the same program
built with -fsanitize=address,undefined and run (a stand-alone program: the sanitizer's runtime is linked into it).  And
tools/knn_walk_count.py, the count the change rests on: at the smallest configuration one loop per lane takes fewer wave
steps than nine wave-wide loops, and joined ranges fewer still."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_knn_walk.cpp")


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0 and "5 tests, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_knn_walk_visits_every_candidate_once_within_its_trip_count(tmp_path):
    exe = str(tmp_path / "test_knn_walk")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    _run(exe)


def test_knn_walk_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "test_knn_walk_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = _run(exe, env=dict(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_walk_count_tool_orders_the_three_forms():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import knn_walk_count as T
    finally:
        sys.path.pop(0)
    row = T.count("C1")
    assert row["nodes"] == 512 and row["k"] == 8
    assert row["joined"] <= row["one_loop"] <= row["nine_loops"]
    assert row["one_loop"] < 0.8 * row["nine_loops"]  # the premise of the one-loop walk: a clear gap, not a tie
    assert 4 * row["one_loop"] >= row["candidates_mean"]  # (the longest lane of a wave covers at least the mean lane)
