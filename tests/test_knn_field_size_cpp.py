"""The size arithmetic of the k-NN field (dynfu_amd/csrc/warped_bricks.hpp: bricks, record bytes, the byte count in size_t,
the max_bytes compare) driven by a stand-alone C++ program on the CPU, tests/cpp/test_knn_field_size.cpp."""
import subprocess


def test_knn_field_size_arithmetic():
    from dynfu_amd import build as B
    import oracle
    oracle.build()  # (build_cpp_tests links the oracle into some of its other programs)
    exe = B.build_cpp_tests()["test_knn_field_size"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "4 tests, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
