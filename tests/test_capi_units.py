"""CPU checks of the C ABI layer as a set of translation units (csrc/capi*.cpp): one entry point of each unit fails its
argument check — before any HIP call, so without a GPU — and dfa_last_error(), which lives in capi.cpp, has the text.  A
unit that wrote an error buffer of its own would return its code and leave the text empty.  The texts are the library's
from before the layer was cut; they are part of what a caller sees."""
import ctypes
import threading

import pytest

vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
DFA_ERR_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (torch's bundled HIP runtime must be the one the library binds to)
    from dynfu_amd import build as B
    L = ctypes.CDLL(B.build())
    L.dfa_last_error.restype = ctypes.c_char_p
    L.dfa_abi_struct_size.restype = ctypes.c_size_t
    L.dfa_abi_struct_size.argtypes = [i]
    L.dfa_tsdf_clear.argtypes = [vp, i, i, i, vp]
    L.dfa_depth_truncate.argtypes = [vp, i, i, i, f, vp]
    L.dfa_knn.argtypes = [vp, vp, i, vp, i, i, vp, vp, vp]
    L.dfa_solver_create.argtypes = [i, i, i, vp]
    L.dfa_solver6_create.argtypes = [i, i, i, vp]
    L.dfa_mc_default_tables.argtypes = [vp, vp]
    return L


HOST = (ctypes.c_float * 4)()  # a non-null pointer for arguments that are checked and never read


def _null_volume(L):
    return L.dfa_tsdf_clear(None, 8, 8, 8, None)


def _no_columns(L):
    return L.dfa_depth_truncate(ctypes.addressof(HOST), 64, 0, 4, 1.0, None)


def _k_zero(L):
    return L.dfa_knn(ctypes.addressof(HOST), None, 1, None, 0, 0, None, None, None)


#         unit                 the failing call                                         dfa_last_error()
CASES = {
    "capi_tsdf.cpp":    (_null_volume,                                      b"dfa_tsdf_clear: bad volume"),
    "capi_image.cpp":   (_no_columns,                                       b"dfa_depth_truncate: bad image"),
    "capi_warp.cpp":    (_k_zero,                                           b"dfa_knn: k out of range 1..16"),
    "capi_solver.cpp":  (lambda L: L.dfa_solver_create(8, 8, 4, None),      b"dfa_solver_create: null out"),
    "capi_solver6.cpp": (lambda L: L.dfa_solver6_create(8, 8, 4, None),     b"dfa_solver6_create: null out"),
    "capi_tsdf.cpp (marching cubes)": (lambda L: L.dfa_mc_default_tables(None, None), b"dfa_mc_default_tables: null table"),
}


@pytest.mark.parametrize("unit", list(CASES))
def test_argument_check_reaches_the_one_error_buffer(lib, unit):
    call, text = CASES[unit]
    other = CASES["capi_warp.cpp" if unit == "capi_tsdf.cpp" else "capi_tsdf.cpp"]
    assert other[0](lib) == DFA_ERR_INVALID and lib.dfa_last_error() == other[1]  # (another unit's text is there first)
    assert call(lib) == DFA_ERR_INVALID
    assert lib.dfa_last_error() == text


def test_unknown_struct_id_has_size_zero(lib):
    """capi.cpp itself: no struct of that id, and asking is not an error"""
    assert _null_volume(lib) == DFA_ERR_INVALID
    assert lib.dfa_abi_struct_size(12345) == 0
    assert lib.dfa_abi_struct_size(-1) == 0
    assert lib.dfa_last_error() == CASES["capi_tsdf.cpp"][1]


def test_every_struct_id_of_the_header_has_a_size(lib):
    """the DFA_STRUCT_* enum of include/dynfu_amd.h, read from the header: ids 0 .. n-1 without a gap, each with a non-zero
    size in the library, and the first id past the enum with none"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dynfu_amd.h")).read(), flags=re.S)
    ids = {name: int(val) for name, val in re.findall(r"\b(DFA_STRUCT_[A-Z0-9_]+)\s*=\s*(\d+)", src)}
    assert "DFA_STRUCT_KNN_FIELD_DESC" in ids and sorted(ids.values()) == list(range(len(ids))), ids
    for name, sid in ids.items():
        assert lib.dfa_abi_struct_size(sid) > 0, name
    assert lib.dfa_abi_struct_size(len(ids)) == 0, "the library knows a struct id the header does not declare"
    # the k-NN field's description: two ints, two 64-bit counts and the byte count (the mirror of dynfu_amd/_lib.py)
    assert lib.dfa_abi_struct_size(ids["DFA_STRUCT_KNN_FIELD_DESC"]) == 4 + 4 + 8 + 8 + 8


def test_error_buffer_is_per_thread(lib):
    """a failing call in a second thread leaves this thread's last message as it was"""
    assert _null_volume(lib) == DFA_ERR_INVALID
    seen = {}

    def second():
        seen["before"] = lib.dfa_last_error()
        seen["rc"] = _k_zero(lib)
        seen["after"] = lib.dfa_last_error()

    t = threading.Thread(target=second)
    t.start()
    t.join()
    assert seen == {"before": b"", "rc": DFA_ERR_INVALID, "after": CASES["capi_warp.cpp"][1]}
    assert lib.dfa_last_error() == CASES["capi_tsdf.cpp"][1]
