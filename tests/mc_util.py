"""shared by the marching-cubes tests: analytic packed TSDF volumes (numpy) and the case tables"""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def default_tables():
    """dfa_mc_default_tables is host code: callable without a GPU (and without torch)"""
    lib = ctypes.CDLL(os.path.join(ROOT, "dynfu_amd", "libdynfu_amd.so"))
    tri, nv = np.zeros((256, 16), np.int32), np.zeros(256, np.int32)
    assert lib.dfa_mc_default_tables(tri.ctypes.data_as(ctypes.c_void_p), nv.ctypes.data_as(ctypes.c_void_p)) == 0
    return tri, nv


def pack(tsdf, weight):
    """float tsdf in [-1, 1] -> half bits (numpy's conversion is round-to-nearest-even) | weight << 16"""
    h = np.asarray(tsdf, np.float32).astype(np.float16).view(np.uint16).astype(np.uint32)
    return h | (np.asarray(weight, np.uint32) << 16)


def blob_volume(dims, seed=0, holes=True, trunc=0.1):
    """(Z, Y, X) uint32 volume: truncated signed distance of two overlapping spheres, weight 0
    outside the truncation band and in random holes (exercises the "any weight == 0" rule)"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid((np.arange(Z) + 0.5) / Z, (np.arange(Y) + 0.5) / Y, (np.arange(X) + 0.5) / X, indexing="ij")
    d1 = np.sqrt((x - 0.4) ** 2 + (y - 0.45) ** 2 + (z - 0.5) ** 2) - 0.27
    d2 = np.sqrt((x - 0.65) ** 2 + (y - 0.6) ** 2 + (z - 0.45) ** 2) - 0.2
    d = np.minimum(d1, d2)
    tsdf = np.clip(d / trunc, -1, 1)
    w = (np.abs(d) < trunc).astype(np.uint32) * rng.integers(1, 65, d.shape).astype(np.uint32)
    if holes:
        w[rng.random(d.shape) < 0.02] = 0
        tsdf = np.where(rng.random(d.shape) < 0.01, 0.0, tsdf)  # exact zeros: f < iso is false
        tsdf = np.where(rng.random(d.shape) < 0.005, -0.0, tsdf)
    return pack(tsdf, w)


def sign_noise_volume(dims, seed=0):
    """(Z, Y, X) uint32 volume: uniform random magnitudes in [0.05, 1], random signs, every weight non-zero.  Every cube
    has a random case: all 254 non-trivial cases, dense segments and the ambiguous configurations a smooth surface never
    produces (tests/test_mc_statement_cpu.py asserts what the kernels' sizing needs of it)."""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.05, 1.0, (Z, Y, X))
    sign = np.where(rng.integers(0, 2, (Z, Y, X)) == 1, -1.0, 1.0)
    w = rng.integers(1, 65, (Z, Y, X)).astype(np.uint32)
    return pack(mag * sign, w)


def checkerboard_volume(dims):
    """(Z, Y, X) uint32 volume whose sign is (x + y + z) % 2: every cube is case 0x5A or 0xA5, 12 vertices each — the
    densest uniform load (3 072 vertices per full 256-cube segment).  Magnitudes vary so that no two edges share a t."""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    mag = 0.125 + ((7 * x + 13 * y + 29 * z) % 32) / 40.0
    sign = np.where((x + y + z) % 2 == 1, -1.0, 1.0)
    return pack(mag * sign, np.full((Z, Y, X), 3, np.uint32))


# fp16 bit patterns a TSDF sweep never writes but the packed format can hold
SPECIAL_HALVES = np.array([0x0001, 0x8001, 0x0200, 0x8200, 0x03FF, 0x83FF,  # denormals of both signs
                           0x0000, 0x8000,                                  # +-0
                           0x7BFF, 0xFBFF,                                  # +-65504
                           0x7C00, 0xFC00,                                  # +-inf
                           0x7E00, 0xFE00, 0x7C01], np.uint32)               # NaN (quiet of both signs, signalling)


def special_values_volume(dims, seed=0, fraction=0.08):
    """a blob volume with the distances of random voxels near the surface (those with a weight) replaced by
    SPECIAL_HALVES; weights untouched"""
    vol = blob_volume(dims, seed=seed)
    rng = np.random.default_rng(seed + 1)
    pick = ((vol >> 16) != 0) & (rng.random(vol.shape) < fraction)
    vals = SPECIAL_HALVES[rng.integers(0, len(SPECIAL_HALVES), vol.shape)]
    return np.where(pick, (vol & np.uint32(0xFFFF0000)) | vals, vol).astype(np.uint32)
