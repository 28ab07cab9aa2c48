"""CPU statement of the point-cloud extraction (TsdfVolume::fetchCloud / fetchNormals) in numpy float32.

What it states is the reference's src/kfusion/cuda/tsdf_volume.cu — FullScan6 (:423-598) for the cloud, ExtractNormals
(:602-680) for the normals — with the output contract of include/dynfu_amd.h (dfa_tsdf_extract_cloud): points in
ascending linear voxel order, within a voxel +x, +y, +z.  Every operation is a float32 operation in the reference's
order; fused multiply-adds happen exactly where the kernels have them (device_math.hpp: dot(), the raycaster's
trilinear interpolate), computed here by fma32 with a single rounding.  The parity tests compare the kernels' bits
against this module; tests/test_tsdf_extract_cpu.py checks the module itself on hand-made volumes.
"""
import numpy as np

f32 = np.float32


def unpack(packed):
    """packed uint32 voxels -> (tsdf float32, weight uint32): low half fp16 distance, high half weight"""
    packed = np.asarray(packed, np.uint32)
    F = (packed & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)
    return F, packed >> 16


def pack(F, W):
    """float distances (rounded to fp16) and weights -> packed uint32 voxels"""
    h = np.asarray(F, np.float32).astype(np.float16).view(np.uint16).astype(np.uint32)
    return h | (np.asarray(W, np.uint32) << 16)


def fma32(a, b, c):
    """float32 a * b + c rounded once.  The product of two floats is exact in float64; the sum is made exact by TwoSum
    and rounded to odd in float64 (53 >= 2 * 24 + 2 bits), so that the final rounding to float32 is the only one."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c)))
    p = a * b
    s = p + c
    with np.errstate(invalid="ignore", over="ignore"):
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _dot(r, v):
    """kfusion dot(): x*x' + y*y' + z*z' with the two trailing products fused (device_math.hpp)"""
    return fma32(r[2], v[2], fma32(r[1], v[1], f32(r[0]) * v[0]).astype(np.float32))


def _mat(R, v):
    """R (3x3 float32) times v (3 arrays)"""
    return [_dot(R[i], v) for i in range(3)]


def _aff(vol2world):
    m = np.asarray(vol2world, np.float32).reshape(-1)
    return m[:9].reshape(3, 3), m[9:12]


def extract_cloud(vol, voxel_size, vol2world, z0=0, z1=None):
    """The points whose SOURCE voxel lies in slices [z0, z1) of `vol` (uint32 (Z, Y, X)), as (n, 4) float32 {x, y, z, 0}
    in the output order.  Slabs taken in ascending z concatenate to the whole cloud."""
    vol = np.asarray(vol, np.uint32)
    Z, Y, X = vol.shape
    z1 = Z - 1 if z1 is None else min(z1, Z - 1)  # sources: z < Z - 1 (:459)
    if z1 <= z0:
        return np.zeros((0, 4), np.float32)
    vs = np.asarray(voxel_size, np.float32)
    c = vol[z0:z1]
    F, W = unpack(c)
    nb = [np.zeros_like(c), np.zeros_like(c), vol[z0 + 1:z1 + 1]]  # +x, +y, +z neighbours; a missing one has weight 0
    nb[0][:, :, :-1] = c[:, :, 1:]
    nb[1][:, :-1, :] = c[:, 1:, :]
    src = (W != 0) & (F != f32(1))  # :462-463
    masks, Fns = [], []
    for n in nb:
        Fn, Wn = unpack(n)
        masks.append(src & (Wn != 0) & (Fn != f32(1)) & (((F > 0) & (Fn < 0)) | ((F < 0) & (Fn > 0))))  # :468-469
        Fns.append(Fn)
    zz, yy, xx, dd = np.nonzero(np.stack(masks, -1))  # C order = (z, y, x, d): the output order
    Fs = F[zz, yy, xx]
    Fn = np.choose(dd, [Fns[0][zz, yy, xx], Fns[1][zz, yy, xx], Fns[2][zz, yy, xx]])
    idx = [xx, yy, zz + z0]
    V = [(idx[k].astype(np.float32) + f32(0.5)) * vs[k] for k in range(3)]  # :453-454, :465
    aF, aFn = np.abs(Fs), np.abs(Fn)
    d_inv = f32(1) / (aF + aFn)
    p = []
    for k in range(3):
        Vn = V[k] + vs[k]
        along = (V[k] * aFn + Vn * aF) * d_inv  # :479-481, :499-501, :519-521
        p.append(np.where(dd == k, along, V[k]).astype(np.float32))
    R, t = _aff(vol2world)
    q = _mat(R, p)  # aff * p = R p + t (device.hpp)
    out = np.zeros((len(zz), 4), np.float32)
    for k in range(3):
        out[:, k] = q[k] + t[k]
    return out


def _interpolate(vol, cf):
    """the raycaster's trilinear interpolate (tsdf_volume.cu:146-171 as csrc/tsdf.hip has it): cf = 3 arrays of voxel
    coordinates; NaN outside [0, dim - 1) on any axis"""
    Z, Y, X = vol.shape
    dims = (X, Y, Z)
    inside = np.ones(cf[0].shape, bool)
    for k in range(3):
        inside &= (cf[k] >= 0) & (cf[k] < f32(dims[k] - 1))
    c = [np.where(inside, cf[k], f32(0)).astype(np.float32) for k in range(3)]
    g = [c[k].astype(np.int64) for k in range(3)]
    a, b, cc = (c[k] - g[k].astype(np.float32) for k in range(3))
    one = f32(1)

    def v(dx, dy, dz):
        return unpack(vol[g[2] + dz, g[1] + dy, g[0] + dx])[0]

    t = np.zeros(a.shape, np.float32)
    t = fma32((v(0, 0, 0) * (one - a)) * (one - b), one - cc, t)
    t = fma32((v(0, 0, 1) * (one - a)) * (one - b), cc, t)
    t = fma32((v(0, 1, 0) * (one - a)) * b, one - cc, t)
    t = fma32((v(0, 1, 1) * (one - a)) * b, cc, t)
    t = fma32((v(1, 0, 0) * a) * (one - b), one - cc, t)
    t = fma32((v(1, 0, 1) * a) * (one - b), cc, t)
    t = fma32((v(1, 1, 0) * a) * b, one - cc, t)
    t = fma32((v(1, 1, 1) * a) * b, cc, t)
    return np.where(inside, t, f32(np.nan)).astype(np.float32)


def extract_normals(vol, voxel_size, vol2world, Rinv, delta_factor, points):
    """ExtractNormals (:602-680) of (n, 4) float32 points -> (n, 4) float32 {nx, ny, nz, 0}"""
    vol = np.asarray(vol, np.uint32)
    Z, Y, X = vol.shape
    pts = np.asarray(points, np.float32).reshape(-1, 4)
    vs = np.asarray(voxel_size, np.float32)
    vi = f32(1) / vs                      # :609-611 (the constructor)
    gd = vs * f32(delta_factor)           # :706
    R, t = _aff(vol2world)
    Ri = np.asarray(Rinv, np.float32).reshape(3, 3)
    q = _mat(Ri, [pts[:, k] - t[k] for k in range(3)])  # :617
    ok = np.ones(len(pts), bool)
    for k, dim in enumerate((X, Y, Z)):
        g = np.rint(q[k] * vi[k])  # __float2int_rn: round half to even (:609-613)
        ok &= (g > 1) & (g < dim - 2)  # :619-620
    n = []
    for k in range(3):  # :622-660: the two samples at +- the delta along axis k, each in voxel units
        hi = [q[j] + gd[k] if j == k else q[j] for j in range(3)]
        lo = [q[j] - gd[k] if j == k else q[j] for j in range(3)]
        Fp = _interpolate(vol, [(hi[j] * vi[j]).astype(np.float32) for j in range(3)])
        Fm = _interpolate(vol, [(lo[j] * vi[j]).astype(np.float32) for j in range(3)])
        n.append((Fp - Fm) / gd[k])  # __fdividef -> the correctly rounded divide
    rn = _mat(R, n)  # :662 normalized(aff.R * n)
    inv = f32(1) / np.sqrt(_dot([rn[0], rn[1], rn[2]], rn)).astype(np.float32)
    out = np.zeros((len(pts), 4), np.float32)
    with np.errstate(invalid="ignore"):
        for k in range(3):
            out[:, k] = np.where(ok, rn[k] * inv, f32(np.nan))
    return out
