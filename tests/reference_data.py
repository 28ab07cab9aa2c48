"""The reference's own answers on the tests' inputs, kept as data under tests/golden/ so that the tests need nothing outside
the repository: its marching-cubes case tables (ref_mc_tables.bin) and what its vendored nanoflann k-NN returns for the
seeded query sets below (ref_knn.npz).  Both are written by tests/golden/make_reference_outputs.py.

Every stored k-NN answer carries a digest of the inputs it was computed from: inputs that no longer come out of their
generator bit for bit fail loudly instead of being compared against another input's answer."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MC_TABLES = os.path.join(GOLDEN, "ref_mc_tables.bin")
KNN = os.path.join(GOLDEN, "ref_knn.npz")
_KNN = None


def mc_tables():
    """the reference's case tables (src/kfusion/marching_cubes.cpp triTable, numVertsTable): (tri (256, 16), nv (256,)) int32"""
    a = np.fromfile(MC_TABLES, dtype="<i4")
    assert a.size == 256 * 16 + 256, MC_TABLES
    return np.ascontiguousarray(a[:4096].reshape(256, 16)), np.ascontiguousarray(a[4096:])


def digest(nodes, query, k):
    h = hashlib.sha256(np.ascontiguousarray(nodes, np.float32).tobytes())
    h.update(np.ascontiguousarray(query, np.float32).tobytes())
    h.update(str(int(k)).encode())
    return h.hexdigest()


def knn(name, nodes, query, k):
    """nanoflann's k nearest nodes of every query (the reference's Warpfield search), stored under `name`: (n_query, k)
    int32, -1 where fewer than k nodes exist"""
    global _KNN
    if _KNN is None:
        with np.load(KNN) as z:
            _KNN = {key: z[key] for key in z.files}
    assert name + "__idx" in _KNN, "no stored reference answer %r in %s" % (name, KNN)
    assert str(_KNN[name + "__sha256"]) == digest(nodes, query, k), \
        "the inputs of %r differ from those its stored reference answer was computed from" % name
    idx = _KNN[name + "__idx"].astype(np.int32)
    assert idx.shape == (len(query), k)
    return idx


def nanoflann_dist2(nodes, query, idx):
    """the squared distances nanoflann reports with its answer (L2_Simple_Adaptor<float>: float differences squared and
    summed x, y, z in that order; -1 where the index is -1)"""
    q = np.ascontiguousarray(query, np.float32)[:, None, :]
    p = np.ascontiguousarray(nodes, np.float32)[np.maximum(idx, 0)]
    d = q - p
    sq = d * d
    out = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    return np.where(idx < 0, np.float32(-1), out).astype(np.float32)


# ------------------------------------------------------------------ the seeded inputs the answers belong to
def random_knn_case(D, k, n_query=3000):
    """nodes uniform in [-1, 1]^3, queries in [-1.2, 1.2]^3 (tests/test_oracle_solve.py::test_knn_matches_reference_nanoflann)"""
    rng = np.random.default_rng(D * 31 + k)
    nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
    query = rng.uniform(-1.2, 1.2, (n_query, 3)).astype(np.float32)
    return nodes, query


RANDOM_KNN_CASES = [(8, 8), (18, 8), (500, 4), (2048, 8), (5, 8)]


def opttest_knn_case(scn):
    """the nodes of both OptTest graphs and every vertex of every scene (tests/golden/opt_scenes.json)"""
    nodes = np.array(scn["nodes"]["g1"] + scn["nodes"]["g2"], np.float32)
    query = np.array([v for s in scn["scenes"] for vs in s["sets"].values() for v in vs], np.float32)
    return nodes, query


def surface_clouds(n_canon, n_live, seed):
    """canonical = points on the synthetic sphere cap, live = a displaced, differently sampled set"""
    from dynfu_amd import synth
    rng = np.random.default_rng(seed)

    def cap(n):
        d = rng.normal(size=(n, 3))
        d[:, 2] = -np.abs(d[:, 2])
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return (synth.SPHERE_C + 0.5 * d).astype(np.float32), d.astype(np.float32)
    cv, cn = cap(n_canon)
    lv, _ = cap(n_live)
    lv += rng.normal(0, 0.004, lv.shape).astype(np.float32)
    return cv, cn, lv


def correspond_clouds(n_canon, n_live):
    """surface_clouds with the first half of the shorter cloud's live points ON canonical points (exact hits)
    (tests/test_gpu_warp.py::test_correspond_bit_exact)"""
    cv, cn, lv = surface_clouds(n_canon, n_live, n_canon + n_live)
    lv[: min(n_live, n_canon) // 2] = cv[: min(n_live, n_canon) // 2]
    return cv, cn, lv


CORRESPOND_CASES = [(65536, 65536), (3000, 10000), (17, 1000), (1, 5), (40000, 129)]
CORRESPOND_QUERIES = 20000
MILLION = (1 << 20, 300000, 77)  # surface_clouds arguments of the million-point correspondence test
MILLION_QUERIES = 60000


def all_cases(scn):
    """(name, nodes, query, k) of every stored answer"""
    for D, k in RANDOM_KNN_CASES:
        yield ("random_D%d_k%d" % (D, k),) + random_knn_case(D, k) + (k,)
    yield ("opttest",) + opttest_knn_case(scn) + (8,)
    for n_canon, n_live in CORRESPOND_CASES:
        cv, _, lv = correspond_clouds(n_canon, n_live)
        yield "correspond_%d_%d" % (n_canon, n_live), cv, lv[:CORRESPOND_QUERIES], 1
    cv, _, lv = surface_clouds(*MILLION)
    yield "correspond_million", cv, lv[:MILLION_QUERIES], 1
