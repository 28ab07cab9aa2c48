#!/usr/bin/env python3
"""Writes the reference's own answers that the tests compare against (tests/reference_data.py reads them):
  ref_mc_tables.bin   its marching-cubes case tables (oracle/extract_ref_mc_tables.py)
  ref_knn.npz         its vendored nanoflann k-NN (oracle/_ref/libref_knn.so, oracle/Makefile) on the seeded inputs of
                      tests/reference_data.all_cases: the indices and a digest of the inputs of every case
Needs a checkout of the reference; nothing of it enters the repository but these outputs.
Run:  python tests/golden/make_reference_outputs.py <reference root>"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import extract_ref_mc_tables  # noqa: E402
import oracle as O  # noqa: E402
import reference_data as R  # noqa: E402
from opt_scene_runner import SCN  # noqa: E402


def main(ref):
    extract_ref_mc_tables.main(ref, R.MC_TABLES)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "ref", "REF=" + os.path.abspath(ref)])
    assert O.ref_lib() is not None, "oracle/_ref/libref_knn.so was not built"
    out = {}
    for name, nodes, query, k in R.all_cases(SCN):
        idx, d = O.ref_knn(nodes, query, k)
        # the tests recompute the distances that go with the indices: they must be nanoflann's own, bit for bit
        assert np.array_equal(R.nanoflann_dist2(nodes, query, idx).view(np.uint32), d.view(np.uint32)), name
        out[name + "__idx"] = idx.astype(np.int16 if len(nodes) < 1 << 15 else np.int32)
        out[name + "__sha256"] = np.array(R.digest(nodes, query, k))
        print("%-24s %d queries, k = %d, %d nodes" % (name, len(query), k, len(nodes)))
    np.savez_compressed(R.KNN, **out)
    print("wrote", R.MC_TABLES, "and", R.KNN)


if __name__ == "__main__":
    main(sys.argv[1])
