"""The per-voxel comparison of a volume after dfa_tsdf_integrate_warped6 with tests/tsdf_warped6_statement.py, shared by
tests/test_gpu_tsdf_warped6.py and the north-star frame statement (tests/northstar_statement.py): on DECIDED voxels the
update set and the weights are the statement's exactly, the unpacked distance is within rho sqrt(3) / trunc + 2^-11 of it,
and what the statement leaves alone is the input bit for bit; an undecided voxel holds its input or a valid update."""
import numpy as np

import tsdf_warped6_cases as C6
import tsdf_warped_statement as WST
from extract_statement import unpack


def valid_update(before, after, tol, max_weight=C6.MAX_WEIGHT):
    """`after` is some update of `before` by the rule of tsdf_volume.cu:82-90: the weight one up (capped) and the distance the
    running average of the old one with a value in [-1, 1]"""
    F0, W0 = unpack(before)
    F1, W1 = unpack(after)
    Wf = W0.astype(np.float64)
    lo, hi = (F0 * Wf - 1) / (Wf + 1), (F0 * Wf + 1) / (Wf + 1)
    return (W1 == np.minimum(W0 + 1, max_weight)) & (F1 >= lo - tol) & (F1 <= hi + tol)


def check(got, c, want=None):
    """`got` against the statement's volume (or `want`) under the bar above.  c: name, vol (the input volume), trunc, ref
    (tsdf_warped6_statement.integrate's dict) and, where it is not tsdf_warped6_cases.MAX_WEIGHT, max_weight"""
    ref = c["ref"]
    want = ref["vol"] if want is None else want
    dec, upd, vol_in = ref["decided"], ref["updated"], c["vol"]
    max_weight = c.get("max_weight", C6.MAX_WEIGHT)
    tol = WST.tsdf_tolerance(ref["rho"], c["trunc"])
    Fg, Wg = unpack(got)
    Fw, Ww = unpack(want)
    m = dec & upd
    print("%s: %d voxels, %d updated by the statement, %d undecided, rho %.3g, tolerance %.3g" %
          (c["name"], got.size, int(upd.sum()), int((~dec).sum()), ref["rho"], tol))
    if m.any():
        print("  largest |tsdf - statement| on decided voxels: %.3g; weights differing: %d" %
              (float(np.abs(Fg[m] - Fw[m]).max()), int((Wg[m] != Ww[m]).sum())))
    print("  decided voxels the statement leaves alone that changed: %d" % int((got != vol_in)[dec & ~upd].sum()))
    sup = dec & upd & ref["supported"]
    sat = (vol_in >> 16) == max_weight
    print("  decided, supported, updated voxels that did not change (unsaturated): %d of %d" %
          (int((got == vol_in)[sup & ~sat].sum()), int((sup & ~sat).sum())))
    assert np.array_equal(Wg[m], Ww[m]), "weights of decided, updated voxels"
    assert np.all(np.abs(Fg[m] - Fw[m]) <= tol), "distances of decided, updated voxels"
    assert np.array_equal(got[dec & ~upd], vol_in[dec & ~upd]), "decided voxels the statement leaves alone"
    und = ~dec
    ok = (got[und] == vol_in[und]) | valid_update(vol_in[und], got[und], 2.0 ** -11, max_weight)
    assert ok.all(), "an undecided voxel holds neither its input nor a valid update"
