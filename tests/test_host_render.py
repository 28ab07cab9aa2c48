"""kfusion::KinFu::renderImage / DynFusion through the C++ host adaptor (tests/cpp/test_host_render.cpp): image sizes
per flag, the flag == 1 rule, equality with the C entry points and with raycast + render; and the PNG it writes, inflated
here with the standard zlib module and compared with the image's bytes."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _png_rgb(data):
    """(rows, cols, 3) uint8 of an 8-bit truecolour, non-interlaced PNG whose rows all use filter 0; chunk CRCs checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, ihdr, names = 8, b"", None, []
    while at < len(data):
        n, name = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(name + body)
        names.append(name)
        if name == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif name == b"IDAT":
            idat += body
        at += 12 + n
    assert names == [b"IHDR", b"IDAT", b"IEND"]  # one IDAT
    cols, rows, bits, colour, comp, filt, interlace = ihdr
    assert (bits, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(rows, 1 + 3 * cols)
    assert not raw[:, 0].any()  # filter 0 on every row
    return raw[:, 1:].reshape(rows, cols, 3)


def test_host_kinfu_render_image(tmp_path):
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_render"]
    png = str(tmp_path / "sphere.png")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, DFA_RENDER_PNG=png))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 tests, 0 failed" in r.stdout
    rgb = _png_rgb(open(png, "rb").read())
    bgr0 = np.fromfile(png + ".raw", np.uint8).reshape(480, 640, 4)
    assert rgb.shape == (480, 640, 3)
    assert np.array_equal(rgb, bgr0[..., 2::-1]) and not bgr0[..., 3].any()  # r, g, b of the PNG == b, g, r of the image
    # what one sees: the ramp from near-black to light blue behind a grey lit surface
    grey = (bgr0[..., 0] == bgr0[..., 1]) & (bgr0[..., 1] == bgr0[..., 2])
    assert 0.1 < grey.mean() < 0.999 and bgr0[240, 320, 0] > 200
    assert bgr0[0, 320].tolist() == [4, 2, 2, 0] and bgr0[479, 320].tolist() == [235, 119, 119, 0]
