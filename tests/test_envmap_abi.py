"""The environment-map ABI without a GPU (include/spt.h): the prototypes against
the ctypes mirror, every refusal of spt_scene_set_envmap that comes before the
scene or the device is touched, spt_envmap_from_latlong against its float64
restatement, and spt_pfm_read against spt_pfm_write."""
import ctypes
import struct
import subprocess

import numpy as np
import pytest

import envmap_ref as E
import sptamd
from sptamd import _lib
from test_accum_abi import HEADER

INV, LIM, IO = _lib.SPT_ERR_INVALID, _lib.SPT_ERR_LIMIT, _lib.SPT_ERR_IO
F = np.float32
NEW = ("spt_scene_set_envmap", "spt_envmap_from_latlong", "spt_pfm_read", "spt_pfm_free")


def test_new_entry_points_are_exported_and_mirrored(tmp_path):
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name
    vp, u32, cp = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p
    fpp = ctypes.POINTER(ctypes.POINTER(ctypes.c_float))
    want = {"spt_scene_set_envmap": (ctypes.c_int32, [vp, vp, u32, vp]),
            "spt_envmap_from_latlong": (ctypes.c_int32, [vp, u32, u32, u32, vp]),
            "spt_pfm_read": (ctypes.c_int32, [cp, fpp, ctypes.POINTER(u32), ctypes.POINTER(u32)]),
            "spt_pfm_free": (None, [ctypes.POINTER(ctypes.c_float)])}
    for name, (res, args) in want.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    # the header declares exactly these prototypes (an incompatible pointer is an error)
    src = tmp_path / "proto.c"
    src.write_text(f'''#include "{HEADER}"
spt_status (*f0)(spt_scene, const float*, uint32_t, const float*) = spt_scene_set_envmap;
spt_status (*f1)(const float*, uint32_t, uint32_t, uint32_t, float*) = spt_envmap_from_latlong;
spt_status (*f2)(const char*, float**, uint32_t*, uint32_t*) = spt_pfm_read;
void (*f3)(float*) = spt_pfm_free;
int main(void) {{ return sizeof(spt_render_params) == 120 && sizeof(spt_config) == 176 && sizeof(spt_accum) == 40 ? 0 : 1; }}
''')
    subprocess.run(["gcc", "-Werror", "-Wall", "-c", "-o", str(tmp_path / "proto.o"), str(src)], check=True)
    # the structs earlier callers and the scene cache know keep their sizes
    assert [ctypes.sizeof(t) for t in (_lib.RenderParams, _lib.Config, _lib.Accum)] == [120, 176, 40]
    for name in ("set_envmap",):
        assert callable(getattr(sptamd.HipBackend, name))
    assert callable(sptamd.envmap_from_latlong) and callable(sptamd.read_pfm)
    assert "envmap_from_latlong" in sptamd.__all__ and "read_pfm" in sptamd.__all__


def _set(scene, img, n, rot=None):
    return _lib.lib.spt_scene_set_envmap(scene, None if img is None else img.ctypes.data, n,
                                         None if rot is None else rot.ctypes.data)


def test_set_envmap_refusals_need_no_device():
    fake = 0x1000    # never dereferenced: every case below is refused first
    img = np.ones((2, 2, 3), F)
    assert _set(None, img, 2) == INV and b"NULL scene" in _lib.lib.spt_last_error()
    assert _set(None, None, 0) == INV
    assert _set(fake, img, 0) == INV
    assert _lib.lib.spt_scene_set_envmap(fake, 0x2000, 4097, None) == LIM      # before a texel is read
    assert _lib.lib.spt_scene_set_envmap(fake, 0x2000, 0xffffffff, None) == LIM
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 5, 11):
            x = img.copy()
            x.reshape(-1)[k] = bad
            assert _set(fake, x, 2) == INV, (bad, k)
            assert b"not finite" in _lib.lib.spt_last_error()
        for k in (0, 4, 8):
            r = np.eye(3, dtype=F)
            r.reshape(-1)[k] = bad
            assert _set(fake, img, 2, r) == INV, (bad, k)
            assert b"rotation" in _lib.lib.spt_last_error()


def _latlong(img, n, out=True):
    h, w = img.shape[:2]
    o = np.full((n, n, 3), -7.0, F)
    rc = _lib.lib.spt_envmap_from_latlong(img.ctypes.data, w, h, n, o.ctypes.data if out else None)
    return rc, o


def test_from_latlong_refusals():
    img = np.ones((8, 16, 3), F)
    assert _lib.lib.spt_envmap_from_latlong(None, 16, 8, 8, 0x1000) == INV
    assert _latlong(img, 8, out=False)[0] == INV
    assert _lib.lib.spt_envmap_from_latlong(img.ctypes.data, 0, 8, 8, 0x1000) == INV
    assert _lib.lib.spt_envmap_from_latlong(img.ctypes.data, 16, 0, 8, 0x1000) == INV
    assert _lib.lib.spt_envmap_from_latlong(img.ctypes.data, 16, 8, 0, 0x1000) == INV
    assert _lib.lib.spt_envmap_from_latlong(img.ctypes.data, 16, 8, 4097, 0x1000) == LIM
    with pytest.raises(ValueError):
        sptamd.envmap_from_latlong(np.ones((8, 16), F), 8)


def ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_from_latlong_equals_the_f64_restatement():
    rng = np.random.default_rng(11)
    img = rng.uniform(0.1, 8.0, size=(8, 16, 3)).astype(F)
    rc, got = _latlong(img, 8)
    assert rc == 0
    want = E.from_latlong(img, 8)
    worst = int(ulps(got, want).max())
    print(f"16 x 8 -> 8: worst difference {worst} ulp")
    assert worst <= 1      # both compute in f64 and round once
    np.testing.assert_array_equal(sptamd.envmap_from_latlong(img, 8), got)
    # a constant image stays constant; the poles read the first and last rows
    rc, c = _latlong(np.full((4, 8, 3), 2.5, F), 5)
    assert rc == 0 and (c == 2.5).all()
    rows = np.zeros((32, 8, 3), F)
    rows[:] = np.arange(32, dtype=F)[:, None, None]
    rc, r = _latlong(rows, 9)
    assert rc == 0 and r[4, 4, 0] == 0.0 and r[0, 0, 0] > 29.0 and r[8, 8, 0] > 29.0
    # phi = atan2(y, x): +x is column 0's left edge, +y a quarter of the way along
    cols = np.zeros((4, 16, 3), F)
    cols[:] = np.arange(16, dtype=F)[None, :, None]
    rc, q = _latlong(cols, 9)
    assert rc == 0 and abs(q[8 - 0, 4, 0] - 3.5) < 1e-5          # (a, b) = (0, 1 - 1/9): +y, u = 1/4 -> 16/4 - 0.5
    assert abs(q[4, 0, 0] - 7.5) < 1e-5                          # -x: u = 1/2


def test_pfm_read_inverts_pfm_write(tmp_path):
    rng = np.random.default_rng(13)
    film = rng.normal(size=(3, 5, 7)).astype(F)
    film[0, 0, 0], film[1, 2, 3], film[2, 4, 6] = 1e30, -0.0, 1e-40     # bits, not values
    path = str(tmp_path / "x.pfm")
    sptamd.write_pfm(path, film)
    got = sptamd.read_pfm(path)
    assert got.shape == (5, 7, 3) and got.dtype == F
    np.testing.assert_array_equal(got.view(np.uint32), np.ascontiguousarray(film.transpose(1, 2, 0)).view(np.uint32))
    # a big-endian file (positive scale), CRLF-free header with a comment-free body
    be = str(tmp_path / "be.pfm")
    with open(be, "wb") as f:
        f.write(b"PF\n7 5\n1.0\n")
        f.write(np.ascontiguousarray(film.transpose(1, 2, 0)[::-1]).astype(">f4").tobytes())
    np.testing.assert_array_equal(sptamd.read_pfm(be).view(np.uint32), got.view(np.uint32))


def test_pfm_read_refusals(tmp_path):
    p, w, h = ctypes.POINTER(ctypes.c_float)(), ctypes.c_uint32(9), ctypes.c_uint32(9)

    def read(path):
        rc = _lib.lib.spt_pfm_read(str(path).encode(), ctypes.byref(p), ctypes.byref(w), ctypes.byref(h))
        assert not p and (w.value, h.value) == (0, 0) if rc else True
        return rc

    assert read(tmp_path / "missing.pfm") == IO
    assert _lib.lib.spt_pfm_read(None, ctypes.byref(p), ctypes.byref(w), ctypes.byref(h)) == INV
    assert _lib.lib.spt_pfm_read(b"x", None, ctypes.byref(w), ctypes.byref(h)) == INV
    cases = {"grey": b"Pf\n2 2\n-1\n" + bytes(16), "magic": b"P6\n2 2\n255\n" + bytes(12), "empty": b"",
             "zero": b"PF\n0 2\n-1\n", "scale0": b"PF\n2 2\n0\n" + bytes(48), "nohdr": b"PF\n2\n",
             "text": b"PF\ntwo 2\n-1\n" + bytes(48)}
    for name, data in cases.items():
        f = tmp_path / f"{name}.pfm"
        f.write_bytes(data)
        assert read(f) == INV, name
    short = tmp_path / "short.pfm"
    short.write_bytes(b"PF\n2 2\n-1\n" + bytes(47))
    assert read(short) == IO
    with pytest.raises(sptamd.SptError):
        sptamd.read_pfm(str(short))
    _lib.lib.spt_pfm_free(None)     # NULL is ignored
    assert struct.calcsize("f") == 4
