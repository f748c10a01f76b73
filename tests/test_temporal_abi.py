"""The temporal-accumulation ABI without a GPU: ctypes layouts against the C
compiler's, the default parameters, and every argument check of
spt_temporal_accumulate — each comes before any device work, so none of the
pointers below is ever dereferenced (include/spt.h)."""
import ctypes
import math
import os
import subprocess

import pytest

from sptamd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spt.h")
INV, LIMIT = _lib.SPT_ERR_INVALID, _lib.SPT_ERR_LIMIT
W = H = 8
PLANE = W * H * 4          # bytes of one plane


def test_struct_layouts_match_header(tmp_path):
    structs = {"spt_history": _lib.History, "spt_temporal_params": _lib.TemporalParams}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        cname, field, val = line.split()
        ct = structs[cname]
        got = ctypes.sizeof(ct) if field == "sizeof" else getattr(ct, field).offset
        assert got == int(val), (cname, field, got, val)
        seen += 1
    assert seen == 2 + len(_lib.History._fields_) + len(_lib.TemporalParams._fields_)
    assert [n for n, _ in _lib.History._fields_] == ["color", "moment2", "length"]


def test_entry_points_are_exported():
    for name in ("spt_default_temporal_params", "spt_temporal_accumulate", "spt_debug_camera_constants"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name


def test_default_temporal_params():
    p = _lib.default_temporal_params()
    r = _lib.default_params()
    assert (p.width, p.height) == (0, 0)
    assert p.samples == 1.0 and p.max_history == 64.0
    assert p.sigma_depth == ctypes.c_float(0.1).value and p.normal_min == ctypes.c_float(0.9).value
    assert list(p.reserved) == [0, 0]
    for cam in (p.camera, p.prev_camera):
        assert bytes(cam) == bytes(r.camera)
    _lib.lib.spt_default_temporal_params(None)   # NULL is ignored


def test_camera_constants_hook():
    p = _lib.default_params()
    c = _lib.camera_constants(p.camera, 70, 50)
    assert c["origin"] == tuple(p.camera.look_from) and (c["fw"], c["fh"]) == (70.0, 50.0)
    assert c["inv_fw"] == 0.0 and _lib.camera_constants(p.camera, 64, 50)["inv_fw"] == 1.0 / 64
    for k in ("bx", "by", "bz"):
        assert abs(math.sqrt(sum(x * x for x in c[k])) - 1.0) < 1e-6
    out = (ctypes.c_float * 22)()
    assert _lib.lib.spt_debug_camera_constants(None, 8, 8, out) == INV
    assert _lib.lib.spt_debug_camera_constants(ctypes.byref(p.camera), 0, 8, out) == INV
    assert _lib.lib.spt_debug_camera_constants(ctypes.byref(p.camera), 8, 8, None) == INV


def _params(**kw):
    p = _lib.default_temporal_params()
    p.width, p.height = W, H
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _aov(base, normals=True, **kw):
    a = _lib.Aov()
    a.depth, a.coverage = base, base + PLANE
    if normals:
        a.normal_x, a.normal_y, a.normal_z = base + 2 * PLANE, base + 3 * PLANE, base + 4 * PLANE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _hist(base, **kw):
    h = _lib.History()
    h.color, h.moment2, h.length = base, base + 3 * PLANE, base + 6 * PLANE
    for k, v in kw.items():
        setattr(h, k, v)
    return h


SUM, SUM_SQ, CUR, PREV, PREV_G, OUT, FILM, VAR = (0x100000 * k for k in range(1, 9))
NONE = object()


def _call(p=NONE, sum_=SUM, sum_sq=SUM_SQ, cur=NONE, prev=NONE, prev_guides=NONE, out=NONE, film=FILM, variance=VAR):
    ref = lambda x, make: None if x is None else ctypes.byref(make() if x is NONE else x)  # noqa: E731
    return _lib.lib.spt_temporal_accumulate(ref(p, _params), sum_, sum_sq, ref(cur, lambda: _aov(CUR)),
                                            ref(prev, lambda: _hist(PREV)), ref(prev_guides, lambda: _aov(PREV_G)),
                                            ref(out, lambda: _hist(OUT)), film, variance, None)


def test_null_arguments():
    assert _call(p=None) == INV
    assert _call(sum_=None) == INV
    assert _call(sum_sq=None) == INV
    assert _call(cur=None) == INV
    assert _call(out=None) == INV
    for member in ("color", "moment2", "length"):
        assert _call(out=_hist(OUT, **{member: None})) == INV and b"out" in _lib.lib.spt_last_error()
        assert _call(prev=_hist(PREV, **{member: None})) == INV


def test_missing_guide_planes():
    for plane in ("depth", "coverage"):
        assert _call(cur=_aov(CUR, **{plane: None})) == INV and b"cur" in _lib.lib.spt_last_error()
        assert _call(prev_guides=_aov(PREV_G, **{plane: None})) == INV and b"prev_guides" in _lib.lib.spt_last_error()


def test_prev_and_prev_guides_go_together():
    assert _call(prev=None) == INV
    assert _call(prev_guides=None) == INV and b"together" in _lib.lib.spt_last_error()


def test_parameter_checks():
    assert _call(p=_params(width=0)) == INV
    assert _call(p=_params(height=0)) == INV
    p = _params()
    p.reserved[1] = 1
    assert _call(p=p) == INV and b"reserved" in _lib.lib.spt_last_error()
    p = _params()
    p.reserved[0] = 7
    assert _call(p=p) == INV
    for bad in (0.0, 0.5, -1.0, float("nan"), float("inf")):
        assert _call(p=_params(samples=bad)) == INV and b"samples" in _lib.lib.spt_last_error(), bad
    for bad in (-1.0, -0.001, float("nan"), float("-inf")):
        assert _call(p=_params(max_history=bad)) == INV and b"max_history" in _lib.lib.spt_last_error(), bad
    assert _call(p=_params(width=65536, height=32768)) == LIMIT
    assert _call(p=_params(width=65536, height=65536)) == LIMIT


@pytest.mark.parametrize("prev", [True, False])
def test_overlapping_ranges(prev):
    kw = {} if prev else {"prev": None, "prev_guides": None}
    last = 4                      # the last float of a range
    inputs = [SUM, SUM + 3 * PLANE - last, SUM_SQ + PLANE, CUR, CUR + PLANE, CUR + 4 * PLANE]
    if prev:
        inputs += [PREV, PREV + 3 * PLANE, PREV + 7 * PLANE - last, PREV_G, PREV_G + PLANE, PREV_G + 5 * PLANE - last]
    for addr in inputs:
        # each output in turn starts on an input's float, or ends on it
        assert _call(film=addr, **kw) == INV and b"overlaps" in _lib.lib.spt_last_error(), hex(addr)
        assert _call(variance=addr - 3 * PLANE + last, **kw) == INV, hex(addr)
        assert _call(out=_hist(OUT, color=addr), **kw) == INV, hex(addr)
        assert _call(out=_hist(OUT, moment2=addr), **kw) == INV, hex(addr)
        assert _call(out=_hist(OUT, length=addr), **kw) == INV, hex(addr)
    # outputs against each other
    assert _call(film=VAR, **kw) == INV
    assert _call(film=OUT + 2 * PLANE, **kw) == INV
    assert _call(variance=OUT + 6 * PLANE, **kw) == INV
    assert _call(out=_hist(OUT, moment2=OUT + 2 * PLANE), **kw) == INV
    assert _call(out=_hist(OUT, length=OUT + 5 * PLANE), **kw) == INV
    if prev:
        # history must be ping-ponged: out = prev is refused
        assert _call(out=_hist(PREV)) == INV and b"prev" in _lib.lib.spt_last_error()
        assert _call(out=_hist(OUT, length=PREV_G + PLANE)) == INV
