"""The adaptive-sampling ABI without a GPU (include/spt.h): ctypes layouts
against the C compiler's, the default parameters, the scratch size and every
refusal of spt_adapt_select / spt_render_accum_list that comes before device work."""
import ctypes
import math
import subprocess

import pytest

from sptamd import _lib
from test_accum_abi import HEADER

INV, LIM = _lib.SPT_ERR_INVALID, _lib.SPT_ERR_LIMIT


def test_struct_layouts_match_header(tmp_path):
    structs = {"spt_adapt_params": _lib.AdaptParams, "spt_pixel_list": _lib.PixelList}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    # the structs the scene cache and earlier callers know keep their sizes
    for cname in ("spt_render_params", "spt_render_stats", "spt_accum", "spt_config", "spt_scene_stats"):
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    old = {"spt_render_params": _lib.RenderParams, "spt_render_stats": _lib.RenderStats, "spt_accum": _lib.Accum,
           "spt_config": _lib.Config, "spt_scene_stats": _lib.SceneStats}
    seen = 0
    for line in filter(None, out):
        cname, field, val = line.split()
        ct = structs.get(cname) or old[cname]
        got = ctypes.sizeof(ct) if field == "sizeof" else getattr(ct, field).offset
        assert got == int(val), (cname, field, got, val)
        seen += 1
    assert seen == 2 + len(_lib.AdaptParams._fields_) + len(_lib.PixelList._fields_) + len(old)
    assert [n for n, _ in _lib.AdaptParams._fields_] == ["min_spp", "max_spp", "tolerance", "floor", "reserved"]
    assert [n for n, _ in _lib.PixelList._fields_] == ["pixels", "n", "reserved", "count"]
    assert ctypes.sizeof(_lib.AdaptParams) == 24 and ctypes.sizeof(_lib.PixelList) == 24
    # the sizes of the commit before this ABI addition
    assert [ctypes.sizeof(old[k]) for k in ("spt_render_params", "spt_render_stats", "spt_accum", "spt_config",
                                            "spt_scene_stats")] == [120, 288, 40, 176, 64]


def test_new_entry_points_are_exported():
    for name in ("spt_default_adapt_params", "spt_adapt_select_scratch_bytes", "spt_adapt_select",
                 "spt_render_accum_list"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name


def test_default_adapt_params():
    p = _lib.default_adapt_params()
    assert (p.min_spp, p.max_spp) == (8, 1024)
    assert p.tolerance == ctypes.c_float(0.05).value and p.floor == ctypes.c_float(0.03).value
    assert list(p.reserved) == [0, 0]
    assert 0 < p.min_spp <= p.max_spp < (1 << 24) and math.isfinite(p.tolerance) and p.tolerance > 0 and p.floor > 0
    q = _lib.AdaptParams()
    q.reserved[0] = q.reserved[1] = 9
    _lib.lib.spt_default_adapt_params(ctypes.byref(q))
    assert list(q.reserved) == [0, 0]
    _lib.lib.spt_default_adapt_params(None)   # NULL is ignored


@pytest.mark.parametrize("npix", [0, 1, 63, 64, 65, 256, 257, 703, 65537, (1 << 31) - 1])
def test_scratch_bytes(npix):
    want = (8 * ((npix + 63) // 64) + 4 * ((npix + 255) // 256 + 1) + 15) & ~15
    assert _lib.lib.spt_adapt_select_scratch_bytes(npix) == want
    assert want % 16 == 0 and want >= 16


def _select(p, npix=64, base=4, sum_=0x1000, sum_sq=0x2000, count=0x3000, lst=0x4000, n=True, scratch=0x5000):
    # the pointers are never dereferenced: every case below is refused first
    out = ctypes.c_uint32(12345)
    rc = _lib.lib.spt_adapt_select(ctypes.byref(p) if p is not None else None, npix, base, sum_, sum_sq, count, lst,
                                   ctypes.byref(out) if n else None, scratch, None)
    return rc


def _rule(**kw):
    p = _lib.default_adapt_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_adapt_select_refusals_need_no_device():
    assert _select(None) == INV
    assert _select(_rule(), lst=None) == INV
    assert _select(_rule(), n=False) == INV
    assert _select(_rule(), scratch=None) == INV
    assert _select(_rule(), sum_=None) == INV
    assert _select(_rule(), sum_sq=None) == INV
    assert _select(_rule(), count=None) == INV and b"sample_base" in _lib.lib.spt_last_error()
    p = _rule(); p.reserved[0] = 1
    assert _select(p) == INV
    p = _rule(); p.reserved[1] = 1
    assert _select(p) == INV
    assert _select(_rule(min_spp=9, max_spp=8)) == INV
    for bad in (-0.5, float("nan"), float("inf"), float("-inf")):
        assert _select(_rule(tolerance=bad)) == INV, bad
        assert _select(_rule(floor=bad)) == INV, bad
    assert _select(_rule(), base=1 << 24) == LIM
    assert _select(_rule(), base=(1 << 24) + 5) == LIM
    assert _select(_rule(), npix=1 << 31) == LIM
    # the refusals hold at sample_base 0 too, where the inputs may be NULL
    assert _select(_rule(min_spp=9, max_spp=8), base=0, sum_=None, sum_sq=None, count=None) == INV
    assert _select(_rule(), base=0, sum_=None, sum_sq=None, count=None, lst=None) == INV


def test_adapt_select_of_no_pixels_needs_no_device():
    out = ctypes.c_uint32(7)
    rc = _lib.lib.spt_adapt_select(ctypes.byref(_rule()), 0, 4, 0x1000, 0x2000, 0x3000, 0x4000, ctypes.byref(out),
                                   0x5000, None)
    assert rc == 0 and out.value == 0


def test_render_accum_list_null_arguments_need_no_device():
    p = _lib.default_params()
    acc = _lib.Accum()
    acc.sum = 0x1000
    pl = _lib.PixelList()
    pl.pixels, pl.n = 0x9000, 1
    f = _lib.lib.spt_render_accum_list
    assert f(None, ctypes.byref(p), ctypes.byref(acc), ctypes.byref(pl), None, None) == INV
