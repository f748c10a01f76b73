"""The AOV / denoiser ABI without a GPU: ctypes layouts against the C
compiler's, the default denoiser parameters, the scratch size and the
argument checks that come before any device work (include/spt.h)."""
import ctypes
import math
import os
import subprocess

import pytest

from sptamd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spt.h")


def test_struct_layouts_match_header(tmp_path):
    structs = {"spt_aov": _lib.Aov, "spt_denoise_params": _lib.DenoiseParams}
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
    assert seen == 2 + len(_lib.Aov._fields_) + len(_lib.DenoiseParams._fields_)
    assert [n for n, _ in _lib.Aov._fields_] == list(_lib.AOV_PLANES)


def test_default_denoise_params():
    p = _lib.default_denoise_params()
    assert (p.width, p.height) == (0, 0)
    assert 1 <= p.iterations <= 8
    for k in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"):
        v = getattr(p, k)
        assert math.isfinite(v) and v > 0, k
    _lib.lib.spt_default_denoise_params(None)   # NULL is ignored


@pytest.mark.parametrize("w,h", [(1, 1), (37, 19), (1024, 1024), (65535, 40000)])
def test_scratch_bytes(w, h):
    assert _lib.lib.spt_denoise_scratch_bytes(w, h) >= 2 * 3 * 4 * w * h


def _denoise(p, color=0x1000, out=0x2000, scratch=0x3000):
    # the pointers are never dereferenced: every case below is refused first
    return _lib.lib.spt_denoise(ctypes.byref(p) if p is not None else None, color, None, out, scratch, None)


def _params(w=8, h=8, it=2):
    p = _lib.default_denoise_params()
    p.width, p.height, p.iterations = w, h, it
    return p


def test_denoise_argument_checks_need_no_device():
    inv = _lib.SPT_ERR_INVALID
    assert _denoise(None) == inv
    assert _denoise(_params(w=0)) == inv
    assert _denoise(_params(h=0)) == inv
    assert _denoise(_params(it=9)) == inv and b"iterations" in _lib.lib.spt_last_error()
    assert _denoise(_params(), color=None) == inv
    assert _denoise(_params(), out=None) == inv
    assert _denoise(_params(), scratch=None) == inv
    assert _denoise(_params(it=1), scratch=None) == inv
    assert _denoise(_params(), color=0x1000, out=0x1000) == inv      # out must not alias color
    assert _denoise(_params(w=65536, h=65536)) == _lib.SPT_ERR_LIMIT


def test_render_aov_null_arguments_need_no_device():
    p = _lib.default_params()
    aov = _lib.Aov()
    assert _lib.lib.spt_render_aov(None, ctypes.byref(p), ctypes.byref(aov), None) == _lib.SPT_ERR_INVALID
