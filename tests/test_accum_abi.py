"""The progressive-render / variance-guided denoiser ABI without a GPU: ctypes
layouts against the C compiler's, the default parameters, the scratch size and
the argument checks that come before any device work (include/spt.h)."""
import ctypes
import math
import os
import subprocess

import pytest

from sptamd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spt.h")


def test_struct_layouts_match_header(tmp_path):
    structs = {"spt_accum": _lib.Accum, "spt_denoise_var_params": _lib.DenoiseVarParams}
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
    assert seen == 2 + len(_lib.Accum._fields_) + len(_lib.DenoiseVarParams._fields_)
    assert [n for n, _ in _lib.Accum._fields_] == ["sample_base", "reserved", "sum", "sum_sq", "film", "variance"]


def test_new_entry_points_are_exported():
    for name in ("spt_render_accum", "spt_render_accum_async", "spt_default_denoise_var_params",
                 "spt_denoise_var_scratch_bytes", "spt_denoise_var"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name), name


def test_default_denoise_var_params():
    p = _lib.default_denoise_var_params()
    d = _lib.default_denoise_params()
    assert (p.width, p.height) == (0, 0)
    assert p.iterations == 5
    assert p.sigma_variance == 4.0
    for k in ("sigma_normal", "sigma_albedo", "sigma_depth"):
        assert getattr(p, k) == getattr(d, k) and math.isfinite(getattr(p, k)) and getattr(p, k) > 0, k
    _lib.lib.spt_default_denoise_var_params(None)   # NULL is ignored


@pytest.mark.parametrize("w,h", [(1, 1), (37, 19), (1024, 1024), (65535, 40000)])
def test_scratch_bytes(w, h):
    assert _lib.lib.spt_denoise_var_scratch_bytes(w, h) == 2 * (3 + 1) * 4 * w * h


def _denoise(p, color=0x1000, variance=0x5000, out=0x2000, vout=0x4000, scratch=0x3000):
    # the pointers are never dereferenced: every case below is refused first
    return _lib.lib.spt_denoise_var(ctypes.byref(p) if p is not None else None, color, variance, None, out, vout,
                                    scratch, None)


def _params(w=8, h=8, it=2):
    p = _lib.default_denoise_var_params()
    p.width, p.height, p.iterations = w, h, it
    return p


def test_denoise_var_argument_checks_need_no_device():
    inv = _lib.SPT_ERR_INVALID
    assert _denoise(None) == inv
    assert _denoise(_params(w=0)) == inv
    assert _denoise(_params(h=0)) == inv
    assert _denoise(_params(it=9)) == inv and b"iterations" in _lib.lib.spt_last_error()
    assert _denoise(_params(), color=None) == inv
    assert _denoise(_params(), variance=None) == inv
    assert _denoise(_params(), out=None) == inv
    assert _denoise(_params(), scratch=None) == inv
    assert _denoise(_params(it=1), scratch=None) == inv
    assert _denoise(_params(), color=0x1000, out=0x1000) == inv      # out must not alias color
    assert _denoise(_params(), variance=0x2000, out=0x2000) == inv   # ... or the variance
    assert _denoise(_params(), vout=0x2000) == inv                   # variance_out must not alias out
    assert _denoise(_params(w=65536, h=65536)) == _lib.SPT_ERR_LIMIT


def test_render_accum_null_arguments_need_no_device():
    p = _lib.default_params()
    acc = _lib.Accum()
    acc.sum = 0x1000
    ticket = ctypes.c_uint64()
    assert _lib.lib.spt_render_accum(None, ctypes.byref(p), ctypes.byref(acc), None, None) == _lib.SPT_ERR_INVALID
    assert _lib.lib.spt_render_accum_async(None, ctypes.byref(p), ctypes.byref(acc), None,
                                           ctypes.byref(ticket)) == _lib.SPT_ERR_INVALID
