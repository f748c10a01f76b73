"""The geometry-update ABI and the refit arithmetic without a GPU: the ctypes
layout of spt_refit_stats against the C compiler's, the exported names, the
argument checks that come before any device work, and the serial host
restatement of the refit (tests/native/refit_check.cpp over csrc/bvh_refit.h)
against the host builders."""
import ctypes
import os
import shutil
import subprocess

from sptamd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spt.h")
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")
NAMES = ("spt_scene_update_geometry", "spt_scene_update_geometry_device", "spt_scene_get_refit_stats")


def test_refit_stats_layout_matches_header(tmp_path):
    ct = _lib.RefitStats
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(spt_refit_stats));']
    for fname, _ in ct._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(spt_refit_stats, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        field, val = line.split()
        got = ctypes.sizeof(ct) if field == "sizeof" else getattr(ct, field).offset
        assert got == int(val), (field, got, val)
        seen += 1
    assert seen == 1 + len(ct._fields_)
    assert [n for n, _ in ct._fields_] == ["updates", "nodes", "tris", "levels", "reserved", "plan_bytes", "plan_ms",
                                           "update_ms", "refit_ms", "area_built", "area_now"]


def test_names_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in _lib.EXPORTED
        assert getattr(lib, n) is not None
        assert getattr(_lib.lib, n).argtypes is not None


def test_null_arguments_need_no_device():
    inv = _lib.SPT_ERR_INVALID
    lib = _lib.lib
    # the pointers are never dereferenced: every case is refused first
    assert lib.spt_scene_update_geometry(None, 0x1000, 0x2000, 3, 1, None, None, 0) == inv
    assert b"NULL scene" in lib.spt_last_error()
    assert lib.spt_scene_update_geometry_device(None, 0x1000, 0x2000, 3, 1, None, None, 0, None) == inv
    assert b"NULL scene" in lib.spt_last_error()
    st = _lib.RefitStats()
    assert lib.spt_scene_get_refit_stats(None, ctypes.byref(st)) == inv
    assert b"spt_scene_get_refit_stats" in lib.spt_last_error()
    assert lib.spt_scene_get_refit_stats(0x1000, None) == inv
    assert b"NULL" in lib.spt_last_error()


def test_host_refit_restates_the_builders(tmp_path):
    """refit_check.cpp: an identity refit leaves every node word of
    build_bvh8 (widths 8 and 6) and build_bvh as built; after a refit with
    moved vertices every stored child box encloses its triangles, empty slots
    stay inverted, the topology words are untouched, and refitting back
    restores the built nodes."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    exe = tmp_path / "refit_check"
    srcs = [os.path.join(ROOT, "tests", "native", "refit_check.cpp"), os.path.join(CSRC, "bvh_build.cpp"),
            os.path.join(CSRC, "bvh8_build.cpp")]
    if cxx:
        cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + CSRC, "-o", str(exe), *srcs, "-lpthread"]
    else:  # no host C++ compiler: hipcc's host side
        cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-ffp-contract=off", "-x", "c++", "-I" + CSRC, "-o",
               str(exe), *srcs, "-lpthread"]
    subprocess.run(cmd, check=True, capture_output=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and '"bad": 0' in res.stdout, res.stdout + res.stderr
