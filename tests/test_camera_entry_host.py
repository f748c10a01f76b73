"""The camera entry table's contract without a GPU (csrc/camera_entry.h, DESIGN.md
§4 "Camera entry"): tests/native/entry_check.cpp, built with the host compiler
under ASan + UBSan together with the host builders, walks every pixel's chain on
trees of 64-B nodes (the 200- and 5000-triangle soups as generated, with a flat
z and with an outlier; a ground with a box on it) under seeded pinhole cameras
at 16 x 16, 64 x 64 and 24 x 17, and at every chain node checks that no camera
ray of the pixel — 64 seeded xi and the four corners, in f32 with the camera
functions of spt_math.h — is accepted by the per-ray visit into a child other
than the chain's.  The ground-and-box scene must have entries below the root,
so the check is not vacuous."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")
LINE = re.compile(r"(\w+) cam(\d) (\d+)x(\d+) pixels (\d+) below (\d+) nodes (\d+) visits (\d+) bad (\d+) deepest (\d+)$")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("entry_check")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = d / "entry_check"
    root = os.environ.get("ROCM_PATH", "/opt/rocm")   # spt_math.h includes the HIP runtime header for its markers
    srcs = [os.path.join(ROOT, "tests", "native", "entry_check.cpp"), os.path.join(CSRC, "bvh_build.cpp"),
            os.path.join(CSRC, "bvh8_build.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests", "native"),
                    "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(root, "include"), "-o", str(exe), *srcs, "-lpthread"],
                   check=True, capture_output=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(run.stdout)
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    return run


def rows(report):
    out = []
    for line in report.stdout.strip().split("\n"):
        m = LINE.match(line)
        if m:
            out.append((m.group(1), int(m.group(2)), (int(m.group(3)), int(m.group(4)))) + tuple(int(v) for v in m.groups()[4:]))
    return out


def test_no_ray_leaves_its_pixels_chain(report):
    rs = rows(report)
    scenes = {r[0] for r in rs}
    assert scenes == {f"soup{n}_{v}" for n in (200, 5000) for v in ("plain", "flat_z", "outlier")} | {"ground_box"}
    assert len(rs) == 7 * 4 * 3
    for name, cam, size, pixels, below, nodes, visits, bad, deepest in rs:
        assert pixels == size[0] * size[1] and visits == 68 * nodes and below <= pixels, (name, cam, size)
        assert bad == 0, (name, cam, size, bad)
    assert report.returncode == 0, report.stderr[-2000:]
    # the chains are there to be checked: over all scenes, many nodes and millions of ray visits
    assert sum(r[5] for r in rs) > 10000 and sum(r[6] for r in rs) > 1000000


def test_ground_and_box_has_entries_below_the_root(report):
    rs = [r for r in rows(report) if r[0] == "ground_box" and r[1] == 0]
    assert len(rs) == 3
    for name, cam, size, pixels, below, nodes, visits, bad, deepest in rs:
        print(f"{name} {size}: {below} of {pixels} pixels enter below the root, deepest chain {deepest}")
        assert below > 0 and deepest >= 1, (size, below)
    # smaller pixels, longer chains: the share at 64 x 64 is at least that at 16 x 16
    share = {r[2]: r[4] / r[3] for r in rs}
    assert share[(64, 64)] >= share[(16, 16)]


def test_cameras_without_a_beam(report):
    assert "no_beam 5 of 5, beam 1" in report.stdout
