"""spt_temporal_accumulate's per-pixel arithmetic on the host, and its kernels
in the built library (no GPU).

tests/native/temporal_check.cpp compiles csrc/temporal.h — the text the kernel
compiles — with the host compiler under ASan + UBSan and holds it against a
float64 restatement on a grid of pixels, sizes and depths: the same view twice
(every pixel snaps onto itself), a moved view, a view turned away.  The
kernels of namespace spt_temporal in libspt.so must be exactly the ones the
GPU tests launch (tests/test_gpu_temporal.py KERNELS), and none of them may sit
in namespace spt, whose kernels tests/instance_matrix.py accounts for."""
import os
import re
import shutil
import subprocess

import pytest

import kernel_inventory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")
LINE = re.compile(r"(\w+) (\d+)x(\d+) z (\S+) pixels (\d+) history (\d+) exact (\d+) flips (\d+) maxerr (\S+)$")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("temporal_check")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = d / "temporal_check"
    root = os.environ.get("ROCM_PATH", "/opt/rocm")   # spt_math.h includes the HIP runtime header for its markers
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(root, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "temporal_check.cpp")], check=True, capture_output=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(run.stdout)
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    return run


def rows(report):
    out = []
    for line in report.stdout.strip().split("\n"):
        m = LINE.match(line)
        if m:
            out.append((m.group(1), (int(m.group(2)), int(m.group(3))), float(m.group(4))) +
                       tuple(int(v) for v in m.groups()[4:8]) + (float(m.group(9)),))
    return out


def test_per_pixel_function_against_float64(report):
    assert report.returncode == 0, report.stdout[-2000:] + report.stderr[-2000:]
    assert "temporal_check ok" in report.stdout and "FAIL" not in report.stdout
    rs = rows(report)
    assert {r[0] for r in rs} == {"same", "same_lens", "moved", "away"}
    assert len(rs) == 4 * 5 * 5                       # views x sizes x depths
    assert {r[2] for r in rs} == {0.05, 0.7, 5.0, 37.0, 500.0}
    for name, size, z, pixels, history, exact, flips, maxerr in rs:
        assert pixels == size[0] * size[1]
        assert maxerr <= 1e-5, (name, size, z, maxerr)
        if name in ("same", "same_lens"):
            assert flips == 0 and history == pixels - (pixels + 3) // 7, (name, size, z)
        if name == "away":
            assert history == 0
    # the moved view is not vacuous: most pixels of the wide images find a history
    assert sum(r[4] for r in rs if r[0] == "moved") > 100000


def test_library_kernels_are_the_ones_the_gpu_tests_launch():
    import test_gpu_temporal
    try:
        names = kernel_inventory.all_kernels()
    except kernel_inventory.InventoryError as e:
        pytest.fail(str(e))
    mine = sorted(n for n in names if "spt_temporal" in n)
    assert mine == sorted(test_gpu_temporal.KERNELS) and len(mine) >= 1
    for n in mine:
        assert n.startswith("_ZN12spt_temporal") and not n.startswith("_ZN3spt")
    # and nothing of this feature went into namespace spt
    assert not [n for n in names if n.startswith("_ZN3spt") and "temporal" in n.lower()]
