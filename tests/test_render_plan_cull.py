"""The bounce-cull switch of the render's policy on the CPU (csrc/render_plan.h
RenderPlan::bounce_cull): on with the sharded camera cast (lockstep_first = 3,
the default) in unit mode, off under SPT_FLAG_NO_BOUNCE_CULL, with any other
first cast, in the albedo / emitter modes, with analytic spheres, without a
wide BVH and for scenes of 256 MiB or more on the device.  The flag changes
nothing else of the plan: test_render_plan.py's table runs with it set and must
give the same rows.
tests/native/plan_cull_check.cpp and plan_check.cpp are built with the host
compiler under the address and undefined-behaviour sanitizers."""
import json
import os
import shutil
import subprocess

from sptamd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")
NO_CULL = _lib.SPT_FLAG_NO_BOUNCE_CULL


def _build(tmp_path, name):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / name
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "native", name + ".cpp")],
                   check=True, capture_output=True)
    return exe


def _run(exe, text):
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    return run.stdout.strip().split("\n")


def test_flag_value_matches_header():
    with open(os.path.join(ROOT, "include", "spt.h")) as f:
        assert "SPT_FLAG_NO_BOUNCE_CULL = 32u" in f.read()
    assert NO_CULL == 32


def test_bounce_cull_resolution(tmp_path):
    # (lockstep_first, flags, mode, nsph, wide_nodes, scene MiB) -> (cam_cast, cam_shards, bounce_cull)
    cases = [
        ((3, 0, 0, 0, 1, 28), (1, 1, 1)),            # the default: on
        ((3, NO_CULL, 0, 0, 1, 28), (1, 1, 0)),      # the switch
        ((3, 8, 0, 0, 1, 28), (1, 1, 1)),            # other flags (SPT_FLAG_WAVEFRONT) leave it on
        ((3, 8 | NO_CULL, 0, 0, 1, 28), (1, 1, 0)),
        ((2, 0, 0, 0, 1, 28), (1, 0, 0)),            # the unsharded camera cast keeps its kernel
        ((1, 0, 0, 0, 1, 28), (0, 0, 0)),
        ((0, 0, 0, 0, 1, 28), (0, 0, 0)),
        ((3, 0, 1, 0, 1, 28), (1, 1, 0)),            # albedo mode: left uncut
        ((3, 0, 2, 0, 1, 28), (1, 1, 0)),            # emitter mode
        ((3, 0, 1, 9, 1, 28), (1, 1, 0)),            # analytic spheres are tested after the BVH
        ((3, 0, 0, 9, 1, 28), (1, 1, 0)),
        ((3, 0, 0, 0, 0, 28), (0, 0, 0)),            # BVH2: no camera cast at all
        ((3, 0, 0, 0, 1, 255), (1, 1, 1)),           # the scene-size rule: below 256 MiB on the device ...
        ((3, 0, 0, 0, 1, 256), (1, 1, 0)),           # ... and from there up (the streamed queue's scenes)
    ]
    exe = _build(tmp_path, "plan_cull_check")
    lines = _run(exe, "".join(" ".join(str(v) for v in c) + "\n" for c, _ in cases))
    assert len(lines) == len(cases)
    for (c, want), line in zip(cases, lines):
        assert tuple(int(x) for x in line.split()) == want, (c, line, want)


def test_flag_changes_nothing_else_of_the_plan(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "render_plan_parent.json")) as f:
        table = json.load(f)
    fi = table["in_columns"].index("flags")
    rows = table["rows"]
    exe = _build(tmp_path, "plan_check")
    text = "".join(" ".join(str(v | NO_CULL if i == fi else v) for i, v in enumerate(r["in"])) + "\n" for r in rows)
    lines = _run(exe, text)
    assert len(lines) == len(rows)
    for r, line in zip(rows, lines):
        assert [int(x) for x in line.split()] == r["out"], r["name"]
