"""The camera entry switch of the render's policy on the CPU (csrc/render_plan.h
RenderPlan::camera_entry) as a truth table over its inputs: on exactly where
the camera cast runs (the wavefront pipeline with lockstep_first >= 2 on a wide
BVH), the tree has 64-B six-wide nodes, the camera is a pinhole and
SPT_FLAG_NO_CAMERA_ENTRY is clear — whatever the path mode and the analytic
spheres — with 4 bytes per tile pixel for the table, none where it is off.  The
flag changes nothing else of the plan: test_render_plan.py's table runs with it
set and must give the same rows.
tests/native/plan_entry_check.cpp and plan_check.cpp are built with the host
compiler under the address and undefined-behaviour sanitizers."""
import itertools
import json
import os

from sptamd import _lib
from test_render_plan_cull import NO_CULL, ROOT, _build, _run
from test_render_plan_root import NO_ROOT

NO_ENTRY = _lib.SPT_FLAG_NO_CAMERA_ENTRY
FUSED, WAVEFRONT = _lib.SPT_FLAG_FUSED, _lib.SPT_FLAG_WAVEFRONT


def test_flag_value_matches_header():
    with open(os.path.join(ROOT, "include", "spt.h")) as f:
        assert "SPT_FLAG_NO_CAMERA_ENTRY = 128u" in f.read()
    assert NO_ENTRY == 128 and NO_ENTRY & (NO_ENTRY - 1) == 0 and NO_ENTRY not in (NO_CULL, NO_ROOT)


def test_camera_entry_truth_table(tmp_path):
    P = 1 << 20
    cases = []
    # every combination of the rule's inputs on config 1's job (a fitting wavefront job)
    for lock, flag, wide, node6, pinhole in itertools.product((0, 1, 2, 3), (0, NO_ENTRY), (0, 1), (0, 1), (0, 1)):
        cam = int(lock >= 2 and wide)
        on = int(cam and node6 and pinhole and not flag)
        cases.append(((lock, flag, wide, node6, pinhole, 0, 0, P), (0, cam, on, 4 * P * on)))
    # the other switches and the path modes leave it alone
    for flags, mode, nsph in ((NO_CULL, 0, 0), (NO_ROOT, 0, 0), (WAVEFRONT, 0, 0), (0, 1, 0), (0, 2, 0), (0, 1, 9)):
        cases.append(((3, flags, 1, 1, 1, mode, nsph, P), (0, 1, 1, 4 * P)))
        cases.append(((3, flags | NO_ENTRY, 1, 1, 1, mode, nsph, P), (0, 1, 0, 0)))
    # the fused pipeline has no camera cast: by the flag, and by the job size (64 x 64 pixels x 64 spp)
    cases.append(((3, FUSED, 1, 1, 1, 0, 0, P), (1, 1, 0, 0)))
    cases.append(((3, 0, 1, 1, 1, 0, 0, 64 * 64), (1, 1, 0, 0)))
    cases.append(((3, WAVEFRONT, 1, 1, 1, 0, 0, 64 * 64), (0, 1, 1, 4 * 64 * 64)))
    cases.append(((3, 0, 1, 1, 1, 0, 0, 1000003), (0, 1, 1, 4 * 1000003)))      # 4 B per tile pixel, any P
    exe = _build(tmp_path, "plan_entry_check")
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
    text = "".join(" ".join(str(v | NO_ENTRY if i == fi else v) for i, v in enumerate(r["in"])) + "\n" for r in rows)
    lines = _run(exe, text)
    assert len(lines) == len(rows)
    for r, line in zip(rows, lines):
        assert [int(x) for x in line.split()] == r["out"], r["name"]
