"""The root hand-off switch of the render's policy on the CPU (csrc/render_plan.h
RenderPlan::root_handoff): on exactly where the bounce cull is on and
SPT_FLAG_NO_ROOT_HANDOFF is clear — over the input grid of
test_render_plan_cull.py, each row with the flag clear and set.  The flag
changes nothing else of the plan: test_render_plan.py's table runs with it set
and must give the same rows.
tests/native/plan_root_check.cpp and plan_check.cpp are built with the host
compiler under the address and undefined-behaviour sanitizers."""
import json
import os

from sptamd import _lib
from test_render_plan_cull import NO_CULL, ROOT, _build, _run

NO_ROOT = _lib.SPT_FLAG_NO_ROOT_HANDOFF


def test_flag_value_matches_header():
    with open(os.path.join(ROOT, "include", "spt.h")) as f:
        assert "SPT_FLAG_NO_ROOT_HANDOFF = 64u" in f.read()
    assert NO_ROOT == 64 and NO_ROOT & (NO_ROOT - 1) == 0 and NO_ROOT != NO_CULL


def test_root_handoff_resolution(tmp_path):
    # (lockstep_first, flags, mode, nsph, wide_nodes, scene MiB) -> bounce_cull (test_render_plan_cull.py's grid)
    grid = [
        ((3, 0, 0, 0, 1, 28), 1),
        ((3, NO_CULL, 0, 0, 1, 28), 0),
        ((3, 8, 0, 0, 1, 28), 1),
        ((3, 8 | NO_CULL, 0, 0, 1, 28), 0),
        ((2, 0, 0, 0, 1, 28), 0),
        ((1, 0, 0, 0, 1, 28), 0),
        ((0, 0, 0, 0, 1, 28), 0),
        ((3, 0, 1, 0, 1, 28), 0),
        ((3, 0, 2, 0, 1, 28), 0),
        ((3, 0, 1, 9, 1, 28), 0),
        ((3, 0, 0, 9, 1, 28), 0),
        ((3, 0, 0, 0, 0, 28), 0),
        ((3, 0, 0, 0, 1, 255), 1),
        ((3, 0, 0, 0, 1, 256), 0),
    ]
    cases = []
    for c, cull in grid:
        cases.append((c, (cull, cull)))                                     # the flag clear: with the cull
        cases.append(((c[0], c[1] | NO_ROOT) + c[2:], (cull, 0)))           # the flag set: off, the cull as it was
    exe = _build(tmp_path, "plan_root_check")
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
    text = "".join(" ".join(str(v | NO_ROOT if i == fi else v) for i, v in enumerate(r["in"])) + "\n" for r in rows)
    lines = _run(exe, text)
    assert len(lines) == len(rows)
    for r, line in zip(rows, lines):
        assert [int(x) for x in line.split()] == r["out"], r["name"]
