"""The light-sampling input of the render's policy on the CPU (csrc/render_plan.h
RenderPlanIn::nee): with it the plan is the fused pipeline at every job size,
under every config and flag of the committed table; without it every row of the
table is the parent's, column for column.  tests/native/plan_nee_check.cpp is
built with the host compiler under the address and undefined-behaviour
sanitizers."""
import json
import os

from test_render_plan_cull import ROOT, _build, _run


def table():
    with open(os.path.join(ROOT, "tests", "golden", "render_plan_parent.json")) as f:
        return json.load(f)


def rows_text(rows, nee):
    return "".join(" ".join(str(v) for v in [nee] + list(r["in"])) + "\n" for r in rows)


def test_without_the_switch_every_plan_is_the_parents(tmp_path):
    t = table()
    exe = _build(tmp_path, "plan_nee_check")
    lines = _run(exe, rows_text(t["rows"], 0))
    assert len(lines) == len(t["rows"])
    for r, line in zip(t["rows"], lines):
        assert [int(x) for x in line.split()] == r["out"], r["name"]


def test_the_switch_forces_the_fused_pipeline(tmp_path):
    t = table()
    out = t["out_columns"]
    fused, limit, K, C = (out.index(k) for k in ("fused", "limit", "K", "C"))
    assert any(r["out"][fused] == 0 for r in t["rows"])          # the table has wavefront plans to turn
    exe = _build(tmp_path, "plan_nee_check")
    lines = _run(exe, rows_text(t["rows"], 1))
    assert len(lines) == len(t["rows"])
    for r, line in zip(t["rows"], lines):
        got = [int(x) for x in line.split()]
        if r["out"][limit]:       # explicit paths in flight beyond 2^31 are refused as before; a job that
            # only hit the limit by fitting in flight has no queues in the fused pipeline and runs
            assert got[limit] == 1 or (got[fused] == 1 and got[C] == 64), r["name"]
            continue
        assert got[limit] == 0 and got[fused] == 1 and got[K] == 1 and got[C] == 64, r["name"]
    # every job size, from one path to the 32-bit limit of a chunk, under each pipeline setting
    ic = t["in_columns"]
    base = list(next(r for r in t["rows"] if r["out"][fused] == 0 and r["out"][limit] == 0)["in"])
    P, spp, pipeline, flags = (ic.index(k) for k in ("P", "spp", "cfg.pipeline", "flags"))
    rows = []
    for pix, s in ((1, 1), (1000, 3), (1 << 20, 1), (1 << 20, 64), (1 << 24, 100), (1 << 26, 1 << 10)):
        for pl in (0, 1, 2):
            for fl in (0, 8, 2):                                  # none, SPT_FLAG_WAVEFRONT, SPT_FLAG_TRAVERSAL_STATS
                r = list(base)
                r[P], r[spp], r[pipeline], r[flags] = pix, s, pl, fl
                rows.append({"in": r})
    for line in _run(exe, rows_text(rows, 1)):
        got = [int(x) for x in line.split()]
        assert got[limit] == 0 and got[fused] == 1
