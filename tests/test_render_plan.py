"""The render's policy on the CPU (csrc/render_plan.h plan_render): which
pipeline runs, whether the job fits in flight and in how many chunks, the paths
the memory rule allows, work order, queue caching, the drain's refill
threshold, sub-wavefronts and film chunk — at thresholds no test render
reaches (a 256 MiB scene, 16M fused paths, 2^28 fit paths, the 4M-pixel tile,
the 2^31 limit).

tests/golden/render_plan_parent.json holds the decisions of the commit before
the policy became a function: its decision block, copied verbatim into a
harness with stubbed inputs, printed the `out` rows (and agreed with
plan_render on 7 000 000 random inputs drawn at, one below and one above every
threshold of the block).  tests/native/plan_check.cpp runs plan_render on the
`in` rows, built with the host compiler under the address and
undefined-behaviour sanitizers."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")


def test_plan_render_matches_parent_decisions(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "render_plan_parent.json")) as f:
        table = json.load(f)
    rows = table["rows"]
    assert len(rows) >= 36 and all(len(r["in"]) == len(table["in_columns"]) for r in rows)
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "native", "plan_check.cpp")],
                   check=True, capture_output=True)
    text = "".join(" ".join(str(v) for v in r["in"]) + "\n" for r in rows)
    # (the leak check needs ptrace, which a sandboxed test run may not have; it is not what this looks for)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    lines = run.stdout.strip().split("\n")
    assert len(lines) == len(rows)
    for r, line in zip(rows, lines):
        got = dict(zip(table["out_columns"], (int(x) for x in line.split())))
        want = dict(zip(table["out_columns"], r["out"]))
        assert got == want, (r["name"], {k: (got[k], want[k]) for k in want if got[k] != want[k]})
