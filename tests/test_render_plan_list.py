"""The render's policy for listed jobs (csrc/render_plan.h RenderPlanIn::A,
spt_render_accum_list) on the CPU: the pipeline, the fit and the paths in
flight follow the A x spp work items, the film chunk the tile's pixels, and a
list of every pixel plans like the full pass.
tests/native/plan_list_check.cpp checks itself, built with the host compiler
under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")


def test_plan_render_for_listed_jobs(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "plan_list_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "native", "plan_list_check.cpp")],
                   check=True, capture_output=True)
    # (the leak check needs ptrace, which a sandboxed test run may not have; it is not what this looks for)
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-2000:])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    last = run.stdout.strip().split("\n")[-1].split()
    assert last[0] == "ok" and int(last[1]) > 3000, run.stdout[-500:]
