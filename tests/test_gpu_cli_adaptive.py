"""spt_render_cli --adaptive (csrc/main.cpp): passes of -s, 2 -s, 4 -s, ...
samples over the pixels spt_adapt_select keeps, until none is left.  The film
is the Python loop's, the spp map its count, the paths printed their sum; with
--gpus above 1 the flag is refused."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sptamd
from sptamd import _lib, scenes
from test_gpu_pbrt import read_pfm

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(_lib.LIB_PATH), "spt_render_cli")
W, H, D = 40, 24, 4
RULE = dict(tolerance=0.1, min_spp=2, max_spp=16)


def test_cli_adaptive_equals_the_python_loop(tmp_path):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    out, spp_map, var = (str(tmp_path / n) for n in ("a.pfm", "spp.pfm", "var.pfm"))
    r = subprocess.run([CLI, "-w", str(W), "-h", str(H), "-d", str(D), obj, "-o", out, "-s", "2", "--adaptive", "0.1",
                        "--min-spp", "2", "--max-spp", "16", "--spp-map", spp_map, "--variance", var],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    s = sptamd.Scene()
    s.add_triangle_mesh(obj)
    s.commit(0)
    acc = s.accumulator(sptamd.make_params(W, H, 2, D))
    size, paths, passes = 2, 0, 0
    while acc.samples < RULE["max_spp"]:
        st = acc.add_adaptive(min(size, RULE["max_spp"] - acc.samples), **RULE)
        if st["active"] == 0:
            break
        paths += st["paths"]
        passes += 1
        size *= 2
    torch.cuda.synchronize()
    count = acc.count.cpu().numpy()
    assert passes >= 2 and count.min() >= 2 and count.max() <= 16 and count.min() < count.max()
    np.testing.assert_array_equal(read_pfm(out), acc.film.cpu().numpy())
    np.testing.assert_array_equal(read_pfm(var), acc.variance.cpu().numpy())
    m = read_pfm(spp_map)
    for c in range(3):
        np.testing.assert_array_equal(m[c], count.astype(np.float32))
    assert paths == int(count.sum())
    got = re.search(r"adaptive passes (\d+) samples up to (\d+) total paths (\d+)", r.stdout)
    assert got, r.stdout
    assert (int(got.group(1)), int(got.group(2)), int(got.group(3))) == (passes, acc.samples, paths)
    assert f"paths {paths} " in r.stdout


def test_cli_adaptive_composes_with_denoise_var(tmp_path):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    out = str(tmp_path / "d.pfm")
    r = subprocess.run([CLI, "-w", str(W), "-h", str(H), "-d", str(D), obj, "-o", out, "-s", "2", "--adaptive", "0.1",
                        "--min-spp", "2", "--max-spp", "8", "--denoise-var"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    raw, clean = read_pfm(out + ".raw.pfm"), read_pfm(out)
    assert raw.shape == clean.shape == (3, H, W) and np.isfinite(clean).all() and not np.array_equal(raw, clean)


@pytest.mark.parametrize("flags", [["--gpus", "2"], ["--passes", "2"]])
def test_cli_refuses_adaptive_with_several_gpus_or_passes(tmp_path, flags):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    r = subprocess.run([CLI, "-w", "8", "-h", "8", "-s", "1", "-d", "1", obj, "--adaptive", "0.1", "-o",
                        str(tmp_path / "x.pfm")] + flags, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode != 0 and "--adaptive" in r.stderr and "one device" in r.stderr
    assert not os.path.exists(tmp_path / "x.pfm")
