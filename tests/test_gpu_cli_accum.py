"""spt_render_cli --passes / --variance / --denoise-var (csrc/main.cpp): N passes
of s samples write the bytes of one render of N x s samples, the variance file
holds the Python accumulator's planes, the variance-guided filter's image is the
Python API's; with --gpus above 1 the flags are refused."""
import os
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


def run(obj, out, *flags):
    r = subprocess.run([CLI, "-w", str(W), "-h", str(H), "-d", str(D), obj, "-o", out] + list(flags),
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_cli_passes_variance_and_denoise_var_equal_the_python_api(tmp_path):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    one, four, var, den = (str(tmp_path / n) for n in ("one.pfm", "four.pfm", "var.pfm", "den.pfm"))
    run(obj, one, "-s", "8")
    r = run(obj, four, "-s", "2", "--passes", "4", "--variance", var)
    assert f"paths {W * H * 8} " in r.stdout
    with open(one, "rb") as a, open(four, "rb") as b:
        assert a.read() == b.read()
    run(obj, den, "-s", "2", "--passes", "4", "--denoise-var")
    s = sptamd.Scene()
    s.add_triangle_mesh(obj)
    s.commit(0)
    p = sptamd.make_params(W, H, 8, D)
    acc = s.accumulator(p)
    for _ in range(4):
        acc.add(2)
    aov = s.render_aov(p)
    clean = sptamd.denoise_var(acc.film, acc.variance, aov)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(read_pfm(four), acc.film.cpu().numpy())
    np.testing.assert_array_equal(read_pfm(var), acc.variance.cpu().numpy())
    assert (acc.variance > 0).any()
    np.testing.assert_array_equal(read_pfm(den + ".raw.pfm"), acc.film.cpu().numpy())
    np.testing.assert_array_equal(read_pfm(den), clean.cpu().numpy())
    assert not np.array_equal(read_pfm(den), read_pfm(four))


@pytest.mark.parametrize("flags", [["--passes", "2"], ["--variance", "v.pfm"], ["--denoise-var"]])
def test_cli_refuses_accumulation_with_several_gpus(tmp_path, flags):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    r = subprocess.run([CLI, "-w", "8", "-h", "8", "-s", "1", "-d", "1", obj, "--gpus", "2", "-o",
                        str(tmp_path / "x.pfm")] + flags, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode != 0 and "--gpus" in r.stderr and "one device" in r.stderr
    assert not os.path.exists(tmp_path / "x.pfm") and not os.path.exists(tmp_path / "v.pfm")
