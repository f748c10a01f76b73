"""spt_render_cli --aov / --denoise (csrc/main.cpp): the feature buffers and the
denoised image the C++ host writes are, bit for bit, the Python API's planes
and denoised film; with --gpus above 1 both flags are refused."""
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
W, H, SPP, D = 40, 24, 3, 4


def test_cli_aov_and_denoise_equal_the_python_api(tmp_path):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    out, prefix = str(tmp_path / "img.pfm"), str(tmp_path / "feat")
    r = subprocess.run([CLI, "-w", str(W), "-h", str(H), "-s", str(SPP), "-d", str(D), obj, "-o", out, "--aov", prefix,
                        "--denoise"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    s = sptamd.Scene()
    s.add_triangle_mesh(obj)
    s.commit(0)
    p = sptamd.make_params(W, H, SPP, D)
    film, _ = s.render(p)
    aov = s.render_aov(p)
    clean = sptamd.denoise(film, aov)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(read_pfm(out + ".raw.pfm"), film.cpu().numpy())
    np.testing.assert_array_equal(read_pfm(prefix + ".albedo.pfm"), aov["albedo"].cpu().numpy())
    np.testing.assert_array_equal(read_pfm(prefix + ".normal.pfm"), aov["normal"].cpu().numpy())
    for name in ("depth", "coverage"):
        img = read_pfm(f"{prefix}.{name}.pfm")
        for c in range(3):
            np.testing.assert_array_equal(img[c], aov[name].cpu().numpy(), err_msg=name)
    np.testing.assert_array_equal(read_pfm(out), clean.cpu().numpy())
    cov = aov["coverage"].cpu().numpy()
    assert 0 < cov.mean() < 1                       # the buffers show surfaces and sky
    assert not np.array_equal(read_pfm(out), film.cpu().numpy())


@pytest.mark.parametrize("flags", [["--aov", "x"], ["--denoise"]])
def test_cli_refuses_aov_with_several_gpus(tmp_path, flags):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    r = subprocess.run([CLI, "-w", "8", "-h", "8", "-s", "1", "-d", "1", obj, "--gpus", "2", "-o",
                        str(tmp_path / "x.pfm")] + flags, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode != 0 and "--gpus" in r.stderr and "one device" in r.stderr
    assert not os.path.exists(tmp_path / "x.pfm") and not os.path.exists(tmp_path / "x.albedo.pfm")
