"""spt_render_cli --frames / --orbit-deg / --temporal (csrc/main.cpp): the frames
it writes are the Python TemporalAccumulator's bit for bit, frames without
--temporal are independent renders of their views, and without --frames the
flags change nothing."""
import math
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
W, H, D, SPP = 40, 24, 4, 4


def run(obj, out, *flags, ok=True):
    r = subprocess.run([CLI, "-w", str(W), "-h", str(H), "-d", str(D), "-s", str(SPP), obj, "-o", out] + list(flags),
                       capture_output=True, text=True, timeout=180)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


@pytest.fixture(scope="module")
def scene():
    s = sptamd.Scene()
    s.add_triangle_mesh(scenes.scene_obj("mitsuba_synth", 0.1))
    s.commit(0)
    return s


def orbit(camera, degrees):
    """The CLI's orbit: `camera` turned `degrees` about up through look_at, in f64, rounded once."""
    if degrees == 0:
        return camera
    f, a, u = (np.array([np.float32(x) for x in camera[k]], np.float64) for k in ("look_from", "look_at", "up"))
    u = u / math.sqrt(float((u * u).sum()))
    v, t = f - a, degrees * 3.14159265358979323846 / 180.0
    x = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
    uv = u[0] * v[0] + u[1] * v[1] + u[2] * v[2]
    r = a + (v * math.cos(t) + x * math.sin(t) + u * uv * (1.0 - math.cos(t)))
    return dict(camera, look_from=tuple(float(np.float32(c)) for c in r))


def test_temporal_frames_equal_the_python_accumulator(tmp_path, scene):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    out = str(tmp_path / "t.pfm")
    r = run(obj, out, "--frames", "3", "--orbit-deg", "0", "--temporal")
    assert f"paths {W * H * SPP * 3} " in r.stdout and "wrote 3 frames" in r.stdout
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith(".pfm"))
    assert files == ["t.000.pfm", "t.001.pfm", "t.002.pfm"]
    t = sptamd.TemporalAccumulator(scene, sptamd.make_params(W, H, SPP, D))
    for k in range(3):
        t.frame(SPP)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(read_pfm(str(tmp_path / f"t.{k:03d}.pfm")), t.film.cpu().numpy(), err_msg=str(k))
    # (all but the pixels that fail the default normal test on themselves: include/spt.h, Limits)
    assert float(t.length.max()) == 3 * SPP and float((t.length == 3 * SPP).float().mean()) > 0.9
    # the frames differ: each adds new samples
    assert not np.array_equal(read_pfm(str(tmp_path / "t.000.pfm")), read_pfm(str(tmp_path / "t.002.pfm")))


def test_temporal_orbit_max_history_and_denoise_var(tmp_path, scene):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    out = str(tmp_path / "o.pfm")
    run(obj, out, "--frames", "3", "--orbit-deg", "2", "--temporal", "--max-history", "6", "--denoise-var")
    base = sptamd.reference_camera()
    t = sptamd.TemporalAccumulator(scene, sptamd.make_params(W, H, SPP, D), max_history=6.0)
    for k in range(3):
        t.frame(SPP, camera=orbit(base, 2.0 * k))
        clean = sptamd.denoise_var(t.film, t.variance, t.aov)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(read_pfm(str(tmp_path / f"o.{k:03d}.raw.pfm")), t.film.cpu().numpy(), err_msg=str(k))
        np.testing.assert_array_equal(read_pfm(str(tmp_path / f"o.{k:03d}.pfm")), clean.cpu().numpy(), err_msg=str(k))
    assert float(t.length.max()) <= 6.0 + SPP and float(t.length.max()) > SPP


def test_frames_without_temporal_are_independent_renders(tmp_path, scene):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    out = str(tmp_path / "f.pfm")
    run(obj, out, "--frames", "3", "--orbit-deg", "5")
    base = sptamd.reference_camera()
    frames = []
    for k in range(3):
        film, _ = scene.render(sptamd.make_params(W, H, SPP, D, camera=orbit(base, 5.0 * k)))
        torch.cuda.synchronize()
        frames.append(read_pfm(str(tmp_path / f"f.{k:03d}.pfm")))
        np.testing.assert_array_equal(frames[-1], film.cpu().numpy(), err_msg=str(k))
    assert not np.array_equal(frames[0], frames[1])
    assert not os.path.exists(out)


def test_without_frames_nothing_changes(tmp_path, scene):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    out = str(tmp_path / "plain.pfm")
    r = run(obj, out)
    assert "writing image" in r.stdout and "done" in r.stdout
    film, _ = scene.render(sptamd.make_params(W, H, SPP, D))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(read_pfm(out), film.cpu().numpy())
    assert sorted(os.listdir(tmp_path)) == ["plain.pfm"]


@pytest.mark.parametrize("flags", [["--temporal"], ["--orbit-deg", "1"], ["--frames", "2", "--max-history", "8"],
                                   ["--frames", "2", "--passes", "2"], ["--frames", "2", "--denoise-var"],
                                   ["--frames", "2", "--temporal", "--max-history", "-1"], ["--frames", "-1"],
                                   ["--frames", "2", "--gpus", "2"]])
def test_cli_refuses_flags_that_do_not_go_together(tmp_path, flags):
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    r = run(obj, str(tmp_path / "x.pfm"), *flags, ok=False)
    assert "--frames" in r.stderr
    assert os.listdir(tmp_path) == []
