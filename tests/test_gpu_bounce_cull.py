"""The camera cast's bounce cull (kernels.hip shade_block's CullTr,
Tracer8T::root_misses; render_plan.h RenderPlan::bounce_cull): a bounce ray that
misses every child of the BVH root ends in the camera-cast kernel instead of in
the drain.  The cull is the drain's own first trace step made early, so the
same scene and parameters rendered with it (the default) and without it
(SPT_FLAG_NO_BOUNCE_CULL) must give the same film bit for bit and the same
device-counted work; the culled paths are exactly the ones the drain no longer
sees.

Shapes: an item count that is no multiple of the 128-thread block (partly
invalid blocks); a ground quad seen from above (every survivor culled: the
drain gets an empty sharded queue); the camera inside a closed box (nothing
culled); a two-tile job; max_depth 1 (no bounce) and 2 (the bounce is the last,
any-hit cast); an empty scene; albedo and emitter-with-spheres scenes (left
uncut: culled == 0); a job in sample chunks (several camera casts and drains).
drain_q8 = 1 makes the drain threshold small enough for these images to take
the camera cast (test_gpu_drain.py)."""
import numpy as np
import pytest
import torch

import oracle as O
import sptamd
from conftest import assert_work_complete
from sptamd import _lib, scenes
from test_gpu_drain import gpu_scene, materials

pytestmark = pytest.mark.gpu
W, H, SPP, D = 50, 37, 3, 4
F = np.float32
SAME = ("ray_casts", "continuations", "paths_started", "paths_terminated", "paths", "lockstep_casts", "streams",
        "paths_in_flight", "fused")


def quads_mesh(quads, n=1):
    """Quads (corner, eu, ev, normal) as n x n grids of two triangles each."""
    b = scenes._Builder()
    for corner, eu, ev, normal in quads:
        p, nr, t = scenes._quad_grid(corner, eu, ev, n, n, normal)
        b.add(p, nr, t, np.zeros_like(t), 0)
    return b.mesh()


def ground_quad():
    return quads_mesh([((-50.0, -1.0, 50.0), (100.0, 0.0, 0.0), (0.0, 0.0, -100.0), (0, 1, 0))])


def closed_box():
    """The cube [-2, 2]^3, normals inward, each wall a 2 x 2 grid (the camera sits at its centre)."""
    a, e = 2.0, 4.0
    return quads_mesh([((-a, -a, a), (e, 0, 0), (0, 0, -e), (0, 1, 0)), ((-a, a, a), (e, 0, 0), (0, 0, -e), (0, -1, 0)),
                       ((-a, -a, a), (0, e, 0), (0, 0, -e), (1, 0, 0)), ((a, -a, a), (0, e, 0), (0, 0, -e), (-1, 0, 0)),
                       ((-a, -a, -a), (e, 0, 0), (0, e, 0), (0, 0, 1)), ((-a, -a, a), (e, 0, 0), (0, e, 0), (0, 0, -1))],
                      n=2)


def camera(look_from, look_at, up=(0.0, 1.0, 0.0)):
    c = sptamd.reference_camera()
    c.update(look_from=look_from, look_at=look_at, up=up)
    return c


@pytest.fixture(scope="module")
def mitsuba():
    return scenes.mitsuba_synth(detail=0.25)


def both_arms(scene, make):
    """The render with the cull (the default) and without it: (film, stats) each."""
    out = []
    for flags in (0, _lib.SPT_FLAG_NO_BOUNCE_CULL):
        p = make()
        p.flags |= flags
        film, st = scene.render(p, stream=torch.cuda.Stream())
        torch.cuda.synchronize()
        out.append((film.cpu().numpy(), st))
    return out


def check_arms(on, off, rows, spp, width=W):
    (f_on, s_on), (f_off, s_off) = on, off
    print({k: (s_on[k], s_off[k]) for k in ("ray_casts", "continuations", "drained_paths", "drained_casts",
                                            "culled_paths", "lockstep_casts")})
    assert f_on.tobytes() == f_off.tobytes()
    for k in SAME:
        assert s_on[k] == s_off[k], (k, s_on[k], s_off[k])
    for st in (s_on, s_off):
        assert_work_complete(st, rows, width, spp)
    assert s_off["culled_paths"] == 0
    culled = s_on["culled_paths"]
    assert s_on["drained_paths"] + culled == s_off["drained_paths"]
    assert s_on["drained_casts"] + culled == s_off["drained_casts"]
    # where the camera cast ran, it and the drain traced every cast
    if s_off["lockstep_casts"] == rows * width * spp:
        assert s_on["ray_casts"] - s_on["drained_casts"] == s_on["lockstep_casts"] + culled
    return culled


def unit_scene(mesh, **knobs):
    return gpu_scene(mesh, {}, drain_q8=1, drain_casts=1, **knobs)


def test_odd_item_count_and_oracle(mitsuba):
    """50 x 37 x 3 = 5550 paths: 43 full blocks and one of 46 valid lanes."""
    s = unit_scene(mitsuba)
    on, off = both_arms(s, lambda: sptamd.make_params(W, H, SPP, D, pipeline="wavefront"))
    check_arms(on, off, H, SPP)
    assert on[1]["lockstep_casts"] == W * H * SPP  # the camera cast ran
    ref, casts = O.OracleScene(mitsuba).render(O.reference_params(W, H, SPP, D))
    np.testing.assert_array_equal(on[0], ref)
    assert on[1]["ray_casts"] == casts


def test_ground_quad_every_survivor_culled():
    """Every camera ray that hits the quad bounces upward out of the root's flat
    children: all culled, the drain's sharded queue is empty (eight segments of 0)."""
    s = unit_scene(ground_quad())
    cam = camera((0.0, 6.0, 0.5), (0.0, -1.0, 0.0))
    on, off = both_arms(s, lambda: sptamd.make_params(W, H, SPP, D, camera=cam, pipeline="wavefront"))
    culled = check_arms(on, off, H, SPP)
    assert on[1]["lockstep_casts"] == W * H * SPP
    assert culled > 0 and culled == on[1]["continuations"]
    assert on[1]["drained_paths"] == 0 and on[1]["drained_casts"] == 0
    assert on[1]["ray_casts"] == W * H * SPP + culled


def test_camera_in_closed_box_nothing_culled():
    """Every bounce ray meets another wall's box: nothing is culled."""
    s = unit_scene(closed_box())
    cam = camera((0.1, 0.2, 0.3), (1.0, 0.5, -2.0))
    on, off = both_arms(s, lambda: sptamd.make_params(W, H, SPP, D, camera=cam, pipeline="wavefront"))
    assert check_arms(on, off, H, SPP) == 0
    assert on[1]["lockstep_casts"] == W * H * SPP and on[1]["continuations"] > 0


def test_two_tiles(mitsuba):
    s = unit_scene(mitsuba)
    for tile in (0, 1):
        rows = _lib.tile_row_count(H, tile, 2, 1)
        on, off = both_arms(s, lambda: sptamd.make_params(W, H, SPP, D, tile_index=tile, tile_count=2,
                                                          rows_per_group=1, pipeline="wavefront"))
        check_arms(on, off, rows, SPP)


@pytest.mark.parametrize("depth", [1, 2])
def test_shallow_paths(mitsuba, depth):
    """max_depth 1: the camera cast is the last cast, nothing bounces; 2: the
    bounce is the path's last cast (an any-hit query in the drain)."""
    s = unit_scene(mitsuba)
    on, off = both_arms(s, lambda: sptamd.make_params(W, H, SPP, depth, pipeline="wavefront"))
    culled = check_arms(on, off, H, SPP)
    if depth == 1:
        assert culled == 0 and on[1]["ray_casts"] == W * H * SPP


def test_empty_scene():
    s = unit_scene({"pos": np.zeros((0, 3), F), "pos_tri": np.zeros((0, 3), np.int32)})
    on, off = both_arms(s, lambda: sptamd.make_params(W, H, SPP, D, pipeline="wavefront"))
    assert check_arms(on, off, H, SPP) == 0
    assert on[1]["ray_casts"] == W * H * SPP


@pytest.mark.parametrize("mode", ["albedo", "emit_spheres"])
def test_other_modes_left_uncut(mitsuba, mode):
    """Albedo / emitter instances keep their kernels; with analytic spheres
    (tested after the BVH) the cull must be off."""
    s = gpu_scene(mitsuba, materials(mitsuba, mode), drain_q8=1, drain_casts=1)
    kw = dict(rr_start_depth=3, env=(1.0, 0.9, 0.8))
    on, off = both_arms(s, lambda: sptamd.make_params(W, H, SPP, D, pipeline="wavefront", **kw))
    assert check_arms(on, off, H, SPP) == 0
    assert on[1]["lockstep_casts"] == W * H * SPP


def test_sample_chunks(mitsuba):
    """fit_paths of two samples: 5 samples run as chunks of 2, 2 and 1, each
    with a camera cast (where its queue is long enough) and a drain of its own."""
    spp = 5
    s = unit_scene(mitsuba, fit_paths=W * H * 2)
    on, off = both_arms(s, lambda: sptamd.make_params(W, H, spp, D, pipeline="wavefront"))
    check_arms(on, off, H, spp)
    assert on[1]["paths_in_flight"] == W * H * 2 and on[1]["lockstep_casts"] >= W * H * 4
    assert on[1]["drain_launches"] >= 3
