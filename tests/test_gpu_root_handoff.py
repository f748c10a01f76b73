"""The root hand-off (kernels.hip Tracer8T::root_visit / enter_root,
render_fused_kernel's kRoot; render_plan.h RenderPlan::root_handoff): the camera
cast that culls keeps the root visit it made for every surviving bounce ray and
writes its word beside the queue entry; the forced drain behind it starts each
queued ray below the BVH root instead of repeating the visit.  The state a lane
starts from is the one its first trace step would have left, so the same scene
and parameters rendered with the hand-off (the default), without it
(SPT_FLAG_NO_ROOT_HANDOFF) and without the cull (SPT_FLAG_NO_BOUNCE_CULL) must
give the same film bit for bit, and the first two the same device-counted work,
counter by counter.

Shapes (50 x 37 px, 3 spp, depth 4 on drain_q8 = 1, the smallest image known to
take the camera cast, test_gpu_bounce_cull.py): a mesh whose root has inner
children, against the oracle; two facing quads (every bounce ray hits a leaf
child of the root: the word carries triangle bits and the root's triangle base
matters); the closed box (mixed children, nothing culled, every survivor handed
off); the ground quad from above (every survivor culled: nothing to hand off);
max_depth 1 and 2 (at 2 the handed-off cast is the any-hit last cast); two
tiles; sample chunks; 80-byte nodes (bvh_width = 8); a sorted drain (the
hand-off must be off); an empty scene; one adaptive list pass (handed off: the
list changes the camera rays only, the drain behind the cast is the same)."""
import numpy as np
import pytest
import torch

import oracle as O
import sptamd
from conftest import assert_work_complete
from sptamd import _lib, scenes
from test_gpu_adaptive import PLANES, SparseBuffers, list_pass
from test_gpu_bounce_cull import camera, closed_box, ground_quad, quads_mesh, unit_scene

pytestmark = pytest.mark.gpu
W, H, SPP, D = 50, 37, 3, 4
F = np.float32
NO_ROOT, NO_CULL = _lib.SPT_FLAG_NO_ROOT_HANDOFF, _lib.SPT_FLAG_NO_BOUNCE_CULL
COUNTERS = ("ray_casts", "continuations", "drained_paths", "drained_casts", "culled_paths", "lockstep_casts")
SAME = COUNTERS + ("paths_started", "paths_terminated", "paths", "streams", "paths_in_flight", "fused", "drain_launches")


def facing_quads():
    """A floor and a ceiling of two triangles each, normals toward each other."""
    return quads_mesh([((-8.0, -1.0, 8.0), (16.0, 0.0, 0.0), (0.0, 0.0, -16.0), (0, 1, 0)),
                       ((-8.0, 1.0, 8.0), (16.0, 0.0, 0.0), (0.0, 0.0, -16.0), (0, -1, 0))])


@pytest.fixture(scope="module")
def mitsuba():
    return scenes.mitsuba_synth(detail=0.25)


def root_drains():
    """Drains this process has queued as the instance that starts below the root (spt.h test hook)."""
    return int(_lib.lib.spt_debug_root_drain_launches())


def arms(scene, make):
    """The render with the hand-off, without it, and without the cull: (film, stats,
    drains queued as the below-the-root instance) each."""
    out = []
    for flags in (0, NO_ROOT, NO_CULL):
        p = make()
        p.flags |= flags
        before = root_drains()
        film, st = scene.render(p, stream=torch.cuda.Stream())
        torch.cuda.synchronize()
        out.append((film.cpu().numpy(), st, root_drains() - before))
    return out


def check(scene, make, rows=H, spp=SPP, handed=None):
    """handed: whether the default arm must (True) or must not (False) have taken the
    hand-off; the film and the counters cannot tell, the launch count does."""
    on, off, uncut = arms(scene, make)
    print({k: (on[1][k], off[1][k], uncut[1][k]) for k in COUNTERS}, "root drains", on[2], off[2], uncut[2])
    assert off[2] == 0 and uncut[2] == 0
    if handed is not None:
        assert (on[2] > 0) == handed, on[2]
    assert on[0].tobytes() == off[0].tobytes()
    assert off[0].tobytes() == uncut[0].tobytes()
    for k in SAME:
        assert on[1][k] == off[1][k], (k, on[1][k], off[1][k])
    for _, st, _ in (on, off, uncut):
        assert_work_complete(st, rows, W, spp)
    return on, off, uncut


def wavefront(**kw):
    return lambda: sptamd.make_params(W, H, SPP, D, pipeline="wavefront", **kw)


def test_inner_children_and_oracle(mitsuba):
    s = unit_scene(mitsuba)
    on, _, _ = check(s, wavefront(), handed=True)
    assert on[1]["lockstep_casts"] == W * H * SPP  # the camera cast ran
    assert 0 < on[1]["culled_paths"] and on[1]["drained_paths"] > 0  # ... culled, and handed rays off
    ref, casts = O.OracleScene(mitsuba).render(O.reference_params(W, H, SPP, D))
    np.testing.assert_array_equal(on[0], ref)
    assert on[1]["ray_casts"] == casts


def test_facing_quads_leaf_children_of_the_root():
    """Four triangles: the root's children are leaves, so a bounce ray from the
    floor carries the ceiling's triangle bits over, and the drain's first step
    tests root_tri_base + their index."""
    mesh = facing_quads()
    s = unit_scene(mesh)
    cam = camera((0.0, 0.0, 0.0), (0.3, -1.0, -0.4), up=(0.0, 0.0, -1.0))
    on, _, _ = check(s, wavefront(camera=cam), handed=True)
    assert on[1]["lockstep_casts"] == W * H * SPP
    assert on[1]["drained_paths"] > 0 and on[1]["drained_casts"] > on[1]["drained_paths"]
    ref, casts = O.OracleScene(mesh).render(O.reference_params(W, H, SPP, D, camera=cam))
    np.testing.assert_array_equal(on[0], ref)
    assert on[1]["ray_casts"] == casts


def test_closed_box_every_survivor_handed_off():
    s = unit_scene(closed_box())
    cam = camera((0.1, 0.2, 0.3), (1.0, 0.5, -2.0))
    on, _, _ = check(s, wavefront(camera=cam), handed=True)
    assert on[1]["culled_paths"] == 0 and on[1]["lockstep_casts"] == W * H * SPP
    # every continuation is a cast the drain traced: the survivors' first casts there, then their bounces
    assert on[1]["drained_paths"] > 0 and on[1]["continuations"] == on[1]["drained_casts"]


def test_ground_quad_nothing_to_hand_off():
    s = unit_scene(ground_quad())
    cam = camera((0.0, 6.0, 0.5), (0.0, -1.0, 0.0))
    on, _, _ = check(s, wavefront(camera=cam))
    assert on[1]["culled_paths"] > 0 and on[1]["drained_paths"] == 0 and on[1]["drained_casts"] == 0


@pytest.mark.parametrize("depth", [1, 2])
def test_shallow_paths(mitsuba, depth):
    s = unit_scene(mitsuba)
    on, _, _ = check(s, lambda: sptamd.make_params(W, H, SPP, depth, pipeline="wavefront"), handed=True if depth == 2 else None)
    if depth == 1:
        assert on[1]["ray_casts"] == W * H * SPP and on[1]["drained_paths"] == 0
    else:  # every handed-off cast is the path's last: one any-hit cast each
        assert on[1]["drained_casts"] == on[1]["drained_paths"] > 0


def test_two_tiles(mitsuba):
    s = unit_scene(mitsuba)
    for tile in (0, 1):
        rows = _lib.tile_row_count(H, tile, 2, 1)
        check(s, wavefront(tile_index=tile, tile_count=2, rows_per_group=1), rows=rows, handed=True)


def test_sample_chunks(mitsuba):
    spp = 5
    s = unit_scene(mitsuba, fit_paths=W * H * 2)
    on, _, _ = check(s, lambda: sptamd.make_params(W, H, spp, D, pipeline="wavefront"), spp=spp, handed=True)
    assert on[1]["paths_in_flight"] == W * H * 2 and on[1]["drain_launches"] >= 3


def test_wide_nodes(mitsuba):
    """bvh_width = 8: the 80-byte node's root words (group and triangle base in w1.x / w1.y)."""
    s = unit_scene(mitsuba, bvh_width=8)
    on, _, _ = check(s, wavefront(), handed=True)
    assert on[1]["lockstep_casts"] == W * H * SPP and on[1]["drained_paths"] > 0
    ref, _ = O.OracleScene(mitsuba).render(O.reference_params(W, H, SPP, D))
    np.testing.assert_array_equal(on[0], ref)


def test_wide_nodes_leaf_children():
    s = unit_scene(facing_quads(), bvh_width=8)
    cam = camera((0.0, 0.0, 0.0), (0.3, -1.0, -0.4), up=(0.0, 0.0, -1.0))
    on, _, _ = check(s, wavefront(camera=cam), handed=True)
    assert on[1]["drained_paths"] > 0


def test_sorted_drain_keeps_the_root_start(mitsuba):
    """drain_sort = 1: the camera cast is not sharded and the drain takes a
    permutation, so nothing is handed off; the result is the same."""
    plain, _, _ = check(unit_scene(mitsuba), wavefront(), handed=True)
    on, _, _ = check(unit_scene(mitsuba, drain_sort=1), wavefront(), handed=False)
    assert on[0].tobytes() == plain[0].tobytes()
    assert on[1]["ray_casts"] == plain[1]["ray_casts"]


def test_empty_scene():
    s = unit_scene({"pos": np.zeros((0, 3), F), "pos_tri": np.zeros((0, 3), np.int32)})
    on, _, _ = check(s, wavefront(), handed=False)  # no root to visit: the cull is off
    assert on[1]["ray_casts"] == W * H * SPP and on[1]["culled_paths"] == 0


def test_adaptive_list_pass(mitsuba):
    """spt_render_accum_list over every other pixel: the kList camera cast culls
    and hands off like the full one (the drain it feeds is the same kernel)."""
    s = unit_scene(mitsuba)
    px = np.arange(0, W * H, 2)
    got = []
    for flags in (0, NO_ROOT, NO_CULL):
        p = sptamd.make_params(W, H, SPP, D, pipeline="wavefront")
        p.flags |= flags
        bufs = SparseBuffers(W * H)
        before = root_drains()
        rc, st = list_pass(s, p, SPP, bufs, 0, px)
        assert rc == 0, _lib.lib.spt_last_error()
        got.append(({k: bufs.bits(k).tobytes() for k in PLANES}, st, root_drains() - before))
    (f_on, s_on, n_on), (f_off, s_off, n_off), (f_uncut, _, n_uncut) = got
    assert n_on > 0 and n_off == 0 and n_uncut == 0  # the list pass is handed off
    print({k: (s_on[k], s_off[k]) for k in COUNTERS})
    assert f_on == f_off and f_off == f_uncut
    for k in SAME:
        assert s_on[k] == s_off[k], (k, s_on[k], s_off[k])
    assert s_on["paths_started"] == s_on["paths_terminated"] == len(px) * SPP and s_on["film_slots_unwritten"] == 0
    assert s_on["lockstep_casts"] == len(px) * SPP and s_on["culled_paths"] > 0 and s_on["drained_paths"] > 0
