"""The camera entry table (csrc/camera_entry.h, camera_entry_kernel; render_plan.h
RenderPlan::camera_entry): the camera cast starts each pixel's rays at the node
their pixel's beam cannot avoid instead of at the BVH root.  Starting there is
culling the chain's siblings, which none of the pixel's rays would have entered,
so the same scene and parameters rendered with the table (the default) and
without it (SPT_FLAG_NO_CAMERA_ENTRY) must give the same film bit for bit and
the same device-counted work, counter by counter.

Cases: the mitsuba mesh under the reference camera in unit and albedo mode, and
smallpt's analytic spheres (tested after the BVH: unaffected); every hostile
family; two tiles; sample-major work; a list render; a thin lens (no table);
a refit between two renders (a second table) and two renders of one view (one
table); the table itself — at least a quarter of the mitsuba image's pixels
enter below the root, and every non-zero word names an inner child of a node
of the device tree.  drain_q8 = 1 makes the drain threshold small enough for
these images to take the camera cast (test_gpu_drain.py)."""
import ctypes

import numpy as np
import pytest
import torch

import bvh_audit as A
import hostile
import sptamd
from conftest import assert_work_complete
from sptamd import _lib, scenes
from test_gpu_adaptive import PLANES, SparseBuffers, list_pass
from test_gpu_drain import gpu_scene, materials

pytestmark = pytest.mark.gpu
W, H, SPP, D = 64, 64, 8, 4
NO_ENTRY = _lib.SPT_FLAG_NO_CAMERA_ENTRY
COUNTERS = ("ray_casts", "continuations", "culled_paths", "drained_paths", "drained_casts", "lockstep_casts")
SAME = COUNTERS + ("paths_started", "paths_terminated", "paths", "streams", "paths_in_flight", "fused", "drain_launches")


def builds():
    """Entry tables this process has built (spt.h test hook)."""
    return int(_lib.lib.spt_debug_entry_builds())


def table(scene):
    """The entry table the scene's last render used (empty: none)."""
    n = ctypes.c_uint32(0)
    assert _lib.lib.spt_debug_entry_table(scene.backend.handle, None, 0, ctypes.byref(n)) == 0
    out = np.zeros(n.value, np.uint32)
    if n.value:
        assert _lib.lib.spt_debug_entry_table(scene.backend.handle, out.ctypes.data, n.value, ctypes.byref(n)) == 0
    return out


def render(scene, p, stream):
    before = builds()
    film, st = scene.render(p, stream=stream)
    torch.cuda.synchronize()
    return film.cpu().numpy(), st, builds() - before


def both(scene, make, stream=None):
    """The render with the table (the default) and without it: (film, stats, tables built) each."""
    stream = stream or torch.cuda.Stream()
    out = []
    for flags in (0, NO_ENTRY):
        p = make()
        p.flags |= flags
        out.append(render(scene, p, stream))
    return out


def check(scene, make, rows=H, width=W, spp=SPP, built=None, stream=None):
    on, off = both(scene, make, stream)
    print({k: (on[1][k], off[1][k]) for k in COUNTERS}, "tables built", on[2], off[2])
    assert off[2] == 0
    if built is not None:
        assert on[2] == built, on[2]
    assert on[0].tobytes() == off[0].tobytes()
    for k in SAME:
        assert on[1][k] == off[1][k], (k, on[1][k], off[1][k])
    for _, st, _ in (on, off):
        assert_work_complete(st, rows, width, spp)
    return on, off


def unit_scene(mesh, **knobs):
    return gpu_scene(mesh, {}, drain_q8=1, drain_casts=1, **knobs)


def wavefront(w=W, h=H, spp=SPP, **kw):
    return lambda: sptamd.make_params(w, h, spp, D, pipeline="wavefront", **kw)


@pytest.fixture(scope="module")
def mitsuba():
    return scenes.mitsuba_synth(detail=0.25)


@pytest.fixture(scope="module")
def mitsuba_scene(mitsuba):
    return unit_scene(mitsuba)


def test_unit_mode_and_the_table(mitsuba, tmp_path):
    s = unit_scene(mitsuba)
    on, _ = check(s, wavefront(), built=1)
    assert on[1]["lockstep_casts"] == W * H * SPP  # the camera cast ran
    # the table of the flag-clear render (the flag-set one that followed used none)
    p = wavefront()()
    _, _, again = render(s, p, torch.cuda.Stream())
    t = table(s)
    assert len(t) == W * H
    below = float((t != 0).mean())
    print(f"mitsuba_synth {W} x {H}: {below:.3f} of the pixels enter below the root "
          f"(deepest word slot {int((t >> 24).max())}, {len(np.unique(t))} distinct words)")
    assert below >= 0.25, f"{below:.3f} of the pixels enter below the root"
    # every non-zero word names an existing inner child of an existing node of the device tree
    path = tmp_path / "scene.sptc"
    s.save(str(path))
    tree = A.parse(str(path))
    assert tree.fmt == 6
    d = A._decode_wide(tree, np.arange(tree.nodes.shape[0]), A._Report())
    inner = d["kid"] >= 0
    group = (tree.nodes[:, 6] & 0x00ffffff).astype(np.uint64)
    words = ((d["meta"][inner] & 7).astype(np.uint64) << 24) | np.repeat(group[:, None], d["K"], 1)[inner]
    kids = d["kid"][inner]
    assert ((kids > 0) & (kids < tree.nodes.shape[0])).all()
    assert (t >> 27 == 0).all()
    nz = np.unique(t[t != 0]).astype(np.uint64)
    assert np.isin(nz, words).all(), [hex(int(x)) for x in nz[~np.isin(nz, words)][:8]]
    # ... and an inner node (it has children of its own): the entry is never a leaf
    kid_of = dict(zip(words.tolist(), kids.tolist()))
    live = d["live"]
    assert all(live[kid_of[int(x)]].any() for x in nz)


def test_albedo_mode(mitsuba):
    s = gpu_scene(mitsuba, materials(mitsuba, "albedo"), drain_q8=1, drain_casts=1)
    on, _ = check(s, wavefront(rr_start_depth=3, env=(1.0, 0.9, 0.8)), built=1)
    assert on[1]["lockstep_casts"] == W * H * SPP


def test_smallpt_analytic_spheres():
    m = scenes.smallpt_analytic(detail=0.5)
    alb, emi = scenes.smallpt_materials(m)
    s = gpu_scene(m, {"albedo": alb, "emission": emi}, drain_q8=1, drain_casts=1)
    on, _ = check(s, wavefront(camera=scenes.cornell_camera(), rr_start_depth=3, env=(0.0, 0.0, 0.0)), built=1)
    assert on[1]["lockstep_casts"] == W * H * SPP and on[0].max() > 0


@pytest.mark.parametrize("name", hostile.FAMILIES)
def test_hostile_families(name):
    w = h = 48
    s = unit_scene(hostile.family(name))
    on, _ = check(s, wavefront(w, h, 4, camera=hostile.camera(name)), rows=h, width=w, spp=4, built=1)
    assert on[1]["lockstep_casts"] == w * h * 4
    t = table(s)   # the last render had the flag set: no table
    assert len(t) == 0


def test_two_tiles(mitsuba_scene):
    for tile in (0, 1):
        rows = _lib.tile_row_count(H, tile, 2, 8)
        on, _ = check(mitsuba_scene, wavefront(tile_index=tile, tile_count=2, rows_per_group=8), rows=rows, built=1)
        assert on[1]["lockstep_casts"] == rows * W * SPP


def test_sample_major(mitsuba):
    s = unit_scene(mitsuba, work_order=_lib.SPT_WORK_SAMPLE_MAJOR)
    on, _ = check(s, wavefront(), built=1)
    assert on[1]["lockstep_casts"] == W * H * SPP and on[1]["work_order"] == _lib.SPT_WORK_SAMPLE_MAJOR


def test_list_render(mitsuba_scene):
    """spt_render_accum_list over every other pixel: the kList camera cast reads the same table."""
    s = mitsuba_scene
    px = np.arange(0, W * H, 2)
    got = []
    for flags in (0, NO_ENTRY):
        p = wavefront()()
        p.flags |= flags
        bufs = SparseBuffers(W * H)
        before = builds()
        rc, st = list_pass(s, p, SPP, bufs, 0, px)
        assert rc == 0, _lib.lib.spt_last_error()
        got.append(({k: bufs.bits(k).tobytes() for k in PLANES}, st, builds() - before))
    (f_on, s_on, n_on), (f_off, s_off, n_off) = got
    print({k: (s_on[k], s_off[k]) for k in COUNTERS}, "tables built", n_on, n_off)
    assert n_on <= 1 and n_off == 0   # (0: the set still holds this view's table)
    assert f_on == f_off
    for k in SAME:
        assert s_on[k] == s_off[k], (k, s_on[k], s_off[k])
    assert s_on["lockstep_casts"] == len(px) * SPP and s_on["film_slots_unwritten"] == 0


def test_thin_lens_builds_no_table(mitsuba_scene):
    cam = sptamd.reference_camera()
    cam.update(lens_radius=0.05, focal_dist=5.0)
    on, off = check(mitsuba_scene, wavefront(camera=cam), built=0)
    assert on[1]["lockstep_casts"] == W * H * SPP
    assert len(table(mitsuba_scene)) == 0


def test_one_view_builds_once_and_a_refit_builds_again(mitsuba):
    s = unit_scene(mitsuba)
    stream = torch.cuda.Stream()
    first = render(s, wavefront()(), stream)
    second = render(s, wavefront()(), stream)
    assert first[2] == 1 and second[2] == 0      # two renders of one view: exactly one table
    assert first[0].tobytes() == second[0].tobytes()
    t0 = table(s)
    # another view of the same scene: a new table; back again: one more (a set keeps one)
    cam = sptamd.reference_camera()
    cam.update(look_from=(1.0, 2.5, 4.5))
    assert render(s, wavefront(camera=cam)(), stream)[2] == 1
    assert render(s, wavefront()(), stream)[2] == 1
    assert np.array_equal(table(s), t0)
    # the geometry moves under the same arrays: the next render of the same view builds again
    rng = np.random.default_rng(5)
    pos = np.asarray(mitsuba["pos"], np.float32)
    moved = (pos * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=pos.shape))).astype(np.float32)
    s.update_geometry(moved)
    on = render(s, wavefront()(), stream)
    assert on[2] == 1
    p = wavefront()()
    p.flags |= NO_ENTRY
    off = render(s, p, stream)
    assert off[2] == 0
    assert on[0].tobytes() == off[0].tobytes() and on[0].tobytes() != first[0].tobytes()
    for k in SAME:
        assert on[1][k] == off[1][k], (k, on[1][k], off[1][k])
