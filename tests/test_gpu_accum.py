"""spt_render_accum (include/spt.h) on the GPU: any split of N samples into
passes gives one pass's sum, sum of squares, film and variance bit for bit, in
every pipeline, work order and film chunking; that film is spt_render's and
the oracle's; the sums and the variance are the CPU restatement's
(tests/accum_ref.py over the oracle's per-sample contributions); optional
planes, guard words, refusals, stats, queued passes, and the jump table's
growth leaving spt_render and spt_render_aov as they were."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import accum_ref as A
import aov_ref
import oracle as O
import sptamd
from sptamd import _lib, scenes
from test_accum_ref import mode_scene

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 37, 19, 8, 4
KW = dict(rr_start_depth=2, env=(0.3, 0.7, 1.0))
PLANES = ("sum", "sum_sq", "film", "variance")


def make_scene(mode, cfg=None, mesh=None):
    m, albedo, emi = mode_scene(mode, mesh)
    s = sptamd.Scene(config=cfg)
    s.add_arrays(m)
    s.commit(0)
    if albedo is not None:
        s.backend.set_albedo(albedo)
    if emi is not None:
        s.backend.set_emission(emi)
    return s


@functools.lru_cache(maxsize=None)
def oracle_scene(mode):
    m, albedo, emi = mode_scene(mode)
    return O.OracleScene(m, albedo=albedo, emission=emi)


@functools.lru_cache(maxsize=None)
def oracle_film(mode, w, h, spp, depth):
    return oracle_scene(mode).render(O.reference_params(w, h, spp, depth, **KW))


def accumulate(scene, params, split, moments=True, stream=None):
    """The four planes (host arrays) after passes of split[0], split[1], ... samples, and the passes' stats."""
    acc = scene.accumulator(params, moments=moments)
    stats = [acc.add(n, stream=stream) for n in split]
    torch.cuda.synchronize()
    assert acc.samples == sum(split)
    out = {k: getattr(acc, k).cpu().numpy() for k in PLANES if getattr(acc, k) is not None}
    return out, stats


def assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what} {k}")


def pipeline_params(pipeline, cfg, **kw):
    """wavefront: a job that fits in flight (camera cast, drain); queued: the
    per-cast wavefront over short queues with the drain; percast: without it."""
    if pipeline == "percast":
        cfg.drain_q8 = 0
    flag = "fused" if pipeline == "fused" else "wavefront"
    wp = 0 if pipeline in ("wavefront", "fused") else 1500
    return sptamd.make_params(W, H, SPP, DEPTH, pipeline=flag, wavefront_paths=wp, **KW, **kw)


SPLITS = [[8], [4, 4], [3, 5], [1] * 8]


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("pipeline", ["wavefront", "queued", "fused", "percast"])
def test_splits_bitexact(pipeline, order):
    cfg = sptamd.default_config()
    cfg.work_order = order
    p = pipeline_params(pipeline, cfg)
    s = make_scene("albedo", cfg)
    whole, stats = accumulate(s, p, SPLITS[0])
    assert stats[0]["work_order"] == order and stats[0]["fused"] == (pipeline == "fused")
    if pipeline == "percast":
        assert stats[0]["drain_launches"] == 0
    for split in SPLITS[1:]:
        got, _ = accumulate(s, p, split)
        assert_same(got, whole, f"{pipeline} order {order} split {split}")
    film, st = s.render(p)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(whole["film"], film.cpu().numpy())
    ref, casts = oracle_film("albedo", W, H, SPP, DEPTH)
    np.testing.assert_array_equal(whole["film"], ref)
    assert (whole["variance"] > 0).any() and np.isfinite(whole["variance"]).all()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("mode", ["unit", "albedo", "emit"])
@pytest.mark.parametrize("pipeline", ["queued", "fused"])
def test_splits_with_two_film_chunks_per_pass(pipeline, mode, order):
    """film_budget_bytes of four samples: the 8-sample pass takes two internal
    chunks, the 5-sample pass a chunk of 4 and one of 1."""
    cfg = sptamd.default_config()
    cfg.work_order = order
    cfg.film_budget_bytes = (1 if mode == "unit" else 12) * W * H * 4
    p = pipeline_params(pipeline, cfg)
    s = make_scene(mode, cfg)
    whole, _ = accumulate(s, p, [8])
    for split in SPLITS[1:]:
        got, _ = accumulate(s, p, split)
        assert_same(got, whole, f"{mode} {pipeline} split {split}")
    # and the unchunked pass gives the same
    s2 = make_scene(mode)
    one, _ = accumulate(s2, pipeline_params(pipeline, sptamd.default_config()), [8])
    assert_same(one, whole, "chunked vs unchunked")
    ref, _ = oracle_film(mode, W, H, SPP, DEPTH)
    np.testing.assert_array_equal(whole["film"], ref)
    film, _ = s.render(p)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(whole["film"], film.cpu().numpy())


@pytest.mark.parametrize("pipeline", ["wavefront", "fused"])
def test_unit_mode_pixel_major_vector_path_and_tail(pipeline):
    """19 samples as [16, 3] in unit mode, pixel-major: the 16-flag reads of the
    flag resolve, then its byte tail; [19] takes the byte loop alone."""
    cfg = sptamd.default_config()
    cfg.work_order = 2
    s = make_scene("unit", cfg)
    p = sptamd.make_params(W, H, 19, DEPTH, pipeline=pipeline, **KW)
    whole, _ = accumulate(s, p, [19])
    for split in ([16, 3], [3, 16], [16, 1, 1, 1]):
        got, _ = accumulate(s, p, split)
        assert_same(got, whole, f"split {split}")
    ref, _ = oracle_film("unit", W, H, 19, DEPTH)
    np.testing.assert_array_equal(whole["film"], ref)
    film, _ = s.render(p)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(whole["film"], film.cpu().numpy())
    # env^2 per escape: sum_sq is sum x env, channel by channel, while a pixel's sum stays small
    assert (whole["sum_sq"][2] == whole["sum"][2]).all()     # env_b = 1
    assert (whole["variance"] > 0).any()


@pytest.mark.parametrize("mode", ["unit", "albedo"])
def test_interleaved_tile(mode):
    """Rank 1 of 3 with 4-row groups: rows 4..7 and 16..18 of the 19."""
    s = make_scene(mode)
    tile = dict(tile_index=1, tile_count=3, rows_per_group=4)
    p = sptamd.make_params(W, H, SPP, DEPTH, pipeline="wavefront", **KW, **tile)
    whole, stats = accumulate(s, p, [8])
    rows = [r for r in range(H) if (r // 4) % 3 == 1]
    assert whole["film"].shape == (3, len(rows), W) and stats[0]["tile_rows"] == len(rows)
    for split in SPLITS[1:]:
        got, _ = accumulate(s, p, split)
        assert_same(got, whole, f"tile split {split}")
    ref, _ = oracle_film(mode, W, H, SPP, DEPTH)
    np.testing.assert_array_equal(whole["film"], ref[:, rows, :])


# ---- the oracle's moments: 12 x 8 x 6 spp

MW, MH, MSPP = 12, 8, 6


@functools.lru_cache(maxsize=None)
def restated(mode, order):
    p = O.reference_params(MW, MH, MSPP, DEPTH, rng_order=order, **KW)
    return A.moments(A.contributions(oracle_scene(mode), p))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("mode", ["unit", "albedo", "emit"])
def test_moments_equal_the_restatement(mode, order):
    s = make_scene(mode)
    p = sptamd.make_params(MW, MH, MSPP, DEPTH, rng_order=order, **KW)
    ref = dict(zip(PLANES, restated(mode, order)))
    for split in ([6], [2, 4], [1] * 6):
        got, _ = accumulate(s, p, split)
        assert_same(got, ref, f"{mode} rng_order {order} split {split}")
    assert (ref["variance"] > 0).any()
    if order == 1:
        assert not np.array_equal(ref["sum"], restated(mode, 0)[0])   # the order reaches the samples


def test_moments_smallpt_spheres_mirror_glass():
    m = scenes.smallpt_analytic(detail=0.5)
    alb, emi = scenes.smallpt_materials(m)
    cam = scenes.cornell_camera()
    kw = dict(rr_start_depth=3, env=(0.0, 0.0, 0.0))
    s = sptamd.Scene()
    s.add_arrays(m)
    s.commit(0)
    s.backend.set_albedo(alb)
    s.backend.set_emission(emi)
    osc = O.OracleScene(m, albedo=alb, emission=emi)
    x = A.contributions(osc, O.reference_params(MW, MH, MSPP, 8, camera=cam, **kw))
    ref = dict(zip(PLANES, A.moments(x)))
    assert ref["sum"].max() > 0 and (ref["variance"] > 0).any()
    p = sptamd.make_params(MW, MH, MSPP, 8, camera=cam, **kw)
    for split in ([6], [4, 2]):
        got, _ = accumulate(s, p, split)
        assert_same(got, ref, f"smallpt split {split}")


# ---- the C ABI directly: optional planes, guards, refusals

GUARD = -7.0
PAD = 64


class Planes:
    """Four 3 x P planes carved out of one guarded buffer."""

    def __init__(self, npix, fill=GUARD):
        self.n = 3 * npix
        self.buf = torch.full((PAD + 4 * (self.n + PAD),), fill, dtype=torch.float32, device="cuda")
        self.t = {k: self.buf[PAD + i * (self.n + PAD): PAD + i * (self.n + PAD) + self.n] for i, k in enumerate(PLANES)}

    def struct(self, base, use=PLANES):
        a = _lib.Accum()
        a.sample_base = base
        for k in use:
            setattr(a, k, self.t[k].data_ptr())
        return a

    def guards_intact(self, unused=()):
        torch.cuda.synchronize()
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        for k in PLANES:
            if k not in unused:
                o = self.t[k].data_ptr() - self.buf.data_ptr()
                keep[o // 4: o // 4 + self.n] = False
        return bool(torch.all(self.buf[keep] == GUARD))

    def host(self, k):
        return self.t[k].cpu().numpy().reshape(3, -1)


def raw_pass(scene, params, spp, acc):
    params.spp = spp
    st = _lib.RenderStats()
    scene.backend.sync_config()
    rc = _lib.lib.spt_render_accum(scene.backend.handle, ctypes.byref(params), ctypes.byref(acc), ctypes.byref(st), None)
    return rc, st.as_dict()


@pytest.mark.parametrize("mode", ["unit", "albedo"])
def test_optional_planes_and_guards(mode):
    s = make_scene(mode)
    p = sptamd.make_params(W, H, SPP, DEPTH, **KW)
    whole, _ = accumulate(s, p, [8])
    flat = {k: v.reshape(3, -1) for k, v in whole.items()}
    for missing in ((), ("sum_sq", "variance"), ("film",), ("variance",), ("film", "variance"),
                    ("sum_sq", "film", "variance")):
        use = tuple(k for k in PLANES if k not in missing)
        pl = Planes(W * H)
        # sample_base = 0 ignores what sum / sum_sq hold (the guard value here)
        for base, n in ((0, 3), (3, 5)):
            rc, st = raw_pass(s, p, n, pl.struct(base, use))
            assert rc == 0, _lib.lib.spt_last_error()
        assert pl.guards_intact(unused=missing), missing
        for k in use:
            np.testing.assert_array_equal(pl.host(k), flat[k], err_msg=f"without {missing}: {k}")


def test_garbage_in_sum_is_ignored_at_sample_base_zero():
    s = make_scene("albedo")
    p = sptamd.make_params(W, H, SPP, DEPTH, **KW)
    whole, _ = accumulate(s, p, [8])
    pl = Planes(W * H, fill=float("nan"))
    rc, _ = raw_pass(s, p, 8, pl.struct(0))
    assert rc == 0
    torch.cuda.synchronize()
    for k in PLANES:
        np.testing.assert_array_equal(pl.host(k), whole[k].reshape(3, -1), err_msg=k)


def test_refusals_leave_the_buffers_alone():
    s = make_scene("albedo")
    p = sptamd.make_params(W, H, SPP, DEPTH, **KW)
    pl = Planes(W * H)
    inv, lim = _lib.SPT_ERR_INVALID, _lib.SPT_ERR_LIMIT
    cases = []
    cases.append((pl.struct(0, ("sum", "film", "variance")), 4, inv))          # variance without sum_sq
    a = pl.struct(0); a.film = a.sum; cases.append((a, 4, inv))                 # film is sum
    a = pl.struct(0); a.sum_sq = a.sum + 4 * (3 * W * H - 1); cases.append((a, 4, inv))   # one float shared
    a = pl.struct(0); a.variance = a.film + 4; cases.append((a, 4, inv))
    a = pl.struct(0); a.reserved = 1; cases.append((a, 4, inv))
    a = pl.struct(0); a.sum = None; cases.append((a, 4, inv))
    cases.append((pl.struct((1 << 24) - 4), 4, lim))                             # sample_base + spp = 2^24
    cases.append((pl.struct(0), 0, inv))                                         # spt_render's own checks
    for acc, n, want in cases:
        rc, _ = raw_pass(s, p, n, acc)
        assert rc == want, (rc, want, _lib.lib.spt_last_error())
    p.spp = 4
    assert _lib.lib.spt_render_accum(s.backend.handle, ctypes.byref(p), None, None, None) == inv
    torch.cuda.synchronize()
    assert bool(torch.all(pl.buf == GUARD))


def test_stats_describe_the_pass():
    s = make_scene("albedo")
    p = sptamd.make_params(W, H, SPP, DEPTH, pipeline="wavefront", **KW)
    _, stats = accumulate(s, p, [3, 5])
    _, st8 = s.render(p)
    for st, n in zip(stats, (3, 5)):
        assert st["paths"] == W * H * n == st["paths_started"] == st["paths_terminated"]
        assert st["film_slots_unwritten"] == 0 and st["tile_rows"] == H
    assert stats[0]["ray_casts"] + stats[1]["ray_casts"] == st8["ray_casts"]
    _, casts = oracle_film("albedo", W, H, SPP, DEPTH)
    assert st8["ray_casts"] == casts


def test_async_passes_on_one_queue_stream():
    s = make_scene("emit")
    p = sptamd.make_params(W, H, SPP, DEPTH, **KW)
    sync, _ = accumulate(s, p, [2, 2, 2, 2])
    q = sptamd.queue_stream()
    acc = s.accumulator(p)
    with torch.cuda.stream(q):
        tickets = [acc.add_async(2, stream=q) for _ in range(4)]
    stats = [acc.wait(t) for t in tickets]
    q.synchronize()
    assert acc.samples == 8 and all(st["paths"] == W * H * 2 for st in stats)
    got = {k: getattr(acc, k).cpu().numpy() for k in PLANES}
    assert_same(got, sync, "async")
    acc.reset()
    assert acc.samples == 0
    acc.add(8)
    torch.cuda.synchronize()
    assert_same({k: getattr(acc, k).cpu().numpy() for k in PLANES}, sync, "after reset")


def test_jump_table_growth_leaves_render_and_aov_as_they_were():
    """16 passes of 1 sample grow the (depth, seed) jump table tail by tail;
    spt_render and spt_render_aov at 16 spp then read the same table."""
    mode = "albedo"
    m, albedo, _ = mode_scene(mode)
    s = make_scene(mode)
    p = sptamd.make_params(MW, MH, 16, DEPTH, **KW)
    got, _ = accumulate(s, p, [1] * 16)
    op = O.reference_params(MW, MH, 16, DEPTH, **KW)
    ref, _ = oracle_scene(mode).render(op)
    np.testing.assert_array_equal(got["film"], ref)
    film, _ = s.render(p)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(film.cpu().numpy(), ref)
    planes = aov_ref.gpu_planes(s, p)
    hits = aov_ref.first_hits(oracle_scene(mode), op, range(MH))
    want = aov_ref.reference_planes(s, m, hits, albedo=albedo)
    for k in want:
        np.testing.assert_array_equal(planes[k], want[k], err_msg=k)
    # a longer table than any so far (a reallocation), then the short one again
    got2, _ = accumulate(s, sptamd.make_params(MW, MH, 16, DEPTH, **KW), [100, 50])
    ref150, _ = oracle_scene(mode).render(O.reference_params(MW, MH, 150, DEPTH, **KW))
    np.testing.assert_array_equal(got2["film"], ref150)
    film, _ = s.render(p)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(film.cpu().numpy(), ref)
