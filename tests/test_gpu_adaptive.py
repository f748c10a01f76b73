"""Adaptive sampling on the GPU (include/spt.h): spt_adapt_select's ordered
compaction against tests/adaptive_ref.py on synthetic planes; a pass of
spt_render_accum_list against plain spt_render_accum passes, bit for bit on
the listed pixels and byte for byte untouched elsewhere, in every pipeline,
work order, film chunking and tile layout; a whole adaptive schedule against
the restatement; refusals that leave the buffers alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import accum_ref as A
import adaptive_ref as R
import sptamd
from sptamd import _lib, scenes
from test_gpu_accum import DEPTH, H, KW, PLANES, W, make_scene, pipeline_params

pytestmark = pytest.mark.gpu

P = W * H
INV = _lib.SPT_ERR_INVALID
RULE = dict(min_spp=2, max_spp=16, tolerance=0.1, floor=0.03)
PASSES = [2, 2, 4, 8]

# ---------------------------------------------------------------- selection

GUARD_I = -559038737   # 0xdeadbeef
PAD = 64


def guarded(n, dtype, fill):
    buf = torch.full((PAD + n + PAD,), fill, dtype=dtype, device="cuda")
    return buf, buf[PAD: PAD + n]


def select_planes(npix, mask, seed):
    """Planes of n = 4 samples whose active set is `mask` (None: random, by
    variance, count mismatches and NaNs).  Returns (sum, sum_sq, count) host arrays."""
    rng = np.random.default_rng(seed)
    n = 4
    x = np.empty((n, 3, 1, npix), np.float32)
    if mask is None:
        amp = rng.choice(np.array([0.0, 0.05, 0.3, 1.0], np.float32), size=npix)
        x[:] = 0.5 + amp * (rng.random((n, 3, 1, npix), dtype=np.float32) - 0.5)
    else:
        x[:] = 0.5
        x[0::2][..., mask] = 0.0     # 0, 1, 0, 1: far from converged
        x[1::2][..., mask] = 1.0
    s, q, _, _ = A.moments(x)
    s, q = s.reshape(3, npix).copy(), q.reshape(3, npix).copy()
    count = np.full(npix, n, np.int32)
    if mask is None:
        count[rng.random(npix) < 0.1] = 2
        count[rng.random(npix) < 0.05] = 8
        nan = rng.random(npix) < 0.03
        s[1, nan] = np.nan
        q[2, rng.random(npix) < 0.02] = np.nan
    return s, q, count, n


MASKS = ["all", "none", "first", "last", "alternating", "random"]


def make_mask(kind, npix):
    m = np.zeros(npix, bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "alternating":
        m[::2] = True
    return None if kind == "random" else m


def run_select(s, q, count, n, npix, rule=RULE):
    """(list buffer with guards, its view, n_active) of one spt_adapt_select call."""
    ds, dq = torch.from_numpy(s).cuda(), torch.from_numpy(q).cuda()
    dc = torch.from_numpy(count).cuda()
    lbuf, lst = guarded(npix, torch.int32, GUARD_I)
    nbytes = _lib.lib.spt_adapt_select_scratch_bytes(npix)
    sbuf, scr = guarded(nbytes, torch.uint8, 0xA5)
    p = _lib.default_adapt_params()
    for k, v in rule.items():
        setattr(p, k, v)
    out = ctypes.c_uint32(0xFFFFFFFF)
    rc = _lib.lib.spt_adapt_select(ctypes.byref(p), npix, n, ds.data_ptr(), dq.data_ptr(), dc.data_ptr(), lst.data_ptr(),
                                   ctypes.byref(out), scr.data_ptr(), None)
    assert rc == 0, _lib.lib.spt_last_error()
    torch.cuda.synchronize()
    assert bool((sbuf[:PAD] == 0xA5).all()) and bool((sbuf[PAD + nbytes:] == 0xA5).all()), "scratch guards"
    assert bool((lbuf[:PAD] == GUARD_I).all()) and bool((lbuf[PAD + npix:] == GUARD_I).all()), "list guards"
    return lst.cpu().numpy(), out.value


@pytest.mark.parametrize("npix", [1, 63, 64, 65, 256, 257, 703, 65537])
def test_select_equals_the_restatement(npix):
    for kind in MASKS:
        mask = make_mask(kind, npix)
        s, q, count, n = select_planes(npix, mask, seed=npix)
        want = R.active(s, q, count, n, **RULE)
        if mask is not None:
            np.testing.assert_array_equal(want, mask, err_msg="the planes must mean this mask")
        else:
            assert npix < 64 or 0 < want.sum() < npix
        idx = np.flatnonzero(want)
        lst, got_n = run_select(s, q, count, n, npix)
        assert got_n == len(idx), (kind, got_n, len(idx))
        np.testing.assert_array_equal(lst[:got_n], idx, err_msg=kind)
        assert (lst[got_n:] == GUARD_I).all(), f"{kind}: list[n:] must stay as it was"
        again, n2 = run_select(s, q, count, n, npix)
        assert n2 == got_n
        np.testing.assert_array_equal(again, lst, err_msg=f"{kind}: two runs differ")


def test_select_at_sample_base_zero_reads_nothing():
    npix = 703
    lbuf, lst = guarded(npix, torch.int32, GUARD_I)
    sbuf, scr = guarded(_lib.lib.spt_adapt_select_scratch_bytes(npix), torch.uint8, 0xA5)
    p = _lib.default_adapt_params()
    out = ctypes.c_uint32(0)
    # NULL inputs: nothing may be read
    rc = _lib.lib.spt_adapt_select(ctypes.byref(p), npix, 0, None, None, None, lst.data_ptr(), ctypes.byref(out),
                                   scr.data_ptr(), None)
    assert rc == 0, _lib.lib.spt_last_error()
    torch.cuda.synchronize()
    assert out.value == npix
    np.testing.assert_array_equal(lst.cpu().numpy(), np.arange(npix))
    assert bool((lbuf[:PAD] == GUARD_I).all()) and bool((lbuf[PAD + npix:] == GUARD_I).all())
    assert bool((sbuf == 0xA5).all())


def test_select_min_and_max_spp():
    npix = 300
    s, q, count, n = select_planes(npix, make_mask("alternating", npix), seed=1)
    for rule, want in ((dict(RULE, min_spp=8), np.ones(npix, bool)),            # n < min_spp: all that hold n
                       (dict(RULE, min_spp=2, max_spp=4), np.zeros(npix, bool)),  # n = max_spp: the cap
                       (dict(RULE, tolerance=0.0, floor=0.0), None)):
        ref = R.active(s, q, count, n, **rule)
        if want is not None:
            np.testing.assert_array_equal(ref, want)
        lst, got = run_select(s, q, count, n, npix, rule)
        np.testing.assert_array_equal(lst[:got], np.flatnonzero(ref))
    free = sptamd.adapt_select(torch.from_numpy(s).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(count).cuda(), n,
                               **RULE)
    np.testing.assert_array_equal(free.cpu().numpy(), np.flatnonzero(R.active(s, q, count, n, **RULE)))


# ------------------------------------------------------------- sparse passes

def nan_pattern(n):
    """n float32 quiet NaNs with distinct payloads (compared as bytes)."""
    bits = (0x7FC00000 | (np.arange(n, dtype=np.int64) % 0x3FFFFF + 1)).astype(np.uint32)
    return bits.view(np.float32)


class SparseBuffers:
    """The four planes and count, pre-filled: NaN payloads / a count pattern."""

    def __init__(self, npix):
        self.npix = npix
        self.init = {k: nan_pattern(3 * npix) for k in PLANES}
        self.count0 = (np.arange(npix) % 5 + 100).astype(np.int32)
        self.t = {k: torch.from_numpy(v.copy()).cuda() for k, v in self.init.items()}
        self.count = torch.from_numpy(self.count0.copy()).cuda()

    def load(self, planes, count):
        for k in PLANES:
            self.t[k].copy_(torch.from_numpy(np.ascontiguousarray(planes[k]).reshape(-1)))
            self.init[k] = np.ascontiguousarray(planes[k]).reshape(-1).copy()
        self.count.fill_(count)
        self.count0 = np.full(self.npix, count, np.int32)

    def accum(self, base):
        a = _lib.Accum()
        a.sample_base = base
        for k in PLANES:
            setattr(a, k, self.t[k].data_ptr())
        return a

    def bits(self, k):
        return self.t[k].cpu().numpy().view(np.uint32).reshape(3, self.npix)


def list_pass(scene, params, spp, bufs, base, pixels, n=None, count=True):
    """(status, stats) of one spt_render_accum_list call over the host index array `pixels`."""
    params.spp = spp
    dev = torch.from_numpy(np.asarray(pixels, np.int32)).cuda() if len(pixels) else torch.zeros(1, dtype=torch.int32,
                                                                                                 device="cuda")
    pl = _lib.PixelList()
    pl.pixels, pl.n = dev.data_ptr(), len(pixels) if n is None else n
    pl.count = bufs.count.data_ptr() if count else None
    acc = bufs.accum(base)
    st = _lib.RenderStats()
    scene.backend.sync_config()
    rc = _lib.lib.spt_render_accum_list(scene.backend.handle, ctypes.byref(params), ctypes.byref(acc), ctypes.byref(pl),
                                        ctypes.byref(st), None)
    torch.cuda.synchronize()
    return rc, st.as_dict()


def full_pass(scene, params, spp):
    """R_spp: the planes (host) and stats of one plain spt_render_accum pass."""
    acc = scene.accumulator(params)
    st = acc.add(spp)
    torch.cuda.synchronize()
    return {k: getattr(acc, k).cpu().numpy() for k in PLANES}, st


def lists_for(npix, seed=3):
    rng = np.random.default_rng(seed)
    out = [np.array([0]), np.array([npix - 1]), np.arange(npix)]
    for n in (1, 63, 64, 65, 257):
        if n < npix:
            out.append(np.sort(rng.choice(npix, size=n, replace=False)))
    return out


def check_sparse(scene, params, npix, spp, ref, what, lists=None, ref_stats=None):
    for px in lists_for(npix) if lists is None else lists:
        bufs = SparseBuffers(npix)
        rc, st = list_pass(scene, params, spp, bufs, 0, px)
        assert rc == 0, (what, _lib.lib.spt_last_error())
        listed = np.zeros(npix, bool)
        listed[px] = True
        for k in PLANES:
            got, want = bufs.bits(k), ref[k].reshape(3, npix).view(np.uint32)
            np.testing.assert_array_equal(got[:, listed], want[:, listed], err_msg=f"{what} n {len(px)} {k}: listed")
            init = bufs.init[k].view(np.uint32).reshape(3, npix)
            np.testing.assert_array_equal(got[:, ~listed], init[:, ~listed],
                                          err_msg=f"{what} n {len(px)} {k}: an unlisted pixel was written")
        cnt = bufs.count.cpu().numpy()
        assert (cnt[listed] == spp).all() and (cnt[~listed] == bufs.count0[~listed]).all(), f"{what}: count"
        n = len(px)
        assert st["paths"] == st["paths_started"] == st["paths_terminated"] == n * spp, (what, n, st)
        assert st["film_slots_unwritten"] == 0
        if n == npix and ref_stats is not None:
            for key in ("paths", "ray_casts", "continuations", "paths_started", "paths_terminated",
                        "film_slots_unwritten", "tile_rows", "work_order", "fused", "streams", "queue_cache"):
                assert st[key] == ref_stats[key], (what, key, st[key], ref_stats[key])


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("pipeline", ["wavefront", "queued", "fused", "percast"])
def test_list_pass_equals_the_full_pass(pipeline, order):
    cfg = sptamd.default_config()
    cfg.work_order = order
    p = pipeline_params(pipeline, cfg)
    s = make_scene("albedo", cfg)
    ref, rst = full_pass(s, p, 8)
    assert rst["work_order"] == order and rst["fused"] == (pipeline == "fused")
    check_sparse(s, p, P, 8, ref, f"{pipeline} order {order}", ref_stats=rst)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("mode", ["unit", "albedo", "emit"])
@pytest.mark.parametrize("pipeline", ["queued", "fused"])
def test_list_pass_with_two_film_chunks(pipeline, mode, order):
    cfg = sptamd.default_config()
    cfg.work_order = order
    cfg.film_budget_bytes = (1 if mode == "unit" else 12) * W * H * 4     # four samples: two chunks per pass
    p = pipeline_params(pipeline, cfg)
    s = make_scene(mode, cfg)
    ref, rst = full_pass(s, p, 8)
    one, _ = full_pass(make_scene(mode), pipeline_params(pipeline, sptamd.default_config()), 8)
    for k in PLANES:
        np.testing.assert_array_equal(ref[k], one[k])
    check_sparse(s, p, P, 8, ref, f"{mode} {pipeline} order {order} chunked", ref_stats=rst)


@pytest.mark.parametrize("lockstep", [0, 1, 2, 3])
def test_list_pass_under_every_lockstep_first(lockstep):
    cfg = sptamd.default_config()
    cfg.lockstep_first = lockstep
    p = pipeline_params("wavefront", cfg)
    s = make_scene("unit", cfg)
    ref, rst = full_pass(s, p, 8)
    rng = np.random.default_rng(lockstep)
    check_sparse(s, p, P, 8, ref, f"lockstep_first {lockstep}",
                 lists=[np.arange(P), np.sort(rng.choice(P, size=257, replace=False))], ref_stats=rst)


@pytest.mark.parametrize("mode", ["unit", "albedo"])
def test_list_pass_on_an_interleaved_tile(mode):
    s = make_scene(mode)
    tile = dict(tile_index=1, tile_count=2, rows_per_group=4)
    p = sptamd.make_params(W, H, 8, DEPTH, pipeline="wavefront", **KW, **tile)
    ref, rst = full_pass(s, p, 8)
    rows = rst["tile_rows"]
    assert 0 < rows < H
    check_sparse(s, p, rows * W, 8, ref, f"tile {mode}", ref_stats=rst)


def test_list_pass_continues_an_accumulation():
    """A full pass of 3 samples, then 5 more on a list: listed pixels hold R_8, the others R_3, byte for byte."""
    s = make_scene("emit")
    p = sptamd.make_params(W, H, 8, DEPTH, **KW)
    r3, _ = full_pass(s, p, 3)
    r8, _ = full_pass(s, p, 8)
    for px in lists_for(P, seed=9):
        bufs = SparseBuffers(P)
        bufs.load(r3, 3)
        rc, st = list_pass(s, p, 5, bufs, 3, px)
        assert rc == 0, _lib.lib.spt_last_error()
        listed = np.zeros(P, bool)
        listed[px] = True
        for k in PLANES:
            got = bufs.bits(k)
            np.testing.assert_array_equal(got[:, listed], r8[k].reshape(3, P).view(np.uint32)[:, listed], err_msg=k)
            np.testing.assert_array_equal(got[:, ~listed], r3[k].reshape(3, P).view(np.uint32)[:, ~listed], err_msg=k)
        cnt = bufs.count.cpu().numpy()
        assert (cnt[listed] == 8).all() and (cnt[~listed] == 3).all()
        assert st["paths"] == len(px) * 5


def test_list_pass_smallpt_spheres_mirror_glass():
    m = scenes.smallpt_analytic(detail=0.5)
    alb, emi = scenes.smallpt_materials(m)
    s = sptamd.Scene()
    s.add_arrays(m)
    s.commit(0)
    s.backend.set_albedo(alb)
    s.backend.set_emission(emi)
    p = sptamd.make_params(W, H, 6, 8, camera=scenes.cornell_camera(), rr_start_depth=3, env=(0.0, 0.0, 0.0))
    ref, rst = full_pass(s, p, 6)
    assert ref["sum"].max() > 0
    check_sparse(s, p, P, 6, ref, "smallpt", ref_stats=rst)


def test_list_pass_without_count_and_optional_planes():
    s = make_scene("albedo")
    p = sptamd.make_params(W, H, 8, DEPTH, **KW)
    ref, _ = full_pass(s, p, 8)
    px = lists_for(P)[-1]
    bufs = SparseBuffers(P)
    rc, _ = list_pass(s, p, 8, bufs, 0, px, count=False)
    assert rc == 0
    np.testing.assert_array_equal(bufs.count.cpu().numpy(), bufs.count0)
    listed = np.zeros(P, bool)
    listed[px] = True
    np.testing.assert_array_equal(bufs.bits("film")[:, listed], ref["film"].reshape(3, P).view(np.uint32)[:, listed])


def test_empty_list_queues_nothing():
    s = make_scene("albedo")
    p = sptamd.make_params(W, H, 8, DEPTH, **KW)
    bufs = SparseBuffers(P)
    rc, st = list_pass(s, p, 8, bufs, 0, np.array([], np.int32))
    assert rc == 0, _lib.lib.spt_last_error()
    assert st["paths"] == 0 and st["paths_started"] == 0 and st["ray_casts"] == 0 and st["iterations"] == 0
    for k in PLANES:
        np.testing.assert_array_equal(bufs.bits(k).reshape(-1), bufs.init[k].view(np.uint32))
    np.testing.assert_array_equal(bufs.count.cpu().numpy(), bufs.count0)


def test_refusals_leave_the_buffers_alone():
    s = make_scene("albedo")
    p = sptamd.make_params(W, H, 8, DEPTH, **KW)
    bufs = SparseBuffers(P)
    good = np.arange(0, P, 3)
    cases = {
        "unsorted": np.array([5, 4, 9]),
        "duplicate": np.array([1, 7, 7, 20]),
        "index = P": np.array([0, 10, P]),
        "far out of range": np.array([0, 10, 0x7FFFFFFF]),
    }
    for what, px in cases.items():
        rc, _ = list_pass(s, p, 4, bufs, 0, px)
        assert rc == INV, (what, rc)
        assert b"ascending" in _lib.lib.spt_last_error()
    rc, _ = list_pass(s, p, 4, bufs, 0, np.arange(P), n=P + 1)               # n > P (never read)
    assert rc == INV
    # pixels overlapping sum; count overlapping film; pixels overlapping count
    pl = _lib.PixelList()
    acc = bufs.accum(0)
    st = _lib.RenderStats()
    p.spp = 4
    f = _lib.lib.spt_render_accum_list
    dev = torch.from_numpy(good.astype(np.int32)).cuda()
    for pixels, count in ((bufs.t["sum"].data_ptr() + 8, bufs.count.data_ptr()),
                          (dev.data_ptr(), bufs.t["film"].data_ptr() + 4 * (3 * P - 1)),
                          (bufs.count.data_ptr() + 4, bufs.count.data_ptr())):
        pl.pixels, pl.n, pl.count, pl.reserved = pixels, len(good), count, 0
        assert f(s.backend.handle, ctypes.byref(p), ctypes.byref(acc), ctypes.byref(pl), ctypes.byref(st), None) == INV
        assert b"overlap" in _lib.lib.spt_last_error()
    pl.pixels, pl.count, pl.reserved = dev.data_ptr(), bufs.count.data_ptr(), 1
    assert f(s.backend.handle, ctypes.byref(p), ctypes.byref(acc), ctypes.byref(pl), ctypes.byref(st), None) == INV
    pl.reserved, pl.pixels = 0, None
    assert f(s.backend.handle, ctypes.byref(p), ctypes.byref(acc), ctypes.byref(pl), ctypes.byref(st), None) == INV
    assert f(s.backend.handle, ctypes.byref(p), ctypes.byref(acc), None, ctypes.byref(st), None) == INV
    # spt_accum's own checks still apply
    pl.pixels = dev.data_ptr()
    acc.film = acc.sum
    assert f(s.backend.handle, ctypes.byref(p), ctypes.byref(acc), ctypes.byref(pl), ctypes.byref(st), None) == INV
    torch.cuda.synchronize()
    for k in PLANES:
        np.testing.assert_array_equal(bufs.bits(k).reshape(-1), bufs.init[k].view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(bufs.count.cpu().numpy(), bufs.count0)
    # and the scene still renders
    rc, st = list_pass(s, p, 4, bufs, 0, good)
    assert rc == 0 and st["paths"] == len(good) * 4


# ------------------------------------------------------- the adaptive schedule

@functools.lru_cache(maxsize=None)
def reference_passes(mode):
    """R_b for b = 2, 4, 8, 16 (plain spt_render_accum passes of one scene)."""
    s = make_scene(mode)
    p = sptamd.make_params(W, H, 16, DEPTH, **KW)
    return {b: full_pass(s, p, b)[0] for b in np.cumsum(PASSES)}


@pytest.mark.parametrize("mode", ["unit", "albedo", "emit"])
def test_adaptive_schedule_end_to_end(mode):
    ref = reference_passes(mode)
    # the restatement's schedule from the reference passes alone
    count = np.zeros(P, np.int64)
    want_active, base = [], 0
    for spp in PASSES:
        r = ref[base] if base else None
        act = R.active(None if r is None else r["sum"].reshape(3, P), None if r is None else r["sum_sq"].reshape(3, P),
                       count, base, **RULE)
        want_active.append(act)
        count[act] = base + spp
        base += spp
    n_act = [int(a.sum()) for a in want_active]
    print(mode, "active per pass", n_act)
    # the condition on the choice of tolerance: no degenerate pass (on the reference alone)
    assert n_act[0] == P and all(0 < n < P for n in n_act[1:]), n_act
    s = make_scene(mode)
    acc = s.accumulator(sptamd.make_params(W, H, 16, DEPTH, **KW))
    for i, spp in enumerate(PASSES):
        st = acc.add_adaptive(spp, **RULE)
        assert st["active"] == n_act[i], (i, st["active"], n_act[i])
        assert st["paths"] == n_act[i] * spp == st["paths_started"] == st["paths_terminated"]
        assert st["film_slots_unwritten"] == 0
    torch.cuda.synchronize()
    got_count = acc.count.cpu().numpy().reshape(-1)
    np.testing.assert_array_equal(got_count, count)
    assert acc.samples == 16 == got_count.max()
    for k in PLANES:
        got = getattr(acc, k).cpu().numpy().reshape(3, P).view(np.uint32)
        for b in np.cumsum(PASSES):
            sel = count == b
            np.testing.assert_array_equal(got[:, sel], ref[int(b)][k].reshape(3, P).view(np.uint32)[:, sel],
                                          err_msg=f"{mode} {k}: pixels that stopped at {b}")
    # nothing is active any more at the cap, and add() refuses after sparse passes
    assert acc.add_adaptive(4, **RULE)["active"] == 0
    with pytest.raises(RuntimeError):
        acc.add(1)
    acc.reset()
    acc.add(2)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(acc.film.cpu().numpy(), ref[2]["film"])
    assert int(acc.count.min()) == int(acc.count.max()) == 2
