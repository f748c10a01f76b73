"""Python host mirror of the reference's hot-path interface, over libspt.so.

    HipBackend   <-> OptixBackend        (src/accel/optix_backend.h:164-504)
    Ray3         <-> Ray<Real3C>         (src/ray.h:5-36)
    TriangleHitInfo <-> TriangleHitInfo  (src/accel/optix_backend.h:99-134)
    Scene        <-> Scene               (src/main.cpp:286-352)
    Scene.render <-> main() render loop  (src/main.cpp:354-429)

Device memory and streams come from torch (HIP tensors); every computation
runs in the HIP kernels of libspt.so.  Errors raise SptError, as the
reference's OPTIX_CHECK / CUDA_CHECK raise std::runtime_error.
"""
from __future__ import annotations

import atexit
import ctypes
import math
import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import (Config, Hits, HitInfo, Rays, RenderParams, RenderStats, SceneStats, check, config_from_env,
                   env_snapshot, lib)

RAY_TMIN = 0.001  # ray.h:16
RAY_TMAX = 1e20


def _stream_handle(stream: Optional[torch.cuda.Stream]) -> Optional[int]:
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream or None


def queue_stream(device: Optional[int] = None) -> torch.cuda.ExternalStream:
    """A caller stream with a hardware queue of its own, for queued renders.

    HIP maps ordinary streams onto the process's GPU_MAX_HW_QUEUES hardware
    queues, and a stream's wait on an event blocks the whole queue it sits on.
    spt_render_async ends by making the caller stream wait for the render, so
    when the two streams renders alternate on share a queue, the next render's
    start (an event recorded on the other stream) waits behind that wait and
    the renders stop overlapping: one run in ten of a tile was ~30 % slow
    (profiles/r05_exp/caller_queues/).  A stream created with a
    CU mask gets a dedicated queue (the library's own sub-wavefront streams are
    made the same way); this one has every CU in its mask.  It is a blocking
    stream, so work on the legacy null stream waits for it.  Made through the
    HIP runtime (torch offers no CU-mask stream), wrapped for torch; it is
    destroyed at interpreter exit, after a device synchronisation, before the
    runtime's own teardown."""
    dev = torch.cuda.current_device() if device is None else device
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    words = (ncu + 31) // 32
    mask = (ctypes.c_uint32 * words)(*([0xFFFFFFFF] * words))
    hip = _hip_runtime()
    handle = ctypes.c_void_p()
    with torch.cuda.device(dev):
        rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(handle), ctypes.c_uint32(words), mask)
    if rc != 0:
        raise _lib.SptError("hipExtStreamCreateWithCUMask", rc, "no stream with a dedicated hardware queue")
    if not _QUEUE_STREAMS:
        atexit.register(_destroy_queue_streams)
    _QUEUE_STREAMS.append((dev, handle.value))
    return torch.cuda.ExternalStream(handle.value, device=torch.device("cuda", dev))


_QUEUE_STREAMS = []


def _hip_runtime():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    return hip


def _destroy_queue_streams():
    hip = _hip_runtime()
    for dev, h in _QUEUE_STREAMS:
        with torch.cuda.device(dev):
            hip.hipStreamSynchronize(h)
            hip.hipStreamDestroy(h)
    _QUEUE_STREAMS.clear()


def _dev_f32(x, device) -> torch.Tensor:
    t = torch.as_tensor(x, dtype=torch.float32)
    return t.to(device).contiguous()


def _host_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


@dataclass
class Ray3:
    """SoA rays (ray.h:28-31).  origin/dir: (3, N) float32 device tensors."""

    origin: torch.Tensor
    dir: torch.Tensor
    tmin: torch.Tensor
    tmax: torch.Tensor

    @staticmethod
    def make(origin, direction, tmin: float = RAY_TMIN, tmax: float = RAY_TMAX, device="cuda") -> "Ray3":
        o = _dev_f32(origin, device)
        d = _dev_f32(direction, device)
        n = o.shape[1]
        return Ray3(o, d, torch.full((n,), tmin, dtype=torch.float32, device=o.device),
                    torch.full((n,), tmax, dtype=torch.float32, device=o.device))

    def __len__(self) -> int:
        return int(self.origin.shape[1])

    def c_struct(self) -> Rays:
        return Rays(self.origin[0].data_ptr(), self.origin[1].data_ptr(), self.origin[2].data_ptr(),
                    self.dir[0].data_ptr(), self.dir[1].data_ptr(), self.dir[2].data_ptr(),
                    self.tmin.data_ptr(), self.tmax.data_ptr())


@dataclass
class TriangleHitInfo:
    """optix_backend.h:99-134; device tensors, planar (3, N) vectors."""

    tri_id: torch.Tensor
    t: torch.Tensor
    barycentric: torch.Tensor
    position: torch.Tensor
    geometry_normal: torch.Tensor
    shading_normal: torch.Tensor
    texcoord: torch.Tensor
    material_id: torch.Tensor


class HipBackend:
    """OptixBackend replacement: init / set_triangles_soup / intersect."""

    def __init__(self, config: Optional[Config] = None):
        self._scene = ctypes.c_void_p()
        self.device = None
        self.stats: dict = {}
        # spt_config: explicit base (default: the library's), with the SPT_*
        # environment variables applied over it before every call that reads it
        self.base_config = config
        self._applied = None
        self._env_key = None

    def __del__(self):
        if getattr(self, "_scene", None) and self._scene.value:
            lib.spt_scene_destroy(self._scene)
            self._scene = ctypes.c_void_p()

    # optix_backend.h:178-186
    def init(self, device: int = 0) -> None:
        check(lib.spt_init(device), "spt_init")
        self.device = torch.device("cuda", device)

    # optix_backend.h:283-364 (arrays are host arrays here; the BVH is built on the host)
    def set_triangles_soup(self, position_triplets, positions, shading_normal_triplets=None, shading_normals=None,
                           texcoord_triplets=None, texcoords=None, material_ids=None, build: int = 0) -> None:
        """build: _lib.SPT_BUILD_AUTO / SPT_BUILD_HOST_SAH / SPT_BUILD_GPU_PLOC."""
        if self.device is None:
            self.init(0)
        pt = np.ascontiguousarray(np.asarray(position_triplets, dtype=np.int32).reshape(-1))
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.float32).reshape(-1))
        nt = None if shading_normal_triplets is None else np.ascontiguousarray(
            np.asarray(shading_normal_triplets, dtype=np.int32).reshape(-1))
        nrm = None if shading_normals is None else np.ascontiguousarray(
            np.asarray(shading_normals, dtype=np.float32).reshape(-1))
        tt = None if texcoord_triplets is None else np.ascontiguousarray(
            np.asarray(texcoord_triplets, dtype=np.int32).reshape(-1))
        tc = None if texcoords is None else np.ascontiguousarray(np.asarray(texcoords, dtype=np.float32).reshape(-1))
        mat = None if material_ids is None else np.ascontiguousarray(np.asarray(material_ids, dtype=np.int32).reshape(-1))
        ntri = pt.size // 3
        if self._scene.value:
            lib.spt_scene_destroy(self._scene)
            self._scene = ctypes.c_void_p()
        cfg = config_from_env(self.base_config)
        if build:
            cfg.build = build
        check(lib.spt_scene_create_cfg(
            _host_ptr(pt), _host_ptr(pos), pos.size // 3, ntri,
            _host_ptr(nt), _host_ptr(nrm), 0 if nrm is None else nrm.size // 3,
            _host_ptr(tt), _host_ptr(tc), 0 if tc is None else tc.size // 2,
            _host_ptr(mat), ctypes.byref(cfg), ctypes.byref(self._scene)), "spt_scene_create")
        self._applied = bytes(cfg)
        self._env_key = None
        st = SceneStats()
        check(lib.spt_scene_get_stats(self._scene, ctypes.byref(st)), "spt_scene_get_stats")
        self.stats = st.as_dict()

    def set_albedo(self, albedo_rgb) -> None:
        a = np.ascontiguousarray(np.asarray(albedo_rgb, dtype=np.float32).reshape(-1, 3))
        check(lib.spt_scene_set_albedo(self._scene, a.ctypes.data, a.shape[0]), "spt_scene_set_albedo")

    def set_emission(self, emission_rgb) -> None:
        e = np.ascontiguousarray(np.asarray(emission_rgb, dtype=np.float32).reshape(-1, 3))
        check(lib.spt_scene_set_emission(self._scene, e.ctypes.data, e.shape[0]), "spt_scene_set_emission")

    def set_spheres(self, center_radius=None, material_ids=None) -> None:
        """smallpt's analytic spheres: (n, 4) (cx, cy, cz, r) float32 and n material ids; None removes them."""
        if center_radius is None or len(center_radius) == 0:
            check(lib.spt_scene_set_spheres(self._scene, None, None, 0), "spt_scene_set_spheres")
            return
        cr = np.ascontiguousarray(np.asarray(center_radius, dtype=np.float32).reshape(-1, 4))
        mat = None if material_ids is None else np.ascontiguousarray(np.asarray(material_ids, dtype=np.int32))
        check(lib.spt_scene_set_spheres(self._scene, cr.ctypes.data, _host_ptr(mat), cr.shape[0]),
              "spt_scene_set_spheres")
        self._spheres = (cr, mat)

    def set_material_kinds(self, kinds) -> None:
        """Per material _lib.SPT_MAT_DIFFUSE / _MIRROR / _GLASS."""
        k = np.ascontiguousarray(np.asarray(kinds, dtype=np.uint32).reshape(-1))
        check(lib.spt_scene_set_material_kinds(self._scene, k.ctypes.data, k.size), "spt_scene_set_material_kinds")

    def set_envmap(self, image=None, rotation=None) -> None:
        """spt_scene_set_envmap: the octahedral sky image, (N, N, 3) float32 (row = b,
        column = a; envmap_from_latlong makes one from a lat-long image), and a
        3 x 3 world -> map rotation (None: identity).  image None removes the map."""
        if image is None:
            check(lib.spt_scene_set_envmap(self._scene, None, 0, None), "spt_scene_set_envmap")
            return
        img = np.ascontiguousarray(np.asarray(image, dtype=np.float32))
        if img.ndim != 3 or img.shape[0] != img.shape[1] or img.shape[2] != 3:
            raise ValueError(f"set_envmap: the image must be (N, N, 3), got {img.shape}")
        rot = None if rotation is None else np.ascontiguousarray(np.asarray(rotation, dtype=np.float32).reshape(9))
        check(lib.spt_scene_set_envmap(self._scene, img.ctypes.data, img.shape[0], _host_ptr(rot)),
              "spt_scene_set_envmap")

    def set_light_sampling(self, on=True) -> None:
        """spt_scene_set_light_sampling: sample the scene's emissive triangles with a
        shadow ray at every diffuse path vertex (next-event estimation).  Renders of
        such a scene run the fused pipeline; stats["shadow_casts"] counts the rays."""
        check(lib.spt_scene_set_light_sampling(self._scene, 1 if on else 0), "spt_scene_set_light_sampling")

    def shadow_casts(self) -> int:
        """spt_scene_get_shadow_casts: the shadow rays of the render collected last."""
        n = ctypes.c_uint64(0)
        check(lib.spt_scene_get_shadow_casts(self._scene, ctypes.byref(n)), "spt_scene_get_shadow_casts")
        return int(n.value)

    def _stats(self, st) -> dict:
        """A collected render's stats dict, with its shadow_casts."""
        d = st.as_dict()
        d["shadow_casts"] = self.shadow_casts()
        return d

    def light_sampling(self):
        """(on, lights): the switch and the size of the scene's light table."""
        on, n = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib.spt_scene_get_light_sampling(self._scene, ctypes.byref(on), ctypes.byref(n)),
              "spt_scene_get_light_sampling")
        return bool(on.value), int(n.value)

    def set_sky_sampling(self, on=True, share=0.5) -> None:
        """spt_scene_set_sky_sampling: sample the sky image (set_envmap) by its
        brightness with a shadow ray at every diffuse path vertex.  share: the
        probability of the sky where set_light_sampling is on too.  Renders of such
        a scene run the fused pipeline; stats["shadow_casts"] counts the rays."""
        check(lib.spt_scene_set_sky_sampling(self._scene, 1 if on else 0, float(share)), "spt_scene_set_sky_sampling")

    def sky_sampling(self):
        """(on, share, cells): the switch, the share and the cells of the sky table (0: none or empty)."""
        on, share, n = ctypes.c_uint32(0), ctypes.c_float(0), ctypes.c_uint32(0)
        check(lib.spt_scene_get_sky_sampling(self._scene, ctypes.byref(on), ctypes.byref(share), ctypes.byref(n)),
              "spt_scene_get_sky_sampling")
        return bool(on.value), float(share.value), int(n.value)

    def set_mis(self, on=True) -> None:
        """spt_scene_set_mis: combine the shadow rays of set_light_sampling /
        set_sky_sampling with the bounce rays by the balance heuristic instead of
        letting them replace the bounce ray's view of those lights.  No ray more or
        less; inert where neither table is non-empty."""
        check(lib.spt_scene_set_mis(self._scene, 1 if on else 0), "spt_scene_set_mis")

    def mis(self) -> bool:
        """The switch of set_mis."""
        on = ctypes.c_uint32(0)
        check(lib.spt_scene_get_mis(self._scene, ctypes.byref(on)), "spt_scene_get_mis")
        return bool(on.value)

    def set_texture(self, material: int, image=None) -> None:
        """Material `material`'s reflectance image (ImageTexture, main.cpp:34-80):
        (H, W, 3) float32, or None to remove it."""
        if image is None:
            check(lib.spt_scene_set_texture(self._scene, material, None, 0, 0), "spt_scene_set_texture")
            return
        img = np.ascontiguousarray(np.asarray(image, dtype=np.float32))
        assert img.ndim == 3 and img.shape[2] == 3, "texture must be (H, W, 3)"
        check(lib.spt_scene_set_texture(self._scene, material, img.ctypes.data, img.shape[1], img.shape[0]),
              "spt_scene_set_texture")

    def update_geometry(self, position_triplets, positions, shading_normal_triplets=None, shading_normals=None,
                        stream=None) -> None:
        """spt_scene_update_geometry: new positions / normals for the scene's
        triangles, the BVH refitted in place (no rebuild; every material setter's
        state stays).  Numpy arrays take the host call; if `positions` is a CUDA
        tensor every given array must be one (int32 / float32) and the device
        call runs on `stream` (default: torch's current stream).  Synchronous."""
        if isinstance(positions, torch.Tensor) and positions.is_cuda:
            given = [a for a in (position_triplets, shading_normal_triplets, shading_normals) if a is not None]
            if not all(isinstance(a, torch.Tensor) and a.is_cuda for a in given):
                raise TypeError("update_geometry: with CUDA positions every given array must be a CUDA tensor")
            pt = position_triplets.to(torch.int32).contiguous().reshape(-1)
            pos = positions.to(torch.float32).contiguous().reshape(-1)
            nt = None if shading_normal_triplets is None else shading_normal_triplets.to(torch.int32).contiguous().reshape(-1)
            nrm = None if shading_normals is None else shading_normals.to(torch.float32).contiguous().reshape(-1)
            # (conversions above ran on torch's current stream)
            s = stream if stream is not None else torch.cuda.current_stream(pos.device)
            s.wait_stream(torch.cuda.current_stream(pos.device))
            check(lib.spt_scene_update_geometry_device(
                self._scene, pt.data_ptr(), pos.data_ptr(), pos.numel() // 3, pt.numel() // 3,
                None if nt is None else nt.data_ptr(), None if nrm is None else nrm.data_ptr(),
                0 if nrm is None else nrm.numel() // 3, s.cuda_stream or None), "spt_scene_update_geometry_device")
            return
        pt = np.ascontiguousarray(np.asarray(position_triplets, dtype=np.int32).reshape(-1))
        pos = None if positions is None else np.ascontiguousarray(np.asarray(positions, dtype=np.float32).reshape(-1))
        nt = None if shading_normal_triplets is None else np.ascontiguousarray(
            np.asarray(shading_normal_triplets, dtype=np.int32).reshape(-1))
        nrm = None if shading_normals is None else np.ascontiguousarray(
            np.asarray(shading_normals, dtype=np.float32).reshape(-1))
        check(lib.spt_scene_update_geometry(
            self._scene, _host_ptr(pt), _host_ptr(pos), 0 if pos is None else pos.size // 3, pt.size // 3,
            _host_ptr(nt), _host_ptr(nrm), 0 if nrm is None else nrm.size // 3), "spt_scene_update_geometry")

    def refit_stats(self) -> dict:
        """spt_scene_get_refit_stats as a dict (zeros before the first update)."""
        st = _lib.RefitStats()
        check(lib.spt_scene_get_refit_stats(self._scene, ctypes.byref(st)), "spt_scene_get_refit_stats")
        return st.as_dict()

    def save(self, path: str, extra: bytes = b"") -> None:
        """spt_scene_save: the committed scene (BVH, arrays, materials) + extra bytes to one file."""
        check(lib.spt_scene_save(self._scene, os.fsencode(path), extra or None, len(extra)), "spt_scene_save")

    def load(self, path: str, device: int = 0) -> bytes:
        """spt_scene_load onto `device`: no parse, no build.  Returns the file's extra bytes."""
        self.init(device)
        if self._scene.value:
            lib.spt_scene_destroy(self._scene)
            self._scene = ctypes.c_void_p()
        n, cap = ctypes.c_uint64(), 1 << 16
        while True:
            buf = ctypes.create_string_buffer(cap)
            check(lib.spt_scene_load(os.fsencode(path), ctypes.byref(self._scene), buf, cap, ctypes.byref(n)),
                  "spt_scene_load")
            if n.value <= cap:
                break
            lib.spt_scene_destroy(self._scene)      # a larger extra than the first buffer: once more
            self._scene = ctypes.c_void_p()
            cap = n.value
        cfg = Config()
        check(lib.spt_scene_get_config(self._scene, ctypes.byref(cfg)), "spt_scene_get_config")
        if self.base_config is None:
            # the file's saved knobs are the base the SPT_* overrides apply to
            # (not the library defaults, which would silently replace them)
            self.base_config = Config.from_buffer_copy(bytes(cfg))
        self._applied = bytes(cfg)
        self._env_key = None
        st = SceneStats()
        check(lib.spt_scene_get_stats(self._scene, ctypes.byref(st)), "spt_scene_get_stats")
        self.stats = st.as_dict()
        return buf.raw[:n.value]

    @property
    def handle(self):
        return self._scene

    def sync_config(self) -> None:
        """Apply base config + SPT_* environment overrides if they changed
        (a render re-reads only the variables: ~2 us when nothing changed)."""
        snap = env_snapshot()
        key = (snap, None if self.base_config is None else bytes(self.base_config))
        if key == self._env_key and self._applied is not None:
            return
        cfg = config_from_env(self.base_config, snapshot=snap)
        if bytes(cfg) != self._applied:
            check(lib.spt_scene_set_config(self._scene, ctypes.byref(cfg)), "spt_scene_set_config")
            self._applied = bytes(cfg)
        self._env_key = key

    @property
    def config(self) -> dict:
        c = Config()
        check(lib.spt_scene_get_config(self._scene, ctypes.byref(c)), "spt_scene_get_config")
        return c.as_dict()

    def _dev_mask(self, mask, dev, stream):
        """Device uint8 copy of mask, kept alive until the launch's stream has
        consumed it (record_stream: the caching allocator will not hand the
        block to another stream's allocation before that)."""
        if mask is None:
            return None, 0, None
        m = torch.as_tensor(mask, dtype=torch.uint8).to(dev).contiguous().reshape(-1)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        m.record_stream(s)
        return m.data_ptr(), m.numel(), m

    def intersect_raw(self, rays: Ray3, mask=None, do_closest: bool = True, stream=None,
                      out: Optional[Sequence[torch.Tensor]] = None):
        """__raygen__rg semantics (wavefront_isect.cu:80-112).  Returns
        (tri_id, t, u, v); masked lanes keep `out`'s values (default -1/0)."""
        n = len(rays)
        dev = rays.origin.device
        if out is None:
            tri_id = torch.full((n,), -1, dtype=torch.int32, device=dev)
            t = torch.zeros(n, dtype=torch.float32, device=dev)
            u = torch.zeros(n, dtype=torch.float32, device=dev)
            v = torch.zeros(n, dtype=torch.float32, device=dev)
        else:
            tri_id, t, u, v = out
        self.sync_config()
        mask_ptr, mask_size, m = self._dev_mask(mask, dev, stream)
        hits = Hits(tri_id.data_ptr(), t.data_ptr(), u.data_ptr(), v.data_ptr())
        rs = rays.c_struct()
        check(lib.spt_intersect(self._scene, ctypes.byref(rs), mask_ptr, mask_size, ctypes.byref(hits), n,
                                1 if do_closest else 0, _stream_handle(stream)), "spt_intersect")
        return tri_id, t, u, v

    # optix_backend.h:422-487
    def intersect(self, rays: Ray3, mask=None, stream=None):
        tri_id, t, u, v = self.intersect_raw(rays, mask, True, stream)
        n = len(rays)
        dev = rays.origin.device
        z3 = lambda: torch.zeros((3, n), dtype=torch.float32, device=dev)  # noqa: E731
        pos, gn, sn, tc = z3(), z3(), z3(), torch.zeros((2, n), dtype=torch.float32, device=dev)
        mat = torch.zeros(n, dtype=torch.int32, device=dev)
        info = HitInfo(pos[0].data_ptr(), pos[1].data_ptr(), pos[2].data_ptr(),
                       gn[0].data_ptr(), gn[1].data_ptr(), gn[2].data_ptr(),
                       sn[0].data_ptr(), sn[1].data_ptr(), sn[2].data_ptr(),
                       tc[0].data_ptr(), tc[1].data_ptr(), mat.data_ptr())
        mask_ptr, mask_size, m = self._dev_mask(mask, dev, stream)
        rs = rays.c_struct()
        hits = Hits(tri_id.data_ptr(), t.data_ptr(), u.data_ptr(), v.data_ptr())
        check(lib.spt_hit_info_compute(self._scene, ctypes.byref(rs), ctypes.byref(hits), mask_ptr, mask_size, n,
                                       ctypes.byref(info), _stream_handle(stream)), "spt_hit_info_compute")
        active = tri_id != -1                                              # optix_backend.h:463
        if mask is not None:
            mt = torch.as_tensor(mask, dtype=torch.bool).to(dev).reshape(-1)
            active = active & (mt if mt.numel() == n else mt.expand(n))
        hit = TriangleHitInfo(tri_id, t, torch.stack([u, v]), pos, gn, sn, tc, mat)
        return hit, active


def reference_camera() -> dict:
    """ThinlensCamera at main.cpp:383."""
    return dict(look_from=(0.0, 3.03, 5.0), look_at=(0.0, 0.03, 0.0), up=(0.0, 1.0, 0.0), lens_radius=0.0,
                focal_dist=1.0, fov_y=float(np.float32(np.float32(40.0) / np.float32(180.0)) * np.float32(math.pi)),
                film_size_y=0.035)


def make_params(width: int, height: int, spp: int, max_depth: int, camera: Optional[dict] = None,
                tile_index: int = 0, tile_count: int = 1, rows_per_group: int = 1, wavefront_paths: int = 0,
                rr_start_depth: int = 1, rng_order: int = 0, env=(1.0, 1.0, 1.0), timing=False,
                rng_initstate: int = _lib.PCG32_DEFAULT_STATE, pipeline: Optional[str] = None) -> RenderParams:
    """pipeline: None (library default / SPT_FUSED), "wavefront" or "fused".
    timing: False, True (HIP events around isect launches) or "all" (every launch)."""
    p = _lib.default_params()
    p.width, p.height, p.spp, p.max_depth = width, height, spp, max_depth
    cam = reference_camera() if camera is None else camera
    for k in ("look_from", "look_at", "up"):
        getattr(p.camera, k)[:] = [float(x) for x in cam[k]]
    p.camera.lens_radius = cam["lens_radius"]
    p.camera.focal_dist = cam["focal_dist"]
    p.camera.fov_y = cam["fov_y"]
    p.camera.film_size_y = cam["film_size_y"]
    p.tile_index, p.tile_count, p.rows_per_group = tile_index, tile_count, rows_per_group
    p.wavefront_paths = wavefront_paths
    p.rr_start_depth = rr_start_depth
    p.rng_order = rng_order
    p.rng_initstate = rng_initstate
    p.env[:] = [float(e) for e in env]
    p.flags = _lib.SPT_FLAG_TIMING if timing else 0     # timing="all": every launch, not only isect
    if timing == "all":
        p.flags |= _lib.SPT_FLAG_TIMING_ALL
    if pipeline == "fused":
        p.flags |= _lib.SPT_FLAG_FUSED
    elif pipeline == "wavefront":
        p.flags |= _lib.SPT_FLAG_WAVEFRONT
    elif pipeline is not None:
        raise ValueError(f"pipeline must be None, 'wavefront' or 'fused', not {pipeline!r}")
    return p


class Scene:
    """main.cpp:286-352: add_triangle_mesh / commit / intersect, plus render()."""

    def __init__(self, config: Optional[Config] = None):
        self.backend = HipBackend(config)
        self.mesh = None
        self.pbrt_info: Optional[dict] = None

    def add_triangle_mesh(self, path: str) -> None:       # main.cpp:288-310
        """An OBJ (load_meshes) or, by extension, a pbrt-v3 scene; for .pbrt
        the file's camera / film / infinite light land in self.pbrt_info."""
        from .scenes import load_obj, load_pbrt
        if path.endswith(".pbrt"):
            self.mesh, self.pbrt_info = load_pbrt(path)
        else:
            self.mesh = load_obj(path)

    def add_arrays(self, mesh: dict) -> None:
        self.mesh = mesh

    def commit(self, device: int = 0, build: int = 0) -> None:  # main.cpp:312-318
        m = self.mesh
        self.backend.init(device)
        self.backend.set_triangles_soup(m["pos_tri"], m["pos"], m.get("nrm_tri"), m.get("nrm"), m.get("tc_tri"),
                                        m.get("tc"), m.get("mat_id"), build=build)
        if m.get("albedo") is not None:
            self.backend.set_albedo(m["albedo"])
        if m.get("emission") is not None:
            self.backend.set_emission(m["emission"])
        if m.get("spheres") is not None:
            self.backend.set_spheres(m["spheres"], m.get("sphere_mat"))
        if m.get("kinds") is not None:
            self.backend.set_material_kinds(m["kinds"])

    def update_geometry(self, pos, nrm=None, pos_tri=None, nrm_tri=None, stream=None) -> None:
        """HipBackend.update_geometry with the triplets of self.mesh unless
        given: pos (and nrm, if nrm_tri is given or the mesh has one) replace the
        mesh's arrays.  With numpy inputs self.mesh becomes a shallow copy that
        carries the new arrays.  A cache-loaded scene (mesh None) needs pos_tri."""
        m = self.mesh
        if pos_tri is None:
            if m is None:
                raise ValueError("update_geometry: a loaded scene has no mesh; pass pos_tri")
            pos_tri = m["pos_tri"]
        if nrm_tri is None and nrm is not None and m is not None:
            nrm_tri = m.get("nrm_tri")
        if nrm_tri is None:
            nrm = None
        elif nrm is None:
            raise ValueError("update_geometry: nrm_tri without nrm")
        on_dev = isinstance(pos, torch.Tensor) and pos.is_cuda
        if on_dev:
            dev = pos.device
            pos_tri = torch.as_tensor(np.asarray(pos_tri, dtype=np.int32), device=dev) \
                if not isinstance(pos_tri, torch.Tensor) else pos_tri
            if nrm_tri is not None and not isinstance(nrm_tri, torch.Tensor):
                nrm_tri = torch.as_tensor(np.asarray(nrm_tri, dtype=np.int32), device=dev)
        self.backend.update_geometry(pos_tri, pos, nrm_tri, nrm, stream=stream)
        if m is not None and not on_dev:
            m = dict(m)
            m["pos"] = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
            m["pos_tri"] = pos_tri
            if nrm_tri is not None:
                m["nrm"], m["nrm_tri"] = np.asarray(nrm, dtype=np.float32).reshape(-1, 3), nrm_tri
            else:
                m.pop("nrm", None)
                m.pop("nrm_tri", None)
            self.mesh = m

    def save(self, path: str) -> None:
        """Binary scene cache of the committed scene (spt_scene_save); pbrt_info rides
        along as the extra bytes (an spt_pbrt_info, as spt_render_cli --save-cache writes)."""
        from .scenes import pbrt_info_to_c
        self.backend.save(path, bytes(pbrt_info_to_c(self.pbrt_info)) if self.pbrt_info is not None else b"")

    @classmethod
    def load(cls, path: str, device: int = 0, config: Optional[Config] = None) -> "Scene":
        """A committed Scene from a spt_scene_save file (no parse, no BVH build); mesh stays None."""
        sc = cls(config)
        extra = sc.backend.load(path, device)
        if len(extra) == ctypes.sizeof(_lib.PbrtInfo):
            from .scenes import pbrt_info_from_c
            sc.pbrt_info = pbrt_info_from_c(_lib.PbrtInfo.from_buffer_copy(extra))
        elif extra:
            raise ValueError(f"{path}: {len(extra)} extra bytes are not an spt_pbrt_info")
        return sc

    def intersect(self, ray: Ray3, active=None):           # main.cpp:320-340
        return self.backend.intersect(ray, active)

    def render(self, params: RenderParams, film: Optional[torch.Tensor] = None, stream=None):
        """One wavefront render of params' tile.  Returns (film (3, rows, W)
        float32 on the device, stats dict)."""
        film = self._film(params, film)
        st = RenderStats()
        self.backend.sync_config()
        check(lib.spt_render(self.backend.handle, ctypes.byref(params), film.data_ptr(), ctypes.byref(st),
                             _stream_handle(stream)), "spt_render")
        return film, self.backend._stats(st)

    def render_async(self, params: RenderParams, film: Optional[torch.Tensor] = None, stream=None):
        """spt_render_async: queue the render and return (film, ticket) without
        waiting for it; collect its stats with render_wait(ticket)."""
        film = self._film(params, film)
        ticket = ctypes.c_uint64()
        self.backend.sync_config()
        check(lib.spt_render_async(self.backend.handle, ctypes.byref(params), film.data_ptr(),
                                   _stream_handle(stream), ctypes.byref(ticket)), "spt_render_async")
        return film, ticket.value

    def render_wait(self, ticket: int) -> dict:
        """spt_render_wait: the stats dict of a queued render (waits for it)."""
        st = RenderStats()
        check(lib.spt_render_wait(self.backend.handle, ticket, ctypes.byref(st)), "spt_render_wait")
        return self.backend._stats(st)

    def accumulator(self, params: RenderParams, moments: bool = True) -> "Accumulator":
        """A progressive render of params' tile (spt_render_accum): an object
        that owns the running sums and adds passes of samples to them.
        params.spp is not used (each add names its own count); moments=False
        keeps no sum of squares (no variance)."""
        return Accumulator(self, params, moments)

    def render_aov(self, params: RenderParams, planes: Sequence[str] = ("albedo", "normal", "depth", "coverage"),
                   stream=None, out: Optional[dict] = None) -> dict:
        """spt_render_aov: the first-hit buffers of params' tile, lined up with
        render(params)'s samples.  planes: any of "albedo", "normal" ((3, rows,
        W) float32 device tensors), "depth", "coverage" ((rows, W)); the others
        are not computed.  Depth and normal are premultiplied by coverage
        (include/spt.h).  out: tensors to fill instead of new ones, by name.
        Queued on `stream` (default: torch's current stream), not waited for."""
        rows = _lib.tile_row_count(params.height, params.tile_index, params.tile_count, params.rows_per_group)
        res, aov = {}, _lib.Aov()
        for name in planes:
            if name not in ("albedo", "normal", "depth", "coverage"):
                raise ValueError(f"render_aov: unknown plane {name!r}")
            shape = (3, rows, params.width) if name in ("albedo", "normal") else (rows, params.width)
            t = None if out is None else out.get(name)
            if t is None:
                t = torch.empty(shape, dtype=torch.float32, device=self.backend.device)
            assert t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == shape, name
            res[name] = t
            if name in ("albedo", "normal"):
                for c, field in enumerate(("albedo_r", "albedo_g", "albedo_b") if name == "albedo"
                                          else ("normal_x", "normal_y", "normal_z")):
                    setattr(aov, field, t[c].data_ptr())
            else:
                setattr(aov, name, t.data_ptr())
        self.backend.sync_config()
        check(lib.spt_render_aov(self.backend.handle, ctypes.byref(params), ctypes.byref(aov),
                                 _stream_handle(stream)), "spt_render_aov")
        return res

    def isect_busy_begin(self) -> None:
        """spt_scene_isect_busy_begin: start collecting isect launch intervals."""
        check(lib.spt_scene_isect_busy_begin(self.backend.handle), "spt_scene_isect_busy_begin")

    def kernel_busy(self, kernels: int = _lib.SPT_KERNEL_ISECT) -> Tuple[float, int]:
        """spt_scene_kernel_busy: (union of the isect / drain launch intervals
        collected since isect_busy_begin, in ms; launches), without stopping
        the collection.  kernels: a mask of _lib.SPT_KERNEL_*."""
        ms, n = ctypes.c_double(0.0), ctypes.c_uint64(0)
        check(lib.spt_scene_kernel_busy(self.backend.handle, kernels, ctypes.byref(ms), ctypes.byref(n)),
              "spt_scene_kernel_busy")
        return ms.value, n.value

    def isect_busy_end(self) -> Tuple[float, int]:
        """spt_scene_isect_busy_end: (union of the intervals collected since
        isect_busy_begin in ms, launches) across every render collected."""
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        check(lib.spt_scene_isect_busy_end(self.backend.handle, ctypes.byref(ms), ctypes.byref(n)),
              "spt_scene_isect_busy_end")
        return ms.value, n.value

    def _film(self, params: RenderParams, film: Optional[torch.Tensor]) -> torch.Tensor:
        rows = _lib.tile_row_count(params.height, params.tile_index, params.tile_count, params.rows_per_group)
        if film is None:
            film = torch.empty((3, rows, params.width), dtype=torch.float32, device=self.backend.device)
        assert film.is_contiguous() and film.numel() >= 3 * rows * params.width
        return film


class Accumulator:
    """Scene.accumulator: the planes of one spt_render_accum accumulation.

    add(spp) renders the next spp samples of every tile pixel and returns the
    pass's stats; add_async / wait are the queued pair (passes queued on one
    stream need no synchronisation in between).  film, variance, sum and sum_sq
    are (3, rows, W) float32 device tensors, current once the last pass has run
    on its stream; any split of N samples into passes gives the same bits, and
    film is Scene.render's at spp = N (include/spt.h).

    Adaptive sampling: add_list(spp, pixels) renders the next spp samples of
    the listed tile pixels only (spt_render_accum_list), add_adaptive(spp, ...)
    of the pixels spt_adapt_select finds unconverged.  count (rows, W; int32
    holding the uint32 values) is the number of samples each pixel's sums hold,
    samples the largest of them.  After a sparse pass add() raises: the pixels'
    sums are no longer prefixes of one length."""

    def __init__(self, scene: "Scene", params: RenderParams, moments: bool = True):
        self.scene = scene
        self.params = RenderParams.from_buffer_copy(params)
        rows = _lib.tile_row_count(params.height, params.tile_index, params.tile_count, params.rows_per_group)
        shape, dev = (3, rows, params.width), scene.backend.device
        self.sum = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.film = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.sum_sq = torch.zeros(shape, dtype=torch.float32, device=dev) if moments else None
        self.variance = torch.zeros(shape, dtype=torch.float32, device=dev) if moments else None
        self._count = torch.zeros(shape[1:], dtype=torch.int32, device=dev)
        self._count_stale = False       # every pixel holds `samples` (add keeps no per-pixel books)
        self.samples = 0
        self.sparse = False
        self._list = self._scratch = None

    @property
    def count(self) -> torch.Tensor:
        """(rows, W) int32: the samples each pixel's sums hold."""
        if self._count_stale:
            self._count.fill_(self.samples)
            self._count_stale = False
        return self._count

    def reset(self) -> None:
        """Start over: the next add renders sample 0 (the planes are rewritten by it)."""
        self.samples = 0
        self.sparse = False
        self._count_stale = True

    def _acc(self, spp: int, sparse: bool = False) -> _lib.Accum:
        if self.sparse and not sparse:
            raise RuntimeError("Accumulator.add after a sparse pass: the pixels hold different sample counts "
                               "(use add_list / add_adaptive, or reset)")
        if spp <= 0:
            raise ValueError("Accumulator.add: spp must be > 0")
        self.params.spp = spp
        a = _lib.Accum()
        a.sample_base = self.samples
        a.sum, a.film = self.sum.data_ptr(), self.film.data_ptr()
        if self.sum_sq is not None:
            a.sum_sq, a.variance = self.sum_sq.data_ptr(), self.variance.data_ptr()
        return a

    def add(self, spp: int, stream=None) -> dict:
        """Render samples [samples, samples + spp) onto the sums; returns the pass's stats."""
        a, st = self._acc(spp), RenderStats()
        self.scene.backend.sync_config()
        check(lib.spt_render_accum(self.scene.backend.handle, ctypes.byref(self.params), ctypes.byref(a),
                                   ctypes.byref(st), _stream_handle(stream)), "spt_render_accum")
        self.samples += spp
        self._count_stale = True
        return self.scene.backend._stats(st)

    def add_list(self, spp: int, pixels: torch.Tensor, n: Optional[int] = None, stream=None) -> dict:
        """spt_render_accum_list: samples [samples, samples + spp) of the tile
        pixels pixels[:n] (an int32 device tensor of strictly ascending tile
        pixel indices) onto their sums; count becomes samples + spp there.
        Synchronous; returns the pass's stats."""
        assert pixels.is_cuda and pixels.is_contiguous() and pixels.dtype == torch.int32, \
            "pixels must be a contiguous int32 device tensor"
        n = pixels.numel() if n is None else int(n)
        assert 0 <= n <= pixels.numel()
        a, st = self._acc(spp, sparse=True), RenderStats()
        if stream is not None:
            with torch.cuda.stream(stream):  # the fill, if one is due, goes where the pass runs
                self.count
        pl = _lib.PixelList()
        pl.pixels, pl.n, pl.count = pixels.data_ptr(), n, self.count.data_ptr()
        self.scene.backend.sync_config()
        check(lib.spt_render_accum_list(self.scene.backend.handle, ctypes.byref(self.params), ctypes.byref(a),
                                        ctypes.byref(pl), ctypes.byref(st), _stream_handle(stream)),
              "spt_render_accum_list")
        if n:
            self.samples += spp
        if n != self.count.numel():
            self.sparse = True
        return self.scene.backend._stats(st)

    def add_adaptive(self, spp: int, tolerance: Optional[float] = None, min_spp: Optional[int] = None,
                     max_spp: Optional[int] = None, floor: Optional[float] = None, stream=None) -> dict:
        """One adaptive pass: spt_adapt_select over the sums (the pixels that
        hold `samples` samples and are short of min_spp, or below max_spp and
        not converged to `tolerance`), then add_list(spp) over them.  Returns
        the pass's stats plus "active", the number of pixels sampled (0: done).
        Parameters default to spt_default_adapt_params.  Needs the moments."""
        if self.sum_sq is None:
            raise RuntimeError("Accumulator.add_adaptive needs moments=True")
        if stream is not None:
            with torch.cuda.stream(stream):
                self.count
        npix = self.count.numel()
        if self._list is None:
            dev = self.count.device
            self._list = torch.empty(max(1, npix), dtype=torch.int32, device=dev)
            self._scratch = torch.empty(lib.spt_adapt_select_scratch_bytes(npix), dtype=torch.uint8, device=dev)
        n = adapt_select(self.sum, self.sum_sq, self.count, self.samples, tolerance=tolerance, min_spp=min_spp,
                         max_spp=max_spp, floor=floor, out=self._list, scratch=self._scratch, stream=stream)
        st = self.add_list(spp, self._list, n, stream=stream)
        st["active"] = n
        return st

    def add_async(self, spp: int, stream=None) -> int:
        """Queue the pass and return its ticket (collect it with wait)."""
        a, ticket = self._acc(spp), ctypes.c_uint64()
        self.scene.backend.sync_config()
        check(lib.spt_render_accum_async(self.scene.backend.handle, ctypes.byref(self.params), ctypes.byref(a),
                                         _stream_handle(stream), ctypes.byref(ticket)), "spt_render_accum_async")
        self.samples += spp
        self._count_stale = True
        return ticket.value

    def wait(self, ticket: int) -> dict:
        """The stats of a queued pass (waits for it)."""
        return self.scene.render_wait(ticket)


def adapt_select(sum: torch.Tensor, sum_sq: torch.Tensor, count: torch.Tensor, sample_base: int,
                 tolerance: Optional[float] = None, min_spp: Optional[int] = None, max_spp: Optional[int] = None,
                 floor: Optional[float] = None, out: Optional[torch.Tensor] = None,
                 scratch: Optional[torch.Tensor] = None, stream=None):
    """spt_adapt_select: the pixels of an accumulation (sum, sum_sq: (3, ...)
    float32 planes, count: int32 samples per pixel) that a pass starting at
    sample_base must still sample, ascending.  Returns the list (an int32
    device tensor of that length), or with `out` (int32, one entry per pixel;
    only the head is written) just their number.  Parameters default to
    spt_default_adapt_params.  Waits for `stream` (default: the current one)."""
    npix = count.numel()
    for t, name, k in ((sum, "sum", 3), (sum_sq, "sum_sq", 3), (count, "count", 1)):
        assert t.is_cuda and t.is_contiguous() and t.numel() == k * npix, f"{name}: a contiguous device tensor"
    assert sum.dtype == torch.float32 and sum_sq.dtype == torch.float32 and count.dtype == torch.int32
    p = _lib.default_adapt_params()
    for k, v in (("tolerance", tolerance), ("min_spp", min_spp), ("max_spp", max_spp), ("floor", floor)):
        if v is not None:
            setattr(p, k, v)
    s = stream if stream is not None else torch.cuda.current_stream(count.device)
    with torch.cuda.stream(s):
        lst = torch.empty(max(1, npix), dtype=torch.int32, device=count.device) if out is None else out
        if scratch is None:
            scratch = torch.empty(lib.spt_adapt_select_scratch_bytes(npix), dtype=torch.uint8, device=count.device)
    assert lst.is_contiguous() and lst.dtype == torch.int32 and lst.numel() >= npix
    n = ctypes.c_uint32()
    check(lib.spt_adapt_select(ctypes.byref(p), npix, sample_base, sum.data_ptr(), sum_sq.data_ptr(), count.data_ptr(),
                               lst.data_ptr(), ctypes.byref(n), scratch.data_ptr(), s.cuda_stream or None),
          "spt_adapt_select")
    return n.value if out is not None else lst[: n.value]


def aov_struct(aov: Optional[dict]) -> _lib.Aov:
    """spt_aov over render_aov's dict (missing names: NULL planes)."""
    a = _lib.Aov()
    for name, fields in (("albedo", ("albedo_r", "albedo_g", "albedo_b")), ("normal", ("normal_x", "normal_y", "normal_z"))):
        t = None if aov is None else aov.get(name)
        if t is not None:
            assert t.is_contiguous() and t.dtype == torch.float32 and t.shape[0] == 3, name
            for c, f in enumerate(fields):
                setattr(a, f, t[c].data_ptr())
    for name in ("depth", "coverage"):
        t = None if aov is None else aov.get(name)
        if t is not None:
            assert t.is_contiguous() and t.dtype == torch.float32, name
            setattr(a, name, t.data_ptr())
    return a


def denoise(film: torch.Tensor, aov: Optional[dict] = None, iterations: int = 5, sigma_color: Optional[float] = None,
            sigma_normal: Optional[float] = None, sigma_albedo: Optional[float] = None,
            sigma_depth: Optional[float] = None, stream=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """spt_denoise: the edge-avoiding a-trous filter of a whole (3, H, W) film,
    guided by render_aov's dict (a missing plane disables its term).  Sigmas
    default to spt_default_denoise_params (sigma_color assumes radiance in
    [0, 1]); <= 0 disables a term.  Scratch and the result come from torch; the
    launches are queued on `stream` (default: the current stream)."""
    assert film.is_cuda and film.is_contiguous() and film.dtype == torch.float32 and film.dim() == 3 and \
        film.shape[0] == 3, "film must be a contiguous (3, H, W) float32 device tensor"
    p = _lib.default_denoise_params()
    p.height, p.width, p.iterations = int(film.shape[1]), int(film.shape[2]), iterations
    for k, v in (("sigma_color", sigma_color), ("sigma_normal", sigma_normal), ("sigma_albedo", sigma_albedo),
                 ("sigma_depth", sigma_depth)):
        if v is not None:
            setattr(p, k, float(v))
    for name in ("albedo", "normal", "depth"):
        t = None if aov is None else aov.get(name)
        assert t is None or tuple(t.shape[-2:]) == tuple(film.shape[1:]), f"{name}: not the film's size"
    s = stream if stream is not None else torch.cuda.current_stream(film.device)
    with torch.cuda.stream(s):
        if out is None:
            out = torch.empty_like(film)
        scratch = torch.empty(max(1, lib.spt_denoise_scratch_bytes(p.width, p.height)), dtype=torch.uint8,
                              device=film.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == film.shape
    guides = aov_struct(aov)
    check(lib.spt_denoise(ctypes.byref(p), film.data_ptr(), ctypes.byref(guides), out.data_ptr(), scratch.data_ptr(),
                          s.cuda_stream or None), "spt_denoise")
    return out


def denoise_var(film: torch.Tensor, variance: torch.Tensor, aov: Optional[dict] = None, iterations: int = 5,
                sigma_variance: Optional[float] = None, sigma_normal: Optional[float] = None,
                sigma_albedo: Optional[float] = None, sigma_depth: Optional[float] = None, stream=None,
                out: Optional[torch.Tensor] = None, return_variance: bool = False):
    """spt_denoise_var: the variance-guided a-trous filter of a whole (3, H, W)
    film, its colour term in standard deviations of `variance` (the (3, H, W)
    per-channel variance of the pixel mean, an Accumulator's), guided by
    render_aov's dict like denoise.  Sigmas default to
    spt_default_denoise_var_params; <= 0 disables a term.  Returns the filtered
    film, or (film, (H, W) remaining variance) with return_variance."""
    for t, name in ((film, "film"), (variance, "variance")):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.dim() == 3 and t.shape[0] == 3, \
            f"{name} must be a contiguous (3, H, W) float32 device tensor"
    assert variance.shape == film.shape, "variance: not the film's size"
    p = _lib.default_denoise_var_params()
    p.height, p.width, p.iterations = int(film.shape[1]), int(film.shape[2]), iterations
    for k, v in (("sigma_variance", sigma_variance), ("sigma_normal", sigma_normal), ("sigma_albedo", sigma_albedo),
                 ("sigma_depth", sigma_depth)):
        if v is not None:
            setattr(p, k, float(v))
    for name in ("albedo", "normal", "depth"):
        t = None if aov is None else aov.get(name)
        assert t is None or tuple(t.shape[-2:]) == tuple(film.shape[1:]), f"{name}: not the film's size"
    s = stream if stream is not None else torch.cuda.current_stream(film.device)
    with torch.cuda.stream(s):
        if out is None:
            out = torch.empty_like(film)
        vout = torch.empty(film.shape[1:], dtype=torch.float32, device=film.device) if return_variance else None
        scratch = torch.empty(max(1, lib.spt_denoise_var_scratch_bytes(p.width, p.height)), dtype=torch.uint8,
                              device=film.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == film.shape
    guides = aov_struct(aov)
    check(lib.spt_denoise_var(ctypes.byref(p), film.data_ptr(), variance.data_ptr(), ctypes.byref(guides),
                              out.data_ptr(), None if vout is None else vout.data_ptr(), scratch.data_ptr(),
                              s.cuda_stream or None), "spt_denoise_var")
    return (out, vout) if return_variance else out


def _camera_struct(camera) -> _lib.Camera:
    """spt_camera from a dict as reference_camera's, or a copy of a _lib.Camera."""
    if isinstance(camera, _lib.Camera):
        return _lib.Camera.from_buffer_copy(camera)
    return _lib.Camera.from_buffer_copy(make_params(1, 1, 1, 1, camera=camera).camera)


def _history_struct(h: dict, shape) -> _lib.History:
    s = _lib.History()
    for name, sh in (("color", (3,) + shape), ("moment2", (3,) + shape), ("length", shape)):
        t = h[name]
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == sh, \
            f"{name}: a contiguous {sh} float32 device tensor"
        setattr(s, name, t.data_ptr())
    return s


def temporal_accumulate(sum: torch.Tensor, sum_sq: torch.Tensor, aov: dict, camera, prev: Optional[dict] = None,
                        prev_aov: Optional[dict] = None, prev_camera=None, samples: float = None,
                        out: Optional[dict] = None, want_film: bool = True, want_variance: bool = True, stream=None,
                        max_history: Optional[float] = None, sigma_depth: Optional[float] = None,
                        normal_min: Optional[float] = None) -> dict:
    """spt_temporal_accumulate: blend one frame's samples with the history of
    the previous view (include/spt.h).  sum, sum_sq: the (3, H, W) planes of an
    accumulation holding `samples` samples per pixel; aov: that frame's
    render_aov dict (depth and coverage needed, normal used when both frames
    have it); camera: the frame's view (a dict as reference_camera's, or a
    _lib.Camera).  prev, prev_aov, prev_camera: the last call's result, guides
    and view — all None on the first frame.  Returns a dict with color, moment2
    ((3, H, W)), length ((H, W)) — the next call's prev — and film, variance
    ((3, H, W), or None when not wanted); `out` supplies tensors to fill by
    name, none of which may be a tensor of prev (history is ping-ponged).
    max_history, sigma_depth, normal_min default to spt_default_temporal_params.
    One launch, queued on `stream` (default: the current stream)."""
    assert sum.is_cuda and sum.is_contiguous() and sum.dtype == torch.float32 and sum.dim() == 3 and \
        sum.shape[0] == 3, "sum must be a contiguous (3, H, W) float32 device tensor"
    assert sum_sq.is_cuda and sum_sq.is_contiguous() and sum_sq.dtype == torch.float32 and sum_sq.shape == sum.shape, \
        "sum_sq: not sum's shape"
    if samples is None:
        raise ValueError("temporal_accumulate: samples (per pixel, in sum / sum_sq) is required")
    if (prev is None) != (prev_aov is None) or (prev is None) != (prev_camera is None):
        raise ValueError("temporal_accumulate: prev, prev_aov and prev_camera go together")
    shape = tuple(sum.shape[1:])
    p = _lib.default_temporal_params()
    p.height, p.width = shape
    p.camera = _camera_struct(camera)
    p.prev_camera = _camera_struct(camera if prev_camera is None else prev_camera)
    p.samples = float(samples)
    for k, v in (("max_history", max_history), ("sigma_depth", sigma_depth), ("normal_min", normal_min)):
        if v is not None:
            setattr(p, k, float(v))
    for guides in (aov, prev_aov):
        for name in ("normal", "depth", "coverage"):
            t = None if guides is None else guides.get(name)
            assert t is None or tuple(t.shape[-2:]) == shape, f"{name}: not the image's size"
    s = stream if stream is not None else torch.cuda.current_stream(sum.device)
    res = {}
    with torch.cuda.stream(s):
        for name, sh, want in (("color", (3,) + shape, True), ("moment2", (3,) + shape, True), ("length", shape, True),
                               ("film", (3,) + shape, want_film), ("variance", (3,) + shape, want_variance)):
            t = None if out is None else out.get(name)
            if t is None and want:
                t = torch.empty(sh, dtype=torch.float32, device=sum.device)
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == sh), \
                f"out[{name!r}]: a contiguous {sh} float32 device tensor"
            res[name] = t if want else None
    cur = aov_struct({k: v for k, v in aov.items() if k != "albedo"})
    new = _history_struct(res, shape)
    old = guides_old = None
    if prev is not None:
        old = ctypes.byref(_history_struct(prev, shape))
        guides_old = ctypes.byref(aov_struct({k: v for k, v in prev_aov.items() if k != "albedo"}))
    check(lib.spt_temporal_accumulate(ctypes.byref(p), sum.data_ptr(), sum_sq.data_ptr(), ctypes.byref(cur), old,
                                      guides_old, ctypes.byref(new),
                                      None if res["film"] is None else res["film"].data_ptr(),
                                      None if res["variance"] is None else res["variance"].data_ptr(),
                                      s.cuda_stream or None), "spt_temporal_accumulate")
    return res


class TemporalAccumulator:
    """Temporal accumulation over a moving view: each frame() renders a few new
    samples per pixel, renders the first-hit buffers of its view and blends the
    samples with the history reprojected from the previous frame
    (spt_temporal_accumulate; ping-pong buffers, swapped per frame).

    frame(spp, camera=None) is frame k = 0, 1, ...: it sets the view if one is
    given, renders samples [base, base + spp) of every pixel (base = the samples
    drawn so far, k spp for a constant spp: a still camera keeps drawing new
    samples) onto zeroed sums, and returns the render pass's stats.  film,
    variance ((3, H, W)), length ((H, W)) and aov (render_aov's dict) are the
    last frame's; downstream: denoise_var(t.film, t.variance, t.aov).
    reset() drops the history (the next frame starts from its own samples; the
    sample counter runs on).  Geometry updates between frames are allowed: a
    surface that changed fails the depth / normal test and restarts.  Whole
    images only (params.tile_count = 1)."""

    def __init__(self, scene: "Scene", params: RenderParams, max_history: float = 64.0,
                 sigma_depth: Optional[float] = None, normal_min: Optional[float] = None,
                 planes: Sequence[str] = ("albedo", "normal", "depth", "coverage")):
        if params.tile_count != 1:
            raise ValueError("TemporalAccumulator: whole images only (tile_count = 1)")
        if "depth" not in planes or "coverage" not in planes:
            raise ValueError("TemporalAccumulator: planes must hold depth and coverage")
        self.scene = scene
        self.params = RenderParams.from_buffer_copy(params)
        self.max_history, self.sigma_depth, self.normal_min = max_history, sigma_depth, normal_min
        self.planes = tuple(planes)
        shape, dev = (3, params.height, params.width), scene.backend.device
        self.sum = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.sum_sq = torch.zeros(shape, dtype=torch.float32, device=dev)
        new = lambda sh: torch.zeros(sh, dtype=torch.float32, device=dev)  # noqa: E731
        self._hist = [{"color": new(shape), "moment2": new(shape), "length": new(shape[1:]), "film": new(shape),
                       "variance": new(shape)} for _ in range(2)]
        self._aov = [None, None]
        self._camera = [None, None]
        self._cur = 0            # the slot the last frame wrote
        self.frames = 0          # frames since the last reset
        self.samples = 0         # samples drawn per pixel over every frame: the next frame's sample_base

    film = property(lambda self: self._hist[self._cur]["film"])
    variance = property(lambda self: self._hist[self._cur]["variance"])
    length = property(lambda self: self._hist[self._cur]["length"])
    color = property(lambda self: self._hist[self._cur]["color"])
    moment2 = property(lambda self: self._hist[self._cur]["moment2"])
    aov = property(lambda self: self._aov[self._cur])

    def reset(self) -> None:
        """Drop the history: the next frame's result is its own samples."""
        self.frames = 0

    def frame(self, spp: int, camera=None, stream=None) -> dict:
        if spp <= 0:
            raise ValueError("TemporalAccumulator.frame: spp must be > 0")
        if camera is not None:
            self.params.camera = _camera_struct(camera)
        self.params.spp = spp
        s = stream if stream is not None else torch.cuda.current_stream(self.sum.device)
        with torch.cuda.stream(s):
            self.sum.zero_()
            self.sum_sq.zero_()
        acc, st = _lib.Accum(), RenderStats()
        acc.sample_base = self.samples
        acc.sum, acc.sum_sq = self.sum.data_ptr(), self.sum_sq.data_ptr()
        self.scene.backend.sync_config()
        check(lib.spt_render_accum(self.scene.backend.handle, ctypes.byref(self.params), ctypes.byref(acc),
                                   ctypes.byref(st), s.cuda_stream or None), "spt_render_accum")
        self.samples += spp
        nxt = 1 - self._cur if self.frames else self._cur
        self._aov[nxt] = self.scene.render_aov(self.params, self.planes, stream=s, out=self._aov[nxt])
        self._camera[nxt] = _lib.Camera.from_buffer_copy(self.params.camera)
        first = self.frames == 0
        temporal_accumulate(self.sum, self.sum_sq, self._aov[nxt], self._camera[nxt],
                            prev=None if first else self._hist[self._cur],
                            prev_aov=None if first else self._aov[self._cur],
                            prev_camera=None if first else self._camera[self._cur], samples=float(spp),
                            out=self._hist[nxt], stream=s, max_history=self.max_history,
                            sigma_depth=self.sigma_depth, normal_min=self.normal_min)
        self._cur = nxt
        self.frames += 1
        return self.scene.backend._stats(st)


def scene_cache_info(path: str) -> dict:
    """spt_scene_cache_info: checks a scene cache file (header, sizes, every
    section's checksum) without a device; returns its stats, config and extra size."""
    st, cfg, n = SceneStats(), Config(), ctypes.c_uint64()
    check(lib.spt_scene_cache_info(os.fsencode(path), ctypes.byref(st), ctypes.byref(cfg), ctypes.byref(n)),
          "spt_scene_cache_info")
    return {"stats": st.as_dict(), "config": cfg.as_dict(), "extra_bytes": n.value}


def write_pfm(path: str, film: np.ndarray) -> None:
    """Fimage::save_pfm via the C ABI; film: (3, H, W) float32 host array."""
    f = np.ascontiguousarray(film, dtype=np.float32)
    _, h, w = f.shape
    check(lib.spt_pfm_write(path.encode(), f[0].ctypes.data, f[1].ctypes.data, f[2].ctypes.data, w, h),
          "spt_pfm_write")


def read_pfm(path: str) -> np.ndarray:
    """spt_pfm_read: a 3-channel PFM of either endianness as an (H, W, 3) float32
    array, rows top-down (write_pfm(path, x) then read_pfm(path) gives x.transpose(1, 2, 0))."""
    p, w, h = ctypes.POINTER(ctypes.c_float)(), ctypes.c_uint32(), ctypes.c_uint32()
    check(lib.spt_pfm_read(os.fsencode(path), ctypes.byref(p), ctypes.byref(w), ctypes.byref(h)), "spt_pfm_read")
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        lib.spt_pfm_free(p)


def light_table_build(tri_vertices, mat_id, emission_rgb):
    """spt_light_table_build: (ids uint32, cdf float32, pdf_area float32) of the light
    table of (T, 9) triangle vertices, T material ids (None: all 0) and (M, 3)
    emission (None: no emitters).  Host only."""
    tv = np.ascontiguousarray(np.asarray(tri_vertices, dtype=np.float32).reshape(-1, 9))
    mat = None if mat_id is None else np.ascontiguousarray(np.asarray(mat_id, dtype=np.int32).reshape(-1))
    if mat is not None and mat.size != tv.shape[0]:
        raise ValueError(f"light_table_build: {mat.size} material ids for {tv.shape[0]} triangles")
    emi = None if emission_rgb is None else np.ascontiguousarray(np.asarray(emission_rgb, dtype=np.float32).reshape(-1, 3))
    nmat = 0 if emi is None else emi.shape[0]
    n = ctypes.c_uint32(0)
    args = (_host_ptr(tv) if tv.size else None, _host_ptr(mat), tv.shape[0], _host_ptr(emi) if nmat else None, nmat)
    check(lib.spt_light_table_build(*args, None, None, None, 0, ctypes.byref(n)), "spt_light_table_build")
    ids, cdf, pdf = np.zeros(n.value, np.uint32), np.zeros(n.value, np.float32), np.zeros(n.value, np.float32)
    if n.value:
        check(lib.spt_light_table_build(*args, ids.ctypes.data, cdf.ctypes.data, pdf.ctypes.data, n.value,
                                        ctypes.byref(n)), "spt_light_table_build")
    return ids, cdf, pdf


def sky_table_build(image):
    """spt_sky_table_build: (marginal (N,), conditional (N, N), density (N, N)) float32 of
    the sampling table of an (N, N, 3) octahedral sky image; three empty arrays for an
    empty table (a map whose weights sum to 0).  Host only."""
    img = np.ascontiguousarray(np.asarray(image, dtype=np.float32))
    if img.ndim != 3 or img.shape[0] != img.shape[1] or img.shape[2] != 3:
        raise ValueError(f"sky_table_build: the image must be (N, N, 3), got {img.shape}")
    n = img.shape[0]
    marg, cond, pdf = np.zeros(n, np.float32), np.zeros((n, n), np.float32), np.zeros((n, n), np.float32)
    cells = ctypes.c_uint32(0)
    check(lib.spt_sky_table_build(img.ctypes.data if n else None, n, marg.ctypes.data, cond.ctypes.data, pdf.ctypes.data,
                                  ctypes.byref(cells)), "spt_sky_table_build")
    if cells.value == 0:
        return np.zeros(0, np.float32), np.zeros((0, 0), np.float32), np.zeros((0, 0), np.float32)
    return marg, cond, pdf


def envmap_from_latlong(img, n: int) -> np.ndarray:
    """spt_envmap_from_latlong: an (H, W, 3) lat-long image (pbrt's convention, z up)
    resampled to the (n, n, 3) octahedral image HipBackend.set_envmap takes.  Host only."""
    src = np.ascontiguousarray(np.asarray(img, dtype=np.float32))
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError(f"envmap_from_latlong: the image must be (H, W, 3), got {src.shape}")
    out = np.empty((max(int(n), 0), max(int(n), 0), 3), np.float32)
    check(lib.spt_envmap_from_latlong(src.ctypes.data, src.shape[1], src.shape[0], int(n), out.ctypes.data),
          "spt_envmap_from_latlong")
    return out
