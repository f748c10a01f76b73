"""The render plan end to end (csrc/render_plan.h plan_render, render.cpp
render_enqueue): a grid of small renders over the knobs the plan reads — 1 and
3 sub-wavefronts, a null and a side caller stream, explicit paths in flight in
the params and in the config, fit_paths 0, fit_bytes small enough to chunk the
fit and to fall back to the per-cast wavefront, two film chunks, every
lockstep_first and drain_casts, the three pipelines, the three path modes and
an spt_render_accum pass that starts at sample 2.  Each film equals the
oracle's bit for bit, and the statistics known when the render was queued
equal tests/golden/render_plan_gpu_parent.json, recorded on the MI355X at the
commit before render_enqueue was split (the split must not change a decision
or a launch sequence).

Compared: fused, streams, paths_in_flight, fit_paths, fit_retries, work_order,
queue_cache, drain_refill_idle, lockstep_casts, ray_casts, and for jobs whose
every path starts in the first refill also iterations and drain_launches.
Jobs that refill (`refills` below) end when the host's lagging readback of
the device cursor says so, so their iterations and drain_launches are not
compared.  The golden file was recorded twice; no other field differed
between the two recordings on any row."""
import json
import os

import numpy as np
import pytest
import torch

import oracle as O
import sptamd
from conftest import assert_work_complete
from sptamd import scenes
from test_gpu_drain import D, H, SPP, W, gpu_scene, materials

pytestmark = pytest.mark.gpu
KW = dict(rr_start_depth=3, env=(1.0, 0.9, 0.8))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_plan_gpu_parent.json")
FIELDS = ("fused", "streams", "paths_in_flight", "fit_paths", "fit_retries", "work_order", "queue_cache",
          "drain_refill_idle", "lockstep_casts", "ray_casts")
FIT_FIELDS = ("iterations", "drain_launches")
# bytes per path in flight: two queues of 16-B planes, the hit record, the film slot
PER_PATH = {"unit": 2 * 16 * 2 + 16 + 1, "albedo": 2 * 16 * 3 + 16 + 12, "emit_spheres": 2 * 16 * 4 + 16 + 12}


def case(name, mode="unit", side=True, wf=0, pipe="wavefront", accum=False, refills=False, **knobs):
    """pipe: make_params' pipeline flag; knobs: spt_config fields."""
    return dict(name=name, mode=mode, side=side, wf=wf, pipe=pipe, accum=accum, refills=refills, knobs=knobs)


CASES = [
    # jobs that fit in flight: sub-wavefronts and caller stream
    case("fit_s1_side", streams=1, fit_streams=1),
    case("fit_s3_side", streams=3, fit_streams=3),
    case("fit_s1_null", side=False, streams=1, fit_streams=1),
    case("fit_s3_null", side=False, streams=3, fit_streams=3),
    case("fit_s3_albedo", mode="albedo", streams=3, fit_streams=3),
    case("fit_s3_emit", mode="emit_spheres", streams=3, fit_streams=3),
    # explicit paths in flight (params, config): the per-cast wavefront, refilling
    case("wf700_s1_side", wf=700, refills=True, streams=1, fit_streams=1),
    case("wf700_s3_side", wf=700, refills=True, streams=3, fit_streams=3),
    case("wf1500_s3_side", wf=1500, refills=True, streams=3, fit_streams=3),
    case("wf1500_s1_null", side=False, wf=1500, refills=True, streams=1, fit_streams=1),
    case("wf1500_s3_null_emit", mode="emit_spheres", side=False, wf=1500, refills=True, streams=3, fit_streams=3),
    case("wf700_s3_albedo", mode="albedo", wf=700, refills=True, streams=3, fit_streams=3),
    case("cfg_wf1500_s3", refills=True, wavefront_paths=1500, streams=3, fit_streams=3),
    # no fit rule: the per-cast wavefront with the whole job in flight
    case("fitpaths0_s3_side", fit_paths=0, streams=3, fit_streams=3),
    case("fitpaths0_s1_null", side=False, fit_paths=0, streams=1, fit_streams=1),
    case("drain_off", drain_q8=0, streams=3, fit_streams=3),
    # the memory rule, machine-independent: chunks of 2 samples, then below one chunk
    case("fitbytes_chunks_unit", fit_bytes=W * H * 2 * PER_PATH["unit"] + 10),
    case("fitbytes_chunks_emit_s3", mode="emit_spheres", fit_bytes=W * H * 2 * PER_PATH["emit_spheres"] + 10,
         streams=3, fit_streams=3),
    case("fitbytes_percast_unit", refills=True, fit_bytes=W * H * PER_PATH["unit"] // 2),
    case("fitbytes_percast_emit_s3", mode="emit_spheres", refills=True,
         fit_bytes=W * H * PER_PATH["emit_spheres"] // 2, streams=3, fit_streams=3),
    case("fitchunks_s3", fit_paths=W * H * 2, streams=3, fit_streams=3),
    case("fitchunks_off", refills=True, fit_paths=W * H * 2, fit_chunks=0),
    # two film chunks
    case("film2_albedo", mode="albedo", film_budget_bytes=12 * W * H * 3),
    case("film2_albedo_fused", mode="albedo", pipe="fused", film_budget_bytes=12 * W * H * 3),
    # the first cast and the forced drain
    case("lockstep0", drain_q8=1, drain_casts=1, lockstep_first=0),
    case("lockstep1_emit", mode="emit_spheres", drain_q8=1, drain_casts=1, lockstep_first=1),
    case("lockstep2", drain_q8=1, drain_casts=1, lockstep_first=2),
    case("lockstep3_s3", drain_q8=1, drain_casts=1, lockstep_first=3, streams=3, fit_streams=3),
    case("drain_casts0_s3", drain_casts=0, streams=3, fit_streams=3),
    case("drain_casts1_q1", drain_q8=1, drain_casts=1),
    case("drain_casts2_s3_emit", mode="emit_spheres", drain_casts=2, streams=3, fit_streams=3),
    # pipelines
    case("fused_unit_side", pipe="fused"),
    case("fused_emit_null", mode="emit_spheres", side=False, pipe="fused"),
    case("auto_unit", pipe=None),
    case("auto_wf700", pipe=None, wf=700, refills=True),
    case("auto_fused_max_1000", pipe=None, fused_max_paths=1000),
    case("cfg_pipeline_wavefront", pipe=None, pipeline=1),
    # a pass of a progressive render: samples [2, 6)
    case("accum_emit_s3", mode="emit_spheres", accum=True, streams=3, fit_streams=3),
    case("accum_unit_wf700", accum=True, wf=700, refills=True),
]


@pytest.fixture(scope="module")
def mesh():
    return scenes.mitsuba_synth(detail=0.25)


@pytest.fixture(scope="module")
def refs(mesh):
    """The oracle's film and ray casts per path mode (every case renders the same image)."""
    out = {}
    for mode in PER_PATH:
        mat = materials(mesh, mode)
        osc = O.OracleScene(mesh, albedo=mat.get("albedo"), emission=mat.get("emission"), spheres=mat.get("spheres"),
                            sphere_mat=mat.get("sphere_mat"), kinds=mat.get("kinds"))
        out[mode] = osc.render(O.reference_params(W, H, SPP, D, **KW))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def run_case(mesh, c):
    """The case's film (numpy) and the stats of its (last) render."""
    s = gpu_scene(mesh, materials(mesh, c["mode"]), **c["knobs"])
    stream = torch.cuda.Stream() if c["side"] else None
    params = sptamd.make_params(W, H, SPP, D, wavefront_paths=c["wf"], pipeline=c["pipe"], **KW)
    if c["accum"]:
        acc = s.accumulator(params)
        torch.cuda.synchronize()  # the planes are zeroed on torch's current stream
        acc.add(2, stream=stream)
        st = acc.add(SPP - 2, stream=stream)
        film = acc.film
    else:
        film, st = s.render(params, stream=stream)
    torch.cuda.synchronize()
    return film.cpu().numpy(), st


def compared(c, st):
    return {f: int(st[f]) for f in FIELDS + (() if c["refills"] else FIT_FIELDS)}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_render_plan_matches_parent(mesh, refs, golden, c, monkeypatch):
    for k in [k for k in list(os.environ) if k.startswith("SPT_")]:
        monkeypatch.delenv(k)
    film, st = run_case(mesh, c)
    ref, casts = refs[c["mode"]]
    np.testing.assert_array_equal(film, ref)
    if not c["accum"]:  # (a pass counts its own samples' work)
        assert st["ray_casts"] == casts
        assert_work_complete(st, H, W, SPP)
    got = compared(c, st)
    print(c["name"], got)
    assert got == golden[c["name"]]
