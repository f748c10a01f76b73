"""The node words the device writes, audited structurally (tests/bvh_audit.py:
topology, index arrays, records, exact float64 enclosure and tightness) instead
of through rays: trees built by both builders and re-laid by gpu_bvh8_holes at
every width and child-group packing, trees refitted by refit.hip after
deformations, on the smallest trees, on a cache-loaded scene and from device
arrays, and the refit of a mesh with NaN / +-inf vertices.  Each case is commit
-> save -> audit of the saved file; -s prints the node count and the largest
slack in quantisation steps."""
import numpy as np
import pytest
import torch

import bvh_audit as A
import sptamd
import test_gpu_build as B
import test_gpu_refit as R
from sptamd import scenes

pytestmark = pytest.mark.gpu

HOST, GPU = R.HOST, R.GPU


def audited(s, mesh, path, what):
    """Save the scene, audit the file against the mesh; returns the parsed tree."""
    s.save(str(path))
    t = A.parse(path)
    info = {}
    A.assert_sound(t, mesh, what, info)
    st = s.backend.stats
    assert t.stats["bvh_width"] == st["bvh_width"] and t.stats["ntri"] == len(np.asarray(mesh["pos_tri"]).reshape(-1, 3))
    assert info["nodes"] == st["nodes"] and info["max_slack"] <= 1.0
    print(f"{what}: {info['nodes']} nodes in {t.nodes.shape[0]} slots, {info['levels']} levels, "
          f"largest slack {info['max_slack']:.6f} steps")
    return t


def config(width, build, pack, collapse=None):
    cfg = R.config(width, build, pack)
    if collapse is not None:
        cfg.collapse = collapse
    return cfg


# ---- built trees

@pytest.mark.parametrize("width,build,pack", R.CONFIGS)
def test_built(width, build, pack, tmp_path):
    m = R.mesh_at(None)
    t = audited(R.scene(config(width, build, pack), m, with_albedo=False), m, tmp_path / "a.sptc",
                f"built {width} {build} {pack}")
    assert t.fmt == width and (t.fmt == 2 or t.shift == (0 if pack else 3))


@pytest.mark.parametrize("width", [6, 8])
@pytest.mark.parametrize("build", [HOST, GPU])
def test_built_greedy_collapse(width, build, tmp_path):
    m = R.mesh_at(None)
    audited(R.scene(config(width, build, 1, collapse=1), m, with_albedo=False), m, tmp_path / "a.sptc",
            f"built greedy {width} {build}")


def tiny_kinds():
    """The four meshes of test_gpu_build.py::test_gpu_build_small_and_degenerate."""
    one = [[[-1, 0, -1], [1, 0, -1], [0, 0, 1]]]
    three = one + [[[-1, 1, -1], [1, 1, -1], [0, 1, 1]], [[-1, -1, -1], [1, -1, -1], [0, -1, 1]]]
    grid = [[[i * 0.1 - 2, 0, j * 0.1 - 2], [i * 0.1 - 2 + 0.1, 0, j * 0.1 - 2], [i * 0.1 - 2, 0, j * 0.1 - 2 + 0.1]]
            for i in range(40) for j in range(40)]
    return {"one": one, "three": three, "stacked": one * 50, "grid": grid}


@pytest.mark.parametrize("build", [HOST, GPU])
@pytest.mark.parametrize("kind", ["one", "three", "stacked", "grid"])
def test_built_small_and_degenerate(kind, build, tmp_path):
    m = B.tiny_mesh(tiny_kinds()[kind])
    s = B.make_scene(m, build)
    assert s.backend.stats["builder"] == build
    t = audited(s, m, tmp_path / "a.sptc", f"built {kind} {build}")
    if kind == "grid" and t.fmt != 2:                     # the zero-extent axis: e = -100, every byte 0
        d = A._decode_wide(t, np.array([0]), A._Report())
        assert d["eb"][0, 1] == 27 and (d["qhi"][0, 1][d["live"][0]] == 0).all()


def test_built_city(tmp_path):
    """A large coordinate range with small boxes far from the origin."""
    m = scenes.city_synth(20_000)
    s = B.make_scene(m, GPU)
    assert s.backend.stats["builder"] == GPU
    audited(s, m, tmp_path / "a.sptc", "built city")


# ---- refitted trees

@pytest.mark.parametrize("width,build,pack", R.CONFIGS)
def test_refitted(width, build, pack, tmp_path):
    m = R.mesh_at(None)
    s = R.scene(config(width, build, pack), m, with_albedo=False)
    built = audited(s, m, tmp_path / "a.sptc", f"built {width} {build} {pack}")
    for phase in (0.7, 1.9, 3.1):
        s.update_geometry(R.deformed_pos(phase), m["nrm"])
        t = audited(s, R.mesh_at(phase), tmp_path / "b.sptc", f"refitted {width} {build} {pack} phase {phase}")
        assert not np.array_equal(t.nodes, built.nodes) and t.nodes.shape == built.nodes.shape


@pytest.mark.parametrize("width", [8, 6, 2])
@pytest.mark.parametrize("name", ["point", "plane"])
def test_refitted_smallest_trees(width, name, tmp_path):
    """The point and plane updates of test_gpu_refit.py::test_smallest_trees."""
    pos, tri = R.tiny_meshes()["nine" if name == "point" else name]
    tri = np.ascontiguousarray(tri, np.int32)
    rng = np.random.default_rng(5)
    if name == "point":
        new = np.tile(np.float32([0.3, 0.9, -0.2]), (len(pos), 1))        # every vertex at one point
    else:
        new = pos.copy()
        new[:, [0, 2]] += rng.uniform(-0.3, 0.3, size=(len(pos), 2)).astype(np.float32)
        new[:, 1] = np.float32(0.5)                                       # still one plane: zero extent in y
    s = R.scene(config(width, HOST, 1), {"pos": pos, "pos_tri": tri}, with_albedo=False)
    s.update_geometry(new)
    audited(s, {"pos": new, "pos_tri": tri}, tmp_path / "a.sptc", f"refitted {name} {width}")


def test_refitted_cache_loaded(tmp_path):
    m = R.mesh_at(None)
    R.scene(config(6, GPU, 2), m, with_albedo=False).save(str(tmp_path / "a.sptc"))
    s = sptamd.Scene.load(str(tmp_path / "a.sptc"))
    s.update_geometry(R.deformed_pos(0.7), m["nrm"], pos_tri=m["pos_tri"], nrm_tri=m["nrm_tri"])
    audited(s, R.mesh_at(0.7), tmp_path / "b.sptc", "refitted after a cache load")


def test_refitted_from_device_arrays(tmp_path):
    m = R.mesh_at(None)
    s = R.scene(config(8, GPU, 1), m, with_albedo=False)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()  # noqa: E731
    s.update_geometry(up(R.deformed_pos(1.9), np.float32), up(m["nrm"], np.float32), pos_tri=up(m["pos_tri"], np.int32),
                      nrm_tri=up(m["nrm_tri"], np.int32))
    torch.cuda.synchronize()
    audited(s, R.mesh_at(1.9), tmp_path / "a.sptc", "refitted from device arrays")


# ---- the non-finite update

@pytest.mark.parametrize("width,build", [(6, HOST), (8, HOST), (6, GPU), (8, GPU)])
def test_non_finite_update(width, build, tmp_path):
    """test_gpu_refit.py::test_non_finite_positions_do_not_fault's mesh: the
    finite triangles stay enclosed (an axis whose frame origin is not finite
    counts as unbounded, bvh_audit.py) and reachable."""
    m = R.mesh_at(None)
    s = R.scene(config(width, build, 1), m, with_albedo=False)
    pos = R.non_finite_pos()
    s.update_geometry(pos, m["nrm"])
    t = audited(s, dict(m, pos=pos), tmp_path / "a.sptc", f"non-finite update {width} {build}")
    assert not np.isfinite(t.nodes[0, :3].view(np.float32)).all()         # the -inf vertex reached the root's frame
    R.assert_non_finite_hits(s)
    s.update_geometry(R.deformed_pos(0.7), m["nrm"])                     # and the tree recovers, exactly
    audited(s, R.mesh_at(0.7), tmp_path / "b.sptc", f"recovered {width} {build}")
