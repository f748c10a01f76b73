"""The scenes of tests/test_specular_ref.py and tests/test_gpu_specular_sampling.py: glass and
mirror, on triangles and on analytic spheres, textures and triangles without vertex normals,
under light sampling, sky sampling and MIS.

  specular   cornell_spheres(0.05) with its tessellated balls (material 4) of glass, the left
             wall emitting (0.3, 0.2, 0.1) beside the cap, and three analytic spheres: a glass
             and a mirror ball in the room and a glass ball around the camera, so that every
             path starts with two glass vertices
  dark       the same without emission: the sky is the only light
  textured   the same with planar texcoords and images on the left wall and the white material
  no_normals / some_normals
             the same without nrm_tri / with index -1 on every third triangle
  moved      one of the two tessellated glass balls moved
  smallpt    scenes.smallpt_analytic(0.05) — its light is a sphere and is never sampled — and an
             emissive quad under the ceiling
"""
import functools

import numpy as np

import accum_ref as A
import mis_ref as M
import oracle as O
from sptamd import _lib, scenes
from test_gpu_mis import DARK, ONE, PLANES, ROT, TEX, TINT

F = np.float32
W, H, SPP, DEPTH = 37, 19, 8, 7
DETAIL = 0.05
CAM = scenes.cornell_camera()
KW = dict(rr_start_depth=2)
MIRROR, GLASS = 6, 7                       # the two appended materials of the analytic spheres
SPHERES = np.array([[0.6, 0.6, 0.9, 0.1], [0.35, 0.62, 0.9, 0.12], [0.5, 0.52, 2.9, 0.12]], F)
SPHERE_MAT = np.array([GLASS, MIRROR, GLASS], np.int32)


def textures():
    """test_gpu_textures.textures()' kinds of image, on the left wall (1) and the white material (3)."""
    rng = np.random.default_rng(3)
    return {1: scenes.checker(8, 8, cell=1),                                 # square
            3: rng.uniform(0.1, 0.95, size=(5, 3, 3)).astype(F)}             # 3 wide, 5 high


@functools.lru_cache(maxsize=None)
def _specular():
    m = dict(scenes.cornell_spheres(DETAIL))
    kd, ke = scenes.smallpt_materials(m)
    kd = np.concatenate([kd, np.array([[0.999, 0.999, 0.999], [0.9, 0.95, 0.999]], F)])
    ke = np.concatenate([ke, np.zeros((2, 3), F)])
    ke[1] = (0.3, 0.2, 0.1)
    kinds = np.zeros(len(kd), np.uint32)
    kinds[4] = kinds[GLASS] = _lib.SPT_MAT_GLASS
    kinds[MIRROR] = _lib.SPT_MAT_MIRROR
    m.update(kinds=kinds, spheres=SPHERES, sphere_mat=SPHERE_MAT)
    return m, kd, ke


@functools.lru_cache(maxsize=None)
def _smallpt():
    m = dict(scenes.smallpt_analytic(DETAIL))
    kd, ke = scenes.smallpt_materials(m)
    quad = len(kd)
    kd = np.concatenate([kd, np.zeros((1, 3), F)])
    ke = np.concatenate([ke, np.array([[9.0, 8.0, 6.0]], F)])
    nv, nn = len(m["pos"]), len(m["nrm"])
    m["pos"] = np.concatenate([m["pos"], np.array([[0.38, 0.8, 0.68], [0.62, 0.8, 0.68], [0.62, 0.8, 0.95], [0.38, 0.8, 0.95]], F)])
    m["nrm"] = np.concatenate([m["nrm"], np.array([[0.0, -1.0, 0.0]], F)])
    m["pos_tri"] = np.concatenate([m["pos_tri"], np.array([[nv, nv + 1, nv + 2], [nv, nv + 2, nv + 3]], np.int32)])
    m["nrm_tri"] = np.concatenate([m["nrm_tri"], np.full((2, 3), nn, np.int32)])
    m["mat_id"] = np.concatenate([m["mat_id"], np.full(2, quad, np.int32)])
    m["kinds"] = np.concatenate([m["kinds"], np.zeros(1, np.uint32)])
    return m, kd, ke


def variant(name):
    """(mesh, albedo, emission, textures) of the named scene."""
    if name == "smallpt":
        return _smallpt() + (None,)
    m, kd, ke = _specular()
    m, tex = dict(m), None
    if name == "dark":
        ke = np.zeros_like(ke)
    elif name == "camera_outside":                # without the glass ball around the camera
        m.update(spheres=SPHERES[:2], sphere_mat=SPHERE_MAT[:2])
    elif name == "textured":
        m, tex = scenes.with_planar_uv(m, scale=1.0, offset=(0.0, 0.0)), textures()
    elif name in ("no_normals", "some_normals"):
        # wound so that the geometric normal points where the vertex normals do: a wall whose
        # substitute normal faced out of the room would send its bounce rays out of the scene
        pt, nt = (np.array(m[k], np.int32).reshape(-1, 3) for k in ("pos_tri", "nrm_tri"))
        v = m["pos"][pt].astype(np.float64)
        back = np.einsum("ij,ij->i", np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), m["nrm"][nt[:, 0]]) < 0
        pt[back], nt[back] = pt[back][:, [0, 2, 1]], nt[back][:, [0, 2, 1]]
        m["pos_tri"] = pt
        if name == "no_normals":
            del m["nrm_tri"], m["nrm"]
        else:
            nt[::3] = -1
            m["nrm_tri"] = nt
    elif name == "moved":                         # the tessellated glass ball at x = 0.73: up and toward the camera
        pos = m["pos"].copy()
        tris = np.nonzero(m["mat_id"] == 4)[0]
        sel = np.unique(m["pos_tri"][tris[len(tris) // 2:]])
        assert pos[sel, 0].min() > 0.5
        pos[sel] += np.array([-0.1, 0.08, 0.3], F)
        m["pos"] = pos
    else:
        assert name == "specular"
    return m, kd, ke, tex


# what a test renders: the scene, the sky image (None: the constant env), the samplers, the share, MIS, env
CASES = {
    "spec_off": dict(name="specular", tex=None, nee=False, sky=False, share=0.5, mis=False, env=DARK),
    "spec_lights": dict(name="specular", tex=None, nee=True, sky=False, share=0.5, mis=False, env=DARK),
    "spec_lights_mis": dict(name="specular", tex=None, nee=True, sky=False, share=0.5, mis=True, env=DARK),
    "spec_sky": dict(name="dark", tex="sun", nee=False, sky=True, share=0.5, mis=False, env=ONE),
    "spec_both": dict(name="specular", tex="sun", nee=True, sky=True, share=0.25, mis=False, env=TINT),
    "spec_both_mis": dict(name="specular", tex="sun", nee=True, sky=True, share=0.25, mis=True, env=TINT),
    "spec_both_off": dict(name="specular", tex="sun", nee=False, sky=False, share=0.25, mis=False, env=TINT),
    "smallpt_lights": dict(name="smallpt", tex=None, nee=True, sky=False, share=0.5, mis=False, env=DARK),
    "smallpt_lights_mis": dict(name="smallpt", tex=None, nee=True, sky=False, share=0.5, mis=True, env=DARK),
    "textured_lights_mis": dict(name="textured", tex=None, nee=True, sky=False, share=0.5, mis=True, env=DARK),
    "textured_sky_mis": dict(name="textured", tex="sun", nee=False, sky=True, share=0.5, mis=True, env=ONE),
    "untextured_lights_mis": dict(name="specular", tex=None, nee=True, sky=False, share=0.5, mis=True, env=DARK),
    "no_normals": dict(name="no_normals", tex=None, nee=True, sky=False, share=0.5, mis=True, env=DARK),
    "some_normals": dict(name="some_normals", tex=None, nee=True, sky=False, share=0.5, mis=True, env=DARK),
    "moved": dict(name="moved", tex=None, nee=True, sky=False, share=0.5, mis=True, env=DARK),
    # the statistical test: under the broad sky image, and the same with the camera outside its glass ball
    "expect": dict(name="specular", tex="dim", nee=True, sky=True, share=0.5, mis=True, env=ONE),
    "expect_outside": dict(name="camera_outside", tex="dim", nee=True, sky=True, share=0.5, mis=True, env=ONE),
}


def oparams(case, w=W, h=H, spp=SPP):
    return O.reference_params(w, h, spp, DEPTH, camera=CAM, env=CASES[case]["env"], **KW)


def sky_of(case):
    c = CASES[case]
    return None if c["tex"] is None else (TEX[c["tex"]], ROT)


@functools.lru_cache(maxsize=None)
def expected(case):
    """The planes, the contributions and the counts of the restatement (mis_ref)."""
    c = CASES[case]
    m, kd, ke, tex = variant(c["name"])
    count = {}
    x = M.contributions(m, oparams(case), kd, ke, sky=sky_of(case), nee=c["nee"], sky_on=c["sky"], share=c["share"],
                        mis=c["mis"], count=count, textures=tex)
    assert np.isfinite(x).all()
    x.setflags(write=False)
    return dict(zip(PLANES, A.moments(x))), x, count
