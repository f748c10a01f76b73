"""The structural BVH audit (tests/bvh_audit.py) itself, without a GPU: the host
builders' trees (tests/native/bvh_dump.cpp: build_bvh8 at width 8 and 6,
optimal and greedy collapse, as 80-B and 64-B nodes, and build_bvh; soups of 1,
9, 200 and 5000 triangles, as generated, with a zero-extent axis, a far
outlier, non-finite coordinates, and coordinates far below the ulp of their
box's origin) audit clean, and every single-field
mutation of the 200-triangle trees is reported under its rule's name."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bvh_audit as A
import test_scene_cache as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")
VARIANTS = ["plain", "flat z", "outlier", "non-finite", "tiny"]
BUILDS = ["w8 optimal", "w8 greedy", "w6 optimal", "w6 greedy", "w6 optimal 64-B", "w6 greedy 64-B", "bvh2"]


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """{(soup size, variant, build): (Tree, mesh)} from one run of bvh_dump."""
    d = tmp_path_factory.mktemp("bvh_dump")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    exe = d / "bvh_dump"
    srcs = [os.path.join(ROOT, "tests", "native", "bvh_dump.cpp"), os.path.join(CSRC, "bvh_build.cpp"),
            os.path.join(CSRC, "bvh8_build.cpp")]
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-I" + CSRC, "-o", str(exe)]
    cmd = [cxx, *flags, *srcs, "-lpthread"] if cxx else \
        ["/opt/rocm/bin/hipcc", *flags[:3], "-x", "c++", *flags[3:], *srcs, "-lpthread"]   # hipcc's host side
    subprocess.run(cmd, check=True, capture_output=True)
    res = subprocess.run([str(exe), str(d / "trees.bin")], capture_output=True, text=True)
    assert res.returncode == 0 and '"ok": 1' in res.stdout, res.stdout + res.stderr
    data = np.fromfile(d / "trees.bin", np.uint32)
    out, at = {}, 0
    while at < len(data):
        magic, fmt, stride, n, nn, leaves, depth, max_leaf, size, variant, build, _ = (int(x) for x in data[at:at + 12])
        assert magic == 0x44485642
        at += 12
        nodes = data[at:at + nn * stride].reshape(nn, stride)
        at += nn * stride
        slot2tri = data[at:at + n]
        at += n
        rec = data[at:at + 16 * n].view(np.float32).reshape(n, 16)
        at += 16 * n
        tv = data[at:at + 9 * n].view(np.float32)
        at += 9 * n
        o2s = np.empty(n, np.int32)
        o2s[slot2tri] = np.arange(n, dtype=np.int32)
        t = A.Tree(fmt, A.COMPACT, nodes, rec, o2s,
                   stats=dict(nodes=nn, leaves=leaves, max_depth=depth, max_leaf=max_leaf))
        mesh = {"pos": tv.reshape(-1, 3), "pos_tri": np.arange(3 * n).reshape(n, 3)}
        out[size, VARIANTS[variant], BUILDS[build]] = (t, mesh)
    assert len(out) == 4 * len(VARIANTS) * len(BUILDS)
    return out


@pytest.mark.parametrize("size", [1, 9, 200, 5000])
def test_host_trees_are_sound(dumped, size):
    for (n, variant, build), (t, mesh) in dumped.items():
        if n != size:
            continue
        info = {}
        A.assert_sound(t, mesh, f"{n} triangles, {variant}, {build}", info)
        # (max_slack is a float64 figure for reports: a step less 1e-30 reads as 1.0; the rule itself is exact)
        assert info["nodes"] == t.nodes.shape[0] and info["max_slack"] <= 1.0
        if t.fmt != 2 and variant != "non-finite" and size > 1:
            assert info["max_slack"] > 0.0            # the planes are quantised: some slack, under one step
    # the edge cases are what they claim to be: e = -100 and all bytes 0 on the flat axis
    t, _ = dumped[size, "flat z", "w8 optimal"]
    assert ((t.nodes[:, 3] >> 16) & 255 == 27).all()
    live = A._decode_wide(t, np.arange(t.nodes.shape[0]), A._Report())
    assert (live["qlo"][:, 2][live["live"]] == 0).all() and (live["qhi"][:, 2][live["live"]] == 0).all()
    t, _ = dumped[size, "non-finite", "w8 optimal"]
    assert (~np.isfinite(t.rec[:, :15])).sum() >= 3 and not np.isfinite(t.nodes[0, :3].view(np.float32)).all()


def test_parse_reads_the_cache_layout(tmp_path):
    """parse() against the file test_scene_cache.py writes from the documented layout."""
    secs = C.sections()
    t = A.parse(C.write(tmp_path / "ok.sptc", C.header(secs), secs))
    assert (t.fmt, t.shift, t.stack_depth) == (6, 0, 1) and t.stats["ntri"] == 2 and t.stats["bvh_width"] == 6
    assert t.nodes.shape == (1, 16) and t.nodes.tobytes() == secs[0]
    assert t.rec.tobytes() == secs[1] and t.snrm.tobytes() == secs[2] and t.orig2slot.tolist() == [1, 0]
    # a root without children: both triangles are in no leaf, the header's counts are off
    assert {"tri-coverage", "stats"} <= A.rules(A.audit(t))


# ---- the mutation matrix: one field of the 200-triangle tree changed, the matching rule reported

def byte_at(t, node, word, byte):
    return (int(t.nodes[node, word]) >> (8 * byte)) & 255


def set_byte(t, node, word, byte, value):
    assert 0 <= value <= 255
    w = int(t.nodes[node, word])
    t.nodes[node, word] = (w & ~(255 << (8 * byte))) | (value << (8 * byte))


def q_at(t, lohi, axis, c):
    """(word, byte) of child c's quantised lo (0) / hi (1) plane on an axis (bvh_build.h)."""
    if t.fmt == 8:
        return (8 if lohi == 0 else 14) + 2 * axis + (c >> 2), c & 3
    return (7 + 2 * axis + lohi, c) if c < 4 else (13 + axis, c - 4 + 2 * lohi)


def e_at(t, axis):
    return (3, axis) if t.fmt == 8 else [(5, 2), (5, 3), (6, 3)][axis]


def meta_at(t, c):
    if t.fmt == 8:
        return 6 + (c >> 2), c & 3
    return (4, c) if c < 4 else (5, c - 4)


def ulp_up(t, node, word, up=True):
    f = t.nodes[node, word:word + 1].view(np.float32)
    t.nodes[node, word] = np.nextafter(f, np.float32(np.inf if up else -np.inf)).view(np.uint32)[0]


def first_where(mask):
    ix = np.argwhere(mask)
    assert len(ix), "the tree has no place for this mutation: choose another tree"
    return tuple(int(i) for i in ix[0])


def mutate(t, what):
    """Apply one mutation in place; returns (the rule it must be reported under, the rules allowed beside it)."""
    any_rule = None
    n = t.nodes.shape[0]
    if t.fmt == 2:
        d = A._decode2(t, np.arange(n), A._Report())
        if what == "box inward":
            ulp_up(t, n // 2, 0, up=True)               # c0.lo.x
            return "enclosure", any_rule
        if what == "box outward":
            ulp_up(t, n // 2, 0, up=False)
            return "bvh2-tight", {"bvh2-tight"}
        if what == "leaf offset":
            node, c = first_where((d["kid"] < 0) & (d["first"] + d["count"] < t.rec.shape[0]))
            code = ~int(t.nodes[node:node + 1, 12 + c].view(np.int32)[0]) + 8
            t.nodes[node:node + 1, 12 + c].view(np.int32)[0] = ~code
            return "tri-coverage", any_rule
    else:
        d = A._decode_wide(t, np.arange(n), A._Report())
        live, qlo, qhi, meta = d["live"], d["qlo"], d["qhi"], d["meta"]          # q: (n, axis, child)
        wide = live[:, None, :] & (qhi > qlo)
        if what in ("qhi - 1", "qlo + 1"):
            node, axis, c = first_where(wide)
            lohi = 1 if what == "qhi - 1" else 0
            word, byte = q_at(t, lohi, axis, c)
            assert byte_at(t, node, word, byte) == int((qhi if lohi else qlo)[node, axis, c])
            set_byte(t, node, word, byte, byte_at(t, node, word, byte) + (-1 if lohi else 1))
            return "enclosure", any_rule
        if what in ("exponent - 1", "exponent + 1"):
            # + 1 keeps enclosing when every child starts at the origin on that axis (q * 2 step only grows hi)
            ok = wide.any(axis=2) if what == "exponent - 1" else \
                wide.any(axis=2) & (np.where(live[:, None, :], qlo, 0) == 0).all(axis=2)
            node, axis = first_where(ok)
            word, byte = e_at(t, axis)
            assert byte_at(t, node, word, byte) == int(d["eb"][node, axis])
            set_byte(t, node, word, byte, byte_at(t, node, word, byte) + (1 if what == "exponent + 1" else -1))
            return ("exponent", {"exponent", "tight-hi"}) if what == "exponent + 1" else ("enclosure", any_rule)
        if what == "origin":
            ulp_up(t, n // 2, 1)
            return "origin", any_rule
        leaf = live & (d["kid"] < 0)
        if what == "count bit":
            node, c = first_where(leaf & (d["count"] >= 2))
            word, byte = meta_at(t, c)
            m = byte_at(t, node, word, byte)
            assert m == int(meta[node, c])
            set_byte(t, node, word, byte, m & ~(1 << (4 + int(d["count"][node, c]))))    # the top count bit
            return "tri-coverage", any_rule
        if what == "leaf offset":
            node, c = first_where(leaf)
            word, byte = meta_at(t, c)
            set_byte(t, node, word, byte, byte_at(t, node, word, byte) + 1)
            return "leaf-offset", any_rule
        if what == "imask":
            node, c = first_where(d["kid"] >= 0)
            assert (int(t.nodes[node, 3]) >> (24 + c)) & 1
            t.nodes[node, 3] = int(t.nodes[node, 3]) & ~(1 << (24 + c))
            return "imask", {"imask"}
        if what == "empty slot":
            node, c = first_where(~live)
            word, byte = q_at(t, 0, 2, c)
            assert byte_at(t, node, word, byte) == 255
            set_byte(t, node, word, byte, 0)
            return "empty-slot-box", {"empty-slot-box"}
    if what == "orig2slot":
        assert len(t.orig2slot) > 77
        t.orig2slot[[3, 77]] = t.orig2slot[[77, 3]]
        return "orig2slot-id", {"orig2slot-id"}
    raise AssertionError(f"format {t.fmt} has no mutation {what!r}")


WIDE = ["qhi - 1", "qlo + 1", "exponent - 1", "exponent + 1", "origin", "count bit", "leaf offset", "orig2slot",
        "empty slot"]
# the greedy collapse makes leaves of two and three triangles (the optimal one prefers single triangles here)
MATRIX = ([("w8 greedy", m) for m in WIDE + ["imask"]] + [("w6 greedy 64-B", m) for m in WIDE] +
          [("bvh2", m) for m in ("box inward", "box outward", "leaf offset", "orig2slot")])


@pytest.mark.parametrize("build,what", MATRIX)
def test_mutation_is_reported(dumped, build, what):
    # a larger step keeps enclosing only where every child starts at the node's origin (q * 2 step > x
    # otherwise): the one-triangle tree; every other mutation has its place in the 200-triangle tree
    t, mesh = dumped[1 if what == "exponent + 1" else 200, "plain", build]
    t = t.copy()
    before = t.nodes.copy(), t.orig2slot.copy()
    rule, allowed = mutate(t, what)
    changed = int((before[0] != t.nodes).sum()) + int((before[1] != t.orig2slot).sum())
    assert changed == (2 if what == "orig2slot" else 1)       # a single field
    vs = A.audit(t, mesh)
    got = A.rules(vs)
    assert rule in got, (rule, [str(v) for v in vs[:10]])
    if allowed is not None:
        assert got <= allowed, [str(v) for v in vs[:10]]       # and nothing unrelated (tightness only, ...)
    named = [v for v in vs if v.rule == rule]
    assert all(v.detail for v in named)
    if rule in ("enclosure", "origin", "exponent", "bvh2-tight"):
        assert all(v.node >= 0 and v.axis >= 0 for v in named)   # the node and axis are named
    if rule in ("enclosure", "bvh2-tight", "leaf-offset", "imask", "empty-slot-box"):
        assert all(v.slot >= 0 for v in named if v.node >= 0)
