"""A structural audit of BVH node arrays in exact float64 arithmetic (a helper
module, not a test).

Every other check of an acceleration structure in this suite goes through
rays; this one reads the node words themselves — from a scene cache file that
the public save wrote (parse), or from the host builders' raw output (Tree) —
and returns a list of named violations (audit).  The tree is walked level by
level with numpy, children first on the way back up, so a mesh of tens of
thousands of triangles takes well under a second.

Formats (decoded from their documentation, not from the builders' code):
  8   the 80-B eight-wide node            bvh_build.h:42-52
  6   the 64-B six-wide node              bvh_build.h:64-73
  2   the BVH2 node                       bvh_build.h:4-10
An inner child of a wide node sits at (group << group_shift) + s with s the
octant slot in its meta byte (bvh_build.h:46-47, :71; kernels.hip:647), or,
with shift = COMPACT, the r-th inner child in slot order at group + r (the
builders' own layout: bvh_build.h:45, bvh_refit.h:33-35, :85 kRefitCompact).

All arithmetic is exact.  float32 values are widened to float64.  A decoded
plane p + q * 2^(e-127) (p float32, q <= 255) is exact in float64 whenever p
and the step are of comparable magnitude, which the frame guarantees except
for an origin far smaller than the step (p = -1e-30 under a step of 2^-7):
the sum's rounding error is therefore kept beside it (two-sum), and enclosure
compares the pair: the rounded plane decides unless it equals the coordinate,
then the error's sign does.  The tightness bounds subtract (x - plane < step),
which may round, but only towards a report: every candidate is confirmed in
rational arithmetic before it is listed.

Rules (the name each violation carries, and where the rule comes from):

 Topology
  node-range      an inner child index lies in the node array (scene_cache.cpp cache_check_nodes)
  node-twice      every reachable node slot is reached once (cache_check_nodes)
  leaf-count      a wide leaf's count bits are unary, 1..3 triangles
                  (bvh_build.h:49, bvh8_build.cpp:304); a BVH2 leaf holds
                  1..kMaxLeafSize (bvh_build.h:10, :17: three count bits)
  leaf-range      a leaf's triangle slots lie in [0, ntri) (cache_check_nodes)
  leaf-offset     a wide node's leaf offsets are contiguous in slot order from
                  tri_base (bvh_build.h:48, bvh8_build.cpp:274-306)
  tri-coverage    every triangle slot belongs to exactly one leaf
  inner-meta      an inner meta byte is 0b001_(24 + s); in the 80-B node s is
                  its own slot, in the 64-B node the slots of a node's inner
                  children are distinct (bvh_build.h:49, :69; bvh8_build.cpp:298)
  imask           80-B node: imask bit s is set exactly when meta[s] is an
                  inner meta byte (bvh_build.h:45, bvh8_build.cpp:297)
  empty-slot-box  an empty slot carries the inverted box 255 / 0
                  (bvh8_build.cpp:272, bvh_refit.h:167)
  stats           the node, leaf, depth and leaf-size counts of the walk equal
                  the header's scene stats.  (max_leaf of a wide tree is the
                  format's constant 3 in the stats, capi.cpp spt_scene_create_cfg: the
                  walk's largest leaf must not exceed it; BVH2: equal.)
  stack-depth     the stack the header declares holds the tree: BVH2 one entry
                  per node level, a wide tree levels - 1, at least 1
                  (cache_check_nodes)
 Index arrays
  orig2slot-perm  orig2slot is a permutation of the slots (cache_check_indices)
  orig2slot-id    float 15 of record orig2slot[i] holds i (spt_internal.h:24-34)
 Records (with a mesh)
  record          every slot's record equals tri_record_fill of the mesh's
                  current vertices of its original triangle, bit for bit
                  (spt_internal.h:25-34)
  normal          supplied vertex normals and the material id in .w of the first
                  normal equal the mesh's, bit for bit (spt_internal.h:85,
                  capi.cpp spt_scene_create_cfg).  Geometric normals made for missing
                  vertex normals are not checked here.
 Enclosure
  enclosure       for every child of every node the decoded box encloses every
                  vertex of every finite triangle below that child, per axis:
                  lo_dec <= min and hi_dec >= max.  A triangle with any
                  non-finite coordinate is left out (it is never hit).  An
                  axis on which the node's frame origin is not finite counts
                  as unbounded: in visit_words (kernels.hip:536-561) and
                  visit_words6 (kernels.hip:494-522, the only six-wide visit
                  routine the kernels have) the slab offset b = (p - o) / d is
                  then +-inf and the margin |b| * kMarginRel is +inf, so of b -
                  m and b + m one is NaN and the other infinite with b's sign;
                  the entry plane is NaN or -inf, the exit plane NaN or +inf,
                  and fmaxf (:521 / :560) / fminf (:522 / :561) drop exactly
                  those.  BVH2: the stored float boxes enclose likewise.
 Tightness (derived from emit(), bvh8_build.cpp:249-295, so exact bounds)
  origin          the node origin is the exact float32 minimum of its subtree
                  on each axis (bvh8_build.cpp:206-211, :266)
  tight-lo/-hi    min < lo_dec + step and max > hi_dec - step, step = 2^(e-127)
                  of the node and axis (floor / ceil held to the exact planes,
                  bvh8_build.cpp:282-288)
  exponent        the exponent is minimal, lo + 255 * 2^(e-1) < hi, unless e sits
                  at the clamp -100 or ext is 0 (then e = -100); a non-finite
                  extent has e = 127 (bvh8_build.cpp:254-264)
  bvh2-tight      BVH2: each stored child box is the exact union of its
                  subtree (bvh_build.cpp:72-76, :196-198)
  Tightness is skipped for nodes whose subtree holds a non-finite triangle
  (the builders' fminf / fmaxf unions take such a triangle's finite
  coordinates and infinities along; the audit leaves the triangle out).

A BVH2 scene of one leaf has a root whose two codes are that leaf, the second
behind a far-away point box (bvh_build.cpp:236-248): that second child is
skipped.
"""
import ctypes
from collections import namedtuple
from fractions import Fraction
from ctypes import c_char, c_uint32, c_uint64

import numpy as np

from sptamd import _lib

SECTIONS = ["nodes", "triangles", "normals", "texcoords", "orig2slot", "albedo", "emission", "spheres",
            "sphere materials", "material kinds", "texture sizes", "texels", "extra"]
TRI_QUADS, NODE6_QUADS, NODE8_QUADS = 4, 4, 8   # spt_internal.h kTriQuads / kNode6Quads / kNode8Quads
CACHE_VERSION = 2               # scene_cache.cpp kCacheVersion (2: 64-B rotated triangle records)
COMPACT = 0xffffffff            # bvh_refit.h kRefitCompact
MAX_LEAF2 = 8                   # bvh_build.h kMaxLeafSize
REPORT_CAP = 20                 # entries listed per rule and level (the audit still fails on one)


def tri_records(v9, ids):
    """spt_internal.h tri_record_fill: per triangle 16 floats, each vertex as
    x y z x y, the original id's bits in float 15."""
    v = np.asarray(v9, np.float32).reshape(-1, 3, 3)
    rec = np.zeros((v.shape[0], 16), np.float32)
    for k in range(3):
        rec[:, 5 * k:5 * k + 3] = v[:, k]
        rec[:, 5 * k + 3:5 * k + 5] = v[:, k, :2]
    rec[:, 15] = np.asarray(ids, np.uint32).view(np.float32)
    return rec


class Header(ctypes.Structure):
    _fields_ = ([("magic", c_char * 8)] +
                [(n, c_uint32) for n in ("version", "header_bytes", "tri_quads", "node_quads", "node6",
                                         "group_shift", "config_bytes", "stats_bytes", "stack_depth", "nmat",
                                         "nemit", "nsph", "nkind", "ntexmat")] +
                [("ntri", c_uint64), ("bytes", c_uint64 * 13), ("sum", c_uint64 * 13),
                 ("cfg", _lib.Config), ("stats", _lib.SceneStats)])


Violation = namedtuple("Violation", "rule node slot axis detail")
Violation.__str__ = lambda v: (f"{v.rule}: node {v.node} child {v.slot} axis {'xyz-'[v.axis]} {v.detail}")


class Tree:
    """Node words and triangle records of one tree.
    fmt 8 / 6 / 2; shift: group_shift or COMPACT; nodes: uint32 (slots, words
    per slot); rec: float32 (ntri, 16); snrm: float32 (ntri, 3, 4) or None;
    orig2slot: int32 (ntri) or None; stats: dict with nodes / leaves /
    max_depth / max_leaf or None; stack_depth: int or None."""

    def __init__(self, fmt, shift, nodes, rec, orig2slot=None, snrm=None, stats=None, stack_depth=None,
                 header=None):
        self.fmt, self.shift = int(fmt), int(shift)
        self.nodes = np.ascontiguousarray(nodes, np.uint32)
        self.rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 16)
        self.orig2slot = None if orig2slot is None else np.ascontiguousarray(orig2slot, np.int32)
        self.snrm = None if snrm is None else np.ascontiguousarray(snrm, np.float32).reshape(-1, 3, 4)
        self.stats, self.stack_depth, self.header = stats, stack_depth, header

    def copy(self):
        return Tree(self.fmt, self.shift, self.nodes.copy(), self.rec.copy(),
                    None if self.orig2slot is None else self.orig2slot.copy(),
                    None if self.snrm is None else self.snrm.copy(), self.stats, self.stack_depth, self.header)


def parse(path):
    """A scene cache file (spt_scene_save) as a Tree; its Header is tree.header."""
    data = open(path, "rb").read()
    h = Header.from_buffer_copy(data[:ctypes.sizeof(Header)])
    assert h.magic == b"SPTSCENE" and h.version == CACHE_VERSION and h.header_bytes == ctypes.sizeof(Header), path
    assert h.tri_quads == TRI_QUADS
    off, sec = ctypes.sizeof(Header), {}
    for name, n in zip(SECTIONS, h.bytes):
        sec[name] = data[off:off + n]
        off += n
    assert off == len(data), "the sections do not add up to the file"
    width = h.stats.bvh_width
    fmt = 2 if width == 2 else (6 if h.node6 else 8)
    assert h.node_quads == {2: 4, 6: NODE6_QUADS, 8: NODE8_QUADS}[fmt]
    ntri = h.ntri
    nodes = np.frombuffer(sec["nodes"], np.uint32).reshape(-1, h.node_quads * 4)
    rec = np.frombuffer(sec["triangles"], np.float32).reshape(ntri, 16)
    snrm = np.frombuffer(sec["normals"], np.float32).reshape(ntri, 3, 4)
    o2s = np.frombuffer(sec["orig2slot"], np.int32)
    return Tree(fmt, h.group_shift, nodes, rec, o2s, snrm, h.stats.as_dict(), h.stack_depth, h)


def _bytes(words):
    """(n, k) uint32 -> (n, 4 k) bytes, low byte first."""
    return np.ascontiguousarray(words, "<u4").view(np.uint8).reshape(words.shape[0], -1)


def _f32(words):
    return np.ascontiguousarray(words, np.uint32).view(np.float32).astype(np.float64)


class _Report:
    def __init__(self):
        self.out = []

    def add(self, rule, mask, nodes, detail, axis_dim=None, confirm=None):
        """mask: (n,), (n, K) or (n, A, K) / (n, K, A) booleans; one entry per set element, at most
        REPORT_CAP.  axis_dim: which dimension of the mask is the axis.  detail(index tuple) -> str.
        confirm(index tuple) -> bool: the same rule in rational arithmetic, for a float64 test that may round."""
        idx = [tuple(int(i) for i in ix) for ix in np.argwhere(mask)]
        listed = 0
        for n, ix in enumerate(idx):
            if listed == REPORT_CAP:
                self.out.append(Violation(rule, -1, -1, -1, f"... and up to {len(idx) - n} more on this level"))
                break
            if confirm is not None and not confirm(ix):
                continue
            slot = axis = -1
            if len(ix) == 2 and axis_dim == 1:
                axis = ix[1]
            elif len(ix) == 2:
                slot = ix[1]
            elif len(ix) == 3:
                axis, slot = (ix[1], ix[2]) if axis_dim == 1 else (ix[2], ix[1])
            self.out.append(Violation(rule, int(nodes[ix[0]]), slot, axis, detail(ix)))
            listed += 1

    def one(self, rule, detail, node=-1, slot=-1, axis=-1):
        self.out.append(Violation(rule, node, slot, axis, detail))


def _two_sum(a, b):
    """a + b rounded, and the rounding error (Knuth): the pair is the exact sum."""
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    return s, np.where(np.isfinite(s), err, 0.0)


def _decode_wide(t, ids, rep):
    """The children of wide nodes `ids`: a dict of per-node arrays, K = 8 or 6 children."""
    w = t.nodes[ids]
    n = len(ids)
    origin = _f32(w[:, 0:3])
    if t.fmt == 8:
        eb = (w[:, 3:4] >> np.array([0, 8, 16], np.uint32)) & 255
        imask, group, tri_base = w[:, 3] >> 24, w[:, 4].astype(np.int64), w[:, 5].astype(np.int64)
        meta = _bytes(w[:, 6:8])
        qlo, qhi = _bytes(w[:, 8:14]).reshape(n, 3, 8), _bytes(w[:, 14:20]).reshape(n, 3, 8)
    else:
        eb = np.stack([(w[:, 5] >> 16) & 255, w[:, 5] >> 24, w[:, 6] >> 24], 1)
        imask, group, tri_base = None, (w[:, 6] & 0x00ffffff).astype(np.int64), w[:, 3].astype(np.int64)
        meta = np.concatenate([_bytes(w[:, 4:5]), _bytes(w[:, 5:6])[:, :2]], 1)
        q03 = _bytes(w[:, 7:13]).reshape(n, 3, 2, 4)     # [axis][lo, hi][child 0..3]
        q45 = _bytes(w[:, 13:16]).reshape(n, 3, 4)       # [axis][lo4 lo5 hi4 hi5]
        qlo = np.concatenate([q03[:, :, 0], q45[:, :, 0:2]], 2)
        qhi = np.concatenate([q03[:, :, 1], q45[:, :, 2:4]], 2)
    K = meta.shape[1]
    meta = meta.astype(np.int64)
    inner = (meta & 0x18) == 0x18          # as the tracer reads it (kernels.hip:467-474)
    leaf = (meta != 0) & ~inner
    empty = meta == 0
    s_of = meta & 7
    # inner meta bytes: 0b001_(24 + s)
    bad_meta = inner & ((meta >> 5) != 1)
    if t.fmt == 8:
        bad_meta |= inner & (s_of != np.arange(8))
        im = ((imask[:, None] >> np.arange(8, dtype=np.uint32)) & 1).astype(bool)
        rep.add("imask", im != inner, ids, lambda ix: f"imask {int(imask[ix[0]]):#04x} meta {int(meta[ix]):#04x}")
    else:
        occ = np.zeros((n, 8), np.int64)
        np.add.at(occ, (np.nonzero(inner)[0], s_of[inner]), 1)
        bad_meta |= inner & (np.take_along_axis(occ, s_of, 1) > 1)
    rep.add("inner-meta", bad_meta, ids, lambda ix: f"meta {int(meta[ix]):#04x}")
    rank = np.cumsum(inner, 1) - 1
    if t.shift == COMPACT:
        kid = group[:, None] + rank
    else:
        kid = (group[:, None] << t.shift) + s_of
    kid = np.where(inner, kid, -1)
    # leaves: unary(count) << 5 | offset, contiguous from tri_base in slot order
    cbits = meta >> 5
    count = np.where(leaf, np.array([0, 1, 1, 2, 1, 2, 2, 3])[cbits], 0)   # popcount, as the tracer and the refit read it
    unary = (cbits == 1) | (cbits == 3) | (cbits == 7)
    rep.add("leaf-count", leaf & ~unary, ids, lambda ix: f"count bits {int(cbits[ix]):#05b}")
    offset = meta & 31
    want = np.cumsum(count, 1) - count
    rep.add("leaf-offset", leaf & (offset != want), ids,
            lambda ix: f"offset {int(offset[ix])}, the leaves before it hold {int(want[ix])}")
    first = np.where(leaf, tri_base[:, None] + offset, 0)
    rep.add("empty-slot-box", empty[:, None, :] & ((qlo != 255) | (qhi != 0)), ids,
            lambda ix: f"qlo {int(qlo[ix])} qhi {int(qhi[ix])}", axis_dim=1)
    step = np.ldexp(1.0, eb.astype(np.int64) - 127)
    with np.errstate(invalid="ignore", over="ignore"):
        lo_dec, lo_err = _two_sum(origin[:, :, None], qlo * step[:, :, None])
        hi_dec, hi_err = _two_sum(origin[:, :, None], qhi * step[:, :, None])
    return dict(ids=ids, K=K, kid=kid, first=first, count=count, live=~empty, origin=origin, eb=eb.astype(np.int64),
                step=step, qlo=qlo, qhi=qhi, meta=meta, lo_err=lo_err, hi_err=hi_err, lo_dec=np.swapaxes(lo_dec, 1, 2), hi_dec=np.swapaxes(hi_dec, 1, 2))


def _decode2(t, ids, rep):
    w = t.nodes[ids]
    n = len(ids)
    code = w[:, 12:14].view(np.int32).astype(np.int64)
    inner = code >= 0
    l = (~code) & 0xffffffff
    kid = np.where(inner, code, -1)
    first = np.where(inner, 0, l >> 3)
    count = np.where(inner, 0, (l & 7) + 1)
    f = _f32(w[:, 0:12])
    at = np.array([[[0, 1], [2, 3], [8, 9]], [[4, 5], [6, 7], [10, 11]]])   # [child][axis][lo, hi]
    lo_dec, hi_dec = f[:, at[:, :, 0]], f[:, at[:, :, 1]]                    # (n, 2, 3)
    live = np.ones((n, 2), bool)
    live[:, 1] &= ~((w[:, 12] == w[:, 13]) & ~inner[:, 0])                   # the far copy of a root leaf
    count = np.where(live, count, 0)
    return dict(ids=ids, K=2, kid=np.where(live, kid, -1), first=first, count=count, live=live, lo_dec=lo_dec,
                hi_dec=hi_dec)


def audit(t, mesh=None, info=None):
    """All violations of the rules in the module docstring, as a list of
    Violation(rule, node, slot, axis, detail); empty: the tree is sound.
    mesh: a dict with pos / pos_tri (and nrm / nrm_tri / mat_id) for the record
    rules.  info: a dict that receives nodes, leaves, levels, max_leaf and
    max_slack (the largest distance between a stored plane and the geometry
    it bounds, in quantisation steps; wide trees)."""
    rep = _Report()
    ntri = t.rec.shape[0]
    nslots = t.nodes.shape[0]
    if ntri == 0:
        return rep.out
    # ---- triangles: exact boxes of the finite ones
    v = t.rec[:, [0, 1, 2, 5, 6, 7, 10, 11, 12]].astype(np.float64).reshape(ntri, 3, 3)
    tbad = ~np.isfinite(v).all(axis=(1, 2))
    tlo = np.where(tbad[:, None], np.inf, v.min(axis=1))     # (ntri, axis); a non-finite triangle is left out
    thi = np.where(tbad[:, None], -np.inf, v.max(axis=1))
    tlo, thi = np.vstack([tlo, np.full((1, 3), np.inf)]), np.vstack([thi, np.full((1, 3), -np.inf)])
    tbad = np.append(tbad, False)
    # ---- the walk down, level by level
    seen = np.zeros(nslots, np.int64)
    owners = np.zeros(ntri + 1, np.int64)
    seen[0] = 1
    levels, frontier = [], np.array([0], np.int64)
    nleaves = max_leaf = 0
    C = 3 if t.fmt != 2 else MAX_LEAF2
    while len(frontier):
        L = _decode_wide(t, frontier, rep) if t.fmt != 2 else _decode2(t, frontier, rep)
        ids = L["ids"]
        isleaf = L["count"] > 0
        beyond = isleaf & (L["first"] + L["count"] > ntri)
        rep.add("leaf-range", beyond, ids, lambda ix: f"slots {int(L['first'][ix])} + {int(L['count'][ix])} of {ntri}")
        L["count"] = np.where(beyond, 0, L["count"])
        isleaf = L["count"] > 0
        tix = L["first"][:, :, None] + np.arange(C)
        tix = np.where(np.arange(C) < L["count"][:, :, None], tix, ntri)
        L["tix"] = tix
        np.add.at(owners, tix.ravel(), 1)
        nleaves += int(isleaf.sum())
        max_leaf = max(max_leaf, int(L["count"].max(initial=0)))
        kid = L["kid"]
        out = (kid >= nslots)
        rep.add("node-range", out, ids, lambda ix: f"child node {int(kid[ix])} of {nslots} slots")
        kid = np.where(out, -1, kid)
        # a node is entered once: the first time it is reached (earlier levels first, then slot order)
        order = np.argsort(kid.ravel(), kind="stable")
        ks = kid.ravel()[order]
        firsts = np.ones(len(ks), bool)
        firsts[1:] = ks[1:] != ks[:-1]
        fresh = np.zeros(kid.size, bool)
        fresh[order] = firsts
        fresh = fresh.reshape(kid.shape) & (kid >= 0) & (seen[np.maximum(kid, 0)] == 0)
        twice = (kid >= 0) & ~fresh
        rep.add("node-twice", twice, ids, lambda ix: f"child node {int(kid[ix])} is reached more than once")
        seen[kid[fresh]] = 1
        L["kid"] = np.where(fresh, kid, -1)
        L["lost"] = twice | out
        levels.append(L)
        frontier = L["kid"][fresh]
    nnodes = sum(len(L["ids"]) for L in levels)
    owners = owners[:ntri]
    for s in np.flatnonzero(owners != 1)[:REPORT_CAP]:
        rep.one("tri-coverage", f"triangle slot {int(s)} belongs to {int(owners[s])} leaves", slot=int(s))
    if (owners != 1).sum() > REPORT_CAP:
        rep.one("tri-coverage", f"... and {int((owners != 1).sum()) - REPORT_CAP} more")
    # ---- stats and stack
    if t.stats is not None:
        got = dict(nodes=nnodes, leaves=nleaves, max_depth=len(levels))
        for k, g in got.items():
            if int(t.stats[k]) != g:
                rep.one("stats", f"{k}: the walk finds {g}, the header says {int(t.stats[k])}")
        hm = int(t.stats["max_leaf"])
        if (t.fmt == 2 and hm != max_leaf) or (t.fmt != 2 and (hm != 3 or max_leaf > 3)):
            rep.one("stats", f"max_leaf: the walk finds {max_leaf}, the header says {hm}")
    if t.stack_depth is not None:
        need = len(levels) if t.fmt == 2 else max(len(levels) - 1, 1)
        if need > t.stack_depth:
            rep.one("stack-depth", f"{len(levels)} levels need {need} entries, the header declares {t.stack_depth}")
    # ---- the way back up: exact subtree boxes, enclosure, tightness
    sub_lo, sub_hi = np.full((nslots, 3), np.inf), np.full((nslots, 3), -np.inf)
    sub_bad = np.zeros(nslots, bool)
    max_slack = 0.0
    for L in reversed(levels):
        ids, kid, live = L["ids"], L["kid"], L["live"]
        inner = kid >= 0
        k0 = np.maximum(kid, 0)
        clo = np.where(inner[:, :, None], sub_lo[k0], tlo[L["tix"]].min(axis=2))     # (n, K, 3)
        chi = np.where(inner[:, :, None], sub_hi[k0], thi[L["tix"]].max(axis=2))
        cbad = np.where(inner, sub_bad[k0], tbad[L["tix"]].any(axis=2))
        checked = live & ~L["lost"]            # children whose subtree the walk did enter
        nlo = np.where(checked[:, :, None], clo, np.inf).min(axis=1)
        nhi = np.where(checked[:, :, None], chi, -np.inf).max(axis=1)
        nbad = (cbad & checked).any(axis=1)
        sub_lo[ids], sub_hi[ids], sub_bad[ids] = nlo, nhi, nbad
        lo_dec, hi_dec = L["lo_dec"], L["hi_dec"]
        bounded = np.ones((len(ids), 1, 3), bool) if t.fmt == 2 else np.isfinite(L["origin"])[:, None, :]
        with np.errstate(invalid="ignore"):
            if t.fmt == 2:
                open_lo, open_hi = ~(lo_dec <= clo), ~(hi_dec >= chi)
            else:   # the rounded plane decides unless it equals the coordinate; then the sum's error does
                elo, ehi = np.swapaxes(L["lo_err"], 1, 2), np.swapaxes(L["hi_err"], 1, 2)
                open_lo = ~((lo_dec < clo) | ((lo_dec == clo) & (elo <= 0)))
                open_hi = ~((hi_dec > chi) | ((hi_dec == chi) & (ehi >= 0)))
            open_lo &= checked[:, :, None] & bounded
            open_hi &= checked[:, :, None] & bounded
        rep.add("enclosure", open_lo, ids, lambda ix: f"lo plane {lo_dec[ix]!r} above the geometry's minimum {clo[ix]!r}")
        rep.add("enclosure", open_hi, ids, lambda ix: f"hi plane {hi_dec[ix]!r} below the geometry's maximum {chi[ix]!r}")
        tight = checked[:, :, None] & ~nbad[:, None, None] & np.isfinite(clo)
        if t.fmt == 2:
            rep.add("bvh2-tight", tight & ((lo_dec != clo) | (hi_dec != chi)), ids,
                    lambda ix: f"stored [{lo_dec[ix]!r}, {hi_dec[ix]!r}], exact union [{clo[ix]!r}, {chi[ix]!r}]")
            continue
        origin, eb, step = L["origin"], L["eb"], L["step"]
        ok = ~nbad & np.isfinite(nlo).all(axis=1)
        rep.add("origin", ok[:, None] & (origin != nlo), ids,
                lambda ix: f"origin {origin[ix]!r}, exact minimum {nlo[ix]!r}", axis_dim=1)
        with np.errstate(invalid="ignore", over="ignore"):
            ext = nhi - nlo
            e = eb - 127
            half, herr = _two_sum(nlo, 255.0 * np.ldexp(1.0, e - 1))      # would e - 1 have reached the maximum?
            loose = ((half > nhi) | ((half == nhi) & (herr >= 0))) & (e > -100)
            wrong0 = (ext == 0) & (e != -100)
            rep.add("exponent", ok[:, None] & (loose | wrong0), ids,
                    lambda ix: f"e = {int(e[ix])} for an extent of {ext[ix]!r}", axis_dim=1)
            # x - plane < step in float64 can only err towards a report (rounding is monotonic and the
            # step is representable): each candidate is confirmed in rational arithmetic
            S = lambda ix: Fraction(2) ** int(e[ix[0], ix[2]])                       # noqa: E731
            plane = lambda q, ix: Fraction(origin[ix[0], ix[2]]) + int(q[ix[0], ix[2], ix[1]]) * S(ix)  # noqa: E731
            rep.add("tight-lo", tight & ~(clo - lo_dec < step[:, None, :]), ids,
                    lambda ix: f"lo plane {lo_dec[ix]!r} a step {step[ix[0], ix[2]]!r} or more below the minimum {clo[ix]!r}",
                    confirm=lambda ix: Fraction(clo[ix]) - plane(L["qlo"], ix) >= S(ix))
            rep.add("tight-hi", tight & ~(hi_dec - chi < step[:, None, :]), ids,
                    lambda ix: f"hi plane {hi_dec[ix]!r} a step {step[ix[0], ix[2]]!r} or more above the maximum {chi[ix]!r}",
                    confirm=lambda ix: plane(L["qhi"], ix) - Fraction(chi[ix]) >= S(ix))
            slack = np.where(tight & bounded, np.maximum(clo - lo_dec, hi_dec - chi) / step[:, None, :], 0.0)
            if slack.size:
                max_slack = max(max_slack, float(np.nanmax(slack)))
    # ---- index arrays
    ids15 = t.rec[:, 15].view(np.uint32).astype(np.int64)
    if t.orig2slot is not None:
        o2s = t.orig2slot.astype(np.int64)
        inr = (o2s >= 0) & (o2s < ntri)
        if len(o2s) != ntri or not inr.all() or len(np.unique(o2s)) != ntri:
            rep.one("orig2slot-perm", f"{len(o2s)} entries, {len(np.unique(o2s[inr]))} distinct slots of {ntri}")
        wrong = np.flatnonzero(ids15[np.clip(o2s, 0, ntri - 1)] != np.arange(len(o2s)))
        for i in wrong[:REPORT_CAP]:
            rep.one("orig2slot-id", f"record orig2slot[{int(i)}] = {int(o2s[i])} carries id {int(ids15[np.clip(o2s[i], 0, ntri - 1)])}",
                    slot=int(o2s[i]))
    # ---- records and normals against the mesh
    if mesh is not None:
        pos = np.asarray(mesh["pos"], np.float32).reshape(-1, 3)
        pt = np.asarray(mesh["pos_tri"], np.int64).reshape(-1, 3)
        orig = np.clip(ids15, 0, len(pt) - 1)
        want = tri_records(pos[pt[orig]].reshape(-1, 9), ids15)
        diff = np.flatnonzero((want.view(np.uint32) != t.rec.view(np.uint32)).any(axis=1) | (ids15 >= len(pt)))
        for s in diff[:REPORT_CAP]:
            rep.one("record", f"slot {int(s)} (triangle {int(ids15[s])}) differs from tri_record_fill of the mesh",
                    slot=int(s))
        if t.snrm is not None:
            mat = np.zeros(len(pt), np.int32) if mesh.get("mat_id") is None else np.asarray(mesh["mat_id"], np.int32)
            got_w = t.snrm[:, 0, 3].view(np.uint32)
            wrong = got_w != mat[orig].view(np.uint32)
            if mesh.get("nrm_tri") is not None and mesh.get("nrm") is not None:
                nt = np.asarray(mesh["nrm_tri"], np.int64).reshape(-1, 3)[orig]
                nrm = np.asarray(mesh["nrm"], np.float32).reshape(-1, 3)
                given = nt >= 0
                wn = nrm[np.maximum(nt, 0)]
                wrong |= (given[:, :, None] & (wn.view(np.uint32) != t.snrm[:, :, :3].view(np.uint32))).any(axis=(1, 2))
            for s in np.flatnonzero(wrong)[:REPORT_CAP]:
                rep.one("normal", f"slot {int(s)} (triangle {int(ids15[s])}): normals / material id differ from the mesh",
                        slot=int(s))
    if info is not None:
        info.update(nodes=nnodes, leaves=nleaves, levels=len(levels), max_leaf=max_leaf, max_slack=max_slack)
    return rep.out


def rules(violations):
    """The set of rule names in a violation list."""
    return {v.rule for v in violations}


def assert_sound(t, mesh=None, what="", info=None):
    """audit() and fail with the listed violations."""
    vs = audit(t, mesh, info)
    assert not vs, f"{what}: {len(vs)} violations\n" + "\n".join(str(v) for v in vs[:40])
