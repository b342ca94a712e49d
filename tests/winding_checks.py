"""Checks the winding-number queries (crt_winding_numbers*, crt_winding_moments_export; include/crt_hip.h) share over the hard
scene and tree classes: tests/test_nonfinite_vertices.py (inert triangles), tests/test_deep_stacks.py (stacks past the LDS
part, a depth4 that moves) and tests/test_winding.py (far from the origin, tiny scenes) call assert_winding from their hubs.
tests/test_winding_checks.py proves on the CPU that these checks can fail.

The expectations come from three sides: tests/winding_reference.c (the contract's operation order, bit for bit), brute force
over the records with the inert ones deleted (so that the expectation does not depend on the rule under test), and
moments_f64, a float64 statement of the moment table written from the header's words alone."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_winding as tw  # noqa: E402
from test_winding import wref  # noqa: E402,F401  (fixture: tests/winding_reference.c)

EXACT_BETAS = (0.0, -1.0, float("inf"))
TREE_BETAS = (2.0, 8.0)
MAX_POINTS = 264
N_FAR = 6
N_SPECIAL = 5  # the last records of points_for: a NaN record, a vertex, an edge midpoint, in a triangle's plane inside / outside it
EMPTY = -1     # CRT_BVH_EMPTY


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def finite_records(recs):
    """the records that are not inert: nine finite floats"""
    return np.isfinite(recs["v0"]).all(axis=1) & np.isfinite(recs["e1"]).all(axis=1) & np.isfinite(recs["e2"]).all(axis=1)


# ---- points

def points_for(sc, seed, n=MAX_POINTS):
    """n <= 264 point records for the scene: points spread over the box of the finite vertices with a 10 % rim (an axis along
    which the scene is flat gets a quarter of the box's diagonal, or every point would lie in the triangles' plane; [-5, 5]^3
    when no triangle is finite), N_FAR points 100 sizes away, and last the N_SPECIAL records: one with a NaN, one equal to a
    vertex of a seeded finite triangle, one on its edge's midpoint, one in its plane inside it and one in its plane outside it
    (box points when no triangle is finite).  Neither shuffled nor scene dependent beyond that: pts[:-N_SPECIAL] keeps clear of
    the places where a winding number jumps."""
    assert N_FAR + N_SPECIAL < n <= MAX_POINTS
    rng = np.random.default_rng(seed)
    corners = []
    for m in sc["meshes"]:
        v = np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3)
        t = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)
        corners.append(v[t].reshape(-1, 3, 3))
    corners = np.concatenate(corners) if corners else np.zeros((0, 3, 3), np.float32)
    fin = np.isfinite(corners).all(axis=(1, 2))
    if fin.any():
        V = corners.reshape(-1, 3)
        V = V[np.isfinite(V).all(axis=1)].astype(np.float64)
        lo, hi = V.min(axis=0), V.max(axis=0)
    else:
        lo, hi = np.full(3, -5.0), np.full(3, 5.0)
    size = float(np.linalg.norm(hi - lo)) or 1.0
    mid, ext = 0.5 * (lo + hi), np.maximum(hi - lo, 0.25 * size)
    n_box = n - N_FAR - N_SPECIAL
    box = mid - 0.6 * ext + rng.random((n_box + N_SPECIAL, 3)) * 1.2 * ext
    far = rng.normal(size=(N_FAR, 3))
    far = mid + far / np.linalg.norm(far, axis=1, keepdims=True) * 100.0 * size
    special = box[n_box:].copy()
    if fin.any():
        a, b, c = corners[fin][rng.integers(0, int(fin.sum()))].astype(np.float64)
        special[1:] = [a, 0.5 * (a + b), a + 0.25 * (b - a) + 0.25 * (c - a), a + 0.75 * (b - a) + 0.75 * (c - a)]
    pts = tw._records(np.float32(np.concatenate([box[:n_box], far, special])))
    pts[n - N_SPECIAL, 1] = np.nan
    assert len(pts) == n
    return pts


# ---- the wide tree as exported: reachable nodes, counts, depths

def _leaf(ref):
    return (~ref) >> 3, (~ref) & 7


def reachable(nodes4q):
    """the nodes the root reaches, parents before children"""
    out, todo, n4 = [], [0] if len(nodes4q) else [], len(nodes4q)
    while todo:
        i = todo.pop()
        out.append(i)
        todo.extend(int(r) for r in nodes4q["ref"][i] if 0 <= int(r) < n4)
    assert len(set(out)) == len(out), "a node has two parents"
    return out


def exact_walk_counts(nodes4q):
    """(inner nodes the root reaches, triangle records in the leaves it reaches): what one walked point of an exact-mode query
    fetches, inert records included"""
    nodes = reachable(nodes4q)
    tris = sum(_leaf(int(r))[1] for i in nodes for r in nodes4q["ref"][i] if int(r) < EMPTY)
    return len(nodes), int(tris)


def exact_walk_depth(nodes4q):
    """the deepest stack of the exact-mode walk, whatever the point: at a node the first non-empty slot becomes current and the
    others are pushed in slot order; a leaf pops"""
    if not len(nodes4q):
        return 0
    stack, cur, deepest = [], 0, 0
    while True:
        if cur >= 0:
            live = [int(r) for r in nodes4q["ref"][cur] if int(r) != EMPTY]
            if live:
                stack.extend(live[1:])
                deepest = max(deepest, len(stack))
                cur = live[0]
                continue
        if not stack:
            return deepest
        cur = stack.pop()


# ---- the moment table in float64, from the header's words

def decoded_boxes(nodes4q):
    """(n, 4, 2, 3) float32: the decoded quantised box (lo / hi, axis) of every slot, fmaf(q, s, lo)"""
    q = nodes4q
    out = np.zeros((len(q), 4, 2, 3), np.float32)
    for a, ax in enumerate("xyz"):
        lo, s = q["lo"][:, a].astype(np.float64), q["s"][:, a].astype(np.float64)
        for k in range(4):
            out[:, k, 0, a] = (((q["qlo_" + ax] >> (8 * k)) & 0xFF).astype(np.float64) * s + lo).astype(np.float32)
            out[:, k, 1, a] = (((q["qhi_" + ax] >> (8 * k)) & 0xFF).astype(np.float64) * s + lo).astype(np.float32)
    return out


def moments_f64(nodes4q, tris):
    """The header's table, per child slot directly over all triangles below the slot (not folded level by level), inert ones
    dropped: N~ = sum 0.5 (e1 x e2), A = sum |0.5 (e1 x e2)|, P = sum A_i (v0 + (e1 + e2) / 3), p~ = P / A, the box centre
    when A = 0.  Returns arrays over (node, slot): "live" (the slot is not empty and its node is reachable), "n" (finite
    triangles below), "N", "p", their tolerances "tolN" = n 2^-52 sum |n_i| and "tolP" = n 2^-51 max |centroid| (the float64
    summation error of both sides; the float32 rounding of the export is added where they are compared), "below" (the leaf-order
    indices of the finite triangles below the slot) and "reachable"."""
    n4 = len(nodes4q)
    v0, e1, e2 = (tris[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    fin = finite_records(tris)
    with np.errstate(invalid="ignore", over="ignore"):
        area_vec = 0.5 * np.cross(e1, e2)
        area = np.sqrt((area_vec * area_vec).sum(axis=1))
        cen = v0 + (e1 + e2) / 3.0
    boxes = decoded_boxes(nodes4q).astype(np.float64)
    out = {"live": np.zeros((n4, 4), bool), "n": np.zeros((n4, 4), np.int64), "N": np.zeros((n4, 4, 3)), "p": np.zeros((n4, 4, 3)),
           "tolN": np.zeros((n4, 4, 3)), "tolP": np.zeros((n4, 4, 3)), "below": {}, "reachable": reachable(nodes4q)}
    below_node = {}
    for i in reversed(out["reachable"]):  # children before their parents
        parts = []
        for k in range(4):
            ref = int(nodes4q["ref"][i][k])
            if ref == EMPTY:
                continue
            if ref >= 0:
                idx = below_node.get(ref, np.zeros(0, np.int64))
            else:
                first, cnt = _leaf(ref)
                idx = np.arange(first, first + cnt, dtype=np.int64)
                idx = idx[fin[idx]]
            parts.append(idx)
            n = len(idx)
            out["live"][i, k], out["n"][i, k], out["below"][(i, k)] = True, n, idx
            A = area[idx].sum()
            out["N"][i, k] = area_vec[idx].sum(axis=0)
            out["tolN"][i, k] = n * 2.0 ** -52 * np.abs(area_vec[idx]).sum(axis=0)
            if A > 0.0:
                out["p"][i, k] = (area[idx, None] * cen[idx]).sum(axis=0) / A
                out["tolP"][i, k] = n * 2.0 ** -51 * np.abs(cen[idx]).max(axis=0)
            else:
                out["p"][i, k] = 0.5 * (boxes[i, k, 0] + boxes[i, k, 1])
        below_node[i] = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return out


def check_moments_f64(moments, nodes4q, tris, what, f64=None):
    """an exported table against moments_f64: N~ and p~ per component to one float32 rounding plus the summation error, r no
    smaller than the distance from the exported p~ to every finite vertex below the slot (less one float32 ulp of r), the
    fourth word of N~ and every empty slot zero"""
    f64 = moments_f64(nodes4q, tris) if f64 is None else f64
    m = np.asarray(moments, dtype=np.float32).reshape(len(nodes4q), 2, 4, 4)  # (node, {p~ r | N~ 0}, slot, word)
    got_p, got_r, got_N = m[:, 0, :, 0:3].astype(np.float64), m[:, 0, :, 3], m[:, 1, :, 0:3].astype(np.float64)
    live = f64["live"]
    reach = np.zeros(len(nodes4q), bool)
    reach[f64["reachable"]] = True
    dead = reach[:, None] & ~live
    assert not _bits(m).reshape(len(nodes4q), 2, 4, 4).transpose(0, 2, 1, 3)[dead].any(), what + ": an empty slot's moments are not zeros"
    assert not _bits(m[:, 1, :, 3])[live].any(), what + ": the word after N~ is not zero"
    for name, got, want, tol in (("N~", got_N, f64["N"], f64["tolN"]), ("p~", got_p, f64["p"], f64["tolP"])):
        bound = 2.0 ** -24 * np.abs(want) + tol
        bad = np.argwhere(live[:, :, None] & ~(np.abs(got - want) <= bound))
        assert len(bad) == 0, "%s: %s of node %d slot %d axis %d is %r, float64 gives %r +- %.3e (%d triangles below)" % (
            what, name, bad[0][0], bad[0][1], bad[0][2], got[tuple(bad[0])], want[tuple(bad[0])], bound[tuple(bad[0])],
            f64["n"][bad[0][0], bad[0][1]])
    v0, e1, e2 = (tris[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    for (i, k), idx in f64["below"].items():
        if not len(idx):
            continue
        corners = np.concatenate([v0[idx], v0[idx] + e1[idx], v0[idx] + e2[idx]])
        far = np.sqrt(((corners - got_p[i, k]) ** 2).sum(axis=1)).max()
        r = got_r[i, k]
        assert float(r) >= far - float(np.spacing(r)), "%s: r of node %d slot %d is %r, a vertex below it is %r from p~" % (what, i, k, r, far)
    return f64


def assert_moments(wref, nodes4q, tris, moments, what):
    """the exported table is finite, no reachable node with a finite triangle below it kept the zeros of the memset, every bit
    is tests/winding_reference.c's, and the table holds against moments_f64"""
    moments = np.asarray(moments, dtype=np.float32)
    assert moments.shape == (len(nodes4q), 32) and len(nodes4q) > 0, what + ": the table's shape"
    assert np.isfinite(moments).all(), what + ": a moment is not finite"
    f64 = moments_f64(nodes4q, tris)
    zero = ~_bits(moments).any(axis=1)
    starved = [i for i in f64["reachable"] if zero[i] and f64["n"][i].any()]
    assert not starved, ("%s: the moment lines of %d reachable nodes with finite triangles below them are all zeros, first node %d: "
                         "the level launches stopped short of the tree's depth (a stale or short depth4)" % (what, len(starved), starved[0]))
    want = tw.ref_moments(wref, nodes4q, tris)
    bad = np.flatnonzero((_bits(moments) != _bits(want)).any(axis=1))
    assert len(bad) == 0, "%s: the moments of %d nodes differ from the reference, first node %d: %r vs %r" % (
        what, len(bad), bad[0], moments[bad[0]], want[bad[0]])
    check_moments_f64(moments, nodes4q, tris, what, f64)


# ---- the hub

def _same_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert len(bad) == 0, "%s: %d of %d differ, first point %d: %r vs %r" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


class _DeviceForm:
    """the device form on torch tensors (on plain host buffers for a stand-in that says host_pointers: the CPU tests)"""

    def __init__(self, r, pts):
        self.r, self.n = r, len(pts)
        if getattr(r, "host_pointers", False):
            self.pts, self.w = np.ascontiguousarray(pts), np.zeros(len(pts), np.float32)
            self.ptrs = (self.pts.ctypes.data, self.w.ctypes.data)
            self.read = lambda: self.w.copy()
        else:
            import torch
            self.pts = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
            self.w = torch.zeros(len(pts), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            self.ptrs = (self.pts.data_ptr(), self.w.data_ptr())
            self.read = lambda: self.w.cpu().numpy().copy()

    def __call__(self, beta):
        st = self.r.winding_numbers_device(self.n, self.ptrs[0], self.ptrs[1], beta, stats=True)
        return self.read(), st


def assert_winding(pkg, wref, r, sc, records_by_gid, pts, what):
    """The scene r holds is sc, whose records by gid are records_by_gid (inert ones as NaNs or not, it does not matter: they are
    deleted).  Over the tree and the table r exports:
      1. the moments are finite, the reference's bit for bit, and hold against moments_f64;
      2. beta 0, -1 and +inf give the bits of brute force over the records with the inert ones deleted;
      3. beta 2 and 8 give the bits of the reference's walk over the exported tree and table, and are finite;
      4. a record with a NaN gives +0;
      5. the device form gives the host form's bits;
      6. counting changes no bit;
      7. with counting, an exact-mode query fetches exact_walk_counts per walked point, and without it reports zeros.
    Returns {"w": {beta: bits}, "counters": {beta: (nodes_visited, tris_tested)}} for what a caller holds across states."""
    pts = tw._records(pts)
    nodes4q, tris = r.bvh_export4q(), np.ascontiguousarray(r.bvh_export()[1])
    n_scene = sum(len(np.asarray(m["triangles"]).reshape(-1, 3)) for m in sc["meshes"])
    assert len(tris) == len(records_by_gid) == n_scene, what + ": the records are not the scene's"
    assert np.array_equal(np.sort(tris["gid"]), np.arange(n_scene)), what + ": the exported gids"
    moments = r.winding_moments()
    assert_moments(wref, nodes4q, tris, moments, what)
    alive = finite_records(records_by_gid)
    assert np.array_equal(finite_records(tris), alive[tris["gid"].astype(np.int64)]), what + ": the exported records' inert triangles"
    exact = tw.ref_exact(wref, np.ascontiguousarray(records_by_gid[alive]), pts)
    want = {beta: exact for beta in EXACT_BETAS}
    for beta in TREE_BETAS:
        want[beta] = tw.ref_tree(wref, nodes4q, tris, moments, beta, pts)
    host = {}
    for beta in EXACT_BETAS + TREE_BETAS:
        host[beta] = r.winding_numbers(pts, beta)
        kind = "exact mode against brute force without the inert records" if beta in EXACT_BETAS else "the walk against the reference's"
        _same_bits(host[beta], want[beta], "%s: beta %r, %s" % (what, beta, kind))
        assert np.isfinite(host[beta]).all(), "%s: beta %r: a winding number is not finite" % (what, beta)
    nan = np.isnan(pts[:, 0:3]).any(axis=1)
    for beta, w in host.items():
        assert not _bits(w)[nan].any(), "%s: beta %r: a record with a NaN does not give +0" % (what, beta)
    inner, fetched = exact_walk_counts(nodes4q)
    walked = int((~nan).sum())
    device = _DeviceForm(r, pts)
    counters = {}
    try:
        for counting in (False, True):
            r.set_counting(counting)
            for beta in EXACT_BETAS + TREE_BETAS:
                w, st = device(beta)
                _same_bits(w, host[beta], "%s: beta %r, the device form (counting=%d) against the host form" % (what, beta, counting))
                assert st["rays_primary"] == len(pts), what
                got = (int(st["nodes_visited"]), int(st["tris_tested"]))
                if not counting:
                    assert got == (0, 0), "%s: beta %r: counters %r without counting" % (what, beta, got)
                    continue
                counters[beta] = got
                if beta in EXACT_BETAS:
                    assert got == (walked * inner, walked * fetched), "%s: beta %r: the exact-mode walk of %d points fetched %r, the tree has %r" % (
                        what, beta, walked, got, (walked * inner, walked * fetched))
    finally:
        r.set_counting(False)
    return {"w": {beta: _bits(w).copy() for beta, w in host.items()}, "counters": counters}
