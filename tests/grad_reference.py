"""tests/grad_reference.c from Python (tests/test_gradients.py): the two builds of the reference, the scene as the explicit arrays it
takes, and the bound the vertex sums are held to."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF


def compile_reference(tmp, double):
    """the float32 build (double=False: the kernels' arithmetic) or the float64 build of grad_reference.c"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler for tests/grad_reference.c")
    out = str(tmp / ("libgrad_reference_%s.so" % ("f64" if double else "f32")))
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC"] + (["-DGRAD_DOUBLE"] if double else []) +
                          [os.path.join(ROOT, "tests", "grad_reference.c"), "-o", out, "-lm"])
    L = C.CDLL(out)
    L.ray_grad_reference.restype = None
    L.ray_grad_reference.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 14
    L.point_grad_reference.restype = None
    L.point_grad_reference.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 12
    L.real = np.float64 if double else np.float32
    return L


class SceneArrays:
    """meshes, a list of (world vertices (nv, 3), triangles (nt, 3)), as the reference takes a scene"""

    def __init__(self, meshes):
        self.n_meshes = len(meshes)
        self.tri_start = np.cumsum([0] + [len(t) for _, t in meshes]).astype(np.uint32)
        self.vert_start = np.cumsum([0] + [len(v) for v, _ in meshes]).astype(np.uint32)
        self.world = np.ascontiguousarray(np.concatenate([np.asarray(v).reshape(-1, 3) for v, _ in meshes]))
        self.idx = np.ascontiguousarray(np.concatenate([np.asarray(t).reshape(-1, 3) for _, t in meshes]), np.uint32)
        self.n_vertices = len(self.world)

    def vertex_ids(self, inst, prim):
        """(n, 3) global vertex numbers of the records' triangles, -1 where the ids name none"""
        inst, prim = np.asarray(inst, np.uint32), np.asarray(prim, np.uint32)
        out = np.full((len(inst), 3), -1, np.int64)
        ok = inst < self.n_meshes
        m = np.where(ok, inst, 0)
        ok &= prim < (self.tri_start[m + 1] - self.tri_start[m])
        g = self.tri_start[m[ok]].astype(np.int64) + prim[ok]
        out[ok] = self.idx[g].astype(np.int64) + self.vert_start[m[ok]].astype(np.int64)[:, None]
        return out


def _ptr(a):
    return None if a is None else a.ctypes.data


def _as(L, a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=L.real)
    return a if shape is None else a.reshape(shape)


def ray_reference(L, scene, rays, inst, prim, t, uv, grad_t, grad_uv):
    """(grad_rays (n, 8), contributions (n, 3 vertices, 3), live (n,)) in the build's precision"""
    n = len(inst)
    world, r, tt, u = _as(L, scene.world), _as(L, rays, (-1, 8)), _as(L, t), _as(L, uv, (-1, 2))
    gt, gu = _as(L, grad_t), _as(L, grad_uv, (-1, 2))
    i, q = np.ascontiguousarray(inst, np.uint32), np.ascontiguousarray(prim, np.uint32)
    grad_rays, contrib, live = np.zeros((n, 8), L.real), np.zeros((n, 3, 3), L.real), np.zeros(n, np.uint8)
    L.ray_grad_reference(n, scene.n_meshes, _ptr(scene.tri_start), _ptr(scene.vert_start), _ptr(world), _ptr(scene.idx), _ptr(r), _ptr(i), _ptr(q),
                         _ptr(tt), _ptr(u), _ptr(gt), _ptr(gu), _ptr(grad_rays), _ptr(contrib), _ptr(live))
    return grad_rays, contrib, live.astype(bool)


def point_reference(L, scene, points, inst, prim, uv, grad_dist):
    """(grad_points (n, 4), contributions (n, 3, 3), live (n,)) in the build's precision"""
    n = len(inst)
    world, p, u, g = _as(L, scene.world), _as(L, points, (-1, 4)), _as(L, uv, (-1, 2)), _as(L, grad_dist)
    i, q = np.ascontiguousarray(inst, np.uint32), np.ascontiguousarray(prim, np.uint32)
    grad_points, contrib, live = np.zeros((n, 4), L.real), np.zeros((n, 3, 3), L.real), np.zeros(n, np.uint8)
    L.point_grad_reference(n, scene.n_meshes, _ptr(scene.tri_start), _ptr(scene.vert_start), _ptr(world), _ptr(scene.idx), _ptr(p), _ptr(i), _ptr(q),
                           _ptr(u), _ptr(g), _ptr(grad_points), _ptr(contrib), _ptr(live))
    return grad_points, contrib, live.astype(bool)


def vertex_sums(scene, inst, prim, contrib, live):
    """per component of grad_xyz what the header's guarantee is stated in: S = the exact sum (math.fsum) of the live records' float32
    contributions, A = the sum of their magnitudes, m = their count.  Three (n_vertices, 3) arrays"""
    ids = scene.vertex_ids(inst, prim)
    lists = [[] for _ in range(3 * scene.n_vertices)]
    c64 = np.asarray(contrib, np.float64)
    for i in np.nonzero(live)[0]:
        for j in range(3):
            base = 3 * int(ids[i, j])
            for k in range(3):
                lists[base + k].append(float(c64[i, j, k]))
    S = np.array([math.fsum(l) for l in lists]).reshape(-1, 3)
    A = np.array([math.fsum(abs(x) for x in l) for l in lists]).reshape(-1, 3)
    m = np.array([len(l) for l in lists], np.float64).reshape(-1, 3)
    return S, A, m


def check_vertex_sums(got, S, A, m, what=""):
    """|got - S| <= 2^-24 |S| + m 2^-52 A per component: the any-order float64 summation error plus one float32 rounding; components
    without a contribution are +0.0 bitwise.  Returns the worst |got - S| in units of the bound."""
    got = np.asarray(got, np.float32).reshape(-1, 3)
    assert got.shape == S.shape, (what, got.shape, S.shape)
    bound = 2.0 ** -24 * np.abs(S) + m * 2.0 ** -52 * A
    err = np.abs(got.astype(np.float64) - S)
    assert np.all(err <= bound), (what, float((err - bound).max()), int((err > bound).sum()))
    untouched = m == 0
    assert np.all(got.view(np.uint32)[untouched] == 0), (what, "a vertex no live record touches is +0.0")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0.0))) if got.size else 0.0
