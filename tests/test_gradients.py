"""Gradients of the closest-hit and closest-point queries (include/crt_hip.h, "gradients"): crt_trace_rays_backward*,
crt_closest_points_backward*, Renderer.trace_rays_torch / closest_points_torch.

tests/grad_reference.c restates the per-record arithmetic in plain C (compiled here with -O2 -ffp-contract=off -fno-fast-math), once
in float32 and once in float64.  On the CPU the float64 build is held against torch.autograd in float64 -- Moeller-Trumbore solved as
a 3x3 system, the point-triangle distance by the closed form of the point's region -- and the float32 build against the float64
build.  On the GPU grad_rays and grad_points equal the float32 build bit for bit and every component of grad_xyz lies within
2^-24 |S| + m 2^-52 A of the exact sum S of the reference's contributions (A: the sum of their magnitudes, m: their count).

Figures observed on the CPU, 4096 seeded records, |d . n| >= 0.1 |d| |n|, no triangle angle below 20 degrees, per record the largest
deviation of any output relative to the largest component of that output's vector: float64 build against torch.autograd 4.1e-15
(rays; 4.9e-15 with another machine's LAPACK) and 8.9e-15 (points); float32 build against float64 build 13.0 x 2^-24 (rays) and 28.7 x 2^-24 (points, each at least 0.05
from its triangle: p - q cancels there)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grad_reference as G  # noqa: E402

SYMBOLS = ("crt_trace_rays_backward_device", "crt_trace_rays_backward", "crt_closest_points_backward_device", "crt_closest_points_backward")
METHODS = ("trace_rays_backward", "trace_rays_backward_device", "closest_points_backward", "closest_points_backward_device", "trace_rays_torch",
           "closest_points_torch")
EINVAL, ESTATE = 1, 5
MISS = 0xFFFFFFFF
N = 2049  # neither a multiple of 64 nor of 256: nine workgroups, the last one with a single live lane
# float32 build against float64 build, the figures of the docstring; the tests allow four times what was measured
MEASURED_RAYS, MEASURED_POINTS = 13.1 * 2.0 ** -24, 28.7 * 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="session")
def refs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("grad_reference")
    return {"f32": G.compile_reference(tmp, False), "f64": G.compile_reference(tmp, True)}


# ---- CPU: the interface

def test_header_binding_and_library_expose_the_gradient_entry_points(pkg):
    L = pkg.lib()
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
        assert ("int %s(" % s) in header, s
    for name in METHODS:
        assert callable(getattr(pkg.Renderer, name, None)), name
    assert L.crt_abi_version() == 1
    buf = np.zeros(64, dtype=np.float32)
    ids = np.zeros(16, dtype=np.uint32)
    P, I = buf.ctypes.data, ids.ctypes.data
    assert L.crt_trace_rays_backward(None, 2, P, I, I, P, P, P, P, P, P, None) == EINVAL
    assert L.crt_trace_rays_backward_device(None, 2, P, I, I, P, P, P, P, P, P, None) == EINVAL
    assert L.crt_closest_points_backward(None, 2, P, I, I, P, P, P, P, None) == EINVAL
    assert L.crt_closest_points_backward_device(None, 2, P, I, I, P, P, P, P, None) == EINVAL
    assert L.crt_trace_rays_backward(None, 0, None, None, None, None, None, None, None, None, None, None) == EINVAL
    assert not buf.any() and not ids.any()


def test_package_imports_without_torch():
    """the torch layer imports torch inside the two calls: the package loads in an interpreter that cannot import it"""
    code = ("import sys, importlib.util\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name == 'torch' or name.startswith('torch.'):\n"
            "            raise ImportError('blocked')\n"
            "sys.meta_path.insert(0, Block())\n"
            "sys.path.insert(0, %r)\n"
            "import __graft_entry__ as e\n"
            "p = e.load_package()\n"
            "assert 'torch' not in sys.modules and callable(p.Renderer.trace_rays_torch)\n" % ROOT)
    subprocess.check_call([sys.executable, "-c", code], timeout=120)


# ---- CPU: the float64 build against torch.autograd, the float32 build against the float64 build

def _triangles(rng, n):
    """n random triangles (n, 3, 3) without an angle below 20 degrees, edge lengths of order 1, anywhere in [-2, 2]^3"""
    out = np.zeros((0, 3, 3))
    while len(out) < n:
        v = rng.uniform(-1, 1, size=(2 * n, 3, 3))
        e = np.stack([v[:, 1] - v[:, 0], v[:, 2] - v[:, 1], v[:, 0] - v[:, 2]], 1)
        ln = np.linalg.norm(e, axis=-1)
        cos = np.stack([-(e[:, 0] * e[:, 2]).sum(-1) / (ln[:, 0] * ln[:, 2]), -(e[:, 1] * e[:, 0]).sum(-1) / (ln[:, 1] * ln[:, 0]),
                        -(e[:, 2] * e[:, 1]).sum(-1) / (ln[:, 2] * ln[:, 1])], 1)
        ok = (np.degrees(np.arccos(np.clip(cos, -1, 1))).min(1) >= 20.0) & (ln.min(1) > 0.3)
        out = np.concatenate([out, v[ok] + rng.uniform(-1, 1, size=(int(ok.sum()), 1, 3))])
    return out[:n]


def _soup(tri):
    """the triangles as one mesh without shared vertices: record i names (inst 0, prim i), vertices 3 i .. 3 i + 2"""
    n = len(tri)
    return G.SceneArrays([(tri.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3))])


def _ray_inputs(seed, n):
    """float32-representable inputs (held in float64): triangles, rays hitting them at known (t, u, v), incoming gradients"""
    rng = np.random.default_rng(seed)
    tri = _triangles(rng, n).astype(np.float32).astype(np.float64)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nrm = np.cross(e1, e2)
    d = np.zeros((n, 3))
    todo = np.ones(n, bool)
    while todo.any():
        c = rng.normal(size=(n, 3))
        c /= np.linalg.norm(c, axis=-1, keepdims=True)
        ok = np.abs((c * nrm).sum(-1)) >= 0.12 * np.linalg.norm(nrm, axis=-1)
        d[todo & ok] = c[todo & ok]
        todo &= ~ok
    d = (d * rng.uniform(0.5, 2.0, size=(n, 1))).astype(np.float32).astype(np.float64)
    assert np.all(np.abs((d * nrm).sum(-1)) >= 0.1 * np.linalg.norm(d, axis=-1) * np.linalg.norm(nrm, axis=-1))
    uv = rng.uniform(0.05, 0.9, size=(n, 2))
    uv[uv.sum(-1) > 0.95] *= 0.5
    t = rng.uniform(0.5, 3.0, size=n)
    o = (tri[:, 0] + uv[:, :1] * e1 + uv[:, 1:] * e2 - t[:, None] * d).astype(np.float32).astype(np.float64)
    rays = np.zeros((n, 8))
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = o, d, np.inf
    g = rng.normal(size=(n, 3)).astype(np.float32).astype(np.float64)
    return tri, rays, g


def _solve_hits(tri, rays):
    """(t, u, v) of o + t d = a + u e1 + v e2 in float64"""
    M = np.stack([-rays[:, 4:7], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]], -1)
    return np.linalg.solve(M, (rays[:, 0:3] - tri[:, 0])[..., None])[..., 0]


def _record_scale(x):
    """per record the largest magnitude of a vector output, for a relative comparison"""
    return np.abs(x).reshape(len(x), -1).max(-1)


def test_reference_rays_equal_autograd(refs):
    """the float64 build's dL/do, dL/dd and vertex contributions equal torch.autograd through the solved 3x3 system, each within
    1e-10 of the record's largest |lambda| (dL/dd: of its largest |t lambda|)"""
    import torch
    n = 4096
    tri, rays, g = _ray_inputs(5, n)
    x = _solve_hits(tri, rays)
    T = torch.tensor(tri, dtype=torch.float64, requires_grad=True)
    o = torch.tensor(rays[:, 0:3], dtype=torch.float64, requires_grad=True)
    d = torch.tensor(rays[:, 4:7], dtype=torch.float64, requires_grad=True)
    M = torch.stack([-d, T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]], -1)
    sol = torch.linalg.solve(M, (o - T[:, 0]).unsqueeze(-1)).squeeze(-1)
    assert np.abs(sol.detach().numpy() - x).max() < 1e-12
    (sol * torch.tensor(g)).sum().backward()
    grad_rays, contrib, live = G.ray_reference(refs["f64"], _soup(tri), rays, np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32), x[:, 0], x[:, 1:],
                                               g[:, 0], g[:, 1:])
    assert live.all()
    lam = _record_scale(grad_rays[:, 0:3])
    worst = max(float((np.abs(grad_rays[:, 0:3] - o.grad.numpy()).max(-1) / lam).max()),
                float((np.abs(grad_rays[:, 4:7] - d.grad.numpy()).max(-1) / _record_scale(grad_rays[:, 4:7])).max()),
                float((np.abs(contrib - T.grad.numpy()).reshape(n, -1).max(-1) / lam).max()))
    print("float64 build against torch.autograd, rays: %.3g" % worst)
    assert worst <= 1e-10, worst
    assert not grad_rays[:, 3].any() and not grad_rays[:, 7].any()


def _closest(tri, p):
    """float64 closest point of each triangle to its point, by candidates: (u, v), region (0 face, 1..3 edge ab / ac / bc, 4..6
    vertex a / b / c)"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    n = len(tri)
    best = np.full(n, np.inf)
    uv, region = np.zeros((n, 2)), np.zeros(n, int)
    e1, e2 = b - a, c - a
    nrm = np.cross(e1, e2)
    ap = p - a
    # face: barycentrics of the projection
    d11, d12, d22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    r1, r2 = (ap * e1).sum(-1), (ap * e2).sum(-1)
    den = d11 * d22 - d12 * d12
    u, v = (d22 * r1 - d12 * r2) / den, (d11 * r2 - d12 * r1) / den
    inside = (u > 0) & (v > 0) & (u + v < 1)
    dist = np.abs((ap * nrm).sum(-1)) / np.linalg.norm(nrm, axis=-1)
    best[inside], uv[inside] = dist[inside], np.stack([u, v], -1)[inside]
    for k, (base, e, to_uv) in enumerate(((a, e1, lambda s: (s, 0 * s)), (a, e2, lambda s: (0 * s, s)), (b, c - b, lambda s: (1 - s, s)))):
        s = np.clip(((p - base) * e).sum(-1) / (e * e).sum(-1), 0, 1)
        dist = np.linalg.norm(p - (base + s[:, None] * e), axis=-1)
        take = ~inside & (dist < best)
        cu, cv = to_uv(s)
        best[take], uv[take] = dist[take], np.stack([cu, cv], -1)[take]
        ends = ((4, 5), (4, 6), (5, 6))[k]
        region[take] = np.where(s[take] <= 0, ends[0], np.where(s[take] >= 1, ends[1], k + 1))
    return uv, region, best


def _points_off(tri, rng):
    """float32-representable points around the triangles, each at least 0.05 from its triangle"""
    n = len(tri)
    p = np.zeros((n, 3))
    todo = np.ones(n, bool)
    while todo.any():
        c = (tri.mean(1) + rng.normal(size=(n, 3)) * rng.uniform(0.3, 1.5, size=(n, 1))).astype(np.float32).astype(np.float64)
        ok = _closest(tri, c)[2] >= 0.05
        p[todo & ok] = c[todo & ok]
        todo &= ~ok
    return p


def test_reference_points_equal_autograd(refs):
    """the float64 build's dL/dp and vertex contributions equal torch.autograd through the distance to the point's region of the
    triangle -- the plane's |(p - a) . n| / |n|, an edge's rejection length, a vertex's |p - vertex| -- within 1e-10 of |g|; all
    seven regions occur"""
    import torch
    n = 4096
    rng = np.random.default_rng(6)
    tri = _triangles(rng, n).astype(np.float32).astype(np.float64)
    p = _points_off(tri, rng)
    g = rng.normal(size=n).astype(np.float32).astype(np.float64)
    uv, region, dist = _closest(tri, p)
    assert dist.min() >= 0.05 and all((region == k).sum() > 20 for k in range(7)), np.bincount(region, minlength=7)
    T = torch.tensor(tri, dtype=torch.float64, requires_grad=True)
    P = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    nrm = torch.linalg.cross(b - a, c - a)
    face = ((P - a) * nrm).sum(-1).abs() / nrm.norm(dim=-1)

    def edge(base, e):
        x = P - base
        return (x - ((x * e).sum(-1) / (e * e).sum(-1)).unsqueeze(-1) * e).norm(dim=-1)
    forms = torch.stack([face, edge(a, b - a), edge(a, c - a), edge(b, c - b), (P - a).norm(dim=-1), (P - b).norm(dim=-1), (P - c).norm(dim=-1)], -1)
    d_torch = forms.gather(1, torch.tensor(region).unsqueeze(-1)).squeeze(-1)
    assert np.abs(d_torch.detach().numpy() - dist).max() < 1e-12
    (d_torch * torch.tensor(g)).sum().backward()
    points = np.concatenate([p, np.full((n, 1), np.inf)], 1)
    grad_points, contrib, live = G.point_reference(refs["f64"], _soup(tri), points, np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32), uv, g)
    assert live.all()
    worst = max(float((np.abs(grad_points[:, 0:3] - P.grad.numpy()).max(-1) / np.abs(g)).max()),
                float((np.abs(contrib - T.grad.numpy()).reshape(n, -1).max(-1) / np.abs(g)).max()))
    print("float64 build against torch.autograd, points: %.3g" % worst)
    assert worst <= 1e-10, worst
    assert not grad_points[:, 3].any()


def test_float_build_against_double_build(refs):
    """the same float32 inputs through both builds: per record the largest deviation of dL/do, of dL/dd and of the vertex
    contributions, each relative to the largest component of its own vector in float64, stays within four times what this
    comparison measured (the module docstring's figures).  This measures the reference's float32 arithmetic, not the kernel"""
    n = 4096
    tri, rays, g = _ray_inputs(7, n)
    x = _solve_hits(tri, rays).astype(np.float32).astype(np.float64)
    ids = (np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32))
    out = {k: G.ray_reference(refs[k], _soup(tri), rays, ids[0], ids[1], x[:, 0], x[:, 1:], g[:, 0], g[:, 1:]) for k in ("f32", "f64")}
    assert out["f32"][2].all() and out["f64"][2].all() and out["f32"][0].dtype == np.float32
    r32, r64, c32, c64 = out["f32"][0].astype(np.float64), out["f64"][0], out["f32"][1].astype(np.float64), out["f64"][1]
    lam = _record_scale(r64[:, 0:3])
    rays_err = max(float((np.abs(r32[:, 0:3] - r64[:, 0:3]).max(-1) / lam).max()),
                   float((np.abs(r32[:, 4:7] - r64[:, 4:7]).max(-1) / _record_scale(r64[:, 4:7])).max()),
                   float((np.abs(c32 - c64).reshape(n, -1).max(-1) / lam).max()))
    rng = np.random.default_rng(8)
    p = _points_off(tri, rng)
    uv, _, dist = _closest(tri, p)
    uv = uv.astype(np.float32).astype(np.float64)
    gd = g[:, 0]
    points = np.concatenate([p, np.full((n, 1), np.inf)], 1)
    out = {k: G.point_reference(refs[k], _soup(tri), points, ids[0], ids[1], uv, gd) for k in ("f32", "f64")}
    assert out["f32"][2].all() and out["f64"][2].all() and dist.min() >= 0.05
    scale = _record_scale(out["f64"][0][:, 0:3])
    points_err = max(float((np.abs(out["f32"][0].astype(np.float64) - out["f64"][0])[:, 0:3].max(-1) / scale).max()),
                     float((np.abs(out["f32"][1].astype(np.float64) - out["f64"][1]).reshape(n, -1).max(-1) / scale).max()))
    print("float32 build against float64 build: rays %.3g x 2^-24, points %.3g x 2^-24" % (rays_err * 2.0 ** 24, points_err * 2.0 ** 24))
    assert rays_err <= 4 * MEASURED_RAYS and points_err <= 4 * MEASURED_POINTS, (rays_err * 2.0 ** 24, points_err * 2.0 ** 24)
    assert rays_err >= 2.0 ** -26 and points_err >= 2.0 ** -26, "the float32 build computes in float32"


# ---- GPU: the scene and the records

def _quad():
    return {"vertices": np.float32([(-3, -1, 0), (-1, -1, 0), (-1, 1, 0), (-3, 1, 0)]), "triangles": np.uint32([(0, 1, 2), (0, 2, 3)]),
            "material_index": 0, "normals": None}


def _icosphere():
    f = (1 + 5 ** 0.5) / 2
    V = np.array([(-1, f, 0), (1, f, 0), (-1, -f, 0), (1, -f, 0), (0, -1, f), (0, 1, f), (0, -1, -f), (0, 1, -f), (f, 0, -1), (f, 0, 1), (-f, 0, -1),
                  (-f, 0, 1)])
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    return {"vertices": (V / np.linalg.norm(V, axis=-1, keepdims=True)).astype(np.float32), "triangles": np.uint32(T), "material_index": 0,
            "normals": None}


def _transform():
    """a rotation by 25 degrees about (1, 2, 3), scaled by 0.8, then a translation: the icosphere sits beside the quad"""
    k = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = math.radians(25.0)
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    return np.concatenate([0.8 * R, np.array([[2.0], [0.1], [-0.3]])], 1).astype(np.float32)


MATS = [{"albedo": (0.8, 0.8, 0.8), "type": 1}]
LIGHTS = [((0.0, 4.0, 2.0), 60.0)]


def _upload_scene(r):
    meshes = [_quad(), _icosphere()]
    r.upload(meshes, LIGHTS, MATS, dynamic=True)
    r.set_mesh_transform(1, _transform())
    return meshes


def _scene_arrays(r, meshes):
    """the scene as the reference takes it: the world vertices as they are traced"""
    return G.SceneArrays([(r.mesh_vertices(m)[0], meshes[m]["triangles"]) for m in range(len(meshes))])


def _edit(rec, hits, n_meshes, tri_counts):
    """the last eight records become copies of hits with one field spoilt each: inst = MISS, inst = the mesh count, prim = the
    mesh's triangle count, u = NaN, v = NaN, an infinite incoming gradient (twice: +inf and -inf), and t = inf"""
    n = len(rec["inst"])
    src = hits[:8]
    assert len(src) == 8
    for j, i in enumerate(range(n - 8, n)):
        for k in rec:
            rec[k][i] = rec[k][src[j]]
    e = n - 8
    rec["inst"][e] = MISS
    rec["inst"][e + 1] = n_meshes
    rec["prim"][e + 2] = tri_counts[rec["inst"][e + 2]]
    rec["uv"][e + 3, 0] = np.nan
    rec["uv"][e + 4, 1] = np.nan
    rec["g0"][e + 5] = np.inf
    rec["g0"][e + 6] = -np.inf
    if "t" in rec:
        rec["t"][e + 7] = np.inf
    else:
        rec["uv"][e + 7] = np.inf
    return np.arange(e, n)


def _ray_records(pkg, r, meshes, world):
    rng = np.random.default_rng(21)
    gx, gy = np.meshgrid(np.linspace(-3.6, 3.4, 40), np.linspace(-1.45, 1.55, 40))
    o = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 5.0)], -1)
    d = np.tile([0.03, -0.02, -1.0], (len(o), 1))
    # through the quad's corners, along its shared diagonal, through the icosphere's world vertices and the midpoints of its edges
    quad, ico = world[0].astype(np.float64), world[1].astype(np.float64)
    diag = quad[0] + np.linspace(0.05, 0.95, 10)[:, None] * (quad[2] - quad[0])
    T = meshes[1]["triangles"]
    mids = np.concatenate([(ico[T[:, a]] + ico[T[:, b]]) / 2 for a, b in ((0, 1), (1, 2), (2, 0))])
    target = np.concatenate([quad, diag, ico, mids])
    o2 = target + np.array([0.3, 0.2, 4.0])
    o, d = np.concatenate([o, o2]), np.concatenate([d, target - o2])
    fill = N - len(o)
    assert fill > 300
    of = np.stack([rng.uniform(-3.5, 3.5, fill), rng.uniform(-1.5, 1.5, fill), np.full(fill, 4.0)], -1)
    df = np.stack([rng.uniform(-0.4, 0.4, fill), rng.uniform(-0.4, 0.4, fill), np.full(fill, -1.0)], -1)
    df[:150] *= 1e-3  # t is in units of |d|: the same hits at t x 1000 ...
    df[150:300] *= 1e3  # ... and at t / 1000
    rays = pkg.make_rays(np.concatenate([o, of]), np.concatenate([d, df]), 0.0, np.inf)
    rays[::7, 7] = 1e6  # a miss of these reports a finite t
    assert len(rays) == N
    hit = r.trace_rays(rays)
    rec = {"rays": rays, "inst": hit["inst"].copy(), "prim": hit["prim"].copy(), "t": hit["t"].copy(), "uv": hit["uv"].copy(),
           "g0": rng.normal(size=N).astype(np.float32), "g1": rng.normal(size=(N, 2)).astype(np.float32)}
    hits = np.nonzero(rec["inst"] != MISS)[0]
    rec["edited"] = _edit(rec, hits[hits < N - 8], len(meshes), [len(m["triangles"]) for m in meshes])
    return rec


def _point_records(pkg, r, meshes, world):
    rng = np.random.default_rng(22)
    p = np.stack([rng.uniform(-4, 4, N), rng.uniform(-2, 2, N), rng.uniform(-2, 2, N)], -1).astype(np.float32)
    p[:4] = world[0]                       # on the quad's corners: dist = 0
    p[4:8] = [(-2.0, 0.25, 0.0)] * 4       # on the quad's face
    p[8:20] = world[1]                     # on the icosphere's vertices
    rmax = np.full(N, np.inf, np.float32)
    rmax[20:120] = 0.05                    # mostly misses
    pts = pkg.make_points(p, rmax)
    hit = r.closest_points(pts)
    rec = {"points": pts, "inst": hit["inst"].copy(), "prim": hit["prim"].copy(), "uv": hit["uv"].copy(), "dist": hit["dist"].copy(),
           "g0": rng.normal(size=N).astype(np.float32)}
    hits = np.nonzero((rec["inst"] != MISS) & (rec["dist"] > 0.1))[0]
    rec["edited"] = _edit(rec, hits[hits < N - 8], len(meshes), [len(m["triangles"]) for m in meshes])
    return rec


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def case(pkg, refs, renderer):
    """the two-mesh scene on the module's renderer, 2049 ray and 2049 point records from the forward queries with their edited tail,
    and the float32 reference's outputs for them.  Computed once; nothing in it is written to afterwards"""
    meshes = _upload_scene(renderer)
    scene = _scene_arrays(renderer, meshes)
    world = [renderer.mesh_vertices(m)[0] for m in range(2)]
    rr, pr = _ray_records(pkg, renderer, meshes, world), _point_records(pkg, renderer, meshes, world)
    c = {"meshes": meshes, "scene": scene, "rays": rr, "points": pr}
    c["ray_ref"] = G.ray_reference(refs["f32"], scene, rr["rays"], rr["inst"], rr["prim"], rr["t"], rr["uv"], rr["g0"], rr["g1"])
    c["point_ref"] = G.point_reference(refs["f32"], scene, pr["points"], pr["inst"], pr["prim"], pr["uv"], pr["g0"])
    c["ray_sums"] = G.vertex_sums(scene, rr["inst"], rr["prim"], c["ray_ref"][1], c["ray_ref"][2])
    c["point_sums"] = G.vertex_sums(scene, pr["inst"], pr["prim"], c["point_ref"][1], c["point_ref"][2])
    for a in list(rr.values()) + list(pr.values()) + list(c["ray_ref"]) + list(c["point_ref"]) + list(c["ray_sums"]) + list(c["point_sums"]):
        a.setflags(write=False)
    return c


def _dev(torch, a, dtype=np.float32):
    if a is None:
        return None
    a = np.array(a, dtype=dtype)
    return torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).cuda()


def _ptr(a):
    return None if a is None else a.data_ptr()


def _run_rays(torch, r, rec, sel=slice(None), grad_t=True, grad_uv=True, want_rays=True, want_xyz=True, n_vertices=16, stats=False):
    """crt_trace_rays_backward_device over the records `sel`: (grad_rays or None, grad_xyz or None, stats); four sentinel floats
    behind each output stay as they are"""
    d = {k: _dev(torch, rec[k][sel], np.uint32 if k in ("inst", "prim") else np.float32) for k in ("rays", "inst", "prim", "t", "uv", "g0", "g1")}
    n = len(d["inst"])
    out_r = torch.full((8 * n + 4,), -7.0, dtype=torch.float32, device="cuda") if want_rays else None
    out_x = torch.full((3 * n_vertices + 4,), -7.0, dtype=torch.float32, device="cuda") if want_xyz else None
    torch.cuda.synchronize()
    st = r.trace_rays_backward_device(n, _ptr(d["rays"]), _ptr(d["inst"]), _ptr(d["prim"]), _ptr(d["t"]), _ptr(d["uv"]), _ptr(d["g0"]) if grad_t else None,
                                      _ptr(d["g1"]) if grad_uv else None, _ptr(out_r), _ptr(out_x), stats=stats)
    r.synchronize()
    got = []
    for o, m in ((out_r, 8 * n), (out_x, 3 * n_vertices)):
        if o is None:
            got.append(None)
            continue
        h = o.cpu().numpy()
        assert np.all(h[m:] == -7.0), "nothing is written behind an output"
        got.append(h[:m])
    return got[0], got[1], st


def _run_points(torch, r, rec, sel=slice(None), want_points=True, want_xyz=True, n_vertices=16, stats=False):
    d = {k: _dev(torch, rec[k][sel], np.uint32 if k in ("inst", "prim") else np.float32) for k in ("points", "inst", "prim", "uv", "g0")}
    n = len(d["inst"])
    out_p = torch.full((4 * n + 4,), -7.0, dtype=torch.float32, device="cuda") if want_points else None
    out_x = torch.full((3 * n_vertices + 4,), -7.0, dtype=torch.float32, device="cuda") if want_xyz else None
    torch.cuda.synchronize()
    st = r.closest_points_backward_device(n, _ptr(d["points"]), _ptr(d["inst"]), _ptr(d["prim"]), _ptr(d["uv"]), _ptr(d["g0"]), _ptr(out_p), _ptr(out_x),
                                          stats=stats)
    r.synchronize()
    got = []
    for o, m in ((out_p, 4 * n), (out_x, 3 * n_vertices)):
        if o is None:
            got.append(None)
            continue
        h = o.cpu().numpy()
        assert np.all(h[m:] == -7.0), "nothing is written behind an output"
        got.append(h[:m])
    return got[0], got[1], st


# ---- GPU

@pytest.mark.gpu
def test_records_cover_the_cases(case):
    """what the assertions below rest on: hits of both meshes, misses with infinite and with finite t, rays through the quad's shared
    diagonal and its corners, points on the surface, and an edited tail that the reference holds inert"""
    rr, pr = case["rays"], case["points"]
    live_r, live_p = case["ray_ref"][2], case["point_ref"][2]
    body = np.arange(N) < N - 8
    for rec in (rr, pr):
        assert all(((rec["inst"] == m) & body).sum() > 50 for m in (0, 1)), "both meshes"
        assert ((rec["inst"] == MISS) & body).sum() > 50, "misses"
    miss = (rr["inst"] == MISS) & body
    assert np.isinf(rr["t"][miss]).any() and np.isfinite(rr["t"][miss]).any()
    assert not live_r[miss].any() and not live_r[rr["edited"]].any() and not live_p[pr["edited"]].any()
    assert live_r[(rr["inst"] != MISS) & body].all(), "every forward hit is a live record"
    on_edge = (rr["inst"] == 0) & body & ((rr["uv"][:, 0] < 1e-5) | (rr["uv"][:, 1] < 1e-5) | (rr["uv"].sum(-1) > 1 - 1e-5))
    assert on_edge.sum() >= 8, "rays through the quad's diagonal and corners hit it there"
    assert (pr["dist"][:4] == 0).all() and not live_p[:4].any(), "a point on the surface is inert"
    assert live_p[(pr["inst"] != MISS) & body & (pr["dist"] > 0)].all()
    S, A, m = case["ray_sums"]
    assert (m[:4] > 0).all() and (m[4:] > 0).sum() >= 18 and m.max() > 100, "shared vertices take hundreds of contributions"
    t = rr["t"][(rr["inst"] != MISS) & body]
    assert t.max() / t.min() > 1e5, "directions scaled by 1e-3 and 1e3"


@pytest.mark.gpu
def test_rays_equal_the_reference(renderer, case):
    """grad_rays equals grad_reference.c bit for bit on all 2049 records; grad_xyz lies within the bound; stats count the records"""
    import torch
    grad_rays, grad_xyz, st = _run_rays(torch, renderer, case["rays"], stats=True)
    assert np.array_equal(_bits(grad_rays), _bits(case["ray_ref"][0]).reshape(-1))
    inert = ~case["ray_ref"][2]
    assert not _bits(grad_rays).reshape(N, 8)[inert].any(), "an inert record's gradient is +0.0"
    worst = G.check_vertex_sums(grad_xyz, *case["ray_sums"], what="rays")
    print("rays: worst |grad_xyz - S| = %.3g of the bound" % worst)
    assert st["rays_primary"] == N and st["kernel_ms"] > 0.0 and st["total_ms"] > 0.0
    assert not any(st[k] for k in ("rays_shadow", "nodes_visited", "tris_tested"))


@pytest.mark.gpu
def test_points_equal_the_reference(renderer, case):
    import torch
    grad_points, grad_xyz, st = _run_points(torch, renderer, case["points"], stats=True)
    assert np.array_equal(_bits(grad_points), _bits(case["point_ref"][0]).reshape(-1))
    assert not _bits(grad_points).reshape(N, 4)[~case["point_ref"][2]].any()
    worst = G.check_vertex_sums(grad_xyz, *case["point_sums"], what="points")
    print("points: worst |grad_xyz - S| = %.3g of the bound" % worst)
    assert st["rays_primary"] == N and st["kernel_ms"] > 0.0
    # the gradient with respect to the point is the unit vector from the surface point, times g
    live = case["point_ref"][2]
    unit = grad_points.reshape(N, 4)[live, :3].astype(np.float64) / case["points"]["g0"][live].astype(np.float64)[:, None]
    assert np.abs(np.linalg.norm(unit, axis=-1) - 1).max() < 1e-6


@pytest.mark.gpu
def test_optional_buffers_and_small_n(refs, renderer, case):
    """a NULL grad_xyz or per-record output changes nothing in the other; grad_t or grad_uv NULL is zeros; n = 1 works; n = 0
    returns CRT_OK, looks at no buffer and writes nothing"""
    import torch
    rr, pr, scene = case["rays"], case["points"], case["scene"]
    grad_rays, none, _ = _run_rays(torch, renderer, rr, want_xyz=False)
    assert none is None and np.array_equal(_bits(grad_rays), _bits(case["ray_ref"][0]).reshape(-1))
    none, grad_xyz, _ = _run_rays(torch, renderer, rr, want_rays=False)
    assert none is None
    G.check_vertex_sums(grad_xyz, *case["ray_sums"], what="rays, grad_rays NULL")
    grad_points, none, _ = _run_points(torch, renderer, pr, want_xyz=False)
    assert none is None and np.array_equal(_bits(grad_points), _bits(case["point_ref"][0]).reshape(-1))
    none, grad_xyz, _ = _run_points(torch, renderer, pr, want_points=False)
    G.check_vertex_sums(grad_xyz, *case["point_sums"], what="points, grad_points NULL")
    for gt, gu in ((True, False), (False, True)):
        want = G.ray_reference(refs["f32"], scene, rr["rays"], rr["inst"], rr["prim"], rr["t"], rr["uv"], rr["g0"] if gt else None, rr["g1"] if gu else None)
        grad_rays, grad_xyz, _ = _run_rays(torch, renderer, rr, grad_t=gt, grad_uv=gu)
        assert np.array_equal(_bits(grad_rays), _bits(want[0]).reshape(-1)), (gt, gu)
        G.check_vertex_sums(grad_xyz, *G.vertex_sums(scene, rr["inst"], rr["prim"], want[1], want[2]), what="one incoming gradient NULL")
    first_hit = int(np.nonzero(case["ray_ref"][2])[0][0])
    sel = slice(first_hit, first_hit + 1)
    grad_rays, grad_xyz, _ = _run_rays(torch, renderer, rr, sel)
    assert np.array_equal(_bits(grad_rays), _bits(case["ray_ref"][0][sel]).reshape(-1)) and grad_rays[:3].any()
    G.check_vertex_sums(grad_xyz, *G.vertex_sums(scene, rr["inst"][sel], rr["prim"][sel], case["ray_ref"][1][sel], case["ray_ref"][2][sel]), what="n = 1")
    assert 0 < (grad_xyz != 0).sum() <= 9 and (_bits(grad_xyz) == 0).sum() >= 3 * 13, "one triangle's vertices; the other 13 read +0.0"
    first_hit = int(np.nonzero(case["point_ref"][2])[0][0])
    sel = slice(first_hit, first_hit + 1)
    grad_points, grad_xyz, _ = _run_points(torch, renderer, pr, sel)
    assert np.array_equal(_bits(grad_points), _bits(case["point_ref"][0][sel]).reshape(-1))
    G.check_vertex_sums(grad_xyz, *G.vertex_sums(scene, pr["inst"][sel], pr["prim"][sel], case["point_ref"][1][sel], case["point_ref"][2][sel]),
                        what="points, n = 1")
    keep = torch.full((64,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = renderer.trace_rays_backward_device(0, None, None, None, None, None, None, None, keep.data_ptr(), keep.data_ptr(), stats=True)
    assert st["rays_primary"] == 0 and st["kernel_ms"] == 0.0
    renderer.closest_points_backward_device(0, None, None, None, None, None, keep.data_ptr(), keep.data_ptr())
    renderer.synchronize()
    assert bool((keep == -7.0).all().item())
    out = renderer.trace_rays_backward(np.zeros((0, 8), np.float32), [], [], [], np.zeros((0, 2), np.float32), grad_t=[])
    assert out["grad_rays"].shape == (0, 8) and out["grad_xyz"].shape == (16, 3)
    out = renderer.closest_points_backward(np.zeros((0, 4), np.float32), [], [], np.zeros((0, 2), np.float32), [])
    assert out["grad_points"].shape == (0, 4)


@pytest.mark.gpu
def test_host_forms_equal_device_forms(renderer, case):
    """the staged host calls give the device calls' per-record bits (which equal the reference) and vertex sums within the bound"""
    rr, pr = case["rays"], case["points"]
    out = renderer.trace_rays_backward(rr["rays"], rr["inst"], rr["prim"], rr["t"], rr["uv"], rr["g0"], rr["g1"])
    assert np.array_equal(_bits(out["grad_rays"]), _bits(case["ray_ref"][0]))
    G.check_vertex_sums(out["grad_xyz"], *case["ray_sums"], what="host rays")
    only = renderer.trace_rays_backward(rr["rays"], rr["inst"], rr["prim"], rr["t"], rr["uv"], rr["g0"], rr["g1"], want=("grad_xyz",))
    assert set(only) == {"grad_xyz"}
    G.check_vertex_sums(only["grad_xyz"], *case["ray_sums"], what="host rays, grad_xyz alone")
    out = renderer.closest_points_backward(pr["points"], pr["inst"], pr["prim"], pr["uv"], pr["g0"])
    assert np.array_equal(_bits(out["grad_points"]), _bits(case["point_ref"][0]))
    G.check_vertex_sums(out["grad_xyz"], *case["point_sums"], what="host points")


@pytest.mark.gpu
def test_contention_on_one_triangle(pkg, refs):
    """65 536 rays that all hit one triangle: each of its nine vertex components is the sum of 65 536 contributions and stays within
    the same bound"""
    import torch
    n = 65536
    tri = {"vertices": np.float32([(-1, -1, 0), (1.5, -1, 0.2), (-0.5, 1.5, -0.1)]), "triangles": np.uint32([(0, 1, 2)]), "material_index": 0,
           "normals": None}
    rng = np.random.default_rng(31)
    uv = rng.uniform(0.02, 0.48, size=(n, 2))
    V = tri["vertices"].astype(np.float64)
    target = V[0] + uv[:, :1] * (V[1] - V[0]) + uv[:, 1:] * (V[2] - V[0])
    o = target + np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(2, 4, n)], -1)
    rays = pkg.make_rays(o, target - o)
    r = pkg.Renderer(0)
    try:
        r.upload([tri], LIGHTS, MATS, dynamic=True)
        hit = r.trace_rays(rays)
        assert (hit["inst"] == 0).all() and (hit["prim"] == 0).all()
        rec = {"rays": rays, "inst": hit["inst"], "prim": hit["prim"], "t": hit["t"], "uv": hit["uv"], "g0": rng.normal(size=n).astype(np.float32),
               "g1": rng.normal(size=(n, 2)).astype(np.float32)}
        scene = G.SceneArrays([(r.mesh_vertices(0)[0], tri["triangles"])])
        want = G.ray_reference(refs["f32"], scene, rays, rec["inst"], rec["prim"], rec["t"], rec["uv"], rec["g0"], rec["g1"])
        assert want[2].all()
        grad_rays, grad_xyz, _ = _run_rays(torch, r, rec, n_vertices=3)
    finally:
        r.close()
    assert np.array_equal(_bits(grad_rays), _bits(want[0]).reshape(-1))
    S, A, m = G.vertex_sums(scene, rec["inst"], rec["prim"], want[1], want[2])
    assert (m == n).all()
    worst = G.check_vertex_sums(grad_xyz, S, A, m, what="contention")
    print("contention: worst |grad_xyz - S| = %.3g of the bound" % worst)


@pytest.mark.gpu
def test_refit_and_rebuild_change_nothing(pkg, refs, case):
    """after update_vertices + crt_refit, and after crt_rebuild with either builder, the per-record outputs for the same records are
    bitwise equal across the three trees and equal the reference over the moved vertices; grad_xyz stays within the bound"""
    import torch
    rr, pr = case["rays"], case["points"]
    r = pkg.Renderer(0)
    try:
        meshes = _upload_scene(r)
        moved = meshes[1]["vertices"] * np.float32(1.05) + np.float32([0.02, -0.01, 0.03])
        r.update_vertices(1, moved)
        r.update_vertices(0, meshes[0]["vertices"] + np.float32([0.0, 0.05, -0.1]))
        r.refit()
        scene = _scene_arrays(r, meshes)
        assert not np.array_equal(scene.world, case["scene"].world)
        want_r = G.ray_reference(refs["f32"], scene, rr["rays"], rr["inst"], rr["prim"], rr["t"], rr["uv"], rr["g0"], rr["g1"])
        want_p = G.point_reference(refs["f32"], scene, pr["points"], pr["inst"], pr["prim"], pr["uv"], pr["g0"])
        sums_r = G.vertex_sums(scene, rr["inst"], rr["prim"], want_r[1], want_r[2])
        sums_p = G.vertex_sums(scene, pr["inst"], pr["prim"], want_p[1], want_p[2])
        for tree in ("refit", "rebuild LBVH", "rebuild PLOC"):
            if tree != "refit":
                r.set_option("gpu_builder", 0 if tree.endswith("LBVH") else 1)
                r.rebuild()
            grad_rays, grad_xyz, _ = _run_rays(torch, r, rr)
            assert np.array_equal(_bits(grad_rays), _bits(want_r[0]).reshape(-1)), tree
            G.check_vertex_sums(grad_xyz, *sums_r, what=tree)
            grad_points, grad_xyz, _ = _run_points(torch, r, pr)
            assert np.array_equal(_bits(grad_points), _bits(want_p[0]).reshape(-1)), tree
            G.check_vertex_sums(grad_xyz, *sums_p, what=tree + ", points")
    finally:
        r.close()


@pytest.mark.gpu
def test_errors(pkg, renderer, case):
    """CRT_ESTATE before an upload and on a scene uploaded without "dynamic"; CRT_EINVAL for a NULL input, for both incoming
    gradients or both outputs NULL and for misaligned device pointers; a failed call writes nothing"""
    import torch
    L = pkg.lib()
    n = 16
    f = torch.full((8 * n + 8,), -7.0, dtype=torch.float32, device="cuda")
    x = torch.full((3 * 16 + 8,), -7.0, dtype=torch.float32, device="cuda")
    ids = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    src = torch.zeros(8 * n + 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    F, X, I, S = f.data_ptr(), x.data_ptr(), ids.data_ptr(), src.data_ptr()
    hf, hx, hi, hs = np.full(8 * n, -7.0, np.float32), np.full(48, -7.0, np.float32), np.zeros(n, np.uint32), np.zeros(8 * n, np.float32)

    def rays_dev(r, **o):
        return L.crt_trace_rays_backward_device(r.h, o.get("n", n), o.get("rays", S), o.get("inst", I), o.get("prim", I), o.get("t", S), o.get("uv", S),
                                                o.get("gt", S), o.get("guv", S), o.get("out", F), o.get("xyz", X), None)

    def points_dev(r, **o):
        return L.crt_closest_points_backward_device(r.h, o.get("n", n), o.get("points", S), o.get("inst", I), o.get("prim", I), o.get("uv", S),
                                                    o.get("g", S), o.get("out", F), o.get("xyz", X), None)

    def rays_host(r, **o):
        p = hs.ctypes.data
        return L.crt_trace_rays_backward(r.h, o.get("n", n), o.get("rays", p), o.get("inst", hi.ctypes.data), o.get("prim", hi.ctypes.data), o.get("t", p),
                                         o.get("uv", p), o.get("gt", p), o.get("guv", p), o.get("out", hf.ctypes.data), o.get("xyz", hx.ctypes.data), None)

    def points_host(r, **o):
        p = hs.ctypes.data
        return L.crt_closest_points_backward(r.h, o.get("n", n), o.get("points", p), o.get("inst", hi.ctypes.data), o.get("prim", hi.ctypes.data),
                                             o.get("uv", p), o.get("g", p), o.get("out", hf.ctypes.data), o.get("xyz", hx.ctypes.data), None)

    def untouched():
        torch.cuda.synchronize()
        return bool((f == -7.0).all().item()) and bool((x == -7.0).all().item()) and np.all(hf == -7.0) and np.all(hx == -7.0)

    fresh = pkg.Renderer(0)
    try:
        for call in (rays_dev, points_dev, rays_host, points_host):
            assert call(fresh) == ESTATE and call(fresh, n=0) == ESTATE, call.__name__
        fresh.upload([_quad()], LIGHTS, MATS, dynamic=False)
        for call in (rays_dev, points_dev, rays_host, points_host):
            assert call(fresh) == ESTATE and "dynamic" in L.crt_last_error(fresh.h).decode(), call.__name__
    finally:
        fresh.close()
    assert untouched()
    r = renderer
    for call, inputs in ((rays_dev, ("rays", "inst", "prim", "t", "uv")), (rays_host, ("rays", "inst", "prim", "t", "uv")),
                         (points_dev, ("points", "inst", "prim", "uv", "g")), (points_host, ("points", "inst", "prim", "uv", "g"))):
        for g in inputs:
            assert call(r, **{g: None}) == EINVAL, (call.__name__, g)
        assert call(r, out=None, xyz=None) == EINVAL and "output" in L.crt_last_error(r.h).decode(), call.__name__
        assert call(r, n=0, inst=None, out=None, xyz=None) == 0, "n = 0 looks at no buffer"
    for call in (rays_dev, rays_host):
        assert call(r, gt=None, guv=None) == EINVAL and "grad_t" in L.crt_last_error(r.h).decode()
    for g in ("rays", "out"):
        assert rays_dev(r, **{g: (S if g == "rays" else F) + 8}) == EINVAL and "aligned" in L.crt_last_error(r.h).decode(), g
    for g in ("uv", "guv"):
        assert rays_dev(r, **{g: S + 4}) == EINVAL, g
    for g, base in (("inst", I), ("prim", I), ("t", S), ("gt", S), ("xyz", X)):
        assert rays_dev(r, **{g: base + 2}) == EINVAL, g
    for g in ("points", "out"):
        assert points_dev(r, **{g: (S if g == "points" else F) + 8}) == EINVAL, g
    assert points_dev(r, uv=S + 4) == EINVAL
    for g, base in (("inst", I), ("prim", I), ("g", S), ("xyz", X)):
        assert points_dev(r, **{g: base + 2}) == EINVAL, g
    assert untouched()
    # the controls: all-zero records name (inst 0, prim 0) with a zero direction, inert by their lambda: the outputs are zeros
    for call in (rays_dev, points_dev, rays_host, points_host):
        assert call(r) == 0, call.__name__
    r.synchronize()
    assert not bool((f[:4 * n] == -7.0).any().item()) and bool((f[8 * n:] == -7.0).all().item())
    assert not bool((x[:48] == -7.0).any().item()) and bool((x[48:] == -7.0).all().item())
    assert not np.any(hf[:4 * n] == -7.0) and not np.any(hx == -7.0)


@pytest.mark.gpu
def test_torch_layer(pkg, renderer, case):
    """.backward() through trace_rays_torch and closest_points_torch gives the raw calls' grad_rays / grad_points bitwise and, per
    mesh named in `vertices`, its slice of grad_xyz times the transposed 3x3 of its transform computed the same way in torch; a mesh
    that is not named gets no gradient; the forward outputs are the plain queries'"""
    import torch
    rr, pr, meshes = case["rays"], case["points"], case["meshes"]
    M3 = torch.from_numpy(np.ascontiguousarray(_transform()[:, :3])).cuda()
    rest = [torch.from_numpy(m["vertices"].copy()).cuda() for m in meshes]
    plain = renderer.trace_rays(rr["rays"])
    w_t, w_uv = torch.from_numpy(np.where(np.isfinite(rr["g0"]), rr["g0"], 1.0).astype(np.float32)).cuda(), torch.from_numpy(rr["g1"].copy()).cuda()
    for named in ((0, 1), (1,)):
        rays = torch.from_numpy(rr["rays"].copy()).cuda().requires_grad_(True)
        verts = {m: rest[m].clone().requires_grad_(True) for m in named}
        other = rest[0].clone().requires_grad_(True)
        t, uv, inst, prim = renderer.trace_rays_torch(rays, verts)
        assert t.requires_grad and uv.requires_grad and not inst.requires_grad and not prim.requires_grad
        assert np.array_equal(_bits(t.detach().cpu().numpy()), _bits(plain["t"])) and np.array_equal(_bits(uv.detach().cpu().numpy()), _bits(plain["uv"]))
        assert np.array_equal(inst.cpu().numpy().view(np.uint32), plain["inst"]) and np.array_equal(prim.cpu().numpy().view(np.uint32), plain["prim"])
        hit = inst >= 0
        (torch.where(hit, t, torch.zeros_like(t)) * w_t).sum().add((uv * w_uv).sum()).backward()
        raw = renderer.trace_rays_backward(rr["rays"], plain["inst"], plain["prim"], plain["t"], plain["uv"], torch.where(hit, w_t, torch.zeros_like(w_t)).cpu().numpy(), rr["g1"])
        assert np.array_equal(_bits(rays.grad.cpu().numpy()), _bits(raw["grad_rays"])), named
        assert not rays.grad[:, 3].any() and not rays.grad[:, 7].any() and not rays.grad[~hit].any(), "tmin, tmax and misses get zero"
        gx = torch.from_numpy(raw["grad_xyz"]).cuda()
        if 0 in named:  # the sums are not bit-reproducible from call to call: within the bound's last bit of each other
            assert torch.allclose(verts[0].grad, gx[:4], rtol=2e-7, atol=1e-9)
        assert torch.allclose(verts[1].grad, gx[4:] @ M3, rtol=1e-5, atol=1e-6) and verts[1].grad.shape == (12, 3)
        assert other.grad is None
    # the transposed 3x3, exactly: a loss whose world gradient is known in closed form.  One ray, one hit on the icosphere
    i = int(np.nonzero(plain["inst"] == 1)[0][0])
    rays = torch.from_numpy(rr["rays"][i:i + 1].copy()).cuda()
    verts = {1: rest[1].clone().requires_grad_(True)}
    t, uv, inst, prim = renderer.trace_rays_torch(rays, verts)
    t.sum().backward()
    raw = renderer.trace_rays_backward(rr["rays"][i:i + 1], plain["inst"][i:i + 1], plain["prim"][i:i + 1], plain["t"][i:i + 1], plain["uv"][i:i + 1],
                                       np.ones(1, np.float32), None, want=("grad_xyz",))
    want = torch.from_numpy(raw["grad_xyz"][4:]).cuda() @ M3  # three contributions, one per vertex: the sums are exact
    assert np.array_equal(_bits(verts[1].grad.cpu().numpy()), _bits(want.cpu().numpy())) and (verts[1].grad != 0).any()
    # points
    plain = renderer.closest_points(pr["points"])
    points = torch.from_numpy(pr["points"].copy()).cuda().requires_grad_(True)
    verts = {1: rest[1].clone().requires_grad_(True)}
    dist, point, uv, inst, prim = renderer.closest_points_torch(points, verts)
    assert dist.requires_grad and not any(o.requires_grad for o in (point, uv, inst, prim))
    assert np.array_equal(_bits(dist.detach().cpu().numpy()), _bits(plain["dist"])) and np.array_equal(_bits(point.cpu().numpy()), _bits(plain["point"]))
    w = torch.from_numpy(np.where(np.isfinite(pr["g0"]), pr["g0"], 1.0).astype(np.float32)).cuda()
    hit = inst >= 0
    (torch.where(hit, dist * w, torch.zeros_like(dist))).sum().backward()
    raw = renderer.closest_points_backward(pr["points"], plain["inst"], plain["prim"], plain["uv"], torch.where(hit, w, torch.zeros_like(w)).cpu().numpy())
    assert np.array_equal(_bits(points.grad.cpu().numpy()), _bits(raw["grad_points"]))
    assert not points.grad[:, 3].any() and points.grad[hit].any()
    assert torch.allclose(verts[1].grad, torch.from_numpy(raw["grad_xyz"][4:]).cuda() @ M3, rtol=1e-5, atol=1e-6)
    # a change of the scene between forward and backward is refused
    verts = {1: rest[1].clone().requires_grad_(True)}
    t, _, inst, _ = renderer.trace_rays_torch(torch.from_numpy(rr["rays"].copy()).cuda(), verts)
    renderer.update_vertices(1, meshes[1]["vertices"])
    with pytest.raises(pkg.CrtError):
        torch.where(inst >= 0, t, torch.zeros_like(t)).sum().backward()


def _descent_simulation():
    """the descent of test_descent in torch float64 with brute-force hits over the quad's two triangles: the four losses"""
    import torch
    V = torch.tensor([(-2, -2, 5), (2, -2, 5), (2, 2, 5), (-2, 2, 5)], dtype=torch.float64, requires_grad=True)
    tris = ((0, 1, 2), (0, 2, 3))
    g = np.linspace(-0.9, 0.9, 16)
    o = torch.tensor(np.stack([np.tile(g, 16), np.repeat(g, 16), np.zeros(256)], -1))
    d = torch.tensor([0.1, -0.05, 1.0], dtype=torch.float64).expand(256, 3)
    losses = []
    for step in range(4):
        ts = []
        for tri in tris:
            a, b, c = V[tri[0]], V[tri[1]], V[tri[2]]
            M = torch.stack([-d, (b - a).expand(256, 3), (c - a).expand(256, 3)], -1)
            x = torch.linalg.solve(M, (o - a).unsqueeze(-1)).squeeze(-1)
            ok = (x[:, 0] > 0) & (x[:, 1] >= 0) & (x[:, 2] >= 0) & (x[:, 1] + x[:, 2] <= 1)
            ts.append(torch.where(ok, x[:, 0], torch.full_like(x[:, 0], float("inf"))))
        t = torch.minimum(ts[0], ts[1])
        assert bool(torch.isfinite(t).all()), "all 256 rays hit throughout"
        loss = ((t - 6.0) ** 2).mean()
        losses.append(float(loss.detach()))
        if step < 3:
            (grad,) = torch.autograd.grad(loss, V)
            V = (V - grad).detach().requires_grad_(True)
    return losses


@pytest.mark.gpu
def test_descent(pkg):
    """a quad [-2, 2]^2 at z = 5, 256 rays from a 16 x 16 grid on [-0.9, 0.9]^2 at z = 0 along (0.1, -0.05, 1), loss mean((t - 6)^2),
    three plain gradient steps on the vertices with lr = 1: every loss lies within 1e-3 relative of the float64 simulation (1, 0.101,
    0.0154, 0.00623 there) and the last one below 1 % of the first"""
    import torch
    sim = _descent_simulation()
    assert abs(sim[0] - 1.0) < 1e-12 and sim[3] < 0.01 * sim[0], sim
    quad = {"vertices": np.float32([(-2, -2, 5), (2, -2, 5), (2, 2, 5), (-2, 2, 5)]), "triangles": np.uint32([(0, 1, 2), (0, 2, 3)]), "material_index": 0,
            "normals": None}
    g = np.linspace(-0.9, 0.9, 16)
    rays = torch.from_numpy(pkg.make_rays(np.stack([np.tile(g, 16), np.repeat(g, 16), np.zeros(256)], -1), (0.1, -0.05, 1.0))).cuda()
    r = pkg.Renderer(0)
    try:
        r.upload([quad], LIGHTS, MATS, dynamic=True)
        V = torch.from_numpy(quad["vertices"].copy()).cuda().requires_grad_(True)
        losses = []
        for step in range(4):
            t, _, inst, _ = r.trace_rays_torch(rays, {0: V})
            assert bool((inst == 0).all().item()), step
            loss = ((t - 6.0) ** 2).mean()
            losses.append(float(loss.detach()))
            if step < 3:
                (grad,) = torch.autograd.grad(loss, V)
                V = (V - grad).detach().requires_grad_(True)
    finally:
        r.close()
    print("descent: GPU losses %s, float64 simulation %s" % (["%.6g" % x for x in losses], ["%.6g" % x for x in sim]))
    for got, want in zip(losses, sim):
        assert abs(got - want) <= 1e-3 * want, (losses, sim)
    assert losses[3] < 0.01 * losses[0]


@pytest.mark.gpu
def test_cpp_layer(pkg, renderer, case, tmp_path):
    """crt::Renderer::traceRaysBackward and closestPointsBackward, from a small C++ program linked against libcrt_hip.so, give the C
    calls' per-record bits on the Cornell box and vertex gradients within a few ulps of them"""
    exe = str(tmp_path / "grad_cpp")
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(lib_dir, "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "grad_cpp.cpp"), "-L" + lib_dir, "-lcrt_hip",
                           "-Wl,-rpath," + lib_dir, "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    import importlib
    scenes = importlib.import_module(pkg.__name__ + ".scenes")
    scene = pkg.Scene.from_arrays(scenes.cornell_box())
    path = str(tmp_path / "cornell.crtbin")
    scene.save(path)
    w, h = 24, 16
    n = w * h
    r = pkg.Renderer(0)
    try:
        r.upload_scene(scene, dynamic=True)
        r.set_camera_from(scene)
        rays = r.camera_rays(w, h)
        hit = r.trace_rays(rays)
        assert 16 <= (hit["inst"] != MISS).sum() < n, "the frame sees the box and its surroundings"
        i = np.arange(n)
        g_t = np.where(hit["inst"] != MISS, (i % 7 + 1) * 0.25, 0.0).astype(np.float32)
        g_uv = np.stack([(i % 5 - 2) * 0.5, (i % 3 - 1) * 0.25], -1).astype(np.float32)
        want = r.trace_rays_backward(rays, hit["inst"], hit["prim"], hit["t"], hit["uv"], g_t, g_uv)
        # the ray origins as points against the hits' surface points: any (inst, prim, uv) is a valid record
        want_p = r.closest_points_backward(pkg.make_points(rays[:, 0:3]), hit["inst"], hit["prim"], hit["uv"], g_t)
    finally:
        r.close()
        scene.close()
    out = str(tmp_path / "out.bin")
    subprocess.check_call([exe, path, str(w), str(h), out], timeout=120)
    raw = np.fromfile(out, dtype=np.float32)
    nv = want["grad_xyz"].size
    assert raw.size == 8 * n + nv + 4 * n + nv
    assert np.array_equal(_bits(raw[:8 * n]), _bits(want["grad_rays"]).reshape(-1)), "traceRaysBackward"
    assert np.allclose(raw[8 * n:8 * n + nv], want["grad_xyz"].reshape(-1), rtol=1e-6, atol=1e-9) and want["grad_xyz"].any()
    assert np.array_equal(_bits(raw[8 * n + nv:12 * n + nv]), _bits(want_p["grad_points"]).reshape(-1)), "closestPointsBackward"
    assert np.allclose(raw[12 * n + nv:], want_p["grad_xyz"].reshape(-1), rtol=1e-6, atol=1e-9) and want_p["grad_xyz"].any()
