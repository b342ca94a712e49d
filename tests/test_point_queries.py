"""Point queries (crt_closest_points* / crt_count_hits* / crt_occupancy*, include/crt_hip.h): closest surface point, hit counts
and occupancy.  The GPU results are compared bit for bit (float bits as uint32) with tests/point_reference.c, a brute-force
restatement of the three queries over the exported triangle records in the kernels' operation order; the reference itself
is checked against an independent float64 closest-point computation and a float64 generalised winding number."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("crt_closest_points_device", "crt_closest_points", "crt_count_hits_device", "crt_count_hits",
           "crt_occupancy_device", "crt_occupancy")
MISS = 0xFFFFFFFF
TREES = {"sah": {"gpu_build": 0}, "lbvh": {"gpu_build": 1, "gpu_builder": 0}, "ploc": {"gpu_build": 1, "gpu_builder": 1}}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the reference (tests/point_reference.c)

@pytest.fixture(scope="session")
def ref(pkg, tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for tests/point_reference.c")
    out = str(tmp_path_factory.mktemp("point_reference") / "libpoint_reference.so")
    base = [cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tests", "point_reference.c"), "-o", out, "-lm"]
    if subprocess.call(base[:1] + ["-fopenmp"] + base[1:], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)  # (no OpenMP: the pragmas are ignored)
    L = C.CDLL(out)
    vp, u32 = C.c_void_p, C.c_uint32
    L.ref_closest_on_tri.argtypes = [vp, vp, vp, vp, vp]
    L.ref_closest_points.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp]
    L.ref_count_hits.argtypes = [vp, u32, u32, vp, vp]
    L.ref_occupancy.argtypes = [vp, u32, u32, vp, vp, vp]
    for f in (L.ref_closest_on_tri, L.ref_closest_points, L.ref_count_hits, L.ref_occupancy):
        f.restype = None
    return L


def _tri_records(pkg, meshes):
    """leaf-order-free records {v0, e1 = v1 - v0, e2 = v2 - v0} in float32 with inst / prim / gid, as an upload writes them"""
    recs, gid = [], 0
    for i, m in enumerate(meshes):
        v = np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3)
        t = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)
        r = np.zeros(len(t), dtype=pkg.TRI_DTYPE)
        r["v0"] = v[t[:, 0]]
        r["e1"] = v[t[:, 1]] - v[t[:, 0]]
        r["e2"] = v[t[:, 2]] - v[t[:, 0]]
        r["inst"] = i
        r["prim"] = np.arange(len(t))
        r["gid"] = gid + np.arange(len(t))
        gid += len(t)
        recs.append(r)
    return np.ascontiguousarray(np.concatenate(recs)) if recs else np.zeros(0, dtype=pkg.TRI_DTYPE)


def ref_closest(ref, tris, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)
    n = len(pts)
    out = {"dist": np.zeros(n, np.float32), "point": np.zeros((n, 3), np.float32), "uv": np.zeros((n, 2), np.float32),
           "inst": np.zeros(n, np.uint32), "prim": np.zeros(n, np.uint32)}
    ref.ref_closest_points(tris.ctypes.data, len(tris), n, pts.ctypes.data, *[out[k].ctypes.data for k in ("dist", "point", "uv", "inst", "prim")])
    return out


def ref_count(ref, tris, rays):
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    out = np.zeros(len(rays), np.uint32)
    ref.ref_count_hits(tris.ctypes.data, len(tris), len(rays), rays.ctypes.data, out.ctypes.data)
    return out


def ref_occupancy(ref, tris, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)
    out = np.zeros(len(pts), np.uint8)
    ref.ref_occupancy(tris.ctypes.data, len(tris), len(pts), pts.ctypes.data, out.ctypes.data, None)
    return out.astype(bool)


# ---- float64 yardsticks

def closest_f64(p, a, b, c):
    """distance from p to triangle (a, b, c) in float64: the plane projection when it lies inside, else the nearest of the
    three segments (degenerate triangles: segments only)"""
    p, a, b, c = (np.asarray(x, dtype=np.float64) for x in (p, a, b, c))

    def seg(s, e):
        d = e - s
        dd = d @ d
        t = 0.0 if dd == 0.0 else min(max((p - s) @ d / dd, 0.0), 1.0)
        return np.linalg.norm(p - (s + t * d))
    best = min(seg(a, b), seg(a, c), seg(b, c))
    n = np.cross(b - a, c - a)
    nn = n @ n
    if nn > 0.0:
        q = p - ((p - a) @ n) / nn * n
        w = [np.cross(c - b, q - b) @ n, np.cross(a - c, q - c) @ n, np.cross(b - a, q - a) @ n]
        if min(w) >= 0.0:
            best = min(best, np.linalg.norm(p - q))
    return best


def winding_number(V, F, pts):
    """generalised winding number (sum of signed solid angles / 4 pi, Van Oosterom-Strackee) of points w.r.t. a mesh, float64"""
    V = np.asarray(V, dtype=np.float64)
    A, B, Cc = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    out = np.zeros(len(pts))
    for i, p in enumerate(np.asarray(pts, dtype=np.float64)):
        a, b, c = A - p, B - p, Cc - p
        la, lb, lc = (np.linalg.norm(x, axis=1) for x in (a, b, c))
        det = np.einsum("ij,ij->i", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("ij,ij->i", a, b) * lc + np.einsum("ij,ij->i", b, c) * la + np.einsum("ij,ij->i", c, a) * lb
        out[i] = np.sum(2.0 * np.arctan2(det, den)) / (4.0 * math.pi)
    return out


def _icosphere_mesh(scenes, subdiv, r, c):
    v, f = scenes._icosphere(subdiv)
    return {"vertices": (np.float32(r * v) + np.float32(c)).astype(np.float32), "triangles": f.astype(np.uint32),
            "material_index": 0, "normals": None}


# ---- CPU: the interface exists, the reference is right

def test_binding_and_library_expose_point_queries(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
    for name in ("closest_points", "count_hits", "occupancy", "signed_distance", "closest_points_device", "count_hits_device",
                 "occupancy_device"):
        assert callable(getattr(pkg.Renderer, name, None)), name
    assert L.crt_abi_version() == 1


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    pts = np.zeros((4, 4), dtype=np.float32)
    rays = np.zeros((4, 8), dtype=np.float32)
    f = np.zeros(4, dtype=np.float32)
    u = np.zeros(4, dtype=np.uint32)
    b = np.zeros(4, dtype=np.uint8)
    assert L.crt_closest_points(None, 4, pts.ctypes.data, f.ctypes.data, None, None, None, None, None) == 1
    assert L.crt_closest_points_device(None, 4, pts.ctypes.data, f.ctypes.data, None, None, None, None, None) == 1
    assert L.crt_count_hits(None, 4, rays.ctypes.data, u.ctypes.data, None) == 1
    assert L.crt_count_hits_device(None, 4, rays.ctypes.data, u.ctypes.data, None) == 1
    assert L.crt_occupancy(None, 4, pts.ctypes.data, b.ctypes.data, None) == 1
    assert L.crt_occupancy_device(None, 0, None, None, None) == 1


def test_make_points_shapes_and_broadcasting(pkg):
    xyz = np.arange(12, dtype=np.float32).reshape(4, 3)
    p = pkg.make_points(xyz)
    assert p.shape == (4, 4) and p.dtype == np.float32 and p.flags["C_CONTIGUOUS"]
    assert np.array_equal(p[:, 0:3], xyz) and np.all(np.isinf(p[:, 3])) and np.all(p[:, 3] > 0)
    p = pkg.make_points(xyz, rmax=np.float32([1, 2, 3, 4]))
    assert np.array_equal(p[:, 3], np.float32([1, 2, 3, 4]))
    assert np.all(pkg.make_points(xyz, rmax=0.5)[:, 3] == 0.5)
    assert pkg.make_points((1.0, 2.0, 3.0)).shape == (1, 4)
    with pytest.raises(ValueError):
        pkg.make_points(np.zeros((4, 2)))


def test_occupancy_directions_are_exact_and_generic():
    """the header's direction constants: exact floats, at least 16 degrees from every axis plane and cube diagonal"""
    text = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    diag = np.array([[1, 1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1]]) / math.sqrt(3.0)
    for k in range(3):
        line = [ln for ln in text.splitlines() if ln.startswith("#define CRT_OCCUPANCY_DIR%d " % k)][0]
        vals = line.split("/*")[0].split(None, 2)[2].replace("f", "").split(",")
        d = np.array([float.fromhex(v.strip()) for v in vals])
        assert np.array_equal(d.astype(np.float32).astype(np.float64), d)
        n = d / np.linalg.norm(d)
        assert np.degrees(np.arcsin(np.abs(n))).min() >= 16.0
        assert np.degrees(np.arccos(np.abs(diag @ n))).min() >= 16.0


def _tri_cases(rng):
    """(p, a, b, c) float32 cases: random triangles and points, the vertex / edge / face regions, slivers, degenerates"""
    cases = []
    for _ in range(400):
        a, b, c = rng.normal(size=(3, 3)) * rng.uniform(0.01, 10.0)
        cases.append((rng.normal(size=3) * 5.0, a, b, c))
    a, b, c = np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.0, 1, 0])
    for p in ([-1, -1, 0.5], [2, -0.5, 1], [-0.5, 2, -1], [0.5, -1, 0.3], [-1, 0.5, 2], [1, 1, 0.1], [0.25, 0.25, 3], [0.3, 0.2, -1e-4]):
        cases.append((np.array(p, dtype=np.float64), a, b, c))
    for _ in range(100):  # slivers: aspect 1e4, in a plane and tilted
        a = rng.normal(size=3)
        e = rng.normal(size=3)
        f = rng.normal(size=3) * 1e-4
        cases.append((a + rng.normal(size=3) * rng.choice([1e-3, 1.0]), a, a + e, a + 0.5 * e + f))
    for _ in range(100):  # degenerate: collinear, two equal vertices, all equal
        a, e = rng.normal(size=3), rng.normal(size=3)
        p = a + rng.normal(size=3)
        cases += [(p, a, a + e, a + 0.3 * e), (p, a, a + e, a - 0.7 * e), (p, a, a, a + e), (p, a, a + e, a + e), (p, a, a, a),
                  (p, a + e, a, a)]
    return [tuple(np.float32(x) for x in cs) for cs in cases]


def test_reference_distance_matches_float64(ref):
    rng = np.random.default_rng(5)
    out = np.zeros(6, dtype=np.float32)
    for i, (p, a, b, c) in enumerate(_tri_cases(rng)):
        ab, ac = np.float32(b - a), np.float32(c - a)
        ref.ref_closest_on_tri(p.ctypes.data, a.ctypes.data, ab.ctypes.data, ac.ctypes.data, out.ctypes.data)
        u, v, d2 = (float(x) for x in out[:3])
        assert np.all(np.isfinite(out)), "case %d: NaN or inf" % i
        assert u >= 0.0 and v >= 0.0 and u + v <= 1.0 + 1e-6, "case %d: barycentrics %g %g" % (i, u, v)
        # the triangle the records describe: (a, a + ab, a + ac) exactly
        a64 = a.astype(np.float64)
        want = closest_f64(p, a64, a64 + ab, a64 + ac)
        scale = float(np.abs(p - a).max() + np.abs(ab).max() + np.abs(ac).max())
        got = math.sqrt(d2)
        assert abs(got - want) <= 1e-5 * want + 1e-6 * scale, "case %d: %r vs float64 %r" % (i, got, want)
        q = out[3:].astype(np.float64)
        assert abs(np.linalg.norm(p - q) - want) <= 1e-5 * want + 4e-6 * scale, "case %d: point" % i


def test_reference_occupancy_matches_winding_number(pkg, ref, scenes):
    rng = np.random.default_rng(9)
    meshes = [_icosphere_mesh(scenes, 2, 1.0, (0.0, 0.0, 0.0)), _icosphere_mesh(scenes, 3, 0.5, (2.0, 0.25, -0.5))]
    tris = _tri_records(pkg, meshes)
    pts = rng.uniform(-1.5, 3.0, size=(3000, 3)).astype(np.float32)
    wn = sum(winding_number(m["vertices"], m["triangles"].astype(np.int64), pts) for m in meshes)
    d = np.minimum(np.abs(np.linalg.norm(pts, axis=1) - 1.0),
                   np.abs(np.linalg.norm(pts - np.float32([2.0, 0.25, -0.5]), axis=1) - 0.5))
    away = d > 2e-2  # the facets of the coarse spheres sit up to ~1e-2 inside the unit sphere
    got = ref_occupancy(ref, tris, pkg.make_points(pts))
    assert away.sum() > 2500 and (wn[away] > 0.5).sum() > 100
    np.testing.assert_array_equal(got[away], wn[away] > 0.5)


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def trees(renderer):
    yield
    for k, v in (("gpu_build", 0), ("gpu_builder", 0)):
        renderer.set_option(k, v)
    renderer.set_counting(False)


def _upload(renderer, sc, tree="sah", dynamic=False):
    for k, v in TREES[tree].items():
        renderer.set_option(k, v)
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"), dynamic=dynamic)
    if "camera" in sc:
        renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])


def _exported(renderer):
    return np.ascontiguousarray(renderer.bvh_export()[1])


def _dragon_points(pkg, sc, rng, n):
    """the point kinds of the issue, concatenated: near-surface, uniform, far, on vertices and edges, specials"""
    V = [np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]]
    T = [np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3) for m in sc["meshes"]]
    v0 = np.concatenate([v[t[:, 0]] for v, t in zip(V, T)])
    v1 = np.concatenate([v[t[:, 1]] for v, t in zip(V, T)])
    v2 = np.concatenate([v[t[:, 2]] for v, t in zip(V, T)])
    allv = np.concatenate(V)
    lo, hi = allv.min(axis=0), allv.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    parts = []
    k = rng.integers(0, len(v0), size=n)
    b = rng.dirichlet((1.0, 1.0, 1.0), size=n).astype(np.float32)
    on = v0[k] * b[:, 0:1] + v1[k] * b[:, 1:2] + v2[k] * b[:, 2:3]
    near = on + rng.normal(size=(n, 3)).astype(np.float32) * np.float32(1e-3 * diag)
    parts.append(pkg.make_points(near, rmax=rng.choice([np.inf, 0.01 * diag, 1e-3 * diag], size=n)))
    parts.append(pkg.make_points(lo + rng.random((n, 3)).astype(np.float32) * (hi - lo), rmax=rng.choice([np.inf, 0.02 * diag], size=n)))
    far = rng.normal(size=(n, 3))
    far = (far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(2.0, 50.0, size=(n, 1)) * diag).astype(np.float32)
    parts.append(pkg.make_points(far, rmax=np.inf))
    m = n // 2
    verts = allv[rng.integers(0, len(allv), size=m)]
    k = rng.integers(0, len(v0), size=m)
    edges = np.where(rng.random((m, 1)) < 0.5, (v0[k] + v1[k]) * np.float32(0.5), (v1[k] + v2[k]) * np.float32(0.5))
    parts.append(pkg.make_points(np.concatenate([verts, edges]), rmax=rng.choice([np.inf, 1e-6, 0.0], size=2 * m)))
    sp = pkg.make_points(lo + rng.random((64, 3)).astype(np.float32) * (hi - lo), rmax=1.0)
    sp[0:8, 0] = np.nan
    sp[8:16, 3] = np.nan
    sp[16:24, 3] = -1.0
    sp[24:32, 3] = -0.0
    sp[32:40, 3] = 0.0
    sp[40:48, 3] = np.float32(3e38)
    parts.append(sp)
    return np.ascontiguousarray(np.concatenate(parts))


def _assert_closest_equal(got, want, what):
    for k in ("inst", "prim"):
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, "%s: %s differs at %d records, first %d: %r vs %r" % (what, k, len(bad), bad[0], got[k][bad[0]], want[k][bad[0]])
    for k in ("dist", "point", "uv"):
        g, w = _bits(got[k]).reshape(len(got["dist"]), -1), _bits(want[k]).reshape(len(want["dist"]), -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert len(bad) == 0, "%s: %s differs at %d records, first %d" % (what, k, len(bad), bad[0])


def _generic_rays(pkg, sc, rng, n):
    allv = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    lo, hi = allv.min(axis=0), allv.max(axis=0)
    o = lo - 0.1 * (hi - lo) + rng.random((n, 3)).astype(np.float32) * 1.2 * (hi - lo)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    rays = pkg.make_rays(o, d, tmin=rng.choice([0.0, 1e-3, -5.0], size=n), tmax=rng.choice([np.inf, 3.0, 1e4], size=n))
    rays[:4, 0] = np.nan
    rays[4:8, 3] = rays[4:8, 7]  # empty interval
    return rays


@pytest.mark.gpu
def test_dragon_closest_points_equal_the_reference(pkg, ref, dragon, renderer, trees):
    rng = np.random.default_rng(11)
    _upload(renderer, dragon)
    pts = _dragon_points(pkg, dragon, rng, 20000)
    tris = _exported(renderer)
    want = ref_closest(ref, tris, pts)
    got = renderer.closest_points(pts)
    _assert_closest_equal(got, want, "dragon")
    hit = got["inst"] != MISS
    assert hit.sum() > len(pts) // 2 and (~hit).sum() > 1000
    assert not np.isnan(got["dist"][hit]).any()
    assert got["stats"]["rays_primary"] == len(pts) and got["stats"]["kernel_ms"] > 0.0
    # misses: dist = rmax, point = the query point, uv = 0
    np.testing.assert_array_equal(_bits(got["dist"][~hit]), _bits(pts[~hit, 3]))
    np.testing.assert_array_equal(_bits(got["point"][~hit]), _bits(pts[~hit, 0:3]))
    assert np.all(got["uv"][~hit] == 0.0)
    # only some outputs; the order of the records does not matter
    perm = rng.permutation(len(pts))
    part = renderer.closest_points(pts[perm], want=("dist", "prim"))
    assert set(part) == {"dist", "prim", "stats"}
    np.testing.assert_array_equal(_bits(part["dist"]), _bits(got["dist"][perm]))
    np.testing.assert_array_equal(part["prim"], got["prim"][perm])


@pytest.mark.gpu
def test_tie_rule_goes_to_the_lower_global_id(pkg, ref, scenes, renderer, trees):
    """a mesh, its exact copy and its mirror image: every point is equidistant to several triangles"""
    m = _icosphere_mesh(scenes, 2, 1.0, (0.0, 0.0, 2.0))
    mirror = dict(m, vertices=m["vertices"] * np.float32([1, 1, -1]))
    sc = {"meshes": [mirror, m, dict(m)], "lights": [], "materials": [{"albedo": (1, 1, 1), "type": 1}]}
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(5000, 3)).astype(np.float32) * np.float32([1.5, 1.5, 0.0])
    pts = pkg.make_points(np.concatenate([pts, m["vertices"]]))
    for tree in TREES:
        _upload(renderer, sc, tree)
        got = renderer.closest_points(pts)
        _assert_closest_equal(got, ref_closest(ref, _exported(renderer), pts), tree)
        assert np.all(got["inst"][:5000] == 0)  # the mirror came first; z = 0 is equidistant from both spheres
        assert np.all(got["inst"][5000:] == 1) and np.all(got["dist"][5000:] == 0.0)  # the sphere before its copy


@pytest.mark.gpu
def test_results_do_not_depend_on_the_tree(pkg, ref, dragon, renderer, trees):
    rng = np.random.default_rng(12)
    pts = _dragon_points(pkg, dragon, rng, 6000)
    rays = _generic_rays(pkg, dragon, rng, 6000)
    res = {}
    for tree in TREES:
        _upload(renderer, dragon, tree)
        res[tree] = (renderer.closest_points(pts), renderer.count_hits(rays), renderer.occupancy(pts[:3 * 6000]))
    want = ref_closest(ref, _exported(renderer), pts)
    for tree, (cp, cnt, occ) in res.items():
        _assert_closest_equal(cp, want, tree)
        np.testing.assert_array_equal(cnt, res["sah"][1], err_msg=tree)
        np.testing.assert_array_equal(occ, res["sah"][2], err_msg=tree)


@pytest.mark.gpu
def test_refit_and_rebuild_equal_the_reference(pkg, ref, dragon, renderer, trees):
    rng = np.random.default_rng(13)
    _upload(renderer, dragon, dynamic=True)
    c, s = math.cos(0.7), math.sin(0.7)
    m = np.float32([c, 0, s, 1.25, 0, 1, 0, -0.5, -s, 0, c, 3.0]).reshape(3, 4)
    renderer.set_mesh_transform(len(dragon["meshes"]) - 1, m)
    renderer.refit()
    moved = [{"vertices": renderer.mesh_vertices(i)[0], "triangles": mm["triangles"]} for i, mm in enumerate(dragon["meshes"])]
    pts = _dragon_points(pkg, {"meshes": moved}, rng, 5000)
    rays = _generic_rays(pkg, {"meshes": moved}, rng, 5000)
    for what in ("refit", "rebuild"):
        if what == "rebuild":
            renderer.rebuild()
        tris = _exported(renderer)
        _assert_closest_equal(renderer.closest_points(pts), ref_closest(ref, tris, pts), what)
        np.testing.assert_array_equal(renderer.count_hits(rays), ref_count(ref, tris, rays), err_msg=what)
        off = pts[:3 * 5000]  # (occupancy is undefined on a surface: the on-vertex / on-edge points are left out)
        np.testing.assert_array_equal(renderer.occupancy(off), ref_occupancy(ref, tris, off), err_msg=what)


def _box_mesh(c, r, n=8):
    """closed axis-aligned box of half size r, every face an n x n grid of quads (two triangles each)"""
    g = np.arange(n + 1) * (2.0 / n) - 1.0
    a, b = np.meshgrid(g, g, indexing="ij")
    verts, tris = [], []
    for axis in range(3):
        for side in (-1.0, 1.0):
            p = np.zeros((n + 1, n + 1, 3))
            p[..., axis] = side
            p[..., (axis + 1) % 3] = a
            p[..., (axis + 2) % 3] = b
            base = sum(len(x) for x in verts)
            verts.append(p.reshape(-1, 3))
            i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
            q = (base + i * (n + 1) + j).reshape(-1)
            if side > 0:
                tris += [np.stack([q, q + n + 1, q + 1], 1), np.stack([q + n + 2, q + 1, q + n + 1], 1)]
            else:
                tris += [np.stack([q, q + 1, q + n + 1], 1), np.stack([q + n + 2, q + n + 1, q + 1], 1)]
    v = (np.float32(r * np.concatenate(verts)) + np.float32(c)).astype(np.float32)
    return {"vertices": v, "triangles": np.concatenate(tris).astype(np.uint32), "material_index": 0, "normals": None}


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0.0, 1024.0, 8192.0, 131072.0])
def test_far_from_origin_closed_meshes(pkg, ref, scenes, renderer, trees, off):
    """closed meshes (an icosphere, a box of small axis-aligned triangles) at offsets up to 2^17 on all three axes: the pruning
    margin keeps the search exact, occupancy equals the reference and the winding number, signed distances agree"""
    c = off * np.array([1.0, 0.75, -0.5])
    r = 0.0625 if off >= 8192.0 else 1.0
    sphere, box = _icosphere_mesh(scenes, 4, r, c), _box_mesh(c + 3.0 * r, r)
    sc = {"meshes": [sphere, box], "lights": [], "materials": [{"albedo": (1, 1, 1), "type": 1}]}
    rng = np.random.default_rng(int(off) + 1)
    n = 4000
    pts = (np.float32(c) + np.float32(r) * rng.uniform(-1.5, 4.5, size=(n, 3)).astype(np.float32)).astype(np.float32)
    V = sphere["vertices"]
    near = V[rng.integers(0, len(V), size=n)] + np.float32(r) * rng.normal(size=(n, 3)).astype(np.float32) * np.float32(0.05)
    xyz = np.concatenate([pts, near]).astype(np.float32)
    P = pkg.make_points(xyz, rmax=np.where(rng.random(2 * n) < 0.5, np.inf, 0.3 * r))
    for tree in ("sah", "lbvh"):
        _upload(renderer, sc, tree)
        tris = _exported(renderer)
        got = renderer.closest_points(P)
        _assert_closest_equal(got, ref_closest(ref, tris, P), "%s %g" % (tree, off))
        occ = renderer.occupancy(P)
        offs = got["dist"] != 0.0  # occupancy is undefined on a surface (at 2^17 the near points snap onto vertices)
        np.testing.assert_array_equal(occ[offs], ref_occupancy(ref, tris, P)[offs], err_msg="%s %g" % (tree, off))
    wn = sum(winding_number(m["vertices"], m["triangles"].astype(np.int64), xyz) for m in sc["meshes"])
    sd = renderer.signed_distance(xyz)
    # away from the surface, where the winding number of the (float32, possibly folded) meshes is a clean 0 or 1
    away = (np.abs(sd) > 1e-3 * r) & (np.abs(wn - np.round(wn)) < 1e-6) & ((np.round(wn) == 0) | (np.round(wn) == 1))
    assert away.sum() > 0.4 * len(xyz) and (wn[away] > 0.5).sum() > 100
    np.testing.assert_array_equal(occ[away], (wn > 0.5)[away])
    np.testing.assert_array_equal(sd[away] < 0, occ[away])


@pytest.mark.gpu
def test_hit_counts_and_occupancy_on_the_dragon(pkg, ref, dragon, renderer, trees):
    rng = np.random.default_rng(14)
    _upload(renderer, dragon)
    tris = _exported(renderer)
    rays = _generic_rays(pkg, dragon, rng, 20000)
    cnt = renderer.count_hits(rays)
    np.testing.assert_array_equal(cnt, ref_count(ref, tris, rays))
    assert (cnt > 1).sum() > 100 and np.all(cnt[:8] == 0)
    # hit counts agree with the closest hit: a ray that crosses something hits something
    hit = renderer.trace_rays(rays, want=("inst",))["inst"] != MISS
    np.testing.assert_array_equal(cnt > 0, hit)
    pts = _dragon_points(pkg, dragon, rng, 5000)[:3 * 5000]  # near-surface, uniform and far points: none on a surface
    occ = renderer.occupancy(pts)
    np.testing.assert_array_equal(occ, ref_occupancy(ref, tris, pts))
    sd = renderer.signed_distance(pts)
    cp = renderer.closest_points(pts, want=("dist",))["dist"]
    np.testing.assert_array_equal(_bits(np.abs(sd)), _bits(np.abs(cp)))
    np.testing.assert_array_equal(sd < 0, occ & (cp > 0))


@pytest.mark.gpu
def test_edge_cases_device_forms_and_streams(pkg, ref, dragon, renderer, trees):
    import torch
    L = pkg.lib()
    rng = np.random.default_rng(15)
    _upload(renderer, dragon)
    pts = _dragon_points(pkg, dragon, rng, 3000)
    rays = _generic_rays(pkg, dragon, rng, 3000)
    host = renderer.closest_points(pts)
    cnt, occ = renderer.count_hits(rays), renderer.occupancy(pts)
    n = len(pts)
    d_pts = torch.from_numpy(np.concatenate([pts.reshape(-1), np.zeros(4, np.float32)])).cuda()
    d_rays = torch.from_numpy(np.concatenate([rays.reshape(-1), np.zeros(8, np.float32)])).cuda()
    d_dist = torch.zeros(n + 2, dtype=torch.float32, device="cuda")
    d_point = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    d_uv = torch.zeros((n + 1, 2), dtype=torch.float32, device="cuda")
    d_inst = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    d_prim = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(len(rays) + 1, dtype=torch.int32, device="cuda")
    d_occ = torch.zeros(n, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    # misaligned device buffers, no output at all, n = 0
    h = renderer.h
    assert L.crt_closest_points_device(h, n, d_pts.data_ptr() + 4, d_dist.data_ptr(), None, None, None, None, None) == 1
    assert L.crt_closest_points_device(h, n, d_pts.data_ptr(), d_dist.data_ptr() + 2, None, None, None, None, None) == 1
    assert L.crt_closest_points_device(h, n, d_pts.data_ptr(), None, None, d_uv.data_ptr() + 4, None, None, None) == 1
    assert L.crt_closest_points_device(h, n, d_pts.data_ptr(), None, d_point.data_ptr() + 1, None, None, None, None) == 1
    assert L.crt_closest_points_device(h, n, d_pts.data_ptr(), None, None, None, None, None, None) == 1
    assert L.crt_count_hits_device(h, len(rays), d_rays.data_ptr() + 8, d_cnt.data_ptr(), None) == 1
    assert L.crt_count_hits_device(h, len(rays), d_rays.data_ptr(), d_cnt.data_ptr() + 2, None) == 1
    assert L.crt_occupancy_device(h, n, d_pts.data_ptr() + 4, d_occ.data_ptr(), None) == 1
    assert L.crt_occupancy_device(h, n, d_pts.data_ptr(), None, None) == 1
    for f in (L.crt_closest_points, L.crt_closest_points_device):
        assert f(h, 0, None, None, None, None, None, None, None) == 0
    assert L.crt_count_hits(h, 0, None, None, None) == 0 and L.crt_occupancy_device(h, 0, None, None, None) == 0
    assert renderer.closest_points(np.zeros((0, 4), np.float32))["dist"].shape == (0,)
    # device forms on a non-default stream, through torch tensors
    side = torch.cuda.Stream()
    try:
        renderer.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            renderer.closest_points_device(n, d_pts.data_ptr(), d_dist.data_ptr(), d_point.data_ptr(), d_uv.data_ptr(), d_inst.data_ptr(),
                                           d_prim.data_ptr())
            renderer.count_hits_device(len(rays), d_rays.data_ptr(), d_cnt.data_ptr())
            st = renderer.occupancy_device(n, d_pts.data_ptr(), d_occ.data_ptr(), stats=True)
        side.synchronize()
    finally:
        renderer.reset_stream()
    assert st["rays_primary"] == 3 * n
    np.testing.assert_array_equal(_bits(d_dist[:n].cpu().numpy()), _bits(host["dist"]))
    np.testing.assert_array_equal(_bits(d_point.cpu().numpy()), _bits(host["point"]))
    np.testing.assert_array_equal(_bits(d_uv[:n].cpu().numpy()), _bits(host["uv"]))
    np.testing.assert_array_equal(d_inst[:n].cpu().numpy().view(np.uint32), host["inst"])
    np.testing.assert_array_equal(d_prim.cpu().numpy().view(np.uint32), host["prim"])
    np.testing.assert_array_equal(d_cnt[:len(rays)].cpu().numpy().view(np.uint32), cnt)
    np.testing.assert_array_equal(d_occ.cpu().numpy(), occ)
    # an empty scene: every point misses, nothing is crossed, nothing is inside
    renderer.upload([], [], [])
    try:
        e = renderer.closest_points(pts)
        assert np.all(e["inst"] == MISS) and np.all(e["prim"] == MISS)
        np.testing.assert_array_equal(_bits(e["dist"]), _bits(pts[:, 3]))
        np.testing.assert_array_equal(_bits(e["point"]), _bits(pts[:, 0:3]))
        assert not renderer.count_hits(rays).any() and not renderer.occupancy(pts).any()
    finally:
        _upload(renderer, dragon)
    # no scene
    fresh = pkg.Renderer(0)
    try:
        out = np.zeros(n, np.float32)
        assert L.crt_closest_points(fresh.h, n, pts.ctypes.data, out.ctypes.data, None, None, None, None, None) == 5
    finally:
        fresh.close()


def _device_queries(renderer, pts, rays):
    """the three point queries through the device forms, with stats: (results, {kind: stats})"""
    import torch
    n, m = len(pts), len(rays)
    d_pts, d_rays = torch.from_numpy(pts).cuda(), torch.from_numpy(rays).cuda()
    d = {"dist": torch.empty(n, dtype=torch.float32, device="cuda"), "point": torch.empty((n, 3), dtype=torch.float32, device="cuda"),
         "uv": torch.empty((n, 2), dtype=torch.float32, device="cuda"), "inst": torch.empty(n, dtype=torch.int32, device="cuda"),
         "prim": torch.empty(n, dtype=torch.int32, device="cuda"), "count": torch.empty(m, dtype=torch.int32, device="cuda"),
         "inside": torch.empty(n, dtype=torch.bool, device="cuda")}
    torch.cuda.synchronize()
    st = {"closest": renderer.closest_points_device(n, d_pts.data_ptr(), *[d[k].data_ptr() for k in ("dist", "point", "uv", "inst", "prim")], stats=True),
          "count": renderer.count_hits_device(m, d_rays.data_ptr(), d["count"].data_ptr(), stats=True),
          "occupancy": renderer.occupancy_device(n, d_pts.data_ptr(), d["inside"].data_ptr(), stats=True)}
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in d.items()}
    for k in ("inst", "prim", "count"):
        res[k] = res[k].view(np.uint32)
    return res, st


@pytest.mark.gpu
def test_tuning_options_change_nothing(pkg, ref, dragon, renderer, trees):
    """2^19 + 37 records per kind -- more than 64 per workgroup the device holds at once, so the cursor, the mid-flight refill
    and the tail of the buffer all run -- with a one- and a three-entry LDS stack (nearly every push spills, the two-word
    entries of the closest-point stack included) and other scheduling thresholds: every output and both fetch counters are
    those of the default options.  A seeded sample of the default run is pinned to the reference."""
    rng = np.random.default_rng(18)
    _upload(renderer, dragon)
    n = (1 << 19) + 37
    k = 1 << 17
    pts = np.ascontiguousarray(_dragon_points(pkg, dragon, rng, k)[-n:])  # (every kind of point; 27 near-surface ones left out)
    rays = _generic_rays(pkg, dragon, rng, n)
    assert len(pts) == n and len(rays) == n
    defaults = (("inner_min", -6), ("inner_min_any", -6), ("stack_entries", 0))
    counters = ("nodes_visited", "tris_tested")
    renderer.set_counting(True)
    try:
        base, st = _device_queries(renderer, pts, rays)
        assert all(st[kind][c] > 0 for kind in st for c in counters)
        for name, value in (("stack_entries", 1), ("stack_entries", 3), ("inner_min", 3), ("inner_min_any", 40), ("inner_min_any", -2)):
            renderer.set_option(name, value)
            got, gs = _device_queries(renderer, pts, rays)
            for o, v in defaults:
                renderer.set_option(o, v)
            what = "%s=%d" % (name, value)
            _assert_closest_equal(got, base, what)
            np.testing.assert_array_equal(got["count"], base["count"], err_msg=what + ": count")
            np.testing.assert_array_equal(got["inside"], base["inside"], err_msg=what + ": occupancy")
            for kind in st:
                for c in counters:
                    assert gs[kind][c] == st[kind][c], "%s: %s %s" % (what, kind, c)
    finally:
        for o, v in defaults:
            renderer.set_option(o, v)
        renderer.set_counting(False)
    tris = _exported(renderer)
    pick = np.sort(np.random.default_rng(19).choice(n, 2000, replace=False))
    _assert_closest_equal({q: base[q][pick] for q in ("dist", "point", "uv", "inst", "prim")}, ref_closest(ref, tris, pts[pick]), "sample")
    np.testing.assert_array_equal(base["count"][pick], ref_count(ref, tris, rays[pick]))
    off = pick[pick < 3 * k - 27]  # (occupancy is undefined on a surface: the on-vertex / on-edge points are left out)
    assert len(off) > 1000
    np.testing.assert_array_equal(base["inside"][off], ref_occupancy(ref, tris, pts[off]))
    assert (base["inst"] != MISS).sum() > n // 2 and (base["count"] > 1).sum() > n // 200  # (the shares the smaller dragon tests ask for)


@pytest.mark.gpu
def test_counting_is_not_brute_force(pkg, scenes, renderer, trees):
    """near-surface points on the 1M-triangle height field fetch few triangle records per query (measured on an MI355X:
    8.2 triangle and 14.6 node records per query; the bound leaves about five times that)"""
    sc = scenes.heightfield()
    _upload(renderer, sc)
    rng = np.random.default_rng(16)
    m = sc["meshes"][1]
    V = np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3)
    n = 20000
    near = V[rng.integers(0, len(V), size=n)] + rng.normal(size=(n, 3)).astype(np.float32) * np.float32(0.05)
    renderer.set_counting(True)
    st = renderer.closest_points(pkg.make_points(near), want=("dist",))["stats"]
    renderer.set_counting(False)
    tris, nodes = st["tris_tested"] / n, st["nodes_visited"] / n
    print("heightfield near-surface closest point: %.1f triangles, %.1f nodes per query" % (tris, nodes))
    assert 0 < tris < 40 and 0 < nodes < 80


@pytest.mark.gpu
def test_queries_leave_frames_untouched(pkg, scenes, renderer, trees):
    import torch
    sc = scenes.cornell_box()
    _upload(renderer, sc)
    rng = np.random.default_rng(17)
    pts = _dragon_points(pkg, sc, rng, 3000)
    rays = _generic_rays(pkg, sc, rng, 3000)
    d_pts = torch.from_numpy(pts).cuda()
    d_occ = torch.empty(len(pts), dtype=torch.bool, device="cuda")
    w = h = 128
    renderer.change_shading_mode(100)
    before = renderer.render_frame(w, h)
    for _ in range(3):
        renderer.closest_points(pts)
        renderer.count_hits(rays)
        renderer.occupancy(pts)
    after = renderer.render_frame(w, h)
    for k in ("rgba8", "hit_inst", "hit_prim", "hit_t"):
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    renderer.change_shading_mode(200)
    try:
        renderer.set_path_params(2, 3, 1234)
        renderer.set_accumulation(1 << 24)
        for i in range(3):
            assert renderer.accumulated_samples() == 2 * i
            renderer.closest_points(pts)
            renderer.occupancy_device(len(pts), d_pts.data_ptr(), d_occ.data_ptr())
            renderer.count_hits(rays)
            assert renderer.accumulated_samples() == 2 * i
            renderer.render_frame(w, h)
        torch.cuda.synchronize()
        assert renderer.accumulated_samples() == 6
    finally:
        renderer.set_accumulation(0)
        renderer.set_path_params(4, 3, 1234)
        renderer.change_shading_mode(3)
