"""Winding numbers (crt_winding_numbers* / crt_winding_moments_export, include/crt_hip.h): the inside test for open meshes and
soups.  The GPU results are compared bit for bit (float bits as uint32) with tests/winding_reference.c, a restatement of the
arctangent, the per-triangle term, the brute-force sum, the moment table and the walk in the contract's operation order; the
reference itself is checked against float64 (atan2, and a Van Oosterom-Strackee winding number restated here).

Measured on the CPU (host SAH tree; 257 points per scene no nearer to a triangle than 1 % of the radius; -s prints them):
    ref_atan2 over the grid of test_reference_atan2_matches_float64: largest |error| 2.94e-7 (ATAN_MEASURED)
    largest |w - w_f64|   exact     beta 1    beta 2    beta 4    beta 8
    sphere                1.18e-7   1.56e-1   2.42e-2   3.44e-3   9.8e-5
    reversed              1.23e-7   1.40e-1   2.43e-2   3.44e-3   9.5e-5
    two nested            2.23e-7   1.92e-1   4.17e-2   6.77e-3   1.36e-4
    one octant removed    9.4e-8    1.38e-1   2.00e-2   3.27e-3   8.7e-5


test_far_from_origin and test_tiny_scenes go through tests/winding_checks.py's assert_winding, the hub that also holds winding
numbers on poisoned scenes (tests/test_nonfinite_vertices.py) and on deep trees and a moving depth4 (tests/test_deep_stacks.py);
tests/test_winding_checks.py has the figures measured on those inputs."""
import ctypes as C
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_point_queries as tp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("crt_winding_numbers_device", "crt_winding_numbers", "crt_winding_moments_export")
TREES = tp.TREES
ATAN_BUDGET = 2.0 ** -20      # per-term cap the error budget of the sum rests on
ATAN_MEASURED = 2.95e-7       # largest |ref_atan2 - atan2| over the grid below (tests/winding_reference.c)
ULP_PI = 2.0 ** -22           # one float32 ulp of pi
MATERIALS = [{"albedo": (1, 1, 1), "type": 1}]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the reference (tests/winding_reference.c)

@pytest.fixture(scope="session")
def wref(pkg, tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for tests/winding_reference.c")
    out = str(tmp_path_factory.mktemp("winding_reference") / "libwinding_reference.so")
    base = [cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tests", "winding_reference.c"), "-o", out, "-lm"]
    if subprocess.call(base[:1] + ["-fopenmp"] + base[1:], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)  # (no OpenMP: the pragmas are ignored)
    L = C.CDLL(out)
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    L.ref_atan2.argtypes, L.ref_atan2.restype = [f32, f32], f32
    L.ref_half_angle.argtypes, L.ref_half_angle.restype = [vp, vp, vp, vp], f32
    L.ref_atan2_array.argtypes, L.ref_atan2_array.restype = [u32, vp, vp, vp], None
    L.ref_winding_exact.argtypes, L.ref_winding_exact.restype = [vp, u32, u32, vp, vp], None
    L.ref_moments.argtypes, L.ref_moments.restype = [vp, u32, vp, vp], None
    L.ref_winding_tree.argtypes, L.ref_winding_tree.restype = [vp, u32, vp, vp, f32, u32, vp, vp], None
    return L


def _records(pts):
    pts = np.asarray(pts, dtype=np.float32)
    if pts.shape[-1] == 3:
        pts = np.concatenate([pts.reshape(-1, 3), np.zeros((pts.size // 3, 1), np.float32)], axis=1)
    return np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)


def ref_exact(wref, tris, pts):
    pts = _records(pts)
    tris = np.ascontiguousarray(tris)
    w = np.zeros(len(pts), np.float32)
    wref.ref_winding_exact(tris.ctypes.data, len(tris), len(pts), pts.ctypes.data, w.ctypes.data)
    return w


def ref_moments(wref, nodes4q, tris):
    nodes4q, tris = np.ascontiguousarray(nodes4q), np.ascontiguousarray(tris)
    m = np.zeros((len(nodes4q), 32), np.float32)
    wref.ref_moments(nodes4q.ctypes.data, len(nodes4q), tris.ctypes.data, m.ctypes.data)
    return m


def ref_tree(wref, nodes4q, tris, moments, beta, pts):
    pts = _records(pts)
    nodes4q, tris, moments = np.ascontiguousarray(nodes4q), np.ascontiguousarray(tris), np.ascontiguousarray(moments, dtype=np.float32)
    w = np.zeros(len(pts), np.float32)
    wref.ref_winding_tree(nodes4q.ctypes.data, len(nodes4q), tris.ctypes.data, moments.ctypes.data, float(beta), len(pts), pts.ctypes.data,
                          w.ctypes.data)
    return w


# ---- float64 yardstick: Van Oosterom-Strackee over the float32 records (the triangles exactly as traced)

def winding_f64(tris, pts):
    v0, e1, e2 = (tris[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    ok = np.isfinite(v0).all(axis=1) & np.isfinite(e1).all(axis=1) & np.isfinite(e2).all(axis=1)
    A, B, Cc = v0[ok], (v0 + e1)[ok], (v0 + e2)[ok]
    out = np.zeros(len(pts))
    for i, p in enumerate(np.asarray(pts, dtype=np.float64)[:, 0:3]):
        a, b, c = A - p, B - p, Cc - p
        la, lb, lc = (np.linalg.norm(x, axis=1) for x in (a, b, c))
        det = np.einsum("ij,ij->i", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("ij,ij->i", a, b) * lc + np.einsum("ij,ij->i", b, c) * la + np.einsum("ij,ij->i", c, a) * lb
        out[i] = np.sum(np.arctan2(det, den)) / (2.0 * math.pi)
    return out


# ---- scenes

CENTRE = np.array([0.3, -0.2, 0.1])


def _sphere(scenes, r=1.0, reverse=False, keep=None):
    v, f = scenes._icosphere(2)
    if reverse:
        f = f[:, ::-1]
    if keep is not None:
        f = f[keep(v[f].mean(axis=1))]
    return {"vertices": (np.float32(r * v) + np.float32(CENTRE)).astype(np.float32), "triangles": np.ascontiguousarray(f).astype(np.uint32),
            "material_index": 0, "normals": None}


def _not_first_octant(c):
    return ~((c[:, 0] > 0) & (c[:, 1] > 0) & (c[:, 2] > 0))


def sphere_scene(scenes, kind):
    """the 320-triangle icosphere: as is, reversed (-1 inside), with a second one of half the radius inside (2 / 1 / 0), and with
    the triangles of one octant removed (fractions)"""
    meshes = {"sphere": lambda: [_sphere(scenes)], "reversed": lambda: [_sphere(scenes, reverse=True)],
              "nested": lambda: [_sphere(scenes), _sphere(scenes, r=0.5)],
              "open": lambda: [_sphere(scenes, keep=_not_first_octant)]}[kind]()
    return {"meshes": meshes, "lights": [], "materials": MATERIALS}


def dragon_mesh_open(dragon, seed=21):
    """the Dragon's own mesh (without the ground quad) with a seeded tenth of its triangles removed"""
    m = max(dragon["meshes"], key=lambda mm: len(np.asarray(mm["triangles"]).reshape(-1, 3)))
    t = np.asarray(m["triangles"], dtype=np.uint32).reshape(-1, 3)
    keep = np.random.default_rng(seed).random(len(t)) >= 0.1
    return {"meshes": [{"vertices": np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3), "triangles": np.ascontiguousarray(t[keep]),
                        "material_index": 0, "normals": None}], "lights": [], "materials": MATERIALS}


def shell_points(rng, n, holes):
    """n points around CENTRE at radii in [0, 2.5] outside the bands `holes`: no nearer to the spheres' facets than 1 % of the radius"""
    pts = []
    while len(pts) < n:
        d = rng.normal(size=3)
        r = rng.uniform(0.0, 2.5)
        if not any(lo < r < hi for lo, hi in holes):
            pts.append(CENTRE + d / np.linalg.norm(d) * r)
    return np.float32(pts)


BANDS = {"sphere": [(0.95, 1.03)], "reversed": [(0.95, 1.03)], "open": [(0.95, 1.03)], "nested": [(0.95, 1.03), (0.47, 0.52)]}
FAR_OFFSETS = (0.0, 1024.0, 8192.0, 131072.0)
FAR_SCENES = ("sphere", "open")


def far_case(scenes, kind, off):
    """a sphere scene and 257 shell points, both moved by (off, -off, 0.5 off) in float32 (a translation rounds the vertices,
    p~ and p~ - q otherwise than a power-of-two scale does), and every point's float64 distance from the moved centre"""
    shift = np.float32([off, -off, 0.5 * off])
    sc = sphere_scene(scenes, kind)
    for m in sc["meshes"]:
        m["vertices"] = (m["vertices"] + shift).astype(np.float32)
    pts = _records((shell_points(np.random.default_rng(200 + int(off)), 257, BANDS[kind]) + shift).astype(np.float32))
    radius = np.linalg.norm(pts[:, 0:3].astype(np.float64) - (np.float32(CENTRE).astype(np.float64) + shift.astype(np.float64)), axis=1)
    return sc, pts, radius


def _min_distance(tris, p, nearest=12):
    """float64 distance from p to the triangle set, over the `nearest` triangles by centroid (test_point_queries.closest_f64)"""
    v0, e1, e2 = (tris[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    cen = v0 + (e1 + e2) / 3.0
    idx = np.argsort(np.linalg.norm(cen - p, axis=1))[:nearest]
    return min(tp.closest_f64(p, v0[i], v0[i] + e1[i], v0[i] + e2[i]) for i in idx)


def host_tree(pkg, meshes):
    """the host SAH tree as an upload builds it, without a GPU: quantised wide nodes and leaf-ordered triangle records"""
    _, tris, _, _ = pkg.build_bvh_host(meshes)
    nodes4, _ = pkg.build_bvh4_host(meshes)
    return pkg.quantize4(nodes4), tris


def query_points(pkg, sc, rng, n=257):
    """the point kinds of the walk test: inside / outside the box, 1e-3 of the size from the surface, 100 x the size away, a NaN
    record, a point equal to a vertex"""
    V = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    lo, hi = V.min(axis=0), V.max(axis=0)
    size = float(np.linalg.norm(hi - lo))
    k = n - 2
    box = lo - 0.1 * (hi - lo) + rng.random((k // 2, 3)) * 1.2 * (hi - lo)
    near = V[rng.integers(0, len(V), size=k // 4)] + rng.normal(size=(k // 4, 3)) * 1e-3 * size
    far = rng.normal(size=(k - k // 2 - k // 4, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * 100.0 * size + (lo + hi) / 2
    pts = pkg.make_points(np.float32(np.concatenate([box, near, far, V[7:8], V[3:4]])))
    pts[-1, 1] = np.nan
    assert len(pts) == n
    return np.ascontiguousarray(rng.permutation(pts))


# ---- CPU: the interface exists, the reference is right

def test_binding_and_library_expose_winding_numbers(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
    for name in ("winding_numbers", "winding_numbers_device", "winding_moments", "inside_winding", "signed_distance"):
        assert callable(getattr(pkg.Renderer, name, None)), name
    assert L.crt_abi_version() == 1
    pts, w = np.zeros((4, 4), np.float32), np.zeros(4, np.float32)
    assert L.crt_winding_numbers(None, 4, pts.ctypes.data, 2.0, w.ctypes.data, None) == 1  # CRT_EINVAL
    assert L.crt_winding_numbers_device(None, 0, None, 2.0, None, None) == 1
    assert L.crt_winding_moments_export(None, None) == 1


def test_header_constants_are_exact_floats():
    text = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    for k in range(7):
        line = [ln for ln in text.splitlines() if ln.startswith("#define CRT_ATAN_C%d " % k)][0]
        v = float.fromhex(line.split()[2].rstrip("f"))
        assert float(np.float32(v)) == v, line


def _atan_grid():
    mant = 1.0 + np.arange(32) / 32.0 + 1.0 / 257.0
    mag = np.concatenate([np.ldexp(mant, e) for e in range(-60, 61, 4)] + [[2.0 ** -60, 2.0 ** 60, 0.0]])
    vals = np.float32(np.concatenate([mag, -mag]))
    y, x = np.meshgrid(vals, vals, indexing="ij")
    return np.ascontiguousarray(y.reshape(-1)), np.ascontiguousarray(x.reshape(-1))


def test_reference_atan2_matches_float64(wref):
    y, x = _atan_grid()
    out = np.zeros(len(y), np.float32)
    wref.ref_atan2_array(len(y), y.ctypes.data, x.ctypes.data, out.ctypes.data)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    # the contract's choices where atan2 has a cut or a sign of zero: y = +-0 with x < 0 is +pi, a zero result is +0
    zero_y = y == 0.0
    want[zero_y & (x < 0)] = math.pi
    want[zero_y & (x >= 0)] = 0.0
    err = np.abs(out.astype(np.float64) - want)
    print("ref_atan2: max abs error %.3e over %d pairs" % (err.max(), len(y)))
    assert err.max() <= ATAN_MEASURED + ULP_PI
    assert ATAN_MEASURED + ULP_PI <= ATAN_BUDGET
    assert np.all(_bits(out[zero_y & (x >= 0)]) == 0) and np.all(_bits(out[zero_y & (x < 0)]) == _bits(np.float32(math.pi)))
    # both axes, the defined specials
    f = wref.ref_atan2
    inf, nan = float("inf"), float("nan")
    assert f(1.0, 0.0) == f(1.0, -0.0) == np.float32(math.pi / 2) and f(-1.0, 0.0) == -np.float32(math.pi / 2)
    for yy, xx in ((0.0, 0.0), (-0.0, -0.0), (nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, inf), (1.0, -inf), (inf, inf)):
        assert f(yy, xx) == 0.0, (yy, xx)


def test_reference_half_angle_special_cases(wref):
    def h(q, a, b, c):
        q, a, b, c = (np.float32(v) for v in (q, a, b, c))
        e1, e2 = np.float32(b - a), np.float32(c - a)
        return wref.ref_half_angle(q.ctypes.data, a.ctypes.data, e1.ctypes.data, e2.ctypes.data)
    a, b, c = [0, 0, 0], [1, 0, 0], [0, 1, 0]
    assert h([2, 2, 0], a, b, c) == 0.0                          # in the plane, outside the triangle
    up, down = h([0.25, 0.25, 0], a, b, c), h([0.25, 0.25, -0.0], a, b, c)
    assert abs(up) == np.float32(math.pi) and up == down         # in the plane, inside: the same bits from both sides
    for v in (a, b, c):
        assert h(v, a, b, c) == 0.0                              # at a vertex
    assert h([0.2, 0.2, 1], a, b, [np.nan, 1, 0]) == 0.0 and h([0.2, 0.2, 1], a, [np.inf, 0, 0], c) == 0.0  # inert triangles
    assert h([0.2, 0.2, -1], a, b, c) > 0 > h([0.2, 0.2, 1], a, b, c)  # the normal (0, 0, 1) points away from the first point


@pytest.fixture(scope="module")
def cpu_cases(pkg, scenes, wref):
    """per sphere scene: upload-order records, the host tree, 257 points clear of the surface and their float64 winding numbers"""
    out = {}
    for i, kind in enumerate(("sphere", "reversed", "nested", "open")):
        sc = sphere_scene(scenes, kind)
        recs = tp._tri_records(pkg, sc["meshes"])
        pts = _records(shell_points(np.random.default_rng(100 + i), 257, BANDS[kind]))
        nodes4q, tris = host_tree(pkg, sc["meshes"])
        out[kind] = {"scene": sc, "records": recs, "points": pts, "nodes4q": nodes4q, "tris": tris,
                     "moments": ref_moments(wref, nodes4q, tris), "f64": winding_f64(recs, pts)}
    return out


def test_points_keep_clear_of_the_surface(cpu_cases):
    for kind, cs in cpu_cases.items():
        d = min(_min_distance(cs["records"], p.astype(np.float64)) for p in cs["points"][:, 0:3])
        assert d >= 0.01, "%s: a point %.4f from a triangle" % (kind, d)


def test_reference_exact_matches_float64(wref, cpu_cases):
    for kind, cs in cpu_cases.items():
        n_tris = len(cs["records"])
        w = ref_exact(wref, cs["records"], cs["points"])
        err = np.abs(w.astype(np.float64) - cs["f64"]).max()
        print("ref_winding_exact %-8s: max |w - f64| = %.3e (bound %.3e)" % (kind, err, n_tris * ATAN_BUDGET / (2 * math.pi)))
        assert err <= n_tris * ATAN_BUDGET / (2 * math.pi)
        r = np.linalg.norm(cs["points"][:, 0:3].astype(np.float64) - CENTRE, axis=1)
        inside, outside = cs["f64"][r < 0.9], cs["f64"][r > 1.1]
        if kind == "open":
            assert ((cs["f64"] > 0.05) & (cs["f64"] < 0.95)).sum() > 20  # fractions
        else:
            want = {"sphere": 1.0, "reversed": -1.0, "nested": 1.0}[kind]
            assert np.allclose(inside[r[r < 0.9] > 0.55], want, atol=1e-7) and np.allclose(outside, 0.0, atol=1e-7)
            if kind == "nested":
                assert np.allclose(cs["f64"][r < 0.45], 2.0, atol=1e-7) and (r < 0.45).sum() > 0
        # the order of the records does not matter
        perm = np.random.default_rng(1).permutation(n_tris)
        np.testing.assert_array_equal(_bits(ref_exact(wref, cs["records"][perm], cs["points"])), _bits(w))


def test_reference_tree_matches_float64(wref, cpu_cases):
    for kind, cs in cpu_cases.items():
        floor = len(cs["records"]) * ATAN_BUDGET / (2 * math.pi)
        exact = ref_exact(wref, cs["records"], cs["points"])
        errs = []
        for beta in (1.0, 2.0, 4.0, 8.0):
            w = ref_tree(wref, cs["nodes4q"], cs["tris"], cs["moments"], beta, cs["points"])
            errs.append(np.abs(w.astype(np.float64) - cs["f64"]).max())
        print("ref_winding_tree %-8s: max |w - f64| at beta 1, 2, 4, 8 = %s" % (kind, " ".join("%.3e" % e for e in errs)))
        for lo, hi in zip(errs[1:], errs[:-1]):
            assert lo <= max(hi, floor), "%s: the error grows with beta: %r" % (kind, errs)
        for beta in (float("inf"), 0.0, -1.0, float("nan")):
            w = ref_tree(wref, cs["nodes4q"], cs["tris"], cs["moments"], beta, cs["points"])
            np.testing.assert_array_equal(_bits(w), _bits(exact), err_msg="%s beta %r" % (kind, beta))


@pytest.fixture(scope="module")
def feature_cases(pkg, scenes, dragon, wref):
    """the open sphere and the Dragon with a tenth of its triangles removed: test points, their float64 winding numbers and the
    margin around 0.5 inside which a point is left out -- twice the beta = 2 error measured over the host tree"""
    out = {}
    for name, sc, seed in (("open sphere", sphere_scene(scenes, "open"), 31), ("open dragon", dragon_mesh_open(dragon), 32)):
        rng = np.random.default_rng(seed)
        V = np.asarray(sc["meshes"][0]["vertices"], dtype=np.float64)
        lo, hi = V.min(axis=0), V.max(axis=0)
        recs = tp._tri_records(pkg, sc["meshes"])
        # 129 points in the box, 128 off the surface along a triangle's normal, either way, by 0.3 .. 3 % of the size
        size = float(np.linalg.norm(hi - lo))
        k = rng.integers(0, len(recs), size=128)
        v0, e1, e2 = (recs[key][k].astype(np.float64) for key in ("v0", "e1", "e2"))
        nrm = np.cross(e1, e2)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        off = rng.uniform(0.003, 0.03, size=(128, 1)) * size * rng.choice([-1.0, 1.0], size=(128, 1))
        pts = _records(np.float32(np.concatenate([lo - 0.05 * (hi - lo) + rng.random((129, 3)) * 1.1 * (hi - lo),
                                                  v0 + (e1 + e2) / 3.0 + off * nrm])))
        nodes4q, tris = host_tree(pkg, sc["meshes"])
        f64 = winding_f64(recs, pts)
        w2 = ref_tree(wref, nodes4q, tris, ref_moments(wref, nodes4q, tris), 2.0, pts)
        margin = 2.0 * float(np.abs(w2.astype(np.float64) - f64).max())
        out[name] = {"scene": sc, "points": pts, "f64": f64, "margin": margin, "judged": np.abs(f64 - 0.5) > margin}
    return out


def test_feature_points_are_mostly_clear_of_one_half(feature_cases):
    for name, cs in feature_cases.items():
        left_out = 1.0 - cs["judged"].mean()
        print("%s: margin %.3e, %.1f %% of the points left out, %d inside" % (name, cs["margin"], 100 * left_out, (cs["f64"] > 0.5).sum()))
        assert left_out <= 0.05, name
        assert (cs["f64"][cs["judged"]] > 0.5).sum() >= 10 and (cs["f64"][cs["judged"]] < 0.5).sum() >= 10, name


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def trees(renderer):
    yield
    for k, v in (("gpu_build", 0), ("gpu_builder", 0), ("stack_entries", 0), ("inner_min", -6), ("inner_min_any", -6)):
        renderer.set_option(k, v)
    renderer.set_counting(False)


def _upload(renderer, sc, tree="sah", dynamic=False):
    tp._upload(renderer, sc, tree, dynamic)


def _exported(renderer):
    return renderer.bvh_export4q(), np.ascontiguousarray(renderer.bvh_export()[1])


def _walk_scene(scenes, dragon, name):
    return dragon if name == "dragon" else sphere_scene(scenes, name)


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("name", ["sphere", "open", "dragon"])
def test_walk_equals_the_reference(pkg, wref, scenes, dragon, renderer, trees, name, tree):
    sc = _walk_scene(scenes, dragon, name)
    pts = query_points(pkg, sc, np.random.default_rng(41))
    _upload(renderer, sc, tree)
    nodes4q, tris = _exported(renderer)
    moments = renderer.winding_moments()
    for beta in (0.0, 1.0, 2.0, 8.0):
        got = renderer.winding_numbers(pts, beta)
        want = ref_tree(wref, nodes4q, tris, moments, beta, pts)
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert len(bad) == 0, "%s %s beta %g: %d differ, first %d: %r vs %r" % (name, tree, beta, len(bad), bad[0], got[bad[0]], want[bad[0]])
    nan = np.isnan(pts[:, 0:3]).any(axis=1)
    assert nan.sum() == 1 and _bits(got[nan])[0] == 0 and np.isfinite(got).all()


def _assert_moments(wref, renderer, what):
    nodes4q, tris = _exported(renderer)
    got, want = renderer.winding_moments(), ref_moments(wref, nodes4q, tris)
    assert got.shape == want.shape and len(got) > 0
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    assert len(bad) == 0, "%s: the moments of %d nodes differ, first node %d: %r vs %r" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
def test_moments_equal_the_reference_and_follow_the_scene(pkg, wref, dragon, renderer, trees, tree):
    _upload(renderer, dragon, tree, dynamic=True)
    first = _assert_moments(wref, renderer, tree)
    assert np.all(first[:, 19::4] == 0.0) and np.all(first[:, 3:16:4] >= 0.0)
    mesh = len(dragon["meshes"]) - 1
    V = np.asarray(dragon["meshes"][mesh]["vertices"], dtype=np.float32).reshape(-1, 3)
    renderer.update_vertices(mesh, (V * np.float32([1.0, 1.25, 1.0]) + np.float32([0.0, 0.5, 0.0])).astype(np.float32))
    moved = _assert_moments(wref, renderer, tree + " after update_vertices")  # no explicit refit: the export applies it
    assert not np.array_equal(_bits(moved), _bits(first))
    c, s = math.cos(0.4), math.sin(0.4)
    renderer.set_mesh_transform(mesh, np.float32([c, 0, s, 1.0, 0, 1, 0, -0.25, -s, 0, c, 2.0]).reshape(3, 4))
    pts = query_points(pkg, dragon, np.random.default_rng(42))
    w = renderer.winding_numbers(pts, 2.0)                        # the query applies the refit and rebuilds the table
    turned = _assert_moments(wref, renderer, tree + " after set_mesh_transform")
    assert not np.array_equal(_bits(turned), _bits(moved))
    nodes4q, tris = _exported(renderer)
    np.testing.assert_array_equal(_bits(w), _bits(ref_tree(wref, nodes4q, tris, turned, 2.0, pts)))
    for builder in (0, 1):
        renderer.set_option("gpu_builder", builder)
        renderer.rebuild()
        _assert_moments(wref, renderer, "%s after rebuild with builder %d" % (tree, builder))


@pytest.mark.gpu
def test_exact_mode_is_the_same_over_every_tree(pkg, wref, scenes, dragon, renderer, trees):
    for name in ("open", "dragon"):
        sc = _walk_scene(scenes, dragon, name)
        pts = query_points(pkg, sc, np.random.default_rng(43))
        want = ref_exact(wref, tp._tri_records(pkg, sc["meshes"]), pts)  # the records in upload order
        for tree in TREES:
            _upload(renderer, sc, tree, dynamic=True)
            for beta in (0.0, -3.0, float("nan"), float("inf")):
                np.testing.assert_array_equal(_bits(renderer.winding_numbers(pts, beta)), _bits(want), err_msg="%s %s beta %r" % (name, tree, beta))
            renderer.set_mesh_transform(0, None)
            renderer.refit()
            np.testing.assert_array_equal(_bits(renderer.winding_numbers(pts, 0.0)), _bits(want), err_msg="%s %s refit" % (name, tree))
            for builder in (0, 1):
                renderer.set_option("gpu_builder", builder)
                renderer.rebuild()
                np.testing.assert_array_equal(_bits(renderer.winding_numbers(pts, 0.0)), _bits(want), err_msg="%s %s rebuild %d" % (name, tree, builder))


@pytest.mark.gpu
@pytest.mark.parametrize("off", FAR_OFFSETS)
def test_far_from_origin(pkg, wref, scenes, renderer, trees, off):
    """the closed and the open sphere at (off, -off, 0.5 off) over all three trees: every check of winding_checks.assert_winding,
    and at beta 2 the inside test of the closed sphere on every point outside the band [0.9, 1.1] around its surface"""
    import winding_checks as wc
    for kind in FAR_SCENES:
        sc, pts, radius = far_case(scenes, kind, off)
        records = tp._tri_records(pkg, sc["meshes"])
        judged = (radius < 0.9) | (radius > 1.1)
        # the band [0.9, 1.1] of the radii drawn from [0, 2.5] less (0.95, 1.03) is 4.8 % of them
        assert 1.0 - judged.mean() <= 0.2, "%s at %g: %.1f %% of the points left out" % (kind, off, 100.0 * (1.0 - judged.mean()))
        assert (radius[judged] < 0.9).sum() >= 20 and (radius[judged] > 1.1).sum() >= 20
        exact = None
        for tree in TREES:
            _upload(renderer, sc, tree)
            out = wc.assert_winding(pkg, wref, renderer, sc, records, pts, "%s at %g, %s" % (kind, off, tree))
            exact = out["w"][0.0] if exact is None else exact
            np.testing.assert_array_equal(out["w"][0.0], exact, err_msg="%s at %g: exact mode over %s" % (kind, off, tree))
            if kind == "sphere":
                inside = out["w"][2.0].view(np.float32) > 0.5
                bad = np.flatnonzero((inside != (radius < 0.9)) & judged)
                assert len(bad) == 0, "%s at %g, %s: %d points on the wrong side at beta 2, first %d at radius %r" % (kind, off, tree, len(bad), bad[0], radius[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_tiny_scenes(pkg, wref, renderer, trees, n):
    """1 to 5 triangles over all three trees: the one-leaf root and a two-node tree"""
    import test_nonfinite_vertices as nf
    import winding_checks as wc
    sc = nf._tiny(n)
    pts = wc.points_for(sc, seed=n)
    records = tp._tri_records(pkg, sc["meshes"])
    for tree in TREES:
        _upload(renderer, sc, tree)
        wc.assert_winding(pkg, wref, renderer, sc, records, pts, "tiny%d %s" % (n, tree))


@pytest.mark.gpu
def test_order_and_size_of_the_buffer(pkg, wref, dragon, renderer, trees):
    rng = np.random.default_rng(44)
    _upload(renderer, dragon)
    pts = np.ascontiguousarray(np.concatenate([query_points(pkg, dragon, np.random.default_rng(50 + i)) for i in range(16)])[:4097])
    nodes4q, tris = _exported(renderer)
    moments = renderer.winding_moments()
    base = renderer.winding_numbers(pts, 2.0)
    np.testing.assert_array_equal(_bits(base), _bits(ref_tree(wref, nodes4q, tris, moments, 2.0, pts)))
    perm = rng.permutation(len(pts))
    np.testing.assert_array_equal(_bits(renderer.winding_numbers(pts[perm], 2.0)), _bits(base[perm]))
    for n in (1, 63, 64, 65):
        np.testing.assert_array_equal(_bits(renderer.winding_numbers(pts[:n], 2.0)), _bits(base[:n]), err_msg=str(n))
    L = pkg.lib()
    assert L.crt_winding_numbers(renderer.h, 0, None, 2.0, None, None) == 0
    assert L.crt_winding_numbers_device(renderer.h, 0, None, 2.0, None, None) == 0
    assert renderer.winding_numbers(np.zeros((0, 4), np.float32)).shape == (0,)


@pytest.mark.gpu
def test_stacks_and_tuning_change_nothing(pkg, dragon, renderer, trees):
    import torch
    _upload(renderer, dragon)
    pts = np.ascontiguousarray(np.concatenate([query_points(pkg, dragon, np.random.default_rng(60 + i)) for i in range(16)])[:4097])
    d_pts = torch.from_numpy(pts).cuda()
    d_w = torch.zeros(len(pts), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.set_counting(True)

    def run(beta):
        st = renderer.winding_numbers_device(len(pts), d_pts.data_ptr(), d_w.data_ptr(), beta, stats=True)
        return d_w.cpu().numpy().copy(), st
    base = {beta: run(beta) for beta in (0.0, 2.0)}
    # stack_entries 0 asks for the default depth; 1 is the smallest LDS stack there is: nearly every push spills
    for name, value in (("stack_entries", 0), ("stack_entries", 1), ("stack_entries", 3), ("inner_min_any", 40), ("inner_min_any", -2), ("inner_min", 3)):
        renderer.set_option(name, value)
        for beta, (w, st) in base.items():
            got, gs = run(beta)
            np.testing.assert_array_equal(_bits(got), _bits(w), err_msg="%s=%d beta %g" % (name, value, beta))
            assert (gs["nodes_visited"], gs["tris_tested"]) == (st["nodes_visited"], st["tris_tested"]), "%s=%d" % (name, value)
        for o, v in (("stack_entries", 0), ("inner_min", -6), ("inner_min_any", -6)):
            renderer.set_option(o, v)
    assert base[2.0][1]["nodes_visited"] < base[0.0][1]["nodes_visited"] and base[2.0][1]["tris_tested"] < base[0.0][1]["tris_tested"]


@pytest.mark.gpu
def test_inside_test_holds_on_open_meshes(pkg, feature_cases, renderer, trees):
    for name, cs in feature_cases.items():
        want = cs["f64"] > 0.5
        for tree in TREES:
            _upload(renderer, cs["scene"], tree)
            got = renderer.inside_winding(cs["points"], 2.0)
            bad = np.flatnonzero((got != want) & cs["judged"])
            assert len(bad) == 0, "%s %s: %d points on the wrong side, first %d: w_f64 = %r" % (name, tree, len(bad), bad[0], cs["f64"][bad[0]])
            sd = renderer.signed_distance(cs["points"], sign="winding")
            plain = renderer.signed_distance(cs["points"])
            dist = renderer.closest_points(cs["points"], want=("dist",))["dist"]
            occ = renderer.occupancy(cs["points"])
            np.testing.assert_array_equal(_bits(np.abs(sd)), _bits(dist))
            np.testing.assert_array_equal((sd < 0)[cs["judged"]], (want & (dist > 0))[cs["judged"]])
            np.testing.assert_array_equal(_bits(plain), _bits(np.where(occ, -dist, dist).astype(np.float32)))  # as before
            np.testing.assert_array_equal(_bits(renderer.signed_distance(cs["points"], sign="parity")), _bits(plain))


@pytest.mark.gpu
def test_call_rules_of_the_device_form(pkg, wref, dragon, renderer, trees):
    import torch
    L = pkg.lib()
    _upload(renderer, dragon)
    pts = query_points(pkg, dragon, np.random.default_rng(45))
    n = len(pts)
    host = renderer.winding_numbers(pts, 2.0)
    d_pts = torch.from_numpy(np.concatenate([pts.reshape(-1), np.zeros(4, np.float32)])).cuda()
    d_w = torch.zeros(n + 2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h = renderer.h
    assert L.crt_winding_numbers_device(h, n, d_pts.data_ptr() + 8, 2.0, d_w.data_ptr(), None) == 1   # CRT_EINVAL
    assert L.crt_winding_numbers_device(h, n, d_pts.data_ptr(), 2.0, d_w.data_ptr() + 2, None) == 1
    assert L.crt_winding_numbers_device(h, n, d_pts.data_ptr(), 2.0, None, None) == 1
    assert L.crt_winding_numbers_device(h, n, None, 2.0, d_w.data_ptr(), None) == 1
    side = torch.cuda.Stream()
    try:
        renderer.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            renderer.winding_numbers_device(n, d_pts.data_ptr(), d_w.data_ptr() + 4, 2.0)
        side.synchronize()
    finally:
        renderer.reset_stream()
    np.testing.assert_array_equal(_bits(d_w[1:n + 1].cpu().numpy()), _bits(host))
    st = renderer.winding_numbers_device(n, d_pts.data_ptr(), d_w.data_ptr(), 2.0, stats=True)
    assert st["rays_primary"] == n and st["kernel_ms"] > 0.0 and st["nodes_visited"] == 0 and st["tris_tested"] == 0
    renderer.set_counting(True)
    st = renderer.winding_numbers_device(n, d_pts.data_ptr(), d_w.data_ptr(), 2.0, stats=True)
    assert st["rays_primary"] == n and st["nodes_visited"] > 0 and st["tris_tested"] > 0
    renderer.set_counting(False)
    np.testing.assert_array_equal(_bits(d_w[:n].cpu().numpy()), _bits(host))
    # an empty scene: nothing winds; no scene: CRT_ESTATE
    renderer.upload([], [], [])
    try:
        assert not renderer.winding_numbers(pts, 2.0).any() and renderer.winding_moments().shape == (0, 32)
    finally:
        _upload(renderer, dragon)
    fresh = pkg.Renderer(0)
    try:
        out = np.zeros(n, np.float32)
        assert L.crt_winding_numbers(fresh.h, n, pts.ctypes.data, 2.0, out.ctypes.data, None) == 5
        assert L.crt_winding_moments_export(fresh.h, out.ctypes.data) == 5
    finally:
        fresh.close()


@pytest.mark.gpu
def test_winding_queries_leave_frames_untouched(pkg, scenes, renderer, trees):
    sc = scenes.cornell_box()
    _upload(renderer, sc)
    pts = query_points(pkg, sc, np.random.default_rng(46))
    renderer.change_shading_mode(100)
    before = renderer.render_frame(128, 128)
    for beta in (0.0, 2.0):
        renderer.winding_numbers(pts, beta)
    renderer.winding_moments()
    after = renderer.render_frame(128, 128)
    renderer.change_shading_mode(3)
    for k in ("rgba8", "hit_inst", "hit_prim", "hit_t"):
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)


@pytest.mark.gpu
def test_cpp_layer(pkg, scenes, renderer, trees, tmp_path):
    """crt::Renderer::windingNumbers / windingMoments, from a small C++ program linked against libcrt_hip.so, agree with the Python
    host path."""
    exe = str(tmp_path / "winding_cpp")
    csrc = os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + csrc,
                           "-o", exe, os.path.join(ROOT, "tests", "winding_cpp.cpp"), "-L" + os.path.dirname(pkg.LIB_PATH), "-lcrt_hip",
                           "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH), "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    sc = scenes.cornell_box()
    scene = pkg.Scene.from_arrays(sc)
    path = str(tmp_path / "cornell.crtbin")
    scene.save(path)
    pts = query_points(pkg, sc, np.random.default_rng(47))
    pts.tofile(str(tmp_path / "points.bin"))
    out = str(tmp_path / "winding.bin")
    subprocess.check_call([exe, path, str(tmp_path / "points.bin"), "2.0", out], timeout=120)
    raw = np.fromfile(out, dtype=np.float32)
    renderer.upload_scene(scene)
    np.testing.assert_array_equal(_bits(raw[:len(pts)]), _bits(renderer.winding_numbers(pts, 2.0)))
    np.testing.assert_array_equal(_bits(raw[len(pts):].reshape(-1, 32)), _bits(renderer.winding_moments()))
    assert np.abs(raw[:len(pts)]).max() > 0.1
    scene.close()
