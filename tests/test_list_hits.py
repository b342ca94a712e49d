"""All-hits ray queries (crt_list_hits*, include/crt_hip.h): every crossing of a ray as a CSR list sorted by (t', global id).
The GPU results are compared bit for bit (float bits as uint32) with tests/list_hits_reference.c, a brute-force restatement
over the exported triangle records; the reference itself is pinned to the hit counts of tests/point_reference.c and to the
oracle's brute-force closest hit.  No tolerance anywhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF
TREES = {"sah": {"gpu_build": 0}, "lbvh": {"gpu_build": 1, "gpu_builder": 0}, "ploc": {"gpu_build": 1, "gpu_builder": 1}}
KEYS = ("t", "uv", "inst", "prim")
SENT_F = np.float32(-12345.5)
SENT_U = np.uint32(0xDEADBEEF)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _compile(tmp_path_factory, name):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for tests/%s.c" % name)
    out = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
    base = [cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tests", name + ".c"), "-o", out, "-lm"]
    if subprocess.call(base[:1] + ["-fopenmp"] + base[1:], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)  # (no OpenMP: the pragmas are ignored)
    return C.CDLL(out)


@pytest.fixture(scope="session")
def ref(pkg, tmp_path_factory):
    L = _compile(tmp_path_factory, "list_hits_reference")
    vp, u32 = C.c_void_p, C.c_uint32
    L.ref_list_hits.argtypes = [vp, u32, u32, vp, vp, C.c_int, vp, vp, vp, vp]
    L.ref_list_hits.restype = None
    return L


@pytest.fixture(scope="session")
def point_ref(pkg, tmp_path_factory):
    L = _compile(tmp_path_factory, "point_reference")
    L.ref_count_hits.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.ref_count_hits.restype = None
    return L


def ref_list(ref, tris, rays):
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    n = len(rays)
    off = np.zeros(n + 1, np.uint64)
    ref.ref_list_hits(tris.ctypes.data, len(tris), n, rays.ctypes.data, off.ctypes.data, 0, None, None, None, None)
    tot = int(off[-1])
    out = {"t": np.zeros(tot, np.float32), "uv": np.zeros((tot, 2), np.float32), "inst": np.zeros(tot, np.uint32),
           "prim": np.zeros(tot, np.uint32)}
    ref.ref_list_hits(tris.ctypes.data, len(tris), n, rays.ctypes.data, off.ctypes.data, 1, *[out[k].ctypes.data for k in KEYS])
    out["offsets"] = off.astype(np.int64)
    return out


def _tri_records(pkg, meshes):
    """records {v0, e1 = v1 - v0, e2 = v2 - v0} in float32 with inst / prim / gid, as an upload writes them (upload order)"""
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
    return np.ascontiguousarray(np.concatenate(recs))


def _generic_rays(pkg, sc, rng, n):
    allv = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    lo, hi = allv.min(axis=0), allv.max(axis=0)
    o = lo - 0.1 * (hi - lo) + rng.random((n, 3)).astype(np.float32) * 1.2 * (hi - lo)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    rays = pkg.make_rays(o, d, tmin=rng.choice([0.0, 1e-3, -5.0], size=n), tmax=rng.choice([np.inf, 3.0, 1e4], size=n))
    rays[:4, 0] = np.nan
    rays[4:8, 3] = rays[4:8, 7]  # empty interval
    return rays


def _icosphere_mesh(scenes, subdiv, r, c):
    v, f = scenes._icosphere(subdiv)
    return {"vertices": (np.float32(r * v) + np.float32(c)).astype(np.float32), "triangles": f.astype(np.uint32),
            "material_index": 0, "normals": None}


def _assert_list_equal(got, want, what, keys=KEYS):
    np.testing.assert_array_equal(np.asarray(got["offsets"], dtype=np.int64), want["offsets"], err_msg="%s: offsets" % what)
    for k in keys:
        if k in ("inst", "prim"):
            g, w = np.asarray(got[k]).view(np.uint32).reshape(-1, 1), want[k].reshape(-1, 1)
        else:
            g, w = _bits(got[k]).reshape(len(want["t"]), -1), _bits(want[k]).reshape(len(want["t"]), -1)
        assert g.shape == w.shape, "%s: %s has %r records, the reference %r" % (what, k, g.shape, w.shape)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert len(bad) == 0, "%s: %s differs at %d of %d records, first %d: %r vs %r" % (what, k, len(bad), len(w), bad[0], g[bad[0]], w[bad[0]])


def _first_records(lst, n):
    """index of every non-empty list's first record, and the mask of the non-empty rays"""
    off = np.asarray(lst["offsets"], dtype=np.int64)
    has = np.diff(off) > 0
    return off[:-1][has], has


# ---- CPU: the interface exists, the reference is pinned to what is already pinned

def test_binding_and_library_expose_list_hits(pkg):
    L = pkg.lib()
    for s in ("crt_list_hits", "crt_list_hits_device"):
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
    for name in ("list_hits", "list_hits_device", "inside_length"):
        assert callable(getattr(pkg.Renderer, name, None)), name
    assert callable(pkg.inside_length)
    assert L.crt_abi_version() == 1


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    rays = np.zeros((4, 8), dtype=np.float32)
    off = np.zeros(5, dtype=np.uint64)
    tot = C.c_uint64(7)
    for f in (L.crt_list_hits, L.crt_list_hits_device):
        assert f(None, 4, rays.ctypes.data, off.ctypes.data, 0, None, None, None, None, C.byref(tot), None) == 1
        assert f(None, 0, None, None, 0, None, None, None, None, None, None) == 1


def test_reference_is_pinned_to_counts_and_closest_hits(pkg, ref, point_ref, oracle, dragon):
    rng = np.random.default_rng(21)
    tris = _tri_records(pkg, dragon["meshes"])
    rays = _generic_rays(pkg, dragon, rng, 3000)
    lst = ref_list(ref, tris, rays)
    off = lst["offsets"]
    cnt = np.zeros(len(rays), np.uint32)
    point_ref.ref_count_hits(tris.ctypes.data, len(tris), len(rays), rays.ctypes.data, cnt.ctypes.data)
    np.testing.assert_array_equal(np.diff(off), cnt.astype(np.int64))
    assert off[0] == 0 and np.all(cnt[:8] == 0) and (cnt > 1).sum() > 100
    o = oracle.OracleScene(dragon["meshes"], dragon["lights"], dragon["materials"])
    want = oracle.trace_rays(o, rays, brute_force=True)
    first, has = _first_records(lst, len(rays))
    np.testing.assert_array_equal(want["inst"] != MISS, has)
    np.testing.assert_array_equal(_bits(lst["t"][first]), _bits(want["t"][has]))
    np.testing.assert_array_equal(lst["inst"][first], want["inst"][has])
    np.testing.assert_array_equal(lst["prim"][first], want["prim"][has])
    np.testing.assert_array_equal(_bits(lst["uv"][first]), _bits(want["uv"][has]))
    # non-decreasing in t; strictly increasing global id inside runs of equal t (one scale exponent per ray: t orders as t')
    gid_of = {}
    for r in tris:
        gid_of[(int(r["inst"]), int(r["prim"]))] = int(r["gid"])
    gid = np.array([gid_of[(int(i), int(p))] for i, p in zip(lst["inst"], lst["prim"])], dtype=np.int64)
    same_ray = np.ones(len(lst["t"]) - 1, dtype=bool)
    same_ray[off[1:-1][(off[1:-1] > 0) & (off[1:-1] < len(lst["t"]))] - 1] = False
    dt = np.diff(lst["t"].astype(np.float64))
    assert np.all(dt[same_ray] >= 0)
    tie = same_ray & (dt == 0)
    assert np.all(np.diff(gid)[tie] > 0)


def test_inside_length_on_reference_lists(pkg, ref, scenes):
    m = _icosphere_mesh(scenes, 3, 1.0, (0.5, -0.25, 2.0))
    tris = _tri_records(pkg, [m])
    rng = np.random.default_rng(22)
    d = rng.normal(size=(200, 3)).astype(np.float32)
    o = (np.float32([0.5, -0.25, 2.0]) - 3.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = pkg.make_rays(o, d / np.linalg.norm(d, axis=1, keepdims=True) * np.float32(1.0001))  # through the centre
    lst = ref_list(ref, tris, rays)
    off = lst["offsets"]
    assert np.all(np.diff(off) == 2)
    got = pkg.inside_length(off, lst["t"])
    assert got.dtype == np.float64 and got.shape == (200,)
    want = lst["t"][1::2].astype(np.float64) - lst["t"][0::2].astype(np.float64)
    np.testing.assert_array_equal(got, want)
    assert np.all(np.abs(got - 2.0) < 0.05)
    # 0, 1 and 3 hits: 0, 0 and the first interval
    t = np.float32([1.5, 1.0, 2.25, 7.0])
    np.testing.assert_array_equal(pkg.inside_length(np.int64([0, 0, 1, 4]), t), np.float64([0.0, 0.0, np.float64(t[2]) - np.float64(t[1])]))
    assert pkg.inside_length(np.int64([0]), np.zeros(0, np.float32)).shape == (0,)


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def trees(renderer):
    yield
    for k, v in (("gpu_build", 0), ("gpu_builder", 0), ("inner_min", -6), ("inner_min_any", -6), ("stack_entries", 0), ("list_short_max", 24)):
        renderer.set_option(k, v)
    renderer.set_counting(False)


def _upload(renderer, sc, tree="sah", dynamic=False):
    for k, v in TREES[tree].items():
        renderer.set_option(k, v)
    renderer.upload(sc["meshes"], sc.get("lights", []), sc.get("materials", [{"albedo": (1, 1, 1), "type": 1}]), sc.get("textures"), dynamic=dynamic)
    if "camera" in sc:
        renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])


def _exported(renderer):
    return np.ascontiguousarray(renderer.bvh_export()[1])


def _raw_host(pkg, renderer, rays, capacity, want=KEYS, stats=False):
    """crt_list_hits with sentinel-prefilled arrays of `capacity` records: (rc, offsets, arrays, total, stats)"""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    n = len(rays)
    off = np.full(n + 1, 0xABABABABABABABAB, dtype=np.uint64)
    arr = {"t": np.full(capacity, SENT_F, np.float32), "uv": np.full((capacity, 2), SENT_F, np.float32),
           "inst": np.full(capacity, SENT_U, np.uint32), "prim": np.full(capacity, SENT_U, np.uint32)}
    tot = C.c_uint64(0xFFFF)
    st = pkg.FrameStats()
    p = [arr[k].ctypes.data if k in want else None for k in KEYS]
    rc = pkg.lib().crt_list_hits(renderer.h, n, rays.ctypes.data, off.ctypes.data, capacity, *p, C.byref(tot), C.byref(st) if stats else None)
    return rc, off.astype(np.int64), arr, tot.value, st.as_dict() if stats else None


def _sentinels_intact(arr, keys=KEYS):
    return all(np.all(arr[k] == (SENT_F if k in ("t", "uv") else SENT_U)) for k in keys)


def _check_against_everything(pkg, ref, renderer, rays, what):
    tris = _exported(renderer)
    want = ref_list(ref, tris, rays)
    tot = int(want["offsets"][-1])
    rc, off, arr, total, _ = _raw_host(pkg, renderer, rays, tot)
    assert rc == 0 and total == tot
    got = dict(arr, offsets=off)
    _assert_list_equal(got, want, what)
    np.testing.assert_array_equal(np.diff(off), renderer.count_hits(rays).astype(np.int64), err_msg="%s: counts" % what)
    tr = renderer.trace_rays(rays)
    first, has = _first_records(got, len(rays))
    np.testing.assert_array_equal(tr["inst"] != MISS, has, err_msg=what)
    for k in KEYS:
        g, w = got[k][first], tr[k][has]
        np.testing.assert_array_equal(_bits(g) if k in ("t", "uv") else g, _bits(w) if k in ("t", "uv") else w, err_msg="%s: first record %s" % (what, k))
    # the convenience wrapper (sizing call, then the filling call)
    py = renderer.list_hits(rays)
    _assert_list_equal(py, want, what + " (list_hits)")
    np.testing.assert_array_equal(py["ray"], np.repeat(np.arange(len(rays), dtype=np.uint32), np.diff(off)))
    assert py["offsets"].dtype == np.int64 and py["ray"].dtype == np.uint32
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
def test_dragon_lists_equal_the_reference(pkg, ref, dragon, renderer, trees, tree):
    rng = np.random.default_rng(31)
    _upload(renderer, dragon, tree, dynamic=True)
    rays = _generic_rays(pkg, dragon, rng, 30000)
    rays[:, 3] = rng.choice([0.0, -5.0, -0.5, 1e-3, 0.4], size=len(rays))
    rays[4:8, 3] = rays[4:8, 7]
    want = _check_against_everything(pkg, ref, renderer, rays, tree)
    cnt = np.diff(want["offsets"])
    assert (cnt > 1).sum() > 1000 and np.all(cnt[:8] == 0)
    # moved geometry: a vertex update (the last mesh bent along x) and a transform, refit, then rebuild
    last = len(dragon["meshes"]) - 1
    v = np.asarray(dragon["meshes"][last]["vertices"], dtype=np.float32).reshape(-1, 3).copy()
    ext = np.float32(v[:, 0].max() - v[:, 0].min())
    v[:, 1] += np.float32(0.05) * ext * np.sin(np.float32(6.0) * v[:, 0] / ext).astype(np.float32)
    v[:, 2] *= np.float32(1.125)
    renderer.update_vertices(last, v)
    c, s = np.cos(0.7), np.sin(0.7)
    m = np.float32([c, 0, s, 0.25, 0, 1, 0, -0.125, -s, 0, c, 0.5]).reshape(3, 4)
    renderer.set_mesh_transform(last, m)
    renderer.refit()
    moved = {"meshes": [{"vertices": renderer.mesh_vertices(i)[0], "triangles": mm["triangles"]} for i, mm in enumerate(dragon["meshes"])]}
    rays2 = _generic_rays(pkg, moved, rng, 10000)
    _check_against_everything(pkg, ref, renderer, rays2, tree + " refit")
    renderer.rebuild()
    _check_against_everything(pkg, ref, renderer, rays2, tree + " rebuild")


@pytest.mark.gpu
def test_tie_rule_orders_equal_t_by_global_id(pkg, ref, scenes, renderer, trees):
    """two meshes holding the same triangles and one mesh holding every triangle twice: equal t, order by global id"""
    a = _icosphere_mesh(scenes, 2, 1.0, (0.0, 0.0, 0.0))
    twice = dict(a, triangles=np.concatenate([a["triangles"], a["triangles"][::-1]]))
    b = _icosphere_mesh(scenes, 1, 2.0, (0.25, 0.0, 0.0))
    rng = np.random.default_rng(32)
    for order in ([a, dict(a), twice, b], [b, twice, dict(a), a]):
        sc = {"meshes": order}
        rays = _generic_rays(pkg, sc, rng, 4000)
        for tree in TREES:
            _upload(renderer, sc, tree)
            tris = _exported(renderer)
            want = ref_list(ref, tris, rays)
            got = renderer.list_hits(rays)
            _assert_list_equal(got, want, tree)
            # every crossing of the unit sphere is reported four times with one t, in ascending global id
            gid_of = np.zeros((4, len(twice["triangles"])), dtype=np.int64)
            gid_of[tris["inst"], tris["prim"]] = tris["gid"]
            gid = gid_of[got["inst"], got["prim"]]
            t, ray = got["t"], got["ray"]
            same = (np.diff(ray) == 0) & (np.diff(t) == 0)
            assert same.sum() > 1000 and np.all(np.diff(gid)[same] > 0)


def _sheet_stack(rng, n_sheets=40000, dz=0.01, half=5000.0):
    """n_sheets parallel two-triangle quads z = k dz (k = 0 .. n_sheets - 1), triangles in shuffled order"""
    z = (np.arange(n_sheets) * dz).astype(np.float32)
    corners = np.float32([[-half, -half], [half, -half], [half, half], [-half, half]])
    v = np.zeros((n_sheets, 4, 3), np.float32)
    v[:, :, 0:2] = corners
    v[:, :, 2] = z[:, None]
    base = 4 * np.arange(n_sheets)[:, None]
    t = np.concatenate([base + np.array([0, 1, 2]), base + np.array([0, 2, 3])])
    t = t[rng.permutation(len(t))]
    return {"vertices": v.reshape(-1, 3), "triangles": t.astype(np.uint32), "material_index": 0, "normals": None}


@pytest.mark.gpu
def test_long_and_awkward_lists(pkg, ref, renderer, trees):
    """a stack of 40 000 sheets crossed by oblique rays whose intervals clip the stack to 0, 1, 2, 3, 63, 64, 65, 127, 129,
    ~1 000 and ~40 000 hits in one launch: both sort paths and the global-memory passes, whatever the crossover is"""
    rng = np.random.default_rng(33)
    mesh = _sheet_stack(rng)
    sc = {"meshes": [mesh]}
    n = 300
    top = 40000 * 0.01
    # random origins below, inside and above the stack, random directions with a z component that carries them through it
    o = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-20.0, top + 20.0, n)], axis=1).astype(np.float32)
    o[:40, 2] = rng.uniform(-20.0, -1.0, 40).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:, 2] = np.where(rng.random(n) < 0.5, 1.0, -1.0) * (np.abs(d[:, 2]) + 0.7)
    d[:40, 2] = np.abs(d[:40, 2])
    rays = pkg.make_rays(o, d, tmin=0.0, tmax=np.inf)
    targets = [0, 1, 2, 3, 63, 64, 65, 127, 129, 1000, 40000]
    for tree in TREES:
        _upload(renderer, sc, tree)
        tris = _exported(renderer)
        full = ref_list(ref, tris, rays)
        off = full["offsets"]
        assert np.all(np.diff(off)[:2 * len(targets)] == 40000)  # the rays the targets are cut from cross every sheet
        clipped = rays.copy()
        for j, k in enumerate(targets + targets):
            t = full["t"][off[j]:off[j + 1]]
            if k < 40000:
                if j < len(targets):  # clip with tmax: the first k sheets
                    clipped[j, 7] = np.float32(0.5 * (float(t[k - 1]) + float(t[k]))) if k else np.float32(0.5 * float(t[0]))
                else:                 # clip with tmin and tmax: k sheets from the 100th on
                    clipped[j, 3] = np.float32(0.5 * (float(t[99]) + float(t[100])))
                    clipped[j, 7] = np.float32(0.5 * (float(t[99 + k]) + float(t[100 + k]))) if k else clipped[j, 3] * np.float32(1.00001)
        clipped[40:, 7] = rng.choice([np.inf, 3.0, 40.0, 1000.0], size=n - 40)
        want = ref_list(ref, tris, clipped)
        cnt = np.diff(want["offsets"])
        np.testing.assert_array_equal(cnt[:2 * len(targets)], np.int64(targets + targets))
        for short_max in (24, 1, 200):  # the crossover changes nothing
            renderer.set_option("list_short_max", short_max)
            rc, goff, arr, total, _ = _raw_host(pkg, renderer, clipped, int(want["offsets"][-1]))
            assert rc == 0 and total == want["offsets"][-1]
            _assert_list_equal(dict(arr, offsets=goff), want, "%s short_max %d" % (tree, short_max))
        np.testing.assert_array_equal(cnt, renderer.count_hits(clipped).astype(np.int64))


@pytest.mark.gpu
def test_direction_scale(pkg, ref, dragon, renderer, trees):
    rng = np.random.default_rng(34)
    rays = _generic_rays(pkg, dragon, rng, 8000)
    rays[:, 3] = rng.choice([0.0, -5.0, 1e-3], size=len(rays))
    rays[:, 7] = rng.choice([3.0, 40.0, 1e4], size=len(rays))  # finite intervals: the scaled ones stay normal floats
    for tree in TREES:
        _upload(renderer, dragon, tree)
        base = renderer.list_hits(rays)
        _assert_list_equal(base, ref_list(ref, _exported(renderer), rays), tree)
        for k in (-100, -20, 20, 100):
            s = rays.copy()
            s[:, 4:7] = np.ldexp(rays[:, 4:7], k)
            s[:, 3] = np.ldexp(rays[:, 3], -k)
            s[:, 7] = np.ldexp(rays[:, 7], -k)
            got = renderer.list_hits(s)
            np.testing.assert_array_equal(got["offsets"], base["offsets"])
            np.testing.assert_array_equal(got["inst"], base["inst"])
            np.testing.assert_array_equal(got["prim"], base["prim"])
            np.testing.assert_array_equal(_bits(got["uv"]), _bits(base["uv"]))
            scaled = np.ldexp(base["t"].astype(np.float64), -k)
            normal = (np.abs(scaled) >= 2.0 ** -126) & (np.abs(scaled) < 2.0 ** 128) & (np.abs(base["t"]) >= np.float32(2.0 ** -126))
            assert normal.sum() > 0.99 * len(scaled)
            np.testing.assert_array_equal(_bits(got["t"][normal]), _bits(scaled[normal].astype(np.float32)))
            _assert_list_equal(got, ref_list(ref, _exported(renderer), s), "%s 2^%d" % (tree, k))


@pytest.mark.gpu
def test_capacity_protocol(pkg, ref, dragon, renderer, trees):
    rng = np.random.default_rng(35)
    rays = _generic_rays(pkg, dragon, rng, 5000)
    for tree in TREES:
        _upload(renderer, dragon, tree)
        want = ref_list(ref, _exported(renderer), rays)
        tot = int(want["offsets"][-1])
        assert tot > 1000
        # one record short: offsets and total right, CRT_OK, no byte of the arrays touched
        rc, off, arr, total, _ = _raw_host(pkg, renderer, rays, tot - 1)
        assert rc == 0 and total == tot and _sentinels_intact(arr)
        np.testing.assert_array_equal(off, want["offsets"])
        # exactly enough
        rc, off, arr, total, _ = _raw_host(pkg, renderer, rays, tot)
        assert rc == 0 and total == tot
        _assert_list_equal(dict(arr, offsets=off), want, tree)
        # more than enough: the tail stays untouched
        rc, off, arr2, total, _ = _raw_host(pkg, renderer, rays, tot + 100)
        assert rc == 0 and total == tot and _sentinels_intact({k: v[tot:] for k, v in arr2.items()})
        _assert_list_equal(dict({k: v[:tot] for k, v in arr2.items()}, offsets=off), want, tree)
        # offsets only
        rc, off, arr0, total, _ = _raw_host(pkg, renderer, rays, 0, want=())
        assert rc == 0 and total == tot
        np.testing.assert_array_equal(off, want["offsets"])
        # subsets of the arrays
        for sub in (("t",), ("inst", "prim"), ("uv",), ("prim",), ("t", "inst")):
            rc, off, part, total, _ = _raw_host(pkg, renderer, rays, tot, want=sub)
            assert rc == 0 and total == tot
            _assert_list_equal(dict(part, offsets=off), want, "%s %r" % (tree, sub), keys=sub)
            assert _sentinels_intact(part, [k for k in KEYS if k not in sub])
        # the wrapper with a guess: too small falls back to the sizing protocol, large enough is used as it is
        for guess in (10, tot, tot + 1000):
            _assert_list_equal(renderer.list_hits(rays, capacity=guess), want, "%s capacity=%d" % (tree, guess))
        only_t = renderer.list_hits(rays, want=("t",))
        assert set(only_t) == {"t", "offsets", "ray", "stats"}
        np.testing.assert_array_equal(renderer.inside_length(rays), pkg.inside_length(want["offsets"], want["t"]))


@pytest.mark.gpu
def test_edge_cases(pkg, ref, dragon, renderer, trees):
    import torch
    L = pkg.lib()
    rng = np.random.default_rng(36)
    rays = _generic_rays(pkg, dragon, rng, 2000)
    rays[:, 7] = np.inf
    for f in range(8):  # a NaN in every field
        rays[8 + f, f] = np.nan
    rays[20:24, 3], rays[20:24, 7] = 2.0, 2.0          # tmin == tmax
    rays[24:28, 3], rays[24:28, 7] = 3.0, 1.0          # tmin > tmax
    rays[28:32, 4:7] = 0.0                             # zero direction
    rays[30:32, 4:7] = -0.0
    rays[32:36, 0:3] = np.float32([500.0, 500.0, 500.0])
    rays[32:36, 4:7] = np.float32([1.0, 0.5, 0.25])    # misses everything
    rays[36:100, 4:7] = rays[36:100, 4:7] * np.float32(1e-42)   # subnormal directions
    rays[36:100, 3] = -np.inf
    rays[100:164, 4:7] = rays[100:164, 4:7] / np.abs(rays[100:164, 4:7]).max(axis=1, keepdims=True) * np.float32(3.0e38)
    rays[100:164, 3] = np.float32(-1e-30)
    for tree in TREES:
        _upload(renderer, dragon, tree)
        want = ref_list(ref, _exported(renderer), rays)
        got = renderer.list_hits(rays)
        _assert_list_equal(got, want, tree)
        cnt = renderer.count_hits(rays)
        np.testing.assert_array_equal(np.diff(got["offsets"]), cnt.astype(np.int64))
        assert np.all(cnt[:16] == 0) and np.all(cnt[20:36] == 0) and (cnt[36:164] > 0).sum() > 30
    h = renderer.h
    # n = 0: CRT_OK, offsets[0] = 0, total = 0
    off = np.full(1, 99, np.uint64)
    tot = C.c_uint64(5)
    assert L.crt_list_hits(h, 0, None, off.ctypes.data, 0, None, None, None, None, C.byref(tot), None) == 0 and off[0] == 0 and tot.value == 0
    assert L.crt_list_hits(h, 0, None, None, 0, None, None, None, None, None, None) == 0
    assert L.crt_list_hits_device(h, 0, None, None, 0, None, None, None, None, None, None) == 0
    e = renderer.list_hits(np.zeros((0, 8), np.float32))
    assert e["offsets"].tolist() == [0] and e["t"].shape == (0,) and e["ray"].shape == (0,)
    # NULL rays / offsets, misaligned device pointers: CRT_EINVAL, nothing launched (the sentinels stay)
    n = len(rays)
    d_rays = torch.from_numpy(np.concatenate([rays.reshape(-1), np.zeros(8, np.float32)])).cuda()
    d_off = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    d_uv = torch.full((100001, 2), float(SENT_F), dtype=torch.float32, device="cuda")
    d_t = torch.full((100001,), float(SENT_F), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    args = (None, None, None, None, None, None)
    assert L.crt_list_hits_device(h, n, None, d_off.data_ptr(), 0, *args) == 1
    assert L.crt_list_hits_device(h, n, d_rays.data_ptr(), None, 0, *args) == 1
    assert L.crt_list_hits(h, n, None, off.ctypes.data, 0, *args) == 1
    assert L.crt_list_hits(h, n, rays.ctypes.data, None, 0, *args) == 1
    assert L.crt_list_hits_device(h, n, d_rays.data_ptr() + 8, d_off.data_ptr(), 0, *args) == 1
    assert L.crt_list_hits_device(h, n, d_rays.data_ptr(), d_off.data_ptr() + 4, 0, *args) == 1
    assert L.crt_list_hits_device(h, n, d_rays.data_ptr(), d_off.data_ptr(), 100000, None, d_uv.data_ptr() + 4, None, None, None, None) == 1
    assert L.crt_list_hits_device(h, n, d_rays.data_ptr(), d_off.data_ptr(), 100000, d_t.data_ptr() + 2, None, None, None, None, None) == 1
    torch.cuda.synchronize()
    assert bool((d_off == -7).all()) and bool((d_uv == float(SENT_F)).all()) and bool((d_t == float(SENT_F)).all())
    # an empty scene: every list is empty
    renderer.upload([], [], [])
    try:
        e = renderer.list_hits(rays)
        assert not e["offsets"].any() and len(e["t"]) == 0
    finally:
        _upload(renderer, dragon)
    # no scene
    fresh = pkg.Renderer(0)
    try:
        o2 = np.zeros(n + 1, np.uint64)
        assert L.crt_list_hits(fresh.h, n, rays.ctypes.data, o2.ctypes.data, 0, *args) == 5
        assert L.crt_list_hits_device(fresh.h, n, d_rays.data_ptr(), d_off.data_ptr(), 0, *args) == 5
    finally:
        fresh.close()


@pytest.mark.gpu
def test_device_form_streams_order_and_tuning(pkg, ref, dragon, renderer, trees):
    import torch
    rng = np.random.default_rng(37)
    rays = _generic_rays(pkg, dragon, rng, 20000)
    n = len(rays)
    for tree in TREES:
        _upload(renderer, dragon, tree)
        host = renderer.list_hits(rays)
        _assert_list_equal(host, ref_list(ref, _exported(renderer), rays), tree)
        tot = int(host["offsets"][-1])
        cap = tot + 17
        d_rays = torch.from_numpy(rays).cuda()
        d_off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
        d_t = torch.full((cap,), float(SENT_F), dtype=torch.float32, device="cuda")
        d_uv = torch.full((cap, 2), float(SENT_F), dtype=torch.float32, device="cuda")
        d_inst = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
        d_prim = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        try:
            renderer.set_stream(side.cuda_stream)
            with torch.cuda.stream(side):
                assert renderer.list_hits_device(n, d_rays.data_ptr(), d_off.data_ptr(), cap, d_t.data_ptr(), d_uv.data_ptr(), d_inst.data_ptr(),
                                                 d_prim.data_ptr()) is None
                # torch work on the same stream consumes the total without a host synchronise
                last = d_off[-1]
                d_live = (torch.arange(cap, device="cuda") < last).sum()
                d_sum = torch.where(torch.arange(cap, device="cuda") < last, d_inst, torch.zeros_like(d_inst)).long().sum()
                # a subset of the arrays on the device: key scratch comes from the context
                d_uv2 = torch.full((cap, 2), float(SENT_F), dtype=torch.float32, device="cuda")
                d_off2 = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
                renderer.list_hits_device(n, d_rays.data_ptr(), d_off2.data_ptr(), cap, d_uv=d_uv2.data_ptr())
                total, st = renderer.list_hits_device(n, d_rays.data_ptr(), d_off2.data_ptr(), 0, total=True, stats=True)
            side.synchronize()
        finally:
            renderer.reset_stream()
        assert total == tot and st["rays_primary"] == n and st["kernel_ms"] > 0.0
        dev = {"offsets": d_off.cpu().numpy(), "t": d_t[:tot].cpu().numpy(), "uv": d_uv[:tot].cpu().numpy(),
               "inst": d_inst[:tot].cpu().numpy(), "prim": d_prim[:tot].cpu().numpy()}
        _assert_list_equal(dev, host, tree + " device")
        assert bool((d_t[tot:] == float(SENT_F)).all()) and bool((d_prim[tot:] == -1).all()) and bool((d_uv2[tot:] == float(SENT_F)).all())
        assert int(d_live) == tot and int(d_sum) == int(host["inst"].astype(np.int64).sum())
        np.testing.assert_array_equal(_bits(d_uv2[:tot].cpu().numpy()), _bits(host["uv"]))
        np.testing.assert_array_equal(d_off2.cpu().numpy(), host["offsets"])
        # shuffling the buffer permutes the lists and changes nothing else
        perm = rng.permutation(n)
        sh = renderer.list_hits(rays[perm])
        cnt = np.diff(host["offsets"])
        np.testing.assert_array_equal(np.diff(sh["offsets"]), cnt[perm])
        src = np.concatenate([np.arange(host["offsets"][i], host["offsets"][i + 1]) for i in perm]) if tot else np.zeros(0, np.int64)
        for k in KEYS:
            a, b = sh[k], host[k][src]
            np.testing.assert_array_equal(_bits(a) if k in ("t", "uv") else a, _bits(b) if k in ("t", "uv") else b, err_msg=k)
        # tuning options change nothing
        for name, value in (("inner_min", 3), ("inner_min_any", 40), ("inner_min_any", -2), ("stack_entries", 4), ("list_short_max", 3)):
            renderer.set_option(name, value)
            _assert_list_equal(renderer.list_hits(rays), host, "%s %s=%d" % (tree, name, value))
        for k, v in (("inner_min", -6), ("inner_min_any", -6), ("stack_entries", 0), ("list_short_max", 24)):
            renderer.set_option(k, v)


@pytest.mark.gpu
def test_device_form_decides_the_capacity_on_the_device(pkg, ref, dragon, renderer, trees):
    """crt_list_hits_device with arrays one record short: the fill and sort kernels themselves read offsets[n] and leave.
    Offsets right, total right (asked for or not), CRT_OK, every sentinel intact, one traversal's fetches; with only uv asked
    for, the context's key scratch (sized from the capacity) is what would be overrun."""
    import torch
    rng = np.random.default_rng(40)
    rays = _generic_rays(pkg, dragon, rng, 20000)
    n = len(rays)
    for tree in TREES:
        _upload(renderer, dragon, tree)
        want = ref_list(ref, _exported(renderer), rays)
        tot = int(want["offsets"][-1])
        assert tot > 1000
        d_rays = torch.from_numpy(rays).cuda()
        d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        renderer.set_counting(True)
        base = renderer.count_hits_device(n, d_rays.data_ptr(), d_cnt.data_ptr(), stats=True)
        for cap in (tot - 1, tot // 2, 1, 0):
            for sub in (KEYS, ("uv",), ("t",), ("inst", "prim")):
                for ask_total in (False, True):
                    # the arrays hold exactly `cap` records and are followed by a guard region in the same allocation
                    guard = 4096
                    arr = {"t": torch.full((cap + guard,), float(SENT_F), dtype=torch.float32, device="cuda"),
                           "uv": torch.full((cap + guard, 2), float(SENT_F), dtype=torch.float32, device="cuda"),
                           "inst": torch.full((cap + guard,), -2, dtype=torch.int32, device="cuda"),
                           "prim": torch.full((cap + guard,), -2, dtype=torch.int32, device="cuda")}
                    d_off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
                    torch.cuda.synchronize()
                    p = {k: (arr[k].data_ptr() if k in sub else None) for k in KEYS}
                    got = renderer.list_hits_device(n, d_rays.data_ptr(), d_off.data_ptr(), cap, p["t"], p["uv"], p["inst"], p["prim"],
                                                    total=ask_total, stats=ask_total)
                    torch.cuda.synchronize()
                    what = "%s cap %d %r total %r" % (tree, cap, sub, ask_total)
                    np.testing.assert_array_equal(d_off.cpu().numpy(), want["offsets"], err_msg=what)
                    for k in KEYS:
                        sent = float(SENT_F) if k in ("t", "uv") else -2
                        assert bool((arr[k] == sent).all()), "%s: %s was written" % (what, k)
                    if ask_total:
                        total, st = got
                        assert total == tot, what
                        for k in ("nodes_visited", "tris_tested"):
                            assert st[k] == base[k], (what, k)  # exactly once: the second traversal did not run
                    else:
                        assert got is None
        # and the same buffers one record larger are filled
        arr = {"t": torch.full((tot,), float(SENT_F), dtype=torch.float32, device="cuda"),
               "uv": torch.full((tot, 2), float(SENT_F), dtype=torch.float32, device="cuda"),
               "inst": torch.full((tot,), -2, dtype=torch.int32, device="cuda"), "prim": torch.full((tot,), -2, dtype=torch.int32, device="cuda")}
        d_off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
        total, st = renderer.list_hits_device(n, d_rays.data_ptr(), d_off.data_ptr(), tot, *[arr[k].data_ptr() for k in KEYS], total=True, stats=True)
        renderer.set_counting(False)
        assert total == tot
        for k in ("nodes_visited", "tris_tested"):
            assert st[k] == 2 * base[k], (tree, k)
        _assert_list_equal(dict({k: v.cpu().numpy() for k, v in arr.items()}, offsets=d_off.cpu().numpy()), want, tree + " cap == total")


@pytest.mark.gpu
def test_listings_in_flight_on_two_streams(pkg, ref, dragon, renderer, trees):
    """a listing on stream A, crt_set_stream, another on stream B, nothing synchronised in between: each has its own counts,
    tile sums and key scratch, so both equal the reference (only uv is asked for: the key scratch is the context's)"""
    import torch
    rng = np.random.default_rng(41)
    _upload(renderer, dragon)
    tris = _exported(renderer)
    sets = [_generic_rays(pkg, dragon, rng, 200000), _generic_rays(pkg, dragon, rng, 150000)]
    want = [ref_list(ref, tris, r) for r in sets]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rep in range(3):
        bufs = []
        for r, w in zip(sets, want):
            cap = int(w["offsets"][-1])
            bufs.append((torch.from_numpy(r).cuda(), torch.full((len(r) + 1,), -7, dtype=torch.int64, device="cuda"),
                         torch.full((cap, 2), float(SENT_F), dtype=torch.float32, device="cuda"),
                         torch.full((cap,), -2, dtype=torch.int32, device="cuda"), cap))
        torch.cuda.synchronize()
        try:
            for s, (d_rays, d_off, d_uv, d_inst, cap) in zip(streams, bufs):
                renderer.set_stream(s.cuda_stream)
                renderer.list_hits_device(len(d_rays), d_rays.data_ptr(), d_off.data_ptr(), cap, d_uv=d_uv.data_ptr(), d_inst=d_inst.data_ptr())
        finally:
            renderer.reset_stream()
        torch.cuda.synchronize()
        for i, ((d_rays, d_off, d_uv, d_inst, cap), w) in enumerate(zip(bufs, want)):
            _assert_list_equal({"offsets": d_off.cpu().numpy(), "uv": d_uv.cpu().numpy(), "inst": d_inst.cpu().numpy()}, w,
                               "stream %d, round %d" % (i, rep), keys=("uv", "inst"))


@pytest.mark.gpu
def test_counting_twice_when_filling_once_when_not(pkg, scenes, renderer, trees):
    sc = scenes.heightfield()
    rng = np.random.default_rng(38)
    rays = _generic_rays(pkg, sc, rng, 20000)
    rays[:, 7] = np.inf
    n = len(rays)
    for tree in TREES:
        _upload(renderer, sc, tree)
        renderer.set_counting(True)
        import torch
        d_rays = torch.from_numpy(rays).cuda()
        d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        base = renderer.count_hits_device(n, d_rays.data_ptr(), d_cnt.data_ptr(), stats=True)
        rc, off, arr, tot, once = _raw_host(pkg, renderer, rays, 0, want=(), stats=True)
        assert rc == 0 and tot > 0
        rc, off, arr, tot2, twice = _raw_host(pkg, renderer, rays, tot, stats=True)
        rc, off, arr, tot3, short = _raw_host(pkg, renderer, rays, tot - 1, stats=True)
        renderer.set_counting(False)
        assert tot2 == tot and tot3 == tot and _sentinels_intact(arr)
        for k in ("nodes_visited", "tris_tested"):
            assert base[k] > 0
            assert once[k] == base[k], (tree, k)
            assert twice[k] == 2 * base[k], (tree, k)
            assert short[k] == base[k], (tree, k)
        assert twice["rays_primary"] == n
        tris, nodes = base["tris_tested"] / n, base["nodes_visited"] / n
        print("%s: heightfield list: %.1f triangles, %.1f nodes per ray and traversal, %.2f hits per ray" % (tree, tris, nodes, tot / n))
        assert 0 < tris < 40 and 0 < nodes < 80


@pytest.mark.gpu
def test_list_queries_leave_frames_untouched(pkg, scenes, renderer, trees):
    import torch
    sc = scenes.cornell_box()
    _upload(renderer, sc)
    rng = np.random.default_rng(39)
    rays = _generic_rays(pkg, sc, rng, 3000)
    d_rays = torch.from_numpy(rays).cuda()
    d_off = torch.zeros(len(rays) + 1, dtype=torch.int64, device="cuda")
    d_t = torch.zeros(100000, dtype=torch.float32, device="cuda")
    w = h = 128
    renderer.change_shading_mode(100)
    before = renderer.render_frame(w, h)
    for _ in range(3):
        renderer.list_hits(rays)
        renderer.list_hits_device(len(rays), d_rays.data_ptr(), d_off.data_ptr(), 100000, d_t=d_t.data_ptr())
    after = renderer.render_frame(w, h)
    for k in ("rgba8", "hit_inst", "hit_prim", "hit_t"):
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    renderer.change_shading_mode(200)
    try:
        renderer.set_path_params(2, 3, 1234)
        frames = {}
        for with_queries in (False, True):
            renderer.set_accumulation(0)
            renderer.set_accumulation(1 << 24)
            for i in range(3):
                assert renderer.accumulated_samples() == 2 * i
                if with_queries:
                    renderer.list_hits(rays)
                    renderer.list_hits_device(len(rays), d_rays.data_ptr(), d_off.data_ptr(), 100000, d_t=d_t.data_ptr())
                    assert renderer.accumulated_samples() == 2 * i
                frames[with_queries] = renderer.render_frame(w, h)
            torch.cuda.synchronize()
            assert renderer.accumulated_samples() == 6
        np.testing.assert_array_equal(frames[False]["rgba8"], frames[True]["rgba8"])
    finally:
        renderer.set_accumulation(0)
        renderer.set_path_params(4, 3, 1234)
        renderer.change_shading_mode(3)
