"""Batched ray queries (crt_trace_rays* / crt_occluded_rays*, include/crt_hip.h): closest hit and occlusion of caller-supplied
rays.  Results are bit for bit those of the CPU oracle's traversal of the same ray; every GPU check here is exact (float bits
compared as uint32), not a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

SYMBOLS = ("crt_trace_rays_device", "crt_occluded_rays_device", "crt_trace_rays", "crt_occluded_rays")
MISS = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- CPU: the interface exists

def test_binding_and_library_expose_ray_queries(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
    for name in ("trace_rays", "occluded", "trace_rays_device", "occluded_device"):
        assert callable(getattr(pkg.Renderer, name, None)), name
    assert callable(getattr(pkg, "make_rays", None))
    assert L.crt_abi_version() == 1


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    rays = np.zeros((4, 8), dtype=np.float32)
    t = np.zeros(4, dtype=np.float32)
    occ = np.zeros(4, dtype=np.uint8)
    assert L.crt_trace_rays(None, 4, rays.ctypes.data, t.ctypes.data, None, None, None, None) == 1
    assert L.crt_occluded_rays(None, 4, rays.ctypes.data, occ.ctypes.data, None) == 1
    assert L.crt_trace_rays_device(None, 4, rays.ctypes.data, t.ctypes.data, None, None, None, None) == 1
    assert L.crt_occluded_rays_device(None, 4, rays.ctypes.data, occ.ctypes.data, None) == 1
    assert L.crt_trace_rays(None, 0, None, None, None, None, None, None) == 1
    assert L.crt_occluded_rays_device(None, 0, None, None, None) == 1


def test_make_rays_shapes_and_broadcasting(pkg):
    o = np.arange(12, dtype=np.float32).reshape(4, 3)
    d = np.ones((4, 3), dtype=np.float32)
    r = pkg.make_rays(o, d)
    assert r.shape == (4, 8) and r.dtype == np.float32 and r.flags["C_CONTIGUOUS"]
    assert np.array_equal(r[:, 0:3], o) and np.array_equal(r[:, 4:7], d)
    assert np.all(r[:, 3] == 0.0) and np.all(np.isinf(r[:, 7])) and np.all(r[:, 7] > 0)
    # one origin for many directions, per-ray tmin, scalar tmax
    r = pkg.make_rays((1.0, 2.0, 3.0), d, tmin=np.array([0.0, 0.5, 1.0, -1.0]), tmax=7.0)
    assert r.shape == (4, 8)
    assert np.array_equal(r[:, 0:3], np.broadcast_to(np.float32([1, 2, 3]), (4, 3)))
    assert np.array_equal(r[:, 3], np.float32([0.0, 0.5, 1.0, -1.0])) and np.all(r[:, 7] == 7.0)
    # many origins, one direction
    r = pkg.make_rays(o, (0.0, 0.0, -1.0), tmax=np.float32([1, 2, 3, 4]))
    assert np.array_equal(r[:, 4:7], np.broadcast_to(np.float32([0, 0, -1]), (4, 3))) and np.array_equal(r[:, 7], np.float32([1, 2, 3, 4]))
    # one ray
    assert pkg.make_rays((0, 0, 0), (0, 0, 1)).shape == (1, 8)
    with pytest.raises(ValueError):
        pkg.make_rays(np.zeros((4, 2)), d)


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _upload(renderer, sc):
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"))
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])


def _camera_rays(oracle, cam, w, h):
    d = np.zeros((h, w, 3), dtype=np.float32)
    for y in range(h):
        for x in range(w):
            d[y, x] = oracle.ray_dir(cam["matrix"], x, y, w, h)
    return d.reshape(-1, 3)


def _scene_triangles(sc):
    """float32 vertices of every triangle, in upload order (global id order), with its (inst, prim)"""
    v0, v1, v2, inst, prim = [], [], [], [], []
    for i, m in enumerate(sc["meshes"]):
        v = np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3)
        t = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)
        v0.append(v[t[:, 0]]); v1.append(v[t[:, 1]]); v2.append(v[t[:, 2]])
        inst.append(np.full(len(t), i, dtype=np.uint32)); prim.append(np.arange(len(t), dtype=np.uint32))
    cat = np.concatenate
    return cat(v0), cat(v1), cat(v2), cat(inst), cat(prim)


def _bounds(sc):
    v = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    return v.min(axis=0), v.max(axis=0)


def _mixed_rays(pkg, sc, n, seed):
    """n seeded rays mixing random rays, axis-aligned and near-axis directions (the kDirEps clamp), negative tmin with
    tmax = inf, rays starting on a surface with tmin = 0, and rays aimed at triangles"""
    rng = np.random.default_rng(seed)
    lo, hi = _bounds(sc)
    ext = hi - lo
    V0, V1, V2, _, _ = _scene_triangles(sc)

    def origins(k):
        return (lo - 0.1 * ext + rng.random((k, 3)) * 1.2 * ext).astype(np.float32)

    def dirs(k):
        d = rng.normal(size=(k, 3))
        return (d * rng.uniform(0.1, 10.0, size=(k, 1))).astype(np.float32)  # not normalised: t in units of |d|
    parts = []
    k = n // 5
    parts.append(pkg.make_rays(origins(k), dirs(k), tmin=0.001, tmax=rng.choice([np.inf, 1e4, 3.0], size=k)))
    axis = np.zeros((k, 3), dtype=np.float32)
    axis[np.arange(k), rng.integers(0, 3, size=k)] = rng.choice([-1.0, 1.0], size=k)
    tiny = rng.random((k, 3)) < 0.5
    axis = np.where(tiny, rng.choice([1e-25, -1e-22, 0.0, 1e-19, -1e-30], size=(k, 3)), axis).astype(np.float32)
    axis[np.all(axis == 0, axis=1), 1] = 1.0
    parts.append(pkg.make_rays(origins(k), axis, tmin=0.0, tmax=np.inf))
    parts.append(pkg.make_rays(origins(k), dirs(k), tmin=rng.uniform(-20.0, -0.01, size=k), tmax=np.inf))
    tri = rng.integers(0, len(V0), size=k)
    b = rng.dirichlet((1.0, 1.0, 1.0), size=k).astype(np.float32)
    on = (V0[tri] * b[:, 0:1] + V1[tri] * b[:, 1:2] + V2[tri] * b[:, 2:3]).astype(np.float32)
    parts.append(pkg.make_rays(on, dirs(k), tmin=0.0, tmax=np.inf))
    m = n - 4 * k
    tri = rng.integers(0, len(V0), size=m)
    b = rng.dirichlet((1.0, 1.0, 1.0), size=m).astype(np.float32)
    target = V0[tri] * b[:, 0:1] + V1[tri] * b[:, 1:2] + V2[tri] * b[:, 2:3]
    o = origins(m)
    parts.append(pkg.make_rays(o, (target - o).astype(np.float32), tmin=rng.uniform(0.0, 0.3, size=m), tmax=rng.choice([np.inf, 2.0, 1.0], size=m)))
    return np.ascontiguousarray(np.concatenate(parts))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cornell", "dragon"])
def test_camera_rays_equal_the_frame(pkg, oracle, scenes, dragon, renderer, which):
    """The frame's own camera rays, handed over as records, hit what the mode-3 frame and the oracle frame hit, and the
    instrumented kernel fetches exactly the nodes and triangles the oracle's traversal fetches."""
    sc, w, h = (scenes.cornell_box(), 256, 256) if which == "cornell" else (dragon, 480, 270)
    cam = sc["camera"]
    _upload(renderer, sc)
    renderer.change_shading_mode(3)
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    try:
        ref = O.render(cam["position"], cam["matrix"], 3, w, h)
        frame = renderer.render_frame(w, h)
        rays = pkg.make_rays(np.asarray(cam["position"], dtype=np.float32), _camera_rays(oracle, cam, w, h), tmin=0.001, tmax=10000.0)
        renderer.set_counting(True)
        got = renderer.trace_rays(rays)
        renderer.set_counting(False)
        plain = renderer.trace_rays(rays)
    finally:
        renderer.set_counting(False)
        O.close()
    for res in (got, plain):
        for src in (frame, ref):
            np.testing.assert_array_equal(res["inst"], src["hit_inst"].reshape(-1))
            np.testing.assert_array_equal(res["prim"], src["hit_prim"].reshape(-1))
            np.testing.assert_array_equal(_bits(res["t"]), _bits(src["hit_t"].reshape(-1)))
    assert (got["inst"] != MISS).sum() > w * h // 10, "the camera sees the scene"
    st, rs = got["stats"], ref["stats"]
    assert st["rays_primary"] == w * h and st["rays_shadow"] == 0
    assert (st["nodes_visited"], st["tris_tested"]) == (rs["nodes_visited"], rs["tris_tested"])
    assert plain["stats"]["nodes_visited"] == 0 and plain["stats"]["kernel_ms"] > 0.0


def _check_against_oracle(oracle, O, sc, rays, got, occ):
    tris = [np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3) for m in sc["meshes"]]
    verts = [np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]]
    hits = 0
    for i in range(len(rays)):
        o, tmin, d, tmax = rays[i, 0:3], rays[i, 3], rays[i, 4:7], rays[i, 7]
        inst, prim = int(got["inst"][i]), int(got["prim"][i])
        t, u, v = got["t"][i], got["uv"][i, 0], got["uv"][i, 1]
        if inst != MISS:
            hits += 1
            tri = tris[inst][prim]
            ok, rt, ru, rv = oracle.intersect_tri(o, d, verts[inst][tri[0]], verts[inst][tri[1]], verts[inst][tri[2]], tmin, tmax)
            assert ok, "ray %d: reported triangle (%d, %d) is not hit" % (i, inst, prim)
            assert _bits([t, u, v]).tolist() == _bits([rt, ru, rv]).tolist(), "ray %d: t, u, v" % i
            assert oracle.occluded(O, o, d, tmin, t) == 0, "ray %d: something strictly closer than the reported hit" % i
            assert occ[i], "ray %d: hit but not occluded" % i
        else:
            assert int(got["prim"][i]) == MISS and u == 0.0 and v == 0.0
            assert _bits([t]).tolist() == _bits([tmax]).tolist(), "ray %d: a miss reports tmax" % i
            assert oracle.occluded(O, o, d, tmin, tmax) == 0, "ray %d: reported a miss, the oracle finds a hit" % i
            assert not occ[i], "ray %d: miss but occluded" % i
        assert bool(occ[i]) == bool(oracle.occluded(O, o, d, tmin, tmax)), "ray %d: occlusion" % i
    return hits


def _soup(scenes):
    return scenes.icosphere_soup(n_spheres=400)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["dragon", "soup"])
def test_arbitrary_rays_against_the_oracle(pkg, oracle, scenes, dragon, renderer, which):
    sc = dragon if which == "dragon" else _soup(scenes)
    _upload(renderer, sc)
    rays = _mixed_rays(pkg, sc, 20000, seed=11)
    got = renderer.trace_rays(rays)
    occ = renderer.occluded(rays)
    assert occ.dtype == np.bool_ and occ.shape == (len(rays),)
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    try:
        hits = _check_against_oracle(oracle, O, sc, rays, got, occ)
    finally:
        O.close()
    assert 2000 < hits < len(rays) - 2000, "the ray mix holds hits and misses (%d hits)" % hits


@pytest.mark.gpu
def _cornell_with_twins(scenes):
    """Cornell plus coincident copies of its triangles: mesh 0 again as a later mesh, and mesh 2's triangles twice in one mesh"""
    sc = scenes.cornell_box()
    meshes = list(sc["meshes"])
    meshes.append(dict(meshes[0]))
    twice = meshes[2]
    meshes.append(dict(twice, triangles=np.concatenate([twice["triangles"], twice["triangles"]])))
    return dict(sc, meshes=meshes)


def _brute_closest(oracle, tris, ray):
    """lowest t in (tmin, tmax), then lowest global id: triangles in global id order, a later one wins only with a smaller t"""
    V0, V1, V2, INST, PRIM = tris
    best = (np.float32(np.inf), 0.0, 0.0, MISS, MISS)
    for k in range(len(V0)):
        ok, t, u, v = oracle.intersect_tri(ray[0:3], ray[4:7], V0[k], V1[k], V2[k], ray[3], ray[7])
        if ok and np.float32(t) < best[0]:
            best = (np.float32(t), u, v, int(INST[k]), int(PRIM[k]))
    return best


def _check_brute(oracle, tris, rays, got):
    for i in range(len(rays)):
        best = _brute_closest(oracle, tris, rays[i])
        assert (int(got["inst"][i]), int(got["prim"][i])) == (best[3], best[4]), "ray %d" % i
        if best[3] != MISS:
            assert _bits([got["t"][i], got["uv"][i, 0], got["uv"][i, 1]]).tolist() == _bits(best[:3]).tolist(), "ray %d" % i


def _interior_targets(rng, tris, n):
    """points inside random triangles, away from their edges (see the boundary-ray limit in include/crt_hip.h)"""
    V0, V1, V2 = tris[:3]
    tri = rng.integers(0, len(V0), size=n)
    b = (0.05 + 0.85 * rng.dirichlet((1.0, 1.0, 1.0), size=n)).astype(np.float32)
    return V0[tri] * b[:, 0:1] + V1[tri] * b[:, 1:2] + V2[tri] * b[:, 2:3]


@pytest.mark.gpu
def test_brute_force_and_ties(pkg, oracle, scenes, renderer):
    """Cornell with coincident triangles: the closest hit, its uv and the tie-break (lowest t, then lowest global triangle
    id) equal a brute-force loop over every triangle."""
    sc = _cornell_with_twins(scenes)
    _upload(renderer, sc)
    rng = np.random.default_rng(5)
    tris = _scene_triangles(sc)
    lo, hi = _bounds(sc)
    n = 1500
    target = _interior_targets(rng, tris, n)  # the coincident copies tie there
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    rays = pkg.make_rays(o, (target - o).astype(np.float32), tmin=0.001, tmax=np.inf)
    got = renderer.trace_rays(rays)
    _check_brute(oracle, tris, rays, got)
    # the duplicates were actually contested: some winners have a coincident twin with a higher id
    assert np.isin(got["inst"], [0, 2]).sum() > 100


@pytest.mark.gpu
def test_negative_t_brute_force_and_ties(pkg, oracle, scenes, renderer):
    """Hits behind the origin (negative tmin, negative tmax): closest hit and tie-break equal the brute-force loop, and a
    triangle strictly inside a negative interval (tmin, tmax) is found by both queries -- the box cull widens a negative bound
    instead of narrowing it."""
    sc = _cornell_with_twins(scenes)
    _upload(renderer, sc)
    rng = np.random.default_rng(8)
    tris = _scene_triangles(sc)
    lo, hi = _bounds(sc)
    n = 600
    o = (lo + (0.1 + 0.8 * rng.random((n, 3))) * (hi - lo)).astype(np.float32)  # inside the box
    d = (o - _interior_targets(rng, tris, n)).astype(np.float32)                 # the aimed-at point lies at t = -1
    rays = pkg.make_rays(o, d, tmin=-1e4, tmax=np.inf)                           # closest = the farthest hit behind
    got = renderer.trace_rays(rays)
    _check_brute(oracle, tris, rays, got)
    assert np.all(got["inst"] != MISS) and np.all(got["t"] < 0.0)
    assert np.isin(got["inst"], [0, 2]).sum() > 30
    # the nearest hit behind the origin, t* < 0; the interval (-1e4, t* (1 - 1e-6)) holds it strictly inside
    near = np.zeros(n, dtype=np.float32)
    for i in range(n):
        best = -np.inf
        for k in range(len(tris[0])):
            ok, t, _, _ = oracle.intersect_tri(rays[i, 0:3], rays[i, 4:7], tris[0][k], tris[1][k], tris[2][k], -1e4, 0.0)
            if ok:
                best = max(best, t)
        near[i] = best
    assert np.all(np.isfinite(near)) and np.all(near < 0.0)
    rays[:, 7] = near * np.float32(1.0 - 1e-6)
    assert np.all(rays[:, 7] > near)
    assert renderer.occluded(rays).all(), "a triangle strictly inside a negative interval is not found"
    got = renderer.trace_rays(rays)
    assert np.all(got["inst"] != MISS)
    _check_brute(oracle, tris, rays, got)


@pytest.mark.gpu
def test_degenerate_input(pkg, scenes, renderer):
    import torch
    L = pkg.lib()
    sc = scenes.cornell_box()
    _upload(renderer, sc)
    cam = sc["camera"]["position"]
    m = sc["meshes"][0]
    target = np.asarray(m["vertices"], dtype=np.float32)[np.asarray(m["triangles"])[0]].mean(axis=0)
    good = pkg.make_rays(cam, (target - cam).astype(np.float32), tmin=0.001, tmax=1e4)[0]  # aimed at a triangle: hits something
    bad = []
    for f in range(8):
        r = good.copy()
        r[f] = np.nan
        bad.append(r)
    for tmin, tmax in ((1.0, 1.0), (2.0, 1.0), (np.inf, np.inf), (-np.inf, -np.inf)):
        r = good.copy()
        r[3], r[7] = tmin, tmax
        bad.append(r)
    r = good.copy()
    r[4:7] = 0.0
    bad.append(r)
    rays = np.stack(bad + [good]).astype(np.float32)
    got = renderer.trace_rays(rays)
    occ = renderer.occluded(rays)
    nb = len(bad)
    assert np.all(got["inst"][:nb] == MISS) and np.all(got["prim"][:nb] == MISS)
    assert np.array_equal(_bits(got["t"][:nb]), _bits(rays[:nb, 7])) and np.all(got["uv"][:nb] == 0.0)
    assert not occ[:nb].any()
    assert got["inst"][nb] != MISS and occ[nb], "the control ray hits"

    # n = 0: OK, nothing launched, NULL buffers allowed
    e = renderer.trace_rays(np.zeros((0, 8), dtype=np.float32))
    assert all(len(e[k]) == 0 for k in ("t", "uv", "inst", "prim")) and e["stats"]["rays_primary"] == 0
    assert renderer.occluded(np.zeros((0, 8), dtype=np.float32)).shape == (0,)
    assert L.crt_trace_rays_device(renderer.h, 0, None, None, None, None, None, None) == 0
    assert L.crt_occluded_rays_device(renderer.h, 0, None, None, None) == 0

    # device buffers: misaligned rays, misaligned outputs, no output at all
    d_rays = torch.from_numpy(np.concatenate([rays.reshape(-1), np.zeros(8, np.float32)])).cuda()
    d_t = torch.zeros(len(rays) + 2, dtype=torch.float32, device="cuda")
    d_occ = torch.zeros(len(rays), dtype=torch.bool, device="cuda")
    n = len(rays)
    assert L.crt_trace_rays_device(renderer.h, n, d_rays.data_ptr() + 4, d_t.data_ptr(), None, None, None, None) == 1
    assert L.crt_occluded_rays_device(renderer.h, n, d_rays.data_ptr() + 8, d_occ.data_ptr(), None) == 1
    assert L.crt_trace_rays_device(renderer.h, n, d_rays.data_ptr(), d_t.data_ptr() + 2, None, None, None, None) == 1
    assert L.crt_trace_rays_device(renderer.h, n, d_rays.data_ptr(), None, d_t.data_ptr() + 4, None, None, None) == 1
    assert L.crt_trace_rays_device(renderer.h, n, d_rays.data_ptr(), None, None, None, None, None) == 1
    assert L.crt_occluded_rays_device(renderer.h, n, d_rays.data_ptr(), None, None) == 1
    assert "aligned" in L.crt_last_error(renderer.h).decode() or "NULL" in L.crt_last_error(renderer.h).decode()
    renderer.trace_rays_device(n, d_rays.data_ptr(), d_t=d_t.data_ptr())
    renderer.occluded_device(n, d_rays.data_ptr(), d_occ.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_t[:n].cpu().numpy()), _bits(got["t"])) and np.array_equal(d_occ.cpu().numpy(), occ)

    # an empty scene: every ray misses
    renderer.upload([], [], [])
    try:
        e = renderer.trace_rays(rays)
        assert np.all(e["inst"] == MISS) and np.all(e["prim"] == MISS) and np.array_equal(_bits(e["t"]), _bits(rays[:, 7]))
        assert not renderer.occluded(rays).any()
    finally:
        _upload(renderer, sc)

    # no scene
    fresh = pkg.Renderer(0)
    try:
        t = np.zeros(n, dtype=np.float32)
        o8 = np.zeros(n, dtype=np.uint8)
        assert L.crt_trace_rays(fresh.h, n, rays.ctypes.data, t.ctypes.data, None, None, None, None) == 5
        assert L.crt_occluded_rays(fresh.h, n, rays.ctypes.data, o8.ctypes.data, None) == 5
        assert L.crt_trace_rays_device(fresh.h, n, d_rays.data_ptr(), d_t.data_ptr(), None, None, None, None) == 5
        assert L.crt_occluded_rays_device(fresh.h, n, d_rays.data_ptr(), d_occ.data_ptr(), None) == 5
        with pytest.raises(pkg.CrtError):
            fresh.trace_rays(rays)
    finally:
        fresh.close()


def _device_query(renderer, rays_np):
    import torch
    n = len(rays_np)
    d_rays = torch.from_numpy(rays_np).cuda()
    t = torch.empty(n, dtype=torch.float32, device="cuda")
    uv = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    inst = torch.empty(n, dtype=torch.int32, device="cuda")
    prim = torch.empty(n, dtype=torch.int32, device="cuda")
    occ = torch.empty(n, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    st = renderer.trace_rays_device(n, d_rays.data_ptr(), t.data_ptr(), uv.data_ptr(), inst.data_ptr(), prim.data_ptr(), stats=True)
    so = renderer.occluded_device(n, d_rays.data_ptr(), occ.data_ptr(), stats=True)
    torch.cuda.synchronize()
    res = {"t": t.cpu().numpy(), "uv": uv.cpu().numpy(), "inst": inst.cpu().numpy().view(np.uint32),
           "prim": prim.cpu().numpy().view(np.uint32), "occ": occ.cpu().numpy()}
    return res, st, so


def _same(a, b, what):
    for k in ("inst", "prim"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=what + " " + k)
    assert np.array_equal(_bits(a["t"]), _bits(b["t"])), what + " t"
    assert np.array_equal(_bits(a["uv"]), _bits(b["uv"])), what + " uv"
    if "occ" in a and "occ" in b:
        np.testing.assert_array_equal(a["occ"], b["occ"], err_msg=what + " occluded")


@pytest.mark.gpu
def test_scale_tail_and_order(pkg, dragon, renderer):
    """2^20 + 37 rays through the device path equal the host path and the same rays shuffled (the cursor, the refill and
    the tail of the buffer all move), permuted back."""
    _upload(renderer, dragon)
    n = (1 << 20) + 37
    rays = _mixed_rays(pkg, dragon, n, seed=3)
    dev, st, so = _device_query(renderer, rays)
    assert st["rays_primary"] == n and st["rays_shadow"] == 0 and st["kernel_ms"] > 0.0
    assert so["rays_shadow"] == n and so["rays_primary"] == 0
    host = renderer.trace_rays(rays)
    host["occ"] = renderer.occluded(rays)
    _same(dev, host, "device vs host")
    perm = np.random.default_rng(9).permutation(n)
    shuf, _, _ = _device_query(renderer, np.ascontiguousarray(rays[perm]))
    back = {k: np.empty_like(v) for k, v in shuf.items()}
    for k, v in shuf.items():
        back[k][perm] = v
    _same(back, dev, "shuffled")
    hits = int((dev["inst"] != MISS).sum())
    assert n // 10 < hits < n - n // 10


@pytest.mark.gpu
def test_tuning_options_change_nothing(pkg, oracle, dragon, renderer):
    """2^19 + 37 rays -- more than 64 per workgroup the device holds at once, so the cursor, the mid-flight refill and the tail
    of the buffer all run -- with a one- and a three-entry LDS stack (nearly every push spills) and other scheduling
    thresholds: every output and both fetch counters are those of the default options.  A seeded sample of the default run
    is pinned to the oracle."""
    _upload(renderer, dragon)
    n = (1 << 19) + 37
    rays = _mixed_rays(pkg, dragon, n, seed=41)
    defaults = (("inner_min", -6), ("inner_min_any", -6), ("stack_entries", 0))
    counters = ("nodes_visited", "tris_tested")
    renderer.set_counting(True)
    try:
        base, st, so = _device_query(renderer, rays)
        assert all(st[k] > 0 and so[k] > 0 for k in counters)
        for name, value in (("stack_entries", 1), ("stack_entries", 3), ("inner_min", 3), ("inner_min_any", 40), ("inner_min_any", -2)):
            renderer.set_option(name, value)
            got, gt, go = _device_query(renderer, rays)
            for k, v in defaults:
                renderer.set_option(k, v)
            what = "%s=%d" % (name, value)
            _same(got, base, what)
            for k in counters:
                assert gt[k] == st[k], "%s: closest hit %s" % (what, k)
                assert go[k] == so[k], "%s: occlusion %s" % (what, k)
    finally:
        for k, v in defaults:
            renderer.set_option(k, v)
        renderer.set_counting(False)
    pick = np.sort(np.random.default_rng(42).choice(n, 2000, replace=False))
    O = oracle.OracleScene(dragon["meshes"], dragon["lights"], dragon["materials"])
    try:
        hits = _check_against_oracle(oracle, O, dragon, rays[pick], {k: base[k][pick] for k in ("t", "uv", "inst", "prim")}, base["occ"][pick])
    finally:
        O.close()
    assert 200 < hits < 1800, "the sample holds hits and misses (%d hits)" % hits


@pytest.mark.gpu
def test_tree_independence(pkg, scenes, dragon, renderer):
    """The same queries over the GPU-built LBVH give identical results, except for the boundary rays of include/crt_hip.h:
    a ray lying in a face of the boxes or starting on a surface can resolve differently where the two trees put their boxes
    differently.  Every difference must be such a ray (the axis-aligned and on-surface parts of the mix), and rare."""
    for sc in (dragon, _soup(scenes)):
        n = 50000
        k = n // 5
        rays = _mixed_rays(pkg, sc, n, seed=17)
        boundary = np.zeros(n, dtype=bool)
        boundary[k:2 * k] = True      # axis-aligned and near-axis directions
        boundary[3 * k:4 * k] = True  # starting on a surface, tmin = 0
        _upload(renderer, sc)
        a = renderer.trace_rays(rays)
        a["occ"] = renderer.occluded(rays)
        try:
            renderer.set_option("gpu_build", 1)
            _upload(renderer, sc)
            b = renderer.trace_rays(rays)
            b["occ"] = renderer.occluded(rays)
        finally:
            renderer.set_option("gpu_build", 0)
        differ = (a["inst"] != b["inst"]) | (a["prim"] != b["prim"]) | (_bits(a["t"]) != _bits(b["t"])) | \
                 np.any(_bits(a["uv"]) != _bits(b["uv"]), axis=1) | (a["occ"] != b["occ"])
        assert not differ[~boundary].any(), "rays %s differ between the trees" % np.flatnonzero(differ & ~boundary)[:10]
        assert differ.sum() <= n // 1000, "%d boundary rays differ" % differ.sum()


def _cornell_all_materials(scenes):
    sc = scenes.cornell_box()
    sc["materials"][1] = {"albedo": (0.9, 0.9, 0.9), "type": 2}
    sc["materials"][2] = {"albedo": (1.0, 1.0, 1.0), "type": 3, "ior": 1.5}
    return sc


@pytest.mark.gpu
def test_no_interference_with_frames(pkg, scenes, renderer):
    """Queries leave every frame as it would be without them: a mode-100 frame, and an accumulating mode-200 run with queries
    (some on another stream) between its frames equals the single K*S-spp frame; only frames advance the sample count."""
    import torch
    sc, w, h, S, K = _cornell_all_materials(scenes), 256, 256, 2, 4
    _upload(renderer, sc)
    rays = _mixed_rays(pkg, sc, 30000, seed=23)
    d_rays = torch.from_numpy(rays).cuda()
    d_t = torch.empty(len(rays), dtype=torch.float32, device="cuda")
    d_occ = torch.empty(len(rays), dtype=torch.bool, device="cuda")
    renderer.change_shading_mode(100)
    before = renderer.render_frame(w, h)
    for _ in range(5):
        renderer.trace_rays(rays)
        renderer.occluded(rays)
    after = renderer.render_frame(w, h)
    for k in ("rgba8", "hit_inst", "hit_prim", "hit_t"):
        np.testing.assert_array_equal(before[k], after[k], err_msg="mode 100 " + k)
    assert np.array_equal(before["rgb"], after["rgb"], equal_nan=True)

    renderer.change_shading_mode(200)
    renderer.set_miss_color((0.0, 0.0, 0.0))
    side = torch.cuda.Stream()
    try:
        renderer.set_path_params(K * S, 3, 1234)
        single = renderer.render_frame(w, h)
        renderer.set_option("spp", S)
        renderer.set_accumulation(1 << 24)
        for i in range(K):
            if i % 2:
                renderer.set_stream(side.cuda_stream)
                renderer.trace_rays_device(len(rays), d_rays.data_ptr(), d_t=d_t.data_ptr())
                renderer.occluded_device(len(rays), d_rays.data_ptr(), d_occ.data_ptr())
                renderer.reset_stream()
            else:
                renderer.trace_rays(rays)
            assert renderer.accumulated_samples() == i * S
            frame = renderer.render_frame(w, h)
            renderer.occluded(rays)
            assert renderer.accumulated_samples() == (i + 1) * S
        torch.cuda.synchronize()
        assert renderer.accumulated_samples() == K * S
        np.testing.assert_array_equal(frame["rgba8"], single["rgba8"])
        assert np.array_equal(frame["rgb"], single["rgb"], equal_nan=True)
    finally:
        renderer.reset_stream()
        renderer.set_accumulation(0)
        renderer.set_path_params(4, 3, 1234)
        renderer.set_miss_color((0.0, 1.0, 1.0))


@pytest.mark.gpu
def test_cpp_layer(pkg, scenes, renderer, tmp_path):
    """crt::Renderer::traceRays / occluded, from a small C++ program linked against libcrt_hip.so, agree with the Python host path."""
    exe = str(tmp_path / "ray_query_cpp")
    csrc = os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + csrc,
                           "-o", exe, os.path.join(ROOT, "tests", "ray_query_cpp.cpp"), "-L" + os.path.dirname(pkg.LIB_PATH), "-lcrt_hip",
                           "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH), "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    sc = scenes.cornell_box()
    scene = pkg.Scene.from_arrays(sc)
    path = str(tmp_path / "cornell.crtbin")
    scene.save(path)
    rays = _mixed_rays(pkg, sc, 4096, seed=31)
    rays.tofile(str(tmp_path / "rays.bin"))
    out = str(tmp_path / "hits.bin")
    subprocess.check_call([exe, path, str(tmp_path / "rays.bin"), out], timeout=120)
    raw = np.fromfile(out, dtype=np.uint8)
    n = len(rays)
    hit = raw[:n * 20].view(np.uint32).reshape(n, 5)
    occ = raw[n * 20:].astype(bool)
    renderer.upload_scene(scene)
    ref = renderer.trace_rays(rays)
    assert np.array_equal(hit[:, 0], _bits(ref["t"])) and np.array_equal(hit[:, 1:3], _bits(ref["uv"]))
    assert np.array_equal(hit[:, 3], ref["inst"]) and np.array_equal(hit[:, 4], ref["prim"])
    np.testing.assert_array_equal(occ, renderer.occluded(rays))
    assert (ref["inst"] != MISS).sum() > 500
    scene.close()
