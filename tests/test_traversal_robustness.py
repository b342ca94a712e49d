"""BVH traversal pinned to brute force far from the origin.

The slab test computes a box's distances as fma(plane, 1/d, -(o/d)); rounding gives that an absolute error of about
2^-23 |o/d| per axis, which does not shrink with t.  Without the pads of the conservative slab test
boxes a ray really enters were culled, and rays passed through closed meshes placed far from the origin.  Every other
traversal test compares the GPU with the oracle's traversal of the same tree, which shares the slab arithmetic; these
compare both with a traversal that has no boxes at all (the oracle's brute force), and brute force with a float64
Moeller-Trumbore (tests/path_reference.py).

Scenes: closed meshes (an icosphere, a box of small axis-aligned triangles) centred at offsets up to 2^17 on all three axes
with radius 1 and 1/16, sliver triangles (aspect 1e4) in an axis plane and tilted, and a height field translated to 2^13;
cameras inside the closed meshes (where every pixel must hit) and outside.  Offsets, radii and grid vertices are powers of
two, so that the translated vertices are the same float32 values whatever the offset's magnitude allows."""
import math

import numpy as np
import pytest

import path_reference as R
import shaded_query_checks as sq

MISS = 0xFFFFFFFF
OFFSETS = (0.0, 128.0, 1024.0, 8192.0, 131072.0)  # ~ 1e2, 1e3, 1e4, 1e5
RADII = (1.0, 0.0625)
AXES = np.array([1.0, 0.75, -0.5])  # the offset is applied on all three axes
W, H = 96, 96
MAT = [{"albedo": (0.8, 0.7, 0.6), "type": 1}]
KEYS = ("hit_inst", "hit_prim", "hit_t", "rgba8", "rgb")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mesh(v, t):
    return {"vertices": np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3),
            "triangles": np.ascontiguousarray(t, dtype=np.uint32).reshape(-1, 3), "material_index": 0, "normals": None}


def _look_from(centre, dist, yaw, pitch):
    """camera at `dist` from centre looking at it: camera_matrix looks along -forward"""
    y, p = math.radians(yaw), math.radians(pitch)
    f = np.array([math.cos(p) * math.sin(y), math.sin(p), math.cos(p) * math.cos(y)])
    return np.float32(centre + dist * f)


def _box_mesh(c, r, n=8):
    """closed axis-aligned box of half size r: every face an n x n grid of quads, two triangles each (grid vertices)"""
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
            tris += [np.stack([q, q + 1, q + n + 1], 1), np.stack([q + n + 2, q + n + 1, q + 1], 1)]
    return _mesh(c + r * np.concatenate(verts), np.concatenate(tris))


def closed_scene(scenes, kind, off, r):
    """an icosphere (5120 triangles) or a box of 768 small triangles, centred at off * AXES; cameras inside and outside"""
    c = off * AXES
    if kind == "sphere":
        sv, sf = scenes._icosphere(4)
        m = _mesh(np.float32(r * sv) + np.float32(c), sf)  # the float32 sum: what a translation by c makes of the mesh at 0
    else:
        m = _box_mesh(c, r)
    inside = {"position": np.float32(c), "matrix": scenes.camera_matrix(20.0, 10.0)}
    outside = {"position": _look_from(c, 3.0 * r, 35.0, 25.0), "matrix": scenes.camera_matrix(35.0, 25.0)}
    light_in = tuple(c + r * np.array([0.25, 0.5, 0.125]))
    return {"meshes": [m], "lights": [(light_in, 4.0 * r * r)], "materials": MAT,
            "cameras": {"inside": inside, "outside": outside}}


def sliver_scene(scenes, off):
    """two patches of right triangles with legs 2r and 2r / 1e4 (aspect 1e4): one in an axis plane (zero-thickness boxes),
    one tilted; the camera above the flat one sees nothing else"""
    r = 1.0
    c = off * AXES
    n = 1024
    w = 2.0 * r * 1e-4
    y = np.arange(n + 1) * w
    v0 = np.stack([np.full(n + 1, -r), y, np.zeros(n + 1)], 1)
    v1 = np.stack([np.full(n + 1, r), y, np.zeros(n + 1)], 1)
    v = np.concatenate([v0, v1])
    i = np.arange(n)
    t = np.concatenate([np.stack([i, i + n + 1, i + 1], 1), np.stack([i + n + 2, i + 1, i + n + 1], 1)])
    flat = v - [0.0, n * w / 2, 0.0]
    tilt = flat @ np.array([[1.0, 0.0, 0.0], [0.0, 0.8, 0.6], [0.0, -0.6, 0.8]]).T + [0.0, 0.0, -0.25]
    meshes = [_mesh(c + flat, t), _mesh(c + tilt, t)]
    # above the flat patch at a height of a tenth of its width, looking straight down at it (through nothing else)
    down = {"position": np.float32(c + [0.0, 0.0, 0.01]), "matrix": np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1])}
    oblique = {"position": _look_from(c, 0.75, 15.0, 30.0), "matrix": scenes.camera_matrix(15.0, 30.0)}
    return {"meshes": meshes, "lights": [(tuple(c + [0.0, 0.5, 0.5]), 2.0)], "materials": MAT,
            "cameras": {"down": down, "oblique": oblique}}


def heightfield_scene(scenes, off=8192.0):
    """a 32 x 32 height field of extent +-1 on a grid of 1/16 (heights on a grid of 2^-10), translated to off * AXES"""
    c = off * AXES
    n = 32
    g = np.arange(n + 1) / 16.0 - 1.0
    x, z = np.meshgrid(g, g, indexing="ij")
    hgt = np.round((0.25 * np.sin(3.0 * x + 1.0) * np.cos(2.0 * z) + 0.1 * np.sin(7.0 * x * z)) * 1024.0) / 1024.0
    v = np.stack([x, hgt, z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).reshape(-1)
    t = np.concatenate([np.stack([a, a + 1, a + n + 1], 1), np.stack([a + n + 2, a + n + 1, a + 1], 1)])
    above = {"position": _look_from(c, 1.5, 30.0, 50.0), "matrix": scenes.camera_matrix(30.0, 50.0)}
    low = {"position": _look_from(c + [0.0, 0.3, 0.0], 1.25, -60.0, 8.0), "matrix": scenes.camera_matrix(-60.0, 8.0)}
    return {"meshes": [_mesh(c + v, t)], "lights": [(tuple(c + [0.5, 2.0, 0.25]), 6.0)], "materials": MAT,
            "cameras": {"above": above, "low": low}}


CLOSED = [(k, off, r) for k in ("sphere", "box") for off in OFFSETS for r in RADII]


def _cid(p):
    return "%s-%g-r%g" % p


def _oracle_scene(oracle, sc):
    return oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])


def _render(oracle, S, cam, mode, w=W, h=H, brute=False):
    return S.render(cam["position"], cam["matrix"], mode, w, h, brute_force=brute)


def _assert_same(got, ref, what):
    for k in KEYS:
        if k not in got:
            continue
        if k in ("hit_t", "rgb"):
            diff = _bits(got[k]) != _bits(ref[k])
        else:
            diff = got[k] != ref[k]
        n = int(np.count_nonzero(diff.reshape(diff.shape[0], diff.shape[1], -1).any(-1) if diff.ndim == 3 else diff))
        assert n == 0, "%s: %s differs from brute force on %d pixels" % (what, k, n)


# mode 200 at 1 spp and 2 bounces (path_params): bounce and shadow rays start on surfaces
MODES = ((3, "mode 3"), (100, "mode 100"), (200, "mode 200"))


@pytest.fixture
def path_params(oracle):
    oracle.set_path_params(1, 2, 77)
    yield
    oracle.set_path_params(4, 3, 1234)


def _surface_rays(pkg, rng, sc, hit, n=1500):
    """rays that start on the surface: origins at the hit points of a brute-force frame (float32, as a shading point is),
    towards random vertices of the scene, tmin 0 or 1e-4, tmax short of the target or beyond it"""
    cam = hit["cam"]
    ok = np.flatnonzero(hit["hit_inst"].reshape(-1) != MISS)
    pix = rng.choice(ok, size=min(n, len(ok)), replace=False)
    d0 = hit["dirs"].reshape(-1, 3)[pix]
    t0 = hit["hit_t"].reshape(-1)[pix]
    o = np.float32(cam["position"] + d0 * t0[:, None])
    allv = np.concatenate([m["vertices"] for m in sc["meshes"]])
    tgt = allv[rng.integers(0, len(allv), size=len(o))]
    d = np.float32(tgt - o)
    keep = np.abs(d).max(1) > 0
    o, d = o[keep], d[keep]
    tmin = rng.choice([0.0, 1e-4], size=len(o))
    tmax = rng.choice([0.999, 2.0, np.inf], size=len(o))
    return pkg.make_rays(o, d, tmin=tmin, tmax=tmax)


def _camera_dirs(oracle, cam, w, h):
    d = np.zeros((h, w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            d[y, x] = oracle.ray_dir(cam["matrix"], x, y, w, h)
    return d


def _check_rays_brute(oracle, S, rays, what):
    """the oracle's wide and binary walks of arbitrary rays equal brute force: closest hit and occlusion"""
    ref = oracle.trace_rays(S, rays, brute_force=True)
    occ_ref = np.array([oracle.occluded(S, q[0:3], q[4:7], q[3], q[7], brute_force=True) for q in rays])
    for width in (4, 2):
        S.set_width(width)
        got = oracle.trace_rays(S, rays)
        for k in ("inst", "prim"):
            n = int(np.count_nonzero(got[k] != ref[k]))
            assert n == 0, "%s width %d: %s differs from brute force on %d of %d rays" % (what, width, k, n, len(rays))
        assert np.array_equal(_bits(got["t"]), _bits(ref["t"])), "%s width %d: t" % (what, width)
        occ = np.array([oracle.occluded(S, q[0:3], q[4:7], q[3], q[7]) for q in rays])
        n = int(np.count_nonzero(occ != occ_ref))
        assert n == 0, "%s width %d: occluded differs from brute force on %d of %d rays" % (what, width, n, len(rays))
    S.set_width(4)
    return ref, occ_ref


def _check_float64(S64, o, d, tmin, tmax, inst, prim, t, what, min_robust=0.5):
    """brute force against the float64 Moeller-Trumbore on the rays whose result is robust (path_reference's margins):
    same triangle, t within rtol 1e-5 (atol 1e-6)"""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    o = np.broadcast_to(o, d.shape)
    tmin, tmax = np.broadcast_to(np.float64(tmin), len(d)), np.broadcast_to(np.float64(tmax), len(d))
    robust_n = 0
    for s in range(0, len(d), 128):
        sl = slice(s, s + 128)
        for tl in np.unique(np.stack([tmin[sl], tmax[sl]], 1), axis=0):
            sel = np.flatnonzero((tmin[sl] == tl[0]) & (tmax[sl] == tl[1])) + s
            hit, tri, tref, _, _, robust = S64.closest(o[sel], d[sel], tl[0], tl[1])
            rb = np.flatnonzero(robust)
            robust_n += len(rb)
            idx = sel[rb]
            want_inst = np.where(hit[rb], S64.inst[tri[rb]], MISS)
            want_prim = np.where(hit[rb], S64.prim[tri[rb]], MISS)
            bad = np.flatnonzero((inst[idx] != want_inst) | (prim[idx] != want_prim))
            assert len(bad) == 0, "%s: brute force and float64 disagree on the triangle of %d robust rays (first: ray %d)" % (
                what, len(bad), idx[bad[0]])
            h = rb[hit[rb]]
            # float32 Moeller-Trumbore: relative error ~1e-6 of the distance to the triangle's corner, which is what sets atol
            # for the short rays between two surfaces
            np.testing.assert_allclose(t[sel[h]], tref[h], rtol=1e-5, atol=1e-6, err_msg=what + ": t against float64")
    assert robust_n >= min_robust * len(d), "%s: only %d of %d rays robust" % (what, robust_n, len(d))


# ----------------------------------------------------------------------------------------------------- CPU: the oracle
@pytest.mark.parametrize("kind,off,r", CLOSED, ids=[_cid(p) for p in CLOSED])
def test_closed_meshes_bvh_equals_brute_force(pkg, oracle, scenes, path_params, kind, off, r):
    sc = closed_scene(scenes, kind, off, r)
    S = _oracle_scene(oracle, sc)
    for cname, cam in sc["cameras"].items():
        for mode, label in MODES:
            w, h = (W, H) if mode == 3 else (48, 48)
            ref = _render(oracle, S, cam, mode, w, h, brute=True)
            if cname == "inside" and mode == 3:
                assert np.all(ref["hit_inst"] != MISS), "brute force misses from inside"
            for width in (4, 2):
                S.set_width(width)
                got = _render(oracle, S, cam, mode, w, h)
                what = "%s %s camera %s width %d" % (_cid((kind, off, r)), cname, label, width)
                if cname == "inside" and mode == 3:
                    n = int(np.count_nonzero(got["hit_inst"] == MISS))
                    assert n == 0, "%s: %d of %d pixels miss a closed mesh from inside" % (what, n, w * h)
                _assert_same(got, ref, what)
            S.set_width(4)


@pytest.mark.parametrize("which", ["slivers", "heightfield"] + ["slivers-%g" % o for o in OFFSETS[1:]])
def test_open_scenes_bvh_equals_brute_force(pkg, oracle, scenes, path_params, which):
    if which == "heightfield":
        sc = heightfield_scene(scenes)
    else:
        sc = sliver_scene(scenes, float(which.split("-")[1]) if "-" in which else 0.0)
    S = _oracle_scene(oracle, sc)
    for cname, cam in sc["cameras"].items():
        for mode, label in MODES:
            w, h = (W, H) if mode == 3 else (48, 48)
            ref = _render(oracle, S, cam, mode, w, h, brute=True)
            if cname == "down" and mode == 3:
                assert np.all(ref["hit_inst"] == 0), "the flat sliver patch fills the view"
            for width in (4, 2):
                S.set_width(width)
                _assert_same(_render(oracle, S, cam, mode, w, h), ref, "%s %s camera %s width %d" % (which, cname, label, width))
            S.set_width(4)


SURFACE_CASES = [("sphere", 131072.0, 0.0625), ("box", 8192.0, 0.0625), ("sphere", 1024.0, 1.0), ("sphere", 0.0, 0.0625),
                 ("slivers", 8192.0, None), ("heightfield", 8192.0, None)]


def _scene_of(scenes, kind, off, r):
    if kind == "slivers":
        return sliver_scene(scenes, off)
    if kind == "heightfield":
        return heightfield_scene(scenes, off)
    return closed_scene(scenes, kind, off, r)


@pytest.mark.parametrize("kind,off,r", SURFACE_CASES, ids=["%s-%g" % (k, o) for k, o, _ in SURFACE_CASES])
def test_rays_from_surfaces_and_float64(pkg, oracle, scenes, kind, off, r):
    """rays that start on surfaces (closest hit and occlusion) through both walks equal brute force, and brute force
    (frames and surface rays) equals the float64 Moeller-Trumbore wherever the float64 result is robust"""
    sc = _scene_of(scenes, kind, off, r)
    S = _oracle_scene(oracle, sc)
    S64 = R.Scene(sc)
    rng = np.random.default_rng(int(off) + 7)
    for cname, cam in sc["cameras"].items():
        w, h = 48, 48
        ref = _render(oracle, S, cam, 3, w, h, brute=True)
        dirs = _camera_dirs(oracle, cam, w, h)
        what = "%s-%g %s camera" % (kind, off, cname)
        _check_float64(S64, cam["position"], dirs.reshape(-1, 3), R.RAY_TMIN, R.RAY_TMAX, ref["hit_inst"].reshape(-1),
                       ref["hit_prim"].reshape(-1), ref["hit_t"].reshape(-1), what + " primary rays")
        rays = _surface_rays(pkg, rng, sc, dict(ref, cam=cam, dirs=dirs), n=600)
        bf, _ = _check_rays_brute(oracle, S, rays, what + " surface rays")
        # (a ray leaving its own surface with tmin 0 or 1e-4 is not robust by path_reference's rule: no share required)
        _check_float64(S64, rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7], bf["inst"], bf["prim"], bf["t"],
                       what + " surface rays", min_robust=0.0)


# ---------------------------------------------------------------------------------------------------------------- GPU
GPU_CASES = [(k, off, r) for k in ("sphere", "box") for off in OFFSETS for r in RADII if not (k == "box" and r == 1.0 and off < 1e4)]
GPU_OPEN = [("slivers", 0.0, None), ("slivers", 131072.0, None), ("heightfield", 8192.0, None)]
TREES = {"sah": {"gpu_build": 0}, "lbvh": {"gpu_build": 1, "gpu_builder": 0}, "ploc": {"gpu_build": 1, "gpu_builder": 1}}


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _gpu_frames_vs_brute(renderer, oracle, S, sc, what, pipelines=(0, 1), cache=None):
    cache = {} if cache is None else cache
    for cname, cam in sc["cameras"].items():
        renderer.set_camera(cam["position"], cam["matrix"])
        for mode in (3, 100, 200):
            w, h = (W, H) if mode == 3 else (48, 48)
            if (cname, mode) not in cache:
                cache[(cname, mode)] = _render(oracle, S, cam, mode, w, h, brute=True)
            ref = cache[(cname, mode)]
            renderer.change_shading_mode(mode)
            variants = [("pipeline %d" % p, p, False) for p in pipelines] if mode == 200 else [("plain", None, False), ("counting", None, True)]
            for label, pipe, counting in variants:
                if pipe is not None:
                    renderer.set_option("path_pipeline", pipe)
                renderer.set_counting(counting)
                got = renderer.render_frame(w, h)
                renderer.set_counting(False)
                _assert_same(got, ref, "%s %s camera mode %d %s" % (what, cname, mode, label))
            renderer.set_option("path_pipeline", 0)


def _gpu_rays_vs_brute(pkg, renderer, oracle, S, sc, rng, what, cache=None):
    """camera rays and rays from surfaces through trace_rays / occluded and their device forms; the same rays through shade_rays
    and path_rays, and the camera's 48 x 48 frame through camera_rays, shade_rays, path_rays and frame_guides (its brute-force
    frames in modes 100 and 200 come from, and go to, the cache _gpu_frames_vs_brute fills)"""
    import torch
    cache = {} if cache is None else cache
    for cname, cam in sc["cameras"].items():
        w, h = 48, 48
        ref = _render(oracle, S, cam, 3, w, h, brute=True)
        dirs = _camera_dirs(oracle, cam, w, h)
        cam_rays = pkg.make_rays(np.broadcast_to(cam["position"], (w * h, 3)), dirs.reshape(-1, 3), tmin=R.RAY_TMIN, tmax=R.RAY_TMAX)
        rays = np.concatenate([cam_rays, _surface_rays(pkg, rng, sc, dict(ref, cam=cam, dirs=dirs), n=1000)])
        bf = oracle.trace_rays(S, rays, brute_force=True)
        occ = np.array([oracle.occluded(S, q[0:3], q[4:7], q[3], q[7], brute_force=True) for q in rays], bool)
        got = renderer.trace_rays(rays)
        n = len(rays)
        d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
        d_t = torch.empty(n, dtype=torch.float32, device="cuda")
        d_inst = torch.empty(n, dtype=torch.int32, device="cuda")
        d_prim = torch.empty(n, dtype=torch.int32, device="cuda")
        d_occ = torch.empty(n, dtype=torch.bool, device="cuda")
        torch.cuda.synchronize()
        renderer.trace_rays_device(n, d_rays.data_ptr(), d_t.data_ptr(), None, d_inst.data_ptr(), d_prim.data_ptr(), stats=True)
        renderer.occluded_device(n, d_rays.data_ptr(), d_occ.data_ptr(), stats=True)
        torch.cuda.synchronize()
        dev = {"t": d_t.cpu().numpy(), "inst": d_inst.cpu().numpy().view(np.uint32), "prim": d_prim.cpu().numpy().view(np.uint32)}
        for form, res, o in (("host", got, renderer.occluded(rays)), ("device", dev, d_occ.cpu().numpy())):
            tag = "%s %s camera %s" % (what, cname, form)
            for k in ("inst", "prim"):
                m = int(np.count_nonzero(res[k] != bf[k]))
                assert m == 0, "%s: trace_rays %s differs from brute force on %d of %d rays" % (tag, k, m, n)
            assert np.array_equal(_bits(res["t"]), _bits(bf["t"])), tag + ": trace_rays t"
            m = int(np.count_nonzero(o != occ))
            assert m == 0, "%s: occluded differs from brute force on %d of %d rays" % (tag, m, n)
        frames = {3: ref}
        for mode in (100, 200):
            if (cname, mode) not in cache:
                cache[(cname, mode)] = _render(oracle, S, cam, mode, w, h, brute=True)
            frames[mode] = cache[(cname, mode)]
        tag = "%s %s camera" % (what, cname)
        renderer.set_camera(cam["position"], cam["matrix"])
        world = {"oracle": oracle, "camera": (cam["position"], cam["matrix"]), "lights": sc["lights"], "O": S, "brute_force": True, "path_held": (1, 2, 77)}
        sq.frame_records_equal_frames(renderer, frames, w, h, (1, 2, 77), tag, scene=sc, cache=cache.setdefault(("shaded", cname), {}), world=world)
        sq.arbitrary_records_equal_trace(renderer, rays, bf, tag)


def _upload(renderer, sc, tree, dynamic=False):
    for k, v in TREES[tree].items():
        renderer.set_option(k, v)
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=dynamic)
    renderer.set_path_params(1, 2, 77)


@pytest.fixture
def gpu_state(renderer, oracle):
    oracle.set_path_params(1, 2, 77)
    yield
    oracle.set_path_params(4, 3, 1234)
    for k, v in (("gpu_build", 0), ("gpu_builder", 0), ("path_pipeline", 0)):
        renderer.set_option(k, v)
    renderer.set_path_params(4, 3, 1234)
    renderer.set_counting(False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,off,r", GPU_CASES + GPU_OPEN, ids=["%s-%g-r%s" % p for p in GPU_CASES + GPU_OPEN])
def test_gpu_frames_equal_brute_force(pkg, oracle, scenes, renderer, gpu_state, kind, off, r):
    sc = _scene_of(scenes, kind, off, r)
    S = _oracle_scene(oracle, sc)
    trees = ("sah", "lbvh", "ploc") if (off >= 8192.0 or kind != "sphere") else ("sah",)
    cache = {}
    for tree in trees:
        _upload(renderer, sc, tree)
        _gpu_frames_vs_brute(renderer, oracle, S, sc, "%s-%g %s" % (kind, off, tree), pipelines=(0, 1) if tree == "sah" else (1,),
                             cache=cache)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,off,r", [("sphere", 131072.0, 0.0625), ("box", 8192.0, 0.0625), ("sphere", 1024.0, 1.0),
                                        ("slivers", 8192.0, None), ("heightfield", 8192.0, None)],
                         ids=["sphere-131072", "box-8192", "sphere-1024", "slivers-8192", "heightfield-8192"])
def test_gpu_ray_queries_equal_brute_force(pkg, oracle, scenes, renderer, gpu_state, kind, off, r):
    sc = _scene_of(scenes, kind, off, r)
    S = _oracle_scene(oracle, sc)
    rng = np.random.default_rng(int(off) + 11)
    cache = {}
    for tree in TREES:
        _upload(renderer, sc, tree)
        _gpu_rays_vs_brute(pkg, renderer, oracle, S, sc, rng, "%s-%g %s" % (kind, off, tree), cache=cache)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [0, 1])
def test_gpu_translated_dynamic_mesh_equals_brute_force(pkg, oracle, scenes, renderer, gpu_state, builder):
    """an icosphere uploaded at the origin, moved to 2^13 by set_mesh_transform: after the refit and after a rebuild every
    frame, mode and ray query equals brute force over the moved vertices"""
    off, r = 8192.0, 0.0625
    moved = closed_scene(scenes, "sphere", off, r)
    at0 = dict(closed_scene(scenes, "sphere", 0.0, r), lights=moved["lights"])  # a transform moves the mesh, not the light
    renderer.set_option("gpu_builder", builder)
    _upload(renderer, at0, "sah", dynamic=True)
    renderer.set_option("gpu_builder", builder)
    m = np.float32([[1, 0, 0, off * AXES[0]], [0, 1, 0, off * AXES[1]], [0, 0, 1, off * AXES[2]]])
    renderer.set_mesh_transform(0, m)
    renderer.refit()
    xyz, _ = renderer.mesh_vertices(0)
    assert np.array_equal(_bits(xyz), _bits(moved["meshes"][0]["vertices"])), "the moved vertices are the float32 sums"
    S = _oracle_scene(oracle, moved)
    rng = np.random.default_rng(5 + builder)
    cache = {}
    for step in ("refit", "rebuild"):
        if step == "rebuild":
            renderer.rebuild()
        _gpu_frames_vs_brute(renderer, oracle, S, moved, "dynamic %s builder %d" % (step, builder), cache=cache)
        _gpu_rays_vs_brute(pkg, renderer, oracle, S, moved, rng, "dynamic %s builder %d" % (step, builder), cache=cache)
