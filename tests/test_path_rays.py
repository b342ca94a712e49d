"""Path-traced ray queries (crt_path_rays*, include/crt_hip.h): the frames' mode-200 paths for caller-supplied rays.  A record
that holds a frame's jittered camera ray is that pixel's path, so a w x h oracle frame at 1 spp is the bit-exact reference of
w * h records and a 1 x 1 frame that of one arbitrary ray with id 0 (tests/path_rays_helpers.py).  Every colour comparison is
exact (float bits compared as uint32)."""
import os
import subprocess

import numpy as np
import pytest

import path_rays_helpers as H
import path_reference as R

SYMBOLS = ("crt_path_rays_device", "crt_path_rays")
MISS = 0xFFFFFFFF
EINVAL, ESTATE = 1, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, HT = 32, 24
SEED = 77
FRAME_SCENES = ("room", "mirrors", "sphere", "textured_room", "textured_glass")
FRAME_BOUNCES = (0, 1, 3)
# what the frames' paths must do over the scenes together, so that every branch of the kernel is compared (the float64
# reference's event counters): each entry is a group of counters whose sum must not be zero
EVENTS = (("mirror",), ("enter",), ("exit",), ("tir",), ("diffuse_bounce",), ("emit_direct",), ("emit_after_mirror", "emit_after_diffuse"),
          ("miss_after_bounce",), ("shadowed",), ("lit",))
HIT_OUTPUTS = ("t", "uv", "inst", "prim")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- CPU: the interface exists

def test_binding_and_library_expose_path_rays(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
    for name in ("path_rays", "path_rays_device"):
        assert callable(getattr(pkg.Renderer, name, None)), name
    assert callable(pkg.path_jitter)
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    for s in SYMBOLS:
        assert ("int %s(" % s) in header, s
    assert L.crt_abi_version() == 1


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    rays = np.zeros((4, 8), dtype=np.float32)
    rgb = np.zeros((4, 3), dtype=np.float32)
    for fn in (L.crt_path_rays, L.crt_path_rays_device):
        assert fn(None, 4, rays.ctypes.data, None, 0, 1, rgb.ctypes.data, None, None, None, None, None, None) == EINVAL
        assert fn(None, 0, None, None, 0, 1, None, None, None, None, None, None, None) == EINVAL


def test_path_jitter_is_the_reference_hash_chain(pkg):
    ids = np.array([0, 1, 2, 767, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32)
    for seed in (0, 77, 1234, 0xFFFFFFFF):
        for sample in (0, 1, 5, 2 ** 24 - 1):
            jx, jy = pkg.path_jitter(ids, sample, seed)
            st = R.rng_start(ids, np.full(len(ids), sample, np.uint32), seed)
            st, rx = R.rng_next(st)
            st, ry = R.rng_next(st)
            assert jx.dtype == np.float32 and jy.dtype == np.float32
            assert np.array_equal(jx.astype(np.float64), rx) and np.array_equal(jy.astype(np.float64), ry), (seed, sample)
            hx, hy = H.reference_jitter(R, ids, sample, seed)
            assert np.array_equal(_bits(jx), _bits(hx)) and np.array_equal(_bits(jy), _bits(hy))
    assert np.all((jx >= 0.0) & (jx < 1.0))


# ---- CPU: the restated camera ray is the oracle's

def _oracle_scene(oracle, sc, build_mode=0):
    return oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], build_mode=build_mode, textures=sc.get("textures") or ())


def test_restated_ray_dir_equals_the_oracle_at_pixel_centres(oracle, scenes):
    cam = scenes.cornell_box()["camera"]
    for i in range(W * HT):
        d = H.ray_dir_j(cam["matrix"], i % W, i // W, 0.5, 0.5, W, HT)
        assert np.array_equal(_bits(d), _bits(oracle.ray_dir(cam["matrix"], i % W, i // W, W, HT))), i


def _compare_hits(got, frame, what):
    np.testing.assert_array_equal(got["inst"], frame["hit_inst"].reshape(-1), err_msg=what)
    np.testing.assert_array_equal(got["prim"], frame["hit_prim"].reshape(-1), err_msg=what)
    assert np.array_equal(_bits(got["t"]), _bits(frame["hit_t"].reshape(-1))), what + ": t"


def test_restated_jittered_rays_hit_what_the_oracle_frame_hits(oracle, scenes):
    """the oracle's own ray query on the restated sample-0 rays reproduces the hits of its mode-200 frame: a Cornell frame, and
    64 random poses as 1 x 1 frames (pixel 0, id 0)"""
    sc = scenes.cornell_box()
    cam = sc["camera"]
    O = _oracle_scene(oracle, sc)
    try:
        oracle.set_path_params(1, 0, SEED)
        frame = O.render(cam["position"], cam["matrix"], 200, W, HT)
        _compare_hits(oracle.trace_rays(O, H.frame_records(R, cam, W, HT, 0, SEED)), frame, "frame")
        assert (frame["hit_inst"] != MISS).sum() >= 64, "the camera sees the scene"
        rng = np.random.default_rng(5)
        lo, hi = _bounds(sc)
        pos = (lo - 0.1 * (hi - lo) + rng.random((64, 3)) * 1.2 * (hi - lo)).astype(np.float32)
        rot = _rotations(rng, 64)
        got = oracle.trace_rays(O, H.pose_records(R, pos, rot, SEED))
        hits = 0
        for k in range(64):
            f = O.render(pos[k], rot[k], 200, 1, 1, n_threads=1)
            assert got["inst"][k] == f["hit_inst"][0, 0] and got["prim"][k] == f["hit_prim"][0, 0], k
            assert _bits(got["t"][k:k + 1])[0] == _bits(f["hit_t"])[0, 0], k
            hits += int(f["hit_inst"][0, 0] != MISS)
        assert hits >= 16
    finally:
        oracle.set_path_params(4, 3, 1234)
        O.close()


def _rotations(rng, n):
    rot = np.empty((n, 9), dtype=np.float32)
    for k in range(n):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        rot[k] = (q * np.sign(np.diag(r))).astype(np.float32).reshape(9)
    return rot


# ---- scenes and references (CPU, computed once, never modified)

@pytest.fixture(scope="module")
def frame_scenes(scenes):
    return {name: R.SCENES[name](scenes) for name in FRAME_SCENES}


@pytest.fixture(scope="module")
def frame_rays(frame_scenes):
    """records of the sample-0 camera rays of every frame scene; further samples are added on demand by _records"""
    return {}


def _records(frame_rays, frame_scenes, name, sample=0):
    if (name, sample) not in frame_rays:
        rays = H.frame_records(R, frame_scenes[name]["camera"], W, HT, sample, SEED)
        rays.setflags(write=False)
        frame_rays[(name, sample)] = rays
    return frame_rays[(name, sample)]


def test_the_frame_scenes_cover_every_branch(frame_scenes):
    """the float64 reference alone: over the five scenes and max_bounces 0, 1, 3 the paths of the compared frames mirror,
    enter and leave glass, reflect totally, bounce diffusely, see an emitter directly and after a bounce, miss after a bounce,
    and find lights shadowed and lit"""
    ev = {}
    for name, sc in frame_scenes.items():
        S = R.Scene(sc)
        for mb in FRAME_BOUNCES:
            ref = R.trace_paths(S, sc["camera"]["position"], sc["camera"]["matrix"], W, HT, R.MISS_RGB, mb, SEED)
            for k, v in ref["ev"].items():
                ev[k] = ev.get(k, 0) + v
    missing = [g for g in EVENTS if sum(ev.get(k, 0) for k in g) == 0]
    assert not missing, "never exercised: %s" % (missing,)


SOUP_LIGHTS = [((9.0, 16.0, 6.0), 3000.0), ((-9.0, 12.0, -4.0), 2000.0), ((0.0, -3.0, 0.0), 800.0)]
N_POSES, POSE_SEED, SOUP_BOUNCES = 256, 20, 2


def _soup(scenes):
    """test_shade_rays' icosphere soup with three lights, its spheres dealt out to four meshes of the four material types"""
    n = 400
    sc = scenes.icosphere_soup(n_spheres=n)
    ground, balls = sc["meshes"]
    v = np.asarray(balls["vertices"], dtype=np.float32).reshape(n, -1, 3)
    t = np.asarray(balls["triangles"], dtype=np.int64).reshape(n, -1, 3) - (np.arange(n) * v.shape[1])[:, None, None]
    meshes = [ground]
    for g in range(4):
        sel = np.arange(g, n, 4)
        m = dict(balls)
        m["vertices"] = v[sel].reshape(-1, 3).copy()
        m["triangles"] = (t[sel] + (np.arange(len(sel)) * v.shape[1])[:, None, None]).reshape(-1, 3).astype(np.uint32)
        m["material_index"] = 1 + g
        meshes.append(m)
    sc["meshes"] = meshes
    sc["materials"] = [{"albedo": (0.8, 0.8, 0.8), "type": R.DIFFUSE}, {"albedo": (0.6, 0.8, 0.9), "type": R.DIFFUSE},
                       {"albedo": (0.9, 0.85, 0.7), "type": R.REFLECTIVE}, {"albedo": (1.0, 1.0, 1.0), "type": R.REFRACTIVE, "ior": 1.5},
                       {"albedo": (1.5, 1.1, 0.7), "type": R.CONSTANT}]
    sc["lights"] = list(SOUP_LIGHTS)
    return sc


def _bounds(sc):
    v = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    return v.min(axis=0), v.max(axis=0)


def _pose_reference(oracle, sc, pos, rot, build_mode):
    O = _oracle_scene(oracle, sc, build_mode)
    n = len(pos)
    ref = {"rgb": np.zeros((n, 3), np.float32), "inst": np.zeros(n, np.uint32), "prim": np.zeros(n, np.uint32), "t": np.zeros(n, np.float32),
           "segments": np.zeros(n, np.uint64)}
    try:
        oracle.set_path_params(1, SOUP_BOUNCES, SEED)
        for k in range(n):
            f = O.render(pos[k], rot[k], 200, 1, 1, miss_rgb=R.MISS_RGB, n_threads=1)
            ref["rgb"][k], ref["inst"][k], ref["prim"][k], ref["t"][k] = f["rgb"][0, 0], f["hit_inst"][0, 0], f["hit_prim"][0, 0], f["hit_t"][0, 0]
            ref["segments"][k] = f["stats"]["rays_primary"]
    finally:
        oracle.set_path_params(4, 3, 1234)
        O.close()
    return ref


@pytest.fixture(scope="module")
def soup_ref(oracle, scenes):
    """the soup, 256 poses in and around it (positions a tenth of the box's extent beyond it on every side, random orthonormal
    rotations, as test_shade_rays builds its own), their sample-0 records with id 0 and the oracle's 1 x 1 mode-200 frames over
    the SAH tree (0) and the LBVH (1)"""
    sc = _soup(scenes)
    rng = np.random.default_rng(POSE_SEED)
    lo, hi = _bounds(sc)
    ext = hi - lo
    pos = (lo - 0.1 * ext + rng.random((N_POSES, 3)) * 1.2 * ext).astype(np.float32)
    rot = _rotations(rng, N_POSES)
    rays = H.pose_records(R, pos, rot, SEED)
    ref = {b: _pose_reference(oracle, sc, pos, rot, b) for b in (0, 1)}
    for v in ref.values():
        for a in v.values():
            a.setflags(write=False)
    rays.setflags(write=False)
    return {"scene": sc, "rays": rays, "ref": ref}


def test_the_poses_cover_hits_misses_and_bounces(soup_ref):
    r = soup_ref["ref"][0]
    hits = int((r["inst"] != MISS).sum())
    assert hits >= 64 and N_POSES - hits >= 64, hits
    assert (r["segments"] == 3).sum() >= 16 and (r["segments"] == 2).sum() >= 8, "paths of every length up to max_bounces + 1"
    assert len(np.unique(r["inst"][r["inst"] != MISS])) == 5, "every mesh (every material type) is seen directly"


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _upload(renderer, sc, dynamic=False):
    renderer.set_accumulation(0)
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"), dynamic=dynamic)
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])


@pytest.fixture()
def path_setup(renderer):
    """mode 200 with the reference's miss colour; everything back to the defaults afterwards"""
    renderer.set_miss_color(R.MISS_RGB)
    renderer.change_shading_mode(200)
    yield renderer
    renderer.set_accumulation(0)
    renderer.set_counting(False)
    renderer.set_path_params(4, 3, 1234)
    renderer.set_miss_color((0.0, 1.0, 1.0))
    renderer.change_shading_mode(0)
    for k, v in (("inner_min", -6), ("inner_min_any", -6), ("stack_entries", 0), ("path_pass_paths", 1 << 24)):
        renderer.set_option(k, v)


IDS = np.arange(W * HT, dtype=np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FRAME_SCENES)
def test_frame_rays_equal_the_frame(oracle, frame_scenes, frame_rays, path_setup, name):
    """the sample-0 jittered camera rays of a 1-spp frame, ids = pixel numbers: rgb equals the frame kernel's rgb_f32 and the
    oracle's bit for bit, t / inst / prim the frame's hit outputs, and the instrumented kernel counts the oracle frame's rays
    and fetches"""
    r, sc = path_setup, frame_scenes[name]
    cam = sc["camera"]
    _upload(r, sc)
    rays = _records(frame_rays, frame_scenes, name)
    O = _oracle_scene(oracle, sc)
    try:
        for mb in FRAME_BOUNCES:
            r.set_path_params(1, mb, SEED)
            oracle.set_path_params(1, mb, SEED)
            frame = r.render_frame(W, HT)
            ref = O.render(cam["position"], cam["matrix"], 200, W, HT, miss_rgb=R.MISS_RGB)
            r.set_counting(True)
            got = r.path_rays(rays, ids=IDS)
            r.set_counting(False)
            what = "%s max_bounces=%d" % (name, mb)
            for src, which in ((frame, "frame"), (ref, "oracle")):
                assert np.array_equal(_bits(got["rgb"]), _bits(src["rgb"].reshape(-1, 3))), "%s: rgb differs from the %s" % (what, which)
                _compare_hits(got, src, what)
            st, rs = got["stats"], ref["stats"]
            print(what, {k: (st[k], rs[k]) for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested")})
            assert st["kernel_ms"] > 0.0
            assert tuple(st[k] for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested")) == \
                tuple(rs[k] for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested")), what
            plain = r.path_rays(rays, ids=IDS, want=("rgb",))
            assert plain["stats"]["rays_primary"] == W * HT and np.array_equal(_bits(plain["rgb"]), _bits(got["rgb"]))
        assert (got["inst"] != MISS).sum() > W * HT // 4, "the camera sees the scene"
    finally:
        oracle.set_path_params(4, 3, 1234)
        O.close()


@pytest.mark.gpu
def test_caller_owned_accumulation(frame_scenes, frame_rays, path_setup):
    """three accumulating 1-spp frames equal three calls with that sample's jittered rays chained through one sums buffer;
    on fixed rays one call of five samples equals five single-sample calls, and without sums the mean of the five radiances"""
    r, sc = path_setup, frame_scenes["room"]
    _upload(r, sc)
    n = W * HT
    r.set_path_params(1, 3, SEED)
    r.set_accumulation(1 << 24)
    sums = np.full((n, 3), 1e30, dtype=np.float64)  # (first_sample = 0 must not read it)
    after2 = None
    for s in range(3):
        frame = r.render_frame(W, HT)
        got = r.path_rays(_records(frame_rays, frame_scenes, "room", s), ids=IDS, first_sample=s, n_samples=1, sums=sums, want=("rgb",))
        assert r.accumulated_samples() == s + 1
        assert np.array_equal(_bits(got["rgb"]), _bits(frame["rgb"].reshape(-1, 3))), "sample %d" % s
        if s == 1:
            after2 = sums.copy()
    r.set_accumulation(0)

    rays = _records(frame_rays, frame_scenes, "room")
    one, five = after2.copy(), after2.copy()
    a = r.path_rays(rays, ids=IDS, first_sample=2, n_samples=5, sums=one, want=("rgb",))
    singles = []
    for s in range(2, 7):
        b = r.path_rays(rays, ids=IDS, first_sample=s, n_samples=1, sums=five, want=("rgb",))
        singles.append(r.path_rays(rays, ids=IDS, first_sample=s, n_samples=1, want=("rgb",))["rgb"])
    assert np.array_equal(one.view(np.uint64), five.view(np.uint64)) and np.array_equal(_bits(a["rgb"]), _bits(b["rgb"]))
    assert not np.array_equal(one.view(np.uint64), after2.view(np.uint64))
    total = np.zeros((n, 3), dtype=np.float64)
    for x in singles:
        total = total + x.astype(np.float64)
    mean = r.path_rays(rays, ids=IDS, first_sample=2, n_samples=5, want=("rgb",))["rgb"]
    assert np.array_equal(_bits(mean), _bits((total / 5.0).astype(np.float32)))
    assert len({x.tobytes() for x in singles}) == 5, "every sample is another path"


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_build", [0, 1])
def test_arbitrary_rays_equal_the_oracle(soup_ref, path_setup, gpu_build):
    """256 poses in and around the soup (four material types, three lights), max_bounces 2, all ids 0: each record equals its
    1 x 1 oracle frame bit for bit, in either buffer order and over either tree"""
    r = path_setup
    sc, rays, ref = soup_ref["scene"], soup_ref["rays"], soup_ref["ref"][gpu_build]
    try:
        r.set_option("gpu_build", gpu_build)
        _upload(r, sc)
    finally:
        r.set_option("gpu_build", 0)
    r.set_path_params(1, SOUP_BOUNCES, SEED)
    zeros = np.zeros(N_POSES, dtype=np.uint32)
    for order in (np.arange(N_POSES), np.arange(N_POSES)[::-1]):
        got = r.path_rays(np.ascontiguousarray(rays[order]), ids=zeros)
        assert np.array_equal(_bits(got["rgb"]), _bits(ref["rgb"][order]))
        np.testing.assert_array_equal(got["inst"], ref["inst"][order])
        np.testing.assert_array_equal(got["prim"], ref["prim"][order])
        assert np.array_equal(_bits(got["t"]), _bits(ref["t"][order]))


@pytest.mark.gpu
def test_ids(frame_scenes, frame_rays, path_setup):
    r, sc = path_setup, frame_scenes["room"]
    _upload(r, sc)
    r.set_path_params(1, 3, SEED)
    rays = _records(frame_rays, frame_scenes, "room")
    base = r.path_rays(rays, ids=IDS, n_samples=2)
    perm = np.random.default_rng(3).permutation(W * HT)
    got = r.path_rays(np.ascontiguousarray(rays[perm]), ids=IDS[perm], n_samples=2)
    for k in ("rgb",) + HIT_OUTPUTS:
        assert np.array_equal(got[k].view(np.uint32), base[k][perm].view(np.uint32)), k
    none = r.path_rays(rays, n_samples=2)
    assert np.array_equal(_bits(none["rgb"]), _bits(base["rgb"]))
    other = r.path_rays(rays, ids=IDS + np.uint32(100000), n_samples=2)
    for k in HIT_OUTPUTS:
        assert np.array_equal(other[k].view(np.uint32), base[k].view(np.uint32)), k
    assert np.any(_bits(other["rgb"]) != _bits(base["rgb"])), "another id is another sample"


@pytest.mark.gpu
def test_sizes_and_passes(soup_ref, path_setup):
    """partial wavefronts, and 4099 records x 17 samples = 69 683 items cut into passes of at most 65 536: the same results as
    in one pass, with and without sums, and as the chained single-sample calls"""
    r = path_setup
    _upload(r, soup_ref["scene"])
    r.set_path_params(1, SOUP_BOUNCES, SEED)
    ref = soup_ref["ref"][0]
    zeros = np.zeros(N_POSES, dtype=np.uint32)
    for n in (1, 63, 65, 200):
        got = r.path_rays(np.ascontiguousarray(soup_ref["rays"][:n]), ids=zeros[:n])
        assert np.array_equal(_bits(got["rgb"]), _bits(ref["rgb"][:n])), n
        np.testing.assert_array_equal(got["prim"], ref["prim"][:n])
        assert got["stats"]["rays_primary"] == n

    n, S = 4099, 17
    rays = np.ascontiguousarray(soup_ref["rays"][np.arange(n) % N_POSES])
    ids = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(3)
    runs = {}
    for cap in (1 << 24, 1 << 16):
        r.set_option("path_pass_paths", cap)
        sums = np.zeros((n, 3), dtype=np.float64)
        runs[cap] = (r.path_rays(rays, ids=ids, n_samples=S), r.path_rays(rays, ids=ids, n_samples=S, sums=sums), sums)
        assert runs[cap][0]["stats"]["rays_primary"] == n * S
    r.set_option("path_pass_paths", 1 << 24)
    one, cut = runs[1 << 24], runs[1 << 16]
    for k in ("rgb",) + HIT_OUTPUTS:
        for i in (0, 1):
            assert np.array_equal(one[i][k].view(np.uint32), cut[i][k].view(np.uint32)), (k, i)
    assert np.array_equal(one[2].view(np.uint64), cut[2].view(np.uint64))
    assert np.array_equal(_bits(one[0]["rgb"]), _bits(one[1]["rgb"])), "first_sample = 0: the same mean with and without sums"
    m = 64
    chained = np.zeros((m, 3), dtype=np.float64)
    for s in range(S):
        last = r.path_rays(rays[:m], ids=ids[:m], first_sample=s, n_samples=1, sums=chained, want=("rgb",))
    assert np.array_equal(chained.view(np.uint64), cut[2][:m].view(np.uint64))
    assert np.array_equal(_bits(last["rgb"]), _bits(cut[0]["rgb"][:m]))
    # one record at many samples: 4096 items of one ray, in one pass
    many = r.path_rays(rays[:1], ids=ids[:1], n_samples=4096, sums=np.zeros((1, 3)))
    assert many["stats"]["rays_primary"] == 4096 and np.all(np.isfinite(many["rgb"]))


def _scaled(rays, k):
    out = rays.copy()
    out[:, 4:7] = np.ldexp(rays[:, 4:7], k)
    out[:, 3] = np.ldexp(rays[:, 3], -k)
    out[:, 7] = np.ldexp(rays[:, 7], -k)
    return out


@pytest.mark.gpu
def test_records(pkg, soup_ref, path_setup):
    r = path_setup
    _upload(r, soup_ref["scene"])
    r.set_path_params(1, SOUP_BOUNCES, SEED)
    rays = np.array(soup_ref["rays"])
    miss = np.float32(R.MISS_RGB)
    hitting = rays[np.flatnonzero(soup_ref["ref"][0]["inst"] != MISS)[0]]
    bad = []
    for f in range(8):
        x = hitting.copy()
        x[f] = np.nan
        bad.append(x)
    for tmin, tmax in ((1.0, 1.0), (2.0, 1.0), (np.inf, np.inf)):
        x = hitting.copy()
        x[3], x[7] = tmin, tmax
        bad.append(x)
    x = hitting.copy()
    x[4:7] = 0.0
    bad.append(x)
    nb = len(bad)
    negative = rays[:32].copy()
    negative[:, 3] = -5.0
    buf = np.concatenate([np.stack(bad), hitting[None], _scaled(rays[:64], 20), _scaled(rays[64:128], -20), negative]).astype(np.float32)
    got = r.path_rays(buf, n_samples=3)
    hit = r.trace_rays(buf)
    for k in HIT_OUTPUTS:
        assert np.array_equal(got[k].view(np.uint32), hit[k].view(np.uint32)), k
    assert np.all(got["inst"][:nb] == MISS) and np.all(got["prim"][:nb] == MISS) and np.all(got["uv"][:nb] == 0.0)
    assert np.array_equal(_bits(got["rgb"][:nb]), _bits(np.tile(miss, (nb, 1))))
    assert np.array_equal(_bits(got["t"][:nb]), _bits(buf[:nb, 7]))
    assert got["inst"][nb] != MISS and (got["inst"][nb + 1:] != MISS).sum() >= 32

    # n = 0: OK, nothing launched, NULL buffers allowed
    e = r.path_rays(np.zeros((0, 8), dtype=np.float32))
    assert all(len(e[k]) == 0 for k in ("rgb",) + HIT_OUTPUTS) and e["stats"]["rays_primary"] == 0
    assert pkg.lib().crt_path_rays_device(r.h, 0, None, None, 0, 1, None, None, None, None, None, None, None) == 0

    # an empty scene: every record misses
    r.upload([], [], [])
    e = r.path_rays(rays, n_samples=2)
    assert np.all(e["inst"] == MISS) and np.array_equal(_bits(e["rgb"]), _bits(np.tile(miss, (len(rays), 1))))
    assert np.array_equal(_bits(e["t"]), _bits(rays[:, 7]))


@pytest.mark.gpu
def test_options_change_nothing(soup_ref, path_setup):
    """other scheduling thresholds, a one-entry LDS stack (deeper entries go to the spill arena) and counting: every output
    and every counter are those of the default options"""
    r = path_setup
    _upload(r, soup_ref["scene"])
    r.set_path_params(1, SOUP_BOUNCES, SEED)
    n = 1000
    rays = np.ascontiguousarray(soup_ref["rays"][np.arange(n) % N_POSES])
    ids = np.arange(n, dtype=np.uint32)
    counters = ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested")
    plain = r.path_rays(rays, ids=ids, n_samples=2)
    r.set_counting(True)
    base = r.path_rays(rays, ids=ids, n_samples=2)
    assert all(base["stats"][k] > 0 for k in counters) and base["stats"]["rays_primary"] > 2 * n
    for k in ("rgb",) + HIT_OUTPUTS:
        assert np.array_equal(plain[k].view(np.uint32), base[k].view(np.uint32)), "counting: " + k
    for name, value, default in (("inner_min", 3, -6), ("inner_min_any", 40, -6), ("inner_min_any", -2, -6), ("stack_entries", 1, 0)):
        r.set_option(name, value)
        got = r.path_rays(rays, ids=ids, n_samples=2)
        r.set_option(name, default)
        for k in ("rgb",) + HIT_OUTPUTS:
            assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), "%s=%d: %s" % (name, value, k)
        for k in counters:
            assert got["stats"][k] == base["stats"][k], "%s=%d: %s" % (name, value, k)


@pytest.mark.gpu
def test_no_interference_with_frames(scenes, path_setup):
    """an accumulating mode-200 run with calls between its frames equals the run without them; the mode and the camera stay;
    a pending vertex update is applied by the call itself"""
    r = path_setup
    sc, w, h, S, K = scenes.cornell_box(), 32, 24, 2, 3
    _upload(r, sc, dynamic=True)
    cam = sc["camera"]
    rays = H.frame_records(R, cam, w, h, 0, 1234)
    ids = np.arange(w * h, dtype=np.uint32)
    runs = []
    for query in (False, True):
        r.change_shading_mode(200)
        r.set_path_params(S, 3, 1234)
        r.set_accumulation(1 << 24)
        for i in range(K):
            frame = r.render_frame(w, h)
            if query:
                r.path_rays(rays, ids=ids, n_samples=3)
            assert r.accumulated_samples() == (i + 1) * S
        runs.append(frame)
        r.set_accumulation(0)
    np.testing.assert_array_equal(runs[0]["rgba8"], runs[1]["rgba8"])
    assert np.array_equal(_bits(runs[0]["rgb"]), _bits(runs[1]["rgb"]))

    # the mode is not read and not changed: the same radiance in mode 3, and the next frame is a mode-3 frame
    r.set_path_params(1, 3, 1234)
    in200 = r.path_rays(rays, ids=ids)
    r.change_shading_mode(3)
    before = r.render_frame(w, h)
    in3 = r.path_rays(rays, ids=ids)
    after = r.render_frame(w, h)
    assert np.array_equal(_bits(in3["rgb"]), _bits(in200["rgb"]))
    assert np.array_equal(_bits(before["rgb"]), _bits(after["rgb"]))
    np.testing.assert_array_equal(before["hit_prim"], after["hit_prim"])

    # dynamic scene: the pending update is applied by the query itself
    r.change_shading_mode(200)
    v = np.asarray(sc["meshes"][4]["vertices"], dtype=np.float32).reshape(-1, 3) + np.float32([0.7, 0.0, 0.9])
    r.update_vertices(4, v)
    got = r.path_rays(rays, ids=ids)
    frame = r.render_frame(w, h)
    assert np.array_equal(_bits(got["rgb"]), _bits(frame["rgb"].reshape(-1, 3)))
    np.testing.assert_array_equal(got["prim"], frame["hit_prim"].reshape(-1))
    assert not np.array_equal(_bits(got["rgb"]), _bits(in200["rgb"])), "the mesh moved"


@pytest.mark.gpu
def test_errors_and_device_form(pkg, soup_ref, path_setup):
    import torch
    L = pkg.lib()
    r = path_setup
    _upload(r, soup_ref["scene"])
    r.set_path_params(1, SOUP_BOUNCES, SEED)
    rays = np.array(soup_ref["rays"])
    n = len(rays)
    ref = soup_ref["ref"][0]
    d_rays = torch.from_numpy(np.concatenate([rays.reshape(-1), np.zeros(8, np.float32)])).cuda()
    d_ids = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    sentinel = 12345.0
    d_out = torch.full((3 * n + 8,), sentinel, dtype=torch.float32, device="cuda")
    d_sums = torch.full((3 * n + 2,), sentinel, dtype=torch.float64, device="cuda")
    rgb = np.full((n, 3), sentinel, dtype=np.float32)

    def untouched():
        torch.cuda.synchronize()
        return bool((d_out == sentinel).all().item()) and bool((d_sums == sentinel).all().item()) and bool(np.all(rgb == sentinel))
    P, Rp, I, S = d_out.data_ptr(), d_rays.data_ptr(), d_ids.data_ptr(), d_sums.data_ptr()
    dev, host = L.crt_path_rays_device, L.crt_path_rays
    assert dev(r.h, n, Rp, None, 0, 1, None, None, None, None, None, None, None) == EINVAL          # every output NULL
    assert host(r.h, n, rays.ctypes.data, None, 0, 1, None, None, None, None, None, None, None) == EINVAL
    assert dev(r.h, n, None, None, 0, 1, P, None, None, None, None, None, None) == EINVAL           # NULL rays
    assert host(r.h, n, None, None, 0, 1, rgb.ctypes.data, None, None, None, None, None, None) == EINVAL
    assert dev(r.h, n, Rp, None, 0, 0, P, None, None, None, None, None, None) == EINVAL             # n_samples = 0
    assert host(r.h, n, rays.ctypes.data, None, 0, 0, rgb.ctypes.data, None, None, None, None, None, None) == EINVAL
    assert dev(r.h, n, Rp, None, (1 << 24) - 1, 2, P, None, None, None, None, None, None) == EINVAL  # past 2^24 samples
    assert host(r.h, n, rays.ctypes.data, None, 1 << 24, 1, rgb.ctypes.data, None, None, None, None, None, None) == EINVAL
    assert "2^24" in L.crt_last_error(r.h).decode()
    assert dev(r.h, n, Rp + 4, None, 0, 1, P, None, None, None, None, None, None) == EINVAL         # rays: 16 bytes
    assert dev(r.h, n, Rp + 8, None, 0, 1, P, None, None, None, None, None, None) == EINVAL
    assert dev(r.h, n, Rp, I + 2, 0, 1, P, None, None, None, None, None, None) == EINVAL            # ids: 4
    assert dev(r.h, n, Rp, None, 0, 1, P, S + 4, None, None, None, None, None) == EINVAL            # sums: 8
    for slot in range(6):  # rgb, sums, t, uv, inst, prim
        args = [None] * 6
        args[slot] = P + 2
        assert dev(r.h, n, Rp, None, 0, 1, *args, None) == EINVAL, slot
    assert dev(r.h, n, Rp, None, 0, 1, P, None, None, P + 4, None, None, None) == EINVAL            # uv: 8
    assert "aligned" in L.crt_last_error(r.h).decode()
    assert untouched()

    # the control: the same buffers, properly aligned, on torch's current stream
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            r.path_rays_device(n, Rp, d_ids=I, d_rgb=P, d_sums=S)
            first = d_out[:3 * n].clone()
            r.path_rays_device(n, Rp, d_ids=I, first_sample=1, n_samples=2, d_rgb=P, d_sums=S)
        finally:
            r.reset_stream()
    stream.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(first.cpu().numpy().reshape(n, 3)), _bits(ref["rgb"]))
    want = r.path_rays(rays, ids=np.zeros(n, np.uint32), n_samples=3)
    assert np.array_equal(_bits(d_out[:3 * n].cpu().numpy().reshape(n, 3)), _bits(want["rgb"]))
    assert bool((d_out[3 * n:] == sentinel).all().item()) and bool((d_sums[3 * n:] == sentinel).all().item())
    st = r.path_rays_device(n, Rp, d_ids=I, d_t=P, stats=True)
    torch.cuda.synchronize()
    assert st["rays_primary"] == n and np.array_equal(_bits(d_out[:n].cpu().numpy()), _bits(ref["t"]))

    fresh = pkg.Renderer(0)
    try:
        assert host(fresh.h, n, rays.ctypes.data, None, 0, 1, rgb.ctypes.data, None, None, None, None, None, None) == ESTATE
        assert dev(fresh.h, n, Rp, None, 0, 1, P, None, None, None, None, None, None) == ESTATE
        with pytest.raises(pkg.CrtError):
            fresh.path_rays(rays)
    finally:
        fresh.close()
    assert np.all(rgb == sentinel)


@pytest.mark.gpu
def test_cpp_layer(pkg, scenes, path_setup, tmp_path):
    """crt::Renderer::pathRays, from a small C++ program linked against libcrt_hip.so, agrees with the Python host path: one
    call, and two calls chained through a sums buffer"""
    r = path_setup
    exe = str(tmp_path / "path_rays_cpp")
    csrc = os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + csrc,
                           "-o", exe, os.path.join(ROOT, "tests", "path_rays_cpp.cpp"), "-L" + os.path.dirname(pkg.LIB_PATH), "-lcrt_hip",
                           "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH), "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    sc = scenes.cornell_box()
    scene = pkg.Scene.from_arrays(sc)
    path = str(tmp_path / "cornell.crtbin")
    scene.save(path)
    rays = H.frame_records(R, sc["camera"], W, HT, 0, SEED)
    rays.tofile(str(tmp_path / "rays.bin"))
    r.upload_scene(scene)
    r.set_miss_color((0.0, 1.0, 1.0))  # the C++ layer's default
    r.set_path_params(1, 2, SEED)
    for first, samples in ((0, 1), (0, 4), (3, 2)):
        out = str(tmp_path / ("paths_%d_%d.bin" % (first, samples)))
        subprocess.check_call([exe, path, str(tmp_path / "rays.bin"), str(first), str(samples), "2", str(SEED), out], timeout=120)
        raw = np.fromfile(out, dtype=np.uint32).reshape(len(rays), 8)
        sums = np.zeros((len(rays), 3)) if first == 0 and samples > 1 else None
        ref = r.path_rays(rays, first_sample=first, n_samples=samples, sums=sums)
        assert np.array_equal(raw[:, 0:3], _bits(ref["rgb"])), (first, samples)
        assert np.array_equal(raw[:, 3], _bits(ref["t"])) and np.array_equal(raw[:, 4:6], _bits(ref["uv"]))
        assert np.array_equal(raw[:, 6], ref["inst"]) and np.array_equal(raw[:, 7], ref["prim"])
    assert (ref["inst"] != MISS).sum() >= 64 and np.any(ref["rgb"][ref["inst"] != MISS] > 0.0), "the camera sees the scene"
    scene.close()
