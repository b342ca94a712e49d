"""Shading mode 120 (CRT_MODE_AMBIENT, include/crt_hip.h "ambient occlusion"): sky visibility per hit, for crt_shade_rays*,
crt_render_frame*, crt::Renderer and crt_render.

Three things hold it, each byte for byte.  The pinned mode-200 path code: with no lights, white DIFFUSE materials, a white miss
colour and an unbounded radius every sample of path_rays at max_bounces = 1 is 1 or 0 as its first bounce ray escapes or not,
summed in float64 and divided once, which is the contract's visibility.  The contract composed from existing queries: hits from
trace_rays, normal, albedo and the point lights from shade_rays in mode 100, the biased origin and the K directions from
tests/ao_reference.c, their occlusion over (0, R) from occluded(), R restated from bvh_export.  And closed forms: an open floor
sees everything, the inside of a closed box nothing, the foot of a wall half.

The scene (y up): a floor, a closed box floating above it, a tall wall and a seeded triangle soup: 216 triangles."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from ambient_checks import ref  # noqa: F401  (fixture: tests/ao_reference.c)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF
W, H = 64, 48
KS = (1, 5, 64)
RADII = (0, 50, 1000)
SEED = 777
OUTPUTS = ("rgb", "normal", "albedo", "t", "uv", "inst", "prim")
HIT_OUTPUTS = ("normal", "albedo", "t", "uv", "inst", "prim")
FRAME_OUTPUTS = ("rgba8", "hit_inst", "hit_prim", "hit_t", "rgb")
BIAS = 1e-3  # kShadowBias
LIGHTS = [((0.0, 9.0, -5.0), 300.0), ((-8.0, 6.0, 8.0), 200.0)]
SKY = (0.25, 0.5, 1.0)
WALL_X = 5.0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, keys, what):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), "%s: %s" % (what, k)


def _mesh(v, t, material):
    return {"vertices": np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3),
            "triangles": np.ascontiguousarray(t, dtype=np.uint32).reshape(-1, 3), "material_index": material, "normals": None}


def _quad(a, b, c, d, material):
    return _mesh([a, b, c, d], [[0, 1, 2], [0, 2, 3]], material)


def make_scene():
    floor = _quad((-10, 0, -10), (10, 0, -10), (10, 0, 10), (-10, 0, 10), 0)
    wall = _quad((WALL_X, 0, -9), (WALL_X, 0, 9), (WALL_X, 8, 9), (WALL_X, 8, -9), 1)
    lo, hi = np.float32([-7.0, 0.5, -7.0]), np.float32([-4.0, 3.5, -4.0])
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float32)
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    box = _mesh(corners, [t for a, b, c, d in faces for t in ((a, b, c), (a, c, d))], 2)
    rng = np.random.default_rng(120)
    centres = rng.uniform((-3.0, 0.6, 2.0), (3.0, 4.0, 8.0), size=(200, 3))
    soup_v = (centres[:, None, :] + rng.uniform(-0.4, 0.4, size=(200, 3, 3))).reshape(-1, 3)
    soup = _mesh(soup_v, np.arange(600).reshape(200, 3), 3)
    meshes = [floor, wall, box, soup]
    assert sum(len(m["triangles"]) for m in meshes) == 216
    materials = [{"albedo": (0.8, 0.7, 0.6), "type": 1}, {"albedo": (0.3, 0.9, 0.4), "type": 1},
                 {"albedo": (0.9, 0.2, 0.2), "type": 2}, {"albedo": (0.5, 0.5, 1.0), "type": 1}]  # (the box is REFLECTIVE: diffuse here)
    return meshes, materials


def make_rays():
    """1792 records from above the scene in all directions of any magnitude (those going up, or past the floor's edge, miss) and
    256 from the centre of the closed box"""
    rng = np.random.default_rng(121)
    n = 1792
    o = rng.uniform((-9.0, 5.0, -9.0), (9.0, 9.0, 9.0), size=(n, 3))
    d = rng.normal(size=(n, 3))
    d[:, 1] = np.where(rng.random(n) < 0.75, -np.abs(d[:, 1]) - 0.3, np.abs(d[:, 1]))
    d *= rng.uniform(0.25, 4.0, size=(n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n + 256, 8), dtype=np.float32)
    rays[:n, 0:3], rays[:n, 4:7] = o, d
    rays[n:, 0:3] = (-5.5, 2.0, -5.5)
    rays[n:, 4:7] = rng.normal(size=(256, 3))
    rays[:, 7] = np.inf
    return rays


# ---- the restatement (tests/ao_reference.c, loaded by tests/ambient_checks.py)

def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- CPU tier

def test_header_and_driver_name_the_mode(pkg):
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    assert "#define CRT_MODE_AMBIENT 120u" in header
    for name in ('"ao_samples"', '"ao_radius"', '"ao_sky"'):
        assert name in header, name
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "crt_render")
    assert os.path.exists(exe), "crt_render not built"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2
    for word in ("120", "--ao-samples", "--ao-radius", "--ao-sky"):
        assert word in out.stderr, "--help names " + word


def test_reference_directions_are_unit_and_above_the_surface(ref):
    """10^4 seeded (N, u1, u2).  Length: the float32 sum of squares, its root, the reciprocal and the three products each round
    once, about 1.6 units of 2^-24 relative in all, so |d| is 1 to 2 ulp of 1 (2^-23).  d . N is sqrt(1 - u1) up to such
    roundings and sqrt(1 - u1) >= 2^-12 for u1 <= 1 - 2^-24: positive."""
    rng = np.random.default_rng(122)
    n = 10000
    N = rng.normal(size=(n, 3))
    N[:100] = np.repeat(np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0]], dtype=np.float64), 25, axis=0)  # sg of either sign, N.z = 0
    N = _f32(N / np.linalg.norm(N, axis=1, keepdims=True))
    u1 = _f32(rng.integers(0, 1 << 24, size=n).astype(np.float64) * 2.0 ** -24)
    u2 = _f32(rng.integers(0, 1 << 24, size=n).astype(np.float64) * 2.0 ** -24)
    u1[:4], u2[:4] = (0.0, 1.0 - 2.0 ** -24, 0.0, 1.0 - 2.0 ** -24), (0.0, 0.0, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24)
    d = np.zeros((n, 3), dtype=np.float32)
    ref.ao_ref_bounce(n, N.ctypes.data, u1.ctypes.data, u2.ctypes.data, d.ctypes.data)
    length = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 2.0 * 2.0 ** -23, np.abs(length - 1.0).max()
    assert ((d.astype(np.float64) * N.astype(np.float64)).sum(axis=1) > 0.0).all()


@pytest.mark.parametrize("args", [["--mode", "120", "--ranks", "2"], ["--mode-at", "3:120", "--ranks", "2"]])
def test_driver_refuses_ranks_at_argument_parsing(pkg, golden_dir, args):
    """as for mode 150 (tests/test_whitted.py): exit status 2, the mode named, no usage text"""
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "crt_render")
    out = subprocess.run([exe, os.path.join(golden_dir, "dragon.crtscene")] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "120" in out.stderr and "usage" not in out.stderr, out.stderr


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _setup(r, lights=LIGHTS, white=False, miss=SKY, ks=0):
    meshes, materials = make_scene()
    if white:
        materials = [{"albedo": (1.0, 1.0, 1.0), "type": 1}] * len(materials)
    r.set_accumulation(0)
    r.set_counting(False)
    r.upload(meshes, lights, materials)
    r.set_camera((0.0, 7.0, 8.0), _camera())
    r.set_miss_color(miss)
    r.set_option("phong_ks", ks)
    r.set_option("phong_exponent", 16)
    r.set_option("seed", SEED)


def _camera():
    import math
    p = math.radians(35.0)  # columns right / up / forward; the camera looks along -forward: towards -z, 35 degrees down
    return np.float32([1, 0, 0, 0, math.cos(p), math.sin(p), 0, -math.sin(p), math.cos(p)])


def _ao(r, k, radius, sky):
    r.set_option("ao_samples", k)
    r.set_option("ao_radius", radius)
    r.set_option("ao_sky", sky)
    r.change_shading_mode(120)


def _restore(r):
    r.set_counting(False)
    for name, v in (("phong_ks", 0), ("phong_exponent", 32), ("max_bounces", 3), ("seed", 1234), ("stack_entries", 0), ("inner_min_any", -6),
                    ("ao_samples", 16), ("ao_radius", 0), ("ao_sky", 0)):
        r.set_option(name, v)
    r.set_miss_color((0.0, 1.0, 1.0))
    r.change_shading_mode(0)


def _radius(r, ref, v):
    if v == 0:
        return np.float32(10000.0)
    nodes, _, _ = r.bvh_export()
    node0 = np.ascontiguousarray(nodes[:1]).view(np.float32)[:12].copy()
    return np.float32(ref.ao_ref_radius(v, node0.ctypes.data))


def _composed(r, ref, rays, k, radius, sky, base, seed=SEED):
    """the contract from existing queries.  base: mode 100's shade_rays of the rays (counting on).  Returns rgb and the number
    of any-hit rays the composition traced"""
    n = len(rays)
    hit = np.flatnonzero(base["inst"] != MISS)
    t = _f32(r.trace_rays(rays, want=("t",))["t"][hit])
    assert np.array_equal(_bits(t), _bits(base["t"][hit]))
    N, albedo, direct = _f32(base["normal"][hit]), _f32(base["albedo"][hit]), _f32(base["rgb"][hit])
    po = np.zeros((len(hit), 3), dtype=np.float32)
    records = _f32(rays[hit])  # (held in a name: the pointer below must outlive the call)
    ref.ao_ref_origins(len(hit), records.ctypes.data, t.ctypes.data, N.ctypes.data, po.ctypes.data)
    dirs = np.zeros((len(hit), k, 3), dtype=np.float32)
    ids = np.ascontiguousarray(hit, dtype=np.uint32)
    ref.ao_ref_directions(len(hit), ids.ctypes.data, k, seed, N.ctypes.data, dirs.ctypes.data)
    R = _radius(r, ref, radius)
    probes = np.zeros((len(hit) * k, 8), dtype=np.float32)
    probes[:, 0:3] = np.repeat(po, k, axis=0)
    probes[:, 4:7] = dirs.reshape(-1, 3)
    probes[:, 7] = R
    visible = np.ascontiguousarray((~r.occluded(probes)).reshape(len(hit), k).sum(axis=1), dtype=np.uint32)
    miss = _f32(SKY)
    rgb = np.tile(miss, (n, 1))
    part = np.zeros((len(hit), 3), dtype=np.float32)
    ref.ao_ref_colour(len(hit), visible.ctypes.data, k, int(sky), albedo.ctypes.data, miss.ctypes.data, direct.ctypes.data, part.ctypes.data)
    rgb[hit] = part
    return rgb, len(hit) * k + (base["stats"]["rays_shadow"] if sky else 0), visible


@pytest.fixture(scope="module")
def lambert(renderer):
    """mode 100 on the test rays with the two lights, Phong off, counting on: computed once, never modified"""
    r = renderer
    _setup(r)
    rays = make_rays()
    r.set_counting(True)
    r.change_shading_mode(100)
    base = r.shade_rays(rays)
    _restore(r)
    for a in list(base.values()) + [rays]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    hits = int((base["inst"] != MISS).sum())
    assert 256 + 800 < hits < len(rays) - 200, "a mix of hits and misses"
    assert 0 < base["stats"]["rays_shadow"] < 2 * hits
    return rays, base


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_equal_to_path_tracing(renderer, lambert, k):
    """no lights, white DIFFUSE materials, a white miss colour, unbounded radius: path_rays with K samples and one bounce"""
    r = renderer
    rays, base = lambert
    try:
        _setup(r, lights=[], white=True, miss=(1.0, 1.0, 1.0))
        r.set_option("max_bounces", 1)
        want = r.path_rays(rays, n_samples=k, want=("rgb",))["rgb"]
        _ao(r, k, 0, 0)
        got = r.shade_rays(rays, want=("rgb",))["rgb"]
        assert np.array_equal(_bits(got), _bits(want)), "%d records differ" % np.any(_bits(got) != _bits(want), axis=1).sum()
        hit = base["inst"] != MISS
        assert np.all(got[~hit] == 1.0) and (got[hit] == 0.0).any() and (got[hit] == 1.0).any()
        if k > 1:
            assert ((got[hit] > 0.0) & (got[hit] < 1.0)).any()
    finally:
        _restore(r)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_equal_to_the_contract_composed_from_queries(renderer, ref, lambert, k):
    r = renderer
    rays, base = lambert
    try:
        _setup(r)
        seen = set()
        for radius in RADII:
            for sky in (0, 1):
                want, _, visible = _composed(r, ref, rays, k, radius, sky, base)
                _ao(r, k, radius, sky)
                got = r.shade_rays(rays)
                what = "K=%d ao_radius=%d ao_sky=%d" % (k, radius, sky)
                bad = np.flatnonzero(np.any(_bits(got["rgb"]) != _bits(want), axis=1))
                assert len(bad) == 0, "%s: %d records differ, first %d: %s, composed %s" % (what, len(bad), bad[0], got["rgb"][bad[0]], want[bad[0]])
                _same(got, base, HIT_OUTPUTS, what)
                seen.add((radius, int(visible.sum())))
        counts = dict(seen)
        assert len(seen) == len(RADII) and counts[50] > counts[1000] >= counts[0] > 0, "a shorter reach sees more: %s" % counts
    finally:
        _restore(r)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [0, 250])
def test_mode_100_underneath(renderer, lambert, ks):
    """a black sky adds nothing: rgb is mode 100's, Phong off and on; the hit outputs are mode 100's in every setting"""
    r = renderer
    rays, _ = lambert
    try:
        _setup(r, miss=(0.0, 0.0, 0.0), ks=ks)
        r.change_shading_mode(100)
        want = r.shade_rays(rays)
        assert (want["rgb"] > 0.0).any()
        for k, radius in ((1, 0), (5, 50)):
            _ao(r, k, radius, 1)
            _same(r.shade_rays(rays), want, OUTPUTS, "ks=%d K=%d" % (ks, k))
            _ao(r, k, radius, 0)
            _same(r.shade_rays(rays), want, HIT_OUTPUTS, "ks=%d K=%d grey" % (ks, k))
    finally:
        _restore(r)


def _down(x, z):
    rays = np.zeros((len(x), 8), dtype=np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2] = x, 4.5, z
    rays[:, 5], rays[:, 7] = -1.0, np.inf
    return rays


@pytest.mark.gpu
def test_closed_forms(renderer, ref):
    r = renderer
    try:
        _setup(r)
        R = float(_radius(r, ref, 50))
        assert 1.4 < R < 1.5  # the box of the scene is 20 x 8 x 20
        # an open floor: nothing within R of these points but the floor itself (box: z <= -4, soup: x >= -3.4)
        rng = np.random.default_rng(123)
        floor = _down(rng.uniform(-9.0, -5.0, 512), rng.uniform(-1.0, 9.0, 512))
        _ao(r, 64, 50, 0)
        got = r.shade_rays(floor)
        assert np.all(got["inst"] == 0) and np.all(got["rgb"] == 1.0)
        # inside the closed box, any reach that spans it
        inside = make_rays()[-256:]
        for radius in (0, 1000):
            _ao(r, 64, radius, 0)
            got = r.shade_rays(inside)
            assert np.all(got["inst"] == 2) and np.all(got["rgb"] == 0.0), radius
        # the foot of the wall: 64 points of the floor 2 x bias in front of it.  The wall reaches 7 to either side of them and 8
        # up, R is 1.47, and the soup (x <= 3.4) is farther than R: the wall hides the half of the hemisphere that leans towards
        # it, except directions within about 2 x bias / R of its plane, whose crossing lies beyond R: that moves the mean by
        # less than 0.001.  Five binomial standard deviations of 64 x 1024 draws at p = 0.5 are 5 x 0.5 / 256
        foot = _down(np.full(64, WALL_X - 2.0 * BIAS), np.linspace(-2.0, 2.0, 64))
        _ao(r, 1024, 50, 0)
        got = r.shade_rays(foot)
        assert np.all(got["inst"] == 0)
        v = got["rgb"][:, 0].astype(np.float64)
        print("foot of the wall: mean visibility %.5f (min %.4f, max %.4f)" % (v.mean(), v.min(), v.max()))
        assert abs(v.mean() - 0.5) <= 5.0 * 0.5 / 256.0, v.mean()
    finally:
        _restore(r)


@pytest.mark.gpu
def test_frames(renderer):
    r = renderer
    try:
        _setup(r)
        rays = r.camera_rays(W, H)
        r.change_shading_mode(100)
        before = [r.render_frame(W, H) for _ in range(2)][-1]
        for k, radius, sky in ((5, 0, 0), (5, 50, 1)):
            _ao(r, k, radius, sky)
            f = r.render_frame(W, H)
            q = r.shade_rays(rays, want=("rgb", "t", "inst", "prim"))
            what = "K=%d ao_radius=%d ao_sky=%d" % (k, radius, sky)
            assert np.array_equal(_bits(q["rgb"]), _bits(f["rgb"]).reshape(-1, 3)), what + ": frame rgb != shade_rays of camera_rays"
            assert np.array_equal(_bits(q["t"]), _bits(f["hit_t"]).reshape(-1)) and np.array_equal(q["inst"], f["hit_inst"].reshape(-1))
            assert np.array_equal(q["prim"], f["hit_prim"].reshape(-1))
            unorm = (np.clip(np.nan_to_num(f["rgb"], nan=0.0), 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
            assert np.array_equal(f["rgba8"][..., :3], unorm) and np.all(f["rgba8"][..., 3] == 255), what + ": rgba8"
            hit = f["hit_inst"] != MISS
            assert hit.mean() > 0.25 and (~hit).mean() > 0.02 and np.all(f["hit_t"][~hit] == np.float32(10000.0))
            assert not np.array_equal(_bits(f["rgb"]), _bits(before["rgb"]))
        r.change_shading_mode(100)
        _same(r.render_frame(W, H), before, FRAME_OUTPUTS, "mode 100 around the mode-120 frames")
    finally:
        _restore(r)


@pytest.mark.gpu
def test_scheduling_and_state(renderer, ref, lambert):
    r = renderer
    rays, base = lambert
    hits = int((base["inst"] != MISS).sum())
    try:
        _setup(r)
        for k, radius, sky in ((5, 50, 1), (64, 0, 0)):
            _ao(r, k, radius, sky)
            r.set_counting(True)
            first = r.shade_rays(rays)
            _, n_any, _ = _composed(r, ref, rays, k, radius, sky, base)
            _ao(r, k, radius, sky)
            what = "K=%d ao_sky=%d" % (k, sky)
            assert first["stats"]["rays_shadow"] == n_any and n_any >= hits * k, what
            assert first["stats"]["rays_primary"] == len(rays)
            _same(r.shade_rays(rays), first, OUTPUTS, what + " twice")
            for name, values, default in (("inner_min_any", (1, 64, -6), -6), ("stack_entries", (2, 16), 0)):
                for v in values:
                    r.set_option(name, v)
                    got = r.shade_rays(rays)
                    _same(got, first, OUTPUTS, "%s %s=%d" % (what, name, v))
                    assert got["stats"]["rays_shadow"] == n_any
                r.set_option(name, default)
            r.set_counting(False)
            got = r.shade_rays(rays)
            _same(got, first, OUTPUTS, what + " counting off")
            assert got["stats"]["rays_shadow"] == 0
            r.set_option("seed", SEED + 1)
            other = r.shade_rays(rays, want=("rgb",))
            assert not np.array_equal(_bits(other["rgb"]), _bits(first["rgb"])), what + ": another seed"
            r.set_option("seed", SEED)
            _same(r.shade_rays(rays), first, OUTPUTS, what + " the seed restored")
            # a record's id is its index: the same rays one place further on draw other directions
            shifted = r.shade_rays(np.ascontiguousarray(np.concatenate([rays[:1], rays])), want=("rgb", "t"))
            assert np.array_equal(_bits(shifted["t"][1:]), _bits(first["t"])) and not np.array_equal(_bits(shifted["rgb"][1:]), _bits(first["rgb"]))
    finally:
        _restore(r)


@pytest.mark.gpu
def test_refusals_and_an_empty_scene(pkg, renderer):
    import torch
    r = renderer
    L = pkg.lib()
    try:
        _setup(r)
        for name, v in (("ao_samples", 0), ("ao_samples", 4097), ("ao_radius", -1), ("ao_radius", 1000001), ("ao_sky", 2), ("ao_sky", -1)):
            assert L.crt_set_option(r.h, name.encode(), v) == 1, "%s = %d is CRT_EINVAL" % (name, v)
        for name, v in (("ao_samples", 1), ("ao_samples", 4096), ("ao_radius", 1000000), ("ao_sky", 1)):
            r.set_option(name, v)
        _ao(r, 5, 50, 0)
        frame = r.render_frame(W, H)
        d = torch.full((4 * W * H,), 7, dtype=torch.int32, device="cuda")
        calls = [lambda: r.render_tiles_device(W, H, 0, 1, d.data_ptr()), lambda: r.render_tiles_device(W, H, 1, 2, d.data_ptr()),
                 lambda: r.render_frames_batch_device(W, H, [d.data_ptr()]), lambda: r.render_tiles_batch_device(W, H, 0, 1, [d.data_ptr()]),
                 lambda: r.render_frame_distributed(W, H, host=True)]
        for call in calls:
            with pytest.raises(pkg.CrtError) as e:
                call()
            assert "rc=1:" in str(e.value) and "120" in str(e.value), str(e.value)
        r.synchronize()
        torch.cuda.synchronize()
        assert bool((d == 7).all().item()), "a refused call writes nothing"
        _same(r.render_frame(W, H), frame, FRAME_OUTPUTS, "mode 120 after the refusals")
        r.change_shading_mode(200)
        with pytest.raises(pkg.CrtError, match="200"):
            r.shade_rays(make_rays())
        for radius in (0, 50):
            _ao(r, 5, radius, 1)
            r.upload([], [], [])
            rays = make_rays()
            e = r.shade_rays(rays)
            assert np.all(e["inst"] == MISS) and np.array_equal(_bits(e["rgb"]), _bits(np.tile(np.float32(SKY), (len(rays), 1))))
            assert np.all(e["normal"] == 0.0) and np.all(e["albedo"] == 0.0) and np.array_equal(_bits(e["t"]), _bits(rays[:, 7]))
            f = r.render_frame(W, H)
            assert np.all(f["hit_inst"] == MISS) and np.array_equal(_bits(f["rgb"]).reshape(-1, 3), _bits(np.tile(np.float32(SKY), (W * H, 1))))
    finally:
        _restore(r)


def _read_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, size = 8, b"", None
    while at < len(raw):
        n, kind = struct.unpack(">I4s", raw[at:at + 8])
        body = raw[at + 8:at + 8 + n]
        if kind == b"IHDR":
            size = struct.unpack(">II", body[:8])
            assert body[8:] == bytes([8, 2, 0, 0, 0]), "8-bit RGB"
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    w, h = size
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert np.all(rows[:, 0] == 0), "unfiltered scanlines"
    return rows[:, 1:].reshape(h, w, 3)


@pytest.mark.gpu
def test_cpp_layer_and_driver(pkg, golden_dir, tmp_path):
    """crt::Renderer::setAmbientOcclusion and shadeRays from a small C++ program linked against libcrt_hip.so, and the frame
    crt_render writes, are the binding's"""
    exe = str(tmp_path / "ao_cpp")
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(lib_dir, "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "ao_cpp.cpp"), "-L" + lib_dir, "-lcrt_hip",
                           "-Wl,-rpath," + lib_dir, "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    path = os.path.join(golden_dir, "dragon.crtscene")
    out = str(tmp_path / "out.bin")
    subprocess.check_call([exe, path, str(W), str(H), "5", "200", "1", out], timeout=120)
    hits = np.fromfile(out, dtype=np.uint32).reshape(W * H, 14)
    scene = pkg.Scene(path)
    r = pkg.Renderer(0)  # a context of its own: the defaults crt_render and crt::Renderer start from
    try:
        r.upload_scene(scene)
        r.set_camera_from(scene)
        _ao(r, 5, 200, 1)
        want = r.shade_rays(r.camera_rays(W, H))
        assert (want["inst"] != MISS).sum() > W * H // 10
        for k, cols in (("rgb", slice(0, 3)), ("normal", slice(3, 6)), ("albedo", slice(6, 9)), ("uv", slice(10, 12))):
            assert np.array_equal(hits[:, cols], _bits(want[k])), k
        assert np.array_equal(hits[:, 9], _bits(want["t"])) and np.array_equal(hits[:, 12], want["inst"]) and np.array_equal(hits[:, 13], want["prim"])

        _ao(r, 8, 0, 0)
        frame = r.render_frame(W, H)
        grey = frame["rgba8"][frame["hit_inst"] != MISS]
        assert np.all(grey[:, 0] == grey[:, 1]) and np.all(grey[:, 1] == grey[:, 2]) and len(np.unique(grey[:, 0])) > 2
        tool = os.path.join(lib_dir, "crt_render")
        subprocess.check_call([tool, path, "--mode", "120", "--ao-samples", "8", "--png", "--size", "%dx%d" % (W, H), "--out", str(tmp_path / "f")],
                              timeout=120, stdout=subprocess.DEVNULL)
        np.testing.assert_array_equal(_read_png(str(tmp_path / "f_0.png")), frame["rgba8"][:, :, :3])
        _ao(r, 3, 100, 1)
        frame = r.render_frame(W, H)
        subprocess.check_call([tool, path, "--mode", "120", "--ao-samples", "3", "--ao-radius", "100", "--ao-sky", "--png",
                               "--size", "%dx%d" % (W, H), "--out", str(tmp_path / "g")], timeout=120, stdout=subprocess.DEVNULL)
        np.testing.assert_array_equal(_read_png(str(tmp_path / "g_0.png")), frame["rgba8"][:, :, :3])
    finally:
        r.close()
        scene.close()
