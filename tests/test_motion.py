"""Temporal reprojection for moving meshes (include/crt_hip.h, "motion"): crt_motion_snapshot keeps the previous world vertices of a
dynamic scene, crt_previous_points* / crt_frame_motion* evaluate them at hits, crt_temporal_accumulate_motion* reprojects a moved
pixel from where its surface element was.

tests/motion_reference.c restates the previous-point formula and the temporal contract with steps 4', 5', 7' and 9' in plain C
(compiled here with -O2 -ffp-contract=off -fno-fast-math).  On the CPU the reference is pinned to what it means on an analytic scene
(a floor, a back wall and a quad in front of the wall that approaches the camera or slides in its own plane); on the GPU the
kernels equal the reference bit for bit.

Figures observed on the CPU (96 x 64, 8 frames): approach -- 168 interior pixels in the last frame, len = 1 without prev_point, len
= k + 1 within 1.4e-7 k with it; slide -- RMSE against the noise-free last frame over 31 interior pixels: with motion 0.1298,
without motion 0.2800, the raw last frame 0.1502; disocclusion -- 2 floor and 10 wall pixels uncovered.  The pipeline's figures are
in test_pipeline's docstring and DESIGN.md 5i."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("crt_motion_snapshot", "crt_previous_points_device", "crt_previous_points", "crt_frame_motion_device", "crt_frame_motion",
           "crt_temporal_accumulate_motion_device", "crt_temporal_accumulate_motion")
METHODS = ("motion_snapshot", "previous_points", "previous_points_device", "frame_motion", "frame_motion_device")
EINVAL, ESTATE = 1, 5
MISS = 0xFFFFFFFF
QNAN_BITS = 0x7FC00000
T_MISS = np.float32(10000.0)
DEFAULTS = {"alpha": 0.1, "depth_tolerance": 0.01, "normal_threshold": 0.9, "max_history": 64, "demodulate": 1}
FRAMES = 8
APPROACH = 0.95  # the quad's distance shrinks by 5 % per frame: five times the default depth_tolerance


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rmse(a, b):
    return float(np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean()))


# ---- the references (tests/motion_reference.c, tests/temporal_reference.c)

def _compile(tmp, name):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for tests/%s.c" % name)
    out = str(tmp / ("lib%s.so" % name))
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(ROOT, "tests", name + ".c"),
                           "-o", out, "-lm"])
    return C.CDLL(out)


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("motion_reference")
    L = _compile(tmp, "motion_reference")
    L.motion_temporal_reference.restype = None
    L.motion_temporal_reference.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 12 + [C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32]
    L.previous_points_reference.restype = None
    L.previous_points_reference.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 9
    P = _compile(tmp, "temporal_reference")
    P.temporal_reference.restype = None
    P.temporal_reference.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 11 + [C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32]
    L.plain = P
    return L


def reference(L, cam_cur, cam_prev, dir_cur, dir_prev, frame, hist_prev=None, prev_point=None, plain=False, **params):
    """one call of motion_temporal_reference (plain: of temporal_reference, which takes no prev_point): (hist_next, out)"""
    prm = dict(DEFAULTS, **params)
    h, w = frame["t"].shape
    a = {k: np.ascontiguousarray(frame[k], dtype=np.float32) for k in ("rgb", "normal", "albedo", "t")}
    cc, cp = np.ascontiguousarray(cam_cur, np.float32), np.ascontiguousarray(cam_prev, np.float32)
    dc, dp = np.ascontiguousarray(dir_cur, np.float32), np.ascontiguousarray(dir_prev, np.float32)
    assert cc.size == 12 and cp.size == 12 and dc.size == 3 * w * h and dp.size == 3 * w * h
    hp = None if hist_prev is None else np.ascontiguousarray(hist_prev, np.float32)
    pp = None if prev_point is None else np.ascontiguousarray(prev_point, np.float32)
    assert pp is None or pp.size == 3 * w * h
    hist = np.zeros((h, w, 8), np.float32)
    out = np.zeros((h, w, 3), np.float32)
    head = [w, h, cc.ctypes.data, cp.ctypes.data, dc.ctypes.data, dp.ctypes.data, a["rgb"].ctypes.data, a["normal"].ctypes.data,
            a["albedo"].ctypes.data if prm["demodulate"] else None, a["t"].ctypes.data]
    tail = [None if hp is None else hp.ctypes.data, hist.ctypes.data, out.ctypes.data, prm["alpha"], prm["depth_tolerance"],
            prm["normal_threshold"], prm["max_history"], prm["demodulate"]]
    if plain:
        assert pp is None
        L.plain.temporal_reference(*(head + tail))
    else:
        L.motion_temporal_reference(*(head + [None if pp is None else pp.ctypes.data] + tail))
    return hist, out


def previous_points_reference(L, meshes_now, meshes_prev, inst, prim, uv):
    """previous_points_reference over lists of (vertices, triangles); meshes_prev None = no snapshot"""
    tri_start = np.cumsum([0] + [len(t) for _, t in meshes_now]).astype(np.uint32)
    vert_start = np.cumsum([0] + [len(v) for v, _ in meshes_now]).astype(np.uint32)
    world = np.ascontiguousarray(np.concatenate([v for v, _ in meshes_now]), np.float32)
    prev = None if meshes_prev is None else np.ascontiguousarray(np.concatenate([v for v, _ in meshes_prev]), np.float32)
    idx = np.ascontiguousarray(np.concatenate([t for _, t in meshes_now]), np.uint32)
    inst, prim = np.ascontiguousarray(inst, np.uint32), np.ascontiguousarray(prim, np.uint32)
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    out = np.zeros((len(inst), 3), np.float32)
    L.previous_points_reference(len(inst), len(meshes_now), tri_start.ctypes.data, vert_start.ctypes.data, world.ctypes.data,
                                None if prev is None else prev.ctypes.data, idx.ctypes.data, inst.ctypes.data, prim.ctypes.data, uv.ctypes.data,
                                out.ctypes.data)
    return out


# ---- the analytic scene: floor y = -1, back wall z = -8, and a quad facing the camera at z = qz, |x - qx| < QUAD_HALF, y < QUAD_TOP

FLOOR_Y, WALL_Z, QUAD_HALF, QUAD_TOP = -1.0, -8.0, 1.5, 1.7
W0, H0 = 96, 64
POS_A = (0.0, 0.6, 2.0)
POS_B = (0.15, 0.6, 2.05)


def camera(pos, rot):
    return np.concatenate([np.asarray(pos, np.float32).reshape(3), np.asarray(rot, np.float32).reshape(9)])


def irradiance(P):
    return 0.55 + 0.2 * np.sin(0.7 * P[..., 0]) * np.cos(0.5 * P[..., 2]) + 0.05 * P[..., 1]


def albedo_at(P):
    return np.stack([0.6 + 0.3 * np.sin(2.0 * P[..., 0]), 0.5 + 0.2 * np.cos(1.5 * P[..., 1]), 0.6 + 0.3 * np.cos(3.0 * P[..., 2])], axis=-1)


def checker(Q):
    """a checker of unit cells in the quad's own coordinates"""
    return np.where((np.floor(Q[..., 0]) + np.floor(Q[..., 1])) % 2 == 0, 0.9, 0.2)


def cast(o, dirs, w, h, qx=0.5, qz=-5.0):
    """the analytic scene along the rays o + t d (float64): surface id (0 floor, 1 wall, 2 quad), t, world point, normal, hit"""
    o = np.asarray(o, np.float64)
    d = np.asarray(dirs, np.float64).reshape(h, w, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        tf = np.where(d[..., 1] < 0, (FLOOR_Y - o[1]) / d[..., 1], np.inf)
        tw = np.where(d[..., 2] < 0, (WALL_Z - o[2]) / d[..., 2], np.inf)
        tq = np.where(d[..., 2] < 0, (qz - o[2]) / d[..., 2], np.inf)
    Pq = o + d * np.where(np.isfinite(tq), tq, 0.0)[..., None]
    tq = np.where((np.abs(Pq[..., 0] - qx) < QUAD_HALF) & (Pq[..., 1] < QUAD_TOP) & (tq > 0), tq, np.inf)
    tf = np.where(tf > 0, tf, np.inf)
    tw = np.where(tw > 0, tw, np.inf)
    ts = np.stack([tf, tw, tq], axis=-1)
    sid = ts.argmin(axis=-1)
    t = ts.min(axis=-1)
    hit = np.isfinite(t)
    P = o + d * np.where(hit, t, 0.0)[..., None]
    n = np.where((sid == 0)[..., None], np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]))
    return sid, t, P, n, hit


def make_frame(o, dirs, w, h, seed=None, noise=0.1, qx=0.5, qz=-5.0, textured=False):
    """a frame of the analytic scene: rgb = albedo(P) irradiance(P) (+ uniform noise of that amplitude).  textured: the quad's
    colour is a checker fixed to the quad (a function of the point's place on it), everything else as before"""
    sid, t, P, n, hit = cast(o, dirs, w, h, qx, qz)
    alb = albedo_at(P)
    clean = alb * irradiance(P)[..., None]
    if textured:
        local = P - np.array([qx, 0.0, qz])
        clean = np.where((sid == 2)[..., None], checker(local)[..., None] * np.ones(3), clean)
    rgb = clean.copy()
    if seed is not None:
        rgb += np.random.default_rng(seed).uniform(-noise, noise, size=rgb.shape)
    f = {"rgb": np.where(hit[..., None], rgb, 0.25).astype(np.float32), "normal": np.where(hit[..., None], n, 0.0).astype(np.float32),
         "albedo": np.where(hit[..., None], alb, 0.0).astype(np.float32), "t": np.where(hit, t, T_MISS).astype(np.float32)}
    f.update(clean=clean, P=P, sid=sid, hit=hit)
    return f


def quad_prev_points(f, shift):
    """the exact previous points of a frame whose quad moved by `shift` since the last one: P - shift on the quad, NaN elsewhere"""
    pp = np.full(f["P"].shape, np.nan, np.float32)
    on = f["sid"] == 2
    pp[on] = (f["P"][on] - np.asarray(shift, np.float64)).astype(np.float32)
    return pp


def poison(f):
    """a miss block, one NaN colour and one NaN normal, wherever the frame has room for them"""
    h, w = f["t"].shape
    if w >= 8 and h >= 4:
        f["rgb"][1:3, 2:5] = (0.0, 1.0, 1.0)
        f["normal"][1:3, 2:5] = 0.0
        f["albedo"][1:3, 2:5] = 0.0
        f["t"][1:3, 2:5] = T_MISS
    if w * h >= 16:
        i, j = np.unravel_index((w * h) // 2, (h, w)), np.unravel_index((w * h) // 2 + 3, (h, w))
        f["rgb"][i][1] = np.nan
        f["normal"][j][2] = np.nan


def oracle_dirs(oracle, rot, w, h):
    return np.array([oracle.ray_dir(rot, px, py, w, h) for py in range(h) for px in range(w)], np.float32)


@pytest.fixture(scope="module")
def views(oracle, scenes):
    """the cameras of the CPU tests with their oracle directions at 96 x 64: A, and B = A translated by (0.15, 0, 0.05) and yawed
    2 degrees"""
    v = {}
    for name, pos, yaw in (("A", POS_A, 0.0), ("B", POS_B, 2.0)):
        rot = scenes.camera_matrix(yaw, 0.0)
        dirs = oracle_dirs(oracle, rot, W0, H0)
        dirs.setflags(write=False)
        v[name] = {"pos": pos, "cam": camera(pos, rot), "dirs": dirs}
    return v


def _project(P, cam_prev, w, h):
    """float64 screen position of world points in the previous camera (the header's steps 5 and 6)"""
    o, R = cam_prev[:3].astype(np.float64), cam_prev[3:].astype(np.float64).reshape(3, 3)
    pc = (P - o) @ R
    s = -pc[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        fx = ((pc[..., 0] / s) / (w / h) + 1) * 0.5 * w - 0.5
        fy = (1 - pc[..., 1] / s) * 0.5 * h - 0.5
    return fx, fy, s


def interior_mask(prev_point, on_now, inside_prev, cam_prev, w, h):
    """the pixels of on_now (h, w bool) whose previous point (float64 projection into cam_prev) has all four bilinear taps inside the
    image and inside the mask inside_prev of the previous frame"""
    fx, fy, s = _project(np.asarray(prev_point, np.float64), cam_prev, w, h)
    ok = on_now & np.isfinite(fx) & np.isfinite(fy) & (s > 0)
    x0 = np.floor(np.where(ok, fx, 0)).astype(int)
    y0 = np.floor(np.where(ok, fy, 0)).astype(int)
    ok &= (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
    xs, ys = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    for dy in (0, 1):
        for dx in (0, 1):
            ok &= inside_prev[ys + dy, xs + dx]
    return ok


# ---- CPU: the interface

def test_header_binding_and_library_expose_the_motion_entry_points(pkg):
    L = pkg.lib()
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
        assert ("int %s(" % s) in header, s
    for step in ("4'.", "5'.", "7'.", "9'."):
        assert step in header, step
    for name in METHODS:
        assert callable(getattr(pkg.Renderer, name, None)), name
    import inspect
    assert "prev_point" in inspect.signature(pkg.Renderer.temporal_accumulate).parameters
    assert "d_prev_point" in inspect.signature(pkg.Renderer.temporal_accumulate_device).parameters
    assert "prev_point" in inspect.signature(pkg.TemporalHistory.push).parameters
    buf = np.zeros(64, dtype=np.float32)
    hist = np.zeros(64, dtype=np.float32)
    ids = np.zeros(16, dtype=np.uint32)
    cam = np.zeros(12, dtype=np.float32)
    P, Hn, K, I = buf.ctypes.data, hist.ctypes.data, cam.ctypes.data, ids.ctypes.data
    assert L.crt_motion_snapshot(None) == EINVAL
    assert L.crt_previous_points(None, 4, I, I, P, P, None) == EINVAL and L.crt_previous_points_device(None, 4, I, I, P, P, None) == EINVAL
    assert L.crt_frame_motion(None, 2, 2, P, None) == EINVAL and L.crt_frame_motion_device(None, 2, 2, P, None) == EINVAL
    assert L.crt_temporal_accumulate_motion(None, 2, 2, K, K, P, P, P, P, P, None, Hn, P, None, None) == EINVAL
    assert L.crt_temporal_accumulate_motion_device(None, 2, 2, K, K, P, P, P, P, P, None, Hn, P, None, None) == EINVAL
    assert not buf.any() and not hist.any()


# ---- CPU: the reference pinned to its meaning

def test_reference_without_motion_is_the_plain_reference(ref, views):
    """prev_point NULL and prev_point all NaN give temporal_reference.c's bits in hist_next and out, for a static and a moved camera,
    with and without history, demodulate 0 and 1, on frames with dead pixels"""
    A, B = views["A"], views["B"]
    nan = np.full((H0, W0, 3), np.nan, np.float32)
    for name, cur in (("static", A), ("moved", B)):
        f0 = make_frame(A["pos"], A["dirs"], W0, H0, seed=11)
        poison(f0)
        f1 = make_frame(cur["pos"], cur["dirs"], W0, H0, seed=12)
        poison(f1)
        for demodulate in (0, 1):
            hist0, _ = reference(ref, A["cam"], A["cam"], A["dirs"], A["dirs"], f0, None, plain=True, demodulate=demodulate)
            for hist in (None, hist0):
                want = reference(ref, cur["cam"], A["cam"], cur["dirs"], A["dirs"], f1, hist, plain=True, demodulate=demodulate)
                for pp in (None, nan):
                    got = reference(ref, cur["cam"], A["cam"], cur["dirs"], A["dirs"], f1, hist, pp, demodulate=demodulate)
                    what = (name, demodulate, hist is not None, pp is not None)
                    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])), what
                if hist is not None:
                    assert (want[0][..., 3] > 1).sum() > W0 * H0 // 2, name


def _approach_frames(V):
    """the quad approaching the static camera A along its normal: its distance shrinks by 5 % per frame"""
    frames, qz = [], -5.0
    for k in range(FRAMES):
        if k:
            qz = V["pos"][2] - (V["pos"][2] - qz) * APPROACH
        frames.append((qz, make_frame(V["pos"], V["dirs"], W0, H0, seed=40 + k, qz=qz)))
    return frames


def test_reference_approach(ref, views):
    """A quad facing the static camera moves along its normal by 5 % of its distance per frame, five times depth_tolerance.  Without
    prev_point every interior quad pixel restarts at len = 1 in every frame; with the exact prev_point its len after frame k is k +
    1 within 1e-3 k.  Interior: the pixel's four taps lie on the quad of the previous frame, on pixels that were interior themselves."""
    A = views["A"]
    hist = {"with": None, "without": None}
    interior, prev_qz, worst = None, None, 0.0
    for k, (qz, f) in enumerate(_approach_frames(A)):
        on = f["sid"] == 2
        pp = None if k == 0 else quad_prev_points(f, (0.0, 0.0, qz - prev_qz))
        interior = on if k == 0 else interior_mask(np.where(on[..., None], f["P"] - np.array([0.0, 0.0, qz - prev_qz]), np.nan), on, interior,
                                                   A["cam"], W0, H0)
        assert interior.sum() > 0, k
        hist["with"], _ = reference(ref, A["cam"], A["cam"], A["dirs"], A["dirs"], f, hist["with"], pp)
        hist["without"], _ = reference(ref, A["cam"], A["cam"], A["dirs"], A["dirs"], f, hist["without"], None)
        assert np.all(hist["without"][..., 3][interior] == 1.0), k
        dev = float(np.abs(hist["with"][..., 3][interior].astype(np.float64) - (k + 1)).max())
        worst = max(worst, dev / max(k, 1))
        assert dev <= 1e-3 * k, (k, dev)
        prev_qz = qz
    print("approach: %d interior pixels in the last frame, worst |len - (k + 1)| / k = %.3g" % (interior.sum(), worst))
    assert np.all(hist["with"][..., 3][f["sid"] != 2] == FRAMES), "the floor and the wall did not move"


SLIDE = 0.13  # world units per frame along x: not a whole number of pixels


def _slide_frames(V, noise=0.25):
    return [(0.5 + SLIDE * k, make_frame(V["pos"], V["dirs"], W0, H0, seed=60 + k, noise=noise, qx=0.5 + SLIDE * k, textured=True))
            for k in range(FRAMES)]


def test_reference_slide(ref, views):
    """A quad with a checker fixed to it slides in its own plane under a static camera, demodulate = 0, seeded noise.  The plane and
    normal tests cannot see that motion: without prev_point the history of another texel is blended in.  After 8 frames, against
    the noise-free last frame over the interior pixels: RMSE(with motion) < RMSE(raw last frame) and < RMSE(without motion)."""
    A = views["A"]
    hist = {"with": None, "without": None}
    out = {}
    interior = None
    for k, (qx, f) in enumerate(_slide_frames(A)):
        on = f["sid"] == 2
        pp = None if k == 0 else quad_prev_points(f, (SLIDE, 0.0, 0.0))
        interior = on if k == 0 else interior_mask(np.where(on[..., None], f["P"] - np.array([SLIDE, 0.0, 0.0]), np.nan), on, interior,
                                                   A["cam"], W0, H0)
        hist["with"], out["with"] = reference(ref, A["cam"], A["cam"], A["dirs"], A["dirs"], f, hist["with"], pp, demodulate=0)
        hist["without"], out["without"] = reference(ref, A["cam"], A["cam"], A["dirs"], A["dirs"], f, hist["without"], None, demodulate=0)
    assert interior.sum() > 0
    clean = f["clean"][interior]
    e_with, e_without, e_raw = _rmse(out["with"][interior], clean), _rmse(out["without"][interior], clean), _rmse(f["rgb"][interior], clean)
    print("slide: RMSE over %d interior pixels: with motion %.4f, without motion %.4f, raw last frame %.4f" %
          (interior.sum(), e_with, e_without, e_raw))
    assert np.all(hist["with"][..., 3][interior] > FRAMES - 0.5) and np.all(hist["without"][..., 3][interior] > FRAMES - 0.5)
    assert e_with < e_raw and e_with < e_without, (e_with, e_without, e_raw)


def test_reference_disocclusion(ref, views):
    """Floor and wall pixels that the sliding quad uncovers get no history: their prev_point is NaN (they did not move), under the
    static camera their tap is their own pixel, whose record belongs to the quad, and the plane test fails.  Floor beside the quad
    keeps its history."""
    A = views["A"]
    (qx0, f0), (qx1, f1) = _slide_frames(A)[:2]
    hist, _ = reference(ref, A["cam"], A["cam"], A["dirs"], A["dirs"], f0, None)
    hist[..., 3] = np.where(hist[..., 3] > 0, np.float32(5.0), hist[..., 3])
    pp = quad_prev_points(f1, (SLIDE, 0.0, 0.0))
    nxt, _ = reference(ref, A["cam"], A["cam"], A["dirs"], A["dirs"], f1, hist, pp)
    uncovered_floor = (f1["sid"] == 0) & (f0["sid"] == 2)
    uncovered_wall = (f1["sid"] == 1) & (f0["sid"] == 2)
    kept = (f1["sid"] == 0) & (f0["sid"] == 0)
    print("disocclusion: %d floor and %d wall pixels uncovered, %d floor pixels kept" % (uncovered_floor.sum(), uncovered_wall.sum(), kept.sum()))
    assert uncovered_floor.sum() > 0 and uncovered_wall.sum() > 0 and kept.sum() > 500
    assert np.all(np.isnan(pp[uncovered_floor])) and np.all(np.isnan(pp[uncovered_wall]))
    assert np.all(nxt[..., 3][uncovered_floor] == 1.0) and np.all(nxt[..., 3][uncovered_wall] == 1.0)
    assert np.all(nxt[..., 3][kept] == 6.0)


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _device(torch, a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def _grid_mesh(cx, cy, z, size=1.2, n=2, material=0):
    """an n x n grid of quads facing +z, centred at (cx, cy, z): 2 n^2 triangles"""
    xs = np.linspace(cx - size / 2, cx + size / 2, n + 1)
    ys = np.linspace(cy - size / 2, cy + size / 2, n + 1)
    V = np.array([(x, y, z + 0.05 * ((i + j) % 2)) for j, y in enumerate(ys) for i, x in enumerate(xs)], np.float32)
    T = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            T += [(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)]
    return {"vertices": V, "triangles": np.array(T, np.uint32), "material_index": material, "normals": None}


MATS = [{"albedo": (0.8, 0.8, 0.8), "type": 1}, {"albedo": (0.7, 0.4, 0.3), "type": 1}]
LIGHTS = [((0.0, 4.0, 2.0), 60.0)]
CAM = (0.0, 0.0, 2.0)


def _four_meshes():
    return [_grid_mesh(-2.4, 0.0, -5.0), _grid_mesh(-0.8, 0.0, -5.0, material=1), _grid_mesh(0.8, 0.0, -5.0), _grid_mesh(2.4, 0.0, -5.0, material=1)]


def _rigid(deg, t):
    a = np.radians(deg)
    return np.array([[np.cos(a), -np.sin(a), 0, t[0]], [np.sin(a), np.cos(a), 0, t[1]], [0, 0, 1, t[2]]], np.float32)


def _inert_vertices(meshes):
    v3 = meshes[3]["vertices"].copy()
    v3[0, 1] = np.nan
    return v3


def _prepare_four(r, meshes):
    """before the snapshot: an update puts a NaN into vertex 0 of mesh 3, whose triangles at that vertex are inert from then on"""
    r.update_vertices(3, _inert_vertices(meshes))


def _move_four(r, meshes):
    """mesh 0: a rotation about z plus a translation; mesh 1: new vertices; mesh 2: static; mesh 3: new vertices, the NaN stays"""
    r.set_mesh_transform(0, _rigid(7.0, (0.1, -0.05, 0.3)))
    v1 = meshes[1]["vertices"] + np.float32([0.07, 0.03, 0.2]) * (1 + np.arange(len(meshes[1]["vertices"]), dtype=np.float32)[:, None] / 16)
    r.update_vertices(1, v1)
    r.update_vertices(3, _inert_vertices(meshes) + np.float32([0.0, 0.1, 0.0]))


def _world(r, meshes):
    return [(r.mesh_vertices(m)[0], meshes[m]["triangles"]) for m in range(len(meshes))]


def _record_pool(scenes, r, meshes, w=48, h=12):
    """hits of the camera rays on the current geometry, then fabricated records: every triangle at a fixed uv, misses, inst and prim
    out of range, NaN barycentrics"""
    r.set_camera(CAM, scenes.camera_matrix(0.0, 0.0))
    hit = r.trace_rays(r.camera_rays(w, h))
    inst, prim, uv = [hit["inst"]], [hit["prim"]], [hit["uv"]]
    for m, mesh in enumerate(meshes):
        nt = len(mesh["triangles"])
        inst.append(np.full(nt, m, np.uint32))
        prim.append(np.arange(nt, dtype=np.uint32))
        uv.append(np.tile(np.float32([0.3, 0.25]), (nt, 1)))
    nt0 = len(meshes[0]["triangles"])
    extra = [(MISS, MISS, 0.0, 0.0), (MISS, 0, 0.2, 0.2), (len(meshes), 0, 0.2, 0.2), (7, 1, 0.1, 0.1), (0, nt0, 0.2, 0.2), (1, MISS, 0.2, 0.2),
             (0, 1, np.nan, 0.2), (1, 1, 0.2, np.nan), (0, 2, np.nan, np.nan), (0x80000000, 0, 0.2, 0.2)]
    inst.append(np.array([e[0] for e in extra], np.uint32))
    prim.append(np.array([e[1] for e in extra], np.uint32))
    uv.append(np.array([e[2:] for e in extra], np.float32))
    return np.concatenate(inst), np.concatenate(prim), np.concatenate(uv)


@pytest.mark.gpu
def test_previous_points_equal_the_reference(pkg, scenes, ref, renderer):
    """crt_previous_points equals motion_reference.c bitwise on four meshes -- one moved by a transform, one by new vertices, one
    static, one whose update put a NaN into a vertex (inert triangles, NaN output) -- over hits of trace_rays mixed with misses, ids out of range and NaN
    barycentrics, for n = 0, 1, 65 and 4097 records; the device form gives the same bits and leaves what lies behind them alone."""
    import torch
    meshes = _four_meshes()
    renderer.upload(meshes, LIGHTS, MATS, dynamic=True)
    _prepare_four(renderer, meshes)
    before = _world(renderer, meshes)
    assert all(np.array_equal(_bits(before[m][0]), _bits(meshes[m]["vertices"])) for m in range(3))
    renderer.motion_snapshot()
    _move_four(renderer, meshes)
    now = _world(renderer, meshes)
    for m in range(3):
        assert np.array_equal(_bits(now[m][0]), _bits(before[m][0])) == (m == 2), m
    inst, prim, uv = _record_pool(scenes, renderer, meshes)
    assert (inst == MISS).any() and all((inst == m).sum() > 8 for m in range(3)), "the camera rays hit the three finite meshes"
    order = np.random.default_rng(3).permutation(len(inst))
    for n in (0, 1, 65, 4097):
        sel = np.resize(order, n)
        i, p, u = inst[sel], prim[sel], uv[sel]
        want = previous_points_reference(ref, now, before, i, p, u)
        got = renderer.previous_points(i, p, u)
        assert got.shape == (n, 3) and np.array_equal(_bits(got), _bits(want)), n
        if n == 0:
            continue
        d_i, d_p, d_u = _device(torch, i, np.uint32).view(torch.int32), _device(torch, p, np.uint32).view(torch.int32), _device(torch, u)
        d_out = torch.full((3 * n + 5,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        st = renderer.previous_points_device(n, d_i.data_ptr(), d_p.data_ptr(), d_u.data_ptr(), d_out.data_ptr(), stats=True)
        dev = d_out.cpu().numpy()
        assert np.array_equal(_bits(dev[:3 * n]), _bits(want).reshape(-1)) and np.all(dev[3 * n:] == -7.0), n
        assert st["rays_primary"] == n and st["kernel_ms"] > 0.0 and st["total_ms"] > 0.0
        assert not any(st[k] for k in ("rays_shadow", "nodes_visited", "tris_tested"))
    # what the bits mean, on the whole pool
    want = previous_points_reference(ref, now, before, inst, prim, uv)
    got = renderer.previous_points(inst, prim, uv)
    assert np.array_equal(_bits(got), _bits(want))
    finite = np.isfinite(got).all(-1)
    assert np.all(_bits(got[~finite]) == QNAN_BITS), "not moved / unknown is three quiet NaNs"
    ok = (inst < 4) & np.isfinite(uv).all(-1)
    ok[ok] &= prim[ok] < 8
    assert np.all(finite[ok & (inst <= 1)]) and not finite[~ok].any() and not finite[inst == 2].any()
    inert = ok & (inst == 3) & np.isin(prim, np.nonzero((meshes[3]["triangles"] == 0).any(-1))[0])
    assert inert.sum() >= 1 and not finite[inert].any() and finite[ok & (inst == 3) & ~inert].all()
    # the moved meshes' previous points lie on the meshes as they were: the same barycentrics over the old vertices (float64)
    for m in (0, 1):
        s = ok & (inst == m)
        V, T = before[m][0].astype(np.float64), before[m][1]
        q = V[T[prim[s]]]
        u64 = uv[s].astype(np.float64)
        exact = q[:, 0] + u64[:, :1] * (q[:, 1] - q[:, 0]) + u64[:, 1:] * (q[:, 2] - q[:, 0])
        assert np.abs(got[s] - exact).max() < 1e-5, m


@pytest.mark.gpu
def test_snapshot_lifecycle(pkg, scenes, ref, renderer):
    """before any snapshot and after a snapshot with nothing moved every output is NaN; after one mesh moved only its records are
    finite; a rebuild with either builder and a refit change no bit; a second snapshot and move report the first move's
    positions; a re-upload drops the snapshot"""
    meshes = _four_meshes()
    renderer.upload(meshes, LIGHTS, MATS, dynamic=True)
    inst, prim, uv = _record_pool(scenes, renderer, meshes)
    assert np.all(_bits(renderer.previous_points(inst, prim, uv)) == QNAN_BITS), "no snapshot"
    renderer.motion_snapshot()
    assert np.all(_bits(renderer.previous_points(inst, prim, uv)) == QNAN_BITS), "nothing moved"
    first = _rigid(5.0, (0.0, 0.2, 0.1))
    renderer.set_mesh_transform(1, first)
    got = renderer.previous_points(inst, prim, uv)
    valid = (inst == 1) & (prim < 8) & np.isfinite(uv).all(-1)
    assert valid.sum() > 8 and np.array_equal(np.isfinite(got).all(-1), valid)
    start = [(m["vertices"], m["triangles"]) for m in meshes]
    moved1 = _world(renderer, meshes)
    assert np.array_equal(_bits(got), _bits(previous_points_reference(ref, moved1, start, inst, prim, uv)))
    try:
        for builder in (0, 1):
            renderer.set_option("gpu_builder", builder)
            renderer.rebuild()
            assert np.array_equal(_bits(renderer.previous_points(inst, prim, uv)), _bits(got)), "rebuild with builder %d" % builder
    finally:
        renderer.set_option("gpu_builder", 0)
    renderer.refit()
    assert np.array_equal(_bits(renderer.previous_points(inst, prim, uv)), _bits(got)), "refit"
    renderer.motion_snapshot()
    assert np.all(_bits(renderer.previous_points(inst, prim, uv)) == QNAN_BITS), "a second snapshot, nothing moved since"
    renderer.set_mesh_transform(1, _rigid(9.0, (0.1, 0.3, 0.2)))
    again = renderer.previous_points(inst, prim, uv)
    moved2 = _world(renderer, meshes)
    assert np.array_equal(_bits(again), _bits(previous_points_reference(ref, moved2, moved1, inst, prim, uv))), "the first move's positions"
    assert np.array_equal(np.isfinite(again).all(-1), valid) and not np.array_equal(_bits(again), _bits(got))
    renderer.upload(meshes, LIGHTS, MATS, dynamic=True)
    renderer.set_mesh_transform(1, first)
    assert np.all(_bits(renderer.previous_points(inst, prim, uv)) == QNAN_BITS), "a re-upload drops the snapshot"


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (65, 5), (130, 9)], ids=lambda s: "%dx%d" % s)
def test_frame_motion_is_previous_points_of_the_centre_rays(pkg, scenes, renderer, size):
    """crt_frame_motion equals previous_points(trace_rays(camera_rays(CENTRE))) bitwise, host and device form, and leaves the
    camera alone"""
    import torch
    w, h = size
    meshes = _four_meshes()
    renderer.upload(meshes, LIGHTS, MATS, dynamic=True)
    _prepare_four(renderer, meshes)
    renderer.motion_snapshot()
    _move_four(renderer, meshes)
    renderer.set_camera(CAM if w > 1 else (-2.4, 0.0, 2.0), scenes.camera_matrix(0.0, 0.0))
    rays = renderer.camera_rays(w, h)
    hit = renderer.trace_rays(rays)
    want = renderer.previous_points(hit["inst"], hit["prim"], hit["uv"]).reshape(h, w, 3)
    assert np.isfinite(want).all(-1).any(), "some pixel sees a moved mesh"
    if w > 1:
        assert np.isnan(want).all(-1).any(), "some pixel sees the background or the static mesh"
    got = renderer.frame_motion(w, h)
    assert got.shape == (h, w, 3) and np.array_equal(_bits(got), _bits(want))
    d_out = torch.full((3 * w * h + 4,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = renderer.frame_motion_device(w, h, d_out.data_ptr(), stats=True)
    dev = d_out.cpu().numpy()
    assert np.array_equal(_bits(dev[:3 * w * h]), _bits(want).reshape(-1)) and np.all(dev[3 * w * h:] == -7.0)
    assert st["rays_primary"] == w * h and st["kernel_ms"] > 0.0
    assert np.array_equal(_bits(renderer.camera_rays(w, h)), _bits(rays))


def _device_dirs(renderer, cam, w, h):
    renderer.set_camera(cam[:3], cam[3:])
    return np.ascontiguousarray(renderer.camera_rays(w, h)[:, 4:7])


def _pairs(scenes):
    a = camera(POS_A, scenes.camera_matrix(0.0, 0.0))
    return (("equal", a, a.copy()), ("move", camera(POS_B, scenes.camera_matrix(2.0, 0.0)), a))


def _mixed_prev_points(f, cam_prev, seed):
    """per pixel one of: NaN (not moved), a finite point near the pixel's own (on screen), one far to the side (off screen), one
    behind the previous camera, a point with an infinite component (+inf, -inf: not moved)"""
    h, w = f["t"].shape
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 6, size=(h, w))
    P = np.where(f["hit"][..., None], f["P"], 0.0)
    pp = (P + rng.uniform(-0.15, 0.15, size=P.shape)).astype(np.float32)
    pp[kind == 0] = np.nan
    pp[kind == 2] += np.float32([300.0, 0.0, 0.0])
    pp[kind == 3] = (cam_prev[:3].astype(np.float64) + np.array([0.3, 0.2, 5.0])).astype(np.float32)  # the camera looks along -z
    pp[kind == 4, 1] = np.inf
    pp[kind == 5, 2] = -np.inf
    return pp


def _run_device(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, d_pp, prm, out="fresh"):
    d_rgb = d["rgb"].clone() if out == "rgb" else d["rgb"]
    d_next = torch.full((h, w, 8), -7.0, dtype=torch.float32, device="cuda")
    d_out = {"fresh": torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda"), "rgb": d_rgb, "none": None}[out]
    torch.cuda.synchronize()
    renderer.temporal_accumulate_device(w, h, cam_cur, cam_prev, d_rgb.data_ptr(), d["normal"].data_ptr(),
                                        d["albedo"].data_ptr() if prm["demodulate"] else None, d["t"].data_ptr(),
                                        None if d_hist is None else d_hist.data_ptr(), d_next.data_ptr(),
                                        None if d_out is None else d_out.data_ptr(), d_prev_point=None if d_pp is None else d_pp.data_ptr(), **prm)
    renderer.synchronize()
    return d_next.cpu().numpy(), None if d_out is None else d_out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (65, 5), (130, 9)], ids=lambda s: "%dx%d" % s)
def test_motion_kernel_equals_the_reference(pkg, scenes, ref, renderer, size):
    """hist_next and out of crt_temporal_accumulate_motion_device equal motion_reference.c's bits with a prev_point buffer that mixes
    NaN, on-screen, off-screen, behind-the-camera and infinite entries: static and moved camera, with and without history,
    demodulate 0 and 1, out NULL, out == rgb; the host form gives the same bits.  prev_point NULL and all NaN equal
    crt_temporal_accumulate_device bitwise."""
    import torch
    w, h = size
    moved_with_history = 0
    for name, cam_cur, cam_prev in _pairs(scenes):
        dir_cur, dir_prev = _device_dirs(renderer, cam_cur, w, h), _device_dirs(renderer, cam_prev, w, h)
        f0 = make_frame(cam_prev[:3], dir_prev, w, h, seed=11)
        poison(f0)
        f1 = make_frame(cam_cur[:3], dir_cur, w, h, seed=12)
        poison(f1)
        pp = _mixed_prev_points(f1, cam_prev, 13)
        nan = np.full((h, w, 3), np.nan, np.float32)
        d = {k: _device(torch, f1[k]) for k in ("rgb", "normal", "albedo", "t")}
        d_pp, d_nan = _device(torch, pp), _device(torch, nan)
        for demodulate in (0, 1):
            prm = dict(DEFAULTS, demodulate=demodulate)
            hist0, _ = reference(ref, cam_prev, cam_prev, dir_prev, dir_prev, f0, None, **prm)
            hist0[..., 3] = np.where(hist0[..., 3] > 0, np.float32(3.0), hist0[..., 3])
            for hist_prev in (None, hist0):
                what = "%dx%d %s demodulate %d history %s" % (w, h, name, demodulate, hist_prev is not None)
                want = reference(ref, cam_cur, cam_prev, dir_cur, dir_prev, f1, hist_prev, pp, **prm)
                d_hist = None if hist_prev is None else _device(torch, hist_prev)
                for out in ("fresh", "rgb", "none"):
                    got = _run_device(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, d_pp, prm, out)
                    assert np.array_equal(_bits(got[0]), _bits(want[0])), what + ": hist_next, out " + out
                    assert out == "none" or np.array_equal(_bits(got[1]), _bits(want[1])), what + ": out " + out
                host = renderer.temporal_accumulate(cam_cur, cam_prev, f1["rgb"], f1["normal"], f1["albedo"] if demodulate else None, f1["t"],
                                                    hist_prev, prev_point=pp, **prm)
                assert np.array_equal(_bits(host[0]), _bits(want[0])) and np.array_equal(_bits(host[1]), _bits(want[1])), what + ": host form"
                plain = _run_device(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, None, prm)
                for label, buf in (("NaN", d_nan),):
                    got = _run_device(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, buf, prm)
                    assert np.array_equal(_bits(got[0]), _bits(plain[0])) and np.array_equal(_bits(got[1]), _bits(plain[1])), what + ": " + label
                null = C.c_void_p(None)
                d_next = torch.full((h, w, 8), -7.0, dtype=torch.float32, device="cuda")
                d_out = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                p_ = pkg.TemporalParams(**prm)
                rc = pkg.lib().crt_temporal_accumulate_motion_device(renderer.h, w, h, cam_cur.ctypes.data, cam_prev.ctypes.data, d["rgb"].data_ptr(),
                                                                     d["normal"].data_ptr(), d["albedo"].data_ptr() if demodulate else None,
                                                                     d["t"].data_ptr(), null, None if d_hist is None else d_hist.data_ptr(),
                                                                     d_next.data_ptr(), d_out.data_ptr(), C.byref(p_), None)
                assert rc == 0
                renderer.synchronize()
                assert np.array_equal(_bits(d_next.cpu().numpy()), _bits(plain[0])) and np.array_equal(_bits(d_out.cpu().numpy()), _bits(plain[1])), \
                    what + ": NULL prev_point"
                if hist_prev is not None:
                    moved = np.isfinite(pp).all(-1)
                    moved_with_history += int(((want[0][..., 3] > 1) & moved).sum())
    if w * h >= 64:
        assert moved_with_history > 0, "some moved pixel took history"
    print("%dx%d: %d moved pixel results with history" % (w, h, moved_with_history))


@pytest.mark.gpu
def test_three_chained_frames(pkg, scenes, ref, renderer):
    """three frames of the sliding, approaching quad along a three-pose camera path, chained through two swapped device buffers with
    the exact prev_point of each frame, equal the reference chained the same way"""
    import torch
    w, h = 65, 23
    cams = [camera(POS_A, scenes.camera_matrix(0.0, 0.0)), camera(POS_B, scenes.camera_matrix(2.0, 0.0)),
            camera((0.3, 0.62, 2.1), scenes.camera_matrix(4.0, 0.0))]
    dirs = [_device_dirs(renderer, c, w, h) for c in cams]
    d_hist = [torch.zeros((h, w, 8), dtype=torch.float32, device="cuda") for _ in range(2)]
    hist_ref, quad_lens = None, []
    pose = [(0.5, -5.0), (0.63, -4.8), (0.76, -4.6)]
    for k in range(3):
        f = make_frame(cams[k][:3], dirs[k], w, h, seed=20 + k, qx=pose[k][0], qz=pose[k][1])
        pp = np.full((h, w, 3), np.nan, np.float32) if k == 0 else quad_prev_points(f, (pose[k][0] - pose[k - 1][0], 0.0, pose[k][1] - pose[k - 1][1]))
        poison(f)
        d = {g: _device(torch, f[g]) for g in ("rgb", "normal", "albedo", "t")}
        d_pp = _device(torch, pp)
        d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        prev = max(k - 1, 0)
        torch.cuda.synchronize()
        renderer.temporal_accumulate_device(w, h, cams[k], cams[prev], d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(),
                                            d["t"].data_ptr(), d_hist[k & 1].data_ptr() if k else None, d_hist[(k & 1) ^ 1].data_ptr(),
                                            d_out.data_ptr(), d_prev_point=d_pp.data_ptr())
        renderer.synchronize()
        hist_ref, out_ref = reference(ref, cams[k], cams[prev], dirs[k], dirs[prev], f, hist_ref, pp)
        assert np.array_equal(_bits(d_hist[(k & 1) ^ 1].cpu().numpy()), _bits(hist_ref)), k
        assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(out_ref)), k
        quad_lens.append(float(hist_ref[..., 3][f["sid"] == 2].max()))
    assert all(abs(l - (k + 1)) < 1e-3 for k, l in enumerate(quad_lens)), quad_lens


@pytest.mark.gpu
def test_errors(pkg, scenes, renderer):
    """every error case returns its code, launches nothing and leaves sentinel-filled outputs untouched: CRT_ESTATE before any
    upload and on a scene uploaded without "dynamic", CRT_EINVAL for NULL and misaligned buffers and bad frame sizes"""
    import torch
    L = pkg.lib()
    n, w, h = 16, 8, 4
    sentinel = -77.0  # no coordinate of the scene
    ids = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    d_uv = torch.zeros(2 * n + 2, dtype=torch.float32, device="cuda")
    d_pt = torch.full((3 * max(n, w * h) + 4,), sentinel, dtype=torch.float32, device="cuda")
    h_ids, h_uv = np.zeros(n, np.uint32), np.zeros((n, 2), np.float32)
    h_pt = np.full((max(n, w * h), 3), sentinel, np.float32)
    torch.cuda.synchronize()
    I, U, P = ids.data_ptr(), d_uv.data_ptr(), d_pt.data_ptr()
    hI, hU, hP = h_ids.ctypes.data, h_uv.ctypes.data, h_pt.ctypes.data

    def untouched():
        torch.cuda.synchronize()
        return bool((d_pt == sentinel).all().item()) and bool(np.all(h_pt == sentinel))

    def state_errors(r):
        assert L.crt_motion_snapshot(r.h) == ESTATE
        assert L.crt_previous_points_device(r.h, n, I, I, U, P, None) == ESTATE and L.crt_previous_points(r.h, n, hI, hI, hU, hP, None) == ESTATE
        assert L.crt_previous_points_device(r.h, 0, I, I, U, P, None) == ESTATE
        assert L.crt_frame_motion_device(r.h, w, h, P, None) == ESTATE and L.crt_frame_motion(r.h, w, h, hP, None) == ESTATE
        assert "dynamic" in L.crt_last_error(r.h).decode()
        assert untouched()
    fresh = pkg.Renderer(0)
    try:
        state_errors(fresh)  # before any upload
    finally:
        fresh.close()
    meshes = _four_meshes()
    renderer.upload(meshes, LIGHTS, MATS, dynamic=False)
    state_errors(renderer)
    renderer.upload(meshes, LIGHTS, MATS, dynamic=True)
    renderer.set_camera(CAM, scenes.camera_matrix(0.0, 0.0))
    renderer.motion_snapshot()
    renderer.set_mesh_transform(0, _rigid(3.0, (0.0, 0.1, 0.0)))
    dev = lambda **o: L.crt_previous_points_device(renderer.h, o.get("n", n), o.get("inst", I), o.get("prim", I), o.get("uv", U), o.get("point", P), None)
    host = lambda **o: L.crt_previous_points(renderer.h, o.get("n", n), o.get("inst", hI), o.get("prim", hI), o.get("uv", hU), o.get("point", hP), None)
    for g in ("inst", "prim", "uv", "point"):
        assert dev(**{g: None}) == EINVAL and host(**{g: None}) == EINVAL, g
    assert dev(inst=I + 2) == EINVAL and dev(prim=I + 2) == EINVAL and dev(point=P + 2) == EINVAL
    assert dev(uv=U + 4) == EINVAL and "aligned" in L.crt_last_error(renderer.h).decode()
    assert dev(n=0, inst=None, point=None) == 0 and host(n=0, uv=None) == 0, "n = 0 looks at no buffer"
    for bad in ((0, h), (w, 0), (1 << 15, 1 << 14)):
        assert L.crt_frame_motion_device(renderer.h, bad[0], bad[1], P, None) == EINVAL and L.crt_frame_motion(renderer.h, bad[0], bad[1], hP, None) == EINVAL
    assert L.crt_frame_motion_device(renderer.h, w, h, None, None) == EINVAL and L.crt_frame_motion(renderer.h, w, h, None, None) == EINVAL
    assert L.crt_frame_motion_device(renderer.h, w, h, P + 2, None) == EINVAL
    assert untouched()
    # the motion temporal call keeps the plain call's argument rules and adds prev_point's alignment
    cam = camera(POS_A, scenes.camera_matrix(0.0, 0.0))
    K = cam.ctypes.data
    px = torch.full((w * h * 3 + 4,), 0.5, dtype=torch.float32, device="cuda")
    tt = torch.full((w * h,), 2.0, dtype=torch.float32, device="cuda")
    d_next = torch.full((w * h * 8,), sentinel, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    X = px.data_ptr()

    def temporal(**o):
        return L.crt_temporal_accumulate_motion_device(renderer.h, o.get("w", w), h, K, K, o.get("rgb", X), X, X, tt.data_ptr(), o.get("pp", X), None,
                                                       o.get("next", d_next.data_ptr()), P, C.byref(o["prm"]) if "prm" in o else None, None)
    assert temporal(pp=X + 2) == EINVAL and temporal(rgb=None) == EINVAL and temporal(next=None) == EINVAL and temporal(w=0) == EINVAL
    assert temporal(prm=pkg.TemporalParams(alpha=2.0)) == EINVAL and temporal(prm=pkg.TemporalParams(depth_tolerance=0.0)) == EINVAL
    torch.cuda.synchronize()
    assert untouched() and bool((d_next == sentinel).all().item())
    # the controls
    assert dev() == 0 and host() == 0 and L.crt_frame_motion_device(renderer.h, w, h, P, None) == 0 and temporal() == 0
    torch.cuda.synchronize()
    assert not bool((d_pt[:3 * w * h] == sentinel).any().item()) and bool((d_pt[3 * w * h:] == sentinel).all().item())
    assert not np.any(h_pt[:n] == sentinel) and not bool((d_next == sentinel).any().item())


def _pipeline_scene():
    floor = {"vertices": np.float32([(-8, -1, 2), (8, -1, 2), (8, -1, -12), (-8, -1, -12)]), "triangles": np.uint32([(0, 1, 2), (0, 2, 3)]),
             "material_index": 0, "normals": None}
    quad = {"vertices": np.float32([(-1.5, -0.4, -5), (1.5, -0.4, -5), (1.5, 1.6, -5), (-1.5, 1.6, -5)]), "triangles": np.uint32([(0, 1, 2), (0, 2, 3)]),
            "material_index": 1, "normals": None}
    return [floor, quad]


@pytest.mark.gpu
def test_pipeline(pkg, scenes, renderer):
    """A dynamic scene at 96 x 64, mode 200, 1 spp, seed advanced per frame: a quad approaches the camera above a floor by 5 % of
    its distance per frame over 8 frames.  Per frame: motion_snapshot, move, frame_guides + frame_motion, TemporalHistory.push.
    Without prev_point every interior quad pixel has len = 1 in every frame; with it len after frame k is k + 1 within 1e-3 k.
    Against a 64-spp render of the last pose, over the quad's interior: RMSE(with motion) < RMSE(1-spp frame).
    Observed on the MI355X: 140 interior pixels in the last frame, worst |len - (k + 1)| = 9.5e-7; RMSE 1 spp 0.0298, with
    motion 0.0171, without motion 0.0298 (the 1-spp frame itself: its history restarts every frame)."""
    w, h = 96, 64
    cam_z = 2.0
    renderer.upload(_pipeline_scene(), LIGHTS, MATS, dynamic=True)
    rot = scenes.camera_matrix(0.0, 0.0)
    renderer.set_camera((0.0, 0.6, cam_z), rot)
    cam = camera((0.0, 0.6, cam_z), rot)
    with_m, without = pkg.TemporalHistory(renderer, w, h), pkg.TemporalHistory(renderer, w, h)
    interior, dist, worst = None, cam_z + 5.0, 0.0
    try:
        renderer.change_shading_mode(200)
        for k in range(FRAMES):
            renderer.motion_snapshot()
            if k:
                dist *= APPROACH
                renderer.set_mesh_transform(1, np.float32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, (cam_z - dist) + 5.0]]))
            renderer.set_path_params(1, 3, 1234 + k)
            noisy = renderer.render_frame(w, h, want=("rgba8", "rgb"))["rgb"]
            g = renderer.frame_guides(w, h)
            pp = renderer.frame_motion(w, h)
            out_with = with_m.push(noisy, g["normal"], g["albedo"], g["t"], prev_point=pp)
            out_without = without.push(noisy, g["normal"], g["albedo"], g["t"])
            on = renderer.trace_rays(renderer.camera_rays(w, h), want=("inst",))["inst"].reshape(h, w) == 1
            moved = np.isfinite(pp).all(-1)
            assert np.array_equal(moved, on if k else np.zeros_like(on)), "exactly the quad's pixels moved"
            interior = on if k == 0 else interior_mask(pp, on, interior, cam, w, h)
            assert interior.sum() > 0, k
            len_with, len_without = with_m.records[..., 3].cpu().numpy(), without.records[..., 3].cpu().numpy()
            assert np.all(len_without[interior] == 1.0), k
            dev = float(np.abs(len_with[interior].astype(np.float64) - (k + 1)).max())
            worst = max(worst, dev)
            assert dev <= 1e-3 * k, (k, dev)
        renderer.set_path_params(64, 3, 99)
        clean = renderer.render_frame(w, h, want=("rgba8", "rgb"))["rgb"]
    finally:
        renderer.set_path_params(4, 3, 1234)
        renderer.change_shading_mode(0)
    e_raw, e_with, e_without = _rmse(noisy[interior], clean[interior]), _rmse(out_with[interior], clean[interior]), _rmse(out_without[interior], clean[interior])
    print("pipeline: %d interior pixels, worst |len - (k + 1)| %.3g; RMSE against 64 spp: 1 spp %.4f, with motion %.4f, without motion %.4f" %
          (interior.sum(), worst, e_raw, e_with, e_without))
    assert e_with < e_raw, (e_with, e_raw)


@pytest.mark.gpu
def test_cpp_layer(pkg, scenes, renderer, tmp_path):
    """crt::Renderer::motionSnapshot / frameMotion / temporalFrame(params, true), from a small C++ program linked against
    libcrt_hip.so, give the Python layer's bits on one 40 x 24 frame of the Cornell box with its last mesh moved"""
    exe = str(tmp_path / "motion_cpp")
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(lib_dir, "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "motion_cpp.cpp"), "-L" + lib_dir, "-lcrt_hip",
                           "-Wl,-rpath," + lib_dir, "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    w, h = 40, 24
    shift = (0.25, 0.125, -0.5)
    scene = pkg.Scene.from_arrays(scenes.cornell_box())
    path = str(tmp_path / "cornell.crtbin")
    scene.save(path)
    mesh = scene.mesh_count - 1
    try:
        renderer.upload_scene(scene, dynamic=True)
        renderer.set_camera_from(scene)
        renderer.change_shading_mode(3)
        th = pkg.TemporalHistory(renderer, w, h)

        def push():
            rgb = renderer.render_frame(w, h, want=("rgba8", "rgb"))["rgb"]
            g = renderer.frame_guides(w, h)
            pp = renderer.frame_motion(w, h)
            return pp, th.push(rgb, g["normal"], g["albedo"], g["t"], prev_point=pp)
        push()
        renderer.motion_snapshot()
        renderer.set_mesh_transform(mesh, np.float32([[1, 0, 0, shift[0]], [0, 1, 0, shift[1]], [0, 0, 1, shift[2]]]))
        want_pp, want_rgb = push()
    finally:
        renderer.change_shading_mode(0)
        scene.close()
    moved = np.isfinite(want_pp).all(-1)
    assert 0 < moved.sum() < w * h, "the moved mesh covers a part of the frame"
    out = str(tmp_path / "out.bin")
    subprocess.check_call([exe, path, str(w), str(h), str(mesh)] + [repr(float(s)) for s in shift] + [out], timeout=120)
    raw = np.fromfile(out, dtype=np.float32)
    assert raw.size == 6 * w * h
    assert np.array_equal(_bits(raw[:3 * w * h]), _bits(want_pp).reshape(-1)), "frameMotion"
    assert np.array_equal(_bits(raw[3 * w * h:]), _bits(want_rgb).reshape(-1)), "temporalFrame(params, true)"
