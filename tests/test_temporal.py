"""Temporal reprojection (crt_temporal_accumulate*, include/crt_hip.h): a path-traced frame blended with the history of earlier
frames, carried across camera moves.

tests/temporal_reference.c restates the header's contract in plain C (compiled here with -O2 -ffp-contract=off); it takes the ray
directions of both cameras as arrays, so it restates no ray generation.  On the CPU the reference is pinned to what it means on an
analytic scene (a floor, a back wall and a pillar face in front of the wall, the colour a smooth function of the world point), with
directions from the oracle's oracle_ray_dir.  On the GPU the kernel equals the reference bit for bit, with directions from
crt_camera_rays.

Figures observed on the CPU (analytic scene, 96 x 64): (a) running mean within 2.0e-7 relative; (b) 95.8 % of the live pixels
keep their history, mean absolute error 0.0006; (d) a strip of 39 pixels.  The pipeline's figures are in test_pipeline's docstring and DESIGN.md 5h."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("crt_temporal_accumulate_device", "crt_temporal_accumulate")
EINVAL = 1
T_MISS = np.float32(10000.0)
DEFAULTS = {"alpha": 0.1, "depth_tolerance": 0.01, "normal_threshold": 0.9, "max_history": 64, "demodulate": 1}
# the pipeline: the ratio predicted on the CPU (test_pipeline_prediction) and the cap of the GPU test, 1.25 x the prediction
PIPELINE_PREDICTION = 0.6363
PIPELINE_CAP = 1.25 * PIPELINE_PREDICTION


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the reference (tests/temporal_reference.c)

@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for tests/temporal_reference.c")
    out = str(tmp_path_factory.mktemp("temporal_reference") / "libtemporal_reference.so")
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "temporal_reference.c"), "-o", out, "-lm"])
    L = C.CDLL(out)
    L.temporal_reference.restype = None
    L.temporal_reference.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 11 + [C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32]
    return L


def reference(L, cam_cur, cam_prev, dir_cur, dir_prev, frame, hist_prev=None, **params):
    """one call of the reference: (hist_next (h, w, 8), out (h, w, 3))"""
    prm = dict(DEFAULTS, **params)
    h, w = frame["t"].shape
    a = {k: np.ascontiguousarray(frame[k], dtype=np.float32) for k in ("rgb", "normal", "albedo", "t")}
    cc, cp = np.ascontiguousarray(cam_cur, np.float32), np.ascontiguousarray(cam_prev, np.float32)
    dc, dp = np.ascontiguousarray(dir_cur, np.float32), np.ascontiguousarray(dir_prev, np.float32)
    assert cc.size == 12 and cp.size == 12 and dc.size == 3 * w * h and dp.size == 3 * w * h
    hp = None if hist_prev is None else np.ascontiguousarray(hist_prev, np.float32)
    hist = np.zeros((h, w, 8), np.float32)
    out = np.zeros((h, w, 3), np.float32)
    L.temporal_reference(w, h, cc.ctypes.data, cp.ctypes.data, dc.ctypes.data, dp.ctypes.data, a["rgb"].ctypes.data, a["normal"].ctypes.data,
                         a["albedo"].ctypes.data if prm["demodulate"] else None, a["t"].ctypes.data, None if hp is None else hp.ctypes.data,
                         hist.ctypes.data, out.ctypes.data, prm["alpha"], prm["depth_tolerance"], prm["normal_threshold"], prm["max_history"],
                         prm["demodulate"])
    return hist, out


# ---- the analytic scene: floor y = -1, back wall z = -8, a pillar face z = -5 for |x - 0.5| < 0.7 and y < 1.2

FLOOR_Y, WALL_Z, PILLAR_Z, PILLAR_X, PILLAR_HALF, PILLAR_TOP = -1.0, -8.0, -5.0, 0.5, 0.7, 1.2


def yaw_matrix(deg, scenes):
    return scenes.camera_matrix(deg, 0.0)


def camera(pos, rot):
    return np.concatenate([np.asarray(pos, np.float32).reshape(3), np.asarray(rot, np.float32).reshape(9)])


def irradiance(P):
    return 0.55 + 0.2 * np.sin(0.7 * P[..., 0]) * np.cos(0.5 * P[..., 2]) + 0.05 * P[..., 1]


def albedo_at(P):
    return np.stack([0.6 + 0.3 * np.sin(2.0 * P[..., 0]), 0.5 + 0.2 * np.cos(1.5 * P[..., 1]), 0.6 + 0.3 * np.cos(3.0 * P[..., 2])], axis=-1)


def cast(o, dirs, w, h):
    """the analytic scene along the rays o + t d (float64): surface id (0 floor, 1 wall, 2 pillar), t, world point, normal"""
    o = np.asarray(o, np.float64)
    d = np.asarray(dirs, np.float64).reshape(h, w, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        tf = np.where(d[..., 1] < 0, (FLOOR_Y - o[1]) / d[..., 1], np.inf)
        tw = np.where(d[..., 2] < 0, (WALL_Z - o[2]) / d[..., 2], np.inf)
        tp = np.where(d[..., 2] < 0, (PILLAR_Z - o[2]) / d[..., 2], np.inf)
    Pp = o + d * np.where(np.isfinite(tp), tp, 0.0)[..., None]
    tp = np.where((np.abs(Pp[..., 0] - PILLAR_X) < PILLAR_HALF) & (Pp[..., 1] < PILLAR_TOP) & (tp > 0), tp, np.inf)
    tf = np.where(tf > 0, tf, np.inf)
    tw = np.where(tw > 0, tw, np.inf)
    ts = np.stack([tf, tw, tp], axis=-1)
    sid = ts.argmin(axis=-1)
    t = ts.min(axis=-1)
    hit = np.isfinite(t)
    P = o + d * np.where(hit, t, 0.0)[..., None]
    n = np.where((sid == 0)[..., None], np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]))
    return sid, t, P, n, hit


def make_frame(o, dirs, w, h, seed=None, noise=0.1):
    """a frame of the analytic scene: rgb = albedo(P) irradiance(P) (+ uniform noise of that amplitude, never below 0.05)"""
    sid, t, P, n, hit = cast(o, dirs, w, h)
    alb = albedo_at(P)
    clean = alb * irradiance(P)[..., None]
    rgb = clean.copy()
    if seed is not None:
        rgb += np.random.default_rng(seed).uniform(-noise, noise, size=rgb.shape)
    f = {"rgb": np.where(hit[..., None], rgb, 0.25).astype(np.float32), "normal": np.where(hit[..., None], n, 0.0).astype(np.float32),
         "albedo": np.where(hit[..., None], alb, 0.0).astype(np.float32), "t": np.where(hit, t, T_MISS).astype(np.float32)}
    f.update(clean=clean, P=P, sid=sid, hit=hit)
    return f


def poison(f):
    """a miss block, one NaN colour and one NaN normal, wherever the frame has room for them; returns the mask of these pixels"""
    h, w = f["t"].shape
    dead = np.zeros((h, w), bool)
    if w >= 8 and h >= 4:
        dead[1:3, 2:5] = True
        f["rgb"][1:3, 2:5] = (0.0, 1.0, 1.0)
        f["normal"][1:3, 2:5] = 0.0
        f["albedo"][1:3, 2:5] = 0.0
        f["t"][1:3, 2:5] = T_MISS
    if w * h >= 16:
        i, j = np.unravel_index((w * h) // 2, (h, w)), np.unravel_index((w * h) // 2 + 3, (h, w))
        f["rgb"][i][1] = np.nan
        f["normal"][j][2] = np.nan
        dead[i] = dead[j] = True
    return dead


def oracle_dirs(oracle, rot, w, h):
    return np.array([oracle.ray_dir(rot, px, py, w, h) for py in range(h) for px in range(w)], np.float32)


def live_mask(f, demodulate=1):
    ok = np.isfinite(f["rgb"]).all(-1) & np.isfinite(f["normal"]).all(-1) & np.isfinite(f["t"]) & (f["normal"] != 0).any(-1) & (f["t"] > 0)
    return ok & np.isfinite(f["albedo"]).all(-1) if demodulate else ok


W0, H0 = 96, 64
POS_A = (0.0, 0.6, 2.0)
POS_B = (0.15, 0.6, 2.05)


@pytest.fixture(scope="module")
def views(oracle, scenes):
    """the cameras of the CPU tests with their oracle directions at 96 x 64: A, B = A translated by (0.15, 0, 0.05) and yawed 2
    degrees, C = A yawed 180 degrees, D = A moved 4 to the right"""
    v = {}
    for name, pos, yaw in (("A", POS_A, 0.0), ("B", POS_B, 2.0), ("C", POS_A, 180.0), ("D", (4.0, 0.6, 2.0), 0.0)):
        rot = yaw_matrix(yaw, scenes)
        dirs = oracle_dirs(oracle, rot, W0, H0)
        dirs.setflags(write=False)
        v[name] = {"pos": pos, "cam": camera(pos, rot), "dirs": dirs}
    return v


# ---- CPU: the interface

def test_binding_and_library_expose_the_new_entry_points(pkg):
    L = pkg.lib()
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
        assert ("int %s(" % s) in header, s
    assert "crt_temporal_params" in header
    for name in ("temporal_accumulate", "temporal_accumulate_device"):
        assert callable(getattr(pkg.Renderer, name, None)), name
    assert callable(getattr(pkg.TemporalHistory, "push", None)) and callable(getattr(pkg.TemporalHistory, "reset", None))
    assert C.sizeof(pkg.TemporalParams) == 20
    d = pkg.TemporalParams()
    assert (d.max_history, d.demodulate) == (64, 1)
    assert np.float32(d.alpha) == np.float32(0.1) and np.float32(d.depth_tolerance) == np.float32(0.01)
    assert np.float32(d.normal_threshold) == np.float32(0.9)
    buf = np.zeros(64, dtype=np.float32)
    hist = np.zeros(64, dtype=np.float32)
    cam = np.zeros(12, dtype=np.float32)
    P, Hn, K = buf.ctypes.data, hist.ctypes.data, cam.ctypes.data
    assert L.crt_temporal_accumulate(None, 2, 2, K, K, P, P, P, P, None, Hn, P, None, None) == EINVAL
    assert L.crt_temporal_accumulate_device(None, 2, 2, K, K, P, P, P, P, None, Hn, P, None, None) == EINVAL
    assert not buf.any() and not hist.any()


# ---- CPU: the reference pinned to its meaning

def test_reference_static_camera_is_the_running_mean(ref, views):
    """(a) static camera, alpha = 0, 6 noisy frames: every live pixel is the float64 running mean within 1e-5 relative and len
    = min(k, max_history) exactly (max_history 64 and 3)"""
    A = views["A"]
    frames = [make_frame(A["pos"], A["dirs"], W0, H0, seed=100 + k, noise=0.03) for k in range(6)]
    live = live_mask(frames[0])
    assert live.all() and min(float(f["rgb"].min()) for f in frames) >= 0.05
    for cap in (64, 3):
        hist, total, worst = None, np.zeros((H0, W0, 3)), 0.0
        for k, f in enumerate(frames, 1):
            hist, out = reference(ref, A["cam"], A["cam"], A["dirs"], A["dirs"], f, hist, alpha=0.0, max_history=cap)
            total += f["rgb"].astype(np.float64)
            assert np.array_equal(hist[..., 3], np.full((H0, W0), np.float32(min(k, cap)))), (cap, k)
            assert np.array_equal(_bits(hist[..., 4:7]), _bits(f["normal"])) and np.array_equal(_bits(hist[..., 7]), _bits(f["t"]))
            if cap == 64:
                mean = total / k
                worst = max(worst, float((np.abs(out - mean) / np.abs(mean)).max()))
        if cap == 64:
            print("(a) worst relative deviation from the float64 running mean: %.3g" % worst)
            assert worst <= 1e-5, worst


def _long_history(ref, V, frame):
    """the records of `frame` (noise-free) as if 2^20 frames had been averaged: a later blend returns the history itself to 1e-6"""
    hist, _ = reference(ref, V["cam"], V["cam"], V["dirs"], V["dirs"], frame, None)
    hist[..., 3] = np.where(hist[..., 3] > 0, np.float32(1 << 20), hist[..., 3])
    return hist


def test_reference_follows_a_camera_move(ref, views):
    """(b) the camera translated by (0.15, 0, 0.05) and yawed 2 degrees: at least 90 % of the live pixels have history, and what
    they take from it is the analytic colour at their world point within 0.02 (mean absolute error).  A numpy prototype of the
    formulas gave 95 % and 0.0054."""
    A, B = views["A"], views["B"]
    hist = _long_history(ref, A, make_frame(A["pos"], A["dirs"], W0, H0))
    fb = make_frame(B["pos"], B["dirs"], W0, H0)
    nxt, out = reference(ref, B["cam"], A["cam"], B["dirs"], A["dirs"], dict(fb, rgb=np.zeros_like(fb["rgb"])), hist, alpha=0.0,
                         max_history=1 << 24)
    live = live_mask(fb)
    have = live & (nxt[..., 3] > 1)
    share = have.sum() / live.sum()
    err = float(np.abs(out.astype(np.float64) - fb["clean"])[have].mean())
    print("(b) %.1f %% of the live pixels have history; mean absolute error %.4f" % (100.0 * share, err))
    assert live.sum() == W0 * H0 and share >= 0.90, share
    assert err < 0.02, err


def test_reference_about_turn_has_no_history(ref, views):
    """(c) a camera yawed 180 degrees sees points that lay behind the previous camera: len == 1 everywhere"""
    A, Cv = views["A"], views["C"]
    hist = _long_history(ref, A, make_frame(A["pos"], A["dirs"], W0, H0))
    fc = make_frame(Cv["pos"], Cv["dirs"], W0, H0, seed=5)
    live = live_mask(fc)
    nxt, out = reference(ref, Cv["cam"], A["cam"], Cv["dirs"], A["dirs"], fc, hist)
    assert live.sum() > W0 * H0 // 4, "the floor is in view"
    assert np.all(nxt[..., 3][live] == 1.0) and np.all(nxt[..., 3][~live] == 0.0)
    nohist, out0 = reference(ref, Cv["cam"], A["cam"], Cv["dirs"], A["dirs"], fc, None)
    assert np.array_equal(_bits(nxt), _bits(nohist)) and np.array_equal(_bits(out), _bits(out0))


def _project(P, cam_prev, w, h):
    """float64 screen position of world points in the previous camera (the header's steps 5 and 6)"""
    o, R = cam_prev[:3].astype(np.float64), cam_prev[3:].astype(np.float64).reshape(3, 3)
    pc = (P - o) @ R
    s = -pc[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        fx = ((pc[..., 0] / s) / (w / h) + 1) * 0.5 * w - 0.5
        fy = (1 - pc[..., 1] / s) * 0.5 * h - 0.5
    return fx, fy, s


def test_reference_disocclusion(ref, views):
    """(d) the camera moved 4 to the right: the strip of wall the pillar hid has len == 1 (the pixels whose four taps all fall
    on the pillar in the previous frame: equal normals, another depth), while the floor beside it keeps its history"""
    A, D = views["A"], views["D"]
    fa = make_frame(A["pos"], A["dirs"], W0, H0)
    hist = _long_history(ref, A, fa)
    fd = make_frame(D["pos"], D["dirs"], W0, H0, seed=9)
    nxt, _ = reference(ref, D["cam"], A["cam"], D["dirs"], A["dirs"], fd, hist)
    fx, fy, s = _project(fd["P"], A["cam"], W0, H0)
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    inner = (s > 0) & (x0 >= 0) & (x0 + 1 < W0) & (y0 >= 0) & (y0 + 1 < H0)
    xs, ys = np.clip(x0, 0, W0 - 2), np.clip(y0, 0, H0 - 2)

    def taps_all(sid):
        m = inner.copy()
        for dy in (0, 1):
            for dx in (0, 1):
                m &= fa["sid"][ys + dy, xs + dx] == sid
        return m
    strip = (fd["sid"] == 1) & taps_all(2)
    floor = (fd["sid"] == 0) & taps_all(0)
    wall = (fd["sid"] == 1) & taps_all(1)
    print("(d) strip %d pixels, floor %d, wall %d" % (strip.sum(), floor.sum(), wall.sum()))
    assert strip.sum() >= 20 and floor.sum() >= 500 and wall.sum() >= 500
    assert np.all(nxt[..., 3][strip] == 1.0)
    assert np.all(nxt[..., 3][floor] > 1.0) and np.all(nxt[..., 3][wall] > 1.0)


def test_reference_dead_pixels(ref, views):
    """(e) pixels that are not live (a miss block, one NaN colour, one NaN normal) pass through bit for bit with len 0, and they
    are never taps: poisoning their records in hist_prev changes no pixel of the next frame"""
    A, B = views["A"], views["B"]
    fa = make_frame(A["pos"], A["dirs"], W0, H0, seed=1)
    true_normal, true_t = fa["normal"].copy(), fa["t"].copy()
    dead = poison(fa)
    assert dead.sum() == 8 and np.array_equal(dead, ~live_mask(fa))
    hist, out = reference(ref, A["cam"], A["cam"], A["dirs"], A["dirs"], fa, None)
    assert np.array_equal(_bits(out[dead]), _bits(fa["rgb"][dead]))
    assert np.array_equal(_bits(hist[dead][:, 0:3]), _bits(fa["rgb"][dead])) and np.all(hist[dead][:, 3] == 0.0)
    assert np.array_equal(_bits(hist[dead][:, 4:7]), _bits(fa["normal"][dead])) and np.array_equal(_bits(hist[dead][:, 7]), _bits(fa["t"][dead]))
    assert np.all(hist[~dead][:, 3] == 1.0)
    fb = make_frame(B["pos"], B["dirs"], W0, H0, seed=2)
    base = reference(ref, B["cam"], A["cam"], B["dirs"], A["dirs"], fb, hist)
    assert (base[0][..., 3] > 1).sum() > W0 * H0 // 2
    for kind in range(3):
        bad = hist.copy()
        if kind == 0:      # huge finite colours, len stays 0
            bad[dead, 0:3] = 1e30
        elif kind == 1:    # the whole record NaN
            bad[dead] = np.nan
        else:              # a positive len on a record with one infinite value
            bad[dead, 3] = 5.0
            bad[dead, 0] = np.inf
        got = reference(ref, B["cam"], A["cam"], B["dirs"], A["dirs"], fb, bad)
        assert np.array_equal(_bits(got[0]), _bits(base[0])) and np.array_equal(_bits(got[1]), _bits(base[1])), kind
    # the control: the same records made usable, on their surfaces, are taps
    bad = hist.copy()
    bad[dead, 0:3] = 1e3
    bad[dead, 3] = 5.0
    bad[dead, 4:7] = true_normal[dead]
    bad[dead, 7] = true_t[dead]
    got = reference(ref, B["cam"], A["cam"], B["dirs"], A["dirs"], fb, bad)
    assert not np.array_equal(_bits(got[1]), _bits(base[1]))


# ---- the pipeline's prediction (CPU oracle)

POSES = [(0.0, 0.0, 15.0, float(f)) for f in range(8)]  # the Cornell box's camera yawing 1 degree per frame


def _oracle_guides(sc, frame, pos, dirs, w, h):
    """normal (geometric, facing the camera), albedo and t of an oracle frame, in crt_frame_guides' layout"""
    normal, albedo = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    t = np.where(frame["hit_inst"] == 0xFFFFFFFF, T_MISS, frame["hit_t"]).astype(np.float32)
    d = dirs.reshape(h, w, 3).astype(np.float64)
    for m, mesh in enumerate(sc["meshes"]):
        V = np.asarray(mesh["vertices"], np.float64)
        T = np.asarray(mesh["triangles"], np.int64)
        ng = np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]])
        ng /= np.linalg.norm(ng, axis=1, keepdims=True)
        sel = frame["hit_inst"] == m
        n = ng[frame["hit_prim"][sel]]
        n = np.where((n * d[sel]).sum(-1, keepdims=True) > 0, -n, n)
        normal[sel] = n
        albedo[sel] = sc["materials"][mesh["material_index"]]["albedo"]
    return normal, albedo, t


def _rmse(a, b):
    return float(np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean()))


def test_pipeline_prediction(ref, oracle, scenes):
    """The ratio the GPU pipeline test is capped by, predicted on the CPU: the oracle's mode-200 frames of the Cornell box (48 x
    48, 3 bounces, 4 spp, seed 1234 + f, eight poses yawing 1 degree per frame) with the geometric normals, albedo and t of the pixel-centre rays (a mode-3 frame) as guides, pushed through
    tests/temporal_reference.c with the defaults.  RMSE(accumulated last frame) / RMSE(last 4-spp frame) against the 1024-spp
    frame of the last pose: the prediction must stay below 0.75 and is the one PIPELINE_CAP was computed from."""
    w = h = 48
    sc = scenes.cornell_box()
    o = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    hist, prev = None, None
    try:
        for f, (x, y, z, yaw) in enumerate(POSES):
            rot = yaw_matrix(yaw, scenes)
            dirs = oracle_dirs(oracle, rot, w, h)
            oracle.set_path_params(4, 3, 1234 + f)
            fr = o.render((x, y, z), rot, 200, w, h)
            centre = o.render((x, y, z), rot, 3, w, h, want=("hit_inst", "hit_prim", "hit_t"))  # the pixel-centre rays' hits
            normal, albedo, t = _oracle_guides(sc, centre, (x, y, z), dirs, w, h)
            cam = camera((x, y, z), rot)
            frame = {"rgb": fr["rgb"], "normal": normal, "albedo": albedo, "t": t}
            hist, out = reference(ref, cam, cam if prev is None else prev[0], dirs, dirs if prev is None else prev[1], frame, hist)
            prev = (cam, dirs)
        oracle.set_path_params(1024, 3, 1234)
        clean = o.render((x, y, z), rot, 200, w, h, want=("rgb",))["rgb"]
    finally:
        oracle.set_path_params(4, 3, 1234)
        o.close()
    ratio = _rmse(out, clean) / _rmse(fr["rgb"], clean)
    print("pipeline prediction: RMSE 4 spp %.4f, accumulated %.4f, ratio %.4f; mean len %.2f" %
          (_rmse(fr["rgb"], clean), _rmse(out, clean), ratio, float(hist[..., 3].mean())))
    assert ratio < 0.75, ratio
    assert abs(ratio - PIPELINE_PREDICTION) < 5e-4, (ratio, PIPELINE_PREDICTION)


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _device(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def _device_dirs(renderer, cam, w, h):
    """the directions of the pixel-centre rays of that camera, from crt_camera_rays"""
    renderer.set_camera(cam[:3], cam[3:])
    return np.ascontiguousarray(renderer.camera_rays(w, h)[:, 4:7])


def _pairs(scenes):
    """(name, cam_cur, cam_prev): bitwise equal, the small move, the 180 degree turn"""
    a = camera(POS_A, yaw_matrix(0.0, scenes))
    return (("equal", a, a.copy()), ("move", camera(POS_B, yaw_matrix(2.0, scenes)), a), ("turn", camera(POS_A, yaw_matrix(180.0, scenes)), a))


def _run_device(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, prm, out_is_rgb=False):
    d_rgb = d["rgb"].clone() if out_is_rgb else d["rgb"]
    d_next = torch.full((h, w, 8), -7.0, dtype=torch.float32, device="cuda")
    d_out = d_rgb if out_is_rgb else torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.temporal_accumulate_device(w, h, cam_cur, cam_prev, d_rgb.data_ptr(), d["normal"].data_ptr(),
                                        d["albedo"].data_ptr() if prm["demodulate"] else None, d["t"].data_ptr(),
                                        None if d_hist is None else d_hist.data_ptr(), d_next.data_ptr(), d_out.data_ptr(), **prm)
    renderer.synchronize()
    return d_next.cpu().numpy(), d_out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (1, 70), (130, 5), (37, 23), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_reference(pkg, scenes, ref, renderer, size):
    """hist_next and out of the device form equal the C reference's bits, for the three camera pairs, demodulate 0 and 1, with
    and without history (the history: the reference's output of an earlier frame with the poisoned pixels; directions from
    crt_camera_rays with each camera set); the host form, out aliased to rgb and a second call give the same bits."""
    import torch
    w, h = size
    with_history = 0
    for name, cam_cur, cam_prev in _pairs(scenes):
        dir_cur, dir_prev = _device_dirs(renderer, cam_cur, w, h), _device_dirs(renderer, cam_prev, w, h)
        f0 = make_frame(cam_prev[:3], dir_prev, w, h, seed=11)
        poison(f0)
        f1 = make_frame(cam_cur[:3], dir_cur, w, h, seed=12)
        poison(f1)
        d = {k: _device(torch, f1[k]) for k in ("rgb", "normal", "albedo", "t")}
        for demodulate in (0, 1):
            prm = dict(DEFAULTS, demodulate=demodulate)
            hist0, _ = reference(ref, cam_prev, cam_prev, dir_prev, dir_prev, f0, None, **prm)
            hist0[..., 3] = np.where(hist0[..., 3] > 0, np.float32(3.0), hist0[..., 3])
            for hist_prev in (None, hist0):
                what = "%dx%d %s demodulate %d history %s" % (w, h, name, demodulate, hist_prev is not None)
                want = reference(ref, cam_cur, cam_prev, dir_cur, dir_prev, f1, hist_prev, **prm)
                d_hist = None if hist_prev is None else _device(torch, hist_prev)
                got = _run_device(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, prm)
                assert np.array_equal(_bits(got[0]), _bits(want[0])), what + ": hist_next"
                assert np.array_equal(_bits(got[1]), _bits(want[1])), what + ": out"
                host = renderer.temporal_accumulate(cam_cur, cam_prev, f1["rgb"], f1["normal"], f1["albedo"] if demodulate else None, f1["t"],
                                                    hist_prev, **prm)
                assert np.array_equal(_bits(host[0]), _bits(want[0])) and np.array_equal(_bits(host[1]), _bits(want[1])), what + ": host form"
                for again in ("in place", "second call"):
                    got = _run_device(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, prm, out_is_rgb=again == "in place")
                    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])), what + ": " + again
                if hist_prev is not None:
                    with_history += int((want[0][..., 3] > 1).sum())
    if w * h >= 64:
        assert with_history > 0, "some pixel took history"
    print("%dx%d: %d pixel results with history" % (w, h, with_history))


@pytest.mark.gpu
def test_three_chained_frames(pkg, scenes, ref, renderer):
    """three frames along a three-pose path, chained through two swapped device buffers, equal the reference chained the same way"""
    import torch
    w, h = 37, 23
    cams = [camera(POS_A, yaw_matrix(0.0, scenes)), camera(POS_B, yaw_matrix(2.0, scenes)), camera((0.3, 0.62, 2.1), yaw_matrix(4.0, scenes))]
    dirs = [_device_dirs(renderer, c, w, h) for c in cams]
    d_hist = [torch.zeros((h, w, 8), dtype=torch.float32, device="cuda") for _ in range(2)]
    hist_ref, lens = None, []
    for k in range(3):
        f = make_frame(cams[k][:3], dirs[k], w, h, seed=20 + k)
        poison(f)
        d = {g: _device(torch, f[g]) for g in ("rgb", "normal", "albedo", "t")}
        d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        prev = max(k - 1, 0)
        torch.cuda.synchronize()
        renderer.temporal_accumulate_device(w, h, cams[k], cams[prev], d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(),
                                            d["t"].data_ptr(), d_hist[k & 1].data_ptr() if k else None, d_hist[(k & 1) ^ 1].data_ptr(),
                                            d_out.data_ptr())
        renderer.synchronize()
        hist_ref, out_ref = reference(ref, cams[k], cams[prev], dirs[k], dirs[prev], f, hist_ref)
        assert np.array_equal(_bits(d_hist[(k & 1) ^ 1].cpu().numpy()), _bits(hist_ref)), k
        assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(out_ref)), k
        lens.append(float(hist_ref[..., 3].max()))
    assert all(abs(l - (k + 1)) < 1e-3 for k, l in enumerate(lens)), lens


@pytest.mark.gpu
def test_errors(pkg, scenes, ref, renderer):
    """every CRT_EINVAL case launches nothing and leaves hist_next and out untouched; a context without a scene works"""
    import torch
    L = pkg.lib()
    w, h = 16, 8
    cam = camera(POS_A, yaw_matrix(0.0, scenes))
    dirs = _device_dirs(renderer, cam, w, h)
    f = make_frame(cam[:3], dirs, w, h, seed=3)
    names = ("rgb", "normal", "albedo", "t")
    host_in = {g: np.ascontiguousarray(f[g], np.float32) for g in names}
    d = {g: _device(torch, f[g]) for g in names}
    sentinel = -5.0
    d_hist_prev = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    d_next = torch.full((w * h * 8 + 8,), sentinel, dtype=torch.float32, device="cuda")
    d_out = torch.full((w * h * 3 + 4,), sentinel, dtype=torch.float32, device="cuda")
    next_h, out_h = np.full((h, w, 8), sentinel, np.float32), np.full((h, w, 3), sentinel, np.float32)
    hist_prev_h = np.zeros((h, w, 8), np.float32)
    K = cam.ctypes.data
    torch.cuda.synchronize()

    def dev(prm=None, w_=w, h_=h, **over):
        a = {g: d[g].data_ptr() for g in names}
        a.update(cur=K, prev=K, hist_prev=d_hist_prev.data_ptr(), hist_next=d_next.data_ptr(), out=d_out.data_ptr())
        a.update(over)
        return L.crt_temporal_accumulate_device(renderer.h, w_, h_, a["cur"], a["prev"], a["rgb"], a["normal"], a["albedo"], a["t"], a["hist_prev"],
                                                a["hist_next"], a["out"], C.byref(prm) if prm else None, None)

    def host(prm=None, w_=w, h_=h, **over):
        a = {g: host_in[g].ctypes.data for g in names}
        a.update(cur=K, prev=K, hist_prev=hist_prev_h.ctypes.data, hist_next=next_h.ctypes.data, out=out_h.ctypes.data)
        a.update(over)
        return L.crt_temporal_accumulate(renderer.h, w_, h_, a["cur"], a["prev"], a["rgb"], a["normal"], a["albedo"], a["t"], a["hist_prev"],
                                         a["hist_next"], a["out"], C.byref(prm) if prm else None, None)

    nan = float("nan")
    bad = [pkg.TemporalParams(alpha=v) for v in (-0.1, 1.5, nan)] + [pkg.TemporalParams(depth_tolerance=v) for v in (0.0, -1.0, nan)]
    bad += [pkg.TemporalParams(normal_threshold=nan), pkg.TemporalParams(max_history=0), pkg.TemporalParams(max_history=(1 << 24) + 1),
            pkg.TemporalParams(demodulate=2)]
    for prm in bad:
        assert dev(prm) == EINVAL and host(prm) == EINVAL
    assert dev(w_=0) == EINVAL and host(w_=0) == EINVAL and dev(h_=0) == EINVAL and host(h_=0) == EINVAL
    assert dev(w_=1 << 15, h_=1 << 14) == EINVAL and host(w_=1 << 15, h_=1 << 14) == EINVAL
    for g in ("cur", "prev", "rgb", "normal", "t", "hist_next", "albedo"):
        assert dev(**{g: None}) == EINVAL and host(**{g: None}) == EINVAL, g
    for g in names:
        assert dev(**{g: d[g].data_ptr() + 2}) == EINVAL, g
    assert dev(out=d_out.data_ptr() + 2) == EINVAL
    assert dev(hist_next=d_next.data_ptr() + 8) == EINVAL and dev(hist_prev=d_hist_prev.data_ptr() + 4) == EINVAL
    assert "aligned" in L.crt_last_error(renderer.h).decode()
    torch.cuda.synchronize()
    assert bool((d_next == sentinel).all().item()) and bool((d_out == sentinel).all().item())
    assert np.all(next_h == sentinel) and np.all(out_h == sentinel)
    # the controls: NULL albedo without demodulation, NULL out, NULL history, the extreme parameters
    assert dev(pkg.TemporalParams(demodulate=0), albedo=None, out=None) == 0
    torch.cuda.synchronize()
    assert not bool((d_next[:w * h * 8] == sentinel).any().item()) and bool((d_out == sentinel).all().item())
    assert dev(pkg.TemporalParams(alpha=1.0, max_history=1 << 24, normal_threshold=-2.0), hist_prev=None) == 0
    assert host(pkg.TemporalParams(alpha=0.0, max_history=1)) == 0
    torch.cuda.synchronize()
    assert not bool((d_out[:w * h * 3] == sentinel).any().item()) and bool((d_out[w * h * 3:] == sentinel).all().item())
    assert bool((d_next[w * h * 8:] == sentinel).all().item())
    assert not np.any(next_h == sentinel) and not np.any(out_h == sentinel)
    st = renderer.temporal_accumulate_device(w, h, cam, cam, d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(),
                                             None, d_next.data_ptr(), d_out.data_ptr(), stats=True)
    assert st["kernel_ms"] > 0.0 and st["total_ms"] > 0.0
    assert not any(st[k] for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested"))
    fresh = pkg.Renderer(0)
    try:
        got = fresh.temporal_accumulate(cam, cam, f["rgb"], f["normal"], f["albedo"], f["t"])
        want = reference(ref, cam, cam, dirs, dirs, f, None)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    finally:
        fresh.close()


@pytest.mark.gpu
def test_pipeline(pkg, scenes, renderer):
    """Cornell box 48 x 48, 3 bounces, 4 spp, eight poses yawing 1 degree per frame, seed 1234 + f, guides from crt_frame_guides,
    pushed through TemporalHistory with the defaults: RMSE(accumulated last frame) / RMSE(last 4-spp frame), both against the
    1024-spp frame of the last pose, stays under PIPELINE_CAP = 1.25 x the ratio predicted on the CPU (test_pipeline_prediction;
    the margin covers shading normals against the oracle's geometric normals).  Predicted 0.6363, cap 0.7954,
    observed on the MI355X: 0.6363 (RMSE 0.1139 for the 4-spp frame, 0.0725 accumulated; the path tracer follows the oracle's
    operation order and the box's shading normals are its geometric ones).  A mode-200 frame rendered after the pushes equals the
    one rendered before them bit for bit, with accumulation on as well."""
    w = h = 48
    sc = scenes.cornell_box()
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"))
    th = pkg.TemporalHistory(renderer, w, h)
    try:
        renderer.change_shading_mode(200)

        def frame(f, spp=4, seed=None):
            x, y, z, yaw = POSES[f]
            renderer.set_camera((x, y, z), yaw_matrix(yaw, scenes))
            renderer.set_path_params(spp, 3, 1234 + f if seed is None else seed)
            return renderer.render_frame(w, h, want=("rgba8", "rgb"))["rgb"]
        before = frame(0)
        renderer.set_accumulation(1 << 24)
        acc = [frame(0), frame(0)]
        renderer.set_accumulation(0)
        for f in range(len(POSES)):
            noisy = frame(f)
            g = renderer.frame_guides(w, h)
            out = th.push(noisy, g["normal"], g["albedo"], g["t"])
            assert out.shape == (h, w, 3) and out.dtype == np.float32
        lens = th.records[..., 3].cpu().numpy()
        clean = frame(len(POSES) - 1, spp=1024, seed=1234)
        assert np.array_equal(_bits(frame(0)), _bits(before)), "a frame after the pushes"
        renderer.set_accumulation(1 << 24)
        again = [frame(0), frame(0)]
        assert renderer.accumulated_samples() == 8
        renderer.set_accumulation(0)
        assert np.array_equal(_bits(again[0]), _bits(acc[0])) and np.array_equal(_bits(again[1]), _bits(acc[1])), "accumulating frames"
        th.reset()
        first = th.push(noisy, g["normal"], g["albedo"], g["t"])
        assert np.all(th.records[..., 3].cpu().numpy() <= 1.0), "reset() drops the history"
        live = th.records[..., 3].cpu().numpy() == 1.0
        assert np.allclose(first[live], noisy[live], rtol=1e-6, atol=1e-7)
    finally:
        renderer.set_accumulation(0)
        renderer.set_path_params(4, 3, 1234)
        renderer.change_shading_mode(0)
    ratio = _rmse(out, clean) / _rmse(noisy, clean)
    print("pipeline: RMSE against 1024 spp: 4 spp %.4f, accumulated %.4f, ratio %.4f (cap %.4f); mean len %.2f, max %.0f" %
          (_rmse(noisy, clean), _rmse(out, clean), ratio, PIPELINE_CAP, float(lens.mean()), float(lens.max())))
    assert lens.max() > len(POSES) - 0.5
    assert ratio < PIPELINE_CAP, (ratio, PIPELINE_CAP)


@pytest.mark.gpu
def test_cpp_layer(pkg, scenes, ref, renderer, tmp_path):
    """crt::Renderer::temporalAccumulate, from a small C++ program linked against libcrt_hip.so, gives the C ABI's bits on the 37
    x 23 case (the small move, with history); crt_render --temporal writes accumulated frames and refuses other modes."""
    exe = str(tmp_path / "temporal_cpp")
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    csrc = os.path.join(lib_dir, "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + csrc,
                           "-o", exe, os.path.join(ROOT, "tests", "temporal_cpp.cpp"), "-L" + lib_dir, "-lcrt_hip",
                           "-Wl,-rpath," + lib_dir, "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    w, h = 37, 23
    _, cam_cur, cam_prev = _pairs(scenes)[1]
    dir_cur, dir_prev = _device_dirs(renderer, cam_cur, w, h), _device_dirs(renderer, cam_prev, w, h)
    f0 = make_frame(cam_prev[:3], dir_prev, w, h, seed=11)
    poison(f0)
    f1 = make_frame(cam_cur[:3], dir_cur, w, h, seed=12)
    poison(f1)
    hist0, _ = reference(ref, cam_prev, cam_prev, dir_prev, dir_prev, f0, None)
    want = renderer.temporal_accumulate(cam_cur, cam_prev, f1["rgb"], f1["normal"], f1["albedo"], f1["t"], hist0)
    assert (want[0][..., 3] > 1).sum() > w * h // 2
    scene = pkg.Scene.from_arrays(scenes.cornell_box())
    path = str(tmp_path / "cornell.crtbin")
    scene.save(path)
    scene.close()
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.ascontiguousarray(a, np.float32).reshape(-1) for a in
                    (cam_cur, cam_prev, f1["rgb"], f1["normal"], f1["albedo"], f1["t"], hist0)]).tofile(src)
    subprocess.check_call([exe, path, str(w), str(h), src, out], timeout=120)
    raw = np.fromfile(out, dtype=np.float32)
    assert raw.size == 11 * w * h
    assert np.array_equal(_bits(raw[:8 * w * h]), _bits(want[0]).reshape(-1)) and np.array_equal(_bits(raw[8 * w * h:]), _bits(want[1]).reshape(-1))

    tool = os.path.join(lib_dir, "crt_render")
    base = [tool, path, "--size", "40x24", "--spp", "2", "--frames", "3", "--orbit", "1"]
    subprocess.check_call(base + ["--mode", "200", "--out", str(tmp_path / "plain")], timeout=120, stdout=subprocess.DEVNULL)
    subprocess.check_call(base + ["--mode", "200", "--temporal", "--out", str(tmp_path / "acc")], timeout=120, stdout=subprocess.DEVNULL)
    assert open(str(tmp_path / "plain_2.ppm"), "rb").read() != open(str(tmp_path / "acc_2.ppm"), "rb").read()
    assert subprocess.run(base + ["--mode", "100", "--temporal"], capture_output=True, timeout=60).returncode == 2
    assert subprocess.run(base + ["--mode", "200", "--temporal", "--temporal-alpha", "2"], capture_output=True, timeout=60).returncode == 2
