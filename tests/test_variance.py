"""SVGF variance (crt_temporal_variance*, crt_denoise_variance*; include/crt_hip.h, "variance"): luminance moments carried with the
temporal history, a per-pixel variance from them, and the a-trous filter whose luminance weight follows that variance.

tests/variance_reference.c restates the temporal contract (steps 1 to 12, 4' to 9', V1 to V6) in plain C, compiled here with -O2
-ffp-contract=off; it takes the ray directions as arrays.  On the CPU it is pinned to what it means on the analytic scene of
tests/test_temporal.py; on the GPU the kernels equal it bit for bit.  tests/variance_reference.py restates the filter in numpy; the
device filter is held to its float64 run by the project's rule, 16 x the deviation of its float32 run, capped at 1e-4.

The pipeline's figures are in test_pipeline_prediction's and test_pipeline's docstrings and in DESIGN.md section 5j."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as R  # noqa: E402
import test_temporal as TT  # noqa: E402
import variance_reference as V  # noqa: E402
from test_temporal import views  # noqa: E402,F401  (the cameras of the CPU tests, a module fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("crt_temporal_variance_device", "crt_temporal_variance", "crt_denoise_variance_device", "crt_denoise_variance")
EINVAL = 1
GUIDES = ("rgb", "normal", "albedo", "t")
DEFAULTS = dict(TT.DEFAULTS, alpha_moments=0.2, min_history=4)
FILTER_DEFAULTS = {"iterations": 5, "sigma_luminance": 0.0625, "sigma_normal": 0.3, "sigma_depth": 0.05, "demodulate": 1}
TOL_FACTOR, TOL_CAP = 16.0, 1e-4  # tests/test_denoise.py's
W0, H0 = TT.W0, TT.H0
LUMA = np.float32([0.2126, 0.7152, 0.0722])
EPS = 2.0 ** -24  # the unit roundoff of float32
# the pipeline: the ratio predicted on the CPU (test_pipeline_prediction), the two it has to beat, and the cap of the GPU test
PIPELINE_PREDICTION = 0.6360
TEMPORAL_ALONE = TT.PIPELINE_PREDICTION
PIPELINE_CAP = 1.25 * PIPELINE_PREDICTION

_bits = TT._bits
_rmse = TT._rmse
camera = TT.camera


# ---- the references

def _compile(tmp, name):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for tests/%s.c" % name)
    out = str(tmp / ("lib%s.so" % name))
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(ROOT, "tests", name + ".c"),
                           "-o", out, "-lm"])
    return C.CDLL(out)


@pytest.fixture(scope="session")
def vref(tmp_path_factory):
    """variance_reference.c, with temporal_reference.c and motion_reference.c beside it for step V3's consequence"""
    tmp = tmp_path_factory.mktemp("variance_reference")
    L = _compile(tmp, "variance_reference")
    L.variance_temporal_reference.restype = None
    L.variance_temporal_reference.argtypes = ([C.c_uint32, C.c_uint32] + [C.c_void_p] * 16 + [C.c_float] * 3 + [C.c_uint32, C.c_uint32, C.c_float,
                                                                                                      C.c_uint32])
    tail = [C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32]
    L.plain = _compile(tmp, "temporal_reference")
    L.plain.temporal_reference.restype = None
    L.plain.temporal_reference.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 11 + tail
    L.motion = _compile(tmp, "motion_reference")
    L.motion.motion_temporal_reference.restype = None
    L.motion.motion_temporal_reference.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 12 + tail
    return L


def _p(a):
    return None if a is None else a.ctypes.data


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def reference(L, cam_cur, cam_prev, dir_cur, dir_prev, frame, hist_prev=None, mom_prev=None, prev_point=None, **params):
    """one call of variance_temporal_reference: a dict of hist (h, w, 8), mom (h, w, 2), var (h, w), out (h, w, 3) and count (h, w),
    the debug return"""
    prm = dict(DEFAULTS, **params)
    h, w = frame["t"].shape
    a = {k: _f32(frame[k]) for k in GUIDES}
    cc, cp, dc, dp = _f32(cam_cur), _f32(cam_prev), _f32(dir_cur), _f32(dir_prev)
    assert cc.size == 12 and cp.size == 12 and dc.size == 3 * w * h and dp.size == 3 * w * h
    hp, mp, pp = _f32(hist_prev), _f32(mom_prev), _f32(prev_point)
    assert (hp is None) == (mp is None)
    r = {"hist": np.zeros((h, w, 8), np.float32), "mom": np.zeros((h, w, 2), np.float32), "var": np.zeros((h, w), np.float32),
         "out": np.zeros((h, w, 3), np.float32), "count": np.zeros((h, w), np.float32)}
    L.variance_temporal_reference(w, h, _p(cc), _p(cp), _p(dc), _p(dp), _p(a["rgb"]), _p(a["normal"]), _p(a["albedo"]) if prm["demodulate"] else None,
                                  _p(a["t"]), _p(pp), _p(hp), _p(r["hist"]), _p(mp), _p(r["mom"]), _p(r["var"]), _p(r["out"]), _p(r["count"]),
                                  prm["alpha"], prm["depth_tolerance"], prm["normal_threshold"], prm["max_history"], prm["demodulate"],
                                  prm["alpha_moments"], prm["min_history"])
    return r


def parent_reference(L, cam_cur, cam_prev, dir_cur, dir_prev, frame, hist_prev, prev_point, **params):
    """temporal_reference.c (prev_point None) or motion_reference.c: (hist_next, out)"""
    prm = dict(TT.DEFAULTS, **params)
    h, w = frame["t"].shape
    a = {k: _f32(frame[k]) for k in GUIDES}
    hist, out = np.zeros((h, w, 8), np.float32), np.zeros((h, w, 3), np.float32)
    head = [w, h, _p(_f32(cam_cur)), _p(_f32(cam_prev)), _p(_f32(dir_cur)), _p(_f32(dir_prev)), _p(a["rgb"]), _p(a["normal"]),
            _p(a["albedo"]) if prm["demodulate"] else None, _p(a["t"])]
    hp, pp = _f32(hist_prev), _f32(prev_point)
    tail = [_p(hp), _p(hist), _p(out), prm["alpha"], prm["depth_tolerance"], prm["normal_threshold"], prm["max_history"], prm["demodulate"]]
    if pp is None:
        L.plain.temporal_reference(*(head + tail))
    else:
        L.motion.motion_temporal_reference(*(head + [_p(pp)] + tail))
    return hist, out


def luminance64(c32):
    """the luminance of float32 colours, evaluated in float64 with the contract's float32 constants"""
    return (np.asarray(c32, np.float64) * LUMA.astype(np.float64)).sum(-1)


# ---- CPU: the interface

def test_binding_and_library_expose_the_new_entry_points(pkg):
    L = pkg.lib()
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
        assert ("int %s(" % s) in header, s
    assert "crt_temporal_variance_params" in header and "crt_denoise_variance_params" in header
    for name in ("temporal_variance", "temporal_variance_device", "denoise_variance", "denoise_variance_device"):
        assert callable(getattr(pkg.Renderer, name, None)), name
    assert C.sizeof(pkg.TemporalVarianceParams) == 28 and C.sizeof(pkg.DenoiseVarianceParams) == 20
    d = pkg.TemporalVarianceParams()
    assert (d.base.max_history, d.base.demodulate, d.min_history) == (64, 1, DEFAULTS["min_history"])
    assert np.float32(d.base.alpha) == np.float32(0.1) and np.float32(d.alpha_moments) == np.float32(DEFAULTS["alpha_moments"])
    assert np.float32(pkg.TemporalVarianceParams(alpha=0.3).base.alpha) == np.float32(0.3)
    f = pkg.DenoiseVarianceParams()
    assert (f.iterations, f.demodulate) == (FILTER_DEFAULTS["iterations"], 1)
    assert np.float32(f.sigma_luminance) == np.float32(FILTER_DEFAULTS["sigma_luminance"])
    assert np.float32(f.sigma_normal) == np.float32(0.3) and np.float32(f.sigma_depth) == np.float32(0.05)
    assert V.DEFAULTS == FILTER_DEFAULTS
    buf, hist, mom, cam = (np.zeros(64, dtype=np.float32) for _ in range(4))
    P, Hn, M, K = buf.ctypes.data, hist.ctypes.data, mom.ctypes.data, cam.ctypes.data
    assert L.crt_temporal_variance(None, 2, 2, K, K, P, P, P, P, None, None, Hn, None, M, P, P, None, None) == EINVAL
    assert L.crt_temporal_variance_device(None, 2, 2, K, K, P, P, P, P, None, None, Hn, None, M, P, P, None, None) == EINVAL
    assert L.crt_denoise_variance(None, 2, 2, P, P, P, P, P, P, P, None, None) == EINVAL
    assert L.crt_denoise_variance_device(None, 2, 2, P, P, P, P, P, P, P, None, None) == EINVAL
    assert not buf.any() and not hist.any() and not mom.any()
    th = pkg.TemporalHistory.__init__.__code__.co_varnames
    assert "variance" in th


# ---- CPU: variance_reference.c pinned to its meaning

def test_reference_static_camera_is_the_population_variance(vref, views):
    """(a) static camera, alpha = alpha_moments = 0, 6 frames with uniform +-0.1 noise on each channel: from frame min_history = 4
    on the variance of every pixel is the float64 population variance of its k luminances, within a bound from float32 rounding.

    The bound.  eps = 2^-24, X = the largest of the pixel's luminances (all are positive here).  l is two fmaf and a product of
    positive terms, each rounding at most eps X: |dl| <= 3 eps X; q = l * l: |dq| <= (2 * 3 + 1) eps X^2.  With a_m = 1 / k exactly
    the weight of a running mean and the static camera's single tap of weight 1, a step m = fmaf(a_m, l - h, h) rounds three times
    (1 / k, the difference, the fmaf), each at most eps times the magnitude at hand, and carries earlier errors with weight <= 1:
    after k frames |dm1| <= (3 k + 3) eps X, |dm2| <= (3 k + 7) eps X^2.  variance = m2 - m1 * m1 rounds the product and the
    difference, at most eps X^2 each, and takes 2 X |dm1| + |dm2| from its inputs (the square of dm1 is far below eps):
    |dvariance| <= ((3 k + 7) + 2 (3 k + 3) + 2) eps X^2 = (9 k + 15) eps X^2.  fmaxf(., 0) only moves a value towards a true
    variance, which is >= 0."""
    A = views["A"]
    K, cap = 6, DEFAULTS["min_history"]
    frames = [TT.make_frame(A["pos"], A["dirs"], W0, H0, seed=300 + k, noise=0.1) for k in range(K)]
    assert TT.live_mask(frames[0]).all()
    hist = mom = None
    lums, worst = [], 0.0
    for k, f in enumerate(frames, 1):
        r = reference(vref, A["cam"], A["cam"], A["dirs"], A["dirs"], f, hist, mom, alpha=0.0, alpha_moments=0.0)
        hist, mom = r["hist"], r["mom"]
        c = f["rgb"] / np.maximum(f["albedo"], np.float32(1e-3))  # step 2, in float32
        assert c.dtype == np.float32
        lums.append(luminance64(c))
        assert lums[-1].min() > 0.0
        assert np.array_equal(hist[..., 3], np.full((H0, W0), np.float32(k)))
        if k < cap:
            assert (r["count"] >= 1).all(), "the spatial branch ran"
            continue
        assert not r["count"].any(), "the long branch everywhere"
        want = np.var(np.stack(lums), axis=0)  # population variance, float64
        bound = (9 * k + 15) * EPS * np.max(np.stack(lums), axis=0) ** 2
        err = np.abs(r["var"].astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (k, float((err / bound).max()))
        assert want.mean() > 1e-3, "there is a variance to measure"
    print("(a) worst error / bound: %.3f" % worst)


def _flat_noisy(V0, seed):
    """the analytic scene's geometry from camera V0 with a flat colour 0.5 and uniform +-0.1 noise on each channel"""
    f = TT.make_frame(V0["pos"], V0["dirs"], W0, H0)
    f["rgb"] = (0.5 + np.random.default_rng(seed).uniform(-0.1, 0.1, size=f["rgb"].shape)).astype(np.float32)
    return f


def _same_surface_count(sid):
    """per pixel the number of pixels of its 7 x 7 window that lie inside the image on the pixel's own surface"""
    n = np.zeros(sid.shape)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            q, inside = R._shifted(sid, dx, dy, fill=-1)
            n += inside & (q == sid)
    return n


def test_reference_first_frame_is_the_spatial_estimate(vref, views):
    """(b) a first frame (len 1 < min_history) takes the spatial branch everywhere.  Flat colour 0.5 with uniform +-0.1 noise on
    each channel, no demodulation: the luminance noise has variance s2 = (0.1^2 / 3) sum w_c^2, and the population variance of N =
    49 window samples has the expectation s2 (N - 1) / N.  Over the M floor pixels whose window counts all 49 taps, the mean of
    variance / min_history must lie within 5 standard errors of that.  The standard error: the variance of one window's estimate
    is ((N - 1)^2 / N^3) (mu4 - s2^2 (N - 3) / (N - 1)), with mu4 = 3 s2^2 - (2 a^4 / 15) sum w_c^4 for the weighted sum of three
    uniforms of half-width a; neighbouring windows overlap, so only M / N of them are taken as independent.
    (c) the window does not cross the pillar / wall step (equal normals, depths 3 apart) nor the floor / wall crease (normals at
    a right angle): N, from the reference's debug return, is the number of window pixels on the pixel's own surface."""
    A = views["A"]
    f = _flat_noisy(A, 41)
    mh = DEFAULTS["min_history"]
    r = reference(vref, A["cam"], A["cam"], A["dirs"], A["dirs"], f, demodulate=0)
    assert np.all(r["hist"][..., 3] == 1.0) and np.all(r["count"] >= 1.0)
    assert np.allclose(r["mom"][..., 0], luminance64(f["rgb"]), rtol=1e-6, atol=0) and np.allclose(r["mom"][..., 1], luminance64(f["rgb"]) ** 2, rtol=1e-6)
    # (c)
    want_n = _same_surface_count(f["sid"])
    assert np.array_equal(r["count"], want_n.astype(np.float32))
    inner = np.zeros((H0, W0), bool)
    inner[3:-3, 3:-3] = True
    fewer = inner & (r["count"] < 49)
    print("(c) %d pixels away from the frame's border count fewer than 49 taps; least %d" % (fewer.sum(), r["count"].min()))
    assert fewer.sum() > 100 and set(np.unique(f["sid"][fewer])) == {0, 1, 2}
    # (b)
    N, a = 49.0, 0.1
    w2, w4 = float((LUMA.astype(np.float64) ** 2).sum()), float((LUMA.astype(np.float64) ** 4).sum())
    s2 = a * a / 3.0 * w2
    mu4 = 3.0 * s2 * s2 - 2.0 * a ** 4 / 15.0 * w4
    var_one = (N - 1) ** 2 / N ** 3 * (mu4 - s2 * s2 * (N - 3) / (N - 1))
    sel = (f["sid"] == 0) & (r["count"] == 49)
    M = int(sel.sum())
    assert M > 1000
    got = float(r["var"][sel].astype(np.float64).mean()) / mh
    want = s2 * (N - 1) / N
    bound = 5.0 * np.sqrt(var_one / (M / N))
    print("(b) %d floor pixels: mean variance / min_history %.6g, expected %.6g, bound %.3g" % (M, got, want, bound))
    assert abs(got - want) <= bound, (got, want, bound)
    # the factor min_history / len itself: the same frame with min_history 8 gives twice the value
    r8 = reference(vref, A["cam"], A["cam"], A["dirs"], A["dirs"], f, demodulate=0, min_history=8)
    assert np.array_equal(_bits(r8["var"]), _bits(r["var"] * np.float32(2.0)))


def _history(vref, Vw, seed, demodulate=1):
    f = TT.make_frame(Vw["pos"], Vw["dirs"], W0, H0, seed=seed)
    return f, reference(vref, Vw["cam"], Vw["cam"], Vw["dirs"], Vw["dirs"], f, demodulate=demodulate)


def test_reference_with_finite_moments_is_the_parent_reference(vref, views):
    """(d) with finite moment records, hist_next and out equal temporal_reference.c's (no prev_point) and motion_reference.c's
    (prev_point given) bit for bit: across the camera move, with history, demodulate 0 and 1"""
    A, B = views["A"], views["B"]
    for demodulate in (0, 1):
        fa, ra = _history(vref, A, 1, demodulate)
        TT.poison(fa)
        ra = reference(vref, A["cam"], A["cam"], A["dirs"], A["dirs"], fa, demodulate=demodulate)
        assert np.isfinite(ra["mom"]).all()
        fb = TT.make_frame(B["pos"], B["dirs"], W0, H0, seed=2)
        rng = np.random.default_rng(5)
        pp = (np.where(fb["hit"][..., None], fb["P"], 0.0) + rng.uniform(-0.1, 0.1, size=fb["P"].shape)).astype(np.float32)
        pp[rng.integers(0, 2, size=(H0, W0)) == 0] = np.nan
        for prev_point in (None, pp):
            got = reference(vref, B["cam"], A["cam"], B["dirs"], A["dirs"], fb, ra["hist"], ra["mom"], prev_point, demodulate=demodulate)
            want = parent_reference(vref, B["cam"], A["cam"], B["dirs"], A["dirs"], fb, ra["hist"], prev_point, demodulate=demodulate)
            assert (want[0][..., 3] > 1).sum() > W0 * H0 // 2
            assert np.array_equal(_bits(got["hist"]), _bits(want[0])) and np.array_equal(_bits(got["out"]), _bits(want[1])), demodulate
        # and without history
        got = reference(vref, B["cam"], A["cam"], B["dirs"], A["dirs"], fb, demodulate=demodulate)
        want = parent_reference(vref, B["cam"], A["cam"], B["dirs"], A["dirs"], fb, None, None, demodulate=demodulate)
        assert np.array_equal(_bits(got["hist"]), _bits(want[0])) and np.array_equal(_bits(got["out"]), _bits(want[1]))


def test_reference_bad_moments_and_dead_pixels(vref, views):
    """(e) a moment record with a NaN or an infinity is never a tap: it acts exactly as a history record with len 0 does.  Pixels
    that are not live write moments {0, 0} and variance 0.  In the spatial window a live neighbour whose luminance overflowed (an
    infinite record) is not counted either, and the overflowing pixel shows its own value."""
    A, B = views["A"], views["B"]
    fa, ra = _history(vref, A, 1)
    fb = TT.make_frame(B["pos"], B["dirs"], W0, H0, seed=2)
    dead = TT.poison(fb)
    base = reference(vref, B["cam"], A["cam"], B["dirs"], A["dirs"], fb, ra["hist"], ra["mom"])
    assert not base["mom"][dead].any() and not base["var"][dead].any() and np.all(base["hist"][dead][:, 3] == 0.0)
    assert np.isfinite(base["mom"]).all() and (base["mom"][~dead][:, 0] > 0).all()
    some = np.zeros((H0, W0), bool)
    some[5::7, 3::5] = True
    cut = ra["hist"].copy()
    cut[some, 3] = 0.0
    want = reference(vref, B["cam"], A["cam"], B["dirs"], A["dirs"], fb, cut, ra["mom"])
    assert not np.array_equal(_bits(want["hist"]), _bits(base["hist"])), "the control: these records were taps"
    for kind, (i, v) in enumerate(((0, np.nan), (1, np.nan), (0, np.inf), (1, -np.inf))):
        bad = ra["mom"].copy()
        bad[some, i] = v
        got = reference(vref, B["cam"], A["cam"], B["dirs"], A["dirs"], fb, ra["hist"], bad)
        for k in ("hist", "mom", "var", "out"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (kind, k)
    # an overflowing luminance in the spatial window
    f = _flat_noisy(A, 43)
    f["albedo"] = np.full_like(f["albedo"], 0.5)
    y, x = 50, 40
    assert f["sid"][y, x] == 0 and (f["sid"][y - 3:y + 4, x - 3:x + 4] == 0).all()
    clean = reference(vref, A["cam"], A["cam"], A["dirs"], A["dirs"], f)
    f["rgb"][y, x] = 3e38
    f["albedo"][y, x] = 1e-3
    r = reference(vref, A["cam"], A["cam"], A["dirs"], A["dirs"], f)
    assert np.isinf(r["mom"][y, x]).all() and r["hist"][y, x, 3] == 1.0
    near = np.zeros((H0, W0), bool)
    near[y - 3:y + 4, x - 3:x + 4] = True
    near[y, x] = False
    assert np.array_equal(r["count"][near], clean["count"][near] - 1) and np.isfinite(r["var"][near]).all()
    assert np.array_equal(_bits(r["var"][~near & ~((np.arange(H0)[:, None] == y) & (np.arange(W0)[None, :] == x))]),
                          _bits(clean["var"][~near & ~((np.arange(H0)[:, None] == y) & (np.arange(W0)[None, :] == x))]))
    assert r["count"][y, x] == clean["count"][y, x], "the centre always counts"


# ---- CPU: variance_reference.py pinned to its meaning

def _b3_blur(img):
    """the plain B3-spline blur h (x) h, renormalised at the border"""
    num, den = np.zeros_like(img, dtype=np.float64), np.zeros(img.shape[:2])
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            q, inside = R._shifted(img.astype(np.float64), dx, dy)
            k = R.H5[dx + 2] * R.H5[dy + 2] * inside
            num += k[..., None] * q
            den += k
    return num / den[..., None]


def test_filter_reference_self_checks():
    """the numpy filter: variance 0 returns a noisy image (the weights vanish); a huge variance with the normal and depth terms
    off is the plain B3-spline blur; a constant variance shrinks by sum k^2 / (sum k)^2 per pass; pixels that are not live pass
    through and are never taps"""
    w, h = 37, 23
    s = R.synthetic(w, h, edge=20)
    k = {g: s[g] for g in GUIDES}
    live = ~s["miss"]
    zero = np.zeros((h, w), np.float32)
    # variance 0: d_p = 1e-4, so a tap weighs in only when its luminance is within a few 1e-4 of the centre's
    wsum = []
    out, vout = V.denoise_variance(**k, variance=zero, iterations=1, sigma_luminance=4.0, weights=wsum)
    quiet = live & (wsum[0] < 1e-3)
    assert quiet.sum() >= 0.8 * live.sum(), quiet.sum()
    assert np.allclose(out[quiet], s["rgb"][quiet].astype(np.float64), rtol=2e-3, atol=0) and not vout.any()
    assert float(np.median(wsum[0][live])) < 1e-6
    # a huge variance, the guides off, no demodulation: every weight is its kernel weight
    inf = float("inf")
    flat = dict(k, normal=np.tile(np.float32([0, 0, 1]), (h, w, 1)), albedo=np.ones((h, w, 3), np.float32), t=np.ones((h, w), np.float32),
                rgb=np.where(s["miss"][..., None], np.float32(0.3), s["rgb"]))
    out, _ = V.denoise_variance(**flat, variance=np.full((h, w), 1e12, np.float32), iterations=1, sigma_luminance=4.0, sigma_normal=inf,
                                sigma_depth=inf, demodulate=0)
    blur = _b3_blur(flat["rgb"])
    assert np.abs(out - blur).max() <= 1e-5 * np.abs(blur).max(), np.abs(out - blur).max()
    out_inf, _ = V.denoise_variance(**flat, variance=zero, iterations=1, sigma_luminance=inf, sigma_normal=inf, sigma_depth=inf, demodulate=0)
    assert np.abs(out_inf - blur).max() <= 1e-12, "+inf switches the luminance term off"
    # a constant variance on a constant image: v_1 = v_0 sum k^2 / (sum k)^2 = v_0 (70 / 256)^2 in the interior
    const = dict(flat, rgb=np.full((h, w, 3), 0.5, np.float32))
    _, v1 = V.denoise_variance(**const, variance=np.full((h, w), 0.25, np.float32), iterations=1, demodulate=0)
    assert np.allclose(v1[2:-2, 2:-2], 0.25 * (70.0 / 256.0) ** 2, rtol=1e-12, atol=0)
    assert (v1[0, 0] > v1[2, 2]), "fewer taps at the border average less"
    # not live: the miss block, a NaN variance and a negative one
    var = (0.5 * luminance64(s["clean"] / np.maximum(s["albedo"], 1e-3))).astype(np.float32) ** 2
    var[12, 30], var[4, 20] = np.nan, -1.0
    dead = s["miss"].copy()
    dead[12, 30] = dead[4, 20] = True
    assert np.array_equal(V.live_mask(**k, variance=var), ~dead)
    for dtype in (np.float64, np.float32):
        out, vout = V.denoise_variance(**k, variance=var, sigma_luminance=4.0, dtype=dtype)
        assert out.dtype == dtype and vout.dtype == dtype
        assert np.array_equal(out[dead], s["rgb"][dead].astype(dtype))
        assert np.array_equal(_bits(vout[dead].astype(np.float32)), _bits(var[dead]))
        loud = dict(k, rgb=np.where(dead[..., None], np.float32(1e30), s["rgb"]))
        out2, vout2 = V.denoise_variance(**loud, variance=var, sigma_luminance=4.0, dtype=dtype)
        assert np.array_equal(out2[~dead], out[~dead]) and np.array_equal(vout2[~dead], vout[~dead])
    # and it denoises: with the noise's own variance the error against the clean image falls well below the input's
    out, vout = V.denoise_variance(**k, variance=var, sigma_luminance=4.0)
    lv = ~dead
    assert _rmse(out[lv], s["clean"][lv]) < 0.5 * _rmse(s["rgb"][lv], s["clean"][lv])
    assert (vout[lv] < var[lv]).all()


# ---- the filter's inputs of the GPU test, and the condition the float32 reference has to meet on them

SIZES = [(1, 1), (1, 70), (130, 5), (37, 23), (64, 64)]
# iterations 1, 5 and 8 at sigma_luminance 4.0, where neighbours really mix, and the luminance term switched off.  The default
# bandwidth 0.0625 is not among them: there the exponents run from 8 to 50, a float32 evaluation of the formulas already deviates
# by 8e-6 in the variance (130 x 5), and 16 x that is past the cap; the defaults run on the device in test_pipeline.
FILTER_SETS = [{"iterations": 1, "sigma_luminance": 4.0}, {"iterations": 5, "sigma_luminance": 4.0}, {"iterations": 8, "sigma_luminance": 4.0},
               {"iterations": 5, "sigma_luminance": float("inf")}]


def _filter_inputs(w, h):
    """the two inputs: the synthetic image with the variance of its Gamma(4, 0.25) noise, (0.5 lum(clean / a))^2, and the same
    with variance 0 on the left half, where the colour is then the clean one (d_p at its floor 1e-4 with luminance differences
    of rounding size is ill-conditioned, so the noise goes with the variance); at 37 x 23 with a NaN colour, an infinite
    colour, a NaN normal, a NaN variance and a negative variance"""
    s = R.synthetic(w, h, edge=20 if (w, h) == (37, 23) else None)
    a = np.maximum(s["albedo"], np.float32(1e-3))
    var = ((0.5 * luminance64(s["clean"] / a)) ** 2).astype(np.float32)
    var[s["miss"]] = 0.0
    if (w, h) == (37, 23):
        s["rgb"][10, 12, 1] = np.nan
        s["rgb"][15, 30, 0] = np.inf
        s["normal"][18, 8, 2] = np.nan
        var[12, 30], var[4, 20] = np.nan, -1.0
    full = {g: s[g] for g in GUIDES}
    full["variance"] = var
    half = {g: s[g].copy() for g in GUIDES}
    left = np.zeros((h, w), bool)
    left[:, :w // 2] = True
    half["rgb"] = np.where((left & ~s["miss"])[..., None] & np.isfinite(s["rgb"]), s["clean"], s["rgb"])
    half["variance"] = np.where(left & np.isfinite(var) & (var >= 0), np.float32(0.0), var)
    for d in (full, half):
        for v in d.values():
            v.setflags(write=False)
    return {"noise": full, "left half 0": half}


_REF_CACHE = {}


def _filter_reference(w, h, name, i):
    """(ref64 out, ref64 variance, tol out, tol variance, live) of one case, computed once"""
    key = (w, h, name, i)
    if key not in _REF_CACHE:
        k = _filter_inputs(w, h)[name]
        prm = FILTER_SETS[i]
        ref = V.denoise_variance(**k, **prm)
        r32 = V.denoise_variance(**k, dtype=np.float32, **prm)
        live = V.live_mask(**k)
        tols = []
        for x32, x64 in zip(r32, ref):
            with np.errstate(invalid="ignore"):  # (pixels that are not live may hold NaN)
                dev32 = float(R.deviation(x32, x64)[live].max()) if live.any() else 0.0
            tols.append(TOL_FACTOR * dev32)
        _REF_CACHE[key] = (ref[0], ref[1], tols[0], tols[1], live)
    return _REF_CACHE[key]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_float32_reference_meets_the_cap(size):
    """on every size, input and parameter set of the GPU test, 16 x the float32 reference's deviation stays below 1e-4"""
    w, h = size
    for name in ("noise", "left half 0"):
        for i in range(len(FILTER_SETS)):
            _, _, tol_c, tol_v, live = _filter_reference(w, h, name, i)
            print("%dx%d %s %r: tol %.3g (colour) %.3g (variance)" % (w, h, name, FILTER_SETS[i], tol_c, tol_v))
            assert tol_c < TOL_CAP and tol_v < TOL_CAP, (name, FILTER_SETS[i], tol_c, tol_v)
    if size == (37, 23):
        assert (~live).sum() == 6 + 5, "the miss block and the five poisoned pixels"


# ---- the pipeline's prediction (CPU oracle)

def test_pipeline_prediction(vref, oracle, scenes):
    """The prediction of the GPU pipeline test, after tests/test_temporal.py::test_pipeline_prediction: the oracle's mode-200
    frames of the Cornell box (48 x 48, 3 bounces, 4 spp, seed 1234 + f, eight poses yawing 1 degree per frame) with geometric
    guides go through variance_reference.c, the last one then through variance_reference.py in float32, all with the defaults.
    RMSE against the 1024-spp frame of the last pose, relative to the last 4-spp frame's.  On the same frames: (i) temporal alone
    (0.6363, test_temporal.py's figure, recomputed here) and (ii) temporal, then the plain filter of denoise_reference.py with its
    defaults (0.9193).  The requirement: the new ratio is below both.  Observed 0.6360.

    What the figures say: at 48 x 48 the error that is left after eight frames sits on the light's edge,
    where no image-space filter helps, and any blur across the box's shading adds error; the plain filter's 0.9193 is that.  The
    defaults were settled on this prediction: sigma_luminance 0.0625 keeps the variance filter from adding error (4.0 gives
    0.9566); the figure does not separate the other parameters (0.634 .. 0.636 for alpha_moments 0.2 .. 0.5, min_history 2 .. 8,
    1 .. 5 passes at that bandwidth), which stay at the suggested values."""
    w = h = 48
    sc = scenes.cornell_box()
    o = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    hist = mom = prev = None
    try:
        for f, (x, y, z, yaw) in enumerate(TT.POSES):
            rot = TT.yaw_matrix(yaw, scenes)
            dirs = TT.oracle_dirs(oracle, rot, w, h)
            oracle.set_path_params(4, 3, 1234 + f)
            fr = o.render((x, y, z), rot, 200, w, h)
            centre = o.render((x, y, z), rot, 3, w, h, want=("hit_inst", "hit_prim", "hit_t"))
            normal, albedo, t = TT._oracle_guides(sc, centre, (x, y, z), dirs, w, h)
            cam = camera((x, y, z), rot)
            frame = {"rgb": fr["rgb"], "normal": normal, "albedo": albedo, "t": t}
            r = reference(vref, cam, cam if prev is None else prev[0], dirs, dirs if prev is None else prev[1], frame, hist, mom)
            hist, mom, prev = r["hist"], r["mom"], (cam, dirs)
        oracle.set_path_params(1024, 3, 1234)
        clean = o.render((x, y, z), rot, 200, w, h, want=("rgb",))["rgb"]
    finally:
        oracle.set_path_params(4, 3, 1234)
        o.close()
    base = _rmse(fr["rgb"], clean)
    alone = _rmse(r["out"], clean) / base
    plain = _rmse(R.denoise(r["out"], normal, albedo, t, dtype=np.float32), clean) / base
    out, _ = V.denoise_variance(r["out"], normal, albedo, t, r["var"], dtype=np.float32)
    ratio = _rmse(out, clean) / base
    print("pipeline prediction: temporal alone %.4f, then the plain filter %.4f, with variance %.4f; mean variance %.4g" %
          (alone, plain, ratio, float(r["var"].mean())))
    assert abs(alone - TEMPORAL_ALONE) < 5e-4, alone
    assert ratio < alone and ratio < plain, (ratio, alone, plain)
    assert abs(ratio - PIPELINE_PREDICTION) < 5e-4, (ratio, PIPELINE_PREDICTION)


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _device(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


OUTPUTS = ("hist", "mom", "var", "out")


def _run_temporal(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, d_mom, d_pp, prm, out_is_rgb=False):
    d_rgb = d["rgb"].clone() if out_is_rgb else d["rgb"]
    d_next = torch.full((h, w, 8), -7.0, dtype=torch.float32, device="cuda")
    d_mnext = torch.full((h, w, 2), -7.0, dtype=torch.float32, device="cuda")
    d_var = torch.full((h, w), -7.0, dtype=torch.float32, device="cuda")
    d_out = d_rgb if out_is_rgb else torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.temporal_variance_device(w, h, cam_cur, cam_prev, d_rgb.data_ptr(), d["normal"].data_ptr(),
                                      d["albedo"].data_ptr() if prm["demodulate"] else None, d["t"].data_ptr(),
                                      None if d_hist is None else d_hist.data_ptr(), d_next.data_ptr(),
                                      None if d_mom is None else d_mom.data_ptr(), d_mnext.data_ptr(), d_var.data_ptr(), d_out.data_ptr(),
                                      d_prev_point=None if d_pp is None else d_pp.data_ptr(), **prm)
    renderer.synchronize()
    return {"hist": d_next.cpu().numpy(), "mom": d_mnext.cpu().numpy(), "var": d_var.cpu().numpy(), "out": d_out.cpu().numpy()}


def _same(got, want, what):
    for k in OUTPUTS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), what + ": " + k


def _mixed_history(vref, cam_prev, dir_prev, f0, prm):
    """the reference's records of an earlier frame (with its poisoned pixels), len set to 2 on every third pixel and to 9 on the
    others, so that len_out is 3 (the spatial branch) and 10 (the long one) side by side in every wavefront; a few moment records
    NaN or infinite"""
    r0 = reference(vref, cam_prev, cam_prev, dir_prev, dir_prev, f0, **prm)
    h, w = f0["t"].shape
    y, x = np.mgrid[0:h, 0:w]
    lens = np.where((x + 2 * y) % 3 == 0, np.float32(2.0), np.float32(9.0))
    hist0, mom0 = r0["hist"], r0["mom"]
    hist0[..., 3] = np.where(hist0[..., 3] > 0, lens, hist0[..., 3])
    if w * h >= 64:
        flat = mom0.reshape(-1, 2)
        flat[7::29, 0] = np.nan
        flat[11::31, 1] = np.inf
    return hist0, mom0


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_temporal_variance_equals_the_reference(pkg, scenes, vref, renderer, size):
    """hist_next, mom_next, variance and out of the device form equal variance_reference.c's bits: the three camera pairs of
    test_temporal.py, demodulate 0 and 1, with and without history and moments (history lengths 2 and 9 side by side, poisoned
    pixels, bad moment records), with and without prev_point; directions from crt_camera_rays.  The host form, out aliased to
    rgb and a second call give the same bits."""
    import torch
    w, h = size
    short = long_ = 0
    for name, cam_cur, cam_prev in TT._pairs(scenes):
        dir_cur, dir_prev = TT._device_dirs(renderer, cam_cur, w, h), TT._device_dirs(renderer, cam_prev, w, h)
        f0 = TT.make_frame(cam_prev[:3], dir_prev, w, h, seed=11)
        TT.poison(f0)
        f1 = TT.make_frame(cam_cur[:3], dir_cur, w, h, seed=12)
        TT.poison(f1)
        rng = np.random.default_rng(13)
        pp = (np.where(f1["hit"][..., None], f1["P"], 0.0) + rng.uniform(-0.1, 0.1, size=f1["P"].shape)).astype(np.float32)
        pp[rng.integers(0, 3, size=(h, w)) == 0] = np.nan
        d = {k: _device(torch, f1[k]) for k in GUIDES}
        d_pp = _device(torch, pp)
        for demodulate in (0, 1):
            prm = dict(DEFAULTS, demodulate=demodulate)
            hist0, mom0 = _mixed_history(vref, cam_prev, dir_prev, f0, prm)
            for history in (False, True):
                hp, mp = (hist0, mom0) if history else (None, None)
                d_hist, d_mom = (_device(torch, hist0), _device(torch, mom0)) if history else (None, None)
                for prev_point in (None, pp):
                    what = "%dx%d %s demodulate %d history %s prev_point %s" % (w, h, name, demodulate, history, prev_point is not None)
                    want = reference(vref, cam_cur, cam_prev, dir_cur, dir_prev, f1, hp, mp, prev_point, **prm)
                    dpp = None if prev_point is None else d_pp
                    _same(_run_temporal(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, d_mom, dpp, prm), want, what)
                    host = renderer.temporal_variance(cam_cur, cam_prev, f1["rgb"], f1["normal"], f1["albedo"] if demodulate else None, f1["t"],
                                                      hp, mp, prev_point=prev_point, **prm)
                    _same(dict(zip(OUTPUTS, host)), want, what + ": host form")
                    _same(_run_temporal(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, d_mom, dpp, prm, out_is_rgb=True), want, what + ": in place")
                    _same(_run_temporal(torch, renderer, w, h, cam_cur, cam_prev, d, d_hist, d_mom, dpp, prm), want, what + ": second call")
                    if history:
                        short += int((want["count"] > 0).sum())
                        long_ += int(((want["count"] == 0) & (want["hist"][..., 3] > 0)).sum())
    if w * h >= 64:
        assert short > 0 and long_ > 0, "both branches of V6 ran"
    print("%dx%d: %d pixel results from the spatial branch with history, %d from the long one" % (w, h, short, long_))


@pytest.mark.gpu
def test_three_chained_frames(pkg, scenes, vref, renderer):
    """three frames along a three-pose path, chained through swapped device buffers, equal the reference chained the same way"""
    import torch
    w, h = 37, 23
    cams = [camera(TT.POS_A, TT.yaw_matrix(0.0, scenes)), camera(TT.POS_B, TT.yaw_matrix(2.0, scenes)),
            camera((0.3, 0.62, 2.1), TT.yaw_matrix(4.0, scenes))]
    dirs = [TT._device_dirs(renderer, c, w, h) for c in cams]
    d_hist = [torch.zeros((h, w, 8), dtype=torch.float32, device="cuda") for _ in range(2)]
    d_mom = [torch.zeros((h, w, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
    d_var = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    r = None
    for k in range(3):
        f = TT.make_frame(cams[k][:3], dirs[k], w, h, seed=20 + k)
        TT.poison(f)
        d = {g: _device(torch, f[g]) for g in GUIDES}
        d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        prev, at = max(k - 1, 0), k & 1
        torch.cuda.synchronize()
        renderer.temporal_variance_device(w, h, cams[k], cams[prev], d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(),
                                          d["t"].data_ptr(), d_hist[at].data_ptr() if k else None, d_hist[at ^ 1].data_ptr(),
                                          d_mom[at].data_ptr() if k else None, d_mom[at ^ 1].data_ptr(), d_var.data_ptr(), d_out.data_ptr(),
                                          min_history=3)
        renderer.synchronize()
        r = reference(vref, cams[k], cams[prev], dirs[k], dirs[prev], f, None if r is None else r["hist"], None if r is None else r["mom"],
                      min_history=3)
        got = {"hist": d_hist[at ^ 1].cpu().numpy(), "mom": d_mom[at ^ 1].cpu().numpy(), "var": d_var.cpu().numpy(), "out": d_out.cpu().numpy()}
        _same(got, r, "frame %d" % k)
    assert (r["count"] > 0).any() and ((r["count"] == 0) & (r["hist"][..., 3] >= 3)).any(), "the third frame has both branches"


def _run_filter(torch, renderer, w, h, d, prm, in_place=False):
    d_rgb = d["rgb"].clone() if in_place else d["rgb"]
    d_var = d["variance"].clone() if in_place else d["variance"]
    d_out = d_rgb if in_place else torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
    d_vout = d_var if in_place else torch.full((h, w), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    renderer.denoise_variance_device(w, h, d_rgb.data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(), d_var.data_ptr(),
                                     d_out.data_ptr(), d_vout.data_ptr(), **prm)
    renderer.synchronize()
    return d_out.cpu().numpy(), d_vout.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_denoise_variance_equals_the_reference(pkg, renderer, size):
    """out and variance_out of the device form within tol of the float64 reference (16 x the float32 reference's deviation, below
    1e-4: test_float32_reference_meets_the_cap) on both inputs, for iterations 1, 5 and 8 and with the luminance term off; pixels
    that are not live bit-equal to their input; the in-place form, the host form and a second call give the device form's bits."""
    import torch
    w, h = size
    worst = [0.0, 0.0]
    for name, k in _filter_inputs(w, h).items():
        d = {g: _device(torch, k[g]) for g in k}
        for i, prm in enumerate(FILTER_SETS):
            ref_c, ref_v, tol_c, tol_v, live = _filter_reference(w, h, name, i)
            assert tol_c < TOL_CAP and tol_v < TOL_CAP
            what = "%dx%d %s %r" % (w, h, name, prm)
            got = _run_filter(torch, renderer, w, h, d, prm)
            with np.errstate(invalid="ignore"):
                dev_c = float(R.deviation(got[0], ref_c)[live].max()) if live.any() else 0.0
                dev_v = float(R.deviation(got[1], ref_v)[live].max()) if live.any() else 0.0
            worst = [max(worst[0], dev_c), max(worst[1], dev_v)]
            print("%s: device deviation %.3g (tol %.3g) colour, %.3g (tol %.3g) variance" % (what, dev_c, tol_c, dev_v, tol_v))
            assert np.isfinite(got[0][live]).all() and np.isfinite(got[1][live]).all() and (got[1][live] >= 0).all(), what
            assert dev_c <= tol_c, (what, dev_c, tol_c)
            assert dev_v <= tol_v, (what, dev_v, tol_v)
            assert np.array_equal(_bits(got[0][~live]), _bits(k["rgb"][~live])), what + ": a pixel that is not live changed"
            assert np.array_equal(_bits(got[1][~live]), _bits(k["variance"][~live])), what + ": the variance of a pixel that is not live changed"
            host = renderer.denoise_variance(k["rgb"], k["normal"], k["albedo"], k["t"], k["variance"], want_variance=True, **prm)
            assert np.array_equal(_bits(host[0]), _bits(got[0])) and np.array_equal(_bits(host[1]), _bits(got[1])), what + ": host form"
            for again in (True, False):
                g2 = _run_filter(torch, renderer, w, h, d, prm, in_place=again)
                assert np.array_equal(_bits(g2[0]), _bits(got[0])) and np.array_equal(_bits(g2[1]), _bits(got[1])), \
                    what + (": in place" if again else ": second call")
        # variance_out is optional
        d_out = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        renderer.denoise_variance_device(w, h, d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(),
                                         d["variance"].data_ptr(), d_out.data_ptr(), None, **prm)
        renderer.synchronize()
        assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(got[0])), "without variance_out"
    print("%dx%d: worst device deviation %.3g colour, %.3g variance" % (w, h, worst[0], worst[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (1, 70), (130, 5), (37, 23)], ids=lambda s: "%dx%d" % s)
def test_with_their_first_term_off_the_two_filters_are_one(pkg, renderer, size):
    """denoise_device with sigma_color = +inf and denoise_variance_device with variance 0 and sigma_luminance = +inf give the same
    bytes.  Both are one kernel (denoise_kernels.hip) that differs in the exponent's first term: |dc|^2 x 0 against |d lum| x 0,
    both +0 on finite colours; the normal and depth terms, the weights, the sums and the multiply-back are the same expressions,
    and with a variance of 0 the two liveness rules agree."""
    import torch
    w, h = size
    s = R.synthetic(w, h, edge=20 if (w, h) == (37, 23) else None)
    d = {g: _device(torch, s[g]) for g in GUIDES}
    ptrs = [d[g].data_ptr() for g in GUIDES]
    d_zero = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    for iterations in (1, 5):
        for demodulate in (0, 1):
            plain = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
            guided = torch.full((h, w, 3), -9.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            renderer.denoise_device(w, h, *ptrs, plain.data_ptr(), iterations=iterations, demodulate=demodulate, sigma_color=float("inf"))
            renderer.denoise_variance_device(w, h, *ptrs, d_zero.data_ptr(), guided.data_ptr(), None, iterations=iterations,
                                             demodulate=demodulate, sigma_luminance=float("inf"))
            renderer.synchronize()
            assert torch.equal(plain.view(torch.int32), guided.view(torch.int32)), (size, iterations, demodulate)
    if (w, h) == (37, 23):
        assert s["miss"].sum() == 6 and np.array_equal(plain.cpu().numpy()[s["miss"]], s["rgb"][s["miss"]]), "the dead block"


@pytest.mark.gpu
def test_errors(pkg, scenes, vref, renderer):
    """every CRT_EINVAL case of both families launches nothing and leaves sentinel-filled outputs untouched; a context without a
    scene works; stats carry times and no counts"""
    import torch
    L = pkg.lib()
    w, h = 16, 8
    cam = camera(TT.POS_A, TT.yaw_matrix(0.0, scenes))
    dirs = TT._device_dirs(renderer, cam, w, h)
    f = TT.make_frame(cam[:3], dirs, w, h, seed=3)
    host_in = {g: np.ascontiguousarray(f[g], np.float32) for g in GUIDES}
    d = {g: _device(torch, f[g]) for g in GUIDES}
    sentinel = -5.0
    shapes = {"hist_next": 8, "mom_next": 2, "variance": 1, "out": 3}
    d_o = {k: torch.full((w * h * n + 8,), sentinel, dtype=torch.float32, device="cuda") for k, n in shapes.items()}
    h_o = {k: np.full((w * h * n,), sentinel, np.float32) for k, n in shapes.items()}
    d_hist_prev = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    d_mom_prev = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    d_pp = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    hist_prev_h, mom_prev_h = np.zeros((h, w, 8), np.float32), np.zeros((h, w, 2), np.float32)
    K = cam.ctypes.data
    torch.cuda.synchronize()

    def call(fn, a, prm):
        return fn(renderer.h, a["w"], a["h"], a["cur"], a["prev"], a["rgb"], a["normal"], a["albedo"], a["t"], a["prev_point"], a["hist_prev"],
                  a["hist_next"], a["mom_prev"], a["mom_next"], a["variance"], a["out"], C.byref(prm) if prm else None, None)

    def dev(prm=None, **over):
        a = {g: d[g].data_ptr() for g in GUIDES}
        a.update(w=w, h=h, cur=K, prev=K, prev_point=d_pp.data_ptr(), hist_prev=d_hist_prev.data_ptr(), mom_prev=d_mom_prev.data_ptr())
        a.update({k: v.data_ptr() for k, v in d_o.items()})
        a.update(over)
        return call(L.crt_temporal_variance_device, a, prm)

    def host(prm=None, **over):
        a = {g: host_in[g].ctypes.data for g in GUIDES}
        a.update(w=w, h=h, cur=K, prev=K, prev_point=None, hist_prev=hist_prev_h.ctypes.data, mom_prev=mom_prev_h.ctypes.data)
        a.update({k: v.ctypes.data for k, v in h_o.items()})
        a.update(over)
        return call(L.crt_temporal_variance, a, prm)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((v == sentinel).all().item()) for v in d_o.values()) and all(np.all(v == sentinel) for v in h_o.values())

    nan = float("nan")
    TP = pkg.TemporalVarianceParams
    bad = [TP(alpha=v) for v in (-0.1, 1.5, nan)] + [TP(depth_tolerance=v) for v in (0.0, -1.0, nan)]
    bad += [TP(normal_threshold=nan), TP(max_history=0), TP(max_history=(1 << 24) + 1), TP(demodulate=2)]
    bad += [TP(alpha_moments=v) for v in (-0.1, 1.5, nan)] + [TP(min_history=0), TP(min_history=(1 << 24) + 1)]
    for prm in bad:
        assert dev(prm) == EINVAL and host(prm) == EINVAL
    for over in ({"w": 0}, {"h": 0}, {"w": 1 << 15, "h": 1 << 14}):
        assert dev(**over) == EINVAL and host(**over) == EINVAL, over
    for g in ("cur", "prev", "rgb", "normal", "t", "albedo", "hist_next", "mom_next", "variance"):
        assert dev(**{g: None}) == EINVAL and host(**{g: None}) == EINVAL, g
    assert dev(mom_prev=None) == EINVAL and host(mom_prev=None) == EINVAL, "history without moments"
    assert dev(hist_prev=None) == EINVAL and host(hist_prev=None) == EINVAL, "moments without history"
    for g in GUIDES:
        assert dev(**{g: d[g].data_ptr() + 2}) == EINVAL, g
    assert dev(out=d_o["out"].data_ptr() + 2) == EINVAL and dev(variance=d_o["variance"].data_ptr() + 2) == EINVAL
    assert dev(prev_point=d_pp.data_ptr() + 2) == EINVAL
    assert dev(hist_next=d_o["hist_next"].data_ptr() + 8) == EINVAL and dev(hist_prev=d_hist_prev.data_ptr() + 4) == EINVAL
    assert dev(mom_next=d_o["mom_next"].data_ptr() + 4) == EINVAL and dev(mom_prev=d_mom_prev.data_ptr() + 4) == EINVAL
    assert "aligned" in L.crt_last_error(renderer.h).decode()
    assert untouched()

    # the filter
    var_h = np.full((h, w), 0.01, np.float32)
    d_var = _device(torch, var_h)
    f_o = {"out": torch.full((w * h * 3 + 8,), sentinel, dtype=torch.float32, device="cuda"),
           "variance_out": torch.full((w * h + 8,), sentinel, dtype=torch.float32, device="cuda")}
    fh_o = {"out": np.full((w * h * 3,), sentinel, np.float32), "variance_out": np.full((w * h,), sentinel, np.float32)}
    torch.cuda.synchronize()

    def fcall(fn, a, prm):
        return fn(renderer.h, a["w"], a["h"], a["rgb"], a["normal"], a["albedo"], a["t"], a["variance"], a["out"], a["variance_out"],
                  C.byref(prm) if prm else None, None)

    def fdev(prm=None, **over):
        a = {g: d[g].data_ptr() for g in GUIDES}
        a.update(w=w, h=h, variance=d_var.data_ptr(), out=f_o["out"].data_ptr(), variance_out=f_o["variance_out"].data_ptr())
        a.update(over)
        return fcall(L.crt_denoise_variance_device, a, prm)

    def fhost(prm=None, **over):
        a = {g: host_in[g].ctypes.data for g in GUIDES}
        a.update(w=w, h=h, variance=var_h.ctypes.data, out=fh_o["out"].ctypes.data, variance_out=fh_o["variance_out"].ctypes.data)
        a.update(over)
        return fcall(L.crt_denoise_variance, a, prm)

    DP = pkg.DenoiseVarianceParams
    fbad = [DP(iterations=0), DP(iterations=9), DP(demodulate=2)]
    fbad += [DP(**{s: v}) for s in ("sigma_luminance", "sigma_normal", "sigma_depth") for v in (0.0, -1.0, nan)]
    for prm in fbad:
        assert fdev(prm) == EINVAL and fhost(prm) == EINVAL
    for over in ({"w": 0}, {"h": 0}, {"w": 1 << 15, "h": 1 << 14}):
        assert fdev(**over) == EINVAL and fhost(**over) == EINVAL, over
    for g in GUIDES + ("variance", "out"):
        assert fdev(**{g: None}) == EINVAL and fhost(**{g: None}) == EINVAL, g
    for g in GUIDES:
        assert fdev(**{g: d[g].data_ptr() + 2}) == EINVAL, g
    assert fdev(variance=d_var.data_ptr() + 2) == EINVAL and fdev(out=f_o["out"].data_ptr() + 2) == EINVAL
    assert fdev(variance_out=f_o["variance_out"].data_ptr() + 2) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((v == sentinel).all().item()) for v in f_o.values()) and all(np.all(v == sentinel) for v in fh_o.values())

    # the controls: the extreme parameters, NULL albedo without demodulation, NULL out, no history, no prev_point; nothing is
    # written behind the buffers
    assert dev(TP(demodulate=0, alpha=1.0, alpha_moments=1.0, max_history=1 << 24, min_history=1 << 24, normal_threshold=-2.0), albedo=None,
               out=None, hist_prev=None, mom_prev=None, prev_point=None) == 0
    assert host(TP(alpha=0.0, alpha_moments=0.0, max_history=1, min_history=1)) == 0
    torch.cuda.synchronize()
    assert bool((d_o["out"] == sentinel).all().item())
    for k, n in shapes.items():
        if k != "out":
            assert not bool((d_o[k][:w * h * n] == sentinel).any().item()) and bool((d_o[k][w * h * n:] == sentinel).all().item()), k
        assert not np.any(h_o[k] == sentinel), k
    assert fdev(DP(iterations=8, sigma_luminance=float("inf"), sigma_normal=float("inf"), sigma_depth=float("inf")), variance_out=None) == 0
    assert fhost(DP(iterations=1)) == 0
    torch.cuda.synchronize()
    assert not bool((f_o["out"][:w * h * 3] == sentinel).any().item()) and bool((f_o["out"][w * h * 3:] == sentinel).all().item())
    assert bool((f_o["variance_out"] == sentinel).all().item())
    assert not np.any(fh_o["out"] == sentinel) and not np.any(fh_o["variance_out"] == sentinel)
    st = renderer.temporal_variance_device(w, h, cam, cam, d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(),
                                           None, d_o["hist_next"].data_ptr(), None, d_o["mom_next"].data_ptr(), d_o["variance"].data_ptr(),
                                           d_o["out"].data_ptr(), stats=True)
    st2 = renderer.denoise_variance_device(w, h, d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(),
                                           d_var.data_ptr(), f_o["out"].data_ptr(), stats=True)
    for s in (st, st2):
        assert s["kernel_ms"] > 0.0 and s["total_ms"] > 0.0
        assert not any(s[k] for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested"))
    fresh = pkg.Renderer(0)
    try:
        got = fresh.temporal_variance(cam, cam, f["rgb"], f["normal"], f["albedo"], f["t"])
        _same(dict(zip(OUTPUTS, got)), reference(vref, cam, cam, dirs, dirs, f), "a context without a scene")
        out = fresh.denoise_variance(f["rgb"], f["normal"], f["albedo"], f["t"], got[2])
        assert np.array_equal(_bits(out), _bits(renderer.denoise_variance(f["rgb"], f["normal"], f["albedo"], f["t"], got[2])))
    finally:
        fresh.close()


@pytest.mark.gpu
def test_pipeline(pkg, scenes, renderer):
    """The prediction's sequence on the device: Cornell box 48 x 48, 3 bounces, 4 spp, eight poses yawing 1 degree per frame, seed
    1234 + f, guides from crt_frame_guides, pushed through TemporalHistory(variance=True), the last accumulated frame then
    through denoise_variance, all with the defaults.  RMSE(filtered last frame) / RMSE(last 4-spp frame) against the 1024-spp
    frame of the last pose stays under PIPELINE_CAP = 1.25 x the CPU prediction (the project's margin for shading against
    geometric normals).  A mode-200 frame and an accumulating pair rendered after the pushes equal those rendered before them
    bit for bit; reset() drops history and moments; without variance=True TemporalHistory does what it did.
    Predicted 0.6360, cap 0.7950; observed on the MI355X: 0.6360 (RMSE 0.1139 for the 4-spp frame, 0.0725 accumulated, 0.0724
    filtered; mean variance 0.1446 before the filter, 0.0710 after)."""
    w = h = 48
    sc = scenes.cornell_box()
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"))
    th = pkg.TemporalHistory(renderer, w, h, variance=True)
    plain = pkg.TemporalHistory(renderer, w, h)
    assert plain.variance is None and plain.moments is None
    try:
        renderer.change_shading_mode(200)

        def frame(f, spp=4, seed=None):
            x, y, z, yaw = TT.POSES[f]
            renderer.set_camera((x, y, z), TT.yaw_matrix(yaw, scenes))
            renderer.set_path_params(spp, 3, 1234 + f if seed is None else seed)
            return renderer.render_frame(w, h, want=("rgba8", "rgb"))["rgb"]
        before = frame(0)
        renderer.set_accumulation(1 << 24)
        acc = [frame(0), frame(0)]
        renderer.set_accumulation(0)
        for f in range(len(TT.POSES)):
            noisy = frame(f)
            g = renderer.frame_guides(w, h)
            out = th.push(noisy, g["normal"], g["albedo"], g["t"])
            same = plain.push(noisy, g["normal"], g["albedo"], g["t"])
            assert out.shape == (h, w, 3) and out.dtype == np.float32
            assert np.array_equal(_bits(out), _bits(same)), "finite moments: the accumulated colour is the plain one"
        assert np.array_equal(_bits(th.records.cpu().numpy()), _bits(plain.records.cpu().numpy()))
        lens = th.records[..., 3].cpu().numpy()
        var = th.variance.cpu().numpy()
        assert var.shape == (h, w) and np.isfinite(var).all() and (var >= 0).all() and (var[lens > 0] > 0).any()
        assert not var[lens == 0].any() and tuple(th.moments.shape) == (h, w, 2)
        filtered, vout = renderer.denoise_variance(out, g["normal"], g["albedo"], g["t"], var, want_variance=True)
        clean = frame(len(TT.POSES) - 1, spp=1024, seed=1234)
        assert np.array_equal(_bits(frame(0)), _bits(before)), "a frame after the pushes"
        renderer.set_accumulation(1 << 24)
        again = [frame(0), frame(0)]
        assert renderer.accumulated_samples() == 8
        renderer.set_accumulation(0)
        assert np.array_equal(_bits(again[0]), _bits(acc[0])) and np.array_equal(_bits(again[1]), _bits(acc[1])), "accumulating frames"
        th.reset()
        first = th.push(noisy, g["normal"], g["albedo"], g["t"])
        rec = th.records[..., 3].cpu().numpy()
        assert np.all(rec <= 1.0), "reset() drops the history"
        live = rec == 1.0
        assert np.allclose(first[live], noisy[live], rtol=1e-6, atol=1e-7)
        m = th.moments.cpu().numpy()
        assert np.allclose(m[live][:, 1], m[live][:, 0] ** 2, rtol=1e-6), "and the moments: m2 = l^2 on a first frame"
    finally:
        renderer.set_accumulation(0)
        renderer.set_path_params(4, 3, 1234)
        renderer.change_shading_mode(0)
    base = _rmse(noisy, clean)
    ratio, alone = _rmse(filtered, clean) / base, _rmse(out, clean) / base
    print("pipeline: RMSE against 1024 spp: 4 spp %.4f, accumulated %.4f (ratio %.4f), filtered with its variance %.4f, ratio %.4f (cap %.4f); "
          "mean len %.2f, mean variance %.4g -> %.4g" % (base, _rmse(out, clean), alone, _rmse(filtered, clean), ratio, PIPELINE_CAP,
                                                         float(lens.mean()), float(var.mean()), float(vout.mean())))
    assert lens.max() > len(TT.POSES) - 0.5
    assert ratio < PIPELINE_CAP, (ratio, PIPELINE_CAP)


@pytest.mark.gpu
def test_cpp_layer(pkg, scenes, vref, renderer, tmp_path):
    """crt::Renderer::temporalVariance and denoiseVariance, from a small C++ program linked against libcrt_hip.so, give the C ABI's
    bits on the 37 x 23 case (the small move, with history and moments).  crt_render --temporal --variance --denoise exits 0 and
    its last frame differs from the run without --variance; --variance needs --temporal; without the flag the output is what it
    was: the frames of --temporal --variance equal those of --temporal, and five command lines without the flag were compared
    once with the parent commit's build on the same MI355X, byte-equal."""
    exe = str(tmp_path / "variance_cpp")
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    csrc = os.path.join(lib_dir, "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + csrc,
                           "-o", exe, os.path.join(ROOT, "tests", "variance_cpp.cpp"), "-L" + lib_dir, "-lcrt_hip",
                           "-Wl,-rpath," + lib_dir, "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    w, h = 37, 23
    n = w * h
    _, cam_cur, cam_prev = TT._pairs(scenes)[1]
    dir_cur, dir_prev = TT._device_dirs(renderer, cam_cur, w, h), TT._device_dirs(renderer, cam_prev, w, h)
    f0 = TT.make_frame(cam_prev[:3], dir_prev, w, h, seed=11)
    TT.poison(f0)
    f1 = TT.make_frame(cam_cur[:3], dir_cur, w, h, seed=12)
    TT.poison(f1)
    hist0, mom0 = _mixed_history(vref, cam_prev, dir_prev, f0, DEFAULTS)
    want = renderer.temporal_variance(cam_cur, cam_prev, f1["rgb"], f1["normal"], f1["albedo"], f1["t"], hist0, mom0)
    assert (want[0][..., 3] > 1).sum() > n // 2
    filt = renderer.denoise_variance(want[3], f1["normal"], f1["albedo"], f1["t"], want[2], want_variance=True)
    scene = pkg.Scene.from_arrays(scenes.cornell_box())
    path = str(tmp_path / "cornell.crtbin")
    scene.save(path)
    scene.close()
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.ascontiguousarray(a, np.float32).reshape(-1) for a in
                    (cam_cur, cam_prev, f1["rgb"], f1["normal"], f1["albedo"], f1["t"], hist0, mom0)]).tofile(src)
    subprocess.check_call([exe, path, str(w), str(h), src, out], timeout=120)
    raw = np.fromfile(out, dtype=np.float32)
    assert raw.size == 18 * n
    at = 0
    for name, a in zip(OUTPUTS + ("filtered", "variance_out"), want + filt):
        assert np.array_equal(_bits(raw[at:at + a.size]), _bits(a).reshape(-1)), name
        at += a.size

    tool = os.path.join(lib_dir, "crt_render")
    base = [tool, path, "--size", "40x24", "--spp", "2", "--frames", "3", "--orbit", "1", "--mode", "200"]

    def run(extra, prefix):
        subprocess.check_call(base + extra + ["--out", str(tmp_path / prefix)], timeout=120, stdout=subprocess.DEVNULL)
        return [open(str(tmp_path / ("%s_%d.ppm" % (prefix, f))), "rb").read() for f in range(3)]
    acc = run(["--temporal"], "acc")
    accv = run(["--temporal", "--variance"], "accv")
    assert accv == acc, "finite moments: the accumulated frames are the plain ones"
    den = run(["--temporal", "--denoise"], "den")
    denv = run(["--temporal", "--variance", "--denoise"], "denv")
    assert denv[:2] == den[:2] and denv[2] != den[2], "the last frame went through the other filter"
    assert subprocess.run(base + ["--variance"], capture_output=True, timeout=60).returncode == 2
    assert subprocess.run(base + ["--denoise", "--variance"], capture_output=True, timeout=60).returncode == 2
