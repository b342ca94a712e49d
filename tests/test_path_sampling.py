"""Statistical pins of the mode-200 sampler against closed forms.  test_path_reference.py shows that the kernels evaluate the
spec's formulas; it cannot show that the formulas sample cosine-weighted directions (a wrong mapping would be restated just as
faithfully).  These tests compare pixel means with physics:

- form factor: a diffuse floor under a parallel CONSTANT rectangle, no lights, black miss colour, max_bounces 1.  A sample is
  exactly 0 or albedo x emission, with mean albedo x emission x F(Po), F the point-to-parallel-rectangle form factor at the
  biased hit point.  The jitter is reproduced with the spec's RNG, so every sample's F and the binomial standard error of every
  pixel are known exactly.  The configuration is rotated to the six axis orientations and one oblique one.
- one interreflection: floor + perpendicular wall + one point light.  max_bounces 1 minus max_bounces 0 (same seed: the same
  first-hit direct light per sample) is the indirect light alone, compared with float64 quadrature over the wall of
  rho_f L_w(Q) cos_P cos_Q / (pi d^2), L_w = rho_w I / (4 pi r^2) cos (this build's Lambert convention); the standard error
  comes from K independent seeds."""
import math

import numpy as np
import pytest

import path_reference as R

RHO = (0.8, 0.6, 0.4)
EMIT = (2.0, 1.5, 1.25)
H_CAM, H_EMIT = 0.5, 1.0
RECT = (-0.5, 0.7, -0.4, 0.6)  # emitter x0, x1, y0, y1 (local frame: floor z = 0, normal +z)


def _corner(a, b, d):
    """form factor from a differential area facing +z to the rectangle [0, a] x [0, b] at height d; odd in a and in b"""
    A, B = np.abs(a) / d, np.abs(b) / d
    sA, sB = np.sqrt(1.0 + A * A), np.sqrt(1.0 + B * B)
    f = (A / sA * np.arctan(B / sA) + B / sB * np.arctan(A / sB)) / (2.0 * math.pi)
    return np.sign(a) * np.sign(b) * f


def form_factor(px, py, d, rect=RECT):
    """point (px, py) on the floor to the parallel rectangle at height d above it: four signed corner rectangles"""
    x0, x1, y0, y1 = rect
    return (_corner(x1 - px, y1 - py, d) - _corner(x0 - px, y1 - py, d) - _corner(x1 - px, y0 - py, d)
            + _corner(x0 - px, y0 - py, d))


def test_form_factor_formula_against_quadrature():
    """the closed form against float64 midpoint quadrature of cos cos' / (pi d^2) = h^2 / (pi r^4)"""
    n = 1200
    for px, py, h in ((0.0, 0.0, 1.0), (0.3, -0.2, 0.999), (-1.4, 0.9, 0.6), (0.69, 0.59, 2.0)):
        x0, x1, y0, y1 = RECT
        xs = x0 + (np.arange(n) + 0.5) * (x1 - x0) / n
        ys = y0 + (np.arange(n) + 0.5) * (y1 - y0) / n
        X, Y = np.meshgrid(xs - px, ys - py)
        r2 = X * X + Y * Y + h * h
        q = np.sum(h * h / (math.pi * r2 * r2)) * (x1 - x0) * (y1 - y0) / n ** 2
        assert abs(form_factor(px, py, h) - q) < 2e-6 * max(q, 1e-3), (px, py, h)


def _frame(n):
    """rotation whose third column is the floor normal n (columns t, b, n, right-handed)"""
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    t = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    b = np.cross(n, t)
    b /= np.linalg.norm(b)
    t = np.cross(b, n)
    return np.stack([t, b, n], axis=1)


ORIENTATIONS = {"+z": (0, 0, 1), "-z": (0, 0, -1), "+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0),
                "oblique": (1.0, 2.0, 3.0)}


def form_factor_scene(normal):
    Rw = _frame(normal)
    rot = lambda p: (Rw @ np.asarray(p, np.float64).T).T  # noqa: E731
    floor = rot([(-20, -20, 0), (20, -20, 0), (20, 20, 0), (-20, 20, 0)])
    x0, x1, y0, y1 = RECT
    emit = rot([(x0, y0, H_EMIT), (x1, y0, H_EMIT), (x1, y1, H_EMIT), (x0, y1, H_EMIT)])
    meshes = [R.quad(*floor, 0), R.quad(*emit, 1)]
    mats = [{"albedo": RHO, "type": R.DIFFUSE}, {"albedo": EMIT, "type": R.CONSTANT}]
    cam_rot = Rw  # the identity camera looks along -z of the local frame: straight down at the floor
    return {"meshes": meshes, "lights": [], "materials": mats,
            "camera": {"position": np.float32(rot([(0.0, 0.0, H_CAM)])[0]), "matrix": np.float32(cam_rot).reshape(9)}}


def expected_form_factor_frame(w, h, spp, seed):
    """per pixel: mean and variance of the mean of the samples' F at their biased hit points (local frame)"""
    n = w * h
    pix = np.repeat(np.arange(n, dtype=np.uint32), spp)
    smp = np.tile(np.arange(spp, dtype=np.uint32), n)
    st = R.rng_start(pix, smp, seed)
    st, jx = R.rng_next(st)
    st, jy = R.rng_next(st)
    d = R.camera_dirs(np.eye(3), pix % w, pix // w, jx, jy, w, h)
    t = H_CAM / -d[:, 2]
    F = form_factor(d[:, 0] * t, d[:, 1] * t, H_EMIT - R.BIAS).reshape(n, spp)
    return F.mean(axis=1).reshape(h, w), (F * (1.0 - F)).sum(axis=1).reshape(h, w) / spp ** 2


def check_form_factor(rgb, mean_F, var_F, what, z2_max=1.4):
    for c in range(3):
        s = RHO[c] * EMIT[c]
        z = (rgb[..., c].astype(np.float64) - s * mean_F) / (s * np.sqrt(var_F))
        assert np.abs(z).max() < 5.0, "%s channel %d: |z| = %.1f" % (what, c, np.abs(z).max())
        assert np.mean(z * z) < z2_max, "%s channel %d: mean z^2 = %.2f" % (what, c, np.mean(z * z))


@pytest.fixture(scope="module")
def ff_cpu():
    return expected_form_factor_frame(16, 16, 256, 11)


@pytest.mark.parametrize("orient", list(ORIENTATIONS))
def test_oracle_form_factor(oracle, ff_cpu, orient):
    sc = form_factor_scene(ORIENTATIONS[orient])
    cam = sc["camera"]
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    oracle.set_path_params(256, 1, 11)
    try:
        got = O.render(cam["position"], cam["matrix"], 200, 16, 16, miss_rgb=(0, 0, 0), want=("rgb",))
    finally:
        oracle.set_path_params(4, 3, 1234)
    check_form_factor(got["rgb"], *ff_cpu, "oracle " + orient)


# ---- one diffuse interreflection

RHO_F, RHO_W = (0.7, 0.5, 0.3), (0.4, 0.8, 0.6)
LIGHT = ((-1.0, 1.5, -2.0), 30.0)
WALL_X, WALL_Y, WALL_Z = 1.0, (0.0, 2.5), (-6.0, 2.0)


def interreflection_scene():
    """floor y = 0 (x <= 1), wall x = 1 facing -x; camera 1 above the floor looking straight down at x in [-1.5, 0.5]"""
    z0, z1 = WALL_Z
    meshes = [R.quad((-3, 0, z1), (WALL_X, 0, z1), (WALL_X, 0, z0), (-3, 0, z0), 0),
              R.quad((WALL_X, WALL_Y[0], z1), (WALL_X, WALL_Y[0], z0), (WALL_X, WALL_Y[1], z0), (WALL_X, WALL_Y[1], z1), 1)]
    mats = [{"albedo": RHO_F, "type": R.DIFFUSE}, {"albedo": RHO_W, "type": R.DIFFUSE}]
    cam_rot = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], np.float32)  # columns right (1,0,0), up (0,0,-1), forward (0,1,0)
    return {"meshes": meshes, "lights": [LIGHT], "materials": mats,
            "camera": {"position": np.float32([-0.5, 1.0, -2.0]), "matrix": cam_rot.reshape(9)}}


def _gauss(a, b, panels, k):
    x, w = np.polynomial.legendre.leggauss(k)
    edges = np.linspace(a, b, panels + 1)
    lo, hi = edges[:-1, None], edges[1:, None]
    return ((lo + hi) / 2 + (hi - lo) / 2 * x).ravel(), ((hi - lo) / 2 * w).ravel()


def expected_indirect(sc, w, h, nodes=8):
    """per pixel, float64: the indirect light averaged over the pixel (3 x 3 Gauss points) by Gauss-Legendre quadrature over
    the wall; biased points as the spec traces them (Po above the floor, the light seen from Qo in front of the wall)"""
    gy, wy = _gauss(*WALL_Y, 5, nodes)
    gz, wz = _gauss(*WALL_Z, 16, nodes)
    Y, Z = np.meshgrid(gy, gz, indexing="ij")
    Wq = np.outer(wy, wz).ravel()
    Q = np.stack([np.full(Y.size, WALL_X), Y.ravel(), Z.ravel()], axis=-1)
    lp, inten = np.float64(LIGHT[0]), LIGHT[1]
    Qo = Q - np.array([R.BIAS, 0.0, 0.0])
    Lq = lp - Qo
    r2 = np.sum(Lq * Lq, axis=-1)
    cos_l = -Lq[:, 0] / np.sqrt(r2)  # wall normal (-1, 0, 0) . (light - Qo) / r
    Lw = inten / (4.0 * math.pi * r2) * np.maximum(cos_l, 0.0)
    sx, sw = np.polynomial.legendre.leggauss(3)
    sx, sw = (sx + 1.0) / 2.0, sw / 2.0
    out = np.zeros((h, w))
    cam = sc["camera"]
    for jy, wyy in zip(sx, sw):
        for jx, wxx in zip(sx, sw):
            pix = np.arange(w * h)
            d = R.camera_dirs(cam["matrix"], pix % w, pix // w, np.full(w * h, jx), np.full(w * h, jy), w, h)
            P = np.float64(cam["position"]) + d * (cam["position"][1] / -d[:, 1])[:, None]
            Po = P + np.array([0.0, R.BIAS, 0.0])
            D = Q[None] - Po[:, None]
            d2 = np.sum(D * D, axis=-1)
            cos_p = D[..., 1] / np.sqrt(d2)
            cos_q = D[..., 0] / np.sqrt(d2)  # wall normal (-1, 0, 0) . (Po - Q) / d
            E = np.sum(Wq * Lw * cos_p * cos_q / (math.pi * d2), axis=1)
            out += wxx * wyy * E.reshape(h, w)
    return out


def test_interreflection_quadrature_converges():
    sc = interreflection_scene()
    a = expected_indirect(sc, 4, 4)
    assert np.all(a > 0.0)
    # half the nodes per panel give the same values: the integrand is smooth (the floor in view stays 0.5 from the wall)
    np.testing.assert_allclose(a, expected_indirect(sc, 4, 4, nodes=4), rtol=1e-6)


def check_indirect(diffs, expected, what, z_max=7.0, z2_max=2.0):
    """diffs: K x h x w x 3 (max_bounces 1 minus max_bounces 0, one per seed)"""
    K = diffs.shape[0]
    mean = diffs.mean(axis=0)
    se = diffs.std(axis=0, ddof=1) / math.sqrt(K)
    for c in range(3):
        want = RHO_F[c] * RHO_W[c] * expected
        z = (mean[..., c] - want) / se[..., c]
        assert np.abs(z).max() < z_max, "%s channel %d: |z| = %.1f" % (what, c, np.abs(z).max())
        assert np.mean(z * z) < z2_max, "%s channel %d: mean z^2 = %.2f" % (what, c, np.mean(z * z))
        assert abs(mean[..., c].mean() / want.mean() - 1.0) < 0.05, what


def test_oracle_interreflection(oracle):
    sc = interreflection_scene()
    cam = sc["camera"]
    w = h = 8
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    diffs = []
    try:
        for seed in range(16):
            f = []
            for mb in (1, 0):
                oracle.set_path_params(256, mb, 1000 + seed)
                f.append(O.render(cam["position"], cam["matrix"], 200, w, h, miss_rgb=(0, 0, 0), want=("rgb",))["rgb"])
            diffs.append(f[0].astype(np.float64) - f[1])
    finally:
        oracle.set_path_params(4, 3, 1234)
    check_indirect(np.stack(diffs), expected_indirect(sc, w, h), "oracle")


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _gpu_setup(r, sc):
    cam = sc["camera"]
    r.set_accumulation(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    r.set_camera(cam["position"], cam["matrix"])
    r.set_miss_color((0.0, 0.0, 0.0))
    r.change_shading_mode(200)


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [0, 1])
def test_gpu_form_factor(renderer, pipeline):
    """32 x 32 px x 4096 spp in each of the seven orientations"""
    mean_F, var_F = expected_form_factor_frame(32, 32, 4096, 5)
    try:
        renderer.set_option("path_pipeline", pipeline)
        for orient, n in ORIENTATIONS.items():
            _gpu_setup(renderer, form_factor_scene(n))
            renderer.set_path_params(4096, 1, 5)
            check_form_factor(renderer.render_frame(32, 32, want=("rgb",))["rgb"], mean_F, var_F, "gpu %s pipeline %d" % (orient, pipeline),
                              z2_max=1.3)
    finally:
        renderer.set_option("path_pipeline", 0)
        renderer.set_path_params(4, 3, 1234)
        renderer.set_miss_color((0.0, 1.0, 1.0))


@pytest.mark.gpu
def test_gpu_interreflection(renderer):
    sc = interreflection_scene()
    w = h = 16
    diffs = []
    _gpu_setup(renderer, sc)
    try:
        for seed in range(16):
            f = []
            for mb in (1, 0):
                renderer.set_path_params(4096, mb, 1000 + seed)
                f.append(renderer.render_frame(w, h, want=("rgb",))["rgb"])
            diffs.append(f[0].astype(np.float64) - f[1])
    finally:
        renderer.set_path_params(4, 3, 1234)
        renderer.set_miss_color((0.0, 1.0, 1.0))
    check_indirect(np.stack(diffs), expected_indirect(sc, w, h), "gpu", z2_max=1.6)
