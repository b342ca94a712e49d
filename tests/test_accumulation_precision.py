"""Precision of the per-pixel sample sums of mode 200.  A pixel whose every sample has the same value c (a miss, a directly seen
CONSTANT emitter) must resolve to float32(c) within 2 ulp however many samples it holds, up to the 2^24 that accumulation
allows.  Float32 running sums fail this long before: 65536 samples of 0.73 came out at 0.73039, 2^22 samples at 0.74569
(2 % high, about 4 RGBA8 steps; a numpy model of 2^24 samples is 9 % low).  The sums are float64 on both sides (path_kernels.hip loadSum / sumMean, oracle_render)."""
import time

import numpy as np
import pytest

MISS = (0.73, 0.3, 2.7)
EMIT = (0.73, 0.73, 0.73)
PER_CALL = 65536  # the largest spp of one call


def _scene(kind):
    """'miss': one small triangle behind the camera, every camera ray misses; 'emit': one CONSTANT triangle filling the view.
    One triangle, not a quad: a jittered ray through a shared edge can pass between the two triangles (Moeller-Trumbore is not
    watertight, on both sides alike) and take the miss colour."""
    if kind == "miss":
        v = np.float32([(0, 0, 5), (0.1, 0, 5), (0, 0.1, 5)])
        t = np.uint32([(0, 1, 2)])
        mats = [{"albedo": (1, 1, 1), "type": 1}]
    else:
        v = np.float32([(-100, -100, -2), (100, -100, -2), (0, 100, -2)])
        t = np.uint32([(0, 1, 2)])
        mats = [{"albedo": EMIT, "type": 4}]
    return {"meshes": [{"vertices": v, "triangles": t, "material_index": 0, "normals": None}], "lights": [], "materials": mats}


def _ulps(got, want):
    """distance in float32 ulps of want, per element"""
    want = np.float32(want)
    return np.abs(got.astype(np.float64) - np.float64(want)) / np.spacing(want).astype(np.float64)


def _check(rgb, kind, what):
    want = np.broadcast_to(np.float32(MISS if kind == "miss" else EMIT), rgb.shape)
    u = _ulps(rgb, want)
    assert u.max() <= 2.0, "%s: %s off by %.0f ulp (got %r, want %r)" % (what, kind, u.max(), rgb.reshape(-1, 3)[int(np.argmax(u.max(-1)))],
                                                                       want.reshape(-1, 3)[0])


@pytest.mark.parametrize("kind", ["miss", "emit"])
def test_oracle_long_frame_sum_is_exact(oracle, kind):
    """one oracle frame of 2^22 samples on two pixels"""
    sc = _scene(kind)
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    oracle.set_path_params(1 << 22, 1, 99)
    try:
        got = O.render((0, 0, 0), np.eye(3, dtype=np.float32).reshape(9), 200, 2, 1, miss_rgb=MISS)
    finally:
        oracle.set_path_params(4, 3, 1234)
    _check(got["rgb"], kind, "oracle 2^22 spp")


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _setup(r, kind):
    sc = _scene(kind)
    r.set_accumulation(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    r.set_camera((0, 0, 0), np.eye(3, dtype=np.float32).reshape(9))
    r.set_miss_color(MISS)
    r.change_shading_mode(200)


def _restore(r):
    r.set_accumulation(0)
    r.set_option("path_pipeline", 0)
    r.set_path_params(4, 3, 1234)
    r.set_miss_color((0.0, 1.0, 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("kind", ["miss", "emit"])
def test_gpu_one_frame_of_65536_samples(renderer, kind, pipeline):
    _setup(renderer, kind)
    try:
        renderer.set_option("path_pipeline", pipeline)
        renderer.set_path_params(PER_CALL, 1, 7)
        got = renderer.render_frame(16, 16)
    finally:
        _restore(renderer)
    _check(got["rgb"], kind, "one frame of %d spp, pipeline %d" % (PER_CALL, pipeline))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["miss", "emit"])
def test_gpu_accumulation_to_the_limit(renderer, kind):
    """64 calls of 65536 spp = 2^22 samples, then on to the 2^24 limit (256 calls) and one resolve-only frame"""
    _setup(renderer, kind)
    w = h = 8
    try:
        renderer.set_path_params(PER_CALL, 1, 7)
        renderer.set_accumulation(1 << 24)
        t0 = time.perf_counter()
        for _ in range(64):
            got = renderer.render_frame(w, h, want=("rgb",))
        dt = (time.perf_counter() - t0) / 64
        assert renderer.accumulated_samples() == 1 << 22
        _check(got["rgb"], kind, "2^22 accumulated samples")
        for _ in range(256 - 64):
            got = renderer.render_frame(w, h, want=("rgb",))
        assert renderer.accumulated_samples() == 1 << 24
        _check(got["rgb"], kind, "2^24 accumulated samples")
        again = renderer.render_frame(w, h, want=("rgb",))  # at the limit: nothing traced, the stored sums resolved again
        assert again["stats"]["rays_primary"] == 0
        np.testing.assert_array_equal(again["rgb"], got["rgb"])
    finally:
        _restore(renderer)
    print("%s: %.2f ms per call of %d spp at %dx%d" % (kind, 1e3 * dt, PER_CALL, w, h))
