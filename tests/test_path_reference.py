"""Mode 200 (path tracing) against an independent float64 reference of the documented spec (tests/path_reference.py).

The bit-exact suite pins the kernels to the CPU oracle; this module pins both to the spec.  At 1 spp a pixel's rgb is one
path, and the reference draws the same random numbers, so each pixel is compared with its float64 path: the cosine-weighted
bounce, the orthonormal basis (both signs of copysign, N.z = +0 and -0), mirrors, Snell's law with entering / exiting and total
internal reflection, origin biases, throughput products, the max_bounces cut per material and the miss colour after bounces.

Tolerance per colour channel: 1e-4 x (closest-hit segments of the path) x |reference| + 1e-5.  A float32 segment carries
relative errors of a few 1e-6 (measured: at most 4e-5 over a 6-segment path); any change of formula moves a pixel by far more.
Paths with a decision margin below path_reference.MARGINS are skipped; at most 3 % may be, per frame."""
from collections import Counter

import numpy as np
import pytest

import path_reference as R

W = H = 32
BOUNCES = (0, 1, 2, 5)
SEEDS = (0, 0xFFFFFFFF, 1234)
MAX_SKIPPED = 0.03
RTOL_SEG, ATOL = 1e-4, 1e-5

# what each scene must make the paths do (summed over its frames), so that no check is vacuous
COVERAGE = {
    "room": ("diffuse_bounce", "basis_sg+", "basis_sg-", "basis_nz=+0", "basis_nz=-0", "shadowed", "light_behind", "lit"),
    "mirrors": ("mirror", "mirror_cut", "emit_direct", "emit_after_mirror", "emit_after_diffuse", "miss_direct",
                "miss_after_bounce", "shadowed", "lit"),
    "slab": ("enter", "exit", "tir", "refract_cut", "miss_after_bounce", "diffuse_bounce"),
    "prism": ("enter", "exit", "tir", "refract_cut"),
    "sphere": ("enter", "exit", "refract_cut", "miss_after_bounce"),
    "textured_room": ("tex_albedo", "tex_edges", "tex_checker", "tex_bitmap", "checker_negative", "checker_above_1",
                      "bitmap_u_low", "bitmap_u_high", "bitmap_v_low", "bitmap_v_high", "edges_edge", "edges_inner",
                      "tex_index_past_table", "tex_after_bounce", "diffuse_bounce", "shadowed", "lit"),
    "textured_glass": ("tex_albedo", "tex_checker", "tex_bitmap", "tex_on_glass_or_mirror", "tex_after_bounce", "checker_negative",
                       "checker_above_1", "bitmap_u_low", "bitmap_u_high", "bitmap_v_high", "enter", "exit", "mirror", "refract_cut"),
}
TEXTURED = ("textured_room", "textured_glass")
# texture events that mode 100 at pixel centres must see as well (every material shaded as diffuse)
CENTRE_COVERAGE = {
    "textured_room": ("tex_albedo", "tex_edges", "tex_checker", "tex_bitmap", "checker_negative", "checker_above_1", "bitmap_u_low",
                      "bitmap_u_high", "bitmap_v_low", "bitmap_v_high", "edges_edge", "edges_inner", "tex_index_past_table"),
    "textured_glass": ("tex_albedo", "tex_checker", "tex_bitmap", "tex_on_glass_or_mirror", "checker_negative", "checker_above_1"),
}


def compare_path_frame(got, ref, what):
    """got: a mode-200 frame at 1 spp (render_frame / OracleScene.render outputs); ref: trace_paths of the same frame"""
    rb = ref["robust"]
    skipped = 1.0 - float(rb.mean())
    assert skipped < MAX_SKIPPED, "%s: %.1f %% of the paths skipped" % (what, 100 * skipped)
    np.testing.assert_array_equal(got["hit_inst"][rb], ref["inst"][rb], err_msg=what + ": hit_inst")
    np.testing.assert_array_equal(got["hit_prim"][rb], ref["prim"][rb], err_msg=what + ": hit_prim")
    np.testing.assert_allclose(got["hit_t"][rb], ref["t"][rb], rtol=1e-5, err_msg=what + ": hit_t")
    err = np.abs(got["rgb"].astype(np.float64) - ref["rgb"])
    tol = RTOL_SEG * ref["segments"][..., None] * np.abs(ref["rgb"]) + ATOL
    bad = np.any(err > tol, axis=-1) & rb
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError("%s: %d pixels off the float64 paths, first (%d, %d): got %s, float64 %s (%d segments)"
                             % (what, int(bad.sum()), x, y, got["rgb"][y, x], ref["rgb"][y, x], ref["segments"][y, x]))
    return skipped


def compare_centres(got, S, cam, mode, miss, ks=0.0, exponent=32, ev=None):
    rgb, rb, inst, prim, t = R.shade_centres(S, cam["position"], cam["matrix"], W, H, mode, miss, ks, exponent, ev=ev)
    assert rb.mean() > 1.0 - MAX_SKIPPED
    np.testing.assert_array_equal(got["hit_inst"][rb], inst[rb])
    np.testing.assert_array_equal(got["hit_prim"][rb], prim[rb])
    np.testing.assert_allclose(got["hit_t"][rb], t[rb], rtol=1e-5)
    tol = (2e-5 if mode == 3 else 1e-4 * np.abs(rgb[rb]) + 1e-6)
    assert np.all(np.abs(got["rgb"][rb] - rgb[rb]) <= tol), "mode %d off the float64 reference" % mode


@pytest.fixture(scope="module")
def built(scenes):
    out = {}
    for name, fn in R.SCENES.items():
        sc = fn(scenes)
        assert sum(len(m["triangles"]) for m in sc["meshes"]) < 200
        out[name] = (sc, R.Scene(sc))
    return out


def _references(built, name):
    sc, S = built[name]
    cam = sc["camera"]
    for mb in BOUNCES:
        for seed in SEEDS:
            yield mb, seed, R.trace_paths(S, cam["position"], cam["matrix"], W, H, R.MISS_RGB, mb, seed)


# ---- CPU: the oracle against the float64 paths

@pytest.mark.parametrize("name", list(R.SCENES))
def test_oracle_paths_equal_float64_reference(oracle, built, name):
    sc, _ = built[name]
    cam = sc["camera"]
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], textures=sc.get("textures", ()))
    ev = {}
    try:
        for mb, seed, ref in _references(built, name):
            oracle.set_path_params(1, mb, seed)
            got = O.render(cam["position"], cam["matrix"], 200, W, H, miss_rgb=R.MISS_RGB)
            compare_path_frame(got, ref, "%s max_bounces=%d seed=%d" % (name, mb, seed))
            for k, v in ref["ev"].items():
                ev[k] = ev.get(k, 0) + v
    finally:
        oracle.set_path_params(4, 3, 1234)
    missing = [k for k in COVERAGE[name] if ev.get(k, 0) == 0]
    assert not missing, "scene %s never exercised %s" % (name, missing)


def test_oracle_centre_modes_equal_float64_reference(oracle, built):
    for name in ("room", "prism") + TEXTURED:
        sc, S = built[name]
        cam = sc["camera"]
        ev = Counter()
        O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], textures=sc.get("textures", ()))
        try:
            for mode in (3, 5, 100):
                oracle.set_phong(250 if mode == 100 else 0, 16)
                got = O.render(cam["position"], cam["matrix"], mode, W, H, miss_rgb=R.MISS_RGB)
                compare_centres(got, S, cam, mode, R.MISS_RGB, 0.25 if mode == 100 else 0.0, 16, ev=ev)
        finally:
            oracle.set_phong(0, 32)
        missing = [k for k in CENTRE_COVERAGE.get(name, ()) if ev[k] == 0]
        assert not missing, "scene %s: mode 100 never exercised %s" % (name, missing)


def test_reference_rng_is_the_spec_hash():
    """pcg_hash known answers (computed by hand from RXS-M-XS 32) and the 24-bit float"""
    assert int(R.pcg_hash(np.uint32(0))) == 129708002
    assert int(R.pcg_hash(np.uint32(1))) == 2831084092
    st, u = R.rng_next(np.uint32(0))
    assert float(u) == (129708002 >> 8) * 2.0 ** -24 and 0.0 <= float(u) < 1.0


# ---- GPU: the kernels (persistent kernel and stage launches) against the float64 paths

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("name", list(R.SCENES))
def test_gpu_paths_equal_float64_reference(renderer, built, name, pipeline):
    sc, _ = built[name]
    cam = sc["camera"]
    r = renderer
    r.set_accumulation(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"))
    r.set_camera(cam["position"], cam["matrix"])
    r.set_miss_color(R.MISS_RGB)
    r.change_shading_mode(200)
    r.set_option("path_pipeline", pipeline)
    try:
        for mb, seed, ref in _references(built, name):
            r.set_path_params(1, mb, seed)
            got = r.render_frame(W, H)
            compare_path_frame(got, ref, "%s max_bounces=%d seed=%d pipeline=%d" % (name, mb, seed, pipeline))
    finally:
        r.set_option("path_pipeline", 0)
        r.set_path_params(4, 3, 1234)
        r.set_miss_color((0.0, 1.0, 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["room", "prism", "sphere"] + list(TEXTURED))
def test_gpu_centre_modes_equal_float64_reference(renderer, built, name):
    """modes 3 (barycentrics), 5 (distance) and 100 (Lambert + Phong, ks 0.25, exponent 16) at pixel centres"""
    sc, S = built[name]
    cam = sc["camera"]
    r = renderer
    r.set_accumulation(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"))
    r.set_camera(cam["position"], cam["matrix"])
    r.set_miss_color(R.MISS_RGB)
    try:
        for mode in (3, 5, 100):
            r.change_shading_mode(mode)
            r.set_option("phong_ks", 250 if mode == 100 else 0)
            r.set_option("phong_exponent", 16)
            compare_centres(r.render_frame(W, H), S, cam, mode, R.MISS_RGB, 0.25 if mode == 100 else 0.0, 16)
    finally:
        r.set_option("phong_ks", 0)
        r.set_option("phong_exponent", 32)
        r.set_miss_color((0.0, 1.0, 1.0))
