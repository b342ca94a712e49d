"""Shading mode 150 (CRT_MODE_WHITTED, include/crt_hip.h "Whitted shading"): mode 100 seen through mirrors and glass, for
crt_shade_rays*, crt_render_frame*, crt::Renderer and crt_render.

Three references hold it.  Where nothing is specular it is mode 100, byte for byte.  Along a specular chain it is the pinned
mode-200 path code: with phong_ks = 0 a record whose chain has k turns gives, at max_bounces = B, the rgb of path_rays at one
sample with max_bounces = min(B, k), byte for byte (at one sample path_rays returns its single radiance exactly; a chain cut
short is black in both; at max_bounces = k the path ends at its first non-specular surface without drawing a bounce; with
ks = 0 addLight<false> and addLight<true> are the same arithmetic).  And everywhere, Phong included, it is the float64
restatement of the contract in tests/whitted_reference.py, within the tolerance of tests/test_path_reference.py: per channel
1e-4 x segments x |reference| + 1e-5, hit_t at rtol 1e-5, ids equal, on the records whose decisions clear
path_reference.MARGINS, of which at most 3 % of a frame may fail to."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import path_reference as R
import whitted_reference as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 32
N = W * H
MISS = 0xFFFFFFFF
BOUNCES = (0, 1, 2, 5, 8)
PHONG = ((0.0, 0), (0.25, 250))  # ks, and the option "phong_ks" in thousandths
EXPONENT = 16
MAX_SKIPPED = 0.03
RTOL_SEG, ATOL = 1e-4, 1e-5
PLAIN = ("room", "textured_room")
SPECULAR = ("mirrors", "slab", "prism", "sphere", "textured_glass")
OUTPUTS = ("rgb", "normal", "albedo", "t", "uv", "inst", "prim")
FRAME_OUTPUTS = ("rgba8", "hit_inst", "hit_prim", "hit_t", "rgb")

# what each scene must make the records do (summed over its frames), so that no check is vacuous
COVERAGE = {
    "mirrors": ("mirror", "mirror_cut", "emit_after_turn", "miss_after_turn", "lit_after_turn", "shadowed_after_turn"),
    "slab": ("enter", "exit", "tir", "refract_cut", "diffuse_after_turn"),
    "prism": ("enter", "exit", "tir", "refract_cut", "diffuse_after_turn"),
    "sphere": ("enter", "exit", "tir", "refract_cut", "diffuse_after_turn"),
    "textured_glass": ("mirror", "enter", "exit", "tex_on_glass_or_mirror"),
}
EIGHT_TURNS = ("sphere", "textured_glass")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def built(scenes):
    out = {}
    for name, fn in R.SCENES.items():
        sc = fn(scenes)
        assert sum(len(m["triangles"]) for m in sc["meshes"]) < 200
        out[name] = (sc, R.Scene(sc))
    return out


@pytest.fixture(scope="module")
def refs(built):
    """the float64 reference of a scene's 32 x 32 frame at (max_bounces, ks), computed once and never modified"""
    memo = {}

    def get(name, mb, ks):
        key = (name, mb, ks)
        if key not in memo:
            sc, S = built[name]
            cam = sc["camera"]
            ref = WR.centres(S, cam["position"], cam["matrix"], W, H, R.MISS_RGB, mb, ks, EXPONENT)
            for a in ref.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            memo[key] = ref
        return memo[key]
    return get


# ---- CPU: the interface, the driver's refusal, and the reference against the project's other float64 references

def test_header_and_driver_name_the_mode(pkg):
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    assert "#define CRT_MODE_WHITTED 150u" in header
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "crt_render")
    assert os.path.exists(exe), "crt_render not built"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "150" in out.stderr, "--help names the mode"


@pytest.mark.parametrize("args", [["--mode", "150", "--ranks", "2"], ["--mode-at", "3:150", "--ranks", "2"],
                                  ["--mode", "150", "--ranks", "2", "--rank", "0", "--id-file", "none"]])
def test_driver_refuses_ranks_at_argument_parsing(pkg, golden_dir, args):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "crt_render")
    out = subprocess.run([exe, os.path.join(golden_dir, "dragon.crtscene")] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "150" in out.stderr and "usage" not in out.stderr, out.stderr


@pytest.mark.parametrize("name", PLAIN)
def test_reference_is_mode_100_where_nothing_is_specular(built, refs, name):
    sc, S = built[name]
    cam = sc["camera"]
    for ks, _ in PHONG:
        rgb, rb, inst, prim, t = R.shade_centres(S, cam["position"], cam["matrix"], W, H, 100, R.MISS_RGB, ks, EXPONENT)
        for mb in (0, 5):
            ref = refs(name, mb, ks)
            assert np.array_equal(ref["rgb"], rgb) and np.array_equal(ref["robust"], rb)
            assert np.array_equal(ref["inst"], inst) and np.array_equal(ref["prim"], prim) and np.array_equal(ref["t"], t)
            assert not ref["turns"].any() and np.all(ref["segments"] == 1)


@pytest.mark.parametrize("name", SPECULAR)
def test_reference_is_the_float64_path_on_a_specular_chain(built, name):
    """with every non-specular material made CONSTANT a mode-200 path is its specular chain: trace_paths at one sample, on its
    own jittered camera rays, is the reference to 1e-12"""
    sc, _ = built[name]
    cam = sc["camera"]
    S = R.Scene(WR.specular_only(sc))
    seed = 1234
    pix = np.arange(N, dtype=np.uint32)
    st = R.rng_start(pix, np.zeros(N, np.uint32), seed)
    st, jx = R.rng_next(st)
    st, jy = R.rng_next(st)
    o = np.repeat(np.float32(cam["position"]).astype(np.float64)[None], N, axis=0)
    d = R.camera_dirs(cam["matrix"], pix % W, pix // W, jx, jy, W, H)
    turned = 0
    for mb in BOUNCES:
        path = R.trace_paths(S, cam["position"], cam["matrix"], W, H, R.MISS_RGB, mb, seed)
        got = WR.trace(S, o, d, R.MISS_RGB, mb)
        np.testing.assert_allclose(got["rgb"], path["rgb"].reshape(-1, 3), rtol=1e-12, atol=1e-12)
        assert np.array_equal(got["segments"], path["segments"].reshape(-1)) and np.array_equal(got["robust"], path["robust"].reshape(-1))
        assert np.array_equal(got["inst"], path["inst"].reshape(-1)) and np.array_equal(got["t"], path["t"].reshape(-1))
        turned += int(got["turns"].sum())
    assert turned > 0


@pytest.mark.parametrize("name", list(R.SCENES))
def test_reference_skips_little_and_covers_the_contract(refs, name):
    ev = Counter()
    most = 0
    for mb in BOUNCES:
        ref = refs(name, mb, 0.0)
        assert 1.0 - ref["robust"].mean() < MAX_SKIPPED
        assert ref["turns"].max() <= mb and np.all(ref["segments"] == ref["turns"] + 1)
        ev.update(ref["ev"])
        most = max(most, int(ref["turns"][ref["robust"]].max()))
    missing = [k for k in COVERAGE.get(name, ()) if ev[k] == 0]
    assert not missing, "scene %s never exercised %s" % (name, missing)
    if name in EIGHT_TURNS:
        assert most == 8
    if name in PLAIN:
        assert most == 0


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _setup(r, sc, miss=R.MISS_RGB, ks=0):
    r.set_accumulation(0)
    r.set_counting(False)
    r.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"))
    r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
    r.set_miss_color(miss)
    r.set_option("phong_ks", ks)
    r.set_option("phong_exponent", EXPONENT)


def _restore(r):
    r.set_counting(False)
    r.set_option("phong_ks", 0)
    r.set_option("phong_exponent", 32)
    r.set_option("max_bounces", 3)
    r.set_option("stack_entries", 0)
    r.set_option("path_pass_paths", 1 << 24)
    r.set_miss_color((0.0, 1.0, 1.0))
    r.change_shading_mode(0)


def _same(a, b, keys, what):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), "%s: %s" % (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [0, 250])
@pytest.mark.parametrize("name", PLAIN)
def test_equal_to_mode_100_where_nothing_is_specular(renderer, built, name, ks):
    """every output of shade_rays and of render_frame, and the counted rays, at max_bounces 0 and 5"""
    r = renderer
    sc, _ = built[name]
    try:
        _setup(r, sc, ks=ks)
        rays = r.camera_rays(W, H)
        r.set_counting(True)
        r.change_shading_mode(100)
        want_q, want_f = r.shade_rays(rays), r.render_frame(W, H)
        assert want_q["stats"]["rays_shadow"] > 0 and (want_q["inst"] != MISS).sum() > N // 2
        for mb in (0, 5):
            r.set_option("max_bounces", mb)
            r.change_shading_mode(150)
            got_q, got_f = r.shade_rays(rays), r.render_frame(W, H)
            what = "%s ks=%d max_bounces=%d" % (name, ks, mb)
            _same(got_q, want_q, OUTPUTS, what + " shade_rays")
            _same(got_f, want_f, FRAME_OUTPUTS, what + " render_frame")
            for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested"):
                assert got_q["stats"][k] == want_q["stats"][k], "%s shade_rays: %s" % (what, k)
            for k in ("rays_primary", "rays_shadow"):  # (the frame kernel of mode 100 walks packets: its fetch counts are its own)
                assert got_f["stats"][k] == want_f["stats"][k], "%s render_frame: %s" % (what, k)
    finally:
        _restore(r)


@pytest.mark.gpu
def test_equal_to_the_pinned_path_code_along_the_chain(renderer, built, refs):
    """module docstring, second reference.  The chain length k of every record comes from pinned code alone: path_rays on a
    copy of the scene whose non-specular materials are white CONSTANT, under a white miss colour, first gives a non-zero
    colour at max_bounces = k (8 if never)."""
    r = renderer
    lengths, ends = Counter(), Counter()
    try:
        for name in SPECULAR:
            sc, _ = built[name]
            _setup(r, WR.specular_only(sc), miss=(1.0, 1.0, 1.0))
            rays = r.camera_rays(W, H)
            r.set_counting(True)
            k = np.full(N, 8)
            for mb in range(8, -1, -1):
                r.set_option("max_bounces", mb)
                path = r.path_rays(rays, n_samples=1, want=("rgb",))
                k[np.any(path["rgb"] != 0.0, axis=1)] = mb
                r.change_shading_mode(150)
                got = r.shade_rays(rays, want=("rgb",))
                assert got["stats"]["rays_primary"] == path["stats"]["rays_primary"], "%s max_bounces=%d: closest-hit rays" % (name, mb)
                assert got["stats"]["rays_primary"] >= N
            _setup(r, sc)
            paths = []
            for mb in range(9):
                r.set_option("max_bounces", mb)
                paths.append(r.path_rays(rays, n_samples=1, want=("rgb",))["rgb"])
            paths = np.stack(paths)
            r.change_shading_mode(150)
            for mb in range(9):
                r.set_option("max_bounces", mb)
                got = r.shade_rays(rays, want=("rgb",))["rgb"]
                want = paths[np.minimum(mb, k), np.arange(N)]
                bad = np.flatnonzero(np.any(_bits(got) != _bits(want), axis=1))
                assert len(bad) == 0, "%s max_bounces=%d: %d records differ from the path code, first %d (k = %d): %s, path %s" % (
                    name, mb, len(bad), bad[0], k[bad[0]], got[bad[0]], want[bad[0]])
            lengths.update(np.minimum(k, 4).tolist())
            ref = refs(name, 8, 0.0)
            ends.update(ref["end"][ref["robust"]].tolist())
            sure = ref["robust"].reshape(-1)
            assert np.array_equal(k[sure], ref["turns"].reshape(-1)[sure]), name + ": the chain lengths are the float64 reference's"
    finally:
        _restore(r)
    assert all(lengths[i] > 0 for i in (0, 1, 2, 4)), "chain lengths 0, 1, 2 and >= 4: %s" % dict(lengths)
    assert all(ends[e] > 0 for e in (WR.END_MISS, WR.END_CONSTANT, WR.END_LIT, WR.END_SHADOWED)), "miss, constant, lit, shadowed: %s" % dict(ends)


def _compare(got, ref, what, worst):
    """got: inst / prim / t / rgb shaped as the reference's; worst: the largest error / tolerance seen so far, updated"""
    rb = ref["robust"]
    skipped = 1.0 - float(rb.mean())
    assert skipped < MAX_SKIPPED, "%s: %.1f %% of the records skipped" % (what, 100 * skipped)
    np.testing.assert_array_equal(got["inst"][rb], ref["inst"][rb], err_msg=what + ": inst")
    np.testing.assert_array_equal(got["prim"][rb], ref["prim"][rb], err_msg=what + ": prim")
    np.testing.assert_allclose(got["t"][rb], ref["t"][rb], rtol=1e-5, err_msg=what + ": t")
    err = np.abs(got["rgb"].astype(np.float64) - ref["rgb"])
    tol = RTOL_SEG * ref["segments"][..., None] * np.abs(ref["rgb"]) + ATOL
    ratio = np.where(rb[..., None], err / tol, 0.0)
    worst[0] = max(worst[0], float(ratio.max()))
    bad = np.any(ratio > 1.0, axis=-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError("%s: %d records off the float64 reference (worst error / tolerance %.2f), first (%d, %d): got %s, float64 %s (%d segments)"
                             % (what, int(bad.sum()), ratio.max(), x, y, got["rgb"][y, x], ref["rgb"][y, x], ref["segments"][y, x]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.SCENES))
def test_equal_to_the_float64_contract(renderer, built, refs, name):
    """frames and shade_rays at max_bounces 0, 1, 2, 5, 8, Phong off and on (ks 0.25, exponent 16), against
    tests/whitted_reference.py; the frame's rgb is shade_rays of its camera rays byte for byte.  Measured on an MI355X: the
    worst error / tolerance of a robust pixel is 0.040 (sphere; 0.006 .. 0.035 on the other scenes), printed per scene below"""
    r = renderer
    sc, _ = built[name]
    worst = [0.0]
    try:
        _setup(r, sc)
        rays = r.camera_rays(W, H)
        r.change_shading_mode(150)
        for ks, option in PHONG:
            r.set_option("phong_ks", option)
            for mb in BOUNCES:
                r.set_option("max_bounces", mb)
                ref = refs(name, mb, ks)
                what = "%s max_bounces=%d ks=%g" % (name, mb, ks)
                f = r.render_frame(W, H)
                _compare({"inst": f["hit_inst"], "prim": f["hit_prim"], "t": f["hit_t"], "rgb": f["rgb"]}, ref, what + " frame", worst)
                q = r.shade_rays(rays, want=("rgb", "t", "inst", "prim"))
                assert np.array_equal(_bits(q["rgb"]), _bits(f["rgb"]).reshape(-1, 3)), what + ": frame rgb != shade_rays of camera_rays"
                assert np.array_equal(_bits(q["t"]), _bits(f["hit_t"]).reshape(-1)) and np.array_equal(q["inst"], f["hit_inst"].reshape(-1))
                assert np.array_equal(q["prim"], f["hit_prim"].reshape(-1))
                unorm = (np.clip(np.nan_to_num(f["rgb"], nan=0.0), 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
                assert np.array_equal(f["rgba8"][..., :3], unorm) and np.all(f["rgba8"][..., 3] == 255), what + ": rgba8"
                assert np.all(f["hit_t"][f["hit_inst"] == MISS] == np.float32(10000.0))
    finally:
        _restore(r)
        print("%s: worst error / tolerance %.3f" % (name, worst[0]))


def _enter(r, built):
    """the state the plain trace was taken in: textured_glass, max_bounces 5, Phong on, mode 150"""
    _setup(r, built["textured_glass"][0], ks=250)
    r.set_option("max_bounces", 5)
    r.change_shading_mode(150)


@pytest.fixture(scope="module")
def plain_trace(renderer, built):
    """textured_glass (mirror, glass, textures, two lights) at max_bounces 5 with Phong on: its 1024 camera rays traced plainly,
    with counting.  Computed once, never modified; a test that uses it enters the same state first (_enter)."""
    r = renderer
    _enter(r, built)
    rays = r.camera_rays(W, H)
    r.set_counting(True)
    base = r.shade_rays(rays)
    r.set_counting(False)
    for a in list(base.values()) + [rays]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    assert base["stats"]["rays_primary"] > N and base["stats"]["rays_shadow"] > 0
    _restore(r)
    return rays, base


@pytest.mark.gpu
def test_scheduling_changes_nothing(renderer, built, plain_trace):
    """record counts around a wavefront, a random permutation (lanes refilled in another order, chains of different length in
    one wavefront), a one-entry LDS stack (every push spills), counting on and off, blocks of records ("path_pass_paths")"""
    r = renderer
    rays, base = plain_trace
    _enter(r, built)
    for n in (1, 63, 64, 65, 1024):
        got = r.shade_rays(np.ascontiguousarray(rays[:n]))
        _same(got, {k: base[k][:n] for k in OUTPUTS}, OUTPUTS, "%d records" % n)
        assert got["stats"]["rays_primary"] == n
    order = np.random.default_rng(150).permutation(N)
    got = r.shade_rays(np.ascontiguousarray(rays[order]))
    _same(got, {k: base[k][order] for k in OUTPUTS}, OUTPUTS, "permuted")
    try:
        r.set_option("stack_entries", 1)
        r.set_counting(True)
        got = r.shade_rays(rays)
        _same(got, base, OUTPUTS, "stack_entries=1")
        for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested"):
            assert got["stats"][k] == base["stats"][k], "stack_entries=1: " + k
        r.set_option("stack_entries", 0)
        _same(r.shade_rays(rays), base, OUTPUTS, "counting")
        r.set_counting(False)
        # 65 x 1024 records in blocks of 65536: the second block holds the last 1024
        r.set_option("path_pass_paths", 1 << 16)
        got = r.shade_rays(np.tile(rays, (65, 1)))
        _same(got, {k: np.tile(base[k], (65,) + (1,) * (base[k].ndim - 1)) for k in OUTPUTS}, OUTPUTS, "two blocks")
    finally:
        _restore(r)


@pytest.mark.gpu
def test_each_output_alone_and_device_buffers(renderer, built, plain_trace):
    import torch
    r = renderer
    rays, base = plain_trace
    _enter(r, built)
    for k in OUTPUTS:
        got = r.shade_rays(rays, want=(k,))
        assert np.array_equal(_bits(got[k]), _bits(base[k])), k
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    shapes = {"rgb": (3, torch.float32), "normal": (3, torch.float32), "albedo": (3, torch.float32), "t": (1, torch.float32),
              "uv": (2, torch.float32), "inst": (1, torch.int32), "prim": (1, torch.int32)}
    out = {k: torch.zeros(N * c, dtype=dt, device="cuda") for k, (c, dt) in shapes.items()}
    r.shade_rays_device(N, d_rays.data_ptr(), **{"d_" + k: v.data_ptr() for k, v in out.items()})
    r.synchronize()
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert np.array_equal(out[k].cpu().numpy().view(np.uint32), _bits(base[k]).reshape(-1).view(np.uint32)), k
    frame = {"rgba8": torch.zeros(N, dtype=torch.int32, device="cuda"), "rgb": torch.zeros(3 * N, dtype=torch.float32, device="cuda")}
    r.render_frame_device(W, H, frame["rgba8"].data_ptr(), d_rgb=frame["rgb"].data_ptr())
    only = torch.zeros(N, dtype=torch.int32, device="cuda")
    r.render_frame_device(W, H, only.data_ptr())  # no float colour wanted: the query writes it to scratch
    r.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(frame["rgb"].cpu().numpy().view(np.uint32), _bits(base["rgb"]).reshape(-1))
    assert bool((only == frame["rgba8"]).all().item()) and bool((only != 0).all().item())
    _restore(r)


@pytest.mark.gpu
def test_untraced_records_and_an_empty_scene(renderer, built, plain_trace):
    """a NaN anywhere and an empty interval give the miss colour and mode 100's other outputs; so does every record in an empty scene"""
    r = renderer
    rays, base = plain_trace
    _enter(r, built)
    hitting = np.array(rays[np.flatnonzero(base["inst"] != MISS)[0]])
    bad = []
    for f in range(8):
        rec = hitting.copy()
        rec[f] = np.nan
        bad.append(rec)
    for tmin, tmax in ((1.0, 1.0), (2.0, 1.0)):
        rec = hitting.copy()
        rec[3], rec[7] = tmin, tmax
        bad.append(rec)
    buf = np.stack(bad + [hitting]).astype(np.float32)
    nb = len(bad)
    got = r.shade_rays(buf)
    r.change_shading_mode(100)
    lambert = r.shade_rays(buf)
    r.change_shading_mode(150)
    _same({k: got[k][:nb] for k in OUTPUTS}, {k: lambert[k][:nb] for k in OUTPUTS}, OUTPUTS, "untraced records")
    assert np.array_equal(_bits(got["rgb"][:nb]), _bits(np.tile(np.float32(R.MISS_RGB), (nb, 1)))) and np.all(got["inst"][:nb] == MISS)
    assert got["inst"][nb] != MISS, "the control record hits"
    try:
        r.upload([], [], [])
        e = r.shade_rays(rays)
        assert np.all(e["inst"] == MISS) and np.array_equal(_bits(e["rgb"]), _bits(np.tile(np.float32(R.MISS_RGB), (N, 1))))
        assert np.all(e["normal"] == 0.0) and np.all(e["albedo"] == 0.0) and np.array_equal(_bits(e["t"]), _bits(rays[:, 7]))
        f = r.render_frame(W, H)
        assert np.all(f["hit_inst"] == MISS) and np.array_equal(_bits(f["rgb"]).reshape(-1, 3), _bits(e["rgb"]))
    finally:
        _restore(r)


@pytest.mark.gpu
def test_frames_of_other_modes_and_refusals(pkg, renderer, built, plain_trace):
    """a mode-100 frame before and after a mode-150 frame; mode 200 still refused by shade_rays; mode 150 refused, with
    CRT_EINVAL and a message naming it, by the tile, batch and distributed entries"""
    import torch
    r = renderer
    rays, base = plain_trace
    _enter(r, built)
    try:
        r.change_shading_mode(100)
        before = [r.render_frame(W, H) for _ in range(2)][-1]
        r.change_shading_mode(150)
        whitted = r.render_frame(W, H)
        r.change_shading_mode(100)
        after = r.render_frame(W, H)
        _same(before, after, FRAME_OUTPUTS, "mode 100 around a mode-150 frame")
        assert not np.array_equal(_bits(whitted["rgb"]), _bits(before["rgb"])), "the mirror and the glass show"
        r.change_shading_mode(200)
        with pytest.raises(pkg.CrtError, match="200"):
            r.shade_rays(rays)
        r.change_shading_mode(150)
        d = torch.full((4 * N,), 7, dtype=torch.int32, device="cuda")
        calls = [lambda: r.render_tiles_device(W, H, 0, 1, d.data_ptr()), lambda: r.render_tiles_device(W, H, 1, 2, d.data_ptr()),
                 lambda: r.render_frames_batch_device(W, H, [d.data_ptr()]), lambda: r.render_tiles_batch_device(W, H, 0, 1, [d.data_ptr()]),
                 lambda: r.render_frame_distributed(W, H, host=True)]
        for call in calls:
            with pytest.raises(pkg.CrtError) as e:
                call()
            assert "rc=1:" in str(e.value) and "150" in str(e.value), str(e.value)
        r.synchronize()
        torch.cuda.synchronize()
        assert bool((d == 7).all().item()), "a refused call writes nothing"
        _same(r.render_frame(W, H), whitted, FRAME_OUTPUTS, "mode 150 after the refusals")
    finally:
        _restore(r)


@pytest.mark.gpu
def test_cpp_layer_and_driver(pkg, scenes, renderer, tmp_path):
    """crt::Renderer::renderFrame and shadeRays in mode 150, from a small C++ program linked against libcrt_hip.so, and the
    frames crt_render writes, are the binding's"""
    exe = str(tmp_path / "whitted_cpp")
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(lib_dir, "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "whitted_cpp.cpp"), "-L" + lib_dir, "-lcrt_hip",
                           "-Wl,-rpath," + lib_dir, "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    w, h, mb = 40, 24, 4
    n = w * h
    scene = pkg.Scene.from_arrays(R.scene_mirrors(scenes))
    path = str(tmp_path / "mirrors.crtbin")
    scene.save(path)
    out = str(tmp_path / "out.bin")
    subprocess.check_call([exe, path, str(w), str(h), str(mb), out], timeout=120)
    raw = np.fromfile(out, dtype=np.uint32)
    assert raw.size == n + 3 * n + 14 * n
    rgba8, rgb, hits = raw[:n], raw[n:4 * n].reshape(n, 3), raw[4 * n:].reshape(n, 14)
    r = renderer
    try:
        r.set_accumulation(0)
        r.upload_scene(scene)
        r.set_camera_from(scene)
        r.set_option("max_bounces", mb)
        r.change_shading_mode(100)
        lambert = r.render_frame(w, h)
        r.change_shading_mode(150)
        frame = r.render_frame(w, h)
        assert not np.array_equal(frame["rgba8"], lambert["rgba8"]), "the mirrors show"
        assert np.array_equal(rgba8, frame["rgba8"].reshape(-1, 4).view(np.uint32).reshape(-1)) and np.array_equal(rgb, _bits(frame["rgb"]).reshape(-1, 3))
        ref = r.shade_rays(r.camera_rays(w, h))
        for k, cols in (("rgb", slice(0, 3)), ("normal", slice(3, 6)), ("albedo", slice(6, 9)), ("uv", slice(10, 12))):
            assert np.array_equal(hits[:, cols], _bits(ref[k])), k
        assert np.array_equal(hits[:, 9], _bits(ref["t"])) and np.array_equal(hits[:, 12], ref["inst"]) and np.array_equal(hits[:, 13], ref["prim"])

        tool = os.path.join(lib_dir, "crt_render")
        size = ["--size", "%dx%d" % (w, h), "--bounces", str(mb)]
        subprocess.check_call([tool, path, "--mode", "100", "--mode-at", "1:150", "--frames", "2", "--out", str(tmp_path / "f")] + size,
                              timeout=120, stdout=subprocess.DEVNULL)
        for i, want in enumerate((lambert, frame)):
            raw = open(str(tmp_path / ("f_%d.ppm" % i)), "rb").read()
            head = raw.split(b"\n", 3)
            assert head[0] == b"P6" and head[1].split() == [str(w).encode(), str(h).encode()]
            np.testing.assert_array_equal(np.frombuffer(head[3], dtype=np.uint8).reshape(h, w, 3), want["rgba8"][:, :, :3], err_msg="frame %d" % i)
        subprocess.check_call([tool, path, "--mode", "150", "--png", "--denoise", "--out", str(tmp_path / "d")] + size, timeout=120, stdout=subprocess.DEVNULL)
        assert open(str(tmp_path / "d_0.png"), "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    finally:
        _restore(r)
        scene.close()
