"""Shaded ray queries (crt_shade_rays*, include/crt_hip.h): colour, shading normal and albedo for caller-supplied rays, in the
context's shading mode.  A 1 x 1 oracle frame is one arbitrary ray with a bit-exact reference colour, so every colour check
here is exact (float bits compared as uint32); only the float64 normal reference has a tolerance."""
import os
import subprocess

import numpy as np
import pytest

from shaded_query_checks import bounds as _bounds, pose_rays as _pose_rays, pose_reference as _pose_reference, poses as _poses

SYMBOLS = ("crt_shade_rays_device", "crt_shade_rays")
MISS = 0xFFFFFFFF
EINVAL, ESTATE = 1, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (0, 1, 2, 3, 4, 5, 6, 42, 100)
MISS_RGB = (0.0, 1.0, 1.0)  # the default miss colour of the renderer and of OracleScene.render
TMIN, TMAX = 0.001, 10000.0
OUTPUTS = ("rgb", "normal", "albedo", "t", "uv", "inst", "prim")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- CPU: the interface exists

def test_binding_and_library_expose_shade_rays(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
    for name in ("shade_rays", "shade_rays_device"):
        assert callable(getattr(pkg.Renderer, name, None)), name
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    for s in SYMBOLS:
        assert ("int %s(" % s) in header, s
    assert L.crt_abi_version() == 1


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    rays = np.zeros((4, 8), dtype=np.float32)
    rgb = np.zeros((4, 3), dtype=np.float32)
    assert L.crt_shade_rays(None, 4, rays.ctypes.data, rgb.ctypes.data, None, None, None, None, None, None, None) == EINVAL
    assert L.crt_shade_rays_device(None, 4, rays.ctypes.data, rgb.ctypes.data, None, None, None, None, None, None, None) == EINVAL
    assert L.crt_shade_rays(None, 0, None, None, None, None, None, None, None, None, None) == EINVAL
    assert L.crt_shade_rays_device(None, 0, None, None, None, None, None, None, None, None, None) == EINVAL


# ---- scenes, poses and references (CPU)

SOUP_LIGHTS = [((9.0, 16.0, 6.0), 3000.0), ((-9.0, 12.0, -4.0), 2000.0), ((0.0, -3.0, 0.0), 800.0)]
N_POSES, POSE_SEED = 256, 20


def _soup(scenes, n_lights=3):
    sc = scenes.icosphere_soup(n_spheres=400)
    sc["lights"] = list(SOUP_LIGHTS[:n_lights])
    return sc


@pytest.fixture(scope="module")
def soup_ref(oracle, scenes):
    """The icosphere soup with three lights, 256 poses and their records, and the oracle's mode-100 references: over the SAH
    tree with 3 lights and with the first light alone, and over the LBVH with 3 lights.  Computed once, never modified."""
    sc = _soup(scenes)
    pos, rot = _poses(sc)
    rays = _pose_rays(oracle, pos, rot)
    ref = {(3, 0): _pose_reference(oracle, sc, pos, rot), (1, 0): _pose_reference(oracle, _soup(scenes, 1), pos, rot),
           (3, 1): _pose_reference(oracle, sc, pos, rot, build_mode=1)}
    for v in ref.values():
        for a in v.values():
            a.setflags(write=False)
    rays.setflags(write=False)
    return {"scene": sc, "pos": pos, "rot": rot, "rays": rays, "ref": ref}


def test_the_poses_cover_hits_misses_and_shadows(soup_ref):
    """the oracle alone: the 256 poses hold at least 64 hits, 64 misses and an occluded light (a hit whose single light was
    reached for by a shadow ray and added nothing)"""
    r3, r1 = soup_ref["ref"][(3, 0)], soup_ref["ref"][(1, 0)]
    hits = int((r3["inst"] != MISS).sum())
    assert hits >= 64 and N_POSES - hits >= 64, hits
    occluded = (r1["inst"] != MISS) & (r1["shadow"] == 1) & np.all(r1["rgb"] == 0.0, axis=1)
    assert occluded.sum() >= 1
    assert (r3["shadow"] > 0).sum() >= 32 and np.any(r3["rgb"][r3["inst"] != MISS] > 0.0)
    assert np.array_equal(_bits(r3["rgb"][r3["inst"] == MISS]), _bits(np.tile(np.float32(MISS_RGB), (N_POSES - hits, 1))))


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _upload(renderer, sc, dynamic=False):
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"), dynamic=dynamic)
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])


def _camera_rays(pkg, oracle, cam, w, h):
    d = np.zeros((h, w, 3), dtype=np.float32)
    for y in range(h):
        for x in range(w):
            d[y, x] = oracle.ray_dir(cam["matrix"], x, y, w, h)
    return pkg.make_rays(np.asarray(cam["position"], dtype=np.float32), d.reshape(-1, 3), tmin=TMIN, tmax=TMAX)


def _frame_equals_rays(renderer, O, sc, rays, w, h, mode, counting=False):
    cam = sc["camera"]
    renderer.change_shading_mode(mode)
    frame = renderer.render_frame(w, h)
    ref = O.render(cam["position"], cam["matrix"], mode, w, h)
    renderer.set_counting(counting)
    try:
        got = renderer.shade_rays(rays)
    finally:
        renderer.set_counting(False)
    what = "mode %d" % mode
    for src, name in ((frame, "frame"), (ref, "oracle")):
        assert np.array_equal(_bits(got["rgb"]), _bits(src["rgb"].reshape(-1, 3))), "%s: rgb differs from the %s" % (what, name)
        np.testing.assert_array_equal(got["inst"], src["hit_inst"].reshape(-1), err_msg=what)
        np.testing.assert_array_equal(got["prim"], src["hit_prim"].reshape(-1), err_msg=what)
        assert np.array_equal(_bits(got["t"]), _bits(src["hit_t"].reshape(-1))), what + ": t"
    assert got["stats"]["rays_primary"] == w * h and got["stats"]["kernel_ms"] > 0.0
    if counting:
        st, rs = got["stats"], ref["stats"]
        assert st["rays_shadow"] > 0
        assert (st["rays_shadow"], st["nodes_visited"], st["tris_tested"]) == (rs["rays_shadow"], rs["nodes_visited"], rs["tris_tested"]), what
    return got


def _textured_smooth_cornell(scenes, golden_dir):
    """the textured Cornell box with vertex normals and smooth materials, its bitmap the 7 x 5 image of tests/golden"""
    sc = scenes.textured_cornell(64, 48)
    raw = open(os.path.join(golden_dir, "tex7x5.ppm"), "rb").read()
    sc["textures"][2] = {"type": "bitmap", "pixels": np.frombuffer(raw[raw.index(b"255\n") + 4:], dtype=np.uint8).reshape(5, 7, 3).copy()}
    for m in sc["meshes"]:
        m["normals"] = scenes.vertex_normals(m["vertices"], m["triangles"]).astype(np.float32)
    for m in sc["materials"]:
        m["smooth_shading"] = True
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cornell", "dragon", "textured"])
def test_camera_rays_equal_the_frame(pkg, oracle, scenes, dragon, golden_dir, renderer, which):
    """A frame's camera rays handed over as records give the frame: rgb, t, inst and prim equal the frame kernel's and the
    oracle's bit for bit in every mode, with and without the Phong term, and the instrumented kernel counts the oracle frame's
    shadow rays and fetches."""
    sc, w, h = {"cornell": (scenes.cornell_box(), 64, 48), "dragon": (dragon, 96, 54),
                "textured": (_textured_smooth_cornell(scenes, golden_dir), 64, 48)}[which]
    _upload(renderer, sc)
    rays = _camera_rays(pkg, oracle, sc["camera"], w, h)
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], textures=sc.get("textures") or ())
    try:
        for mode in (100,) if which == "textured" else MODES:
            got = _frame_equals_rays(renderer, O, sc, rays, w, h, mode, counting=mode == 100)
        assert (got["inst"] != MISS).sum() > w * h // 10, "the camera sees the scene"
        if which == "textured":
            assert len(np.unique(got["albedo"], axis=0)) > 8, "the textures show"
        try:
            renderer.set_option("phong_ks", 300)
            oracle.set_phong(300, 32)
            phong = _frame_equals_rays(renderer, O, sc, rays, w, h, 100, counting=True)
        finally:
            renderer.set_option("phong_ks", 0)
            oracle.set_phong(0, 32)
        assert not np.array_equal(_bits(phong["rgb"]), _bits(got["rgb"])), "the specular term shows"
    finally:
        O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_build", [0, 1])
def test_arbitrary_rays_equal_the_oracle(soup_ref, renderer, gpu_build):
    """256 poses anywhere in and around the soup, three lights: each record's colour is the oracle's 1 x 1 frame at that pose,
    bit for bit, in either buffer order and over either tree"""
    sc, rays, ref = soup_ref["scene"], soup_ref["rays"], soup_ref["ref"][(3, gpu_build)]
    try:
        renderer.set_option("gpu_build", gpu_build)
        _upload(renderer, sc)
    finally:
        renderer.set_option("gpu_build", 0)
    renderer.change_shading_mode(100)
    for order in (np.arange(N_POSES), np.arange(N_POSES)[::-1]):
        got = renderer.shade_rays(np.ascontiguousarray(rays[order]))
        assert np.array_equal(_bits(got["rgb"]), _bits(ref["rgb"][order]))
        np.testing.assert_array_equal(got["inst"], ref["inst"][order])
        np.testing.assert_array_equal(got["prim"], ref["prim"][order])
        assert np.array_equal(_bits(got["t"]), _bits(ref["t"][order]))


@pytest.mark.gpu
@pytest.mark.parametrize("n_lights", [0, 1, 3])
def test_light_counts_and_partial_wavefronts(scenes, soup_ref, renderer, n_lights):
    """0, 1 and 3 lights on buffers of 1, 63, 65 and 1000 records (the poses, repeated): no light leaves black hits and the miss
    colour; otherwise the oracle's frames with those lights.  With counting, shadow rays and fetches are the oracle's sums."""
    _upload(renderer, _soup(scenes, n_lights))
    renderer.change_shading_mode(100)
    ref = soup_ref["ref"][(n_lights or 3, 0)]
    for n in (1, 63, 65, 1000):
        pick = np.arange(n) % N_POSES
        renderer.set_counting(True)
        try:
            got = renderer.shade_rays(np.ascontiguousarray(soup_ref["rays"][pick]))
        finally:
            renderer.set_counting(False)
        hit = ref["inst"][pick] != MISS
        np.testing.assert_array_equal(got["inst"], ref["inst"][pick])
        if n_lights == 0:
            assert np.all(got["rgb"][hit] == 0.0) and np.array_equal(_bits(got["rgb"][~hit]), _bits(np.tile(np.float32(MISS_RGB), ((~hit).sum(), 1))))
            assert got["stats"]["rays_shadow"] == 0
        else:
            assert np.array_equal(_bits(got["rgb"]), _bits(ref["rgb"][pick])), "%d lights, n = %d" % (n_lights, n)
            st = got["stats"]
            assert (st["rays_shadow"], st["nodes_visited"], st["tris_tested"]) == tuple(int(ref[k][pick].sum()) for k in ("shadow", "nodes", "tris"))
        assert got["stats"]["rays_primary"] == n


def _scaled(rays, k):
    out = rays.copy()
    out[:, 4:7] = np.ldexp(rays[:, 4:7], k)
    out[:, 3] = np.ldexp(rays[:, 3], -k)
    out[:, 7] = np.ldexp(rays[:, 7], -k)
    return out


@pytest.mark.gpu
def test_scale_and_degenerate_records(pkg, scenes, soup_ref, renderer):
    sc, rays = soup_ref["scene"], np.array(soup_ref["rays"])
    _upload(renderer, sc)
    miss = np.float32(MISS_RGB)
    for mode in (0, 1, 2, 3, 6, 5, 100):
        renderer.change_shading_mode(mode)
        base = renderer.shade_rays(rays)
        for k in (-20, 7, 60):
            got = renderer.shade_rays(_scaled(rays, k))
            for name in ("inst", "prim", "uv", "normal", "albedo"):
                assert np.array_equal(got[name].view(np.uint32), base[name].view(np.uint32)), "mode %d, 2^%d: %s" % (mode, k, name)
            assert np.array_equal(_bits(np.ldexp(got["t"], k)), _bits(base["t"])), "mode %d, 2^%d: t" % (mode, k)
            if mode in (0, 1, 2, 3, 6):
                assert np.array_equal(_bits(got["rgb"]), _bits(base["rgb"])), "mode %d, 2^%d: rgb" % (mode, k)
    assert (base["inst"] != MISS).sum() >= 64

    # records that are not traced: a NaN anywhere, an empty interval, a zero direction
    hitting = rays[np.flatnonzero(base["inst"] != MISS)[0]]
    bad = []
    for f in range(8):
        r = hitting.copy()
        r[f] = np.nan
        bad.append(r)
    for tmin, tmax in ((1.0, 1.0), (2.0, 1.0), (np.inf, np.inf)):
        r = hitting.copy()
        r[3], r[7] = tmin, tmax
        bad.append(r)
    r = hitting.copy()
    r[4:7] = 0.0
    bad.append(r)
    buf = np.stack(bad + [hitting]).astype(np.float32)
    nb = len(bad)
    for mode in (3, 100):
        renderer.change_shading_mode(mode)
        got = renderer.shade_rays(buf)
        assert np.all(got["inst"][:nb] == MISS) and np.all(got["prim"][:nb] == MISS) and np.all(got["uv"][:nb] == 0.0)
        assert np.array_equal(_bits(got["rgb"][:nb]), _bits(np.tile(miss, (nb, 1))))
        assert np.all(got["normal"][:nb] == 0.0) and np.all(got["albedo"][:nb] == 0.0)
        assert np.array_equal(_bits(got["t"][:nb]), _bits(buf[:nb, 7]))
        assert got["inst"][nb] != MISS, "the control record hits"

    # n = 0: OK, nothing launched, NULL buffers allowed
    e = renderer.shade_rays(np.zeros((0, 8), dtype=np.float32))
    assert all(len(e[k]) == 0 for k in OUTPUTS) and e["stats"]["rays_primary"] == 0
    assert pkg.lib().crt_shade_rays_device(renderer.h, 0, None, None, None, None, None, None, None, None, None) == 0

    # an empty scene: every record misses
    renderer.upload([], [], [])
    renderer.change_shading_mode(100)
    e = renderer.shade_rays(rays)
    assert np.all(e["inst"] == MISS) and np.array_equal(_bits(e["rgb"]), _bits(np.tile(miss, (len(rays), 1))))
    assert np.all(e["normal"] == 0.0) and np.all(e["albedo"] == 0.0) and np.array_equal(_bits(e["t"]), _bits(rays[:, 7]))


def _aimed_rays(pkg, sc, n, seed):
    """n seeded rays from in and around the scene's box towards points inside random triangles, directions not normalised"""
    rng = np.random.default_rng(seed)
    lo, hi = _bounds(sc)
    ext = hi - lo
    V = [np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3)[np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)] for m in sc["meshes"]]
    V = np.concatenate(V)
    tri = rng.integers(0, len(V), size=n)
    b = (0.05 + 0.85 * rng.dirichlet((1.0, 1.0, 1.0), size=n)).astype(np.float32)
    target = V[tri, 0] * b[:, 0:1] + V[tri, 1] * b[:, 1:2] + V[tri, 2] * b[:, 2:3]
    o = (lo - 0.1 * ext + rng.random((n, 3)) * 1.2 * ext).astype(np.float32)
    d = (target - o) * rng.uniform(0.2, 5.0, size=(n, 1))
    return pkg.make_rays(o, d.astype(np.float32), tmin=0.001, tmax=np.inf)


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [False, True])
def test_attributes(pkg, scenes, renderer, smooth):
    """t / uv / inst / prim are crt_trace_rays' bit for bit; the normal is unit, faces the ray and is within 1e-5 per component
    (a dozen float32 roundings of a unit vector are about 1e-6; a wrong triangle or a missed flip is off by 0.1 or more) of a
    float64 reference: the cross product of the edges, or the blend of the vertex normals of a smooth material; the albedo is
    the material's colour, or color_a of an albedo texture, exactly."""
    sc = _soup(scenes)
    sc["textures"] = [{"type": "albedo", "color_a": (0.3, 0.8, 0.4)}]
    sc["materials"][0]["texture"] = 0  # the ground
    if smooth:
        m = sc["meshes"][1]
        m["normals"] = scenes.vertex_normals(m["vertices"], m["triangles"]).astype(np.float32)
        sc["materials"][1]["smooth_shading"] = True
    _upload(renderer, sc)
    rays = _aimed_rays(pkg, sc, 3000, seed=77)
    renderer.change_shading_mode(3)  # a debug mode: the surface is evaluated for the two outputs alone
    got = renderer.shade_rays(rays)
    hit = renderer.trace_rays(rays)
    for k in ("t", "uv", "inst", "prim"):
        assert np.array_equal(got[k].view(np.uint32), hit[k].view(np.uint32)), k
    renderer.change_shading_mode(100)
    lit = renderer.shade_rays(rays, want=("normal", "albedo", "inst"))
    assert np.array_equal(_bits(lit["normal"]), _bits(got["normal"])) and np.array_equal(_bits(lit["albedo"]), _bits(got["albedo"]))
    h = got["inst"] != MISS
    assert h.sum() > 2000 and (got["inst"][h] == 0).sum() > 20 and (got["inst"][h] == 1).sum() > 1000
    assert np.all(got["normal"][~h] == 0.0) and np.all(got["albedo"][~h] == 0.0)
    N = got["normal"][h].astype(np.float64)
    d = rays[h, 4:7].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(N, axis=1) - 1.0) <= 2.0 ** -20)
    assert np.all(got["normal"][h, 0] * rays[h, 4] + got["normal"][h, 1] * rays[h, 5] + got["normal"][h, 2] * rays[h, 6] <= 0.0)
    ref = np.zeros_like(N)
    inst, prim, uv = got["inst"][h], got["prim"][h], got["uv"][h].astype(np.float64)
    for i in (0, 1):
        sel = inst == i
        m = sc["meshes"][i]
        v = np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3).astype(np.float64)
        t = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)[prim[sel]]
        n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
        if smooth and i == 1:
            vn = np.asarray(m["normals"], dtype=np.float32).astype(np.float64)
            u, w = uv[sel, 0:1], uv[sel, 1:2]
            n = vn[t[:, 0]] * (1.0 - u - w) + vn[t[:, 1]] * u + vn[t[:, 2]] * w
        ref[sel] = n / np.linalg.norm(n, axis=1, keepdims=True)
    ref[np.einsum("ij,ij->i", ref, d) > 0.0] *= -1.0
    assert np.abs(N - ref).max() <= 1e-5, np.abs(N - ref).max()
    albedo = np.float32([(0.3, 0.8, 0.4), sc["materials"][1]["albedo"]])
    assert np.array_equal(_bits(got["albedo"][h]), _bits(albedo[inst]))


@pytest.mark.gpu
def test_options_change_nothing(soup_ref, renderer):
    """other scheduling thresholds and a four-entry LDS stack (deeper entries go to the spill arena): every output, the shadow
    rays and both fetch counts are those of the default options"""
    _upload(renderer, soup_ref["scene"])
    renderer.change_shading_mode(100)
    rays = np.ascontiguousarray(soup_ref["rays"][np.arange(1000) % N_POSES])
    defaults = (("inner_min", -6), ("inner_min_any", -6), ("stack_entries", 0))
    counters = ("rays_shadow", "nodes_visited", "tris_tested")
    renderer.set_counting(True)
    try:
        base = renderer.shade_rays(rays)
        assert all(base["stats"][k] > 0 for k in counters)
        for name, value in (("inner_min", 3), ("inner_min_any", 40), ("inner_min_any", -2), ("stack_entries", 4)):
            renderer.set_option(name, value)
            got = renderer.shade_rays(rays)
            for k, v in defaults:
                renderer.set_option(k, v)
            for k in OUTPUTS:
                assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), "%s=%d: %s" % (name, value, k)
            for k in counters:
                assert got["stats"][k] == base["stats"][k], "%s=%d: %s" % (name, value, k)
    finally:
        for k, v in defaults:
            renderer.set_option(k, v)
        renderer.set_counting(False)


@pytest.mark.gpu
def test_no_interference_with_frames(pkg, oracle, scenes, renderer):
    """Shade queries leave every frame as it would be without them: a mode-100 frame; an accumulating mode-200 run with a
    shade query (issued in mode 100) between its frames; and after update_vertices without a refit the query sees the moved
    mesh, as the next frame does."""
    sc, w, h, S, K = scenes.cornell_box(), 64, 48, 2, 3
    _upload(renderer, sc, dynamic=True)
    rays = _camera_rays(pkg, oracle, sc["camera"], w, h)
    renderer.change_shading_mode(100)
    before = renderer.render_frame(w, h)
    for _ in range(3):
        renderer.shade_rays(rays)
    after = renderer.render_frame(w, h)
    for k in ("rgba8", "hit_inst", "hit_prim", "hit_t"):
        np.testing.assert_array_equal(before[k], after[k], err_msg="mode 100 " + k)
    assert np.array_equal(_bits(before["rgb"]), _bits(after["rgb"]))

    renderer.set_miss_color((0.0, 0.0, 0.0))
    try:
        runs = []
        for query in (False, True):
            renderer.change_shading_mode(200)
            renderer.set_path_params(S, 3, 1234)
            renderer.set_accumulation(1 << 24)
            for i in range(K):
                frame = renderer.render_frame(w, h)
                if query:
                    renderer.change_shading_mode(100)
                    renderer.shade_rays(rays)
                    renderer.change_shading_mode(200)
                assert renderer.accumulated_samples() == (i + 1) * S
            runs.append(frame)
            renderer.set_accumulation(0)
        np.testing.assert_array_equal(runs[0]["rgba8"], runs[1]["rgba8"])
        assert np.array_equal(_bits(runs[0]["rgb"]), _bits(runs[1]["rgb"]))
    finally:
        renderer.set_accumulation(0)
        renderer.set_path_params(4, 3, 1234)
        renderer.set_miss_color(MISS_RGB)

    # dynamic scene: the pending update is applied by the query itself
    renderer.change_shading_mode(100)
    v = np.asarray(sc["meshes"][4]["vertices"], dtype=np.float32).reshape(-1, 3) + np.float32([0.7, 0.0, 0.9])
    renderer.update_vertices(4, v)
    got = renderer.shade_rays(rays)
    frame = renderer.render_frame(w, h)
    assert np.array_equal(_bits(got["rgb"]), _bits(frame["rgb"].reshape(-1, 3)))
    np.testing.assert_array_equal(got["prim"], frame["hit_prim"].reshape(-1))
    assert not np.array_equal(_bits(frame["rgb"]), _bits(before["rgb"])), "the mesh moved"


@pytest.mark.gpu
def test_errors(pkg, scenes, soup_ref, renderer):
    import torch
    L = pkg.lib()
    _upload(renderer, soup_ref["scene"])
    rays = np.array(soup_ref["rays"])
    n = len(rays)
    d_rays = torch.from_numpy(np.concatenate([rays.reshape(-1), np.zeros(8, np.float32)])).cuda()
    sentinel = 12345.0
    d_out = torch.full((3 * n + 8,), sentinel, dtype=torch.float32, device="cuda")
    rgb = np.full((n, 3), sentinel, dtype=np.float32)

    def untouched():
        torch.cuda.synchronize()
        return bool((d_out == sentinel).all().item()) and bool(np.all(rgb == sentinel))
    P, R = d_out.data_ptr(), d_rays.data_ptr()
    renderer.change_shading_mode(200)
    assert L.crt_shade_rays_device(renderer.h, n, R, P, None, None, None, None, None, None, None) == EINVAL
    assert L.crt_shade_rays(renderer.h, n, rays.ctypes.data, rgb.ctypes.data, None, None, None, None, None, None, None) == EINVAL
    assert "200" in L.crt_last_error(renderer.h).decode()
    with pytest.raises(pkg.CrtError):
        renderer.shade_rays(rays)
    assert untouched()
    renderer.change_shading_mode(100)
    assert L.crt_shade_rays_device(renderer.h, n, R, None, None, None, None, None, None, None, None) == EINVAL
    assert L.crt_shade_rays(renderer.h, n, rays.ctypes.data, None, None, None, None, None, None, None, None) == EINVAL
    assert L.crt_shade_rays_device(renderer.h, n, None, P, None, None, None, None, None, None, None) == EINVAL
    assert L.crt_shade_rays(renderer.h, n, None, rgb.ctypes.data, None, None, None, None, None, None, None) == EINVAL
    assert L.crt_shade_rays_device(renderer.h, n, R + 4, P, None, None, None, None, None, None, None) == EINVAL   # rays: 16 bytes
    assert L.crt_shade_rays_device(renderer.h, n, R + 8, P, None, None, None, None, None, None, None) == EINVAL
    for slot in range(7):  # rgb, normal, albedo, t, inst, prim: 4 bytes; uv: 8
        args = [None] * 7
        args[slot] = P + 2
        assert L.crt_shade_rays_device(renderer.h, n, R, *args, None) == EINVAL, slot
    assert L.crt_shade_rays_device(renderer.h, n, R, P, None, None, None, P + 4, None, None, None) == EINVAL      # uv
    assert "aligned" in L.crt_last_error(renderer.h).decode()
    assert untouched()
    # the control: the same buffers, properly aligned, are written
    renderer.shade_rays_device(n, R, d_rgb=P)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_out[:3 * n].cpu().numpy().reshape(n, 3)), _bits(soup_ref["ref"][(3, 0)]["rgb"]))
    assert bool((d_out[3 * n:] == sentinel).all().item())

    fresh = pkg.Renderer(0)
    try:
        assert L.crt_shade_rays(fresh.h, n, rays.ctypes.data, rgb.ctypes.data, None, None, None, None, None, None, None) == ESTATE
        assert L.crt_shade_rays_device(fresh.h, n, R, P, None, None, None, None, None, None, None) == ESTATE
        with pytest.raises(pkg.CrtError):
            fresh.shade_rays(rays)
    finally:
        fresh.close()
    assert np.all(rgb == sentinel)


@pytest.mark.gpu
def test_cpp_layer(pkg, scenes, renderer, tmp_path):
    """crt::Renderer::shadeRays, from a small C++ program linked against libcrt_hip.so, agrees with the Python host path."""
    exe = str(tmp_path / "shade_rays_cpp")
    csrc = os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + csrc,
                           "-o", exe, os.path.join(ROOT, "tests", "shade_rays_cpp.cpp"), "-L" + os.path.dirname(pkg.LIB_PATH), "-lcrt_hip",
                           "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH), "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    sc = scenes.cornell_box()
    scene = pkg.Scene.from_arrays(sc)
    path = str(tmp_path / "cornell.crtbin")
    scene.save(path)
    rays = _aimed_rays(pkg, sc, 2048, seed=31)
    rays.tofile(str(tmp_path / "rays.bin"))
    out = str(tmp_path / "shaded.bin")
    subprocess.check_call([exe, path, str(tmp_path / "rays.bin"), "100", out], timeout=120)
    raw = np.fromfile(out, dtype=np.uint32).reshape(len(rays), 14)
    renderer.upload_scene(scene)
    renderer.change_shading_mode(100)
    ref = renderer.shade_rays(rays)
    for k, cols in (("rgb", slice(0, 3)), ("normal", slice(3, 6)), ("albedo", slice(6, 9)), ("uv", slice(10, 12))):
        assert np.array_equal(raw[:, cols], _bits(ref[k])), k
    assert np.array_equal(raw[:, 9], _bits(ref["t"])) and np.array_equal(raw[:, 12], ref["inst"]) and np.array_equal(raw[:, 13], ref["prim"])
    assert (ref["inst"] != MISS).sum() > 500 and np.any(ref["rgb"][ref["inst"] != MISS] > 0.0)
    scene.close()
