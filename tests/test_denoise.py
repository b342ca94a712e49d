"""Camera rays, frame guide buffers and the edge-avoiding a-trous denoiser (crt_camera_rays*, crt_frame_guides*, crt_denoise*,
include/crt_hip.h).  The denoiser is checked against the float64 numpy reference of tests/denoise_reference.py with a
tolerance computed at run time: 16 x the deviation of the reference's own float32 run on the same input (the factor allows for
a device exponential and hoisted reciprocals a few ulp from correctly rounded, compounded over at most 8 passes).  Camera rays
and guides are compared bit for bit with the frames and with crt_shade_rays / crt_path_rays.

Observed on the MI355X: see DESIGN.md section 5g."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("crt_camera_rays_device", "crt_camera_rays", "crt_frame_guides_device", "crt_frame_guides", "crt_denoise_device", "crt_denoise")
EINVAL, ESTATE = 1, 5
GUIDES = ("rgb", "normal", "albedo", "t")
TOL_FACTOR, TOL_CAP = 16.0, 1e-4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _inputs(w, h):
    """the synthetic image of that size; at 37 x 23 (edge at column 20) with a NaN colour, an infinite colour and a NaN normal"""
    s = R.synthetic(w, h, edge=20 if (w, h) == (37, 23) else None)
    if (w, h) == (37, 23):
        s["rgb"][10, 12, 1] = np.nan
        s["rgb"][15, 30, 0] = np.inf
        s["normal"][18, 8, 2] = np.nan
    for k in GUIDES:
        s[k].setflags(write=False)
    return s


def _tolerance(k, ref64, **prm):
    """16 x the float32 reference's deviation from the float64 one over the live pixels; the condition tol < 1e-4 is part of it"""
    live = R.live_mask(k["rgb"], k["normal"], k["albedo"], k["t"])
    ref32 = R.denoise(k["rgb"], k["normal"], k["albedo"], k["t"], dtype=np.float32, **prm)
    dev32 = float(R.deviation(ref32, ref64)[live].max()) if live.any() else 0.0
    tol = TOL_FACTOR * dev32
    assert tol < TOL_CAP, tol
    return tol, live


# ---- CPU: the interface exists; the reference is pinned

def test_binding_and_library_expose_the_new_entry_points(pkg):
    L = pkg.lib()
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
        assert ("int %s(" % s) in header, s
    for name in ("camera_rays", "camera_rays_device", "frame_guides", "frame_guides_device", "denoise", "denoise_device"):
        assert callable(getattr(pkg.Renderer, name, None)), name
    assert ctypes.sizeof(pkg.DenoiseParams) == 20
    d = pkg.DenoiseParams()
    assert (d.iterations, d.demodulate) == (5, 1) and np.float32(d.sigma_color) == np.float32(4.0)
    assert np.float32(d.sigma_normal) == np.float32(0.3) and np.float32(d.sigma_depth) == np.float32(0.05)
    buf = np.zeros(64, dtype=np.float32)
    P = buf.ctypes.data
    assert L.crt_camera_rays(None, 2, 2, pkg.SAMPLE_CENTRE, P, None) == EINVAL
    assert L.crt_camera_rays_device(None, 2, 2, pkg.SAMPLE_CENTRE, P, None) == EINVAL
    assert L.crt_frame_guides(None, 2, 2, P, None, None, None) == EINVAL
    assert L.crt_frame_guides_device(None, 2, 2, P, None, None, None) == EINVAL
    assert L.crt_denoise(None, 2, 2, P, P, P, P, P, None, None) == EINVAL
    assert L.crt_denoise_device(None, 2, 2, P, P, P, P, P, None, None) == EINVAL
    assert not buf.any()


def test_reference_self_checks():
    """the yardstick itself, on the 37 x 23 synthetic input with the defaults: it denoises, it keeps the edge, it bleeds when
    the guides are switched off, it leaves the miss block alone, and its float32 run stays within 2e-6"""
    s = R.synthetic(37, 23, edge=20)
    k = {g: s[g] for g in GUIDES}
    live, right = ~s["miss"], s["right"] & ~s["miss"]
    ref = R.denoise(**k)

    def rmse(a):
        return float(np.sqrt((((a - s["clean"])[live]) ** 2).mean()))

    def irradiance_right(a):
        return float((a / np.maximum(s["albedo"], 1e-3)).mean(axis=2)[right].mean())
    assert rmse(ref) <= 0.25 * rmse(s["rgb"]), (rmse(ref), rmse(s["rgb"]))  # prototype: 0.13
    assert irradiance_right(ref) < 0.45                                      # prototype: 0.37
    bleed = R.denoise(**k, sigma_normal=1e6, sigma_depth=1e6, sigma_color=16.0)
    assert irradiance_right(bleed) > 0.55                                    # prototype: 0.61
    ref32 = R.denoise(**k, dtype=np.float32)
    assert ref32.dtype == np.float32 and np.array_equal(_bits(ref32[s["miss"]]), _bits(s["rgb"][s["miss"]]))
    assert np.array_equal(ref[s["miss"]], s["rgb"][s["miss"]].astype(np.float64))
    assert float(R.deviation(ref32, ref)[live].max()) <= 2e-6


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _upload(renderer, sc):
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"))
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])


def _device(torch, a):
    """a copy of `a` in device memory (the array itself may be read-only)"""
    return torch.from_numpy(np.array(a)).cuda()


def _ready(torch):
    """torch fills its tensors on its own stream: they are complete before the renderer's stream touches them"""
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(37, 23), (1, 1), (1, 70), (130, 5), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_denoiser_equals_the_reference(pkg, renderer, size):
    """Device output within tol of the float64 reference for iterations 1, 5, 8 with and without demodulation; pixels that are
    not live bit-equal to their input; host form, in-place form and a second call give the device form's bits."""
    import torch
    w, h = size
    s = _inputs(w, h)
    k = {g: s[g] for g in GUIDES}
    d = {g: _device(torch, s[g]) for g in GUIDES}
    worst = 0.0
    for iterations in (1, 5, 8):
        for demodulate in (0, 1):
            prm = {"iterations": iterations, "demodulate": demodulate}
            ref = R.denoise(**k, **prm)
            tol, live = _tolerance(k, ref, **prm)
            d_out = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
            _ready(torch)
            renderer.denoise_device(w, h, d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(), d_out.data_ptr(), **prm)
            renderer.synchronize()
            got = d_out.cpu().numpy()
            what = "%dx%d iterations %d demodulate %d" % (w, h, iterations, demodulate)
            dev = float(R.deviation(got, ref)[live].max()) if live.any() else 0.0
            worst = max(worst, dev)
            print("%s: device deviation %.3g, tol %.3g" % (what, dev, tol))
            assert np.isfinite(got[live]).all(), what
            assert dev <= tol, (what, dev, tol)
            assert np.array_equal(_bits(got[~live]), _bits(s["rgb"][~live])), what + ": a pixel that is not live changed"
            host = renderer.denoise(s["rgb"], s["normal"], s["albedo"], s["t"], **prm)
            assert np.array_equal(_bits(host), _bits(got)), what + ": host form"
            d_in_place = d["rgb"].clone()
            P = d_in_place.data_ptr()
            _ready(torch)
            renderer.denoise_device(w, h, P, d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(), P, **prm)
            renderer.denoise_device(w, h, d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(), d_out.data_ptr(), **prm)
            renderer.synchronize()
            assert np.array_equal(_bits(d_in_place.cpu().numpy()), _bits(got)), what + ": in place"
            assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(got)), what + ": second call"
    if (w, h) == (37, 23):
        assert (~live).sum() == 6 + 3, "the miss block and the three poisoned pixels"
    print("%dx%d: worst device deviation %.3g" % (w, h, worst))


@pytest.fixture(scope="module")
def cornell(scenes):
    sc = scenes.cornell_box()
    sc["camera"]["matrix"] = scenes.camera_matrix(20, -10)
    return sc


@pytest.mark.gpu
def test_camera_rays_are_the_frames_rays(pkg, renderer, cornell):
    """The CRT_SAMPLE_CENTRE records through crt_shade_rays give the frame's rgb and hit_t bit for bit in modes 3 and 100; the
    records of samples 0..5 through six chained crt_path_rays calls give the 6-spp mode-200 frame's rgb bit for bit; the
    host form equals the device form."""
    import torch
    w, h, spp = 67, 41, 6
    _upload(renderer, cornell)
    rays = renderer.camera_rays(w, h)
    assert rays.shape == (w * h, 8)
    assert np.array_equal(_bits(rays[:, 0:3]), _bits(np.tile(np.float32(cornell["camera"]["position"]), (w * h, 1))))
    assert np.all(rays[:, 3] == np.float32(0.001)) and np.all(rays[:, 7] == np.float32(10000.0))
    for mode in (3, 100):
        renderer.change_shading_mode(mode)
        frame = renderer.render_frame(w, h)
        got = renderer.shade_rays(rays, want=("rgb", "t"))
        assert np.array_equal(_bits(got["rgb"]), _bits(frame["rgb"].reshape(-1, 3))), "mode %d rgb" % mode
        assert np.array_equal(_bits(got["t"]), _bits(frame["hit_t"].reshape(-1))), "mode %d t" % mode
    assert (frame["hit_inst"] != pkg.MISS).sum() > w * h // 10, "the camera sees the box"

    try:
        renderer.change_shading_mode(200)
        renderer.set_path_params(spp, 3, 4321)
        frame = renderer.render_frame(w, h)
        sums = np.zeros((w * h, 3), dtype=np.float64)
        jx, jy = pkg.path_jitter(np.arange(w * h), 2, 4321)
        for k in range(spp):
            recs = renderer.camera_rays(w, h, sample=k)
            got = renderer.path_rays(recs, first_sample=k, n_samples=1, sums=sums, want=("rgb",))
            if k == 2:
                assert not np.array_equal(_bits(recs[:, 4:7]), _bits(rays[:, 4:7])), "the jitter shows"
                assert jx.min() >= 0.0 and jx.max() < 1.0 and jy.max() < 1.0
        assert np.array_equal(_bits(got["rgb"]), _bits(frame["rgb"].reshape(-1, 3))), "mode 200"
        assert renderer.render_frame(w, h)["stats"]["kernel_ms"] > 0.0

        d_rays = torch.zeros(w * h * 8 + 8, dtype=torch.float32, device="cuda")
        for sample in (None, 3):
            d_rays.fill_(-1.0)
            _ready(torch)
            st = renderer.camera_rays_device(w, h, d_rays.data_ptr(), sample=sample, stats=True)
            assert st["kernel_ms"] > 0.0 and st["rays_primary"] == w * h
            back = d_rays.cpu().numpy()
            assert np.array_equal(_bits(back[:w * h * 8].reshape(-1, 8)), _bits(renderer.camera_rays(w, h, sample=sample)))
            assert np.all(back[w * h * 8:] == -1.0), "nothing is written behind the records"
    finally:
        renderer.set_path_params(4, 3, 1234)
        renderer.change_shading_mode(0)


@pytest.mark.gpu
def test_frame_guides(pkg, renderer, cornell):
    """Guides = normal, albedo and t of crt_shade_rays on the pixel-centre records, bit for bit, in mode 3 and in mode 200
    with accumulation on; an accumulating run does not notice the call; each output is optional."""
    import torch
    L = pkg.lib()
    w, h = 67, 41
    _upload(renderer, cornell)
    renderer.change_shading_mode(3)
    ref = renderer.shade_rays(renderer.camera_rays(w, h), want=("normal", "albedo", "t"))
    g3 = renderer.frame_guides(w, h)
    for k in ("normal", "albedo", "t"):
        assert np.array_equal(_bits(g3[k]).reshape(-1), _bits(ref[k]).reshape(-1)), k
    miss = ref["t"] == np.float32(10000.0)
    assert not ref["normal"][miss].any() and not ref["albedo"][miss].any()
    assert (~miss).sum() > w * h // 10 and len(np.unique(ref["albedo"][~miss], axis=0)) >= 3
    assert g3["stats"]["kernel_ms"] > 0.0 and g3["stats"]["rays_primary"] == w * h
    try:
        runs = []
        for call in (False, True):
            renderer.change_shading_mode(200)
            renderer.set_path_params(2, 3, 1234)
            renderer.set_accumulation(1 << 24)
            renderer.render_frame(w, h)
            if call:
                g200 = renderer.frame_guides(w, h)
                for k in ("normal", "albedo", "t"):
                    assert np.array_equal(_bits(g200[k]), _bits(g3[k])), "mode 200 " + k
            assert renderer.accumulated_samples() == 2
            runs.append(renderer.render_frame(w, h))
            assert renderer.accumulated_samples() == 4
            renderer.set_accumulation(0)
        np.testing.assert_array_equal(runs[0]["rgba8"], runs[1]["rgba8"])
        assert np.array_equal(_bits(runs[0]["rgb"]), _bits(runs[1]["rgb"]))
    finally:
        renderer.set_accumulation(0)
        renderer.set_path_params(4, 3, 1234)
        renderer.change_shading_mode(0)

    # each output alone; the device form; all three NULL
    for k in ("normal", "albedo", "t"):
        one = renderer.frame_guides(w, h, want=(k,))
        assert set(one) == {k, "stats"} and np.array_equal(_bits(one[k]), _bits(g3[k])), k
    d_n = torch.full((w * h * 3 + 4,), -1.0, dtype=torch.float32, device="cuda")
    d_t = torch.full((w * h + 4,), -1.0, dtype=torch.float32, device="cuda")
    _ready(torch)
    renderer.frame_guides_device(w, h, d_normal=d_n.data_ptr(), d_t=d_t.data_ptr())
    renderer.synchronize()
    assert np.array_equal(_bits(d_n.cpu().numpy()[:w * h * 3]), _bits(g3["normal"]).reshape(-1))
    assert np.array_equal(_bits(d_t.cpu().numpy()[:w * h]), _bits(g3["t"]).reshape(-1))
    assert bool((d_n[w * h * 3:] == -1.0).all().item()) and bool((d_t[w * h:] == -1.0).all().item())
    assert L.crt_frame_guides(renderer.h, w, h, None, None, None, None) == EINVAL
    assert L.crt_frame_guides_device(renderer.h, w, h, None, None, None, None) == EINVAL
    assert "NULL" in L.crt_last_error(renderer.h).decode()


@pytest.mark.gpu
def test_pipeline_denoises_a_path_traced_frame(pkg, scenes, renderer):
    """Cornell box 48 x 48, identity camera, 3 bounces, seed 1234: the 4-spp frame denoised with its guides and the defaults is
    within tol of the reference run on the same buffers and closer to the 1024-spp frame than the 4-spp frame is (RMSE below
    0.9 x; the reference gives 0.79 on the CPU oracle's frames with geometric normals)."""
    w = h = 48
    sc = scenes.cornell_box()
    _upload(renderer, sc)
    try:
        renderer.change_shading_mode(200)
        renderer.set_path_params(4, 3, 1234)
        noisy = renderer.render_frame(w, h, want=("rgba8", "rgb"))["rgb"]
        g = renderer.frame_guides(w, h)
        out = renderer.denoise(noisy, g["normal"], g["albedo"], g["t"])
        renderer.set_path_params(1024, 3, 1234)
        clean = renderer.render_frame(w, h, want=("rgba8", "rgb"))["rgb"]
    finally:
        renderer.set_path_params(4, 3, 1234)
        renderer.change_shading_mode(0)
    k = {"rgb": noisy, "normal": g["normal"], "albedo": g["albedo"], "t": g["t"]}
    ref = R.denoise(**k)
    tol, live = _tolerance(k, ref)
    dev = float(R.deviation(out, ref)[live].max())
    print("pipeline: device deviation %.3g, tol %.3g" % (dev, tol))
    assert live.sum() > w * h // 10
    assert dev <= tol, (dev, tol)
    assert np.array_equal(_bits(out[~live]), _bits(noisy[~live]))

    def rmse(a):
        return float(np.sqrt(((a.astype(np.float64) - clean) ** 2).mean()))
    print("pipeline: RMSE against 1024 spp: 4 spp %.4f, denoised %.4f, ratio %.3f" % (rmse(noisy), rmse(out), rmse(out) / rmse(noisy)))
    assert rmse(out) < 0.9 * rmse(noisy), (rmse(out), rmse(noisy))


@pytest.mark.gpu
def test_errors(pkg, renderer, cornell):
    """every failed call launches nothing and leaves out untouched"""
    import torch
    L = pkg.lib()
    w, h = 16, 8
    s = R.synthetic(w, h)
    d = {g: _device(torch, s[g]) for g in GUIDES}
    sentinel = -5.0
    d_out = torch.full((w * h * 3 + 4,), sentinel, dtype=torch.float32, device="cuda")
    out = np.full((h, w, 3), sentinel, dtype=np.float32)
    P = {g: d[g].data_ptr() for g in GUIDES}
    H = {g: s[g].ctypes.data for g in GUIDES}
    _ready(torch)

    def dev(prm=None, w_=w, **over):
        a = dict(P, out=d_out.data_ptr())
        a.update(over)
        return L.crt_denoise_device(renderer.h, w_, h, a["rgb"], a["normal"], a["albedo"], a["t"], a["out"], ctypes.byref(prm) if prm else None, None)

    def host(prm=None, w_=w, **over):
        a = dict(H, out=out.ctypes.data)
        a.update(over)
        return L.crt_denoise(renderer.h, w_, h, a["rgb"], a["normal"], a["albedo"], a["t"], a["out"], ctypes.byref(prm) if prm else None, None)

    def untouched():
        torch.cuda.synchronize()
        return bool((d_out == sentinel).all().item()) and bool(np.all(out == sentinel))
    bad = [pkg.DenoiseParams(iterations=0), pkg.DenoiseParams(iterations=9), pkg.DenoiseParams(demodulate=2)]
    for name in ("sigma_color", "sigma_normal", "sigma_depth"):
        bad += [pkg.DenoiseParams(**{name: v}) for v in (0.0, -1.0, float("nan"))]
    for prm in bad:
        assert dev(prm) == EINVAL and host(prm) == EINVAL
    assert dev(w_=0) == EINVAL and host(w_=0) == EINVAL
    for g in GUIDES + ("out",):
        assert dev(**{g: None}) == EINVAL and host(**{g: None}) == EINVAL, g
        assert dev(**{g: (d_out.data_ptr() if g == "out" else P[g]) + 2}) == EINVAL, g
    assert "aligned" in L.crt_last_error(renderer.h).decode()
    assert L.crt_denoise_device(renderer.h, 1 << 15, 1 << 14, P["rgb"], P["normal"], P["albedo"], P["t"], d_out.data_ptr(), None, None) == EINVAL
    assert untouched()
    # camera rays
    d_rays = torch.full((w * h * 8 + 8,), sentinel, dtype=torch.float32, device="cuda")
    rays = np.full((w * h, 8), sentinel, dtype=np.float32)
    _ready(torch)
    for sample in (1 << 24, 0xFFFFFFFE):
        assert L.crt_camera_rays_device(renderer.h, w, h, sample, d_rays.data_ptr(), None) == EINVAL
        assert L.crt_camera_rays(renderer.h, w, h, sample, rays.ctypes.data, None) == EINVAL
    assert L.crt_camera_rays_device(renderer.h, w, h, 0, d_rays.data_ptr() + 8, None) == EINVAL
    assert L.crt_camera_rays_device(renderer.h, w, h, 0, None, None) == EINVAL and L.crt_camera_rays(renderer.h, w, h, 0, None, None) == EINVAL
    assert L.crt_camera_rays_device(renderer.h, 0, h, 0, d_rays.data_ptr(), None) == EINVAL
    assert L.crt_camera_rays(renderer.h, w, 0, 0, rays.ctypes.data, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((d_rays == sentinel).all().item()) and np.all(rays == sentinel)
    # the controls: the same buffers, properly used, are written
    assert dev(pkg.DenoiseParams(sigma_color=float("inf"))) == 0 and host() == 0
    assert L.crt_camera_rays_device(renderer.h, w, h, (1 << 24) - 1, d_rays.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert not bool((d_out[:w * h * 3] == sentinel).any().item()) and bool((d_out[w * h * 3:] == sentinel).all().item())
    assert not np.any(out == sentinel)
    assert not bool((d_rays[:w * h * 8] == sentinel).any().item()) and bool((d_rays[w * h * 8:] == sentinel).all().item())
    # guides: no scene; the denoiser and the camera rays need none
    fresh = pkg.Renderer(0)
    try:
        assert L.crt_frame_guides(fresh.h, w, h, out.ctypes.data, None, None, None) == ESTATE
        assert L.crt_frame_guides_device(fresh.h, w, h, d_out.data_ptr(), None, None, None) == ESTATE
        with pytest.raises(pkg.CrtError):
            fresh.frame_guides(w, h)
        assert fresh.camera_rays(w, h).shape == (w * h, 8)
        got = fresh.denoise(s["rgb"], s["normal"], s["albedo"], s["t"])
        assert np.array_equal(_bits(got), _bits(out))
    finally:
        fresh.close()


def _read_ppm(path):
    raw = open(path, "rb").read()
    head = raw.split(b"\n", 3)
    assert head[0] == b"P6" and head[2] == b"255"
    w, h = (int(x) for x in head[1].split())
    return np.frombuffer(head[3], dtype=np.uint8).reshape(h, w, 3)


@pytest.mark.gpu
def test_cpp_layer(pkg, scenes, renderer, tmp_path):
    """crt::Renderer::cameraRays, frameGuides and denoise, from a small C++ program linked against libcrt_hip.so, give the bits
    of the C ABI; crt_render --denoise writes another image than crt_render, whose own image is the frame's RGBA8."""
    exe = str(tmp_path / "denoise_cpp")
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    csrc = os.path.join(lib_dir, "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + csrc,
                           "-o", exe, os.path.join(ROOT, "tests", "denoise_cpp.cpp"), "-L" + lib_dir, "-lcrt_hip",
                           "-Wl,-rpath," + lib_dir, "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    w, h, sample = 40, 24, 5
    n = w * h
    scene = pkg.Scene.from_arrays(scenes.cornell_box())
    path = str(tmp_path / "cornell.crtbin")
    scene.save(path)
    out = str(tmp_path / "out.bin")
    subprocess.check_call([exe, path, str(w), str(h), "200", str(sample), out], timeout=120)
    raw = np.fromfile(out, dtype=np.float32)
    parts = np.split(raw, np.cumsum([8 * n, 8 * n, 3 * n, 3 * n, n, 3 * n]))
    assert len(parts) == 7 and parts[6].size == 3 * n
    renderer.upload_scene(scene)
    renderer.set_camera_from(scene)
    try:
        renderer.change_shading_mode(200)
        renderer.set_path_params(4, 3, 1234)
        assert np.array_equal(_bits(parts[0]), _bits(renderer.camera_rays(w, h)).reshape(-1))
        assert np.array_equal(_bits(parts[1]), _bits(renderer.camera_rays(w, h, sample=sample)).reshape(-1))
        g = renderer.frame_guides(w, h)
        for i, k in ((2, "normal"), (3, "albedo"), (4, "t")):
            assert np.array_equal(_bits(parts[i]), _bits(g[k]).reshape(-1)), k
        frame = renderer.render_frame(w, h, want=("rgba8", "rgb"))
        assert np.array_equal(_bits(parts[5]), _bits(frame["rgb"]).reshape(-1))
        den = renderer.denoise(frame["rgb"], g["normal"], g["albedo"], g["t"])
        assert np.array_equal(_bits(parts[6]), _bits(den).reshape(-1))
        assert not np.array_equal(_bits(den), _bits(frame["rgb"]))

        tool = os.path.join(lib_dir, "crt_render")
        base = [tool, path, "--mode", "200", "--size", "%dx%d" % (w, h), "--spp", "4"]
        subprocess.check_call(base + ["--out", str(tmp_path / "plain")], timeout=120, stdout=subprocess.DEVNULL)
        subprocess.check_call(base + ["--denoise", "--out", str(tmp_path / "den")], timeout=120, stdout=subprocess.DEVNULL)
        plain, filtered = _read_ppm(str(tmp_path / "plain_0.ppm")), _read_ppm(str(tmp_path / "den_0.ppm"))
        np.testing.assert_array_equal(plain, frame["rgba8"][:, :, :3])
        assert plain.shape == filtered.shape and not np.array_equal(plain, filtered)
        unorm = (np.clip(np.nan_to_num(den, nan=0.0), 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
        np.testing.assert_array_equal(filtered, unorm)
        assert subprocess.run(base + ["--denoise", "--denoise-iterations", "9"], capture_output=True, timeout=60).returncode == 2
    finally:
        renderer.set_path_params(4, 3, 1234)
        renderer.change_shading_mode(0)
        scene.close()
