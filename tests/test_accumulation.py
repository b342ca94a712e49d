"""Progressive accumulation of mode 200 (crt_set_accumulation, include/crt_hip.h).  A frame traces samples n .. n+spp-1 of
one long run and adds them to per-pixel sums in sample order, so K frames of S spp are, bit for bit, one frame of K*S spp --
which the CPU oracle renders directly (oracle.set_path_params(spp=K*S)).  Every GPU check here is exact, not a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

SYMBOLS = ("crt_set_accumulation", "crt_reset_accumulation", "crt_accumulated_samples")
FULL = ("rgba8", "hit_inst", "hit_prim", "hit_t", "rgb")
MAX = 1 << 24


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _with_normals(scenes, sc):
    sc = dict(sc)
    sc["meshes"] = [dict(m, normals=scenes.vertex_normals(m["vertices"], m["triangles"])) for m in sc["meshes"]]
    return sc


def _cornell_all_materials(scenes):
    sc = scenes.cornell_box()
    sc["materials"][1] = {"albedo": (0.9, 0.9, 0.9), "type": 2}              # left wall mirror
    sc["materials"][2] = {"albedo": (1.0, 1.0, 1.0), "type": 3, "ior": 1.5}  # right wall glass
    return sc


# ---- CPU: the interface exists

def test_binding_and_library_expose_accumulation(pkg):
    for name in ("set_accumulation", "reset_accumulation", "accumulated_samples"):
        assert callable(getattr(pkg.Renderer, name, None)), name
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
    assert L.crt_abi_version() == 1


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    n = C.c_uint32(7)
    assert L.crt_set_accumulation(None, 16) == 1
    assert L.crt_set_accumulation(None, 0) == 1
    assert L.crt_reset_accumulation(None) == 1
    assert L.crt_accumulated_samples(None, C.byref(n)) == 1


def test_driver_usage_lists_accumulate(pkg):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "crt_render")
    assert os.path.exists(exe), "crt_render not built"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)  # no scene: usage, before anything touches a GPU
    assert out.returncode == 2 and "--accumulate MAX" in out.stderr


# ---- GPU

def _setup(renderer, sc, miss=(0.0, 0.0, 0.0), spp=4, bounces=3, seed=1234):
    renderer.set_accumulation(0)
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"))
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
    renderer.set_miss_color(miss)
    renderer.change_shading_mode(200)
    renderer.set_path_params(spp, bounces, seed)


def _restore(renderer):
    renderer.set_accumulation(0)
    renderer.set_counting(False)
    renderer.set_path_params(4, 3, 1234)
    renderer.set_miss_color((0.0, 1.0, 1.0))
    for k, v in (("path_pipeline", 0), ("path_tile", 0), ("path_ranges", 8), ("path_pass_paths", 1 << 24)):
        renderer.set_option(k, v)


def _single(renderer, w, h, spp):
    """one frame of spp samples with accumulation off"""
    acc = renderer.accumulated_samples()
    assert acc == 0, "call with accumulation off"
    renderer.set_option("spp", spp)
    return renderer.render_frame(w, h)


def _accumulate(renderer, w, h, spps, between=None):
    """accumulation on from scratch, one frame per entry of spps; returns the frames and the counts after each"""
    renderer.set_accumulation(MAX)
    frames, counts = [], []
    for i, s in enumerate(spps):
        if between:
            between(i)
        renderer.set_option("spp", s)
        frames.append(renderer.render_frame(w, h))
        counts.append(renderer.accumulated_samples())
    renderer.set_accumulation(0)
    return frames, counts


def _oracle_frame(oracle, O, cam, w, h, spp, bounces=3, seed=1234, miss=(0.0, 0.0, 0.0), rows=None):
    oracle.set_path_params(spp, bounces, seed)
    try:
        return O.render(cam["position"], cam["matrix"], oracle.MODE_PATH, w, h, miss_rgb=miss, rows=rows)
    finally:
        oracle.set_path_params(4, 3, 1234)


def _same_image(a, b, what):
    np.testing.assert_array_equal(a["rgba8"], b["rgba8"], err_msg=what + " rgba8")
    assert np.array_equal(a["rgb"], b["rgb"], equal_nan=True), what + " rgb"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cornell", "dragon"])
def test_k_frames_equal_one_long_frame(pkg, oracle, scenes, dragon, renderer, which):
    """K frames of S spp == one GPU frame of K*S spp == the oracle at K*S spp, for multi-pass frames (37 spp: passes of 16 + 16
    + 5), spp that changes between frames, both pipelines, both tile sizes, and tuning options changed mid-accumulation."""
    sc, w, h = (_cornell_all_materials(scenes), 256, 256) if which == "cornell" else (_with_normals(scenes, dragon), 640, 360)
    cam = sc["camera"]
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], textures=sc.get("textures") or ())
    _setup(renderer, sc)
    try:
        for spps in ((4, 4, 4, 4), (37, 37), (4, 1, 3)):
            total = sum(spps)
            long = _single(renderer, w, h, total)
            # the long GPU frame is the oracle's (Dragon at 74 spp: every 9th row, the oracle is a CPU)
            rows = (0, h, 9) if (which == "dragon" and total > 16) else None
            ref = _oracle_frame(oracle, O, cam, w, h, total, rows=rows)
            sel = slice(None) if rows is None else slice(rows[0], rows[1], rows[2])
            for k in FULL:
                np.testing.assert_array_equal(long[k][sel], ref[k][sel], err_msg="%s %r %s vs oracle" % (which, spps, k))
            first = _single(renderer, w, h, spps[0])
            for pipeline, tile in ((0, 8), (0, 16), (1, 8)):
                renderer.set_option("path_pipeline", pipeline)
                renderer.set_option("path_tile", tile)
                frames, counts = _accumulate(renderer, w, h, spps)
                assert counts == list(np.cumsum(spps)), counts
                what = "%s %r pipeline %d tile %d" % (which, spps, pipeline, tile)
                _same_image(frames[-1], long, what)
                _same_image(frames[0], first, what + " first frame")
                for k in ("hit_inst", "hit_prim", "hit_t"):  # the first frame after a reset reports sample 0, as without accumulation
                    np.testing.assert_array_equal(frames[0][k], long[k], err_msg=what + " " + k)
            renderer.set_option("path_pipeline", 0)
            renderer.set_option("path_tile", 0)
        # tuning options changed between frames: the sums continue
        knobs = [{}, {"path_tile": 16, "path_ranges": 1}, {"path_pipeline": 1, "path_tile": 8, "path_pass_paths": 65536}, {"path_pipeline": 0}]

        def switch(i):
            for k, v in knobs[i].items():
                renderer.set_option(k, v)
        frames, counts = _accumulate(renderer, w, h, (4, 4, 4, 4), between=switch)
        assert counts == [4, 8, 12, 16]
        _restore(renderer)
        _setup(renderer, sc)
        _same_image(frames[-1], _single(renderer, w, h, 16), which + " options changed mid-accumulation")
    finally:
        _restore(renderer)


@pytest.mark.gpu
def test_limit_then_resolve_only(pkg, oracle, scenes, renderer):
    """max_samples 10 at 4 spp: 4, 8, 10 (a 2-sample frame), then 10 again with nothing traced; frame 3 is the oracle's 10 spp."""
    sc, w, h = _cornell_all_materials(scenes), 256, 256
    _setup(renderer, sc)
    try:
        renderer.set_accumulation(10)
        renderer.set_counting(True)
        frames, counts = [], []
        for _ in range(4):
            frames.append(renderer.render_frame(w, h))
            counts.append(renderer.accumulated_samples())
        assert counts == [4, 8, 10, 10]
        O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
        ref = _oracle_frame(oracle, O, sc["camera"], w, h, 10)
        _same_image(frames[2], ref, "frame 3 vs oracle at 10 spp")
        _same_image(frames[3], frames[2], "saturated frame")
        assert frames[2]["stats"]["rays_primary"] > 0
        st = frames[3]["stats"]
        assert (st["rays_primary"], st["rays_shadow"], st["nodes_visited"], st["tris_tested"]) == (0, 0, 0, 0)
        # the device entry point at the limit: the same bytes, from the stored sums
        import torch
        d = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        rgb = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        st = renderer.render_frame_device(w, h, d.data_ptr(), d_rgb=rgb.data_ptr(), stats=True)
        assert st["rays_primary"] == 0 and renderer.accumulated_samples() == 10
        assert np.array_equal(d.cpu().numpy().view(np.uint8).reshape(h, w, 4), frames[2]["rgba8"])
        assert np.array_equal(rgb.cpu().numpy().reshape(h, w, 3), frames[2]["rgb"])
    finally:
        _restore(renderer)


@pytest.mark.gpu
def test_reset_rules(pkg, scenes, renderer):
    sc, w, h, S = _cornell_all_materials(scenes), 128, 96, 2
    cam = sc["camera"]
    moved = np.float32(cam["position"]) + np.float32([0.05, 0.0, 0.0])
    _setup(renderer, sc, spp=S)
    try:
        def fresh(w_=w, h_=h):
            renderer.set_accumulation(0)
            return _single(renderer, w_, h_, S)

        def two_then(change, w2=w, h2=h):
            """two accumulated frames, then `change` and one more frame: it must be a fresh S-spp frame"""
            renderer.set_accumulation(MAX)
            renderer.render_frame(w, h)
            renderer.render_frame(w, h)
            assert renderer.accumulated_samples() == 2 * S
            change()
            got = renderer.render_frame(w2, h2)
            n = renderer.accumulated_samples()
            ref = fresh(w2, h2)
            return got, n, ref

        cases = {
            "camera": (lambda: renderer.set_camera(moved, cam["matrix"]), lambda: renderer.set_camera(cam["position"], cam["matrix"])),
            "miss colour": (lambda: renderer.set_miss_color((0.3, 0.2, 0.1)), lambda: renderer.set_miss_color((0.0, 0.0, 0.0))),
            "seed": (lambda: renderer.set_option("seed", 77), lambda: renderer.set_option("seed", 1234)),
            "max_bounces": (lambda: renderer.set_option("max_bounces", 1), lambda: renderer.set_option("max_bounces", 3)),
            "scene": (lambda: renderer.upload(sc["meshes"], sc["lights"], sc["materials"]), lambda: None),
        }
        for what, (change, undo) in cases.items():
            got, n, ref = two_then(change)
            assert n == S, what
            _same_image(got, ref, what)
            undo()
        got, n, ref = two_then(lambda: None, 96, 64)
        assert n == S
        _same_image(got, ref, "resolution")
        # the same pose set again, and 200 -> 3 -> 200: the sums continue
        renderer.set_accumulation(MAX)
        renderer.render_frame(w, h)
        renderer.set_camera(np.float32(cam["position"]).copy(), np.float32(cam["matrix"]).copy())
        renderer.render_frame(w, h)
        assert renderer.accumulated_samples() == 2 * S
        renderer.change_shading_mode(3)
        renderer.render_frame(w, h)
        assert renderer.accumulated_samples() == 2 * S
        renderer.change_shading_mode(200)
        got = renderer.render_frame(w, h)
        assert renderer.accumulated_samples() == 3 * S
        renderer.set_accumulation(0)
        _same_image(got, _single(renderer, w, h, 3 * S), "same pose / mode 3 in between")
        # crt_reset_accumulation starts over
        renderer.set_option("spp", S)
        renderer.set_accumulation(MAX)
        renderer.render_frame(w, h)
        renderer.reset_accumulation()
        assert renderer.accumulated_samples() == 0
        got = renderer.render_frame(w, h)
        assert renderer.accumulated_samples() == S
        _same_image(got, fresh(), "after reset")
    finally:
        _restore(renderer)


@pytest.mark.gpu
def test_other_modes_are_untouched(pkg, scenes, renderer):
    sc, w, h = _cornell_all_materials(scenes), 160, 120
    _setup(renderer, sc)
    try:
        for mode in (3, 100):
            renderer.change_shading_mode(mode)
            off = renderer.render_frame(w, h)
            renderer.set_accumulation(64)
            on = [renderer.render_frame(w, h) for _ in range(2)]
            assert renderer.accumulated_samples() == 0
            renderer.set_accumulation(0)
            for f in on:
                for k in FULL:
                    np.testing.assert_array_equal(f[k], off[k], err_msg="mode %d %s" % (mode, k))
    finally:
        _restore(renderer)


@pytest.mark.gpu
def test_tile_shares_accumulate_per_rank(pkg, scenes, dragon, renderer):
    """One context per rank (N = 2, 4 on one GPU), K frames each through crt_render_tiles_device: the untiled shares are the
    whole frame accumulated over the same K frames."""
    import torch
    sc, w, h, K, S = _with_normals(scenes, dragon), 333, 190, 3, 2
    _setup(renderer, sc, spp=S)
    try:
        frames, _ = _accumulate(renderer, w, h, (S,) * K)
        whole = frames[-1]["rgba8"].view(np.uint32).reshape(h, w)
        for n in (2, 4):
            slots = pkg.tile_slots(w, h, n)
            gathered = torch.zeros(n * slots * 256, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ranks = [pkg.Renderer(0) for _ in range(n)]
            try:
                for r in ranks:
                    _setup(r, sc, spp=S)
                    r.set_accumulation(MAX)
                for _ in range(K):
                    for rank, r in enumerate(ranks):
                        r.render_tiles_device(w, h, rank, n, gathered.data_ptr() + rank * slots * 1024)
                for r in ranks:
                    r.synchronize()
                    assert r.accumulated_samples() == K * S
            finally:
                for r in ranks:
                    r.close()
            host = pkg.untile_host(gathered.cpu().numpy().view(np.uint32), w, h, n)
            np.testing.assert_array_equal(host.reshape(h, w), whole, err_msg="%d ranks" % n)
    finally:
        _restore(renderer)


@pytest.mark.gpu
def test_batch_entry_points_refuse_to_accumulate(pkg, scenes, renderer):
    import torch
    sc, w, h, S = _cornell_all_materials(scenes), 128, 96, 2
    _setup(renderer, sc, spp=S)
    try:
        renderer.set_accumulation(MAX)
        renderer.render_frame(w, h)
        outs = [torch.zeros(h * w, dtype=torch.int32, device="cuda") for _ in range(2)]
        staging = [torch.zeros(pkg.tile_slots(w, h, 2) * 256, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        with pytest.raises(pkg.CrtError, match="accumulat"):
            renderer.render_frames_batch_device(w, h, [o.data_ptr() for o in outs])
        with pytest.raises(pkg.CrtError, match="accumulat"):
            renderer.render_tiles_batch_device(w, h, 0, 2, [s.data_ptr() for s in staging])
        torch.cuda.synchronize()
        assert not any(o.any().item() for o in outs + staging)
        assert renderer.accumulated_samples() == S
        got = renderer.render_frame(w, h)  # the sums were left as they were
        assert renderer.accumulated_samples() == 2 * S
        renderer.set_accumulation(0)
        _same_image(got, _single(renderer, w, h, 2 * S), "after the refused batches")
    finally:
        _restore(renderer)


@pytest.mark.gpu
def test_frames_on_alternating_streams(pkg, scenes, renderer):
    """Accumulating frames issued on two streams, without host synchronisation in between: ordered on the GPU through the sums."""
    import torch
    sc, w, h, S, K = _cornell_all_materials(scenes), 256, 256, 3, 6
    _setup(renderer, sc, spp=S)

    def run(streams):
        outs = [torch.zeros(h * w, dtype=torch.int32, device="cuda") for _ in range(K)]
        rgb = [torch.zeros(h * w * 3, dtype=torch.float32, device="cuda") for _ in range(K)]
        torch.cuda.synchronize()
        renderer.set_accumulation(MAX)
        for i in range(K):
            renderer.set_stream(streams[i % len(streams)].cuda_stream)
            renderer.render_frame_device(w, h, outs[i].data_ptr(), d_rgb=rgb[i].data_ptr())
        torch.cuda.synchronize()
        assert renderer.accumulated_samples() == K * S
        renderer.set_accumulation(0)
        renderer.reset_stream()
        return [o.cpu().numpy() for o in outs], [x.cpu().numpy() for x in rgb]

    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        one = run([s1])
        two = run([s1, s2])
        for i in range(K):
            assert np.array_equal(one[0][i], two[0][i]), "frame %d rgba8" % i
            assert np.array_equal(one[1][i], two[1][i]), "frame %d rgb" % i
    finally:
        renderer.reset_stream()
        _restore(renderer)


@pytest.mark.gpu
def test_driver_accumulates_until_the_camera_moves(pkg, oracle, scenes, dragon, tmp_path, golden_dir):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "crt_render")
    scene_file = os.path.join(golden_dir, "dragon.crtscene")
    w, h = 160, 96
    sc = _with_normals(scenes, dragon)
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])

    def ppm(path):
        raw = open(path, "rb").read()
        end = raw.index(b"255\n") + 4
        assert raw[:end] == b"P6\n%d %d\n255\n" % (w, h)
        return np.frombuffer(raw[end:], dtype=np.uint8).reshape(h, w, 3)

    def ref(pos, rot, spp):
        oracle.set_path_params(spp, 3, 1234)
        try:
            return O.render(pos, rot, 200, w, h)["rgba8"][..., :3]
        finally:
            oracle.set_path_params(4, 3, 1234)

    s = pkg.Scene(scene_file)
    pos, rot = s.camera()
    prefix = str(tmp_path / "still")
    out = subprocess.run([exe, scene_file, "--mode", "200", "--spp", "2", "--frames", "4", "--accumulate", "64", "--size", "%dx%d" % (w, h),
                          "--out", prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "8 samples accumulated" in out.stdout
    np.testing.assert_array_equal(ppm(prefix + "_3.ppm"), ref(pos, rot, 8), err_msg="still camera, frame 3")
    # the camera moves before frame 2: frame 2 starts over (2 spp at the new pose), frame 3 continues (4 spp)
    path = tmp_path / "path.txt"
    path.write_text("\n\nrotate 5 0\n\n")
    prefix = str(tmp_path / "moving")
    out = subprocess.run([exe, scene_file, "--mode", "200", "--spp", "2", "--frames", "4", "--accumulate", "64", "--size", "%dx%d" % (w, h),
                          "--path", str(path), "--out", prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    s.rotate(5.0, 0.0)
    pos2, rot2 = s.camera()
    np.testing.assert_array_equal(ppm(prefix + "_1.ppm"), ref(pos, rot, 4), err_msg="moving camera, frame 1")
    np.testing.assert_array_equal(ppm(prefix + "_2.ppm"), ref(pos2, rot2, 2), err_msg="moving camera, frame 2")
    np.testing.assert_array_equal(ppm(prefix + "_3.ppm"), ref(pos2, rot2, 4), err_msg="moving camera, frame 3")
