"""The host forms of the C ABI are their device forms run over the context's staging buffer ("Host forms"): the same
kernels on the same bytes, so every comparison here is bit for bit (torch.equal on the raw bytes), on the smallest shapes that
reach every branch -- 8 x 8 and 24 x 16 frames, 64 and 384 records, a dynamic scene of two quads (four triangles) of which one
has moved since the snapshot.

What the arithmetic tests never visit is aimed at here: a stage pointer held across a regrow, room given to a buffer the caller
left out, a forgotten or misplaced download, one call's layout still in the stage when the next call plans its own.  The cases
share one context and run back to back; the growth test makes a context of its own so that its stage is certain to grow."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL, LARGE = (8, 8), (24, 16)
MATS = [{"albedo": (0.8, 0.8, 0.8), "type": 1}, {"albedo": (0.7, 0.4, 0.3), "type": 1}]
LIGHTS = [((0.0, 4.0, 2.0), 60.0)]
CAM = (0.0, 0.0, 2.0)
MOVE = np.float32([[1, 0, 0, 0.15], [0, 1, 0, -0.1], [0, 0, 1, 0.2]])


def _quad(cx, z, material):
    """a quad of two triangles facing +z, 2.4 wide, centred at (cx, 0, z)"""
    V = np.float32([(cx - 1.2, -1.2, z), (cx + 1.2, -1.2, z), (cx + 1.2, 1.2, z), (cx - 1.2, 1.2, z)])
    return {"vertices": V, "triangles": np.uint32([(0, 1, 2), (0, 2, 3)]), "material_index": material, "normals": None}


def _context(pkg, scenes):
    """the two quads overlap for |x| < 0.6 (rays there cross both); the front one moves after the snapshot"""
    r = pkg.Renderer(0)
    r.upload([_quad(-0.6, -1.0, 0), _quad(0.6, -2.0, 1)], LIGHTS, MATS, dynamic=True)
    r.set_camera(CAM, scenes.camera_matrix(0.0, 0.0))
    r.motion_snapshot()
    r.set_mesh_transform(0, MOVE)
    return r


@pytest.fixture(scope="module")
def r(pkg, scenes):
    ctx = _context(pkg, scenes)
    yield ctx
    ctx.close()


def _raw(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())


def _up(a):
    """a host array's bytes on the device"""
    return None if a is None else _raw(a).cuda()


def _room(nbytes, fill=0xA5):
    import torch
    return torch.full((int(nbytes),), fill, dtype=torch.uint8, device="cuda")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _same(host, dev):
    import torch
    return torch.equal(_raw(host), dev.cpu())


def _cam(scenes, pos):
    return np.concatenate([np.float32(pos), np.asarray(scenes.camera_matrix(0.0, 0.0), np.float32).reshape(9)])


def _frame(r, scenes, size, seed=5):
    """the inputs of the frame calls at one size: a random colour over the scene's real guides and previous points, and the
    history and moments a first host call (no history) leaves"""
    w, h = size
    g = r.frame_guides(w, h)
    f = {"w": w, "h": h, "normal": g["normal"], "albedo": g["albedo"], "t": g["t"], "prev_point": r.frame_motion(w, h),
         "rgb": np.random.default_rng(seed).random((h, w, 3), dtype=np.float32), "cur": _cam(scenes, CAM), "prev": _cam(scenes, (0.05, 0.0, 2.02))}
    assert (g["t"] < 10000.0).any() and (g["t"] == 10000.0).any() and np.isfinite(f["prev_point"]).any(), "hits, misses and moved pixels"
    f["hist"], f["mom"], f["var"], _ = r.temporal_variance(f["prev"], f["prev"], f["rgb"] * 0.5, f["normal"], f["albedo"], f["t"])
    return f


# what a caller may leave out of the temporal calls, one at a time
TEMPORAL_VARIANTS = {"all": {}, "no out": {"out": False}, "no albedo": {"albedo": False}, "no prev_point": {"prev_point": False},
                     "no history": {"history": False}}


def _temporal_pair(r, f, moments, out=True, albedo=True, prev_point=True, history=True):
    """one temporal call in its host and its device form: [(host array, device bytes), ...] of every output"""
    w, h, n = f["w"], f["h"], f["w"] * f["h"]
    prm = {} if albedo else {"demodulate": 0}
    alb = f["albedo"] if albedo else None
    pp = f["prev_point"] if prev_point else None
    hp, mp = (f["hist"], f["mom"]) if history else (None, None)
    d_in = [_up(a) for a in (f["rgb"], f["normal"], alb, f["t"], hp, mp, pp)]
    d_hist, d_mom, d_var, d_out = _room(n * 32), _room(n * 8), _room(n * 4), _room(n * 12) if out else None
    import torch
    torch.cuda.synchronize()
    if moments:
        host = r.temporal_variance(f["cur"], f["prev"], f["rgb"], f["normal"], alb, f["t"], hp, mp, want_out=out, prev_point=pp, **prm)
        r.temporal_variance_device(w, h, f["cur"], f["prev"], _ptr(d_in[0]), _ptr(d_in[1]), _ptr(d_in[2]), _ptr(d_in[3]), _ptr(d_in[4]),
                                   _ptr(d_hist), _ptr(d_in[5]), _ptr(d_mom), _ptr(d_var), _ptr(d_out), d_prev_point=_ptr(d_in[6]), **prm)
        pairs = [(host[0], d_hist), (host[1], d_mom), (host[2], d_var)]
    else:
        host = r.temporal_accumulate(f["cur"], f["prev"], f["rgb"], f["normal"], alb, f["t"], hp, want_out=out, prev_point=pp, **prm)
        r.temporal_accumulate_device(w, h, f["cur"], f["prev"], _ptr(d_in[0]), _ptr(d_in[1]), _ptr(d_in[2]), _ptr(d_in[3]), _ptr(d_in[4]),
                                     _ptr(d_hist), _ptr(d_out), d_prev_point=_ptr(d_in[6]), **prm)
        pairs = [(host[0], d_hist)]
    r.synchronize()
    assert (host[-1] is None) == (not out)
    return pairs + ([(host[-1], d_out)] if out else [])


def _assert_pairs(pairs, what):
    for k, (host, dev) in enumerate(pairs):
        assert _same(host, dev), "%s: output %d" % (what, k)


def test_stage_growth_and_reuse(r, pkg, scenes):
    """on a fresh context the call with the most planes runs at 8 x 8, at 24 x 16 (the stage regrows) and at 8 x 8 again (the stage
    is larger than the layout); with a host query between them whose layout is another one.  Every result equals the device
    form's and the third equals the first.  (The inputs come from the shared context: the fresh one's stage grows in the calls
    that are compared.)"""
    frames = {size: _frame(r, scenes, size) for size in (SMALL, LARGE)}
    ctx = _context(pkg, scenes)
    try:
        results = []
        for size in (SMALL, LARGE, SMALL):
            f = frames[size]
            pairs = _temporal_pair(ctx, f, True)
            _assert_pairs(pairs, "temporal_variance at %d x %d" % size)
            results.append([host.copy() for host, _ in pairs])
            rays = ctx.camera_rays(*size)
            hit = ctx.trace_rays(rays)
            d_t = _room(4 * len(rays))
            ctx.trace_rays_device(len(rays), _ptr(_up(rays)), d_t=_ptr(d_t), stats=True)
            assert _same(hit["t"], d_t), "trace_rays at %d x %d" % size
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(results[0], results[2]))
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", list(TEMPORAL_VARIANTS))
@pytest.mark.parametrize("moments", [False, True], ids=["accumulate", "variance"])
def test_temporal_forms(r, scenes, moments, variant):
    """crt_temporal_accumulate / _motion / crt_temporal_variance: every buffer given, and out, albedo (demodulate = 0),
    prev_point, and hist_prev with mom_prev left out in turn"""
    _assert_pairs(_temporal_pair(r, _frame(r, scenes, SMALL), moments, **TEMPORAL_VARIANTS[variant]), variant)


@pytest.mark.parametrize("variance_out", [None, False, True], ids=["denoise", "variance", "variance with variance_out"])
def test_denoise_forms(r, scenes, variance_out):
    """crt_denoise and crt_denoise_variance, the latter without and with variance_out; the device forms filter in place as the
    host forms do in the stage"""
    import torch
    f = _frame(r, scenes, LARGE)
    w, h = f["w"], f["h"]
    d = [_up(f[k]) for k in ("rgb", "normal", "albedo", "t", "var")]
    torch.cuda.synchronize()
    if variance_out is None:
        host = r.denoise(f["rgb"], f["normal"], f["albedo"], f["t"], iterations=3)
        r.denoise_device(w, h, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), _ptr(d[0]), iterations=3)
    else:
        host = r.denoise_variance(f["rgb"], f["normal"], f["albedo"], f["t"], f["var"], want_variance=variance_out, iterations=3)
        r.denoise_variance_device(w, h, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), _ptr(d[4]), _ptr(d[0]),
                                  _ptr(d[4]) if variance_out else None, iterations=3)
    r.synchronize()
    if variance_out:
        assert _same(host[1], d[4]), "variance_out"
        host = host[0]
    else:
        assert _same(f["var"], d[4]), "the variance is left alone"
    assert _same(host, d[0]) and not np.array_equal(host, f["rgb"])


QUERIES = {  # host method, device method, record kind, outputs: (name, bytes per record)
    "trace_rays": ("trace_rays_device", "rays", (("t", 4), ("uv", 8), ("inst", 4), ("prim", 4))),
    "shade_rays": ("shade_rays_device", "rays", (("rgb", 12), ("normal", 12), ("albedo", 12), ("t", 4), ("uv", 8), ("inst", 4), ("prim", 4))),
    "closest_points": ("closest_points_device", "points", (("dist", 4), ("point", 12), ("uv", 8), ("inst", 4), ("prim", 4))),
}


def _records(r, pkg, size):
    rays = r.camera_rays(*size)
    points = pkg.make_points(rays[:, :3] + rays[:, 4:7] * np.float32(6.5))
    return {"rays": rays, "points": points}


@pytest.mark.parametrize("name", list(QUERIES))
def test_query_outputs_alone_and_together(r, pkg, name):
    """crt_trace_rays, crt_shade_rays and crt_closest_points with every output and with each output alone: an output left out
    takes no room, and the others land where the kernel was told"""
    import torch
    device, kind, outputs = QUERIES[name]
    rec = _records(r, pkg, SMALL)[kind]
    n = len(rec)
    d_rec = _up(rec)
    r.change_shading_mode(100)
    for want in [tuple(k for k, _ in outputs)] + [(k,) for k, _ in outputs]:
        host = getattr(r, name)(rec, want=want)
        d = {k: _room(n * b) for k, b in outputs if k in want}
        torch.cuda.synchronize()
        getattr(r, device)(n, _ptr(d_rec), **{"d_" + k: _ptr(v) for k, v in d.items()})
        r.synchronize()
        for k in want:
            assert _same(host[k], d[k]), "%s of %s" % (k, want)


def test_single_output_queries_guides_and_previous_points(r, pkg):
    """crt_occluded_rays, crt_count_hits, crt_occupancy, crt_previous_points, and crt_frame_guides with each guide alone"""
    import torch
    rec = _records(r, pkg, SMALL)
    n = len(rec["rays"])
    d_rays, d_points = _up(rec["rays"]), _up(rec["points"])
    for host, device, d_rec, per in ((r.occluded(rec["rays"]), r.occluded_device, d_rays, 1), (r.count_hits(rec["rays"]), r.count_hits_device, d_rays, 4),
                                     (r.occupancy(rec["points"]), r.occupancy_device, d_points, 1)):
        d_out = _room(n * per)
        torch.cuda.synchronize()
        device(n, _ptr(d_rec), _ptr(d_out), stats=True)
        assert _same(host, d_out), device.__name__
    hit = r.trace_rays(rec["rays"])
    assert (hit["inst"] == 0).any() and (hit["inst"] == 1).any() and (hit["inst"] == 0xFFFFFFFF).any()
    host = r.previous_points(hit["inst"], hit["prim"], hit["uv"])
    d_out = _room(n * 12)
    d_in = [_up(hit[k]) for k in ("inst", "prim", "uv")]
    torch.cuda.synchronize()
    r.previous_points_device(n, _ptr(d_in[0]), _ptr(d_in[1]), _ptr(d_in[2]), _ptr(d_out), stats=True)
    assert _same(host, d_out) and np.isfinite(host).any() and np.isnan(host).any()
    w, h = SMALL
    for want in (("normal", "albedo", "t"), ("normal",), ("albedo",), ("t",)):
        host = r.frame_guides(w, h, want=want)
        d = {k: _room(w * h * (4 if k == "t" else 12)) for k in want}
        torch.cuda.synchronize()
        r.frame_guides_device(w, h, **{"d_" + k: _ptr(v) for k, v in d.items()}, stats=True)
        for k in want:
            assert _same(host[k], d[k]), "%s of %s" % (k, want)


def test_alternating_entry_points(r, pkg, scenes):
    """crt_denoise, crt_trace_rays, crt_temporal_variance and crt_path_rays by turns on one context: each call plans its layout
    over what the one before left in the stage, and every round gives the bits of the first"""
    f = _frame(r, scenes, SMALL)
    rays = _records(r, pkg, LARGE)["rays"]
    first = None
    for _ in range(3):
        got = [r.denoise(f["rgb"], f["normal"], f["albedo"], f["t"]), r.trace_rays(rays)["t"],
               *r.temporal_variance(f["cur"], f["prev"], f["rgb"], f["normal"], f["albedo"], f["t"], f["hist"], f["mom"], prev_point=f["prev_point"]),
               r.path_rays(rays, n_samples=2)["rgb"], r.frame_guides(*SMALL, want=("t",))["t"]]
        first = first or got
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, got))
    pairs = _temporal_pair(r, f, True)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, (b, _) in zip(first[2:6], pairs))
    _assert_pairs(pairs, "after the rounds")


def _call(r, pkg, name, *args):
    rc = getattr(pkg.lib(), name)(r.h, *args)
    assert rc == 0, "%s: %d (%s)" % (name, rc, pkg.lib().crt_last_error(r.h))


def test_stats_change_no_output(r, pkg, scenes):
    """crt_denoise, crt_trace_rays, crt_path_rays and crt_list_hits with and without stats: equal outputs, and positive kernel_ms
    and total_ms when they were asked for"""
    f = _frame(r, scenes, SMALL)
    rays = _records(r, pkg, SMALL)["rays"]
    n, (w, h) = len(rays), SMALL
    p = lambda a: a.ctypes.data  # noqa: E731

    def run(st):
        s = None if st is None else C.byref(st)
        out = [np.zeros((h, w, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n + 1, np.uint64)]
        _call(r, pkg, "crt_denoise", w, h, p(f["rgb"]), p(f["normal"]), p(f["albedo"]), p(f["t"]), p(out[0]), None, s)
        times = [] if st is None else [(st.kernel_ms, st.total_ms)]
        _call(r, pkg, "crt_trace_rays", n, p(rays), p(out[1]), None, None, None, s)
        times += [] if st is None else [(st.kernel_ms, st.total_ms)]
        _call(r, pkg, "crt_path_rays", n, p(rays), None, 0, 2, p(out[2]), None, None, None, None, None, s)
        times += [] if st is None else [(st.kernel_ms, st.total_ms)]
        _call(r, pkg, "crt_list_hits", n, p(rays), p(out[3]), 0, None, None, None, None, None, s)
        times += [] if st is None else [(st.kernel_ms, st.total_ms)]
        return out, times
    plain, _ = run(None)
    timed, times = run(pkg.FrameStats())
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(plain, timed))
    assert len(times) == 4 and all(k > 0.0 and t > 0.0 for k, t in times), times
    assert plain[3][-1] > 0, "the listing found hits"


def test_path_rays_sums(r, pkg):
    """crt_path_rays honours the sums it is given once first_sample > 0 and ignores them at first_sample = 0: two calls of 2
    samples equal one call of 4 (as tests/test_path_rays.py holds the device form to), and equal the device form's bytes"""
    import torch
    rays = _records(r, pkg, SMALL)["rays"]
    n = len(rays)
    whole_sums = np.full((n, 3), -3e9, np.float64)  # (a first call must not read them)
    whole = r.path_rays(rays, n_samples=4, sums=whole_sums, want=("rgb",))["rgb"]
    sums = np.full((n, 3), 1e9, np.float64)
    r.path_rays(rays, first_sample=0, n_samples=2, sums=sums, want=())
    assert (sums < 1e8).all() and (sums > 0.0).any()
    half = sums.copy()
    got = r.path_rays(rays, first_sample=2, n_samples=2, sums=sums, want=("rgb",))["rgb"]
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)) and np.array_equal(sums.view(np.uint64), whole_sums.view(np.uint64))
    assert not np.array_equal(sums, half)
    d_rays, d_sums, d_rgb = _up(rays), _up(half), _room(n * 12)
    torch.cuda.synchronize()
    r.path_rays_device(n, _ptr(d_rays), first_sample=2, n_samples=2, d_rgb=_ptr(d_rgb), d_sums=_ptr(d_sums), stats=True)
    assert _same(got, d_rgb) and _same(sums, d_sums)
    # other sums in, another mean out: they are read
    other = r.path_rays(rays, first_sample=2, n_samples=2, sums=half * 2.0 + 1.0, want=("rgb",))["rgb"]
    assert not np.array_equal(other, got)


def test_list_hits_capacity(r, pkg):
    """crt_list_hits with a capacity one too small, exactly sufficient and zero: offsets and total equal the device form's; the
    record arrays are filled only when the total fits, and equal the device form's then"""
    import torch
    rays = _records(r, pkg, LARGE)["rays"]
    n = len(rays)
    counts = np.diff(r.list_hits(rays, want=())["offsets"])
    total = int(counts.sum())
    assert (counts == 0).any() and (counts == 2).any(), "rays miss, and rays through the quads' overlap cross both"
    d_rays = _up(rays)
    p = lambda a: a.ctypes.data  # noqa: E731
    for capacity in (total - 1, total, 0):
        off, tot = np.zeros(n + 1, np.uint64), C.c_uint64(0)
        rec = {"t": np.full(total, -7.0, np.float32), "uv": np.full((total, 2), -7.0, np.float32), "inst": np.full(total, 77, np.uint32),
               "prim": np.full(total, 77, np.uint32)}
        untouched = {k: v.copy() for k, v in rec.items()}
        _call(r, pkg, "crt_list_hits", n, p(rays), p(off), capacity, p(rec["t"]), p(rec["uv"]), p(rec["inst"]), p(rec["prim"]), C.byref(tot), None)
        d_off = _room(8 * (n + 1))
        d = {"t": _room(4 * total), "uv": _room(8 * total), "inst": _room(4 * total), "prim": _room(4 * total)}
        torch.cuda.synchronize()
        d_tot = r.list_hits_device(n, _ptr(d_rays), _ptr(d_off), capacity, **{"d_" + k: _ptr(v) for k, v in d.items()}, total=True)
        r.synchronize()
        assert tot.value == d_tot == total and _same(off, d_off), capacity
        for k in rec:
            if capacity == total:
                assert _same(rec[k], d[k]) and not np.array_equal(rec[k], untouched[k]), k
            else:
                assert np.array_equal(rec[k], untouched[k]), "%s with capacity %d" % (k, capacity)


def test_frame_and_query_on_two_streams(r, pkg):
    """a mode-200 frame on one stream and a path-traced query on another, issued by turns on one context: the frames' arenas and
    the queries' arenas are pools apart, so each result equals its single-stream run"""
    import torch
    w, h = LARGE
    rays = _records(r, pkg, LARGE)["rays"]
    n = len(rays)
    d_rays = _up(rays)
    r.change_shading_mode(200)
    try:
        def issue():
            frame, rgb = _room(4 * w * h), _room(12 * n)
            return frame, rgb, lambda: r.render_frame_device(w, h, _ptr(frame)), lambda: r.path_rays_device(n, _ptr(d_rays), n_samples=3, d_rgb=_ptr(rgb))
        want_frame, want_rgb, frame_call, query_call = issue()
        torch.cuda.synchronize()
        frame_call()
        query_call()
        r.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        rounds = [issue() for _ in range(3)]
        torch.cuda.synchronize()
        for _, _, frame_call, query_call in rounds:
            r.set_stream(streams[0].cuda_stream)
            frame_call()
            r.set_stream(streams[1].cuda_stream)
            query_call()
        torch.cuda.synchronize()
        r.reset_stream()
        assert len(torch.unique(want_frame)) > 4, "the frame shows the scene"
        for frame, rgb, _, _ in rounds:
            assert torch.equal(frame, want_frame) and torch.equal(rgb, want_rgb)
    finally:
        r.reset_stream()
        r.change_shading_mode(0)
