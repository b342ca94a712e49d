"""Ray queries at any direction magnitude (include/crt_hip.h, ray records: "t is in units of |d|").

The slab reciprocal clamps every direction component below 1e-20 to +-1e-20.  Applied to the record as given, that clamp
cut the slabs of a ray whose direction is merely short (|d| ~ 1e-21): the box along the clamped axis was left at
gap * 1e20 instead of gap / |d_i|, and every box beyond was culled.  The kernels and the oracle shared that arithmetic, so
only a comparison with brute force (no boxes) sees it.  Queries now trace each record prescaled by the power of two that
brings its largest direction component into [1, 2).  Checked here:
- a record scaled by 2^k gives the same hit, u / v bits, occlusion and fetch counts, and t * 2^k is the unscaled t, bit
  for bit, wherever the scaled values stay exact;
- at any scale (1e-30 .. 1e30, not powers of two) and for mixed magnitudes (a component 2^-40 .. 2^-140 of the largest,
  signed zeros) the oracle's walks of the SAH, LBVH and PLOC trees equal brute force bit for bit, and brute force equals a
  float64 Moeller-Trumbore on the robust rays;
- hit counts (tests/point_reference.c) do not depend on the scale, and their parity on closed meshes is the winding number;
- the ends of the supported range (largest component 2^-149 and FLT_MAX) and a zero direction just outside it;
- on the GPU: trace_rays / occluded / count_hits and their device forms over SAH, LBVH and PLOC uploads and a moved dynamic
  mesh equal the oracle's walk of the exported tree and brute force, fetch counters included."""
import numpy as np
import pytest

import path_reference as R
import ploc_reference as spec
from test_point_queries import _tri_records, ref, ref_count, winding_number  # noqa: F401  (ref: the reference fixture)
from test_traversal_robustness import _check_float64, closed_scene, sliver_scene

MISS = 0xFFFFFFFF
FLT_MAX = np.float32(3.4028234663852886e38)
POW2 = (-100, -90, -70, -67, -66, -64, -40, -1, 1, 24, 66, 67, 90, 100)
SCALES = (1e-30, 3.7e-25, 1e-21, 7e-20, 1e-15, 0.3, 7.0, 1e15, 2.5e21, 1e30)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mesh(v, t):
    return {"vertices": np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3),
            "triangles": np.ascontiguousarray(t, dtype=np.uint32).reshape(-1, 3), "material_index": 0, "normals": None}


def quad_stack(n=64):
    """n parallel quads at x = 1..n spanning y, z in [-1, 1]: the scene of the clamp's failure"""
    v, t = [], []
    for k in range(n):
        x = float(k + 1)
        v += [(x, -1, -1), (x, 1, -1), (x, 1, 1), (x, -1, 1)]
        t += [(4 * k, 4 * k + 1, 4 * k + 2), (4 * k, 4 * k + 2, 4 * k + 3)]
    return {"meshes": [_mesh(v, t)], "lights": [], "materials": []}


def _scene(name, scenes, dragon):
    if name == "quads":
        return quad_stack()
    if name == "dragon":
        return dragon
    kind, off = name.split("-")
    if kind == "slivers":
        return sliver_scene(scenes, float(off))
    return closed_scene(scenes, kind, float(off), 0.0625 if kind == "sphere" else 1.0)


def _all_tris(sc):
    v0, v1, v2 = [], [], []
    for m in sc["meshes"]:
        v = np.asarray(m["vertices"], np.float32).reshape(-1, 3)
        t = np.asarray(m["triangles"], np.int64).reshape(-1, 3)
        v0.append(v[t[:, 0]]); v1.append(v[t[:, 1]]); v2.append(v[t[:, 2]])
    return np.concatenate(v0), np.concatenate(v1), np.concatenate(v2)


def _unit(d):
    """directions with the largest component in [1, 2) (powers of two away from what the rays are scaled by)"""
    d = np.asarray(d, np.float64)
    m = np.abs(d).max(1, keepdims=True)
    return np.float32(d / np.exp2(np.floor(np.log2(np.where(m > 0, m, 1.0)))))


def base_rays(pkg, sc, rng, n):
    """n seeded rays in five families: from outside the scene (tmin 0); starting on surfaces (tmin 0); tmin > 0 intervals
    that skip the first hits; negative tmin with tmax = inf; origins within 1e-3 of a plane of the geometry (a box face)"""
    V0, V1, V2 = _all_tris(sc)
    allv = np.concatenate([V0, V1, V2])
    lo, hi = allv.min(0), allv.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    k = n // 5

    def inside(m):
        return np.float32(lo + rng.random((m, 3)) * ext)

    def outside(m):
        o = lo - 0.5 * ext + rng.random((m, 3)) * 2.0 * ext
        far = rng.integers(0, 3, size=m)
        o[np.arange(m), far] = np.where(rng.random(m) < 0.5, lo[far] - 0.25 * ext[far], hi[far] + 0.25 * ext[far])
        return np.float32(o)

    def towards(o):
        d = inside(len(o)) - o
        d[np.abs(d).max(1) == 0, 0] = 1.0
        return _unit(d)

    def on_surface(m):
        tri = rng.integers(0, len(V0), size=m)
        b = rng.dirichlet((1.0, 1.0, 1.0), size=m).astype(np.float32)
        return np.float32(V0[tri] * b[:, 0:1] + V1[tri] * b[:, 1:2] + V2[tri] * b[:, 2:3])

    parts = []
    o = outside(k)
    parts.append(pkg.make_rays(o, towards(o), tmin=0.0, tmax=rng.choice([np.inf, 1e4], size=k)))
    o = on_surface(k)
    parts.append(pkg.make_rays(o, _unit(rng.normal(size=(k, 3))), tmin=0.0, tmax=np.inf))
    o = outside(k)
    d = towards(o)
    parts.append(pkg.make_rays(o, d, tmin=np.float32(rng.uniform(0.2, 1.0, size=k) * np.linalg.norm(ext) / np.abs(d).max(1)),
                               tmax=np.inf))
    o = inside(k)
    parts.append(pkg.make_rays(o, _unit(rng.normal(size=(k, 3))), tmin=np.float32(-rng.uniform(0.01, 2.0, size=k) * ext.max()),
                               tmax=np.inf))
    m = n - 4 * k
    o = np.float64(inside(m))
    ax = rng.integers(0, 3, size=m)
    o[np.arange(m), ax] = allv[rng.integers(0, len(allv), size=m), ax] + rng.uniform(-1e-3, 1e-3, size=m)
    o = np.float32(o)
    parts.append(pkg.make_rays(o, towards(o), tmin=0.0, tmax=np.inf))
    return np.ascontiguousarray(np.concatenate(parts))


def scale_rays(rays, s):
    """(o, tmin / s, d * s, tmax / s) in float32: the same ray with t in units of s |d|"""
    r = np.array(rays, np.float32, copy=True)
    if isinstance(s, int):  # a power of two, 2^s: exact wherever the scaled values stay in range
        r[:, 4:7] = np.ldexp(r[:, 4:7], s)
        r[:, [3, 7]] = np.ldexp(r[:, [3, 7]], -s)
    else:
        r[:, 4:7] = np.float32(np.float64(r[:, 4:7]) * s)
        r[:, [3, 7]] = np.float32(np.float64(r[:, [3, 7]]) / s)
    return r


def _exact(x, k):
    """x * 2^k is exact (neither rounded into the subnormals nor overflowed) and stays a normal float or zero"""
    x = np.asarray(x, np.float32)
    y = np.ldexp(x, k)
    return (np.ldexp(y, -k) == x) & ((y == 0) | (np.abs(y) >= np.float32(2.0 ** -126)) | np.isinf(x))


def mixed_rays(rays, rng):
    """the rays with their smallest direction component replaced by 2^-40 .. 2^-140 of the largest, or by a signed zero"""
    r = np.array(rays, np.float32, copy=True)
    n = len(r)
    d = r[:, 4:7]
    small = np.argmin(np.abs(d), axis=1)
    e = rng.choice([-40, -60, -66, -67, -70, -90, -120, -140], size=n)
    big = np.abs(d).max(1)
    v = np.float32(np.ldexp(np.float64(big), e) * rng.choice([-1.0, 1.0], size=n))
    z = rng.random(n) < 0.2
    v = np.where(z, np.float32(rng.choice([0.0, -0.0], size=n)), v)
    d[np.arange(n), small] = v
    return r


def oracle_trees(pkg, oracle, sc):
    """oracle scenes over the SAH tree, the LBVH (build_mode 1) and the PLOC tree of tests/ploc_reference.py"""
    sah = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    lbvh = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], build_mode=1)
    order = lbvh.tris()["gid"].astype(np.int64)
    nodes, gids, _, _ = spec.build(spec.tri_boxes(sc["meshes"]), order, pkg.NODE_DTYPE)
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))
    pick = inv[gids]
    ploc = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    ploc.set_bvh(nodes, lbvh.tris()[pick], lbvh.shade()[pick])
    return {"sah": sah, "lbvh": lbvh, "ploc": ploc}


def _assert_hits_equal(got, want, what, keys=("inst", "prim")):
    for k in keys:
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, "%s: %s differs on %d of %d rays (first: ray %d)" % (what, k, len(bad), len(got[k]), bad[0])
    for k in ("t", "uv"):
        if k in got and k in want:
            bad = np.flatnonzero((_bits(got[k]) != _bits(want[k])).reshape(len(got["inst"]), -1).any(1))
            assert len(bad) == 0, "%s: %s bits differ on %d rays (first: ray %d)" % (what, k, len(bad), bad[0])


CPU_SCENES = ["quads", "dragon", "sphere-0", "sphere-8192", "box-0", "box-8192", "slivers-0", "slivers-8192"]


# ---------------------------------------------------------------------------------------------------------- CPU: the oracle

def test_short_directions_through_the_quad_stack(pkg, oracle):
    """o = (0.2, 0.1, 0.05), d = s (1, 0.013, -0.007), tmin = 10.5 / s hits quad 11 (prims 20, 21) at t s = 10.8 for every s,
    over the tree as over every triangle; with tmin = 0, and from o = (0.2, 0.5, 0.05), the first quad.  Before the prescale
    the tree walk missed from s = 1e-19 down."""
    S = oracle.OracleScene(quad_stack()["meshes"])
    try:
        for o, tmin_s, prims in (((0.2, 0.1, 0.05), 10.5, (20, 21)), ((0.2, 0.1, 0.05), 0.0, (0, 1)), ((0.2, 0.5, 0.05), 0.0, (0, 1))):
            for s in (1.0, 1e-10, 1e-18, 1e-19, 1e-21, 1e-25, 1e-30, 1e-36, 1e20, 1e36):
                d = np.float32(np.float64([1.0, 0.013, -0.007]) * s)
                rays = pkg.make_rays(o, d, tmin=np.float32(tmin_s / s), tmax=np.inf)
                for brute in (False, True):
                    res = oracle.trace_rays(S, rays, brute_force=brute)
                    what = "o %s s %g brute %d" % (o, s, brute)
                    assert res["inst"][0] == 0 and res["prim"][0] in prims, what
                    np.testing.assert_allclose(np.float64(res["t"][0]) * np.float64(d[0]), 10.8 if tmin_s else 0.8,
                                               rtol=1e-5, err_msg=what)
                    assert oracle.occluded_rays(S, rays, brute_force=brute)["occluded"][0] == 1, what
    finally:
        S.close()


@pytest.mark.parametrize("name", CPU_SCENES)
def test_power_of_two_scale_invariance(pkg, oracle, scenes, dragon, name):
    """a record scaled by 2^k: same inst / prim / u / v bits, occlusion and fetch counts, and t 2^k is the unscaled t, for
    k in [-100, 100] wherever every scaled value stays exact"""
    sc = _scene(name, scenes, dragon)
    S = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    rng = np.random.default_rng(17)
    try:
        rays = base_rays(pkg, sc, rng, 1000)
        rays = np.concatenate([rays, mixed_rays(rays[:300], rng)])
        base = oracle.trace_rays(S, rays)
        bocc = oracle.occluded_rays(S, rays)
        assert (base["inst"] != MISS).sum() > len(rays) // 10
        checked = 0
        for k in POW2:
            rk = scale_rays(rays, k)
            hit = base["inst"] != MISS
            ok = _exact(rays[:, 4:7], k).all(1) & _exact(rays[:, 3], -k) & _exact(rays[:, 7], -k) & (~hit | _exact(base["t"], -k))
            got = oracle.trace_rays(S, rk)
            occ = oracle.occluded_rays(S, rk)
            sel = np.flatnonzero(ok)
            checked += len(sel)
            what = "%s 2^%d" % (name, k)
            back = {"t": np.ldexp(got["t"], k), "uv": got["uv"], "inst": got["inst"], "prim": got["prim"]}
            _assert_hits_equal({q: v[sel] for q, v in back.items()}, {q: base[q][sel] for q in back}, what)
            for q in ("nodes", "tris"):
                assert np.array_equal(got[q][sel], base[q][sel]), "%s: closest-hit %s fetched" % (what, q)
                assert np.array_equal(occ[q][sel], bocc[q][sel]), "%s: occlusion %s fetched" % (what, q)
            assert np.array_equal(occ["occluded"][sel], bocc["occluded"][sel]), what + ": occluded"
        assert checked >= 0.9 * len(POW2) * len(rays)
    finally:
        S.close()


@pytest.mark.parametrize("name", CPU_SCENES)
def test_any_scale_bvh_equals_brute_force(pkg, oracle, scenes, dragon, name):
    """non-power-of-two scales 1e-30 .. 1e30 and mixed magnitudes: the walks of the SAH, LBVH and PLOC trees equal brute force
    bit for bit (t, u, v, inst, prim, occlusion)"""
    sc = _scene(name, scenes, dragon)
    trees = oracle_trees(pkg, oracle, sc)
    rng = np.random.default_rng(23)
    try:
        base = base_rays(pkg, sc, rng, 500)
        sets = [scale_rays(base, s) for s in SCALES] + [scale_rays(mixed_rays(base, rng), s) for s in (1e-25, 1.0, 1e25)]
        rays = np.concatenate(sets)
        bf = oracle.trace_rays(trees["sah"], rays, brute_force=True)
        bocc = oracle.occluded_rays(trees["sah"], rays, brute_force=True)["occluded"]
        assert (bf["inst"] != MISS).sum() > len(rays) // 10
        for tname, S in trees.items():
            _assert_hits_equal(oracle.trace_rays(S, rays), bf, "%s %s" % (name, tname))
            occ = oracle.occluded_rays(S, rays)["occluded"]
            bad = np.flatnonzero(occ != bocc)
            assert len(bad) == 0, "%s %s: occluded differs from brute force on %d rays (first: ray %d)" % (name, tname, len(bad), bad[0])
    finally:
        for S in trees.values():
            S.close()


@pytest.mark.parametrize("name", ["quads", "sphere-0", "sphere-8192", "box-8192", "slivers-0"])
def test_brute_force_against_float64_at_any_scale(pkg, oracle, scenes, dragon, name):
    """brute force of the scaled records against the float64 Moeller-Trumbore of the unscaled ones (tests/path_reference.py
    margins decide which rays are robust): same triangle, and t s within rtol 1e-5 of the float64 t"""
    sc = _scene(name, scenes, dragon)
    S = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    S64 = R.Scene(sc)
    rng = np.random.default_rng(29)
    try:
        base = base_rays(pkg, sc, rng, 250)
        for s in (1e-30, 1e-21, -70, 1.0, 1e21, 1e30):
            bf = oracle.trace_rays(S, scale_rays(base, s), brute_force=True)
            back = np.float64(bf["t"]) * (np.exp2(s) if isinstance(s, int) else s)
            _check_float64(S64, base[:, 0:3], base[:, 4:7], base[:, 3], base[:, 7], bf["inst"], bf["prim"], back,
                           "%s scale %g" % (name, np.exp2(s) if isinstance(s, int) else s), min_robust=0.4)
    finally:
        S.close()


@pytest.mark.parametrize("name", ["quads", "dragon", "sphere-8192", "box-0"])
def test_reference_hit_counts_at_any_scale(pkg, oracle, scenes, dragon, ref, name):
    """tests/point_reference.c counts: the same at every power-of-two scale (exact records), and on closed meshes the parity
    of rays from points away from the surface is the winding number (the box's own inside) at every scale"""
    sc = _scene(name, scenes, dragon)
    tris = _tri_records(pkg, sc["meshes"])
    rng = np.random.default_rng(31)
    rays = base_rays(pkg, sc, rng, 1000)
    rays = np.concatenate([rays, mixed_rays(rays[:300], rng)])
    c0 = ref_count(ref, tris, rays)
    assert c0.sum() > 0
    for k in POW2:
        ok = _exact(rays[:, 4:7], k).all(1) & _exact(rays[:, 3], -k) & _exact(rays[:, 7], -k)
        np.testing.assert_array_equal(ref_count(ref, tris, scale_rays(rays, k))[ok], c0[ok], err_msg="%s 2^%d" % (name, k))
    if name in ("sphere-8192", "box-0"):
        m = sc["meshes"][0]
        V = np.asarray(m["vertices"], np.float64)
        c = V.mean(0)
        rad = np.abs(V - c).max()
        pts = np.float32(c + rng.uniform(-1.5, 1.5, size=(600, 3)) * rad)
        if name.startswith("box"):  # (its faces are not wound consistently: the parity is that of the box itself)
            gap = rad - np.abs(np.float64(pts) - c).max(1)
            away, inside = np.abs(gap) > 1e-3, gap[np.abs(gap) > 1e-3] > 0
        else:
            wn = winding_number(m["vertices"], m["triangles"].astype(np.int64), pts)
            away = np.abs(wn - np.round(wn)) < 1e-3
            inside = np.round(wn[away]) > 0.5
        assert away.sum() > 500 and inside.sum() > 50
        d = _unit(rng.normal(size=(away.sum(), 3)))
        for s in (1e-30, 1e-21, 1.0, 1e21, 1e30):
            r = scale_rays(pkg.make_rays(pts[away], d, tmin=0.0, tmax=np.inf), s)
            np.testing.assert_array_equal((ref_count(ref, tris, r) & 1) == 1, inside, err_msg="%s scale %g: parity" % (name, s))


def range_end_rays(pkg):
    """the ends of the supported direction range and a zero direction just outside it, against the quad x = 0 (y, z in
    [-1, 1]): largest component 2^-149 (t' = 2^-30, t = 2^119), FLT_MAX (t ~ 2^33 / FLT_MAX), zero.  Returns rays and the
    expected t (inf: a miss)"""
    tiny = np.float32(2.0 ** -149)
    o_near = (-(2.0 ** -30), 0.25, 0.125)
    o_far = (-(2.0 ** 33), 0.25, 0.125)
    rows = [(o_near, (tiny, 0.0, 0.0), 2.0 ** 119), (o_near, (tiny, 0.0, -0.0), 2.0 ** 119),
            (o_far, (FLT_MAX, 0.0, 0.0), 2.0 ** 33 / float(FLT_MAX)), (o_far, (FLT_MAX, -0.0, 0.0), 2.0 ** 33 / float(FLT_MAX)),
            (o_near, (0.0, 0.0, 0.0), np.inf), (o_near, (-0.0, 0.0, -0.0), np.inf)]
    rays = np.concatenate([pkg.make_rays(o, np.float32(d), tmin=0.0, tmax=np.inf) for o, d, _ in rows])
    return rays, np.float64([t for _, _, t in rows])


def range_end_scene():
    return {"meshes": [_mesh([(0, -1, -1), (0, 1, -1), (0, 1, 1), (0, -1, 1)], [(0, 1, 2), (0, 2, 3)])], "lights": [], "materials": []}


def _assert_range_ends(res, occ, cnt, want, what):
    for i, tw in enumerate(want):
        if np.isinf(tw):  # just outside the range: a zero direction is a miss, not occluded, no crossing
            assert res["inst"][i] == MISS and res["prim"][i] == MISS and np.isinf(res["t"][i]) and not occ[i] and cnt[i] == 0, \
                "%s ray %d: a zero direction hits nothing" % (what, i)
        else:
            assert res["inst"][i] == 0 and occ[i] and cnt[i] == 1, "%s ray %d: the quad is hit" % (what, i)
            np.testing.assert_allclose(np.float64(res["t"][i]), tw, rtol=1e-6, err_msg="%s ray %d" % (what, i))


def test_range_ends_and_zero_direction(pkg, oracle, ref):
    sc = range_end_scene()
    S = oracle.OracleScene(sc["meshes"])
    rays, want = range_end_rays(pkg)
    cnt = ref_count(ref, _tri_records(pkg, sc["meshes"]), rays)
    try:
        for brute in (False, True):
            res = oracle.trace_rays(S, rays, brute_force=brute)
            _assert_range_ends(res, oracle.occluded_rays(S, rays, brute_force=brute)["occluded"], cnt, want, "brute %d" % brute)
        assert np.ldexp(np.float64(oracle.trace_rays(S, rays)["t"][0]), -119) == 1.0, "t' = 2^-30 scaled back exactly"
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------------------------------- GPU

TREES = {"sah": {"gpu_build": 0}, "lbvh": {"gpu_build": 1, "gpu_builder": 0}, "ploc": {"gpu_build": 1, "gpu_builder": 1}}
GPU_SCALES = (-100, -67, 1e-30, 1e-21, 1.0, 1e21, 1e30, 100)


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    for k in ("gpu_build", "gpu_builder"):
        r.set_option(k, 0)
    r.close()


def gpu_rays(pkg, sc, seed, n=400):
    rng = np.random.default_rng(seed)
    base = base_rays(pkg, sc, rng, n)
    return np.ascontiguousarray(np.concatenate([scale_rays(base, s) for s in GPU_SCALES] + [mixed_rays(base, rng)]))


def _device_queries(renderer, rays):
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    d_t = torch.empty(n, dtype=torch.float32, device="cuda")
    d_uv = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    d_inst = torch.empty(n, dtype=torch.int32, device="cuda")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda")
    d_occ = torch.empty(n, dtype=torch.bool, device="cuda")
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    renderer.trace_rays_device(n, d_rays.data_ptr(), d_t.data_ptr(), d_uv.data_ptr(), d_inst.data_ptr(), d_prim.data_ptr(), stats=True)
    renderer.occluded_device(n, d_rays.data_ptr(), d_occ.data_ptr(), stats=True)
    renderer.count_hits_device(n, d_rays.data_ptr(), d_cnt.data_ptr(), stats=True)
    torch.cuda.synchronize()
    res = {"t": d_t.cpu().numpy(), "uv": d_uv.cpu().numpy(), "inst": d_inst.cpu().numpy().view(np.uint32),
           "prim": d_prim.cpu().numpy().view(np.uint32)}
    return res, d_occ.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)


def check_gpu(pkg, oracle, ref, renderer, sc, rays, bf, bocc, what):
    """the uploaded tree's queries against the oracle's walk of the exported tree (results and fetch counters), brute force
    and the reference counts; host and device forms"""
    nodes, tris, shade = renderer.bvh_export()
    S = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    try:
        S.set_bvh(nodes, tris, shade)
        walk = oracle.trace_rays(S, rays)
        wocc = oracle.occluded_rays(S, rays)
    finally:
        S.close()
    cnt_ref = ref_count(ref, _tri_records(pkg, sc["meshes"]), rays)
    renderer.set_counting(True)
    try:
        got = renderer.trace_rays(rays)
        occ = renderer.occluded(rays)
        cnt = renderer.count_hits(rays)
    finally:
        renderer.set_counting(False)
    st = got["stats"]
    assert (st["nodes_visited"], st["tris_tested"]) == (int(walk["nodes"].sum()), int(walk["tris"].sum())), what + ": fetch counters"
    dev, docc, dcnt = _device_queries(renderer, rays)
    for form, res, o, c in (("host", got, occ, cnt), ("device", dev, docc, dcnt)):
        tag = "%s %s" % (what, form)
        _assert_hits_equal(res, walk, tag + " vs the oracle's walk")
        _assert_hits_equal(res, bf, tag + " vs brute force")
        assert np.array_equal(np.asarray(o, bool), wocc["occluded"] == 1), tag + ": occluded vs the walk"
        assert np.array_equal(np.asarray(o, bool), bocc == 1), tag + ": occluded vs brute force"
        bad = np.flatnonzero(np.asarray(c, np.uint32) != cnt_ref)
        assert len(bad) == 0, "%s: count_hits differs from the reference on %d rays (first: ray %d)" % (tag, len(bad), bad[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quads", "dragon", "sphere-8192", "box-0", "slivers-0"])
def test_gpu_queries_at_any_scale(pkg, oracle, scenes, dragon, ref, renderer, name):
    sc = _scene(name, scenes, dragon)
    rays = gpu_rays(pkg, sc, 41)
    S = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    try:
        bf = oracle.trace_rays(S, rays, brute_force=True)
        bocc = oracle.occluded_rays(S, rays, brute_force=True)["occluded"]
    finally:
        S.close()
    try:
        for tree, opts in TREES.items():
            for k, v in opts.items():
                renderer.set_option(k, v)
            renderer.upload(sc["meshes"], sc["lights"], sc["materials"])
            check_gpu(pkg, oracle, ref, renderer, sc, rays, bf, bocc, "%s %s" % (name, tree))
    finally:
        for k in ("gpu_build", "gpu_builder"):
            renderer.set_option(k, 0)


@pytest.mark.gpu
def test_gpu_moved_dynamic_mesh_at_any_scale(pkg, oracle, scenes, ref, renderer):
    """an icosphere uploaded at the origin and moved to 2^13 by set_mesh_transform + refit: queries at every scale over the
    refitted tree"""
    off, r = 8192.0, 0.0625
    moved = closed_scene(scenes, "sphere", off, r)
    at0 = dict(closed_scene(scenes, "sphere", 0.0, r), lights=moved["lights"])
    renderer.upload(at0["meshes"], at0["lights"], at0["materials"], dynamic=True)
    ax = np.array([1.0, 0.75, -0.5])
    renderer.set_mesh_transform(0, np.float32([[1, 0, 0, off * ax[0]], [0, 1, 0, off * ax[1]], [0, 0, 1, off * ax[2]]]))
    renderer.refit()
    xyz, _ = renderer.mesh_vertices(0)
    assert np.array_equal(_bits(xyz), _bits(moved["meshes"][0]["vertices"]))
    rays = gpu_rays(pkg, moved, 43)
    S = oracle.OracleScene(moved["meshes"], moved["lights"], moved["materials"])
    try:
        bf = oracle.trace_rays(S, rays, brute_force=True)
        bocc = oracle.occluded_rays(S, rays, brute_force=True)["occluded"]
    finally:
        S.close()
    check_gpu(pkg, oracle, ref, renderer, moved, rays, bf, bocc, "dynamic refit")


@pytest.mark.gpu
def test_gpu_range_ends_and_zero_direction(pkg, oracle, ref, renderer):
    sc = range_end_scene()
    rays, want = range_end_rays(pkg)
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"])
    dev, docc, dcnt = _device_queries(renderer, rays)
    for form, res, occ, cnt in (("host", renderer.trace_rays(rays), renderer.occluded(rays), renderer.count_hits(rays)),
                                ("device", dev, docc, dcnt)):
        _assert_range_ends(res, occ, cnt, want, form)
    S = oracle.OracleScene(sc["meshes"])
    try:
        _assert_hits_equal(dev, oracle.trace_rays(S, rays), "range ends vs the oracle")
    finally:
        S.close()
