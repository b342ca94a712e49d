"""Dynamic geometry (crt_update_vertices* / crt_set_mesh_transform / crt_refit / crt_mesh_vertices, include/crt_hip.h): vertices
and per-mesh transforms change after upload and a GPU refit carries them into the uploaded tree.  Every GPU check is exact: records
and trees by bytes, frames and hits by bits, against the CPU oracle of the moved meshes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import shaded_query_checks as sq

SYMBOLS = ("crt_update_vertices", "crt_update_vertices_device", "crt_set_mesh_transform", "crt_refit", "crt_mesh_vertices")
METHODS = ("update_vertices", "set_mesh_transform", "refit", "mesh_vertices")
EINVAL, ESTATE = 1, 5
MODES = (0, 1, 2, 3, 4, 5, 6, 100, 200)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- CPU: the interface exists

def test_binding_and_library_expose_dynamic_geometry(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(L, s), s
    for m in METHODS:
        assert callable(getattr(pkg.Renderer, m, None)), m
    assert L.crt_abi_version() == 1


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    xyz = np.zeros((4, 3), dtype=np.float32)
    m = np.eye(3, 4, dtype=np.float32)
    ms = C.c_double()
    assert L.crt_update_vertices(None, 0, 4, xyz.ctypes.data, None) == EINVAL
    assert L.crt_update_vertices_device(None, 0, 4, xyz.ctypes.data, None) == EINVAL
    assert L.crt_set_mesh_transform(None, 0, m.ctypes.data) == EINVAL
    assert L.crt_set_mesh_transform(None, 0, None) == EINVAL
    assert L.crt_refit(None, C.byref(ms)) == EINVAL and ms.value == 0.0
    assert L.crt_refit(None, None) == EINVAL
    assert L.crt_mesh_vertices(None, 0, xyz.ctypes.data, None) == EINVAL


# ---- helpers (numpy statements of the contract)

def _with_normals(scenes, sc):
    out = []
    for m in sc["meshes"]:
        m = dict(m)
        if m.get("normals") is None:
            m["normals"] = scenes.vertex_normals(m["vertices"], m["triangles"]).astype(np.float32)
        out.append(m)
    return dict(sc, meshes=out)


def _moved(meshes, mesh, xyz, normals=None):
    out = [dict(m) for m in meshes]
    out[mesh]["vertices"] = np.ascontiguousarray(xyz, dtype=np.float32)
    if normals is not None:
        out[mesh]["normals"] = np.ascontiguousarray(normals, dtype=np.float32)
    return out


def _apply(m, v):
    """x' = ((m0*x + m1*y) + m2*z) + m3 in float32, row by row (no fused multiply-add)"""
    m = np.asarray(m, dtype=np.float32).reshape(3, 4)
    v = np.asarray(v, dtype=np.float32)
    out = np.empty_like(v)
    for r in range(3):
        out[:, r] = ((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3]
    return out


def _normal_matrix(m):
    """the inverse transpose of the 3x3 as crt_set_mesh_transform takes it: cofactors and determinant in double (Python floats,
    the same operations in the same order), each quotient rounded to float32 once"""
    M = [float(x) for x in np.asarray(m, dtype=np.float32).reshape(12)]
    a, b, c, d, e, f, g, h, k = M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]
    A, B, Cc = e * k - f * h, -(d * k - f * g), d * h - e * g
    det = a * A + b * B + c * Cc
    cof = [A, B, Cc, -(b * k - c * h), a * k - c * g, -(a * h - b * g), b * f - c * e, -(a * f - c * d), a * e - b * d]
    return np.array([x / det for x in cof], dtype=np.float64).astype(np.float32).reshape(3, 3)


def _apply_normals(m, n):
    a = _normal_matrix(m)
    n = np.asarray(n, dtype=np.float32)
    out = np.empty_like(n)
    for r in range(3):
        out[:, r] = (a[r, 0] * n[:, 0] + a[r, 1] * n[:, 1]) + a[r, 2] * n[:, 2]
    return out


def test_normal_matrix_restatement_is_within_one_ulp_of_numpy_inv():
    """np.linalg.inv is the yardstick, not the statement: for well-conditioned matrices (rotation, anisotropic scale, shear) the
    cofactor / determinant formula lands within one float32 ulp of it"""
    rng = np.random.default_rng(17)
    worst = 0.0
    for _ in range(300):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        shear = np.eye(3)
        shear[0, 1], shear[1, 2] = rng.uniform(-1, 1, 2)
        m = np.concatenate([q @ np.diag(rng.uniform(0.5, 2.0, 3)) @ shear, rng.normal(size=(3, 1))], 1).astype(np.float32)
        got = _normal_matrix(m)
        ref = np.linalg.inv(m.astype(np.float64)[:, :3]).T.astype(np.float32)
        worst = max(worst, float((np.abs(got.astype(np.float64) - ref) / np.spacing(np.maximum(np.abs(got), np.abs(ref)))).max()))
    assert worst <= 1.0, worst


def _numpy_refit(nodes, tris, meshes):
    """binary boxes of the exported tree's shape from the meshes' vertices: leaf = union of its triangles' vertex boxes (the
    point (0, 0, 0) for a triangle with a non-finite coordinate), inner = union of the child's two boxes"""
    V = [np.asarray(m["vertices"], dtype=np.float32) for m in meshes]
    T = [np.asarray(m["triangles"], dtype=np.int64) for m in meshes]
    starts = np.cumsum([0] + [len(t) for t in T])
    lo_g = np.zeros((starts[-1], 3), np.float32)
    hi_g = np.zeros((starts[-1], 3), np.float32)
    for k in range(len(meshes)):
        if len(T[k]):
            p = V[k][T[k]]
            ok = np.isfinite(p).all(axis=(1, 2))[:, None]  # an inert triangle (crt_hip.h) counts as the point (0, 0, 0)
            with np.errstate(invalid="ignore"):
                lo_g[starts[k]:starts[k + 1]] = np.where(ok, p.min(axis=1), 0)
                hi_g[starts[k]:starts[k + 1]] = np.where(ok, p.max(axis=1), 0)
    gid = tris["gid"].astype(np.int64)
    box = {}

    def child_box(ref):
        if ref >= 0:
            return box[ref]
        leaf = ~int(ref)
        first, cnt = leaf >> 3, leaf & 7
        if cnt == 0:
            return None
        g = gid[first:first + cnt]
        return lo_g[g].min(axis=0), hi_g[g].max(axis=0)

    order, k = [0], 0
    while k < len(order):
        for ch in (int(nodes[order[k]]["left"]), int(nodes[order[k]]["right"])):
            if ch >= 0:
                order.append(ch)
        k += 1
    want = np.zeros((len(nodes), 2, 2, 3), np.float32)  # node, child, lo/hi, axis
    for b in reversed(order):
        lb, rb = child_box(int(nodes[b]["left"])), child_box(int(nodes[b]["right"]))
        lb = lb if lb is not None else rb
        rb = rb if rb is not None else lb
        want[b] = (lb, rb)
        box[b] = (np.minimum(lb[0], rb[0]), np.maximum(lb[1], rb[1]))
    return want


def _node_boxes(nodes):
    f = lambda k: nodes[k].astype(np.float32)  # noqa: E731
    lo = np.stack([np.stack([f("lx0"), f("ly0"), f("lz0")], 1), np.stack([f("rx0"), f("ry0"), f("rz0")], 1)], 1)
    hi = np.stack([np.stack([f("lx1"), f("ly1"), f("lz1")], 1), np.stack([f("rx1"), f("ry1"), f("rz1")], 1)], 1)
    return np.stack([lo, hi], 2)


def _by_gid(recs, tris):
    return recs[np.argsort(tris["gid"], kind="stable")]


def _frame(r, w, h):
    f = r.render_frame(w, h)
    return {k: f[k] for k in ("rgba8", "hit_inst", "hit_prim", "hit_t", "rgb")}, f["stats"]


def _assert_frames_equal(a, b, what):
    for k in ("rgba8", "hit_inst", "hit_prim"):
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (what, k))
    for k in ("hit_t", "rgb"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), "%s %s bits" % (what, k)


def _check_frames_vs_oracle(r, O, cam, w, h, modes, counters=True):
    for mode in modes:
        r.change_shading_mode(mode)
        r.set_counting(counters)
        got, st = _frame(r, w, h)
        r.set_counting(False)
        ref = O.render(cam["position"], cam["matrix"], mode, w, h)
        _assert_frames_equal(got, ref, "mode %d" % mode)
        if counters:
            rs = ref["stats"]
            assert (st["rays_primary"], st["rays_shadow"], st["nodes_visited"], st["tris_tested"]) == \
                   (rs["rays_primary"], rs["rays_shadow"], rs["nodes_visited"], rs["tris_tested"]), "mode %d counters" % mode


def _rays(pkg, meshes, n, seed):
    rng = np.random.default_rng(seed)
    allv = np.concatenate([m["vertices"] for m in meshes])
    lo, hi = allv.min(0), allv.max(0)
    ext = hi - lo
    o = (lo - 0.2 * ext + rng.random((n, 3)) * 1.4 * ext).astype(np.float32)
    tgt = (lo + rng.random((n, 3)) * ext).astype(np.float32)
    return pkg.make_rays(o, tgt - o, tmin=0.0, tmax=rng.choice([np.inf, 0.5, 2.0], size=n))


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _upload(r, sc, gpu_build, dynamic=True):
    r.set_option("gpu_build", gpu_build)
    r.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=dynamic)
    r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
    r.set_path_params(2, 2, 99)


def _small_scenes(scenes):
    return [scenes.heightfield(n=48, n_lights=2), scenes.displaced_sphere(n_lat=40, n_lon=40)]


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_build", [0, 1])
def test_identity_update_changes_nothing(pkg, scenes, oracle, renderer, gpu_build):
    w, h = 160, 96
    for sc in _small_scenes(scenes):
        sc = _with_normals(scenes, sc)
        _upload(renderer, sc, gpu_build)
        oracle.set_path_params(2, 2, 99)
        info = renderer.bvh_info()
        nodes, tris, shade = renderer.bvh_export()
        n4, d4 = renderer.bvh_export4()
        n4q, planes = renderer.bvh_export4q(), renderer.bvh_export_planes4q()
        before = {}
        for mode in MODES:
            renderer.change_shading_mode(mode)
            before[mode] = _frame(renderer, w, h)[0]
        for i, m in enumerate(sc["meshes"]):
            renderer.update_vertices(i, m["vertices"], m["normals"])
        assert renderer.refit() > 0.0
        assert renderer.refit() == 0.0  # nothing pending
        nodes2, tris2, shade2 = renderer.bvh_export()
        assert np.array_equal(_node_boxes(nodes2), _node_boxes(nodes))  # by value
        assert np.array_equal(nodes2["left"], nodes["left"]) and np.array_equal(nodes2["right"], nodes["right"])
        assert tris2.tobytes() == tris.tobytes() and shade2.tobytes() == shade.tobytes()
        n42, d42 = renderer.bvh_export4()
        assert n42.tobytes() == n4.tobytes() and d42 == d4
        assert renderer.bvh_export4q().tobytes() == n4q.tobytes()
        assert renderer.bvh_export_planes4q().tobytes() == planes.tobytes()
        assert renderer.bvh_info() == info
        for mode in MODES:
            renderer.change_shading_mode(mode)
            _assert_frames_equal(_frame(renderer, w, h)[0], before[mode], "mode %d after the identity refit" % mode)
        oracle.set_path_params(4, 3, 1234)


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_build", [0, 1])
def test_deformation_matches_the_oracle(pkg, scenes, oracle, renderer, gpu_build):
    w, h = 160, 96
    rng = np.random.default_rng(2024 + gpu_build)
    oracle.set_path_params(2, 2, 99)
    try:
        for si, sc in enumerate(_small_scenes(scenes)):
            sc = _with_normals(scenes, sc)
            _upload(renderer, sc, gpu_build)
            cam = sc["camera"]
            n4_before, d4_before = renderer.bvh_export4()
            v = sc["meshes"][1]["vertices"].copy()
            if si == 0:  # heightfield: seeded height displacement, spiky
                v[:, 1] += rng.normal(0.0, 1.5, size=len(v)).astype(np.float32)
            else:        # displaced sphere: seeded radial displacement
                v *= rng.uniform(0.6, 1.5, size=(len(v), 1)).astype(np.float32)
            nrm = scenes.vertex_normals(v, sc["meshes"][1]["triangles"]).astype(np.float32)
            renderer.update_vertices(1, v, nrm)
            moved = _moved(sc["meshes"], 1, v, nrm)
            nodes, tris, shade = renderer.bvh_export()  # (the refit runs here)
            n4, d4 = renderer.bvh_export4()
            assert len(n4) != len(n4_before) or d4 != d4_before, "the deformation must change the wide tree's size or depth"
            fresh = oracle.OracleScene(moved, sc["lights"], sc["materials"])
            assert _by_gid(tris, tris).tobytes() == _by_gid(fresh.tris(), fresh.tris()).tobytes()
            assert _by_gid(shade, tris).tobytes() == _by_gid(fresh.shade(), fresh.tris()).tobytes()
            assert np.array_equal(_node_boxes(nodes), _numpy_refit(nodes, tris, moved))
            S = oracle.OracleScene(moved, sc["lights"], sc["materials"])
            S.set_bvh(nodes, tris, shade)
            assert n4.tobytes() == S.nodes4().tobytes() and d4 == S.depth4
            assert renderer.bvh_export4q().tobytes() == S.nodes4q().tobytes()
            _check_frames_vs_oracle(renderer, S, cam, w, h, MODES)
            # the same frames through camera_rays, shade_rays, path_rays and frame_guides
            sq.frame_records_equal_frames(renderer, {m: S.render(cam["position"], cam["matrix"], m, w, h) for m in (3, 100, 200)}, w, h,
                                          (2, 2, 99), "deformed scene %d, gpu_build %d" % (si, gpu_build), scene=dict(sc, meshes=moved),
                                          world={"oracle": oracle, "camera": (cam["position"], cam["matrix"]), "lights": sc["lights"], "O": S,
                                                 "path_held": (2, 2, 99)})
            for mode in (3, 100):  # hits do not depend on the tree
                renderer.change_shading_mode(mode)
                got = _frame(renderer, w, h)[0]
                ref = fresh.render(cam["position"], cam["matrix"], mode, w, h)
                for k in ("hit_inst", "hit_prim", "rgba8"):
                    np.testing.assert_array_equal(got[k], ref[k], err_msg="vs a fresh build, mode %d %s" % (mode, k))
            # ray queries: the refitted tree against a fresh upload of the moved meshes, and the oracle's occlusion
            rays = _rays(pkg, moved, 4000, seed=si)
            q = renderer.trace_rays(rays)
            occ = renderer.occluded(rays)
            r2 = pkg.Renderer(0)
            try:
                r2.set_option("gpu_build", gpu_build)
                r2.upload(moved, sc["lights"], sc["materials"])
                q2 = r2.trace_rays(rays)
                np.testing.assert_array_equal(occ, r2.occluded(rays))
            finally:
                r2.close()
            for k in ("inst", "prim"):
                np.testing.assert_array_equal(q[k], q2[k], err_msg=k)
            assert np.array_equal(_bits(q["t"]), _bits(q2["t"])) and np.array_equal(_bits(q["uv"]), _bits(q2["uv"]))
            assert (q["inst"] != 0xFFFFFFFF).sum() > 1000
            for i in range(0, len(rays), 40):
                ray = rays[i]
                assert bool(occ[i]) == bool(oracle.occluded(S, ray[0:3], ray[4:7], ray[3], ray[7])), "ray %d" % i
    finally:
        oracle.set_path_params(4, 3, 1234)


def _shaded_records_vs_oracle(renderer, oracle, S, sc, moved, what, w=48, h=32):
    """a small frame of the moved scene through camera_rays, shade_rays (modes 3, 100, 120 and 150), path_rays and frame_guides
    against the oracle over the exported tree S (tests/shaded_query_checks.py); mode 120's bounded reach follows the root box
    as exported now"""
    cam = sc["camera"]
    oracle.set_path_params(2, 2, 99)
    try:
        frames = {m: S.render(cam["position"], cam["matrix"], m, w, h) for m in (3, 100, 200)}
    finally:
        oracle.set_path_params(4, 3, 1234)
    sq.frame_records_equal_frames(renderer, frames, w, h, (2, 2, 99), what, scene=dict(sc, meshes=moved),
                                  world={"oracle": oracle, "camera": (cam["position"], cam["matrix"]), "lights": sc["lights"], "O": S})


@pytest.mark.gpu
def test_transforms_on_the_dragon(pkg, scenes, oracle, renderer, dragon):
    sc = _with_normals(scenes, dragon)
    w, h = 192, 108
    _upload(renderer, sc, 0)
    cam = sc["camera"]
    a = np.deg2rad(30.0)
    rot = np.float32([[np.cos(a), 0.0, np.sin(a), 1.5], [0.0, 1.0, 0.0, -0.75], [-np.sin(a), 0.0, np.cos(a), 2.0]])
    scale = np.float32([[1.5, 0.0, 0.0, 0.0], [0.0, 0.5, 0.0, 0.0], [0.0, 0.0, 2.0, 0.0]])
    dragon_mesh = int(np.argmax([len(m["triangles"]) for m in sc["meshes"]]))
    ground = 1 - dragon_mesh
    renderer.set_mesh_transform(dragon_mesh, rot)
    renderer.set_mesh_transform(ground, np.vstack([scale, np.float32([[0, 0, 0, 1]])]))  # 4x4 form
    moved = [dict(m) for m in sc["meshes"]]
    for i, m in ((dragon_mesh, rot), (ground, scale)):
        xyz, nrm = renderer.mesh_vertices(i)
        want_v, want_n = _apply(m, sc["meshes"][i]["vertices"]), _apply_normals(m, sc["meshes"][i]["normals"])
        assert np.array_equal(_bits(xyz), _bits(want_v)), "mesh %d vertices" % i
        assert np.array_equal(_bits(nrm), _bits(want_n)), "mesh %d normals" % i
        moved[i] = dict(moved[i], vertices=want_v, normals=want_n)
    nodes, tris, shade = renderer.bvh_export()
    S = oracle.OracleScene(moved, sc["lights"], sc["materials"])
    S.set_bvh(nodes, tris, shade)
    _check_frames_vs_oracle(renderer, S, cam, w, h, (3, 100))
    _shaded_records_vs_oracle(renderer, oracle, S, sc, moved, "the dragon turned, the ground scaled")
    fresh = oracle.OracleScene(moved, sc["lights"], sc["materials"])
    renderer.change_shading_mode(100)
    got = _frame(renderer, w, h)[0]
    ref = fresh.render(cam["position"], cam["matrix"], 100, w, h)
    for k in ("hit_inst", "hit_prim", "rgba8"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)

    # out of the original root box: split packets cut rays against the refitted root box
    lo0 = renderer.bvh_export4q()[0]["lo"].copy()
    far = np.float32([[1, 0, 0, 0], [0, 1, 0, 4.0], [0, 0, 1, -45.0]])
    renderer.set_mesh_transform(dragon_mesh, far)
    renderer.set_mesh_transform(ground, None)
    moved = [dict(m) for m in sc["meshes"]]
    moved[dragon_mesh] = dict(moved[dragon_mesh], vertices=_apply(far, sc["meshes"][dragon_mesh]["vertices"]),
                              normals=_apply_normals(far, sc["meshes"][dragon_mesh]["normals"]))
    xyz, _ = renderer.mesh_vertices(dragon_mesh)
    assert np.array_equal(_bits(xyz), _bits(moved[dragon_mesh]["vertices"]))
    assert not np.array_equal(renderer.bvh_export4q()[0]["lo"], lo0)
    S = oracle.OracleScene(moved, sc["lights"], sc["materials"])
    S.set_bvh(*renderer.bvh_export())
    _shaded_records_vs_oracle(renderer, oracle, S, sc, moved, "the dragon moved out of the root box")
    import torch
    W, H, n_ranks = 320, 180, 4
    cam_far = cam
    fresh = oracle.OracleScene(moved, sc["lights"], sc["materials"])
    for mode in (3, 100):
        renderer.change_shading_mode(mode)
        slots = pkg.tile_slots(W, H, n_ranks)
        staged = []
        for rank in range(n_ranks):
            buf = torch.zeros(slots * 256, dtype=torch.int32, device="cuda")
            renderer.render_tiles_device(W, H, rank, n_ranks, buf.data_ptr())
            renderer.synchronize()
            staged.append(buf.cpu().numpy().view(np.uint32))
        frame = pkg.untile_host(np.stack(staged), W, H, n_ranks)
        ref = fresh.render(cam_far["position"], cam_far["matrix"], mode, W, H)
        assert (ref["hit_inst"] == dragon_mesh).sum() > 100
        np.testing.assert_array_equal(frame, ref["rgba8"].view(np.uint32).reshape(H, W), err_msg="tiles, mode %d" % mode)


@pytest.mark.gpu
def test_an_update_restarts_accumulation(pkg, scenes, oracle, renderer):
    sc = scenes.displaced_sphere(n_lat=32, n_lon=32)
    w, h = 96, 64
    _upload(renderer, sc, 0)
    renderer.change_shading_mode(200)
    renderer.set_accumulation(64)
    try:
        renderer.set_path_params(2, 2, 5)
        renderer.render_frame(w, h)
        renderer.render_frame(w, h)
        assert renderer.accumulated_samples() == 4
        v = sc["meshes"][1]["vertices"] * np.float32(1.1)
        renderer.update_vertices(1, v)
        assert renderer.accumulated_samples() == 0
        for _ in range(3):
            got = renderer.render_frame(w, h)
        assert renderer.accumulated_samples() == 6
        r2 = pkg.Renderer(0)
        try:
            r2.upload(_moved(sc["meshes"], 1, v), sc["lights"], sc["materials"])
            r2.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
            r2.change_shading_mode(200)
            r2.set_accumulation(64)
            r2.set_path_params(6, 2, 5)
            one = r2.render_frame(w, h)
        finally:
            r2.close()
        np.testing.assert_array_equal(got["rgba8"], one["rgba8"])
        assert np.array_equal(_bits(got["rgb"]), _bits(one["rgb"]))
    finally:
        renderer.set_accumulation(0)
        renderer.set_path_params(4, 3, 1234)


@pytest.mark.gpu
def test_state_and_argument_errors(pkg, scenes, renderer):
    L = pkg.lib()
    sc = _with_normals(scenes, scenes.cornell_box())
    m0 = sc["meshes"][0]
    _upload(renderer, sc, 0, dynamic=False)
    assert L.crt_update_vertices(renderer.h, 0, len(m0["vertices"]), m0["vertices"].ctypes.data, None) == ESTATE
    assert L.crt_set_mesh_transform(renderer.h, 0, None) == ESTATE
    assert L.crt_refit(renderer.h, None) == ESTATE
    xyz = np.zeros((len(m0["vertices"]), 3), np.float32)
    assert L.crt_mesh_vertices(renderer.h, 0, xyz.ctypes.data, None) == ESTATE

    nn = _with_normals(scenes, scenes.cornell_box())
    meshes = [dict(m) for m in nn["meshes"]]
    meshes[1] = dict(meshes[1], normals=None)  # one mesh without normals
    renderer.set_option("gpu_build", 0)
    renderer.upload(meshes, sc["lights"], sc["materials"], dynamic=True)
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
    renderer.change_shading_mode(100)
    before = _frame(renderer, 128, 128)[0]
    v0 = np.ascontiguousarray(meshes[0]["vertices"], np.float32)
    v1 = np.ascontiguousarray(meshes[1]["vertices"], np.float32)
    n0 = np.ascontiguousarray(meshes[0]["normals"], np.float32)
    shift = np.float32([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 0]])
    bad_inf = shift.copy()
    bad_inf[1, 3] = np.inf
    bad_nan = shift.copy()
    bad_nan[0, 0] = np.nan
    singular = np.float32([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0]])
    n_meshes = len(meshes)
    cases = [
        L.crt_update_vertices(renderer.h, n_meshes, len(v0), v0.ctypes.data, None),          # bad mesh index
        L.crt_update_vertices(renderer.h, 0, len(v0) - 1, v0.ctypes.data, None),             # other vertex count
        L.crt_update_vertices(renderer.h, 0, len(v0), None, None),                           # xyz NULL
        L.crt_update_vertices(renderer.h, 1, len(v1), v1.ctypes.data, v1.ctypes.data),       # normals for a mesh without
        L.crt_update_vertices_device(renderer.h, n_meshes, len(v0), None, None),
        L.crt_set_mesh_transform(renderer.h, n_meshes, shift.ctypes.data),
        L.crt_set_mesh_transform(renderer.h, 0, bad_inf.ctypes.data),                        # non-finite
        L.crt_set_mesh_transform(renderer.h, 0, bad_nan.ctypes.data),
        L.crt_set_mesh_transform(renderer.h, 0, singular.ctypes.data),                       # singular, mesh has normals
        L.crt_mesh_vertices(renderer.h, n_meshes, v0.ctypes.data, None),
        L.crt_mesh_vertices(renderer.h, 1, v1.copy().ctypes.data, v1.copy().ctypes.data),    # normals of a mesh without
    ]
    assert cases == [EINVAL] * len(cases)
    assert renderer.refit() == 0.0  # nothing was staged
    _assert_frames_equal(_frame(renderer, 128, 128)[0], before, "after failed calls")
    # a singular 3x3 is accepted on a mesh without normals
    renderer.set_mesh_transform(1, singular)
    assert renderer.refit() > 0.0
    renderer.set_mesh_transform(1, None)
    renderer.update_vertices(0, v0 + np.float32(0.01), n0)
    renderer.refit()
    assert not np.array_equal(_frame(renderer, 128, 128)[0]["rgba8"], before["rgba8"])
    # a re-upload after a refit replaces the scene: the frame of the original meshes, as a plain upload renders it
    renderer.upload(meshes, sc["lights"], sc["materials"], dynamic=True)
    _assert_frames_equal(_frame(renderer, 128, 128)[0], before, "re-upload after a refit")
    renderer.upload(meshes, sc["lights"], sc["materials"], dynamic=False)
    _assert_frames_equal(_frame(renderer, 128, 128)[0], before, "plain upload")


@pytest.mark.gpu
def test_device_update_equals_host_update(pkg, scenes, renderer):
    import torch
    sc = _with_normals(scenes, scenes.displaced_sphere(n_lat=32, n_lon=32))
    rng = np.random.default_rng(11)
    v = sc["meshes"][1]["vertices"] * rng.uniform(0.8, 1.2, size=(len(sc["meshes"][1]["vertices"]), 1)).astype(np.float32)
    n = scenes.vertex_normals(v, sc["meshes"][1]["triangles"]).astype(np.float32)
    out = []
    for device in (False, True):
        _upload(renderer, sc, 1)
        renderer.change_shading_mode(100)
        if device:
            renderer.update_vertices(1, torch.from_numpy(v).cuda(), torch.from_numpy(n).cuda())
        else:
            renderer.update_vertices(1, v, n)
        f = _frame(renderer, 128, 96)[0]
        out.append((f, renderer.bvh_export(), renderer.mesh_vertices(1)))
    _assert_frames_equal(out[0][0], out[1][0], "device vs host update")
    for a, b in zip(out[0][1], out[1][1]):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(_bits(out[0][2][0]), _bits(v)) and np.array_equal(_bits(out[1][2][1]), _bits(n))


@pytest.mark.gpu
def test_cpp_layer(pkg, scenes, renderer, tmp_path):
    """crt::Renderer::setDynamicGeometry / setMeshTransform / updateMeshVertices from a small C++ program: a moved mesh is hit
    where it moved to"""
    exe = str(tmp_path / "dynamic_cpp")
    csrc = os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + csrc,
                           "-o", exe, os.path.join(ROOT, "tests", "dynamic_cpp.cpp"), "-L" + os.path.dirname(pkg.LIB_PATH), "-lcrt_hip",
                           "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH), "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib")], timeout=300)
    sc = scenes.cornell_box()
    scene = pkg.Scene.from_arrays(sc)
    path = str(tmp_path / "cornell.crtbin")
    scene.save(path)
    mesh = len(sc["meshes"]) - 1
    t = np.float32([0.25, -0.5, 0.75])
    moved_v = sc["meshes"][mesh]["vertices"] + t
    cen = moved_v.mean(axis=0)
    rng = np.random.default_rng(5)
    o = (cen + rng.normal(size=(512, 3)) * 0.05 + np.float32([0.0, 0.0, 30.0])).astype(np.float32)
    rays = pkg.make_rays(o, cen - o, tmin=0.0, tmax=np.inf)
    rays.tofile(str(tmp_path / "rays.bin"))
    out = str(tmp_path / "hits.bin")
    subprocess.check_call([exe, path, str(tmp_path / "rays.bin"), out, str(mesh)] + [repr(float(x)) for x in t], timeout=120)
    hit = np.fromfile(out, dtype=np.uint32).reshape(-1, 5)
    m = [dict(x) for x in scene.meshes()]
    m[mesh] = dict(m[mesh], vertices=(m[mesh]["vertices"] + t).astype(np.float32))
    renderer.set_option("gpu_build", 0)
    renderer.upload(m, sc["lights"], sc["materials"])
    ref = renderer.trace_rays(rays)
    assert np.array_equal(hit[:, 0], _bits(ref["t"])) and np.array_equal(hit[:, 1:3], _bits(ref["uv"]))
    assert np.array_equal(hit[:, 3], ref["inst"]) and np.array_equal(hit[:, 4], ref["prim"])
    assert (ref["inst"] == mesh).sum() > 100
    scene.close()
