"""GPU rebuild of a dynamic scene (crt_rebuild) and the PLOC builder (option "gpu_builder" = 1), include/crt_hip.h.  PLOC trees are
checked byte for byte against tests/ploc_reference.py; a rebuild against a fresh "gpu_build" upload of the moved meshes; frames and
ray queries against the CPU oracle over the same tree."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ploc_reference as spec  # noqa: E402
import shaded_query_checks as sq  # noqa: E402

EINVAL, ESTATE = 1, 5
MODES = (0, 1, 2, 3, 4, 5, 6, 100, 200)
LBVH, PLOC = 0, 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _with_normals(scenes, sc):
    out = []
    for m in sc["meshes"]:
        m = dict(m)
        if m.get("normals") is None:
            m["normals"] = scenes.vertex_normals(m["vertices"], m["triangles"]).astype(np.float32)
        out.append(m)
    return dict(sc, meshes=out)


def _apply(m, v):
    """x' = ((m0*x + m1*y) + m2*z) + m3 in float32, row by row (no fused multiply-add): the transform of a dynamic mesh"""
    m = np.asarray(m, dtype=np.float32).reshape(3, 4)
    v = np.asarray(v, dtype=np.float32)
    out = np.empty_like(v)
    for r in range(3):
        out[:, r] = ((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3]
    return out


def _apply_normals(m, n):
    """normals by the inverse transpose of the 3x3 (double, rounded to float once), not renormalised"""
    a = np.linalg.inv(np.asarray(m, dtype=np.float64).reshape(3, 4)[:, :3]).T.astype(np.float32)
    n = np.asarray(n, dtype=np.float32)
    out = np.empty_like(n)
    for r in range(3):
        out[:, r] = (a[r, 0] * n[:, 0] + a[r, 1] * n[:, 1]) + a[r, 2] * n[:, 2]
    return out


def _rot(deg, axis=1, t=(0.0, 0.0, 0.0)):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    R = np.eye(3)
    i, j = [k for k in range(3) if k != axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return np.concatenate([R, np.asarray(t, dtype=np.float64).reshape(3, 1)], 1).astype(np.float32)


def _chain(n=80, ratio=1.5):
    """unit triangles at geometrically growing spacing: a PLOC tree about n deep, where the depth rule must fire"""
    f = np.float32
    tri = f([(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    xs = np.cumsum(ratio ** np.arange(n))
    v = np.concatenate([tri + f([x, 0, -3]) for x in xs]).astype(f)
    return {"meshes": [{"vertices": v, "triangles": np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)}], "lights": [], "materials": [],
            "camera": {"position": f([2, 0.3, 0]), "matrix": np.eye(3, dtype=f)}}


def _soup(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-5, 5, (n, 1, 3)).astype(np.float32)
    v = (c + rng.uniform(-0.4, 0.4, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    return [{"vertices": v, "triangles": np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)}]


def _expected(pkg, oracle, meshes, lights=(), materials=(), textures=()):
    """what a PLOC build must give: (nodes, tris, shade, uvs or None, max_depth).  The initial order and the records come from the
    oracle's LBVH (build_mode=1): its leaf order is the Morton order, and a record depends on its triangle only."""
    O = oracle.OracleScene(meshes, lights, materials, build_mode=1, textures=list(textures))
    order = O.tris()["gid"].astype(np.int64)
    nodes, gids, depth, _ = spec.build(spec.tri_boxes(meshes), order, pkg.NODE_DTYPE)
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))
    pick = inv[gids]  # LBVH leaf position of every triangle in PLOC leaf order
    uvs = O.uvs()
    return nodes, O.tris()[pick], O.shade()[pick], (uvs[pick] if uvs is not None else None), depth


# ---- CPU: the interface exists, and the numpy statement holds its own invariants

def test_binding_and_library_expose_rebuild(pkg):
    L = pkg.lib()
    assert "crt_rebuild" in pkg.ABI_SYMBOLS and hasattr(L, "crt_rebuild")
    assert callable(getattr(pkg.Renderer, "rebuild", None))
    assert L.crt_abi_version() == 1


def test_null_context_is_einval(pkg):
    L = pkg.lib()
    ms = C.c_double(7.0)
    assert L.crt_rebuild(None, C.byref(ms)) == EINVAL and ms.value == 0.0
    assert L.crt_rebuild(None, None) == EINVAL
    assert L.crt_set_option(None, b"gpu_builder", 1) == EINVAL


def _check_tree(nodes, gids, boxes_by_gid, n):
    """every triangle exactly once; leaf boxes = folds of their triangles; inner boxes = unions of their children's boxes"""
    assert np.array_equal(np.sort(gids), np.arange(n))
    cb = spec.child_boxes(nodes)
    covered = np.zeros(n, np.int64)
    for b in range(len(nodes)):
        for side, ref in enumerate((int(nodes[b]["left"]), int(nodes[b]["right"]))):
            if ref >= 0:
                assert ref > b  # pre-order
                u = spec.union(cb[ref, 0], cb[ref, 1])
                assert _bits(cb[b, side]).tolist() == _bits(u).tolist(), "node %d side %d" % (b, side)
            else:
                first, cnt = (~ref) >> 3, (~ref) & 7
                assert 1 <= cnt <= spec.LEAF_MAX
                covered[first:first + cnt] += 1
                f = spec._fold(boxes_by_gid[gids[first:first + cnt]])
                assert _bits(cb[b, side]).tolist() == _bits(f).tolist()
    assert (covered == 1).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_spec_trees_are_complete_and_exact(pkg, oracle, seed):
    meshes = _soup(300 + 97 * seed, seed)
    n = len(meshes[0]["triangles"])
    order = oracle.OracleScene(meshes, build_mode=1).tris()["gid"].astype(np.int64)
    boxes = spec.tri_boxes(meshes)
    nodes, gids, depth, T = spec.build(boxes, order, pkg.NODE_DTYPE)
    _check_tree(nodes, gids, boxes, n)
    assert depth == spec.max_depth(nodes) <= 32
    assert len(nodes) == T["size"][T["root"]]
    # the leaf rule closed some nodes of 2..4 triangles, and kept others open
    merged = np.arange(n, 2 * n - 1)
    small = merged[T["count"][merged] <= 4]
    assert T["leaf"][small].any() and (~T["leaf"][small]).any()


def test_spec_merges_follow_the_mutual_nearest_neighbour_rule(pkg):
    """brute force, one pair at a time in plain Python floats rounded to float32, on a tiny soup"""
    meshes = _soup(40, 9)
    boxes = spec.tri_boxes(meshes)
    order = np.random.default_rng(3).permutation(40)
    T = spec.cluster(boxes[order])
    cl = [tuple(float(x) for x in b) for b in boxes[order]]
    ids = list(range(40))

    def d(a, b):
        lo = [np.float32(a[k] if a[k] < b[k] else b[k]) for k in range(3)]
        hi = [np.float32(a[3 + k] if a[3 + k] > b[3 + k] else b[3 + k]) for k in range(3)]
        dx, dy, dz = (np.float32(hi[k] - lo[k]) for k in range(3))
        return np.float32(np.float32(np.float32(dx * dy) + np.float32(dy * dz)) + np.float32(dz * dx))

    for mi, mj, new in T["history"]:
        m = len(ids)
        nn = []
        for i in range(m):
            best, bj = None, None
            for j in range(max(0, i - 16), min(m, i + 17)):
                if j != i and (bj is None or d(cl[i], cl[j]) < best):
                    best, bj = d(cl[i], cl[j]), j
            nn.append(bj)
        pairs = [(i, nn[i]) for i in range(m) if nn[nn[i]] == i and i < nn[i]]
        assert [p[0] for p in pairs] == mi.tolist() and [p[1] for p in pairs] == mj.tolist()
        for k, (i, j) in enumerate(pairs):
            assert T["left"][new[k]] == ids[i] and T["right"][new[k]] == ids[j]
            ids[i] = int(new[k])
            cl[i] = tuple(float(x) for x in spec.union(np.float32(cl[i]), np.float32(cl[j])))
        drop = {j for _, j in pairs}
        ids = [x for p, x in enumerate(ids) if p not in drop]
        cl = [x for p, x in enumerate(cl) if p not in drop]
    assert len(ids) == 1 and ids[0] == T["root"]


def test_spec_depth_rule_bounds_the_geometric_chain(pkg, oracle):
    sc = _chain()
    n = len(sc["meshes"][0]["triangles"])
    order = oracle.OracleScene(sc["meshes"], build_mode=1).tris()["gid"].astype(np.int64)
    boxes = spec.tri_boxes(sc["meshes"])
    nodes, gids, depth, T = spec.build(boxes, order, pkg.NODE_DTYPE)
    assert T["height"][T["root"]] > 32  # PLOC alone would put leaves below depth 32: the rule fires
    assert depth <= 32 and depth == spec.max_depth(nodes)
    _check_tree(nodes, gids, boxes, n)


def test_spec_small_scenes_use_one_leaf(pkg):
    for n in (1, 2, 4):
        meshes = _soup(n, n)
        nodes, gids, depth, _ = spec.build(spec.tri_boxes(meshes), np.arange(n), pkg.NODE_DTYPE)
        assert len(nodes) == 1 and nodes[0]["left"] == ~n and nodes[0]["right"] == ~0 and depth == 1


# ---- GPU

@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _spec_cases(scenes, dragon):
    f = np.float32
    tri = f([(0, 0, -3), (1, 0, -3), (0, 1, -3)])
    small = [{"meshes": [{"vertices": np.concatenate([tri + f([1.5 * i, 0, 0]) for i in range(n)]),
                          "triangles": np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)}], "lights": [], "materials": [],
              "camera": {"position": f([2, 0.3, 0]), "matrix": scenes.IDENTITY}} for n in (1, 2, 4, 5, 9)]
    rng = np.random.default_rng(5)
    same = {"meshes": [{"vertices": np.tile(tri, (5000, 1)), "triangles": np.arange(15000, dtype=np.uint32).reshape(-1, 3)}], "lights": [],
            "materials": [], "camera": {"position": f([0.3, 0.3, 0]), "matrix": scenes.IDENTITY}}
    clump = np.concatenate([tri + (f([0, 0, 0]) if i % 3 else f([40, 0, 0])) + f(rng.uniform(0, 1e-3, 3)) for i in range(6151)])
    clumps = {"meshes": [{"vertices": clump.astype(np.float32), "triangles": np.arange(3 * 6151, dtype=np.uint32).reshape(-1, 3)}], "lights": [],
              "materials": [], "camera": {"position": f([0.3, 0.3, 0]), "matrix": scenes.IDENTITY}}
    return [(s, 64, 64, (3,)) for s in small] + [(same, 48, 48, (3,)), (clumps, 48, 48, (3,)), (_chain(), 64, 64, (3,))] + [
        (scenes.cornell_box(), 128, 128, MODES),
        (_with_normals(scenes, dragon), 320, 180, MODES),
        (scenes.displaced_sphere(), 320, 180, (100,)),
    ]


def _check_against_spec(pkg, oracle, r, sc, what):
    nodes, tris, shade = r.bvh_export()
    want = _expected(pkg, oracle, sc["meshes"], sc["lights"], sc["materials"], sc.get("textures", ()))
    assert nodes.tobytes() == want[0].tobytes(), "%s: PLOC binary nodes differ" % what
    assert tris.tobytes() == want[1].tobytes() and shade.tobytes() == want[2].tobytes(), "%s: records differ" % what
    assert r.bvh_info()["max_depth"] == want[4] <= 32
    S = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    S.set_bvh(nodes, tris, shade)
    n4, d4 = r.bvh_export4()
    assert n4.tobytes() == S.nodes4().tobytes() and d4 == S.depth4, what
    assert r.bvh_export4q().tobytes() == S.nodes4q().tobytes(), what
    return S, want


@pytest.mark.gpu
def test_ploc_upload_matches_its_spec_and_renders_identically(pkg, oracle, scenes, dragon, renderer):
    r = renderer
    r.set_option("gpu_build", 1)
    r.set_option("gpu_builder", PLOC)
    try:
        for sc, w, h, modes in _spec_cases(scenes, dragon):
            n_tris = sum(len(m["triangles"]) for m in sc["meshes"])
            r.upload(sc["meshes"], sc["lights"], sc["materials"])
            assert r.build_stats()["device_build_ms"] > 0 or n_tris <= 4
            S, _ = _check_against_spec(pkg, oracle, r, sc, "%d tris" % n_tris)
            cam = sc["camera"]
            r.set_camera(cam["position"], cam["matrix"])
            sah = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
            for mode in modes:
                r.change_shading_mode(mode)
                r.set_counting(True)
                got = r.render_frame(w, h)
                r.set_counting(False)
                ref = S.render(cam["position"], cam["matrix"], mode, w, h)
                for k in ("hit_inst", "hit_prim", "rgba8"):
                    np.testing.assert_array_equal(got[k], ref[k], err_msg="mode %d %s" % (mode, k))
                assert np.array_equal(_bits(got["hit_t"]), _bits(ref["hit_t"])) and np.array_equal(got["rgb"], ref["rgb"], equal_nan=True)
                assert (got["stats"]["nodes_visited"], got["stats"]["tris_tested"]) == (ref["stats"]["nodes_visited"], ref["stats"]["tris_tested"])
                if mode != 200:
                    s = sah.render(cam["position"], cam["matrix"], mode, w, h)
                    for k in ("hit_inst", "hit_prim", "hit_t", "rgba8"):
                        np.testing.assert_array_equal(got[k], s[k], err_msg="vs SAH tree, mode %d %s" % (mode, k))
            if n_tris > 1000:  # ray queries over the same tree
                rays = _rays(pkg, sc["meshes"], 2000, seed=n_tris)
                occ = r.occluded(rays)
                for i in range(0, len(rays), 20):
                    ray = rays[i]
                    assert bool(occ[i]) == bool(oracle.occluded(S, ray[0:3], ray[4:7], ray[3], ray[7])), "ray %d" % i
        # uvs and textures through the device gather
        sc = scenes.textured_cornell()
        r.upload(sc["meshes"], sc["lights"], sc["materials"], sc["textures"])
        _, want = _check_against_spec(pkg, oracle, r, sc, "textured cornell")
        assert r.bvh_export_uv().tobytes() == want[3].tobytes()
        cam = sc["camera"]
        r.set_camera(cam["position"], cam["matrix"])
        r.change_shading_mode(100)
        got = r.render_frame(160, 120)
        ref = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], textures=sc["textures"]).render(cam["position"], cam["matrix"], 100, 160, 120)
        np.testing.assert_array_equal(got["rgba8"], ref["rgba8"])
    finally:
        r.set_option("gpu_builder", LBVH)
        r.set_option("gpu_build", 0)


def _rays(pkg, meshes, n, seed):
    rng = np.random.default_rng(seed)
    allv = np.concatenate([m["vertices"] for m in meshes])
    lo, hi = allv.min(0), allv.max(0)
    ext = hi - lo
    o = (lo - 0.2 * ext + rng.random((n, 3)) * 1.4 * ext).astype(np.float32)
    tgt = (lo + rng.random((n, 3)) * ext).astype(np.float32)
    return pkg.make_rays(o, tgt - o, tmin=0.0, tmax=rng.choice([np.inf, 0.5, 2.0], size=n))


@pytest.mark.gpu
def test_ploc_tree_is_no_worse_than_the_lbvh(pkg, scenes, dragon, renderer):
    r = renderer
    r.set_option("gpu_build", 1)
    try:
        for sc in (dragon, scenes.heightfield(), scenes.icosphere_soup()):
            cost = {}
            for b in (LBVH, PLOC):
                r.set_option("gpu_builder", b)
                r.upload(sc["meshes"], sc["lights"], sc["materials"])
                cost[b] = spec.sah_cost(r.bvh_export()[0])
                assert r.bvh_info()["max_depth"] <= 32
            assert cost[PLOC] <= cost[LBVH], cost
    finally:
        r.set_option("gpu_builder", LBVH)
        r.set_option("gpu_build", 0)


def _export(r):
    nodes, tris, shade = r.bvh_export()
    uv = r.bvh_export_uv()
    n4, d4 = r.bvh_export4()
    return [nodes.tobytes(), tris.tobytes(), shade.tobytes(), None if uv is None else uv.tobytes(), n4.tobytes(), d4,
            r.bvh_export4q().tobytes(), r.bvh_export_planes4q().tobytes(), r.bvh_info()]


def _fresh(pkg, sc, meshes, builder, textures=None):
    r2 = pkg.Renderer(0)
    try:
        r2.set_option("gpu_build", 1)
        r2.set_option("gpu_builder", builder)
        r2.upload(meshes, sc["lights"], sc["materials"], textures)
        return _export(r2)
    finally:
        r2.close()


def _road_scenes():
    """Where the one-leaf host path, the hand-over between it and the device path and the slack behind the records can go wrong:
    1, 4 (= kLeafMax), 5 (the smallest device build) and 9 triangles over two meshes, the first with normals and uvs, the second
    with neither (and, for one triangle, with nothing at all); and the 9 triangles again with a NaN corner in one of them."""
    f = np.float32
    rng = np.random.default_rng(11)

    def mesh(n, full):
        v = (rng.uniform(-3, 3, (n, 1, 3)) + rng.uniform(-0.5, 0.5, (n, 3, 3))).astype(f).reshape(-1, 3)
        m = {"vertices": v, "triangles": np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)}
        if full:
            m["normals"] = rng.normal(size=(3 * n, 3)).astype(f)
            m["uvs"] = rng.random((3 * n, 3)).astype(f)
        return m

    out = [{"meshes": [mesh((n + 1) // 2, True), mesh(n // 2, False)], "lights": [], "materials": []} for n in (1, 4, 5, 9)]
    inert = [dict(m) for m in out[-1]["meshes"]]
    inert[0]["vertices"] = inert[0]["vertices"].copy()
    inert[0]["vertices"][7, 1] = np.nan  # triangle 2 of the first mesh
    return out + [{"meshes": inert, "lights": [], "materials": []}]


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [LBVH, PLOC])
def test_rebuild_without_changes_reproduces_the_upload(pkg, scenes, renderer, builder):
    r = renderer
    for sc in [scenes.textured_cornell(), _with_normals(scenes, scenes.displaced_sphere(n_lat=40, n_lon=40)), _chain()] + _road_scenes():
        r.set_option("gpu_build", 1)
        r.set_option("gpu_builder", builder)
        r.upload(sc["meshes"], sc["lights"], sc["materials"], sc.get("textures"), dynamic=True)
        before = _export(r)
        ms = r.rebuild()
        assert ms > 0
        assert _export(r) == before
    r.set_option("gpu_builder", LBVH)
    r.set_option("gpu_build", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_build,builder", [(1, LBVH), (1, PLOC), (0, LBVH)], ids=["lbvh", "ploc", "host-sah"])
def test_every_road_to_hbm_gives_the_same_bytes(pkg, renderer, gpu_build, builder):
    """A static upload, a dynamic upload and a dynamic upload followed by an identity update_vertices + refit leave the same binary,
    wide and quantised nodes, plane table, records and uvs in HBM, for both GPU builders and the host SAH tree.  (The rebuild with
    nothing pending is held to the dynamic upload by test_rebuild_without_changes_reproduces_the_upload, on the same scenes.)"""
    r = renderer
    r.set_option("gpu_build", gpu_build)
    r.set_option("gpu_builder", builder)
    try:
        for sc in _road_scenes():
            meshes = sc["meshes"]
            what = "%d triangles" % sum(len(m["triangles"]) for m in meshes)
            r.upload(meshes, sc["lights"], sc["materials"])
            static = _export(r)
            assert static[3] is not None, what + ": uv records"
            r.upload(meshes, sc["lights"], sc["materials"], dynamic=True)
            assert _export(r) == static, what + ": dynamic upload"
            for i, m in enumerate(meshes):
                if len(m["vertices"]):
                    r.update_vertices(i, m["vertices"], m.get("normals"))
            r.refit()
            assert _export(r) == static, what + ": identity refit"
    finally:
        r.set_option("gpu_builder", LBVH)
        r.set_option("gpu_build", 0)


def _shaded_outputs(r, rays, w, h):
    """every output of shade_rays (mode 100) and path_rays (2 samples) on `rays` and on the frame's camera rays, and the guides"""
    r.change_shading_mode(100)
    centre = r.camera_rays(w, h)
    out = {"camera_rays": centre}
    for tag, recs in (("rays", rays), ("camera rays", centre)):
        shaded, paths = r.shade_rays(recs), r.path_rays(recs, n_samples=2)
        out.update({"shade_rays %s, %s" % (k, tag): shaded[k] for k in sq.SHADE_OUTPUTS})
        out.update({"path_rays %s, %s" % (k, tag): paths[k] for k in ("rgb",) + sq.HIT_OUTPUTS})
    guides = r.frame_guides(w, h)
    out.update({"frame_guides " + k: guides[k] for k in ("normal", "albedo", "t")})
    # the kernels with phase machines of their own: ambient occlusion (bounded by the root box) and Whitted
    r.set_option("ao_samples", 5)
    r.set_option("ao_radius", 50)
    r.set_option("ao_sky", 1)
    for mode in (120, 150):
        r.change_shading_mode(mode)
        for tag, recs in (("rays", rays), ("camera rays", centre)):
            shaded = r.shade_rays(recs)
            out.update({"shade_rays mode %d %s, %s" % (mode, k, tag): shaded[k] for k in sq.SHADE_OUTPUTS})
        frame = r.render_frame(w, h)
        out.update({"render_frame mode %d %s" % (mode, k): frame[k] for k in ("rgb", "hit_t", "hit_inst", "hit_prim")})
    for name, v in sq.AO_DEFAULTS:
        r.set_option(name, v)
    r.change_shading_mode(100)
    return out


def _guides_and_paths_hold(r, w, h, what):
    """guides == shade_rays on the centre records; path_rays on the sample-0 records == the 1-spp mode-200 frame"""
    r.set_path_params(1, 2, 99)
    try:
        r.change_shading_mode(200)
        frame = r.render_frame(w, h)
        got = r.path_rays(r.camera_rays(w, h, sample=0))
        assert np.array_equal(_bits(got["rgb"]), _bits(frame["rgb"].reshape(-1, 3))), what + ": path_rays rgb"
        assert np.array_equal(_bits(got["t"]), _bits(frame["hit_t"].reshape(-1))), what + ": path_rays t"
        np.testing.assert_array_equal(got["inst"], frame["hit_inst"].reshape(-1), err_msg=what)
        np.testing.assert_array_equal(got["prim"], frame["hit_prim"].reshape(-1), err_msg=what)
        assert (got["inst"] != 0xFFFFFFFF).sum() > w * h // 10, what + ": the camera sees the scene"
        r.change_shading_mode(100)
        ref = r.shade_rays(r.camera_rays(w, h), want=("normal", "albedo", "t"))
        guides = r.frame_guides(w, h)
        for k in ("normal", "albedo", "t"):
            assert np.array_equal(_bits(guides[k]).reshape(-1), _bits(ref[k]).reshape(-1)), "%s: frame_guides %s" % (what, k)
    finally:
        r.set_path_params(4, 3, 1234)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [LBVH, PLOC])
def test_rebuild_of_moved_meshes_equals_a_fresh_build(pkg, scenes, oracle, dragon, renderer, builder):
    import torch
    r = renderer
    sc = _with_normals(scenes, scenes.cornell_box())
    d = _with_normals(scenes, dragon)
    sc = dict(sc, meshes=sc["meshes"] + d["meshes"])
    cam = sc["camera"]
    w, h = 160, 120
    r.set_option("gpu_build", 0)  # a host SAH upload: the rebuild must regrow every capacity
    r.set_option("gpu_builder", builder)
    r.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=True)
    r.set_camera(cam["position"], cam["matrix"])
    r.set_path_params(2, 2, 99)
    oracle.set_path_params(2, 2, 99)
    try:
        moved = [dict(m) for m in sc["meshes"]]
        # host vertex update of mesh 0, device update of the last mesh, a transform of mesh 1
        rng = np.random.default_rng(1)
        v0 = (sc["meshes"][0]["vertices"] + rng.uniform(-0.05, 0.05, sc["meshes"][0]["vertices"].shape)).astype(np.float32)
        r.update_vertices(0, v0)
        moved[0]["vertices"] = v0
        k = len(moved) - 1
        vk = (sc["meshes"][k]["vertices"] * np.float32(1.1)).astype(np.float32)
        r.update_vertices(k, torch.from_numpy(vk).cuda())
        moved[k]["vertices"] = vk
        M = _rot(10.0, 1, (0.1, 0.0, -0.2))
        r.set_mesh_transform(1, M)
        moved[1]["vertices"] = _apply(M, sc["meshes"][1]["vertices"])
        moved[1]["normals"] = _apply_normals(M, sc["meshes"][1]["normals"])
        ms = r.rebuild()
        assert ms > 0
        assert _export(r) == _fresh(pkg, sc, moved, builder)
        nodes, tris, shade = r.bvh_export()
        if builder == LBVH:
            O = oracle.OracleScene(moved, sc["lights"], sc["materials"], build_mode=1)
            assert nodes.tobytes() == O.nodes().tobytes() and tris.tobytes() == O.tris().tobytes()
        else:
            want = _expected(pkg, oracle, moved, sc["lights"], sc["materials"])
            assert nodes.tobytes() == want[0].tobytes() and tris.tobytes() == want[1].tobytes()
        S = oracle.OracleScene(moved, sc["lights"], sc["materials"])
        S.set_bvh(nodes, tris, shade)
        for mode in MODES:
            r.change_shading_mode(mode)
            r.set_counting(True)
            got = r.render_frame(w, h)
            r.set_counting(False)
            ref = S.render(cam["position"], cam["matrix"], mode, w, h)
            for key in ("hit_inst", "hit_prim", "rgba8"):
                np.testing.assert_array_equal(got[key], ref[key], err_msg="mode %d %s" % (mode, key))
            assert np.array_equal(_bits(got["hit_t"]), _bits(ref["hit_t"])) and np.array_equal(got["rgb"], ref["rgb"], equal_nan=True)
            assert (got["stats"]["nodes_visited"], got["stats"]["tris_tested"]) == (ref["stats"]["nodes_visited"], ref["stats"]["tris_tested"])
        rays = _rays(pkg, moved, 2000, seed=4)
        occ = r.occluded(rays)
        for i in range(0, len(rays), 20):
            ray = rays[i]
            assert bool(occ[i]) == bool(oracle.occluded(S, ray[0:3], ray[4:7], ray[3], ray[7])), "ray %d" % i
        # the shaded, path-traced and guide queries: the rebuilt context against a fresh upload of the moved meshes, every bit
        r2 = pkg.Renderer(0)
        try:
            r2.set_option("gpu_build", 1)
            r2.set_option("gpu_builder", builder)
            r2.upload(moved, sc["lights"], sc["materials"])
            r2.set_camera(cam["position"], cam["matrix"])
            r2.set_path_params(2, 2, 99)
            rebuilt, fresh = _shaded_outputs(r, rays, w, h), _shaded_outputs(r2, rays, w, h)
        finally:
            r2.close()
        for key in rebuilt:
            assert np.array_equal(rebuilt[key].view(np.uint32), fresh[key].view(np.uint32)), "%s: rebuilt and fresh differ" % key
        assert (rebuilt["shade_rays inst, rays"] != 0xFFFFFFFF).sum() > 500 and (rebuilt["path_rays inst, camera rays"] != 0xFFFFFFFF).sum() > w * h // 10
        # modes 120 and 150 of the rebuilt context against the oracle over its tree and brute-force probes (a small frame)
        small = {m: S.render(cam["position"], cam["matrix"], m, 48, 32) for m in (3, 100)}
        sq.new_modes_equal_references(r, small, 48, 32, 2, 99, "rebuilt, builder %d" % builder, dict(sc, meshes=moved),
                                      {"oracle": oracle, "camera": (cam["position"], cam["matrix"]), "lights": sc["lights"], "O": S, "path_held": (2, 2, 99)},
                                      held=(2, 99, 100))
        # a later deformation + refit refits the rebuilt shape
        v2 = (moved[0]["vertices"] + np.float32(0.02)).astype(np.float32)
        r.update_vertices(0, v2)
        moved2 = [dict(m) for m in moved]
        moved2[0]["vertices"] = v2
        r.refit()
        n2, t2, s2 = r.bvh_export()
        assert np.array_equal(n2["left"], nodes["left"]) and np.array_equal(n2["right"], nodes["right"])
        f2 = oracle.OracleScene(moved2, sc["lights"], sc["materials"], build_mode=1)
        by = lambda recs, t: recs[np.argsort(t["gid"], kind="stable")]  # noqa: E731
        assert by(t2, t2).tobytes() == by(f2.tris(), f2.tris()).tobytes() and by(s2, t2).tobytes() == by(f2.shade(), f2.tris()).tobytes()
        cb = spec.child_boxes(n2)
        boxes = spec.tri_boxes(moved2)
        gids = t2["gid"].astype(np.int64)
        for b in range(len(n2)):
            for side, ref in enumerate((int(n2[b]["left"]), int(n2[b]["right"]))):
                want = spec.union(cb[ref, 0], cb[ref, 1]) if ref >= 0 else spec._fold(boxes[gids[((~ref) >> 3):((~ref) >> 3) + ((~ref) & 7)]])
                assert _bits(cb[b, side]).tolist() == _bits(want).tolist()
    finally:
        oracle.set_path_params(4, 3, 1234)
        r.set_option("gpu_builder", LBVH)


@pytest.mark.gpu
def test_rebuild_builders_in_turn_then_refit(pkg, scenes, oracle, renderer):
    r = renderer
    sc = _with_normals(scenes, scenes.heightfield(n=48, n_lights=2))
    r.set_option("gpu_build", 0)
    r.set_option("gpu_builder", LBVH)
    r.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=True)
    r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
    M = _rot(10.0, 1)
    r.set_mesh_transform(0, M)
    moved = [dict(m) for m in sc["meshes"]]
    moved[0] = dict(sc["meshes"][0], vertices=_apply(M, sc["meshes"][0]["vertices"]), normals=_apply_normals(M, sc["meshes"][0]["normals"]))
    try:
        r.rebuild()
        assert _export(r) == _fresh(pkg, sc, moved, LBVH)
        _guides_and_paths_hold(r, 128, 96, "rebuilt with the LBVH")
        r.set_option("gpu_builder", PLOC)
        r.rebuild()
        assert _export(r) == _fresh(pkg, sc, moved, PLOC)
        _guides_and_paths_hold(r, 128, 96, "rebuilt with PLOC")
        r.set_mesh_transform(0, None)
        r.refit()
        _guides_and_paths_hold(r, 128, 96, "refitted to the rest pose")
        nodes, tris, shade = r.bvh_export()
        S = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
        S.set_bvh(nodes, tris, shade)
        assert r.bvh_export4q().tobytes() == S.nodes4q().tobytes()
        cam = sc["camera"]
        r.set_camera(cam["position"], cam["matrix"])
        r.change_shading_mode(100)
        got = r.render_frame(128, 96)
        ref = S.render(cam["position"], cam["matrix"], 100, 128, 96)
        np.testing.assert_array_equal(got["rgba8"], ref["rgba8"])
    finally:
        r.set_option("gpu_builder", LBVH)


@pytest.mark.gpu
def test_rebuild_restarts_accumulation(pkg, scenes, renderer):
    r = renderer
    sc = scenes.cornell_box()
    r.set_option("gpu_build", 1)
    r.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=True)
    r.set_option("gpu_build", 0)
    cam = sc["camera"]
    r.set_camera(cam["position"], cam["matrix"])
    r.change_shading_mode(200)
    r.set_path_params(2, 2, 5)
    r.set_accumulation(64)
    try:
        r.render_frame(64, 64)
        r.render_frame(64, 64)
        assert r.accumulated_samples() == 4
        r.rebuild()
        assert r.accumulated_samples() == 0
        r.render_frame(64, 64)
        assert r.accumulated_samples() == 2
    finally:
        r.set_accumulation(0)


@pytest.mark.gpu
def test_rebuild_state_and_option_errors(pkg, scenes, oracle, renderer):
    L = pkg.lib()
    r = renderer
    ms = C.c_double(3.0)
    for v in (-1, 2, 7):
        assert L.crt_set_option(r.h, b"gpu_builder", v) == EINVAL
    sc = scenes.cornell_box()
    r.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=False)
    assert L.crt_rebuild(r.h, C.byref(ms)) == ESTATE and ms.value == 0.0
    with pytest.raises(pkg.CrtError):
        r.rebuild()
    r2 = pkg.Renderer(0)
    try:
        assert L.crt_rebuild(r2.h, None) == ESTATE  # no scene
        # "gpu_builder" leaves host SAH uploads alone
        r2.set_option("gpu_builder", PLOC)
        r2.upload(sc["meshes"], sc["lights"], sc["materials"])
        O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
        nodes, tris, shade = r2.bvh_export()
        assert nodes.tobytes() == O.nodes().tobytes() and tris.tobytes() == O.tris().tobytes()
        assert r2.bvh_export4q().tobytes() == O.nodes4q().tobytes()
    finally:
        r2.close()


@pytest.mark.gpu
def test_two_contexts_build_identical_bytes(pkg, scenes):
    sc = scenes.icosphere_soup()
    outs = [_fresh(pkg, sc, sc["meshes"], PLOC) for _ in range(2)]
    assert outs[0] == outs[1]
