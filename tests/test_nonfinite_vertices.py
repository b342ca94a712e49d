"""Non-finite vertices (include/crt_hip.h, "inert triangles"): a triangle with a NaN or an inf among its nine vertex coordinates is
never reported, and every result equals the result for the scene without it -- over every tree.  The rule that makes it so sits
where a triangle's box and centroid are taken (such a triangle is the point (0, 0, 0) to every builder and to the refit, and its
record is nine quiet NaNs); these tests pin it by comparing every tree walk with brute force over the same records, bit for bit, on scenes poisoned with NaN,
+inf, -inf and a mix of them at the places listed in _CASES.  Winding numbers, whose walk enters every cluster and whose moment table sums over every
triangle below a node, are held by tests/winding_checks.py's assert_winding: exact mode to brute force over the records with the
inert ones deleted, the moment table to a float64 statement that drops them (tests/test_winding_checks.py shows on the CPU that
the points of every case would see an inert triangle that was counted)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ploc_reference as spec  # noqa: E402
import shaded_query_checks as sq  # noqa: E402
import test_list_hits as lh  # noqa: E402
import test_point_queries as pq  # noqa: E402
import winding_checks as wc  # noqa: E402
from test_dynamic_geometry import _numpy_refit  # noqa: E402
from test_list_hits import ref as list_ref  # noqa: E402,F401  (fixture: tests/list_hits_reference.c)
from test_point_queries import ref as point_ref  # noqa: E402,F401  (fixture: tests/point_reference.c)
from winding_checks import wref  # noqa: E402,F401  (fixture: tests/winding_reference.c)

MISS = 0xFFFFFFFF
KINDS = {"nan": (np.nan,), "+inf": (np.inf,), "-inf": (-np.inf,), "mix": (np.nan, np.inf, -np.inf)}
FRAME_MODES = (3, 100, 200)
ALL_MODES = (0, 1, 2, 3, 4, 5, 6, 100, 200)
LBVH, PLOC = 0, 1
N_RAYS = 2000
PATH_PARAMS = (2, 2, 99)
N_SEEDED, MAX_AIMED = 64, 8  # poses per case: seeded ones, and one aimed at each of up to 8 inert triangles


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- scenes and poison

def _scene(meshes, lights=None, materials=None, cam=(0.0, 0.0, 15.0), textures=None):
    sc = {"meshes": meshes, "lights": [((0.0, 4.5, 6.0), 600.0)] if lights is None else lights,
          "materials": [{"albedo": (0.7, 0.7, 0.7), "type": 1}] if materials is None else materials,
          "camera": {"position": np.float32(cam), "matrix": np.eye(3, dtype=np.float32).reshape(9)}}
    if textures is not None:
        sc["textures"] = textures
    return sc


def _probe_mesh(n, seed):
    """n small triangles: a centre in [-5, 5]^3, vertices within 0.15 of it (edges about 0.3)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-5, 5, (n, 1, 3))
    v = (c + rng.uniform(-0.15, 0.15, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    return {"vertices": v, "triangles": np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), "material_index": 0, "normals": None}


def _icosphere(scenes, subdiv=3, r=2.0, c=(0.0, 0.0, 0.0)):
    v, f = scenes._icosphere(subdiv)
    return {"vertices": (np.float32(r * v) + np.float32(c)).astype(np.float32), "triangles": f.astype(np.uint32),
            "material_index": 0, "normals": None}


def _poisoned(sc, picks, kind, seed=0):
    """a copy of the scene in which every picked vertex (mesh, vertex indices) holds a bad value: one seeded coordinate of it
    for NaN / +inf / -inf, all three (NaN, +inf, -inf in a seeded rotation) for the mix"""
    rng = np.random.default_rng(seed)
    bad = KINDS[kind]
    meshes = [dict(m) for m in sc["meshes"]]
    for mesh, verts in picks:
        v = np.array(meshes[mesh]["vertices"], dtype=np.float32).reshape(-1, 3)
        for i in np.atleast_1d(verts):
            if len(bad) == 1:
                v[i, rng.integers(3)] = bad[0]
            else:
                v[i] = np.roll(np.float32(bad), rng.integers(3))
        meshes[mesh]["vertices"] = v
    return dict(sc, meshes=meshes, clean=sc["meshes"])


def _inert_mask(meshes):
    """per mesh, the triangles with a non-finite value among their nine coordinates"""
    out = []
    for m in meshes:
        v = np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3)
        t = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)
        out.append(~np.isfinite(v[t]).all(axis=(1, 2)) if len(t) else np.zeros(0, bool))
    return out


def _records(pkg, meshes):
    """the triangle records an upload writes, by gid: {v0, e1 = v1 - v0, e2 = v2 - v0}, and nine quiet NaNs of the bits
    0x7FC00000 for an inert triangle (what a subtraction makes of a NaN's sign depends on who compiles it)"""
    assert np.float32(np.nan).view(np.uint32) == 0x7FC00000
    with np.errstate(invalid="ignore"):
        recs = pq._tri_records(pkg, meshes)
    dead = np.concatenate(_inert_mask(meshes))
    for k in ("v0", "e1", "e2"):
        recs[k][dead] = np.float32(np.nan)
    return recs


def _with_normals(scenes, meshes, which):
    out = [dict(m) for m in meshes]
    for i in which:
        out[i]["normals"] = scenes.vertex_normals(out[i]["vertices"], out[i]["triangles"]).astype(np.float32)
    return out


def _leaf_vertices(oracle, sc, mesh):
    """the first vertex of every triangle of one leaf of the clean scene's SAH tree: the fullest leaf that holds triangles of
    `mesh` only (the first such leaf in node order)"""
    O = oracle.OracleScene(sc["meshes"])
    nodes, tris = O.nodes(), O.tris()
    best = None
    for ref in np.stack([nodes["left"], nodes["right"]], 1).reshape(-1):
        first, cnt = (~int(ref)) >> 3, (~int(ref)) & 7
        if ref < 0 and np.all(tris["inst"][first:first + cnt] == mesh) and (best is None or cnt > best[1]):
            best = (first, cnt)
    first, cnt = best
    t = np.asarray(sc["meshes"][mesh]["triangles"]).reshape(-1, 3)
    return np.unique(t[tris["prim"][first:first + cnt], 0])


def _tiny(n):
    f = np.float32
    tri = f([(0, 0, -3), (1, 0, -3), (0, 1, -3)])
    v = np.concatenate([tri + f([1.5 * i - 2.0, 0.1 * i, 0]) for i in range(n)])
    return _scene([{"vertices": v, "triangles": np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), "material_index": 0, "normals": None}],
                  cam=(0.0, 0.3, 4.0))


def _build_case(name, kind, scenes, oracle, dragon):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("probe100", "probe2000"):  # three random vertices, and the first and the last vertex of the mesh
        n = int(name[5:])
        sc = _scene([_probe_mesh(n, n)])
        return _poisoned(sc, [(0, np.concatenate([rng.integers(0, 3 * n, 3), [0, 3 * n - 1]]))], kind)
    if name == "cornell_first_last":  # the first vertex of the first mesh and the last of the last one
        sc = scenes.cornell_box()
        return _poisoned(sc, [(0, 0), (5, len(sc["meshes"][5]["vertices"]) - 1)], kind)
    if name == "cornell_whole_mesh":  # every vertex of the short box
        sc = scenes.cornell_box()
        return _poisoned(sc, [(4, np.arange(len(sc["meshes"][4]["vertices"])))], kind)
    if name == "dragon_shared_vertex":  # the vertex most triangles share
        big = int(np.argmax([len(m["triangles"]) for m in dragon["meshes"]]))
        valence = np.bincount(np.asarray(dragon["meshes"][big]["triangles"]).reshape(-1))
        return _poisoned(dragon, [(big, int(np.argmax(valence)))], kind)
    if name == "heightfield_leaf":  # every triangle of one leaf
        sc = scenes.heightfield(n=48, n_lights=2)
        return _poisoned(sc, [(1, _leaf_vertices(oracle, sc, 1))], kind)
    if name == "icosphere_pole":  # a closed mesh; vertex 0 is shared by five triangles
        return _poisoned(_scene([_icosphere(scenes)], cam=(0.0, 0.0, 7.0)), [(0, 0)], kind)
    if name.startswith("tiny"):  # 1 to 5 triangles, one of them inert: the one-leaf root, the host path of the rebuild
        n = int(name[4:])
        return _poisoned(_tiny(n), [(0, 3 * (n // 2) + 1)], kind)
    if name == "all_inert":  # every triangle of the scene
        sc = _scene([_probe_mesh(50, 7)])
        return _poisoned(sc, [(0, 3 * np.arange(50) + rng.integers(0, 3, 50))], kind)
    if name == "finite_beside_inert":  # one finite mesh beside one fully inert mesh
        sc = _scene([_icosphere(scenes, 2), dict(_probe_mesh(40, 11), material_index=0)], cam=(0.0, 0.0, 9.0))
        return _poisoned(sc, [(1, 3 * np.arange(40) + rng.integers(0, 3, 40))], kind)
    if name == "normals_and_uvs":  # an inert triangle in a mesh without normals, and in one with normals and uvs
        sc = scenes.textured_cornell()
        sc = dict(sc, meshes=_with_normals(scenes, sc["meshes"], (4, 5)))
        return _poisoned(sc, [(0, 5), (4, 2)], kind)
    raise KeyError(name)


_CASES = ("probe100", "probe2000", "cornell_first_last", "cornell_whole_mesh", "dragon_shared_vertex", "heightfield_leaf",
          "icosphere_pole", "tiny1", "tiny2", "tiny3", "tiny4", "tiny5", "all_inert", "finite_beside_inert", "normals_and_uvs")
_PARAMS = [(c, k) for c in _CASES for k in KINDS]
_IDS = ["%s-%s" % p for p in _PARAMS]
_cache = {}


@pytest.fixture(scope="module")
def case(scenes, oracle, dragon):
    def get(name, kind):
        if (name, kind) not in _cache:
            sc = _build_case(name, kind, scenes, oracle, dragon)
            inert = _inert_mask(sc["meshes"])
            assert sum(int(m.sum()) for m in inert) > 0
            sc["inert"] = inert
            sc["rays"] = _rays(sc, N_RAYS, seed=len(_cache))
            _cache[(name, kind)] = sc
        return _cache[(name, kind)]
    return get


def _rays(sc, n, seed):
    """generic rays: random origins around the finite vertices, aimed at the centroids of random finite triangles (at random
    points of the same region when no triangle is finite)"""
    import __graft_entry__ as entry
    pkg = entry.load_package()
    rng = np.random.default_rng(1000 + seed)
    cents, verts = [], []
    for m, dead in zip(sc["meshes"], _inert_mask(sc["meshes"])):
        v = np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3)
        t = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)
        if len(t):
            cents.append(v[t[~dead]].astype(np.float64).mean(axis=1))
        verts.append(v[np.isfinite(v).all(axis=1)])
    cents, verts = np.concatenate(cents), np.concatenate(verts)
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    ext = np.maximum(hi - lo, 1.0)
    o = (lo - 0.3 * ext + rng.random((n, 3)) * 1.6 * ext).astype(np.float32)
    tgt = cents[rng.integers(0, len(cents), n)] if len(cents) else lo + rng.random((n, 3)) * ext
    return pkg.make_rays(o, (tgt - o).astype(np.float32), tmin=0.0, tmax=rng.choice([np.inf, np.inf, 2.0], size=n))


def _oracle_scene(oracle, sc, build_mode=0, meshes=None):
    return oracle.OracleScene(sc["meshes"] if meshes is None else meshes, sc["lights"], sc["materials"], build_mode=build_mode,
                              textures=list(sc.get("textures", ())))


def _inert_ids(sc):
    """(inst, prim) of the inert triangles as one uint64 key each"""
    return np.concatenate([(np.uint64(i) << np.uint64(32)) | np.flatnonzero(d).astype(np.uint64) for i, d in enumerate(sc["inert"])])


def _assert_none_inert(sc, inst, prim, what):
    hit = np.asarray(inst).reshape(-1) != MISS
    key = (np.asarray(inst).reshape(-1)[hit].astype(np.uint64) << np.uint64(32)) | np.asarray(prim).reshape(-1)[hit].astype(np.uint64)
    assert not np.isin(key, _inert_ids(sc)).any(), "%s: an inert triangle was reported" % what


def _aimed_poses(sc):
    """one pose per inert triangle (at most MAX_AIMED, spread evenly over them): at C + 0.25 L n for the centroid C, the unit
    normal n and the shortest edge L of the triangle's clean vertices, turned so that the pixel-centre ray of a 1 x 1 frame
    (the camera's -z axis: the rotation's third column is n) runs along -n.  In the clean scene that ray's closest hit is the
    triangle.  Returns positions, rotations and the (inst, prim) aimed at."""
    clean = sc.get("clean", sc["meshes"])
    ids = [(i, int(p)) for i, dead in enumerate(sc["inert"]) for p in np.flatnonzero(dead)]
    if len(ids) > MAX_AIMED:
        ids = [ids[k] for k in np.linspace(0, len(ids) - 1, MAX_AIMED).astype(int)]
    pos, rot = np.zeros((len(ids), 3), np.float32), np.zeros((len(ids), 9), np.float32)
    for k, (i, p) in enumerate(ids):
        v = np.asarray(clean[i]["vertices"], dtype=np.float32).reshape(-1, 3).astype(np.float64)
        a, b, c = v[np.asarray(clean[i]["triangles"], dtype=np.int64).reshape(-1, 3)[p]]
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        L = min(np.linalg.norm(b - a), np.linalg.norm(c - b), np.linalg.norm(a - c))
        x = np.cross(np.eye(3)[np.argmin(np.abs(n))], n)
        x /= np.linalg.norm(x)
        pos[k] = (a + b + c) / 3.0 + 0.25 * L * n
        rot[k] = np.stack([x, np.cross(n, x), n], axis=1).astype(np.float32).reshape(9)
    return pos, rot, ids


def _pose_refs(oracle, sc):
    """the case's poses with their brute-force 1 x 1 oracle frames in modes 100 and 200 (PATH_PARAMS), computed once and
    shared: N_SEEDED seeded poses over the finite vertices' box, then the aimed ones"""
    if "poses" not in sc:
        pos, rot = sq.poses(sc, n=N_SEEDED)
        apos, arot, aimed = _aimed_poses(sc)
        P = sq.pose_set(oracle, sc, np.concatenate([pos, apos]), np.concatenate([rot, arot]), PATH_PARAMS, brute_force=True)
        P["aimed"], P["n_seeded"] = aimed, len(pos)
        for mode in (100, 200):
            _assert_none_inert(sc, P[mode]["inst"], P[mode]["prim"], "poses mode %d" % mode)
            for a in P[mode].values():
                a.setflags(write=False)
        sc["poses"] = P
    return sc["poses"]


def _assert_tree_equals_brute_force(oracle, O, sc, what, w=96, h=96):
    """the oracle's walk over the tree O holds against brute force over the same records: closest hits and occlusion of the
    case's generic rays, frames in modes 3, 100 and 200 -- every bit, no exemptions"""
    rays = sc["rays"]
    a, b = oracle.trace_rays(O, rays), oracle.trace_rays(O, rays, brute_force=True)
    for k in ("inst", "prim"):
        bad = np.flatnonzero(a[k] != b[k])
        assert len(bad) == 0, "%s: %s of %d rays differ from brute force, first ray %d: tree %r, brute force %r (t %r vs %r)" % (
            what, k, len(bad), bad[0], a[k][bad[0]], b[k][bad[0]], a["t"][bad[0]], b["t"][bad[0]])
    assert np.array_equal(_bits(a["t"]), _bits(b["t"])) and np.array_equal(_bits(a["uv"]), _bits(b["uv"])), what
    _assert_none_inert(sc, b["inst"], b["prim"], what)
    np.testing.assert_array_equal(oracle.occluded_rays(O, rays)["occluded"], oracle.occluded_rays(O, rays, brute_force=True)["occluded"],
                                  err_msg=what)
    cam = sc["camera"]
    oracle.set_path_params(*PATH_PARAMS)
    try:
        for mode in FRAME_MODES:
            f = O.render(cam["position"], cam["matrix"], mode, w, h)
            g = O.render(cam["position"], cam["matrix"], mode, w, h, brute_force=True)
            for k in ("hit_inst", "hit_prim", "rgba8"):
                n = int((f[k] != g[k]).sum())
                assert n == 0, "%s: mode %d %s differs from brute force at %d of %d" % (what, mode, k, n, f[k].size)
            assert np.array_equal(_bits(f["hit_t"]), _bits(g["hit_t"])) and np.array_equal(_bits(f["rgb"]), _bits(g["rgb"])), \
                "%s: mode %d" % (what, mode)
            _assert_none_inert(sc, g["hit_inst"], g["hit_prim"], "%s mode %d" % (what, mode))
    finally:
        oracle.set_path_params(4, 3, 1234)


def _ploc_tree(pkg, oracle, sc):
    """(nodes, tris, shade, max_depth) of the PLOC statement (tests/ploc_reference.py) for the scene"""
    O = _oracle_scene(oracle, sc, build_mode=1)
    order = O.tris()["gid"].astype(np.int64)
    nodes, gids, depth, _ = spec.build(spec.tri_boxes(sc["meshes"]), order, pkg.NODE_DTYPE)
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))
    pick = inv[gids]
    return nodes, O.tris()[pick], O.shade()[pick], depth


def _refit_tree(oracle, sc):
    """the clean scene's SAH tree refitted to the poisoned vertices: (nodes, tris, shade)"""
    clean = _oracle_scene(oracle, sc, meshes=sc["clean"])
    nodes, shape = clean.nodes(), clean.tris()
    P = _oracle_scene(oracle, sc)
    by_gid = np.argsort(P.tris()["gid"], kind="stable")
    pick = by_gid[shape["gid"].astype(np.int64)]
    tris, shade = P.tris()[pick], P.shade()[pick]
    want = _numpy_refit(nodes, tris, sc["meshes"])  # (node, child, lo / hi, axis)
    for c, side in enumerate("lr"):
        for a, ax in enumerate("xyz"):
            nodes[side + ax + "0"], nodes[side + ax + "1"] = want[:, c, 0, a], want[:, c, 1, a]
    return nodes, tris, shade


# ---- CPU: every tree walk equals brute force (these fail without the rule)

@pytest.mark.parametrize("build_mode", [0, 1])
@pytest.mark.parametrize("name,kind", _PARAMS, ids=_IDS)
def test_oracle_tree_equals_brute_force(oracle, case, name, kind, build_mode):
    sc = case(name, kind)
    _assert_tree_equals_brute_force(oracle, _oracle_scene(oracle, sc, build_mode), sc, "%s %s build_mode %d" % (name, kind, build_mode))


@pytest.mark.parametrize("name,kind", _PARAMS, ids=_IDS)
def test_ploc_statement_terminates_and_equals_brute_force(pkg, oracle, case, name, kind):
    sc = case(name, kind)
    nodes, tris, shade, depth = _ploc_tree(pkg, oracle, sc)
    assert np.all(np.isfinite(spec.child_boxes(nodes))) and depth <= 32
    assert np.array_equal(np.sort(tris["gid"]), np.arange(len(tris)))
    O = _oracle_scene(oracle, sc)
    O.set_bvh(nodes, tris, shade)
    _assert_tree_equals_brute_force(oracle, O, sc, "%s %s PLOC" % (name, kind), 64, 64)
    _assert_finite_triangles_are_contained(sc, O, "%s %s PLOC" % (name, kind))


@pytest.mark.parametrize("name,kind", _PARAMS, ids=_IDS)
def test_refitted_tree_equals_brute_force(oracle, case, name, kind):
    sc = case(name, kind)
    nodes, tris, shade = _refit_tree(oracle, sc)
    assert np.all(np.isfinite(spec.child_boxes(nodes)))
    O = _oracle_scene(oracle, sc)
    O.set_bvh(nodes, tris, shade)
    _assert_tree_equals_brute_force(oracle, O, sc, "%s %s refit" % (name, kind), 64, 64)
    _assert_finite_triangles_are_contained(sc, O, "%s %s refit" % (name, kind))


# ---- CPU: as if the inert triangles were absent

def _without_inert(sc):
    """the scene with the inert triangles deleted (every mesh stays, so `inst` keeps its meaning), and per mesh the original
    prim id of every triangle that is left"""
    meshes, back = [], []
    for m, dead in zip(sc["meshes"], sc["inert"]):
        t = np.asarray(m["triangles"], dtype=np.uint32).reshape(-1, 3)
        meshes.append(dict(m, triangles=np.ascontiguousarray(t[~dead])))
        back.append(np.flatnonzero(~dead).astype(np.uint32))
    return meshes, back


def _map_back(inst, prim, back):
    out = np.array(prim, dtype=np.uint32, copy=True)
    for i, b in enumerate(back):
        sel = (inst == i) & (prim != MISS)
        out[sel] = b[prim[sel]]
    return out


def _points(pkg, sc, n, seed):
    """points around the finite vertices: uniform ones with rmax = inf, and ones near finite vertices with a finite rmax"""
    rng = np.random.default_rng(2000 + seed)
    v = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    v = v[np.isfinite(v).all(axis=1)]
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, 1.0)
    uni = (lo - 0.2 * ext + rng.random((n, 3)) * 1.4 * ext).astype(np.float32)
    near = (v[rng.integers(0, len(v), n)] + rng.normal(size=(n, 3)) * 0.05 * ext.max()).astype(np.float32)
    return np.concatenate([pkg.make_points(uni), pkg.make_points(near, rmax=rng.choice([0.02, 0.1, 0.5], size=n) * float(ext.max()))])


@pytest.mark.parametrize("name,kind", _PARAMS, ids=_IDS)
def test_brute_force_results_equal_the_scene_without_the_inert_triangles(pkg, oracle, point_ref, list_ref, case, name, kind):
    sc = case(name, kind)
    meshes, back = _without_inert(sc)
    what = "%s %s" % (name, kind)
    rays = sc["rays"]
    # closest hits and occlusion (oracle, brute force)
    P, D = _oracle_scene(oracle, sc), _oracle_scene(oracle, sc, meshes=meshes)
    a, b = oracle.trace_rays(P, rays, brute_force=True), oracle.trace_rays(D, rays, brute_force=True)
    np.testing.assert_array_equal(a["inst"], b["inst"], err_msg=what)
    np.testing.assert_array_equal(a["prim"], _map_back(b["inst"], b["prim"], back), err_msg=what)
    assert np.array_equal(_bits(a["t"]), _bits(b["t"])) and np.array_equal(_bits(a["uv"]), _bits(b["uv"])), what
    np.testing.assert_array_equal(oracle.occluded_rays(P, rays, brute_force=True)["occluded"],
                                  oracle.occluded_rays(D, rays, brute_force=True)["occluded"], err_msg=what)
    # closest points (rmax infinite and finite), hit counts, occupancy (tests/point_reference.c) and lists (list_hits_reference.c)
    tp, td = _records(pkg, sc["meshes"]), _records(pkg, meshes)
    pts = _points(pkg, sc, 1000, len(name))
    cp, cd = pq.ref_closest(point_ref, tp, pts), pq.ref_closest(point_ref, td, pts)
    _assert_none_inert(sc, cp["inst"], cp["prim"], what + " closest points")
    np.testing.assert_array_equal(cp["inst"], cd["inst"], err_msg=what)
    np.testing.assert_array_equal(cp["prim"], _map_back(cd["inst"], cd["prim"], back), err_msg=what)
    for k in ("dist", "point", "uv"):
        assert np.array_equal(_bits(cp[k]), _bits(cd[k])), "%s closest points %s" % (what, k)
    if len(td):
        assert (cp["inst"] != MISS).sum() > 1000 and (cp["inst"][1000:] == MISS).any()
    np.testing.assert_array_equal(pq.ref_count(point_ref, tp, rays), pq.ref_count(point_ref, td, rays), err_msg=what)
    np.testing.assert_array_equal(pq.ref_occupancy(point_ref, tp, pts), pq.ref_occupancy(point_ref, td, pts), err_msg=what)
    lp, ld = lh.ref_list(list_ref, tp, rays), lh.ref_list(list_ref, td, rays)
    np.testing.assert_array_equal(lp["offsets"], ld["offsets"], err_msg=what)
    _assert_none_inert(sc, lp["inst"], lp["prim"], what + " lists")
    np.testing.assert_array_equal(lp["inst"], ld["inst"], err_msg=what)
    np.testing.assert_array_equal(lp["prim"], _map_back(ld["inst"], ld["prim"], back), err_msg=what)
    assert np.array_equal(_bits(lp["t"]), _bits(ld["t"])) and np.array_equal(_bits(lp["uv"]), _bits(ld["uv"])), what
    # the poses of the shaded and path-traced queries: colour and hit of the 1 x 1 frames (oracle, brute force)
    poses = _pose_refs(oracle, sc)
    for mode in (100, 200):
        p = poses[mode]
        d = sq.pose_reference(oracle, sc, poses["pos"], poses["rot"], mode, brute_force=True, path_params=PATH_PARAMS, meshes=meshes)
        np.testing.assert_array_equal(p["inst"], d["inst"], err_msg="%s poses mode %d" % (what, mode))
        np.testing.assert_array_equal(p["prim"], _map_back(d["inst"], d["prim"], back), err_msg="%s poses mode %d" % (what, mode))
        assert np.array_equal(_bits(p["rgb"]), _bits(d["rgb"])) and np.array_equal(_bits(p["t"]), _bits(d["t"])), "%s poses mode %d" % (what, mode)


# ---- CPU: the scenes of the GPU tests can show an inert triangle that is hit, that occludes or that is bounced onto

def test_poses_and_frames_would_show_an_inert_triangle_that_is_hit_or_occludes(oracle, case):
    """the oracle alone, over _GPU_PARAMS together: every aimed pose hits its triangle in the clean scene and not in the poisoned
    one, and there are at least 20 of them; "never occlude": the camera frame of cornell_whole_mesh has at least 16 pixels whose
    primary hit is the same with and without the short box and whose mode-100 colour differs (its shadow on the floor); "never
    bounced onto": some pose or pixel in mode 200 has the same primary hit and another colour"""
    def changed(a, b, inst="inst", prim="prim"):
        same = (a[inst] == b[inst]) & (a[prim] == b[prim]) & (a[inst] != MISS)
        return int((same & np.any(_bits(a["rgb"]) != _bits(b["rgb"]), axis=-1)).sum())

    aimed, lit, bounced, shadow_pixels = 0, 0, 0, None
    for name, kind in _GPU_PARAMS:
        sc = case(name, kind)
        clean = _clean_scene(sc)
        P = _pose_refs(oracle, sc)
        C = {m: sq.pose_reference(oracle, clean, P["pos"], P["rot"], m, brute_force=True, path_params=PATH_PARAMS) for m in (100, 200)}
        for j, (inst, prim) in enumerate(P["aimed"]):
            k = P["n_seeded"] + j
            assert (C[100]["inst"][k], C[100]["prim"][k]) == (inst, prim), "%s %s: aimed pose %d misses its triangle in the clean scene" % (name, kind, j)
            assert (P[100]["inst"][k], P[100]["prim"][k]) != (inst, prim), "%s %s: aimed pose %d" % (name, kind, j)
        aimed += len(P["aimed"])
        lit += changed(P[100], C[100])
        bounced += changed(P[200], C[200])
        if name == "cornell_whole_mesh":
            cam = sc["camera"]
            oracle.set_path_params(*PATH_PARAMS)
            try:
                f = {(which, m): _oracle_scene(oracle, s).render(cam["position"], cam["matrix"], m, W, H, brute_force=True)
                     for which, s in (("poisoned", sc), ("clean", clean)) for m in (100, 200)}
            finally:
                oracle.set_path_params(4, 3, 1234)
            shadow_pixels = changed(f[("poisoned", 100)], f[("clean", 100)], "hit_inst", "hit_prim")
            bounced += changed(f[("poisoned", 200)], f[("clean", 200)], "hit_inst", "hit_prim")
    print("aimed poses %d; same primary hit, other colour: %d mode-100 poses, %d cornell_whole_mesh mode-100 pixels, %d mode-200 poses and pixels"
          % (aimed, lit, shadow_pixels, bounced))
    assert aimed >= 20, aimed
    assert shadow_pixels >= 16, shadow_pixels
    assert bounced >= 1, bounced


# ---- CPU: the host builder writes the oracle's bytes, and every ancestor's quantised box holds every finite triangle

def _decoded_slots(q):
    """(n, 4, 2, 3) float32: the decoded quantised box (lo / hi, axis) of every slot -- the kernels' fma(q, s, lo)"""
    out = np.zeros((len(q), 4, 2, 3), np.float32)
    for a, (qlo, qhi) in enumerate((("qlo_x", "qhi_x"), ("qlo_y", "qhi_y"), ("qlo_z", "qhi_z"))):
        lo, s = q["lo"][:, a].astype(np.float64), q["s"][:, a].astype(np.float64)
        for k in range(4):
            out[:, k, 0, a] = (((q[qlo] >> (8 * k)) & 0xFF).astype(np.float64) * s + lo).astype(np.float32)  # one rounding = fmaf
            out[:, k, 1, a] = (((q[qhi] >> (8 * k)) & 0xFF).astype(np.float64) * s + lo).astype(np.float32)
    return out


def _assert_finite_triangles_are_contained(sc, O, what):
    """walk the quantised wide tree of O from the root: the vertex box of every finite triangle lies inside the decoded box of
    the leaf slot that holds it and of every slot above it"""
    q, tris = O.nodes4q(), O.tris()
    if not len(q):
        return
    dec = _decoded_slots(q)
    V = [np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]]
    T = [np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3) for m in sc["meshes"]]
    p = np.stack([V[i][T[i][j]] for i, j in zip(tris["inst"], tris["prim"])])  # (n, 3 vertices, 3 axes), leaf order
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(p).all(axis=(1, 2))
        tlo, thi = p.min(axis=1), p.max(axis=1)
    seen = np.zeros(len(tris), np.int64)
    stack = [(0, np.full(3, -np.inf, np.float32), np.full(3, np.inf, np.float32))]  # node, the intersection of the boxes above it
    while stack:
        node, lo, hi = stack.pop()
        for k in range(4):
            ref = int(q["ref"][node][k])
            if ref == -1:
                continue
            l, u = np.maximum(lo, dec[node, k, 0]), np.minimum(hi, dec[node, k, 1])
            if ref >= 0:
                stack.append((ref, l, u))
                continue
            first, cnt = (~ref) >> 3, (~ref) & 7
            seen[first:first + cnt] += 1
            for j in range(first, first + cnt):
                if finite[j]:
                    assert np.all(l <= tlo[j]) and np.all(thi[j] <= u), \
                        "%s: triangle gid %d (%r .. %r) sticks out of a box above it (%r .. %r)" % (what, tris["gid"][j], tlo[j], thi[j], l, u)
    assert np.all(seen == 1), what


@pytest.mark.parametrize("name,kind", _PARAMS, ids=_IDS)
def test_host_builder_equals_the_oracle_and_boxes_contain_finite_triangles(pkg, oracle, case, name, kind):
    sc = case(name, kind)
    what = "%s %s" % (name, kind)
    O = _oracle_scene(oracle, sc)
    nodes, tris, shade, md = pkg.build_bvh_host(sc["meshes"])
    assert nodes.tobytes() == O.nodes().tobytes() and tris.tobytes() == O.tris().tobytes() and shade.tobytes() == O.shade().tobytes(), what
    assert md == O.max_depth
    n4, d4 = pkg.build_bvh4_host(sc["meshes"])
    assert n4.tobytes() == O.nodes4().tobytes() and d4 == O.depth4, what
    assert pkg.quantize4(n4).tobytes() == O.nodes4q().tobytes(), what
    assert np.all(np.isfinite(spec.child_boxes(nodes)))
    # the records: the vertices' values, and nine quiet NaNs for an inert triangle
    assert tris[np.argsort(tris["gid"], kind="stable")].tobytes() == _records(pkg, sc["meshes"]).tobytes(), what
    for bm in (0, 1):
        _assert_finite_triangles_are_contained(sc, _oracle_scene(oracle, sc, bm), "%s build_mode %d" % (what, bm))


# ---- GPU: the kernels over every upload, refit and rebuild

TREES = {"sah": {"gpu_build": 0, "gpu_builder": LBVH}, "lbvh": {"gpu_build": 1, "gpu_builder": LBVH}, "ploc": {"gpu_build": 1, "gpu_builder": PLOC}}
W, H = 96, 64
# the kinds in turn over the cases, and every kind at the first one
_GPU_PARAMS = [(c, list(KINDS)[i % 4]) for i, c in enumerate(_CASES)] + [("probe100", k) for k in ("+inf", "-inf", "mix")]
_GPU_IDS = ["%s-%s" % p for p in _GPU_PARAMS]


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def defaults(renderer, oracle):
    renderer.set_path_params(*PATH_PARAMS)
    oracle.set_path_params(*PATH_PARAMS)
    yield
    for k, v in (("gpu_build", 0), ("gpu_builder", LBVH), ("path_pipeline", 0)):
        renderer.set_option(k, v)
    renderer.set_counting(False)
    renderer.set_path_params()
    oracle.set_path_params(4, 3, 1234)


def _upload(r, sc, tree, dynamic=False, meshes=None):
    for k, v in TREES[tree].items():
        r.set_option(k, v)
    r.upload(sc["meshes"] if meshes is None else meshes, sc["lights"], sc["materials"], sc.get("textures"), dynamic=dynamic)
    r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])


def _export(r):
    nodes, tris, shade = r.bvh_export()
    uv = r.bvh_export_uv()
    n4, d4 = r.bvh_export4()
    return [nodes.tobytes(), tris.tobytes(), shade.tobytes(), None if uv is None else uv.tobytes(), n4.tobytes(), d4,
            r.bvh_export4q().tobytes(), r.bvh_export_planes4q().tobytes(), r.bvh_info()]


def _references(pkg, oracle, sc, point_ref, list_ref):
    """brute force over the scene, computed once and shared: frames in every mode, closest hits, occlusion, hit counts, lists,
    closest points and occupancy; the winding points and the records by gid (winding_checks.assert_winding computes its own
    expectations from them and from the exported tree)"""
    if "refs" not in sc:
        P = _oracle_scene(oracle, sc)
        recs, rays, cam = P.tris(), sc["rays"], sc["camera"]
        pts = _points(pkg, sc, 1000, 5)
        poses = _pose_refs(oracle, sc)  # (leaves the oracle's default path parameters behind)
        oracle.set_path_params(*PATH_PARAMS)
        sc["refs"] = {
            "poses": poses, "shaded_cache": {},
            "frames": {m: P.render(cam["position"], cam["matrix"], m, W, H, brute_force=True) for m in ALL_MODES},
            "trace": oracle.trace_rays(P, rays, brute_force=True), "occluded": oracle.occluded_rays(P, rays, brute_force=True)["occluded"],
            "count": pq.ref_count(point_ref, recs, rays), "lists": lh.ref_list(list_ref, recs, rays), "points": pts,
            "closest": pq.ref_closest(point_ref, recs, pts), "occupancy": pq.ref_occupancy(point_ref, recs, pts),
            "winding_points": wc.points_for(sc, seed=7), "records": _records(pkg, sc["meshes"])}
        for k in ("trace", "lists", "closest"):
            _assert_none_inert(sc, sc["refs"][k]["inst"], sc["refs"][k]["prim"], k)
    return sc["refs"]


def _device_queries(r, rays, pts, total):
    """the device forms of the six queries on torch tensors, read back as numpy arrays"""
    import torch
    n, m = len(rays), len(pts)
    d_rays, d_pts = torch.from_numpy(np.ascontiguousarray(rays)).cuda(), torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    f32, i32 = dict(dtype=torch.float32, device="cuda"), dict(dtype=torch.int32, device="cuda")
    tr = {"t": torch.zeros(n, **f32), "uv": torch.zeros((n, 2), **f32), "inst": torch.zeros(n, **i32), "prim": torch.zeros(n, **i32)}
    occ = torch.zeros(n, dtype=torch.bool, device="cuda")
    cnt = torch.zeros(n, **i32)
    cp = {"dist": torch.zeros(m, **f32), "point": torch.zeros((m, 3), **f32), "uv": torch.zeros((m, 2), **f32),
          "inst": torch.zeros(m, **i32), "prim": torch.zeros(m, **i32)}
    inside = torch.zeros(m, dtype=torch.bool, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    cap = max(total, 1)
    ls = {"t": torch.zeros(cap, **f32), "uv": torch.zeros((cap, 2), **f32), "inst": torch.zeros(cap, **i32), "prim": torch.zeros(cap, **i32)}
    torch.cuda.synchronize()
    r.trace_rays_device(n, d_rays.data_ptr(), *[tr[k].data_ptr() for k in ("t", "uv", "inst", "prim")])
    r.occluded_device(n, d_rays.data_ptr(), occ.data_ptr())
    r.count_hits_device(n, d_rays.data_ptr(), cnt.data_ptr())
    r.closest_points_device(m, d_pts.data_ptr(), *[cp[k].data_ptr() for k in ("dist", "point", "uv", "inst", "prim")])
    r.occupancy_device(m, d_pts.data_ptr(), inside.data_ptr())
    got_total = r.list_hits_device(n, d_rays.data_ptr(), off.data_ptr(), cap, *[ls[k].data_ptr() for k in ("t", "uv", "inst", "prim")], total=True)
    r.synchronize()
    torch.cuda.synchronize()
    host = lambda d: {k: (v.cpu().numpy().view(np.uint32) if v.dtype == torch.int32 else v.cpu().numpy()) for k, v in d.items()}  # noqa: E731
    lists = {k: v[:total] for k, v in host(ls).items()}
    lists["offsets"] = off.cpu().numpy()
    assert got_total == total
    return {"trace": host(tr), "occluded": occ.cpu().numpy(), "count": cnt.cpu().numpy().view(np.uint32), "closest": host(cp),
            "occupancy": inside.cpu().numpy(), "lists": lists}


def _assert_queries(got, refs, what):
    for k in ("inst", "prim"):
        np.testing.assert_array_equal(got["trace"][k], refs["trace"][k], err_msg="%s: closest hit %s" % (what, k))
    for k in ("t", "uv"):
        assert np.array_equal(_bits(got["trace"][k]), _bits(refs["trace"][k])), "%s: closest hit %s" % (what, k)
    np.testing.assert_array_equal(np.asarray(got["occluded"], dtype=np.uint8), refs["occluded"], err_msg="%s: occlusion" % what)
    np.testing.assert_array_equal(got["count"], refs["count"], err_msg="%s: hit counts" % what)
    if len(refs["lists"]["t"]):
        lh._assert_list_equal(got["lists"], refs["lists"], what + ": lists")
    else:  # (no ray crosses anything: the offsets are all there is to compare)
        np.testing.assert_array_equal(np.asarray(got["lists"]["offsets"], dtype=np.int64), refs["lists"]["offsets"], err_msg=what + ": lists")
        assert all(len(got["lists"][k]) == 0 for k in lh.KEYS), what + ": lists"
    pq._assert_closest_equal(got["closest"], refs["closest"], what + ": closest points")
    np.testing.assert_array_equal(np.asarray(got["occupancy"], dtype=bool), refs["occupancy"], err_msg="%s: occupancy" % what)


def _assert_frame(got, ref, what, rgb=True):
    for k in ("hit_inst", "hit_prim", "rgba8"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (what, k))
    assert np.array_equal(_bits(got["hit_t"]), _bits(ref["hit_t"])), what + " hit_t"
    if rgb:
        assert np.array_equal(got["rgb"], ref["rgb"], equal_nan=True), what + " rgb"


def _check_gpu(pkg, oracle, wref, r, sc, refs, what, same_tree=None):
    """the scene r holds is sc: its wide and quantised trees are the oracle's collapse of its binary tree, its frames in every
    mode (both path pipelines) equal the oracle's over that tree with the fetch counters, and the brute-force frames; the host
    and device forms of the six queries equal their brute-force references; camera_rays through shade_rays and path_rays give
    the brute-force frames, frame_guides the frames' surfaces, and shade_rays / path_rays on the generic rays and on the poses
    their brute-force references (tests/shaded_query_checks.py); the winding numbers and the moment table pass
    winding_checks.assert_winding.  same_tree: an oracle scene known to hold the same tree (it
    keeps uvs, which OracleScene.set_bvh drops)."""
    nodes, tris, shade = r.bvh_export()
    S = same_tree
    if S is None:
        S = _oracle_scene(oracle, sc)
        S.set_bvh(nodes, tris, shade)
    n4, d4 = r.bvh_export4()
    assert n4.tobytes() == S.nodes4().tobytes() and d4 == S.depth4, what
    assert r.bvh_export4q().tobytes() == S.nodes4q().tobytes(), what
    assert np.all(np.isfinite(spec.child_boxes(nodes))), what
    _assert_finite_triangles_are_contained(sc, S, what)
    over_tree = same_tree is not None or not sc.get("textures")
    cam = sc["camera"]
    for mode in ALL_MODES:
        r.change_shading_mode(mode)
        for pipeline in ((0, 1) if mode == 200 else (0,)):
            r.set_option("path_pipeline", pipeline)
            r.set_counting(True)
            got = r.render_frame(W, H)
            r.set_counting(False)
            r.set_option("path_pipeline", 0)
            tag = "%s mode %d pipeline %d" % (what, mode, pipeline)
            _assert_frame(got, refs["frames"][mode], tag + " vs brute force")
            if over_tree:
                ref = S.render(cam["position"], cam["matrix"], mode, W, H)
                _assert_frame(got, ref, tag + " vs the oracle over the same tree")
                if pipeline == 0:
                    assert (got["stats"]["nodes_visited"], got["stats"]["tris_tested"]) == (ref["stats"]["nodes_visited"], ref["stats"]["tris_tested"]), tag
    rays, pts = sc["rays"], refs["points"]
    host = {"trace": r.trace_rays(rays), "occluded": r.occluded(rays), "count": r.count_hits(rays), "lists": r.list_hits(rays),
            "closest": r.closest_points(pts), "occupancy": r.occupancy(pts)}
    _assert_queries(host, refs, what + " (host forms)")
    _assert_queries(_device_queries(r, rays, pts, int(refs["lists"]["offsets"][-1])), refs, what + " (device forms)")
    # shade_rays, path_rays and frame_guides: the frame's camera_rays, the generic rays and the poses
    scene = {"meshes": sc["meshes"], "materials": sc["materials"], "textures": sc.get("textures")}
    sq.frame_records_equal_frames(r, refs["frames"], W, H, PATH_PARAMS, what, scene=scene, texture_color=oracle.texture_color,
                                  cache=refs["shaded_cache"], world={"oracle": oracle, "camera": (cam["position"], cam["matrix"]), "lights": sc["lights"], "path_held": PATH_PARAMS})
    sq.arbitrary_records_equal_trace(r, rays, refs["trace"], what, meshes=sc["meshes"])
    sq.pose_records_equal_oracle(r, refs["poses"], what, meshes=sc["meshes"])
    wc.assert_winding(pkg, wref, r, sc, refs["records"], refs["winding_points"], what)
    return nodes, tris, shade


def _expected_tree(pkg, oracle, sc, tree):
    """(nodes, tris, shade, oracle scene holding that tree or None) a fresh upload of sc over `tree` must give"""
    if tree == "ploc":
        nodes, tris, shade, _ = _ploc_tree(pkg, oracle, sc)
        return nodes, tris, shade, None
    O = _oracle_scene(oracle, sc, build_mode=0 if tree == "sah" else 1)
    return O.nodes(), O.tris(), O.shade(), O


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", _GPU_PARAMS, ids=_GPU_IDS)
def test_uploads_of_poisoned_scenes(pkg, oracle, point_ref, list_ref, wref, renderer, defaults, case, name, kind):
    r, sc = renderer, case(name, kind)
    refs = _references(pkg, oracle, sc, point_ref, list_ref)
    for tree in TREES:
        what = "%s %s %s" % (name, kind, tree)
        _upload(r, sc, tree)  # (PLOC included: the upload returns CRT_OK and the scene is kept)
        nodes, tris, shade = r.bvh_export()
        want = _expected_tree(pkg, oracle, sc, tree)
        assert nodes.tobytes() == want[0].tobytes(), what + ": binary nodes"
        assert tris.tobytes() == want[1].tobytes() and shade.tobytes() == want[2].tobytes(), what + ": records"
        _check_gpu(pkg, oracle, wref, r, sc, refs, what, same_tree=want[3])


def _assert_vertices(r, meshes, what):
    for i, m in enumerate(meshes):
        got = r.mesh_vertices(i)[0]
        assert np.array_equal(_bits(got), _bits(np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3))), "%s: mesh_vertices(%d)" % (what, i)


def _assert_refitted(pkg, r, shape, sc, what):
    """the tree kept its shape; its boxes are the numpy refit's and its records a fresh build's, by gid"""
    nodes, tris, shade = r.bvh_export()
    assert np.array_equal(nodes["left"], shape["left"]) and np.array_equal(nodes["right"], shape["right"]), what
    want = _numpy_refit(nodes, tris, sc["meshes"])
    got = np.stack([np.stack([np.stack([nodes[s + a + "0"] for a in "xyz"], 1), np.stack([nodes[s + a + "1"] for a in "xyz"], 1)], 1)
                    for s in "lr"], 1)
    assert np.array_equal(_bits(got), _bits(want)), what + ": refitted boxes"
    assert tris[np.argsort(tris["gid"], kind="stable")].tobytes() == _records(pkg, sc["meshes"]).tobytes(), what + ": records"


def _dynamic_round_trip(pkg, oracle, wref, point_ref, list_ref, r, builder, clean, sc, poison, heal, what):
    """upload clean; poison() + refit; heal() + refit; poison() + rebuild; heal() + rebuild.  After every step the checks of
    _check_gpu hold and crt_mesh_vertices returns the traced values bit for bit; the healed scene equals the upload, its
    exact-mode winding numbers included."""
    tree = "lbvh" if builder == LBVH else "ploc"
    refs, clean_refs = _references(pkg, oracle, sc, point_ref, list_ref), _references(pkg, oracle, clean, point_ref, list_ref)
    _upload(r, clean, tree, dynamic=True)
    fresh = _export(r)
    shape = r.bvh_export()[0]
    wpts = clean_refs["winding_points"]
    w_fresh = _bits(r.winding_numbers(wpts, 0.0))
    poison()
    r.refit()
    _assert_vertices(r, sc["meshes"], what + " refit")
    _assert_refitted(pkg, r, shape, sc, what + " refit")
    _check_gpu(pkg, oracle, wref, r, sc, refs, what + " refit")
    heal()
    r.refit()
    _assert_vertices(r, clean["meshes"], what + " healed by a refit")
    assert _export(r) == fresh, what + ": healed by a refit"
    wc.assert_winding(pkg, wref, r, clean, clean_refs["records"], wpts, what + " healed by a refit")
    np.testing.assert_array_equal(_bits(r.winding_numbers(wpts, 0.0)), w_fresh, err_msg=what + ": exact-mode winding numbers healed by a refit")
    poison()
    r.rebuild()  # (PLOC included: the rebuild returns CRT_OK -- the binding raises otherwise -- and the scene is kept)
    _assert_vertices(r, sc["meshes"], what + " rebuild")
    nodes, tris, shade = r.bvh_export()
    want = _expected_tree(pkg, oracle, sc, tree)
    assert nodes.tobytes() == want[0].tobytes() and tris.tobytes() == want[1].tobytes() and shade.tobytes() == want[2].tobytes(), what + " rebuild"
    _check_gpu(pkg, oracle, wref, r, sc, refs, what + " rebuild")
    heal()
    r.rebuild()
    assert _export(r) == fresh, what + ": healed by a rebuild"
    _check_gpu(pkg, oracle, wref, r, clean, clean_refs, what + " healed")
    np.testing.assert_array_equal(_bits(r.winding_numbers(wpts, 0.0)), w_fresh, err_msg=what + ": exact-mode winding numbers healed by a rebuild")


def _clean_scene(sc):
    clean = {k: v for k, v in sc.items() if k not in ("meshes", "clean", "inert", "rays", "refs", "poses")}
    clean["meshes"] = sc["clean"]
    clean["inert"] = [np.zeros(len(np.asarray(m["triangles"]).reshape(-1, 3)), bool) for m in sc["clean"]]
    clean["rays"] = sc["rays"]
    return clean


_DYNAMIC = [("probe100", "nan"), ("heightfield_leaf", "mix"), ("icosphere_pole", "+inf"), ("tiny3", "-inf"), ("tiny5", "nan"),
            ("cornell_whole_mesh", "mix"), ("all_inert", "nan")]


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [LBVH, PLOC], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("name,kind", _DYNAMIC, ids=["%s-%s" % p for p in _DYNAMIC])
def test_vertex_updates_poison_and_heal_a_dynamic_scene(pkg, oracle, point_ref, list_ref, wref, renderer, defaults, case, name, kind, builder):
    import torch
    r, sc = renderer, case(name, kind)
    clean = _cache.setdefault((name, "clean"), _clean_scene(sc))
    changed = [i for i, (a, b) in enumerate(zip(sc["meshes"], sc["clean"])) if a["vertices"] is not b["vertices"]]

    def send(meshes):
        for k, i in enumerate(changed):  # the host form and the device form in turn
            v = np.ascontiguousarray(meshes[i]["vertices"], dtype=np.float32)
            r.update_vertices(i, v if (k + builder) % 2 == 0 else torch.from_numpy(v).cuda())

    _dynamic_round_trip(pkg, oracle, wref, point_ref, list_ref, r, builder, clean, sc, lambda: send(sc["meshes"]), lambda: send(clean["meshes"]),
                        "%s %s builder %d" % (name, kind, builder))


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [LBVH, PLOC], ids=["lbvh", "ploc"])
def test_a_transform_that_overflows_makes_the_mesh_inert(pkg, scenes, oracle, point_ref, list_ref, wref, renderer, defaults, builder):
    """finite rest vertices, a finite non-singular transform, products beyond FLT_MAX: every world x of the mesh is +inf"""
    from test_dynamic_geometry import _apply
    probe = _probe_mesh(60, 21)
    probe["vertices"] = (probe["vertices"] * np.float32([0.1, 1, 1]) + np.float32([3, 0, 0])).astype(np.float32)  # x in [2.4, 3.6]
    key = ("overflow", "clean")
    if key not in _cache:
        clean = _scene([_icosphere(scenes, 2), probe], cam=(0.0, 0.0, 9.0))
        clean["inert"] = _inert_mask(clean["meshes"])
        clean["rays"] = _rays(clean, N_RAYS, seed=77)
        M = np.float32([[2e38, 0, 0, 0], [0, 1, 0, 0.5], [0, 0, 1, -0.25]])
        with np.errstate(over="ignore"):
            moved = [clean["meshes"][0], dict(probe, vertices=_apply(M, probe["vertices"]))]
        sc = dict(clean, meshes=moved, inert=_inert_mask(moved), clean=clean["meshes"])
        assert sc["inert"][1].all() and np.isposinf(moved[1]["vertices"][:, 0]).all() and np.isfinite(moved[1]["vertices"][:, 1:]).all()
        _cache[key], _cache[("overflow", "moved")] = clean, (sc, M)
    clean, (sc, M) = _cache[key], _cache[("overflow", "moved")]
    _dynamic_round_trip(pkg, oracle, wref, point_ref, list_ref, renderer, builder, clean, sc, lambda: renderer.set_mesh_transform(1, M),
                        lambda: renderer.set_mesh_transform(1, None), "overflowing transform, builder %d" % builder)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [LBVH, PLOC], ids=["lbvh", "ploc"])
def test_rebuild_of_an_uploaded_poisoned_scene_reproduces_the_upload(pkg, renderer, defaults, case, builder):
    r = renderer
    for name, kind in (("probe2000", "nan"), ("dragon_shared_vertex", "-inf"), ("tiny4", "mix"), ("all_inert", "+inf")):
        sc = case(name, kind)
        _upload(r, sc, "lbvh" if builder == LBVH else "ploc", dynamic=True)
        before = _export(r)
        r.rebuild()
        assert _export(r) == before, "%s %s" % (name, kind)
        _assert_vertices(r, sc["meshes"], "%s %s" % (name, kind))
