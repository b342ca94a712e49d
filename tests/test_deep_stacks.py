"""Stacks past the LDS part.  Every traversal kernel -- the frame kernels, the query kinds, and among them the two with phase
machines of their own, mode 120 (ao_kernels.hip: closest hit, shadow rays, K any-hit probes) and mode 150 (whitted_kernels.hip:
closest hit, turn, closest hit, shadow rays), which reset the stack by hand between phases -- keeps the first `stack_entries`
entries (default 16) of a lane's stack in LDS
and the deeper ones in the lane's slice of a global spill arena, which the host sizes as 3 * depth4 + 1 - stack_entries entries
(api_frames.cpp runRender and api_queries.cpp beginQuery; twice as many ints for the closest-point kernel's pairs).  The scenes of
tests/deep_stack_scenes.py put lanes up to 60 entries deep -- one entry short of that bound -- in every walk class (closest hit, any
hit, the no-cull walks of the counts and lists, closest point) over every builder's tree, so a wrong stride, a stale depth4 or a
wrong slice index makes lanes overwrite each other's pending nodes and the comparisons below fail.  A mirror in front of chain B
sends mode 150's mirrored rays 27 to 35 entries deep into it and the shadow rays behind that turn as deep back through it; the
occlusion probes mode 120 draws on the plate hold 26 to 57.

The CPU tests prove that the GPU tests cannot pass vacuously: the depths come from the oracle's own walk (oracle_set_stack_output,
oracle_debug_max_sp) or from plain float64 models of the walks the oracle does not have, never from the product kernels.  The GPU
tests then hold frames, queries, split packets, batches, tile shares and contexts whose depth4 moves to the existing references, at
LDS parts of 0 (= 16), 1, 5 and 32 entries, counting off and on.

Winding numbers in exact mode enter or push every non-empty child, whatever the geometry: over chain A a lane holds 36 (SAH),
50 (LBVH) and 28 (PLOC) entries, over the plate and chain B 27, 57 and 30 (tests/test_winding_checks.py measures them from the
trees alone).  tests/winding_checks.py's assert_winding holds them to brute force, to the reference's walk and to the moment
table in float64 here, and after every move of depth4, where the level launches of the moment table take their count from it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ambient_checks as A  # noqa: E402
import deep_stack_scenes as D  # noqa: E402
import path_rays_helpers as PH  # noqa: E402
import path_reference as PR  # noqa: E402
import ploc_reference as spec  # noqa: E402
import shaded_query_checks as sq  # noqa: E402
import test_list_hits as tl  # noqa: E402
import test_point_queries as tp  # noqa: E402
import test_ray_queries as tr  # noqa: E402
import winding_checks as wc  # noqa: E402
from test_list_hits import ref as list_ref  # noqa: E402,F401  (fixture: tests/list_hits_reference.c)
from test_point_queries import ref as point_ref  # noqa: E402,F401  (fixture: tests/point_reference.c)
from winding_checks import wref  # noqa: E402,F401  (fixture: tests/winding_reference.c)

MISS = 0xFFFFFFFF
TREES = tp.TREES  # sah / lbvh / ploc -> the upload options
BUILDERS = tuple(TREES)
STACK_ENTRIES = (0, 1, 5, 32)  # 0 = the default, 16
LDS_DEFAULT, LDS_MOST = 16, 32  # the default LDS part and kStackEntries, the largest one
PATH = (2, 2, 77)  # spp, bounces, seed of the mode-200 frames
SIZES = {"chain": (48, 32), "shadow": (48, 32)}
MODES = {"chain": (3,), "shadow": (3, 100, 200)}  # chain A: deep camera rays; the plate and chain B: deep shadow and bounce rays
N_APEX = 512
DEEP_AO = ((5, 0, 1), (64, 0, 0), (64, 50, 1))  # (ao_samples, ao_radius, ao_sky): at K = 64 lanes wait and start in groups while others are deep
ROUTE_AO = ((5, 0, 0), (5, 50, 1))
LAUNCH_COPIES = 129  # copies of a 48 x 32 frame's records: 198144, which "path_pass_paths" = 65536 splits into four launches


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scenes():
    return {"chain": D.chain_a(), "shadow": D.plate_and_chain_b()}


def oracle_tree(pkg, oracle, sc, builder):
    """the oracle over the tree `builder` gives: its own SAH and LBVH builds, tests/ploc_reference.py's PLOC tree"""
    if builder != "ploc":
        return oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], build_mode=1 if builder == "lbvh" else 0)
    L = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], build_mode=1)
    order = L.tris()["gid"].astype(np.int64)
    nodes, gids, _, _ = spec.build(spec.tri_boxes(sc["meshes"]), order, pkg.NODE_DTYPE)
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))
    pick = inv[gids]
    L.set_bvh(nodes, L.tris()[pick], L.shade()[pick])
    return L


def _world(oracle, sc, O=None):
    """what tests/shaded_query_checks.py needs for the references of modes 120 and 150; O: the oracle over the tree the context holds"""
    out = {"oracle": oracle, "camera": (sc["camera"]["position"], sc["camera"]["matrix"]), "lights": sc["lights"]}
    if O is not None:
        out["O"] = O
    return out


def _frame(oracle, O, cam, mode, w, h, brute_force=False, depth=False, path=PATH):
    """an oracle frame (mode 200: PATH) and, with depth, the deepest stack of every pixel's rays; the frame then also holds
    "secondary_depth", that of the pixel's shadow and bounce rays alone"""
    d, d2 = np.zeros((h, w), dtype=np.uint32), np.zeros((h, w), dtype=np.uint32)
    if depth:
        oracle.lib().oracle_set_stack_output(d.ctypes.data_as(C.c_void_p))
        oracle.lib().oracle_set_stack_output2(d2.ctypes.data_as(C.c_void_p))
    oracle.set_path_params(*path)
    try:
        f = O.render(cam["position"], cam["matrix"], mode, w, h, brute_force=brute_force)
    finally:
        oracle.set_path_params(4, 3, 1234)
        oracle.lib().oracle_set_stack_output(None)
        oracle.lib().oracle_set_stack_output2(None)
    if depth:
        f["secondary_depth"] = d2
    return (f, d) if depth else f


def camera_records(pkg, oracle, sc, w, h):
    cam = sc["camera"]
    return pkg.make_rays(np.asarray(cam["position"], dtype=np.float32), tr._camera_rays(oracle, cam, w, h), tmin=D.TMIN, tmax=D.TMAX)


def query_rays(pkg, oracle, sc, w, h):
    """the scene's camera rays, apex rays into chain A, then N_APEX apex rays into chain B (tmin = 0, tmax = inf: every plate of
    the chain is crossed)"""
    return np.ascontiguousarray(np.concatenate([camera_records(pkg, oracle, sc, w, h), D.apex_rays(pkg.make_rays, N_APEX // 2, seed=4, towards=-1.0),
                                                D.apex_rays(pkg.make_rays, N_APEX, seed=3)]))


def query_depths(oracle, O, rays, any_hit):
    """deepest stack of every record in the oracle's own closest-hit or any-hit walk, one record at a time on this thread"""
    L = oracle.lib()
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    out = np.zeros(len(rays), dtype=np.int64)
    for i in range(len(rays)):
        L.oracle_debug_max_sp(1)
        L.oracle_query_rays(O.h, 1, rays[i].ctypes.data, 0, int(any_hit), *([None] * 7))
        out[i] = L.oracle_debug_max_sp(1)
    return out


# ---- plain float64 models of the walks the oracle does not have

def _children(n4, i):
    nd = n4[i]
    box = np.stack([nd["minx"], nd["miny"], nd["minz"], nd["maxx"], nd["maxy"], nd["maxz"]], 1).astype(np.float64)  # (4, 6)
    return box, [int(r) for r in nd["ref"]]


def _pierced(box, o, inv, tmin, tmax):
    """the ray crosses the full-precision box with a clear margin: every axis' entry lies a relative 1e-9 before every OTHER
    axis' exit and before tmax, and every exit as far behind tmin (an axis is compared with itself exactly: a flat box is one
    point of the ray).  The kernels test the quantised box, which contains this one, with conservatively rounded slabs
    (DESIGN.md section 3), so they push every child counted here"""
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = (box[0:3] - o) * inv, (box[3:6] - o) * inv
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    if np.isnan(lo).any() or np.isnan(hi).any():
        return False
    margin = lambda x, y: 1e-9 * (abs(x) + abs(y)) if np.isfinite(x) and np.isfinite(y) else 0.0  # noqa: E731
    for i in range(3):
        for j in range(3):
            if i != j and not lo[i] + margin(lo[i], hi[j]) <= hi[j]:
                return False
        if not (lo[i] + margin(lo[i], tmax) <= tmax and tmin + margin(tmin, hi[i]) <= hi[i]):
            return False
    return True


def no_cull_depth(n4, ray):
    """Lower bound of the stack a lane of the every-hit walk (counts, lists, occupancy: query.hip.h everyHitIteration) holds on
    `ray`: the walk takes the first hit child in slot order, pushes the other hit children last slot first, and never ends
    early.  Walking only the children _pierced counts visits a subsequence of the kernel's nodes, with a subset of its pending
    entries at each of them."""
    o, d = ray[0:3].astype(np.float64), ray[4:7].astype(np.float64)
    with np.errstate(divide="ignore"):
        inv = 1.0 / d
    tmin, tmax = float(ray[3]), float(ray[7])
    stack, cur, deepest = [], 0, 0
    while True:
        if cur >= 0:
            box, refs = _children(n4, cur)
            hit = [k for k in range(4) if refs[k] != -1 and _pierced(box[k], o, inv, tmin, tmax)]
            if hit:
                stack.extend(refs[k] for k in reversed(hit[1:]))
                deepest = max(deepest, len(stack))
                cur = refs[hit[0]]
                continue
        if not stack:
            return deepest
        cur = stack.pop()


def closest_point_depth(n4, p, cur=0):
    """Entries a closest-point lane with rmax = +inf holds at the first leaf of its nearest-first descent, at least: at every
    node every non-empty child is within the bound, the nearest becomes current and the others are pushed.  The kernel measures
    the quantised boxes, so a child counts as possibly nearest when its full-precision box is within two steps of the node's
    quantisation grid of the nearest one (the coincident copies of a plate tie exactly), and the descent that holds least is
    taken."""
    p = np.asarray(p, dtype=np.float64)
    box, refs = _children(n4, cur)
    live = [k for k in range(4) if refs[k] != -1]
    gap = np.maximum(np.maximum(box[:, 0:3] - p, p - box[:, 3:6]), 0.0)
    dist = np.sqrt((gap * gap).sum(axis=1))
    step = (box[live, 3:6].max(axis=0) - box[live, 0:3].min(axis=0)) / 255.0
    near = [k for k in live if dist[k] <= min(dist[live]) + 2.0 * np.linalg.norm(step)]
    return len(live) - 1 + min(closest_point_depth(n4, p, refs[k]) if refs[k] >= 0 else 0 for k in near)


def apex_points(pkg, n, seed):
    """points just in front of chain A's apex, outside every box: the group of the smallest plates is the nearest at every node"""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-0.002, 0.002, n), rng.uniform(-0.002, 0.002, n), rng.uniform(0.001, 0.004, n)], 1).astype(np.float32)
    return pkg.make_points(xyz, rmax=np.inf)


OCCUPANCY_DIR0 = np.float32([0.730209529, 0.288103759, 0.619508088])  # CRT_OCCUPANCY_DIR0 (include/crt_hip.h)


def occupancy_points(pkg, n, seed):
    """points whose first occupancy ray passes the apex and runs on into chain B's boxes"""
    rng = np.random.default_rng(seed)
    xyz = (-OCCUPANCY_DIR0 * rng.uniform(1e-4, 1e-3, (n, 1)) + rng.uniform(-1e-5, 1e-5, (n, 3))).astype(np.float32)
    return pkg.make_points(xyz, rmax=np.inf)


# ---- the references: computed once, never changed

@pytest.fixture(scope="module")
def refs(pkg, oracle):
    """per scene and builder: the oracle over that tree, its frames (tree walk and brute force) with the per-pixel stack depth,
    and the query rays"""
    out = {}
    for name, sc in _scenes().items():
        w, h = SIZES[name]
        entry = {"scene": sc, "rays": query_rays(pkg, oracle, sc, w, h), "trees": {}, "cache": {}}
        for b in BUILDERS:
            O = oracle_tree(pkg, oracle, sc, b)
            t = {"oracle": O, "depth4": O.depth4, "frames": {}, "depth": {}, "brute": {}}
            for mode in MODES[name]:
                t["frames"][mode], t["depth"][mode] = _frame(oracle, O, sc["camera"], mode, w, h, depth=True)
                t["brute"][mode] = _frame(oracle, O, sc["camera"], mode, w, h, brute_force=True)
            entry["trees"][b] = t
        out[name] = entry
    yield out
    for entry in out.values():
        for t in entry["trees"].values():
            t["oracle"].close()


@pytest.fixture(scope="module")
def mirror_refs(pkg, oracle):
    """the plate as a mirror in front of chain B: the oracle over every builder's tree"""
    sc = D.mirror_and_chain_b()
    out = {"scene": sc, "trees": {b: oracle_tree(pkg, oracle, sc, b) for b in BUILDERS}, "cache": {}}
    yield out
    for O in out["trees"].values():
        O.close()


def _walk_equals_brute_force(got, brute, what):
    """inst, prim and the bits of t, on every ray: none is left out as a boundary ray"""
    for k in ("hit_inst", "hit_prim") if "hit_inst" in got else ("inst", "prim"):
        np.testing.assert_array_equal(got[k], brute[k], err_msg="%s: %s, tree walk against brute force" % (what, k))
    k = "hit_t" if "hit_t" in got else "t"
    np.testing.assert_array_equal(_bits(got[k]), _bits(brute[k]), err_msg="%s: t, tree walk against brute force" % what)


# ---- CPU: the scenes do what the GPU tests need

def test_closest_hit_walks_leave_the_lds_part(oracle, refs):
    """chain A, mode 3 and trace_rays on the camera rays: over every builder's tree some lane holds more than 16 entries, over the
    LBVH tree more than 32 and within 2 of 3 * depth4 -- the host's bound 3 * depth4 + 1 is tight"""
    e = refs["chain"]
    n_cam = SIZES["chain"][0] * SIZES["chain"][1]
    deepest = {}
    for b, t in e["trees"].items():
        frame_deepest = int(t["depth"][3].max())
        qd = query_depths(oracle, t["oracle"], e["rays"][:n_cam], any_hit=False)
        print("chain A, %s: depth4 %d, bound %d, deepest frame lane %d, deepest trace_rays lane %d, pixels deeper than 16: %d" % (
            b, t["depth4"], 3 * t["depth4"] + 1, frame_deepest, int(qd.max()), int((t["depth"][3] > LDS_DEFAULT).sum())))
        np.testing.assert_array_equal(qd, t["depth"][3].reshape(-1), err_msg="a camera ray is as deep as a record as in the frame")
        assert frame_deepest > LDS_DEFAULT, b
        assert frame_deepest <= 3 * t["depth4"] + 1, b
        deepest[b] = frame_deepest
        _walk_equals_brute_force(t["frames"][3], t["brute"][3], "chain A, " + b)
        got, brute = oracle.trace_rays(t["oracle"], e["rays"]), oracle.trace_rays(t["oracle"], e["rays"], brute_force=True)
        _walk_equals_brute_force(got, brute, "chain A records, " + b)
        assert (got["inst"] != MISS).sum() > 100 + N_APEX // 2, "the camera and the apex rays see chain A"
    assert max(deepest.values()) > LDS_MOST
    assert deepest["lbvh"] >= 3 * refs["chain"]["trees"]["lbvh"]["depth4"] - 2


def test_any_hit_walks_leave_the_lds_part(oracle, refs):
    """a plate and chain B: the camera rays hold nothing, the shadow rays of the mode-100 frame (measured apart from the camera
    rays) and occluded_rays on the apex rays into chain B are deep"""
    e = refs["shadow"]
    deepest = {}
    for b, t in e["trees"].items():
        assert int(t["depth"][3].max()) == 0, b
        assert t["frames"][100]["stats"]["rays_shadow"] > 100
        shadow = int(t["frames"][100]["secondary_depth"].max())
        qd = query_depths(oracle, t["oracle"], e["rays"], any_hit=True)
        print("plate and chain B, %s: depth4 %d, deepest shadow ray %d, deepest occluded_rays lane %d (records deeper than 16: %d)" % (
            b, t["depth4"], shadow, int(qd.max()), int((qd > LDS_DEFAULT).sum())))
        assert shadow > LDS_DEFAULT and int(qd.max()) > LDS_DEFAULT, b
        deepest[b] = min(shadow, int(qd.max()))
        for mode in (3, 100):
            _walk_equals_brute_force(t["frames"][mode], t["brute"][mode], "plate and chain B, mode %d, %s" % (mode, b))
        got, brute = oracle.occluded_rays(t["oracle"], e["rays"]), oracle.occluded_rays(t["oracle"], e["rays"], brute_force=True)
        np.testing.assert_array_equal(got["occluded"], brute["occluded"])
        assert got["occluded"][-N_APEX:].all()
        _walk_equals_brute_force(oracle.trace_rays(t["oracle"], e["rays"]), oracle.trace_rays(t["oracle"], e["rays"], brute_force=True),
                                 "plate and chain B records, " + b)
    assert max(deepest.values()) > LDS_MOST


def test_shadow_and_bounce_rays_of_path_frames_leave_the_lds_part(oracle, refs):
    """the plate and chain B, mode 200: the rays that follow the camera ray (bounces off the plate into chain B, nearest child
    first, and their shadow rays) are deep, as are closest-hit records from the apex into chain B"""
    e = refs["shadow"]
    w, h = SIZES["shadow"]
    deepest = {}
    for b, t in e["trees"].items():
        f = t["frames"][200]
        secondary = int(f["secondary_depth"].max())
        qd = query_depths(oracle, t["oracle"], e["rays"][-N_APEX:], any_hit=False)
        print("plate and chain B, %s: depth4 %d, mode 200: deepest shadow or bounce ray %d (pixels deeper than 16: %d), camera rays %d; "
              "closest-hit apex records %d" % (b, t["depth4"], secondary, int((f["secondary_depth"] > LDS_DEFAULT).sum()),
                                               int(t["depth"][3].max()), int(qd.max())))
        assert f["stats"]["rays_primary"] > PATH[0] * w * h and f["stats"]["rays_shadow"] > 100, "bounce and shadow rays were traced"
        assert LDS_DEFAULT < secondary <= 3 * t["depth4"] + 1 and int(qd.max()) > LDS_DEFAULT, b
        _walk_equals_brute_force(f, t["brute"][200], "plate and chain B, mode 200, " + b)
        deepest[b] = min(secondary, int(qd.max()))
    assert max(deepest.values()) > LDS_MOST


def test_no_cull_walks_leave_the_lds_part(pkg, refs):
    """counts and lists walk without culling in slot order, and so do the three rays of an occupancy query: the float64 model's
    lower bound on the apex rays into chain B (every 8th ray: the model is plain Python) and on the first occupancy ray of
    occupancy_points"""
    e = refs["shadow"]
    pts = occupancy_points(pkg, 32, seed=8)
    occ_rays = pkg.make_rays(pts[:, 0:3], np.tile(OCCUPANCY_DIR0, (len(pts), 1)), tmin=0.0, tmax=np.inf)
    deepest = {}
    for b, t in e["trees"].items():
        n4 = t["oracle"].nodes4()
        d = np.array([no_cull_depth(n4, ray) for ray in e["rays"][-N_APEX::8]])
        o = np.array([no_cull_depth(n4, ray) for ray in occ_rays])
        print("plate and chain B, %s: depth4 %d, no-cull walk holds at least %d entries on the apex rays (deeper than 16: %d of %d), "
              "%d on the occupancy rays (deeper than 16: %d of %d)" % (b, t["depth4"], int(d.max()), int((d > LDS_DEFAULT).sum()), len(d),
                                                                      int(o.max()), int((o > LDS_DEFAULT).sum()), len(o)))
        assert int(d.max()) > LDS_DEFAULT and int(o.max()) > LDS_DEFAULT, b
        assert max(int(d.max()), int(o.max())) <= 3 * t["depth4"] + 1
        deepest[b] = min(int(d.max()), int(o.max()))
    assert max(deepest.values()) > LDS_MOST


def test_closest_point_walks_leave_the_lds_part(pkg, refs):
    """rmax = +inf: every non-empty child of every node of the descent is pending, whatever the geometry"""
    pts = apex_points(pkg, 64, seed=5)
    deepest = {}
    for b, t in refs["chain"]["trees"].items():
        n4 = t["oracle"].nodes4()
        d = np.array([closest_point_depth(n4, p[0:3]) for p in pts])
        print("chain A, %s: depth4 %d, a closest-point lane holds at least %d .. %d entries at its first leaf" % (b, t["depth4"], int(d.min()), int(d.max())))
        assert int(d.max()) > LDS_DEFAULT and int(d.max()) <= 3 * t["depth4"] + 1, b
        deepest[b] = int(d.max())
    assert max(deepest.values()) > LDS_MOST


def test_mirrored_rays_and_occlusion_probes_leave_the_lds_part(pkg, oracle, refs, mirror_refs):
    """What the phase machines of modes 150 and 120 send after their camera rays.  Mode 150 over the mirror, chain B and the
    backdrop (deep_stack_scenes.mirror_and_chain_b): the rays mirrored off the front square (closest hit, nearest child first),
    the shadow rays to the apex light from where they end on the backdrop (any hit, slot order, through the whole chain), and
    both as the oracle's mode-200 frame at one bounce sends them: a deep closest hit, then a deep any-hit walk behind one turn.
    Mode 120 over the plate and chain B: the K = 5 probes of the composed reference (tests/ambient_checks.py) of every pixel
    that sees the plate.  On every builder's tree some ray of each walk holds more than 16 entries, over the LBVH tree more
    than 32.

    Measured (depth4 of the mirror scene: deepest mirrored record / deepest shadow ray behind a turn / deepest bounce or shadow
    ray of the frame; depth4 of the plate scene: deepest probe): SAH 10: 27 / 27 / 27; 9: 26, LBVH 12: 35 / 35 / 35; 19: 57,
    PLOC 11: 30 / 30 / 30; 10: 29.  All 865 mirrored records, all 215 shadow rays from the backdrop (61 % of them lit) and 1734 of
    the 3370 probes hold more than 16 entries; 43 % of the probes are occluded."""
    w, h = SIZES["shadow"]
    seed = PATH[2]
    L = A.reference()
    msc = mirror_refs["scene"]
    recs = PH.frame_records(PR, msc["camera"], w, h, 0, seed)  # the jittered records of sample 0
    centre = camera_records(pkg, oracle, refs["shadow"]["scene"], w, h)
    deepest = {}
    for b in BUILDERS:
        # mode 150
        O = mirror_refs["trees"][b]
        first = oracle.trace_rays(O, recs)
        on = np.flatnonzero(first["inst"] == 0)
        assert len(on) > 100, "the camera sees the mirror"
        P = recs[on, 0:3] + recs[on, 4:7] * first["t"][on, None]
        mirrored = pkg.make_rays(np.float32(P + np.float32([0, 0, 1e-3])), np.float32(recs[on, 4:7] * np.float32([1, 1, -1])), tmin=0.0, tmax=D.TMAX)
        d_mirror = query_depths(oracle, O, mirrored, any_hit=False)
        second = oracle.trace_rays(O, mirrored)
        lit = np.flatnonzero(second["inst"] == 2)
        assert (second["inst"] == 1).sum() > 100 and len(lit) > 100, "mirrored rays end on chain B, and behind it on the backdrop"
        assert int(d_mirror[lit].max()) > LDS_DEFAULT, "the rays that reach the backdrop crossed the chain deep"
        P2 = mirrored[lit, 0:3] + mirrored[lit, 4:7] * second["t"][lit, None] - np.float32([0, 0, 1e-3])
        shadow = pkg.make_rays(np.float32(P2), np.float32(np.float64(D.APEX_LIGHT[0]) - P2), tmin=0.0, tmax=1.0)
        d_shadow = query_depths(oracle, O, shadow, any_hit=True)
        lit_share = 1.0 - float(oracle.occluded_rays(O, shadow)["occluded"].mean())
        assert 0.2 < lit_share < 0.8, "lit and shadowed points behind a turn"
        f, d_cam = _frame(oracle, O, msc["camera"], 200, w, h, depth=True, path=(1, 1, seed))
        _walk_equals_brute_force(f, _frame(oracle, O, msc["camera"], 200, w, h, brute_force=True, path=(1, 1, seed)), "the mirror and chain B, " + b)
        assert f["stats"]["rays_primary"] == w * h + len(on) and 100 < f["stats"]["rays_shadow"] <= len(on), "a mirrored ray per pixel on the mirror, a shadow ray behind it"
        lit_rgb = f["rgb"].reshape(-1, 3)[first["inst"] == 0]
        assert len(np.unique(lit_rgb, axis=0)) > len(on) // 4, "the light of a mirrored pixel depends on where its ray arrived"
        d_frame = int(f["secondary_depth"].max())
        # mode 120
        t = refs["shadow"]["trees"][b]
        f3 = {k: t["frames"][3][k].reshape(-1) for k in ("hit_inst", "hit_prim", "hit_t")}
        hit = np.flatnonzero(f3["hit_inst"] != MISS)
        N = sq.geometric_normals(refs["shadow"]["scene"]["meshes"], f3["hit_inst"][hit], f3["hit_prim"][hit], centre[hit, 4:7])[0].astype(np.float32)
        probes = A.probe_records(L, centre[hit], f3["hit_t"][hit], N, hit, 5, seed, A.UNBOUNDED)
        d_probe = query_depths(oracle, t["oracle"], probes, any_hit=True)
        occ = oracle.occluded_rays(t["oracle"], probes)["occluded"]
        np.testing.assert_array_equal(occ, oracle.occluded_rays(t["oracle"], probes, brute_force=True)["occluded"])
        print("%s: depth4 %d; mode 150: deepest mirrored record %d (deeper than 16: %d of %d), deepest shadow ray behind a turn %d (deeper than 16: %d of "
              "%d, lit %.0f %%), deepest bounce or shadow ray of the mode-200 frame at one bounce %d (of all its rays %d); depth4 %d; mode 120: deepest probe %d (deeper than 16: %d of %d, occluded %.0f %%)" % (
                  b, O.depth4, int(d_mirror.max()), int((d_mirror > LDS_DEFAULT).sum()), len(d_mirror), int(d_shadow.max()), int((d_shadow > LDS_DEFAULT).sum()),
                  len(d_shadow), 100.0 * lit_share, d_frame, int(d_cam.max()), t["depth4"],
                  int(d_probe.max()), int((d_probe > LDS_DEFAULT).sum()), len(d_probe), 100.0 * occ.mean()))
        assert int(d_cam.max()) == d_frame
        walks = (int(d_mirror.max()), int(d_shadow.max()), d_frame, int(d_probe.max()))
        assert min(walks) > LDS_DEFAULT and max(walks[:3]) <= 3 * O.depth4 + 1 and walks[3] <= 3 * t["depth4"] + 1, (b, walks)
        assert 0.2 < occ.mean() < 0.8, "occluded and escaping probes"
        deepest[b] = min(walks)
    assert deepest["lbvh"] > LDS_MOST


# ---- a depth4 that moves under a live context: the states the GPU test walks through, predicted on the CPU

def refitted_tree(oracle, topology, sc):
    """the oracle over what a refit leaves: the binary tree of the oracle scene `topology` (same triangle counts) with the boxes
    of sc's vertices -- leaves folded from their triangles, inner boxes the unions of their children's (tests/test_rebuild.py
    holds the refit to exactly that) -- and sc's records in the topology's leaf order"""
    nodes, leaf = topology.nodes().copy(), topology.tris()
    gids = leaf["gid"].astype(np.int64)
    S = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    by_gid = np.argsort(S.tris()["gid"], kind="stable")
    boxes = spec.tri_boxes(sc["meshes"])
    order, todo = [], [0]  # parents before their children, whatever the builder's numbering (the LBVH's is not pre-order)
    while todo:
        b = todo.pop()
        order.append(b)
        todo.extend(int(nodes[b][key]) for key in ("left", "right") if int(nodes[b][key]) >= 0)
    for b in reversed(order):  # children first
        for side, key in (("l", "left"), ("r", "right")):
            ref = int(nodes[b][key])
            if ref >= 0:
                cb = spec.child_boxes(nodes[ref:ref + 1])[0]
                box = spec.union(cb[0], cb[1])
            else:
                first, cnt = (~ref) >> 3, (~ref) & 7
                box = spec._fold(boxes[gids[first:first + cnt]])
            for a, ax in enumerate("xyz"):
                nodes[b][side + ax + "0"], nodes[b][side + ax + "1"] = box[a], box[3 + a]
    S.set_bvh(nodes, S.tris()[by_gid][gids], S.shade()[by_gid][gids])
    return S


ROUTE_SIZE = (16, 16)


def route_states(pkg, oracle):
    """[(name, scene, oracle over the tree the route leaves, route)] in the order the GPU test takes them; route: "upload",
    "refit" (a vertex update, then a refit), "lbvh" or "ploc" (a rebuild with that builder)"""
    deep = D.chain_a()
    shallow = D.shallow_like(deep)
    sah_shallow = oracle_tree(pkg, oracle, shallow, "sah")
    lbvh_deep = oracle_tree(pkg, oracle, deep, "lbvh")
    return [("shallow upload", shallow, sah_shallow, "upload"),
            ("deep re-upload", deep, oracle_tree(pkg, oracle, deep, "sah"), "upload"),
            ("shallow upload again", shallow, sah_shallow, "upload"),
            ("vertex update and refit to deep", deep, refitted_tree(oracle, sah_shallow, deep), "refit"),
            ("LBVH rebuild", deep, lbvh_deep, "lbvh"),
            ("refit to shallow", shallow, refitted_tree(oracle, lbvh_deep, shallow), "refit"),
            ("refit to deep", deep, refitted_tree(oracle, lbvh_deep, deep), "refit"),
            ("PLOC rebuild", deep, oracle_tree(pkg, oracle, deep, "ploc"), "ploc")]


def test_depth4_moves_on_every_route(pkg, oracle):
    """What the slices of a context have to follow: depth4 of every state, and the deepest lane of its mode-3 frame."""
    states = route_states(pkg, oracle)
    w, h = ROUTE_SIZE
    seen = []
    for name, sc, O, _ in states:
        f, d = _frame(oracle, O, sc["camera"], 3, w, h, depth=True)
        _walk_equals_brute_force(f, _frame(oracle, O, sc["camera"], 3, w, h, brute_force=True), name)
        rays = query_rays(pkg, oracle, sc, w, h)
        _walk_equals_brute_force(oracle.trace_rays(O, rays), oracle.trace_rays(O, rays, brute_force=True), name + ", records")
        seen.append((name, O.depth4, int(d.max())))
        print("%s: depth4 %d, bound %d, deepest lane %d" % (name, O.depth4, 3 * O.depth4 + 1, int(d.max())))
        assert int(d.max()) <= 3 * O.depth4 + 1
    by = {n: (d4, deepest) for n, d4, deepest in seen}
    for a, b in zip(seen, seen[1:]):
        assert a[1] != b[1], "%s -> %s: depth4 stays %d" % (a[0], b[0], a[1])
    # slices sized for the state before would be too short for a lane of the state after: a stale depth4 shows in the results
    for before, after in (("shallow upload", "deep re-upload"), ("vertex update and refit to deep", "LBVH rebuild"), ("refit to shallow", "refit to deep")):
        assert by[after][1] > max(LDS_MOST, 3 * by[before][0] + 1), (before, after, by[before], by[after])
    # (the refit of the shallow upload's balanced tree stays within 16 entries: there a stale depth4 shows at LDS parts of 1 and 5
    #  entries, and in what crt_bvh_info4 reports)
    before, after = by["shallow upload again"], by["vertex update and refit to deep"]
    assert after[1] > max(5, 3 * before[0] + 1), (before, after)
    assert by["refit to deep"] == by["LBVH rebuild"]


# ---- GPU

RING = 4  # frames a context keeps in flight (crt_ctx.h kRing): one spill arena each
DEFAULTS = (("gpu_build", 0), ("gpu_builder", 0), ("stack_entries", 0), ("path_pipeline", 0), ("path_tile", 0), ("split_units", -1),
            ("split_rays", 4), ("split_segments", 16), ("list_short_max", 24), ("path_pass_paths", 1 << 24), ("ao_samples", 16), ("ao_radius", 0),
            ("ao_sky", 0))
PATH_FORMS = ((0, 0), (1, 0), (0, 16))  # (path_pipeline, path_tile): path_tile = 16 runs with path_pipeline = 0


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _restore(renderer):
    for k, v in DEFAULTS:
        renderer.set_option(k, v)
    renderer.set_counting(False)
    renderer.set_path_params(4, 3, 1234)
    renderer.change_shading_mode(0)


def _upload(renderer, sc, builder, dynamic=False):
    for k, v in TREES[builder].items():
        renderer.set_option(k, v)
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=dynamic)
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])


def _same_tree(renderer, O, what):
    """the context walks the tree the CPU tests measured, and sizes its slices by that tree's depth4 (crt_bvh_info4)"""
    assert renderer.bvh_export4q().tobytes() == O.nodes4q().tobytes(), what + ": the wide tree is not the oracle's"
    assert renderer.bvh_export()[1].tobytes() == O.tris().tobytes(), what + ": the leaf order is not the oracle's"
    assert renderer.bvh_export4()[1] == O.depth4, what + ": depth4"


def _check_frame(renderer, w, h, ref, brute, what):
    """the plain and the counting kernel's frame against the oracle's over the same tree, bit for bit and counter for counter; hit
    ids and t against brute force"""
    for counting in (False, True):
        renderer.set_counting(counting)
        try:
            got = renderer.render_frame(w, h)
        finally:
            renderer.set_counting(False)
        tag = "%s counting=%d" % (what, counting)
        for k in ("hit_inst", "hit_prim", "rgba8"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (tag, k))
        np.testing.assert_array_equal(_bits(got["hit_t"]), _bits(ref["hit_t"]), err_msg=tag + " hit_t")
        np.testing.assert_array_equal(_bits(got["rgb"]), _bits(ref["rgb"]), err_msg=tag + " rgb")
        _walk_equals_brute_force(got, brute, tag)
        if counting:
            for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested"):
                assert got["stats"][k] == ref["stats"][k], "%s %s" % (tag, k)
    return got


def _check_modes(renderer, w, h, t, modes, what):
    for mode in modes:
        renderer.change_shading_mode(mode)
        if mode != 200:
            _check_frame(renderer, w, h, t["frames"][mode], t["brute"][mode], "%s mode %d" % (what, mode))
            continue
        renderer.set_path_params(*PATH)
        for pipeline, tile in PATH_FORMS:
            renderer.set_option("path_pipeline", pipeline)
            renderer.set_option("path_tile", tile)
            _check_frame(renderer, w, h, t["frames"][200], t["brute"][200], "%s mode 200 pipeline %d tile %d" % (what, pipeline, tile))
        renderer.set_option("path_pipeline", 0)
        renderer.set_option("path_tile", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("entries", STACK_ENTRIES)
@pytest.mark.parametrize("builder", BUILDERS)
def test_frames_match_the_oracle(refs, renderer, builder, entries):
    """modes 3, 100 and 200 (1 persistent kernel, stage launches, 16 x 16 tiles) of the three scenes over one builder's tree"""
    try:
        renderer.set_option("stack_entries", entries)
        for name, e in refs.items():
            t = e["trees"][builder]
            _upload(renderer, e["scene"], builder)
            what = "%s, %s, stack_entries=%d" % (name, builder, entries)
            _same_tree(renderer, t["oracle"], what)
            _check_modes(renderer, *SIZES[name], t, MODES[name], what)
    finally:
        _restore(renderer)


def _counting_forms(renderer, call):
    """call() with counting off, then on"""
    out = []
    for counting in (False, True):
        renderer.set_counting(counting)
        try:
            out.append(call())
        finally:
            renderer.set_counting(False)
    return out


def _check_ray_queries(oracle, renderer, O, rays, what, frame=None):
    """trace_rays and occluded against the oracle's walk of the same tree (results and fetch counters) and against brute force;
    returns what trace_rays gave"""
    walk, brute = oracle.trace_rays(O, rays), oracle.trace_rays(O, rays, brute_force=True)
    wocc, bocc = oracle.occluded_rays(O, rays), oracle.occluded_rays(O, rays, brute_force=True)
    for counting, got in enumerate(_counting_forms(renderer, lambda: renderer.trace_rays(rays))):
        tag = "%s: trace_rays counting=%d" % (what, counting)
        sq._same_hits(got, walk, tag + " against the oracle's walk", keys=sq.HIT_OUTPUTS)
        sq._same_hits(got, brute, tag + " against brute force")
        if counting:
            assert (got["stats"]["nodes_visited"], got["stats"]["tris_tested"]) == (int(walk["nodes"].sum()), int(walk["tris"].sum())), tag
        if frame is not None:  # the camera rays come first: a record is the frame's ray
            n = frame["hit_t"].size
            sq._same_hits({k: got[k][:n] for k in ("t", "inst", "prim")}, frame, tag + " against the frame",
                          names={"t": "hit_t", "inst": "hit_inst", "prim": "hit_prim"})
    for counting, occ in enumerate(_counting_forms(renderer, lambda: renderer.occluded(rays))):
        tag = "%s: occluded counting=%d" % (what, counting)
        np.testing.assert_array_equal(np.asarray(occ, bool), wocc["occluded"] == 1, err_msg=tag + " against the oracle's walk")
        np.testing.assert_array_equal(np.asarray(occ, bool), bocc["occluded"] == 1, err_msg=tag + " against brute force")
    return got


def _check_closest_points(pkg, point_ref, renderer, sc, pts, what):
    want = tp.ref_closest(point_ref, tp._tri_records(pkg, sc["meshes"]), pts)
    for counting, got in enumerate(_counting_forms(renderer, lambda: renderer.closest_points(pts))):
        tp._assert_closest_equal(got, want, "%s: closest_points counting=%d" % (what, counting))
    assert (want["inst"] != MISS).sum() > len(pts) // 2


def _some_points(pkg, sc, n, seed):
    """apex points (deep descents), then points in and around the scene's box with rmax = inf and a finite rmax"""
    rng = np.random.default_rng(seed)
    lo, hi = sq.bounds(sc)
    xyz = (lo - 0.1 * (hi - lo) + rng.random((n, 3)) * 1.2 * (hi - lo)).astype(np.float32)
    near = rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([apex_points(pkg, n, seed), pkg.make_points(near, rmax=np.inf),
                                                pkg.make_points(xyz, rmax=rng.choice([np.inf, 50.0], size=n))]))


def winding_points(pkg, sc, seed):
    """192 points: 64 at chain A's apex, 120 of _some_points, 8 a hundred sizes away, the last of them with a NaN"""
    lo, hi = sq.bounds(sc)
    far = np.random.default_rng(seed).normal(size=(8, 3))
    far = pkg.make_points(np.float32(0.5 * (lo + hi) + far / np.linalg.norm(far, axis=1, keepdims=True) * 100.0 * np.linalg.norm(hi - lo)))
    far[-1, 2] = np.nan
    pts = np.ascontiguousarray(np.concatenate([apex_points(pkg, 64, seed), _some_points(pkg, sc, 40, seed + 1), far]))
    assert len(pts) == 192
    return pts


_winding_seen = {}  # (scene, builder) -> what assert_winding returned at the first LDS part that ran


def _check_winding(pkg, wref, renderer, name, sc, builder, tag):
    """winding numbers over the deep tree: every check of winding_checks.assert_winding; the bits and the fetch counters are the
    same at every LDS part"""
    out = wc.assert_winding(pkg, wref, renderer, sc, tp._tri_records(pkg, sc["meshes"]), winding_points(pkg, sc, seed=9), "%s, %s" % (name, tag))
    first = _winding_seen.setdefault((name, builder), out)
    for beta, bits in out["w"].items():
        np.testing.assert_array_equal(bits, first["w"][beta], err_msg="%s, %s: beta %r depends on stack_entries" % (name, tag, beta))
    assert out["counters"] == first["counters"], "%s, %s: the fetch counters depend on stack_entries" % (name, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("entries", STACK_ENTRIES)
@pytest.mark.parametrize("builder", BUILDERS)
def test_queries_match_their_references(pkg, oracle, refs, list_ref, point_ref, wref, renderer, builder, entries):
    """every query kernel on the camera rays and the apex rays: chain A for the closest-hit and closest-point walks, the plate
    and chain B for the any-hit and no-cull walks and, its shadow and bounce rays being deep, for the shaded (modes 3, 100,
    120 and 150), path-traced and guide queries; test_whitted_and_ambient_queries_match_the_oracle adds the mirror for mode 150
    and K = 64 for mode 120"""
    try:
        renderer.set_option("stack_entries", entries)
        tag = "%s, stack_entries=%d" % (builder, entries)
        # chain A
        e = refs["chain"]
        t, sc, (w, h) = e["trees"][builder], e["scene"], SIZES["chain"]
        _upload(renderer, sc, builder)
        renderer.change_shading_mode(3)
        got = _check_ray_queries(oracle, renderer, t["oracle"], e["rays"], "chain A, " + tag, frame=t["frames"][3])
        pick = np.arange(0, len(e["rays"]), 16)  # the plain-Python brute force of tests/test_ray_queries.py on every 16th ray
        tr._check_brute(oracle, tr._scene_triangles(sc), e["rays"][pick], {k: got[k][pick] for k in sq.HIT_OUTPUTS})
        _check_closest_points(pkg, point_ref, renderer, sc, _some_points(pkg, sc, 192, seed=5), "chain A, " + tag)
        _check_winding(pkg, wref, renderer, "chain A", sc, builder, tag)
        # the plate and chain B
        e = refs["shadow"]
        t, sc = e["trees"][builder], e["scene"]
        _upload(renderer, sc, builder)
        _check_ray_queries(oracle, renderer, t["oracle"], e["rays"], "plate and chain B, " + tag)
        records = tp._tri_records(pkg, sc["meshes"])
        want = tp.ref_count(point_ref, records, e["rays"])
        assert want[-N_APEX:].min() == len(sc["meshes"][1]["triangles"]), "an apex ray crosses every plate of chain B"
        for counting, cnt in enumerate(_counting_forms(renderer, lambda: renderer.count_hits(e["rays"]))):
            np.testing.assert_array_equal(cnt, want, err_msg="%s: count_hits counting=%d" % (tag, counting))
        for short_max in (24, 1024):  # an apex ray's 120 records: sorted by a wavefront, then by one lane
            renderer.set_option("list_short_max", short_max)
            for counting in (False, True):
                renderer.set_counting(counting)
                tl._check_against_everything(pkg, list_ref, renderer, e["rays"], "%s list_short_max=%d counting=%d" % (tag, short_max, counting))
            renderer.set_counting(False)
        renderer.set_option("list_short_max", 24)
        pts = np.ascontiguousarray(np.concatenate([occupancy_points(pkg, 192, seed=8), _some_points(pkg, sc, 192, seed=6)]))
        inside = tp.ref_occupancy(point_ref, records, pts)
        for counting, occ in enumerate(_counting_forms(renderer, lambda: renderer.occupancy(pts))):
            np.testing.assert_array_equal(occ, inside, err_msg="%s: occupancy counting=%d" % (tag, counting))
        _check_closest_points(pkg, point_ref, renderer, sc, pts, "plate and chain B, " + tag)
        _check_winding(pkg, wref, renderer, "plate and chain B", sc, builder, tag)
        # shade_rays (modes 3 and 100; host, counting and device forms), path_rays and frame_guides against the frames
        w, h = SIZES["shadow"]
        sq.frame_records_equal_frames(renderer, t["frames"], w, h, PATH, "plate and chain B, " + tag, scene=sc, cache=e["cache"],
                                      world=_world(oracle, sc, t["oracle"]))
        apex = e["rays"][w * h:]
        sq.arbitrary_records_equal_trace(renderer, apex, oracle.trace_rays(t["oracle"], apex, brute_force=True), "apex rays, " + tag)
    finally:
        _restore(renderer)


@pytest.mark.gpu
@pytest.mark.parametrize("entries", STACK_ENTRIES)
@pytest.mark.parametrize("builder", BUILDERS)
def test_whitted_and_ambient_queries_match_the_oracle(pkg, oracle, refs, mirror_refs, renderer, builder, entries):
    """Mode 150 over the mirror and chain B: the three forms and the frame against the oracle's mode-200 frames along the
    specular chain (shaded_query_checks.whitted_reference), and 129 copies of the frame's records in four launches
    ("path_pass_paths" = 65536) against one launch, every output bit for bit.  Mode 120 over the plate and chain B at K = 5
    and K = 64 against the contract composed on the CPU (shaded_query_checks.ambient_reference).
    test_mirrored_rays_and_occlusion_probes_leave_the_lds_part measures how deep these rays go."""
    try:
        renderer.set_option("stack_entries", entries)
        tag = "%s, stack_entries=%d" % (builder, entries)
        w, h = SIZES["shadow"]
        _, bounces, seed = PATH
        sc, O = mirror_refs["scene"], mirror_refs["trees"][builder]
        _upload(renderer, sc, builder)
        _same_tree(renderer, O, "the mirror and chain B, " + tag)
        renderer.set_path_params(1, bounces, seed)
        centre, recs = renderer.camera_rays(w, h), renderer.camera_rays(w, h, sample=0)
        got = sq.collect_whitted_records(renderer, recs, bounces, True, frame=(w, h, centre))
        ref = sq.whitted_reference(_world(oracle, sc, O), sc, w, h, bounces, seed, tag, mirror_refs["cache"].setdefault(builder, {}))
        assert (ref["turns"] == 1).sum() > 500 and (ref["turns"] == 0).sum() > 500, "pixels on the mirror, and beside it"
        sq.assert_whitted_records(got, ref, "the mirror and chain B, " + tag, sc["meshes"])
        many = np.ascontiguousarray(np.tile(recs, (LAUNCH_COPIES, 1)))
        assert len(many) > 3 * (1 << 16)
        renderer.change_shading_mode(150)
        one = renderer.shade_rays(many)
        sq._same_bits(one["rgb"].reshape(LAUNCH_COPIES, -1), np.tile(ref["rgb"][bounces].reshape(1, -1), (LAUNCH_COPIES, 1)), tag + ": every copy of the records, rgb")
        renderer.set_option("path_pass_paths", 1 << 16)
        for counting, several in enumerate(_counting_forms(renderer, lambda: renderer.shade_rays(many))):
            for k in sq.SHADE_OUTPUTS:
                (sq._same_ids if k in ("inst", "prim") else sq._same_bits)(several[k], one[k], "%s: four launches against one, counting=%d, %s" % (tag, counting, k))
        assert several["stats"]["rays_primary"] == len(many) + LAUNCH_COPIES * int((ref["turns"] >= 1).sum()), tag + ": the counters go on over the launches"
        renderer.set_option("path_pass_paths", 1 << 24)

        e = refs["shadow"]
        t, sc = e["trees"][builder], e["scene"]
        _upload(renderer, sc, builder)
        centre = renderer.camera_rays(w, h)
        got = sq.collect_ambient_records(renderer, centre, seed, DEEP_AO, frame=(w, h, centre))
        ref = sq.ambient_reference(got, sq.frame_hits(t["frames"]), _world(oracle, sc, t["oracle"]), sc, e["cache"])
        sq.assert_surface(got["surface"], centre, sc, "plate and chain B, " + tag)
        sq.assert_ambient_records(got, ref, "plate and chain B, " + tag, sc["meshes"])
        occ = ref["occluded"][0]
        assert len(ref["hit"]) > 500 and 0.2 < occ.mean() < 0.8 and (occ.sum(axis=1) % 64 != 0).any(), "occluded and escaping probes within one record"
    finally:
        _restore(renderer)


def _tile_shares(pkg, renderer, w, h, n):
    import torch
    slots = pkg.tile_slots(w, h, n)
    gathered = torch.zeros(n * slots * 256, dtype=torch.int32, device="cuda")
    frame = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for rank in range(n):
        renderer.render_tiles_device(w, h, rank, n, gathered.data_ptr() + rank * slots * 1024)
    renderer.untile_device(w, h, n, gathered.data_ptr(), frame.data_ptr())
    renderer.synchronize()
    return frame.cpu().numpy().view(np.uint32).reshape(h, w)


def _split_batch_tiles(pkg, oracle, scenes, renderer, name, e, entries, counting):
    import torch
    t, sc, (w, h) = e["trees"]["lbvh"], e["scene"], SIZES[name]
    cam = sc["camera"]
    plain = {mode: t["frames"][mode]["rgba8"].view(np.uint32).reshape(h, w) for mode in MODES[name]}
    _upload(renderer, sc, "lbvh")
    _same_tree(renderer, t["oracle"], name)
    renderer.set_path_params(*PATH)
    renderer.set_counting(counting)
    for mode in [m for m in MODES[name] if m != 200]:
        renderer.change_shading_mode(mode)
        for rays, segs in ((4, 16), (16, 4), (8, 8)):
            renderer.set_option("split_units", 6)
            renderer.set_option("split_rays", rays)
            renderer.set_option("split_segments", segs)
            for frame in range(2 * RING + 2):  # the launch order (and with it the split) comes from an earlier frame's costs
                got = renderer.render_frame(w, h)
            what = "%s stack_entries=%d counting=%d mode %d split %d x %d" % (name, entries, counting, mode, rays, segs)
            ref = t["frames"][mode]
            for k in ("hit_inst", "hit_prim", "rgba8"):
                np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (what, k))
            np.testing.assert_array_equal(_bits(got["hit_t"]), _bits(ref["hit_t"]), err_msg=what)
            np.testing.assert_array_equal(_bits(got["rgb"]), _bits(ref["rgb"]), err_msg=what)
            if counting:  # every wavefront of a split packet walks from the root: the fetch counters grow where packets were split
                assert got["stats"]["nodes_visited"] > ref["stats"]["nodes_visited"], what + ": no packet was split"
            for rep in range(RING + 1):  # the shares of three ranks, split as well
                shares = _tile_shares(pkg, renderer, w, h, 3)
            np.testing.assert_array_equal(shares, plain[mode], err_msg=what + " three tile shares")
        renderer.set_option("split_units", -1)
        renderer.set_option("split_rays", 4)
        renderer.set_option("split_segments", 16)
    # four frames in one launch: the plain frame, and three cameras turned a little at the apex
    cams = [(np.float32(cam["position"]), np.float32(cam["matrix"]).reshape(9))] + [
        (np.float32(cam["position"]), scenes.camera_matrix(yaw_deg=y, pitch_deg=p)) for y, p in ((2.0, 0.0), (0.0, -3.0), (-4.0, 1.0))]
    for mode, pipeline in [(m, 0) for m in MODES[name]] + ([(200, 1)] if 200 in MODES[name] else []):
        renderer.change_shading_mode(mode)
        renderer.set_option("path_pipeline", pipeline)
        oracle.set_path_params(*PATH)
        try:
            want = [t["oracle"].render(p, r, mode, w, h)["rgba8"].view(np.uint32).reshape(-1) for p, r in cams]
        finally:
            oracle.set_path_params(4, 3, 1234)
        np.testing.assert_array_equal(want[0], plain[mode].reshape(-1))
        bufs = [torch.full((w * h,), 0x7E57AB1E, dtype=torch.int32, device="cuda") for _ in cams]
        torch.cuda.synchronize()
        renderer.render_frames_batch_device(w, h, [b.data_ptr() for b in bufs], cams, stats=True)
        what = "%s stack_entries=%d counting=%d mode %d pipeline %d" % (name, entries, counting, mode, pipeline)
        for k, b in enumerate(bufs):
            np.testing.assert_array_equal(b.cpu().numpy().view(np.uint32), want[k], err_msg="%s batch frame %d" % (what, k))
        renderer.set_camera(*cams[0])
        np.testing.assert_array_equal(_tile_shares(pkg, renderer, w, h, 3), plain[mode], err_msg=what + " three tile shares")
    renderer.set_option("path_pipeline", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("entries", STACK_ENTRIES)
def test_split_packets_batches_and_tile_shares_render_the_same_frame(pkg, oracle, scenes, refs, renderer, entries):
    """chain A (deep camera rays) and the plate with chain B (deep shadow and bounce rays) over the LBVH tree, plain and counting
    kernels: the six most expensive packets split over 4 / 8 / 16 wavefronts (slices behind the frame's own, 16 groups per split
    packet), four frames in one launch, and the tile shares of three ranks reassembled"""
    try:
        renderer.set_option("stack_entries", entries)
        for name, e in refs.items():
            for counting in (False, True):
                _split_batch_tiles(pkg, oracle, scenes, renderer, name, e, entries, counting)
    finally:
        _restore(renderer)


@pytest.mark.gpu
@pytest.mark.parametrize("entries", STACK_ENTRIES)
def test_slices_follow_a_depth4_that_moves(pkg, oracle, point_ref, wref, renderer, entries):
    """One context through the states of test_depth4_moves_on_every_route: uploads, a vertex update with a refit, rebuilds with
    both builders, refits back and forth.  After every step crt_bvh_info4 reports the predicted tree's depth4, and more frames than
    the context has ring slots, the ray queries and the closest-point query (arenas of their own) equal the oracle over the
    exported tree.  So do the winding numbers and their moment table (winding_checks.assert_winding): the table a winding query
    built just before the move is stale after it, and is built again with the new tree's level count and node count."""
    w, h = ROUTE_SIZE
    states = route_states(pkg, oracle)
    r = renderer

    def move(route, sc):
        if route == "upload":
            _upload(r, sc, "sah", dynamic=True)
        elif route == "refit":
            r.update_vertices(0, sc["meshes"][0]["vertices"])
            r.refit()
        else:
            r.set_option("gpu_builder", {"lbvh": 0, "ploc": 1}[route])
            r.rebuild()
    try:
        r.set_option("stack_entries", entries)
        held = None  # the points and the beta = 2 bits of the state the context holds
        for name, sc, O, route in states:
            what = "%s, stack_entries=%d" % (name, entries)
            if held is not None:  # the moment table is this state's when the move comes
                np.testing.assert_array_equal(_bits(r.winding_numbers(held[0], 2.0)), held[1], err_msg=what + ": before the move")
            move(route, sc)
            # the oracle over the tree the context now holds; it has the predicted state's depth4 and deepest lane
            nodes, tris, shade = r.bvh_export()
            S = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
            try:
                S.set_bvh(nodes, tris, shade)
                _same_tree(r, S, what)
                assert r.bvh_export4()[1] == O.depth4, what + ": depth4 is not the predicted tree's"
                ref, depth = _frame(oracle, S, sc["camera"], 3, w, h, depth=True)
                assert int(depth.max()) == int(_frame(oracle, O, sc["camera"], 3, w, h, depth=True)[1].max()), what + ": deepest lane"
                brute = _frame(oracle, S, sc["camera"], 3, w, h, brute_force=True)
                r.change_shading_mode(3)
                for k in range(RING + 2):  # every ring slot's arena has to follow
                    if k in (0, RING + 1):
                        _check_frame(r, w, h, ref, brute, "%s frame %d" % (what, k))
                    else:
                        r.render_frame(w, h, want=("rgba8",))
                _check_ray_queries(oracle, r, S, query_rays(pkg, oracle, sc, w, h), what, frame=ref)
                # a query and a frame of modes 120 and 150: arenas of beginQuery with phase machines of their own over them
                sq.new_modes_equal_references(r, {3: ref, 100: _frame(oracle, S, sc["camera"], 100, w, h)}, w, h, PATH[1], PATH[2], what, sc,
                                              _world(oracle, sc, S), settings=ROUTE_AO)
                _check_closest_points(pkg, point_ref, r, sc, apex_points(pkg, 128, seed=7), what)
                wpts = winding_points(pkg, sc, seed=11)
                held = (wpts, wc.assert_winding(pkg, wref, r, sc, tp._tri_records(pkg, sc["meshes"]), wpts, what)["w"][2.0])
            finally:
                S.close()
    finally:
        for state in states:
            state[2].close()
        _restore(r)
