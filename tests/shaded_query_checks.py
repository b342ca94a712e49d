"""Shared checks for the shaded, path-traced, camera-ray and guide queries (crt_shade_rays*, crt_path_rays*, crt_camera_rays*,
crt_frame_guides*, include/crt_hip.h) on scenes other test files build: poisoned, rebuilt, refitted, textured or far from the origin.

A camera-ray record is the frame's ray bit for bit, so a reference frame (an oracle frame, brute force where the caller has one) is
the reference of w * h records; a 1 x 1 oracle frame is the reference of one arbitrary pose.  Every comparison here is exact (float
bits as uint32, ids by value) except the float64 geometric normal, which keeps test_shade_rays.test_attributes' bound of 1e-5.

Each check is split in two: collect_* runs the queries on a renderer, assert_* compares what was collected with the reference and
touches no GPU, so tests/test_shaded_query_checks.py can feed the assertions their own reference and one-value corruptions of it."""
import numpy as np

import path_rays_helpers as H
import path_reference as R

MISS = 0xFFFFFFFF
TMIN, TMAX = 0.001, 10000.0
N_POSES, POSE_SEED = 256, 20
NORMAL_TOL = 1e-5  # per component, against the float64 unit normal: test_shade_rays.test_attributes' bound and reasoning
SHADE_OUTPUTS = ("rgb", "normal", "albedo", "t", "uv", "inst", "prim")
HIT_OUTPUTS = ("t", "uv", "inst", "prim")
FORMS = ("host", "counting", "device")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, ref, what):
    g, r = _bits(got).reshape(-1), _bits(ref).reshape(-1)
    assert g.shape == r.shape, "%s: %d values, the reference has %d" % (what, g.size, r.size)
    bad = np.flatnonzero(g != r)
    assert len(bad) == 0, "%s: %d of %d floats differ in their bits, first at %d: 0x%08x, reference 0x%08x" % (
        what, len(bad), g.size, bad[0], g[bad[0]], r[bad[0]])


def _same_ids(got, ref, what):
    g, r = np.asarray(got).reshape(-1).astype(np.uint32), np.asarray(ref).reshape(-1).astype(np.uint32)
    assert g.shape == r.shape, "%s: %d values, the reference has %d" % (what, g.size, r.size)
    bad = np.flatnonzero(g != r)
    assert len(bad) == 0, "%s: %d of %d ids differ, first at %d: %d, reference %d" % (what, len(bad), g.size, bad[0], g[bad[0]], r[bad[0]])


def _same_hits(got, ref, what, keys=("t", "inst", "prim"), names=None):
    names = names or {k: k for k in keys}
    for k in keys:
        (_same_ids if k in ("inst", "prim") else _same_bits)(got[k], ref[names[k]], "%s %s" % (what, k))


# ---- the scene as the checks read it

def inert_mask(meshes):
    """per mesh, the triangles with a non-finite value among their nine coordinates (include/crt_hip.h, "inert triangles")"""
    out = []
    for m in meshes:
        v = np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3)
        t = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)
        out.append(~np.isfinite(v[t]).all(axis=(1, 2)) if len(t) else np.zeros(0, bool))
    return out


def assert_none_inert(meshes, inst, prim, what):
    """a reported hit on an inert triangle of `meshes` (the poisoned vertices) is a failure by itself"""
    inert = inert_mask(meshes)
    if not any(d.any() for d in inert):
        return
    ids = np.concatenate([(np.uint64(i) << np.uint64(32)) | np.flatnonzero(d).astype(np.uint64) for i, d in enumerate(inert)])
    inst, prim = np.asarray(inst).reshape(-1), np.asarray(prim).reshape(-1)
    hit = inst != MISS
    key = (inst[hit].astype(np.uint64) << np.uint64(32)) | prim[hit].astype(np.uint64)
    assert not np.isin(key, ids).any(), "%s: an inert triangle was reported" % what


def geometric_normals(meshes, inst, prim, dirs):
    """(float64 unit normal of triangle (inst, prim) flipped to face the ray, checked): the cross product of the edges of the
    float32 vertices; checked marks the hits on meshes without vertex normals, the only ones the value is stated for"""
    inst, prim = np.asarray(inst).reshape(-1), np.asarray(prim).reshape(-1)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    ref = np.zeros((len(inst), 3))
    checked = np.zeros(len(inst), bool)
    for i, m in enumerate(meshes):
        sel = inst == i
        if m.get("normals") is not None or not sel.any():
            continue
        v = np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3).astype(np.float64)
        t = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)[prim[sel]]
        n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
        ref[sel] = n / np.linalg.norm(n, axis=1, keepdims=True)
        checked |= sel
    ref[np.einsum("ij,ij->i", ref, d) > 0.0] *= -1.0
    return ref, checked


def _fma(a, b, c):
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return np.float32(np.float32(a * b) + c)  # (infinities and NaN come out the same with one rounding or two)
    return H.fmaf(a, b, c)


def expected_albedo(scene, inst, prim, uv, texture_color=None):
    """(albedo, checked) at hits (inst, prim) with barycentrics uv: the material's colour (white past the material table) for an
    untextured material; for a textured one, where texture_color (the oracle's) is given, the texture's colour at the hit's
    barycentrics (edges) or at uv0 * w + uv1 * u + uv2 * v formed in float32 in the documented order."""
    inst, prim = np.asarray(inst).reshape(-1), np.asarray(prim).reshape(-1)
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    mats, textures = list(scene.get("materials") or ()), list(scene.get("textures") or ())
    out = np.zeros((len(inst), 3), np.float32)
    checked = np.zeros(len(inst), bool)
    for i, m in enumerate(scene["meshes"]):
        sel = np.flatnonzero(inst == i)
        if not len(sel):
            continue
        mi = int(m.get("material_index", 0))
        mat = mats[mi] if 0 <= mi < len(mats) else {"albedo": (1.0, 1.0, 1.0)}
        ti = int(mat.get("texture", -1))
        if not 0 <= ti < len(textures):
            out[sel] = np.float32(mat.get("albedo", (1.0, 1.0, 1.0)))
            checked[sel] = True
            continue
        if texture_color is None:
            continue
        tex = textures[ti]
        muv = m.get("uvs")
        tri = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)
        for k in sel:
            u, v = uv[k]
            tu, tv = u, v
            if tex["type"] != "edges":
                tu = tv = np.float32(0.0)
                if muv is not None:
                    U = np.asarray(muv, dtype=np.float32).reshape(-1, 3)[tri[prim[k]]]
                    w = np.float32(np.float32(1.0) - u) - v
                    tu = _fma(U[2, 0], v, _fma(U[1, 0], u, U[0, 0] * w))
                    tv = _fma(U[2, 1], v, _fma(U[1, 1], u, U[0, 1] * w))
            out[k] = texture_color(tex, tu, tv)
            checked[k] = True
    return out, checked


# ---- frames: camera rays through the shaded and the path queries, and the guides

def _shade_device(renderer, rays):
    """crt_shade_rays_device on torch buffers, every output, read back as numpy arrays"""
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float32)).cuda()
    shapes = {"rgb": (n, 3), "normal": (n, 3), "albedo": (n, 3), "t": (n,), "uv": (n, 2), "inst": (n,), "prim": (n,)}
    out = {k: torch.zeros(shapes[k], dtype=torch.int32 if k in ("inst", "prim") else torch.float32, device="cuda") for k in SHADE_OUTPUTS}
    torch.cuda.synchronize()
    renderer.shade_rays_device(n, d_rays.data_ptr(), *[out[k].data_ptr() for k in SHADE_OUTPUTS])
    renderer.synchronize()
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().view(np.uint32) if k in ("inst", "prim") else v.cpu().numpy()) for k, v in out.items()}


def _shade_forms(renderer, rays):
    plain = renderer.shade_rays(rays)
    renderer.set_counting(True)
    try:
        counted = renderer.shade_rays(rays)
    finally:
        renderer.set_counting(False)
    return {"host": plain, "counting": counted, "device": _shade_device(renderer, rays)}


def _path_chain(renderer, records_of_sample, spp, ids=None):
    """samples 0 .. spp - 1, one call each with that sample's records, chained through one sums buffer: rgb of the last call
    (the mean over spp samples) and the hit outputs of the first"""
    sums = None
    for k in range(spp):
        recs = records_of_sample(k)
        if sums is None:
            sums = np.zeros((len(recs), 3), dtype=np.float64)
        got = renderer.path_rays(recs, ids=ids, first_sample=k, n_samples=1, sums=sums)
        if k == 0:
            first = got
    return {"rgb": got["rgb"], "t": first["t"], "uv": first["uv"], "inst": first["inst"], "prim": first["prim"]}


def collect_frame_records(renderer, w, h, path_params):
    spp, bounces, seed = path_params
    renderer.set_path_params(spp, bounces, seed)
    centre = renderer.camera_rays(w, h)
    got = {"centre": centre, "shade": {}}
    for mode in (3, 100):
        renderer.change_shading_mode(mode)
        got["shade"][mode] = _shade_forms(renderer, centre)
    got["path"] = _path_chain(renderer, lambda k: renderer.camera_rays(w, h, sample=k), spp)
    got["guides"] = renderer.frame_guides(w, h)
    got["guides_ref"] = renderer.shade_rays(centre, want=("normal", "albedo", "t"))
    return got


def assert_frame_records(got, frames, w, h, what, scene=None, texture_color=None, cache=None):
    """got: collect_frame_records' dict; frames: {3, 100, 200: a reference frame}; scene: {meshes (the vertices as uploaded,
    poisoned ones included), materials, textures} for the checks on normal, albedo and inert ids; cache: a dict the caller keeps
    with `frames`, where the expected albedo of these frames is computed once"""
    n = w * h
    meshes = scene["meshes"] if scene is not None else None
    host3 = got["shade"][3]["host"]
    for mode in (3, 100):
        ref = frames[mode]
        for form in FORMS:
            g, tag = got["shade"][mode][form], "%s: shade_rays mode %d (%s)" % (what, mode, form)
            _same_bits(g["rgb"], ref["rgb"], tag + " rgb")
            _same_hits(g, ref, tag, names={"t": "hit_t", "inst": "hit_inst", "prim": "hit_prim"})
            for k in ("normal", "albedo", "uv"):
                _same_bits(g[k], host3[k], "%s %s against the host form in mode 3" % (tag, k))
            if meshes is not None:
                assert_none_inert(meshes, g["inst"], g["prim"], tag)
    hit = np.asarray(frames[3]["hit_inst"]).reshape(-1) != MISS
    bary = np.asarray(frames[3]["rgb"], dtype=np.float32).reshape(-1, 3)[:, 1:3]  # a mode-3 colour is (1 - u - v, u, v)
    _same_bits(host3["uv"][hit], bary[hit], what + ": shade_rays uv against the mode-3 frame")
    assert not np.asarray(host3["uv"])[~hit].any(), what + ": shade_rays uv on a miss"

    _same_bits(got["path"]["rgb"], frames[200]["rgb"], what + ": path_rays chained over the samples, rgb")
    _same_hits(got["path"], frames[200], what + ": path_rays sample 0", names={"t": "hit_t", "inst": "hit_inst", "prim": "hit_prim"})
    if meshes is not None:
        assert_none_inert(meshes, got["path"]["inst"], got["path"]["prim"], what + ": path_rays")

    gd = got["guides"]
    for k in ("normal", "albedo", "t"):
        assert np.asarray(gd[k]).shape == ((h, w, 3) if k != "t" else (h, w)), "%s: frame_guides %s shape" % (what, k)
        _same_bits(gd[k], got["guides_ref"][k], "%s: frame_guides %s against shade_rays on the centre records" % (what, k))
        _same_bits(gd[k], host3[k], "%s: frame_guides %s against shade_rays in mode 3" % (what, k))
    N, A, T = (np.asarray(gd[k], dtype=np.float32).reshape(n, -1) for k in ("normal", "albedo", "t"))
    assert not N[~hit].any() and not A[~hit].any(), what + ": guides on a reference miss are not zero"
    _same_bits(T[~hit], np.full(int((~hit).sum()), TMAX, np.float32), what + ": guide t on a reference miss")
    _same_bits(T[hit], np.asarray(frames[3]["hit_t"]).reshape(-1)[hit], what + ": guide t on a reference hit")
    if scene is None:
        return
    inst, prim = np.asarray(frames[3]["hit_inst"]).reshape(-1)[hit], np.asarray(frames[3]["hit_prim"]).reshape(-1)[hit]
    ref_n, checked = geometric_normals(meshes, inst, prim, np.asarray(got["centre"])[hit, 4:7])
    if checked.any():
        err = np.abs(N[hit][checked].astype(np.float64) - ref_n[checked]).max()
        assert err <= NORMAL_TOL, "%s: guide normal %.3g off the float64 geometric normal" % (what, err)
    cache = {} if cache is None else cache
    if "albedo" not in cache:
        cache["albedo"] = expected_albedo(scene, inst, prim, bary[hit], texture_color)
    ref_a, checked = cache["albedo"]
    _same_bits(A[hit][checked], ref_a[checked], what + ": guide albedo")


def frame_records_equal_frames(renderer, frames, w, h, path_params, what, scene=None, texture_color=None, cache=None):
    """With the scene and the camera set: the centre records of camera_rays(w, h) through shade_rays in modes 3 and 100 (host
    form, with counting, device form) equal frames[mode] in rgb, t, inst and prim; the records of samples 0 .. spp - 1 through
    chained path_rays calls equal frames[200]; frame_guides equals shade_rays on the centre records, is (0, 0, 0, 10000) on
    reference misses, and on reference hits holds the frame's t, the geometric normal and the material's or texture's colour.
    Returns what was collected."""
    got = collect_frame_records(renderer, w, h, path_params)
    assert_frame_records(got, frames, w, h, what, scene, texture_color, cache)
    return got


# ---- caller rays with a brute-force closest-hit reference

def collect_arbitrary_records(renderer, rays):
    renderer.change_shading_mode(3)
    return {"shade": renderer.shade_rays(rays), "path": renderer.path_rays(rays, n_samples=2)}


def assert_arbitrary_records(got, trace_ref, what, meshes=None):
    for name in ("shade", "path"):
        _same_hits(got[name], trace_ref, "%s: %s_rays" % (what, name), keys=HIT_OUTPUTS)
        if meshes is not None:
            assert_none_inert(meshes, got[name]["inst"], got[name]["prim"], "%s: %s_rays" % (what, name))
    miss = np.asarray(trace_ref["inst"]).reshape(-1) == MISS
    assert not got["shade"]["normal"][miss].any() and not got["shade"]["albedo"][miss].any(), what + ": normal or albedo on a reference miss"


def arbitrary_records_equal_trace(renderer, rays, trace_ref, what, meshes=None):
    """t, uv, inst and prim of shade_rays (mode 3) and of path_rays (2 samples) equal the brute-force trace_rays reference bit
    for bit; shade_rays' normal and albedo are zero on reference misses"""
    got = collect_arbitrary_records(renderer, rays)
    assert_arbitrary_records(got, trace_ref, what, meshes)
    return got


# ---- poses: one arbitrary ray each, with a 1 x 1 oracle frame as its reference

def bounds(sc):
    """the box of the scene's finite vertices"""
    v = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    v = v[np.isfinite(v).all(axis=1)]
    return v.min(axis=0), v.max(axis=0)


def poses(sc, n=N_POSES, seed=POSE_SEED):
    """n seeded poses: positions in and around the scene's box (a tenth of its extent beyond it on every side), rotations
    random orthonormal float32 matrices"""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(sc)
    ext = hi - lo
    pos = (lo - 0.1 * ext + rng.random((n, 3)) * 1.2 * ext).astype(np.float32)
    rot = np.empty((n, 9), dtype=np.float32)
    for k in range(n):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        rot[k] = (q * np.sign(np.diag(r))).astype(np.float32).reshape(9)
    return pos, rot


def pose_rays(oracle, pos, rot):
    """the pixel-centre ray of the 1 x 1 frame at every pose (modes 0 .. 100)"""
    rays = np.empty((len(pos), 8), dtype=np.float32)
    for k in range(len(pos)):
        rays[k, 0:3], rays[k, 3], rays[k, 4:7], rays[k, 7] = pos[k], TMIN, oracle.ray_dir(rot[k], 0, 0, 1, 1), TMAX
    return rays


def pose_rays_200(pos, rot, seed, sample=0):
    """the jittered ray of that sample of the 1 x 1 mode-200 frame at every pose (pixel 0, so path id 0)"""
    return H.pose_records(R, pos, rot, seed, sample)


def pose_reference(oracle, sc, pos, rot, mode=100, build_mode=0, brute_force=False, path_params=None, meshes=None):
    """1 x 1 oracle frames: per pose the colour, the hit and the frame's statistics.  Mode 200 needs path_params (spp,
    max_bounces, seed), which are set in the oracle for the frames and put back to its defaults."""
    O = oracle.OracleScene(sc["meshes"] if meshes is None else meshes, sc["lights"], sc["materials"], build_mode=build_mode,
                           textures=sc.get("textures") or ())
    n = len(pos)
    ref = {"rgb": np.zeros((n, 3), np.float32), "inst": np.zeros(n, np.uint32), "prim": np.zeros(n, np.uint32),
           "t": np.zeros(n, np.float32), "shadow": np.zeros(n, np.uint64), "nodes": np.zeros(n, np.uint64), "tris": np.zeros(n, np.uint64)}
    try:
        if mode == 200:
            oracle.set_path_params(*path_params)
        for k in range(n):
            f = O.render(pos[k], rot[k], mode, 1, 1, n_threads=1, brute_force=brute_force)
            ref["rgb"][k], ref["inst"][k], ref["prim"][k], ref["t"][k] = f["rgb"][0, 0], f["hit_inst"][0, 0], f["hit_prim"][0, 0], f["hit_t"][0, 0]
            ref["shadow"][k], ref["nodes"][k], ref["tris"][k] = f["stats"]["rays_shadow"], f["stats"]["nodes_visited"], f["stats"]["tris_tested"]
    finally:
        if mode == 200:
            oracle.set_path_params(4, 3, 1234)
        O.close()
    return ref


def pose_set(oracle, sc, pos, rot, path_params, brute_force=True, meshes=None):
    """the poses' records and 1 x 1 oracle frames in modes 100 and 200: what pose_records_equal_oracle compares with"""
    spp, _, seed = path_params
    return {"pos": pos, "rot": rot, "path_params": tuple(path_params), "rays": pose_rays(oracle, pos, rot),
            "rays200": [pose_rays_200(pos, rot, seed, k) for k in range(spp)],
            100: pose_reference(oracle, sc, pos, rot, 100, brute_force=brute_force, meshes=meshes),
            200: pose_reference(oracle, sc, pos, rot, 200, brute_force=brute_force, path_params=path_params, meshes=meshes)}


def collect_pose_records(renderer, pose_ref):
    spp, bounces, seed = pose_ref["path_params"]
    renderer.set_path_params(spp, bounces, seed)
    renderer.change_shading_mode(100)
    zeros = np.zeros(len(pose_ref["rays"]), dtype=np.uint32)
    return {"shade": renderer.shade_rays(pose_ref["rays"]), "path": _path_chain(renderer, lambda k: pose_ref["rays200"][k], spp, ids=zeros)}


def assert_pose_records(got, pose_ref, what, meshes=None):
    for name, mode in (("shade", 100), ("path", 200)):
        tag = "%s: %s_rays on the poses" % (what, name)
        _same_bits(got[name]["rgb"], pose_ref[mode]["rgb"], tag + " rgb")
        _same_hits(got[name], pose_ref[mode], tag)
        if meshes is not None:
            assert_none_inert(meshes, got[name]["inst"], got[name]["prim"], tag)


def pose_records_equal_oracle(renderer, pose_ref, what, meshes=None):
    """mode-100 shade_rays on the poses' centre records and path_rays (ids = 0, chained over the samples) on their jittered
    records equal the 1 x 1 oracle frames bit for bit: rgb, t, inst and prim"""
    if not len(pose_ref["rays"]):
        return None
    got = collect_pose_records(renderer, pose_ref)
    assert_pose_records(got, pose_ref, what, meshes)
    return got
