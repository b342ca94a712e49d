"""Shared checks for the shaded, path-traced, camera-ray and guide queries (crt_shade_rays*, crt_path_rays*, crt_camera_rays*,
crt_frame_guides*, include/crt_hip.h) on scenes other test files build: poisoned, rebuilt, refitted, textured or far from the origin.
Every shaded kernel is meant: modes 3 and 100 of shade_kernels.hip, and the two kinds with phase machines of their own over
the shared traversal, mode 120 (ambient occlusion, ao_kernels.hip) and mode 150 (Whitted, whitted_kernels.hip), as queries in
their three forms and as frames (runShaded).  Mode 120 has a reference made on the CPU alone
(ambient_reference: the oracle's hits and direct light, tests/ao_reference.c, brute-force occlusion of the probes); mode 150 is
mode 100 where every material is mode 100's and the oracle's mode-200 frames along its chain elsewhere (whitted_reference).

A camera-ray record is the frame's ray bit for bit, so a reference frame (an oracle frame, brute force where the caller has one) is
the reference of w * h records; a 1 x 1 oracle frame is the reference of one arbitrary pose.  Every comparison here is exact (float
bits as uint32, ids by value) except the float64 geometric normal, which keeps test_shade_rays.test_attributes' bound of 1e-5.

Each check is split in two: collect_* runs the queries on a renderer, assert_* compares what was collected with the reference and
touches no GPU, so tests/test_shaded_query_checks.py can feed the assertions their own reference and one-value corruptions of it."""
import hashlib

import numpy as np

import ambient_checks as AO
import path_rays_helpers as H
import path_reference as R

MISS = 0xFFFFFFFF
TMIN, TMAX = 0.001, 10000.0
N_POSES, POSE_SEED = 256, 20
NORMAL_TOL = 1e-5  # per component, against the float64 unit normal: test_shade_rays.test_attributes' bound and reasoning
SHADE_OUTPUTS = ("rgb", "normal", "albedo", "t", "uv", "inst", "prim")
HIT_OUTPUTS = ("t", "uv", "inst", "prim")
FORMS = ("host", "counting", "device")
MISS_RGB = (0.0, 1.0, 1.0)  # the miss colour of a context and of the oracle's frames unless a caller sets another
AO_SETTINGS = tuple((k, radius, sky) for k in (1, 5) for radius in (0, 50) for sky in (0, 1))  # (ao_samples, ao_radius, ao_sky)
AO_DEFAULTS = (("ao_samples", 16), ("ao_radius", 0), ("ao_sky", 0))
# ray-triangle tests one check's brute-force probe reference may cost: about 10^8 a second and thread on the CPU, so a few seconds.
# A frame over a larger scene is checked on a seeded subset of its records
PROBE_TESTS = 4.0e8
SUBSET_SEED = 120


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


# ---- modes 120 (ambient occlusion) and 150 (Whitted): references made on the CPU alone

def n_triangles(meshes):
    return sum(len(np.asarray(m["triangles"]).reshape(-1, 3)) for m in meshes)


def departs_from_mode_100(scene):
    """some mesh of the scene has a REFLECTIVE, REFRACTIVE or CONSTANT material: mode 150 turns there, or ends with the
    material's colour as mode 200 does (include/crt_hip.h, "Whitted"); everywhere else it is mode 100"""
    mats = list(scene.get("materials") or ())
    for m in scene["meshes"]:
        mi = int(m.get("material_index", 0))
        if 0 <= mi < len(mats) and int(mats[mi].get("type", 1)) in (R.REFLECTIVE, R.REFRACTIVE, R.CONSTANT) and len(np.asarray(m["triangles"]).reshape(-1, 3)):
            return True
    return False


def turns_only(scene):
    """a copy of the scene that only counts turns: every material untextured white, those that are neither REFLECTIVE nor
    REFRACTIVE made CONSTANT, type and ior kept; no lights, no textures"""
    mats = []
    for m in scene.get("materials") or ():
        spec = int(m.get("type", 1)) in (R.REFLECTIVE, R.REFRACTIVE)
        mats.append({"albedo": (1.0, 1.0, 1.0), "type": int(m["type"]) if spec else R.CONSTANT, "ior": m.get("ior", 1.0),
                     "smooth_shading": m.get("smooth_shading", False)})
    n = len(mats)
    mats.append({"albedo": (1.0, 1.0, 1.0), "type": R.CONSTANT})  # for the meshes past the material table (white DIFFUSE there)
    meshes = [dict(m, material_index=mi if 0 <= mi < n else n) for m, mi in ((m, int(m.get("material_index", 0))) for m in scene["meshes"])]
    return dict(scene, meshes=meshes, materials=mats, lights=[], textures=[])


def _world_scene(world, scene, cache, key, build):
    """an oracle scene of the checks' own, kept in the caller's cache"""
    if key not in cache:
        sc = build(scene)
        cache[key] = world["oracle"].OracleScene(sc["meshes"], sc.get("lights") or (), sc.get("materials") or (), textures=list(sc.get("textures") or ()))
    return cache[key]


def assert_turn_counts(G, what):
    """G[m]: the frames of the turns-only copy under a white miss colour at max_bounces = m.  Every value is exactly 0 or
    exactly 1, and a record that is white at m is white at every larger m.  Returns k, the smallest m at which a record is
    white (len(G) where it never is)"""
    G = np.stack([np.asarray(g, dtype=np.float32).reshape(-1, 3) for g in G])
    bits = G.view(np.uint32)
    assert np.all((bits == 0) | (bits == 0x3F800000)), what + ": a frame of the turns-only copy holds a value other than 0 and 1"
    white = np.all(bits == 0x3F800000, axis=2)
    assert np.all(white | np.all(bits == 0, axis=2)), what + ": a record of the turns-only copy is neither black nor white"
    assert np.all(white[1:] >= white[:-1]), what + ": a record of the turns-only copy is white at m and black at m + 1"
    return np.where(white.any(axis=0), white.argmax(axis=0), len(G))


def whitted_reference(world, scene, w, h, bounces, seed, what, cache=None):
    """The oracle's restatement of mode 150 on the jittered records of sample 0 of a w x h frame (phong_ks = 0): for
    max_bounces = B in (0, bounces), rgb[i] = F[min(B, k_i)][i], F[m] the oracle's mode-200 frame at spp = 1, max_bounces = m and
    this seed, k_i the number of turns of record i, counted on the turns-only copy (assert_turn_counts); t, inst and prim are
    F[0]'s.  world: {"oracle": the module, "camera": (position, matrix), "lights": ..., "O": an oracle scene to render F on
    (optional; the scene is built here otherwise), "brute_force": frames by brute force (default: the tree walk), "miss": the
    miss colour the context holds (default MISS_RGB), "path_held": the mode-200 parameters the caller keeps in the oracle, which
    are put back (default: the oracle's own, 4, 3, 1234)}."""
    cache = {} if cache is None else cache
    oracle, (pos, rot) = world["oracle"], world["camera"]
    key = ("whitted", w, h, bounces, seed, np.float32(pos).tobytes(), np.float32(rot).tobytes())
    if key in cache:
        return cache[key]
    brute = bool(world.get("brute_force", False))
    O = world.get("O") or _world_scene(world, scene, cache, "oracle scene", lambda sc: dict(sc, lights=world["lights"]))
    T = _world_scene(world, scene, cache, "turns-only scene", turns_only)
    F, G = [], []
    try:
        for m in range(bounces + 1):
            oracle.set_path_params(1, m, seed)
            F.append(O.render(pos, rot, 200, w, h, miss_rgb=world.get("miss", MISS_RGB), brute_force=brute))
            G.append(T.render(pos, rot, 200, w, h, miss_rgb=(1.0, 1.0, 1.0), brute_force=brute)["rgb"])
    finally:
        oracle.set_path_params(*world.get("path_held", (4, 3, 1234)))
    k = assert_turn_counts(G, what)
    rgb = np.stack([np.asarray(f["rgb"], dtype=np.float32).reshape(-1, 3) for f in F])
    idx = np.arange(w * h)
    ref = {"turns": k, "t": F[0]["hit_t"].reshape(-1), "inst": F[0]["hit_inst"].reshape(-1), "prim": F[0]["hit_prim"].reshape(-1),
           "rgb": {B: rgb[np.minimum(B, k), idx] for B in sorted({0, bounces})}}
    cache[key] = ref
    return ref


def _set_ambient(renderer, k, radius, sky):
    for name, v in zip(("ao_samples", "ao_radius", "ao_sky"), (k, radius, sky)):
        renderer.set_option(name, v)
    renderer.change_shading_mode(120)


def record_subset(n, n_tris, k_most, n_radii):
    """the records of a call the brute-force probe reference can afford: all n, or a seeded sorted subset (at least 64)"""
    afford = int(PROBE_TESTS / max(1.0, float(n_tris) * k_most * n_radii))
    if afford >= n:
        return None
    return np.sort(np.random.default_rng(SUBSET_SEED).choice(n, size=max(64, afford), replace=False))


def collect_ambient_records(renderer, rays, seed, settings=AO_SETTINGS, frame=None, pick=None, leave_mode=100):
    """mode 120 on `rays` (a call of its own: a record's id is its index in it) in every setting and form, with the surface the
    contract draws from (shade_rays in mode 3, host form), mode 100's counted shadow rays and the root node as exported now.
    frame = (w, h, centre records): render_frame in every setting, and shade_rays of the whole frame's records; pick: the
    indices of `rays` in the frame (None: all of it).  An option cannot be read back, so the caller says what it holds: the
    option "seed" is set to `seed` and left so (the seed of the caller's path parameters), the ao_* options go back to their
    defaults (AO_DEFAULTS) and the mode to leave_mode."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    out = {"rays": rays, "seed": int(seed), "pick": pick, "runs": {}, "nodes": np.array(renderer.bvh_export()[0][:1])}
    renderer.set_option("seed", seed)
    try:
        renderer.change_shading_mode(3)
        out["surface"] = renderer.shade_rays(rays)
        renderer.change_shading_mode(100)
        renderer.set_counting(True)
        try:
            out["shadow100"] = int(renderer.shade_rays(rays, want=("inst",))["stats"]["rays_shadow"])
        finally:
            renderer.set_counting(False)
        for k, radius, sky in settings:
            _set_ambient(renderer, k, radius, sky)
            run = _shade_forms(renderer, rays)
            if frame is not None:
                w, h, centre = frame
                run["frame"] = renderer.render_frame(w, h)
                run["full"] = run["host"] if pick is None else renderer.shade_rays(centre)
            out["runs"][(k, radius, sky)] = run
    finally:
        for name, v in AO_DEFAULTS:
            renderer.set_option(name, v)
        renderer.change_shading_mode(leave_mode)
    return out


def ambient_reference(got, hits, world, scene, cache=None):
    """what assert_ambient_records compares with, from the CPU alone.  hits: {"t", "inst", "prim", "direct"} per record of
    got["rays"], the oracle's closest hit and its mode-100 colour; the occlusion of the probes is oracle.occluded_rays by
    brute force over the scene's triangles.  The normals the directions are drawn about are got["surface"]'s (module
    docstring of tests/ambient_checks.py).  Returns {"hit": indices, "t", "inst", "prim", "direct", "miss", "R": {radius: R},
    "occluded": {radius: (hits, K) bool}, "probes": number of probes traced}"""
    cache = {} if cache is None else cache
    L = AO.reference()
    inst = np.asarray(hits["inst"]).reshape(-1)
    hit = np.flatnonzero(inst != MISS)
    t = np.asarray(hits["t"], dtype=np.float32).reshape(-1)
    k_most = max(k for k, _, _ in got["runs"])
    ref = {"hit": hit, "t": t, "inst": inst, "prim": np.asarray(hits["prim"]).reshape(-1), "miss": np.float32(world.get("miss", MISS_RGB)),
           "direct": np.asarray(hits["direct"], dtype=np.float32).reshape(-1, 3), "R": {}, "occluded": {}, "probes": 0}
    O = world.get("O") or _world_scene(world, scene, cache, "oracle scene", lambda sc: dict(sc, lights=world["lights"]))
    normal = np.asarray(got["surface"]["normal"], dtype=np.float32).reshape(-1, 3)[hit]
    for radius in sorted({r for _, r, _ in got["runs"]}):
        Rr = AO.radius(L, radius, got["nodes"])
        probes = AO.probe_records(L, got["rays"][hit], t[hit], normal, hit, k_most, got["seed"], Rr)
        key = ("probes", hashlib.sha1(probes.tobytes()).digest())
        if key not in cache:
            cache[key] = world["oracle"].occluded_rays(O, probes, brute_force=True)["occluded"].astype(bool).reshape(len(hit), k_most)
        ref["R"][radius], ref["occluded"][radius] = Rr, cache[key]
        ref["probes"] += len(probes)
    return ref


def ambient_colours(got, ref):
    """{setting: the contract's rgb of every record of got["rays"]}: steps 4 and 5 from the number of a record's first K probes
    that escape, the albedo of got["surface"], the reference's direct light and miss colour"""
    L = AO.reference()
    hit = ref["hit"]
    albedo = np.asarray(got["surface"]["albedo"], dtype=np.float32).reshape(-1, 3)[hit]
    return {(k, radius, sky): AO.composed_rgb(L, len(got["rays"]), hit, (~ref["occluded"][radius][:, :k]).sum(axis=1), k, sky, albedo, ref["miss"],
                                             ref["direct"][hit]) for k, radius, sky in got["runs"]}


def assert_ambient_records(got, ref, what, meshes=None):
    """got: collect_ambient_records' dict; ref: ambient_reference's.  In every setting and form: rgb is the contract's colour
    for the number of the record's first K probes that escape, t / inst / prim are the oracle's, normal / albedo / uv are the
    mode-3 host form's bits; no inert triangle is reported; the counted any-hit rays are hits x K, plus mode 100's with
    ao_sky = 1; render_frame equals shade_rays of the frame's records byte for byte"""
    n, hit = len(got["rays"]), ref["hit"]
    surface = got["surface"]
    _same_hits(surface, ref, what + ": mode 3 under mode 120")
    colours = ambient_colours(got, ref)
    for (k, radius, sky), run in got["runs"].items():
        want = colours[(k, radius, sky)]
        for form in FORMS:
            g, tag = run[form], "%s: shade_rays mode 120 K=%d ao_radius=%d ao_sky=%d (%s)" % (what, k, radius, sky, form)
            _same_bits(g["rgb"], want, tag + " rgb")
            _same_hits(g, ref, tag)
            for key in ("normal", "albedo", "uv"):
                _same_bits(g[key], surface[key], "%s %s against the host form in mode 3" % (tag, key))
            if meshes is not None:
                assert_none_inert(meshes, g["inst"], g["prim"], tag)
        counted = run["counting"]["stats"]
        assert counted["rays_shadow"] == len(hit) * k + (got["shadow100"] if sky else 0), "%s: K=%d ao_radius=%d ao_sky=%d: %d any-hit rays counted, %d hits" % (
            what, k, radius, sky, counted["rays_shadow"], len(hit))
        assert counted["rays_primary"] == n, what + ": mode 120 rays_primary"
        if "frame" in run:
            _assert_frame_is_its_query(run["frame"], run["full"], "%s: mode 120 K=%d ao_radius=%d ao_sky=%d" % (what, k, radius, sky))
            if got["pick"] is not None:
                for key in ("t", "inst", "prim", "normal", "albedo", "uv"):  # (rgb draws from the record's index: the subset is another query)
                    (_same_ids if key in ("inst", "prim") else _same_bits)(np.asarray(run["full"][key])[got["pick"]], run["host"][key],
                                                                           "%s: mode 120 %s of the subset against the whole frame's" % (what, key))


def _assert_frame_is_its_query(frame, query, what):
    """render_frame's rgb / hit_t / hit_inst / hit_prim are shade_rays' of the frame's records byte for byte, rgba8 their
    colour quantised"""
    _same_bits(frame["rgb"], query["rgb"], what + ": render_frame rgb against shade_rays of camera_rays")
    _same_hits(query, frame, what + ": shade_rays of camera_rays against render_frame", names={"t": "hit_t", "inst": "hit_inst", "prim": "hit_prim"})
    rgb = np.asarray(query["rgb"], dtype=np.float32).reshape(frame["rgba8"].shape[0], frame["rgba8"].shape[1], 3)
    with np.errstate(invalid="ignore"):
        unorm = (np.clip(np.nan_to_num(rgb, nan=0.0), 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(frame["rgba8"][..., :3], unorm) and np.all(frame["rgba8"][..., 3] == 255), what + ": rgba8"


def collect_whitted_records(renderer, recs, bounces, chain, frame=None, leave_mode=100):
    """mode 150 at max_bounces 0 and `bounces` in the three forms on `recs` (the centre records where no material departs from mode 100 (departs_from_mode_100), the
    jittered records of sample 0 otherwise); frame = (w, h, centre records): render_frame as well, with shade_rays of the
    centre records.  Puts back max_bounces and the mode"""
    out = {"chain": bool(chain), "bounces": int(bounces), "runs": {}}
    try:
        if frame is not None and not chain:  # the counted rays of the mode-100 frame, which mode 150's must equal
            renderer.change_shading_mode(100)
            renderer.set_counting(True)
            try:
                out["frame100"] = renderer.render_frame(frame[0], frame[1], want=("rgba8",))["stats"]
            finally:
                renderer.set_counting(False)
        for B in sorted({0, int(bounces)}):
            renderer.set_option("max_bounces", B)
            renderer.change_shading_mode(150)
            run = _shade_forms(renderer, recs)
            if frame is not None:
                w, h, centre = frame
                renderer.set_counting(True)
                try:
                    run["frame"] = renderer.render_frame(w, h)
                finally:
                    renderer.set_counting(False)
                run["full"] = renderer.shade_rays(centre) if chain else run["host"]
            out["runs"][B] = run
    finally:
        renderer.set_option("max_bounces", bounces)
        renderer.change_shading_mode(leave_mode)
    return out


def assert_whitted_records(got, ref, what, meshes=None, mode100=None):
    """got: collect_whitted_records' dict.  Where no material departs from mode 100 (departs_from_mode_100) ref is the mode-100 reference (a frame, or the poses'
    dict) and mode100 the collected mode-100 forms of the same records: every output of shade_rays and the frame are mode
    100's, as are the counted rays.  Otherwise ref is whitted_reference's or pose_whitted_reference's"""
    framed = "hit_t" in ref
    names = {"t": "hit_t", "inst": "hit_inst", "prim": "hit_prim"} if framed else None
    for B, run in got["runs"].items():
        want = ref["rgb"][B] if got["chain"] else ref["rgb"]
        for form in FORMS:
            g, tag = run[form], "%s: shade_rays mode 150 max_bounces=%d (%s)" % (what, B, form)
            _same_bits(g["rgb"], want, tag + " rgb")
            _same_hits(g, ref, tag, names=names)
            for key in ("normal", "albedo", "uv"):
                _same_bits(g[key], run["host"][key], "%s %s against the host form" % (tag, key))
            if meshes is not None:
                assert_none_inert(meshes, g["inst"], g["prim"], tag)
        tag = "%s: mode 150 max_bounces=%d" % (what, B)
        if not got["chain"] and mode100 is not None:
            for key in ("normal", "albedo", "uv"):
                _same_bits(run["host"][key], mode100["host"][key], "%s %s against mode 100" % (tag, key))
            for key in ("rays_primary", "rays_shadow"):
                assert run["counting"]["stats"][key] == mode100["counting"]["stats"][key], "%s: %s is not mode 100's" % (tag, key)
        if "frame" not in run:
            continue
        _assert_frame_is_its_query(run["frame"], run["full"], tag)
        if meshes is not None:
            assert_none_inert(meshes, run["frame"]["hit_inst"], run["frame"]["hit_prim"], tag + " render_frame")
        if not got["chain"]:
            _same_bits(run["frame"]["rgb"], ref["rgb"], tag + " render_frame rgb against the mode-100 frame")
            if "rgba8" in ref:
                assert np.array_equal(run["frame"]["rgba8"], ref["rgba8"]), tag + " render_frame rgba8 against the mode-100 frame"
            for key in ("rays_primary", "rays_shadow"):  # (the fetch counts of a mode-100 frame are its packets': not compared)
                assert run["frame"]["stats"][key] == got["frame100"][key], "%s: render_frame %s is not the mode-100 frame's" % (tag, key)


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


def collect_frame_records(renderer, w, h, path_params, scene):
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
    pick = record_subset(w * h, n_triangles(scene["meshes"]), max(k for k, _, _ in AO_SETTINGS), len({r for _, r, _ in AO_SETTINGS}))
    got["ambient"] = collect_ambient_records(renderer, centre if pick is None else centre[pick], seed, frame=(w, h, centre), pick=pick)
    chain = departs_from_mode_100(scene)
    got["whitted"] = collect_whitted_records(renderer, renderer.camera_rays(w, h, sample=0) if chain else centre, bounces, chain, frame=(w, h, centre))
    return got


def frame_hits(frames, pick=None):
    """the reference frames as ambient_reference's hits: the mode-3 frame's closest hit and the mode-100 frame's colour"""
    pick = slice(None) if pick is None else pick
    return {"t": np.asarray(frames[3]["hit_t"]).reshape(-1)[pick], "inst": np.asarray(frames[3]["hit_inst"]).reshape(-1)[pick],
            "prim": np.asarray(frames[3]["hit_prim"]).reshape(-1)[pick], "direct": np.asarray(frames[100]["rgb"]).reshape(-1, 3)[pick]}


def assert_surface(surface, rays, scene, what, texture_color=None):
    """the mode-3 outputs the mode-120 reference draws from are right by themselves: on the hits, the normal is within NORMAL_TOL
    of the float64 geometric normal (meshes without vertex normals) and the albedo is the material's or, with the oracle's
    texture_color, the texture's colour (expected_albedo); on the misses both are zero"""
    inst, prim = np.asarray(surface["inst"]).reshape(-1), np.asarray(surface["prim"]).reshape(-1)
    hit = inst != MISS
    N, alb = (np.asarray(surface[k], dtype=np.float32).reshape(-1, 3) for k in ("normal", "albedo"))
    assert not N[~hit].any() and not alb[~hit].any(), what + ": normal or albedo on a miss"
    ref_n, checked = geometric_normals(scene["meshes"], inst[hit], prim[hit], np.asarray(rays)[hit, 4:7])
    if checked.any():
        err = np.abs(N[hit][checked].astype(np.float64) - ref_n[checked]).max()
        assert err <= NORMAL_TOL, "%s: normal %.3g off the float64 geometric normal" % (what, err)
    ref_a, checked = expected_albedo(scene, inst[hit], prim[hit], np.asarray(surface["uv"], dtype=np.float32).reshape(-1, 2)[hit], texture_color)
    _same_bits(alb[hit][checked], ref_a[checked], what + ": albedo")


def assert_new_modes(got, frames, w, h, what, scene, world, cache=None, ambient_ref=None, whitted_ref=None, texture_color=None):
    """modes 120 and 150 of collect_frame_records' dict against references made on the CPU (ambient_reference over the
    frames' hits; the mode-100 frame, or whitted_reference where a material departs from mode 100); a caller may pass
    references of its own.  The normal and the albedo the mode-120 reference draws from are held by assert_surface
    (texture_color: the oracle's, for textured hits)"""
    if ambient_ref is None:
        ambient_ref = ambient_reference(got["ambient"], frame_hits(frames, got["ambient"]["pick"]), world, scene, cache)
    assert_surface(got["ambient"]["surface"], got["ambient"]["rays"], scene, what + ": mode 3 under mode 120", texture_color)
    assert_ambient_records(got["ambient"], ambient_ref, what, scene["meshes"])
    wh = got["whitted"]
    assert wh["chain"] == departs_from_mode_100(scene), what + ": mode 150 was collected for another kind of scene"
    if whitted_ref is None:
        whitted_ref = whitted_reference(world, scene, w, h, wh["bounces"], got["ambient"]["seed"], what, cache) if wh["chain"] else frames[100]
    assert_whitted_records(wh, whitted_ref, what, scene["meshes"], mode100=got["shade"][100])


def new_modes_equal_references(renderer, frames, w, h, bounces, seed, what, scene, world, cache=None, settings=AO_SETTINGS,
                               held=(3, 1234, 0), texture_color=None):
    """the part of frame_records_equal_frames on modes 120 and 150 alone, for a caller that holds only frames[3] and
    frames[100]: a query in the three forms and a frame of each mode, in the given settings of mode 120 and at max_bounces 0
    and `bounces` in mode 150; the mode-3 normal and albedo under mode 120 are held as assert_surface says.  held: the
    (max_bounces, seed, mode) the caller's context holds (an option cannot be read back; default: a context's own), which are
    put back with the ao_* options"""
    try:
        renderer.set_option("max_bounces", bounces)
        renderer.set_option("seed", seed)
        centre = renderer.camera_rays(w, h)
        renderer.change_shading_mode(100)
        got = {"shade": {100: _shade_forms(renderer, centre)}}
        pick = record_subset(w * h, n_triangles(scene["meshes"]), max(k for k, _, _ in settings), len({r for _, r, _ in settings}))
        got["ambient"] = collect_ambient_records(renderer, centre if pick is None else centre[pick], seed, settings, frame=(w, h, centre), pick=pick)
        chain = departs_from_mode_100(scene)
        got["whitted"] = collect_whitted_records(renderer, renderer.camera_rays(w, h, sample=0) if chain else centre, bounces, chain, frame=(w, h, centre))
    finally:
        renderer.set_option("max_bounces", held[0])
        renderer.set_option("seed", held[1])
        renderer.change_shading_mode(held[2])
    assert_new_modes(got, frames, w, h, what, scene, world, cache, texture_color=texture_color)
    return got


def assert_frame_records(got, frames, w, h, what, scene=None, texture_color=None, cache=None, world=None, ambient_ref=None, whitted_ref=None):
    """got: collect_frame_records' dict; frames: {3, 100, 200: a reference frame}; scene: {meshes (the vertices as uploaded,
    poisoned ones included), materials, textures} for the checks on normal, albedo and inert ids; cache: a dict the caller keeps
    with `frames`, where the expected albedo of these frames, the oracle scenes of the checks' own and the probes' occlusion
    are computed once; world: {"oracle": the oracle module, "camera": (position, matrix), "lights": the scene's} for the
    references of modes 120 and 150 (whitted_reference, ambient_reference)"""
    n = w * h
    meshes = scene["meshes"] if scene is not None else None
    assert scene is not None and (world is not None or (ambient_ref is not None and whitted_ref is not None)), what + ": modes 120 and 150 need the scene and the oracle"
    cache = {} if cache is None else cache
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
    assert_new_modes(got, frames, w, h, what, scene, world, cache, ambient_ref, whitted_ref, texture_color=texture_color)


def frame_records_equal_frames(renderer, frames, w, h, path_params, what, scene=None, texture_color=None, cache=None, world=None):
    """With the scene and the camera set: the centre records of camera_rays(w, h) through shade_rays in modes 3 and 100 (host
    form, with counting, device form) equal frames[mode] in rgb, t, inst and prim; the records of samples 0 .. spp - 1 through
    chained path_rays calls equal frames[200]; frame_guides equals shade_rays on the centre records, is (0, 0, 0, 10000) on
    reference misses, and on reference hits holds the frame's t, the geometric normal and the material's or texture's colour.
    Modes 120 and 150, the kernels with phase machines of their own (ao_kernels.hip, whitted_kernels.hip), in the three forms
    and as frames: mode 120 in every setting of AO_SETTINGS equals the contract composed on the CPU (ambient_reference: the
    frames' hits, tests/ao_reference.c, brute-force occlusion of the probes; over a large scene on a seeded subset of the
    records), mode 150 at max_bounces 0 and the path bounces equals frames[100] where no material departs from mode 100 (departs_from_mode_100) and the oracle's
    mode-200 frames along the specular chain otherwise (whitted_reference).  Needs scene (with its materials) and world
    (assert_frame_records).  Returns what was collected."""
    assert scene is not None and world is not None, what + ": modes 120 and 150 need the scene and the oracle"
    got = collect_frame_records(renderer, w, h, path_params, scene)
    assert_frame_records(got, frames, w, h, what, scene, texture_color, cache, world)
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


def pose_reference(oracle, sc, pos, rot, mode=100, build_mode=0, brute_force=False, path_params=None, meshes=None, miss_rgb=MISS_RGB):
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
            f = O.render(pos[k], rot[k], mode, 1, 1, miss_rgb=miss_rgb, n_threads=1, brute_force=brute_force)
            ref["rgb"][k], ref["inst"][k], ref["prim"][k], ref["t"][k] = f["rgb"][0, 0], f["hit_inst"][0, 0], f["hit_prim"][0, 0], f["hit_t"][0, 0]
            ref["shadow"][k], ref["nodes"][k], ref["tris"][k] = f["stats"]["rays_shadow"], f["stats"]["nodes_visited"], f["stats"]["tris_tested"]
    finally:
        if mode == 200:
            oracle.set_path_params(4, 3, 1234)
        O.close()
    return ref


def pose_whitted_reference(oracle, sc, pos, rot, bounces, seed, brute_force=True):
    """whitted_reference for the poses' jittered records of sample 0, from 1 x 1 frames"""
    T = turns_only(sc)
    F = [pose_reference(oracle, sc, pos, rot, 200, brute_force=brute_force, path_params=(1, m, seed)) for m in range(bounces + 1)]
    G = [pose_reference(oracle, T, pos, rot, 200, brute_force=brute_force, path_params=(1, m, seed), miss_rgb=(1.0, 1.0, 1.0))["rgb"]
         for m in range(bounces + 1)]
    k = assert_turn_counts(G, "the poses")
    rgb = np.stack([f["rgb"] for f in F])
    return {"turns": k, "t": F[0]["t"], "inst": F[0]["inst"], "prim": F[0]["prim"],
            "rgb": {B: rgb[np.minimum(B, k), np.arange(len(pos))] for B in sorted({0, bounces})}}


def pose_set(oracle, sc, pos, rot, path_params, brute_force=True, meshes=None):
    """the poses' records and 1 x 1 oracle frames in modes 100 and 200: what pose_records_equal_oracle compares with.  For modes
    120 and 150 it keeps the scene, the oracle and a cache for the probes' occlusion, and where the scene has mirrors or glass
    the reference of mode 150 along the specular chain"""
    spp, bounces, seed = path_params
    scene = dict(sc, meshes=sc["meshes"] if meshes is None else meshes)
    out = {"pos": pos, "rot": rot, "path_params": tuple(path_params), "rays": pose_rays(oracle, pos, rot),
           "rays200": [pose_rays_200(pos, rot, seed, k) for k in range(spp)],
           100: pose_reference(oracle, sc, pos, rot, 100, brute_force=brute_force, meshes=meshes),
           200: pose_reference(oracle, sc, pos, rot, 200, brute_force=brute_force, path_params=path_params, meshes=meshes),
           "scene": scene, "world": {"oracle": oracle, "lights": sc["lights"]}, "cache": {}, "chain": departs_from_mode_100(scene)}
    if out["chain"] and len(pos):
        out[150] = pose_whitted_reference(oracle, scene, pos, rot, bounces, seed, brute_force)
    return out


def collect_pose_records(renderer, pose_ref):
    spp, bounces, seed = pose_ref["path_params"]
    renderer.set_path_params(spp, bounces, seed)
    renderer.change_shading_mode(100)
    zeros = np.zeros(len(pose_ref["rays"]), dtype=np.uint32)
    got = {"shade": renderer.shade_rays(pose_ref["rays"]), "path": _path_chain(renderer, lambda k: pose_ref["rays200"][k], spp, ids=zeros)}
    got["shade100"] = _shade_forms(renderer, pose_ref["rays"])
    got["ambient"] = collect_ambient_records(renderer, pose_ref["rays"], seed)
    got["whitted"] = collect_whitted_records(renderer, pose_ref["rays200"][0] if pose_ref["chain"] else pose_ref["rays"], bounces, pose_ref["chain"])
    return got


def assert_pose_records(got, pose_ref, what, meshes=None, ambient_ref=None):
    for name, mode in (("shade", 100), ("path", 200)):
        tag = "%s: %s_rays on the poses" % (what, name)
        _same_bits(got[name]["rgb"], pose_ref[mode]["rgb"], tag + " rgb")
        _same_hits(got[name], pose_ref[mode], tag)
        if meshes is not None:
            assert_none_inert(meshes, got[name]["inst"], got[name]["prim"], tag)
    if ambient_ref is None:
        hits = dict(pose_ref[100], direct=pose_ref[100]["rgb"])
        ambient_ref = ambient_reference(got["ambient"], hits, pose_ref["world"], pose_ref["scene"], pose_ref["cache"])
    assert_surface(got["ambient"]["surface"], got["ambient"]["rays"], pose_ref["scene"], what + ": the poses, mode 3 under mode 120",
                   pose_ref["world"]["oracle"].texture_color)
    assert_ambient_records(got["ambient"], ambient_ref, what + ": the poses", meshes)
    assert_whitted_records(got["whitted"], pose_ref[150] if pose_ref["chain"] else pose_ref[100], what + ": the poses", meshes, mode100=got["shade100"])


def pose_records_equal_oracle(renderer, pose_ref, what, meshes=None):
    """mode-100 shade_rays on the poses' centre records and path_rays (ids = 0, chained over the samples) on their jittered
    records equal the 1 x 1 oracle frames bit for bit: rgb, t, inst and prim.  Mode 120 on the centre records (every setting of
    AO_SETTINGS, the three forms) equals the contract composed on the CPU from those frames; mode 150 equals the mode-100 frames
    where no material departs from mode 100 (departs_from_mode_100), and on the jittered records of sample 0 the oracle's mode-200 frames along the chain otherwise"""
    if not len(pose_ref["rays"]):
        return None
    got = collect_pose_records(renderer, pose_ref)
    assert_pose_records(got, pose_ref, what, meshes)
    return got
