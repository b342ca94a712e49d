"""The assertion helpers of tests/shaded_query_checks.py can fail (CPU only): each is fed its own reference as "device output" and
passes, and fails when one float of rgb is moved by one ulp, when one inst is swapped, and when the id of an inert triangle is put
in -- into the reference as well, so that nothing but the inert check can notice.  The halves for modes 120 and 150 are fed the
contract composed on the CPU and the oracle's frames along the specular chain, and fail on one ulp of their rgb, on one swapped
inst, on an inert id, and when the occlusion of one probe of K is flipped in the reference.  Nothing on the GPU is broken on
purpose."""
import copy

import numpy as np
import pytest

import deep_stack_scenes as D
import shaded_query_checks as sq

MISS = 0xFFFFFFFF
W, H = 24, 16
PATH_PARAMS = (2, 2, 99)


def _ulp_up(a, index):
    a.reshape(-1).view(np.uint32)[index] += 1


@pytest.fixture(scope="module")
def ref(pkg, oracle, scenes):
    """the Cornell box with vertex 0 of its first mesh a NaN: brute-force frames, a closest-hit reference of 300 rays and the
    references of 16 poses, and each of them restated as the outputs a faultless device would give"""
    sc = scenes.cornell_box()
    meshes = [dict(m) for m in sc["meshes"]]
    v = np.array(meshes[0]["vertices"], dtype=np.float32).reshape(-1, 3)
    v[0, 1] = np.nan
    meshes[0]["vertices"] = v
    # (the light's CONSTANT material made DIFFUSE: mode 150 is mode 100's on this scene; the mirror scene below has a chain)
    sc = dict(sc, meshes=meshes, materials=[dict(m, type=1) for m in sc["materials"]])
    assert not sq.departs_from_mode_100(sc)
    inert = sq.inert_mask(meshes)
    assert inert[0].any() and not inert[0].all()
    cam = sc["camera"]
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    oracle.set_path_params(*PATH_PARAMS)
    try:
        frames = {m: O.render(cam["position"], cam["matrix"], m, W, H, brute_force=True) for m in (3, 100, 200)}
    finally:
        oracle.set_path_params(4, 3, 1234)
    centre = np.zeros((W * H, 8), np.float32)
    centre[:, 0:3], centre[:, 3], centre[:, 7] = np.float32(cam["position"]), sq.TMIN, sq.TMAX
    for i in range(W * H):
        centre[i, 4:7] = oracle.ray_dir(cam["matrix"], i % W, i // W, W, H)
    rng = np.random.default_rng(3)
    lo, hi = sq.bounds(sc)
    o = (lo + rng.random((300, 3)) * (hi - lo)).astype(np.float32)
    rays = pkg.make_rays(o, rng.normal(size=(300, 3)).astype(np.float32), tmin=0.0, tmax=rng.choice([np.inf, 1.0], size=300))
    trace = oracle.trace_rays(O, rays, brute_force=True)
    pos, rot = sq.poses(sc, n=16)
    poses = sq.pose_set(oracle, sc, pos, rot, PATH_PARAMS)
    nodes = O.nodes()[:1].copy()
    O.close()
    scene = {"meshes": sc["meshes"], "materials": sc["materials"], "textures": None}
    world = {"oracle": oracle, "camera": (cam["position"], cam["matrix"]), "lights": sc["lights"]}
    return {"scene": scene, "frames": frames, "centre": centre, "trace": trace, "poses": poses, "world": world, "cache": {}, "nodes": nodes,
            "inert_id": (0, int(np.flatnonzero(inert[0])[0]))}


def _unorm(rgb):
    with np.errstate(invalid="ignore"):
        return (np.clip(np.nan_to_num(np.asarray(rgb, np.float32), nan=0.0), 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def _forms(outputs, stats):
    return {form: dict(copy.deepcopy(outputs), stats=dict(stats)) for form in sq.FORMS}


def _ambient_outputs(ref, rays, surface, hits, shadow100, size=None):
    """(collect_ambient_records' dict, ambient_reference's) of a faultless device: the contract composed on the CPU in every
    setting, in the three forms, with the counted rays and, with size = (w, h), as frames"""
    got = {"rays": rays, "seed": PATH_PARAMS[2], "pick": None, "nodes": ref["nodes"], "surface": copy.deepcopy(surface), "shadow100": shadow100,
           "runs": dict.fromkeys(sq.AO_SETTINGS)}
    aref = sq.ambient_reference(got, hits, ref["world"], dict(ref["scene"], lights=ref["world"]["lights"]), ref["cache"])
    n_hit = int((np.asarray(hits["inst"]) != MISS).sum())
    for (k, radius, sky), rgb in sq.ambient_colours(got, aref).items():
        run = _forms(dict(surface, rgb=rgb), {"rays_primary": len(rays), "rays_shadow": n_hit * k + (shadow100 if sky else 0)})
        if size is not None:
            w, h = size
            run["frame"] = {"rgb": rgb.reshape(h, w, 3).copy(), "hit_t": surface["t"].reshape(h, w).copy(), "hit_inst": surface["inst"].reshape(h, w).copy(),
                            "hit_prim": surface["prim"].reshape(h, w).copy(), "rgba8": np.dstack([_unorm(rgb.reshape(h, w, 3)), np.full((h, w), 255, np.uint8)])}
            run["full"] = run["host"]
        got["runs"][(k, radius, sky)] = run
    return got, aref


def _whitted_outputs(outputs, stats, frame=None):
    """collect_whitted_records' dict where nothing is specular: mode 100's outputs at max_bounces 0 and the path bounces"""
    runs = {}
    for B in sorted({0, PATH_PARAMS[1]}):
        runs[B] = _forms(outputs, stats)
        if frame is not None:
            runs[B]["frame"], runs[B]["full"] = copy.deepcopy(frame), runs[B]["host"]
    out = {"chain": False, "bounces": PATH_PARAMS[1], "runs": runs}
    if frame is not None:
        out["frame100"] = dict(frame["stats"])
    return out


def _frame_outputs(ref):
    """the reference frames as collect_frame_records' dict"""
    frames, scene = ref["frames"], ref["scene"]
    n = W * H
    inst, prim = frames[3]["hit_inst"].reshape(-1), frames[3]["hit_prim"].reshape(-1)
    hit = inst != MISS
    uv = np.where(hit[:, None], frames[3]["rgb"].reshape(-1, 3)[:, 1:3], 0.0).astype(np.float32)
    normal, albedo = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    normal[hit] = sq.geometric_normals(scene["meshes"], inst[hit], prim[hit], ref["centre"][hit, 4:7])[0].astype(np.float32)
    albedo[hit] = sq.expected_albedo(scene, inst[hit], prim[hit], uv[hit])[0]
    t = np.where(hit, frames[3]["hit_t"].reshape(-1), np.float32(sq.TMAX)).astype(np.float32)

    def shade(mode):
        f = frames[mode]
        return {"rgb": f["rgb"].reshape(-1, 3).copy(), "normal": normal.copy(), "albedo": albedo.copy(), "t": f["hit_t"].reshape(-1).copy(),
                "uv": uv.copy(), "inst": f["hit_inst"].reshape(-1).copy(), "prim": f["hit_prim"].reshape(-1).copy(),
                "stats": {"rays_primary": n, "rays_shadow": f["stats"]["rays_shadow"]}}
    f = frames[200]
    guides = {"normal": normal.reshape(H, W, 3).copy(), "albedo": albedo.reshape(H, W, 3).copy(), "t": t.reshape(H, W).copy()}
    surface = {k: v for k, v in shade(3).items() if k != "stats"}
    shadow100 = frames[100]["stats"]["rays_shadow"]
    ambient, aref = _ambient_outputs(ref, ref["centre"], surface, sq.frame_hits(frames), shadow100, size=(W, H))
    lambert = {k: v for k, v in shade(100).items() if k != "stats"}
    return {"centre": ref["centre"], "shade": {m: {form: shade(m) for form in sq.FORMS} for m in (3, 100)},
            "path": {"rgb": f["rgb"].reshape(-1, 3).copy(), "t": f["hit_t"].reshape(-1).copy(), "uv": uv.copy(),
                     "inst": f["hit_inst"].reshape(-1).copy(), "prim": f["hit_prim"].reshape(-1).copy()},
            "guides": guides, "guides_ref": {k: v.reshape(n, -1).copy() for k, v in guides.items()},
            "ambient": ambient, "ambient_ref": aref,
            "whitted": _whitted_outputs(lambert, {"rays_primary": n, "rays_shadow": shadow100}, frame=frames[100])}


def _arbitrary_outputs(ref):
    tr = ref["trace"]
    hits = {k: tr[k].copy() for k in sq.HIT_OUTPUTS}
    hit = tr["inst"] != MISS
    ones = np.where(hit[:, None], np.float32(0.5), np.float32(0.0)) * np.ones((1, 3), np.float32)
    return {"shade": dict(copy.deepcopy(hits), rgb=ones.copy(), normal=ones.copy(), albedo=ones.copy()), "path": dict(copy.deepcopy(hits), rgb=ones.copy())}


def _pose_outputs(ref):
    P = ref["poses"]
    n = len(P["rays"])
    hit = P[100]["inst"] != MISS
    normal, albedo = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    with np.errstate(invalid="ignore"):
        normal[hit] = sq.geometric_normals(ref["scene"]["meshes"], P[100]["inst"][hit], P[100]["prim"][hit], P["rays"][hit, 4:7])[0].astype(np.float32)
    albedo[hit] = sq.expected_albedo(ref["scene"], P[100]["inst"][hit], P[100]["prim"][hit], np.zeros((int(hit.sum()), 2), np.float32))[0]
    surface = {"normal": normal, "albedo": albedo, "uv": np.zeros((n, 2), np.float32), "t": np.array(P[100]["t"]), "inst": np.array(P[100]["inst"]),
               "prim": np.array(P[100]["prim"])}
    shadow100 = int(P[100]["shadow"].sum())
    ambient, aref = _ambient_outputs(ref, P["rays"], surface, dict(P[100], direct=P[100]["rgb"]), shadow100)
    lambert = dict(surface, rgb=np.array(P[100]["rgb"]))
    stats = {"rays_primary": n, "rays_shadow": shadow100}
    return {"shade": {k: np.array(P[100][k]) for k in ("rgb", "t", "inst", "prim")}, "path": {k: np.array(P[200][k]) for k in ("rgb", "t", "inst", "prim")},
            "shade100": _forms(lambert, stats), "ambient": ambient, "ambient_ref": aref, "whitted": _whitted_outputs(lambert, stats)}


def _check_frames(ref, got, frames=None, ambient_ref=None):
    """(the reference of mode 120 is made again from the frames by assert_frame_records unless one is passed)"""
    sq.assert_frame_records(got, frames or ref["frames"], W, H, "self-check", scene=dict(ref["scene"], lights=ref["world"]["lights"]),
                            world=ref["world"], cache=dict(ref["cache"]), ambient_ref=ambient_ref)


def _check_arbitrary(ref, got, trace=None):
    sq.assert_arbitrary_records(got, trace or ref["trace"], "self-check", meshes=ref["scene"]["meshes"])


def _check_poses(ref, got, poses=None, ambient_ref=None):
    sq.assert_pose_records(got, poses or ref["poses"], "self-check", meshes=ref["scene"]["meshes"], ambient_ref=ambient_ref)


def test_the_references_pass_as_device_output(ref):
    assert (ref["frames"][3]["hit_inst"] != MISS).sum() >= 32 and (ref["trace"]["inst"] != MISS).sum() > 100
    assert (ref["poses"][100]["inst"] != MISS).sum() >= 4
    _check_frames(ref, _frame_outputs(ref))
    _check_arbitrary(ref, _arbitrary_outputs(ref))
    _check_poses(ref, _pose_outputs(ref))


def _first_hit(inst):
    return int(np.flatnonzero(np.asarray(inst).reshape(-1) != MISS)[0])


FRAME_SPOTS = [("shade", 3, "host"), ("shade", 100, "counting"), ("shade", 100, "device"), ("path",)]


def _spot(got, where):
    for k in where:
        got = got[k]
    return got


@pytest.mark.parametrize("where", FRAME_SPOTS, ids=["-".join(map(str, w)) for w in FRAME_SPOTS])
def test_frame_check_fails_on_one_ulp_and_on_one_swapped_inst(ref, where):
    got = _frame_outputs(ref)
    k = _first_hit(_spot(got, where)["inst"])
    _ulp_up(_spot(got, where)["rgb"], 3 * k + 1)
    with pytest.raises(AssertionError, match="rgb"):
        _check_frames(ref, got)
    got = _frame_outputs(ref)
    _spot(got, where)["inst"][k] ^= 1
    with pytest.raises(AssertionError, match="inst"):
        _check_frames(ref, got)


def test_frame_check_fails_on_guides(ref):
    k = _first_hit(ref["frames"][3]["hit_inst"])
    miss = int(np.flatnonzero(ref["frames"][3]["hit_inst"].reshape(-1) == MISS)[0]) if (ref["frames"][3]["hit_inst"] == MISS).any() else None
    for name, index in (("normal", 3 * k), ("albedo", 3 * k + 2), ("t", k)):
        got = _frame_outputs(ref)
        _ulp_up(got["guides"][name], index)
        with pytest.raises(AssertionError, match="frame_guides " + name):
            _check_frames(ref, got)
    # guides and shade_rays wrong together: only the float64 normal and the material's colour can tell
    for name, index, match in (("normal", 3 * k, "geometric normal"), ("albedo", 3 * k, "guide albedo")):
        got = _frame_outputs(ref)
        for form in sq.FORMS:
            for mode in (3, 100):
                if name == "normal":
                    got["shade"][mode][form]["normal"][k] *= -1.0
                elif name == "albedo":
                    _ulp_up(got["shade"][mode][form]["albedo"], index)
        if name == "normal":
            got["guides"]["normal"].reshape(-1, 3)[k] *= -1.0
            got["guides_ref"]["normal"][k] *= -1.0
        else:
            _ulp_up(got["guides"][name], index)
            _ulp_up(got["guides_ref"][name], index)
        with pytest.raises(AssertionError, match=match):
            _check_frames(ref, got)
    if miss is not None:
        got = _frame_outputs(ref)
        for d in [got["guides"], got["guides_ref"]] + [got["shade"][m][f] for m in (3, 100) for f in sq.FORMS]:
            d["albedo"].reshape(-1, 3)[miss, 0] = 1.0
        with pytest.raises(AssertionError, match="miss"):
            _check_frames(ref, got)


def test_frame_check_fails_on_an_inert_id(ref):
    """the inert id goes into the reference too: the comparison with it passes, the inert check alone fails"""
    inst, prim = ref["inert_id"]
    frames = copy.deepcopy(ref["frames"])
    k = _first_hit(frames[3]["hit_inst"])
    for m in (3, 100, 200):
        frames[m]["hit_inst"].reshape(-1)[k], frames[m]["hit_prim"].reshape(-1)[k] = inst, prim
    with np.errstate(invalid="ignore"):
        got = _frame_outputs(dict(ref, frames=frames))
    with pytest.raises(AssertionError, match="inert"):
        _check_frames(ref, got, frames)


def test_arbitrary_check_fails(ref):
    k = _first_hit(ref["trace"]["inst"])
    miss = int(np.flatnonzero(ref["trace"]["inst"] == MISS)[0])
    for name in ("shade", "path"):
        got = _arbitrary_outputs(ref)
        _ulp_up(got[name]["t"], k)
        with pytest.raises(AssertionError, match=name + "_rays t"):
            _check_arbitrary(ref, got)
        got = _arbitrary_outputs(ref)
        _ulp_up(got[name]["uv"], 2 * k)
        with pytest.raises(AssertionError, match=name + "_rays uv"):
            _check_arbitrary(ref, got)
        got = _arbitrary_outputs(ref)
        got[name]["inst"][k] ^= 1
        with pytest.raises(AssertionError, match=name + "_rays inst"):
            _check_arbitrary(ref, got)
        trace = copy.deepcopy(ref["trace"])
        trace["inst"][k], trace["prim"][k] = ref["inert_id"]
        with pytest.raises(AssertionError, match="inert"):
            _check_arbitrary(ref, _arbitrary_outputs(dict(ref, trace=trace)), trace)
    got = _arbitrary_outputs(ref)
    got["shade"]["normal"][miss, 2] = np.float32(1e-30)
    with pytest.raises(AssertionError, match="miss"):
        _check_arbitrary(ref, got)


def test_pose_check_fails(ref):
    for name, mode in (("shade", 100), ("path", 200)):
        k = _first_hit(ref["poses"][mode]["inst"])
        got = _pose_outputs(ref)
        _ulp_up(got[name]["rgb"], 3 * k)
        with pytest.raises(AssertionError, match="rgb"):
            _check_poses(ref, got)
        got = _pose_outputs(ref)
        got[name]["inst"][k] ^= 1
        with pytest.raises(AssertionError, match="inst"):
            _check_poses(ref, got)
        poses = dict(ref["poses"])
        poses[mode] = {key: np.array(v) for key, v in poses[mode].items()}
        poses[mode]["inst"][k], poses[mode]["prim"][k] = ref["inert_id"]
        with pytest.raises(AssertionError, match="inert"):
            _check_poses(ref, _pose_outputs(dict(ref, poses=poses)), poses)


# ---- modes 120 and 150

NEW_SPOTS = [("ambient", "runs", (1, 0, 0), "host"), ("ambient", "runs", (5, 50, 1), "counting"), ("ambient", "runs", (5, 0, 1), "device"),
             ("whitted", "runs", 0, "device"), ("whitted", "runs", PATH_PARAMS[1], "host")]


@pytest.mark.parametrize("where", NEW_SPOTS, ids=["-".join(map(str, w)) for w in NEW_SPOTS])
def test_new_mode_checks_fail_on_one_ulp_and_on_one_swapped_inst(ref, where):
    for outputs, check in ((_frame_outputs, _check_frames), (_pose_outputs, _check_poses)):
        got = outputs(ref)
        k = _first_hit(_spot(got, where)["inst"])
        _ulp_up(_spot(got, where)["rgb"], 3 * k + 1)
        with pytest.raises(AssertionError, match="mode %d.* rgb" % (120 if where[0] == "ambient" else 150)):
            check(ref, got)
        got = outputs(ref)
        _spot(got, where)["inst"][k] ^= 1
        with pytest.raises(AssertionError, match="mode %d.* inst" % (120 if where[0] == "ambient" else 150)):
            check(ref, got)


def test_new_mode_checks_fail_on_frames_and_counted_rays(ref):
    got = _frame_outputs(ref)
    k = _first_hit(ref["frames"][3]["hit_inst"])
    _ulp_up(got["ambient"]["runs"][(5, 0, 0)]["frame"]["rgb"], 3 * k)
    with pytest.raises(AssertionError, match="render_frame rgb"):
        _check_frames(ref, got)
    got = _frame_outputs(ref)
    _ulp_up(got["whitted"]["runs"][0]["frame"]["rgb"], 3 * k)
    with pytest.raises(AssertionError, match="render_frame rgb"):
        _check_frames(ref, got)
    got = _frame_outputs(ref)
    got["ambient"]["runs"][(5, 50, 1)]["counting"]["stats"]["rays_shadow"] += 1
    with pytest.raises(AssertionError, match="any-hit rays"):
        _check_frames(ref, got)
    got = _frame_outputs(ref)
    got["whitted"]["runs"][PATH_PARAMS[1]]["counting"]["stats"]["rays_primary"] += 1
    with pytest.raises(AssertionError, match="rays_primary"):
        _check_frames(ref, got)


def test_ambient_check_fails_on_one_flipped_probe(ref):
    """one sample of K, occluded where it escaped or the other way, in the reference alone: the record's colour moves by 1 / K"""
    for outputs, check in ((_frame_outputs, _check_frames), (_pose_outputs, _check_poses)):
        got = outputs(ref)
        check(ref, got, ambient_ref=got["ambient_ref"])
        for radius, sample in ((0, 0), (50, 4)):
            flipped = copy.deepcopy(got["ambient_ref"])
            flipped["occluded"][radius][len(flipped["hit"]) // 2, sample] ^= True
            with pytest.raises(AssertionError, match="mode 120 K=%d ao_radius=%d.* rgb" % (1 if sample == 0 else 5, radius)):
                check(ref, got, ambient_ref=flipped)


def test_new_mode_checks_fail_on_an_inert_id(ref):
    """the inert id in the output and in the reference: every comparison passes, the inert check of each mode fails"""
    inst, prim = ref["inert_id"]
    frames = copy.deepcopy(ref["frames"])
    k = _first_hit(frames[3]["hit_inst"])
    for m in (3, 100, 200):
        frames[m]["hit_inst"].reshape(-1)[k], frames[m]["hit_prim"].reshape(-1)[k] = inst, prim
    with np.errstate(invalid="ignore"):
        got = _frame_outputs(dict(ref, frames=frames))
        for mode, match in ((120, "mode 120.*inert"), (150, "mode 150.*inert")):
            with pytest.raises(AssertionError, match=match):
                if mode == 120:
                    sq.assert_ambient_records(got["ambient"], got["ambient_ref"], "self-check", ref["scene"]["meshes"])
                else:
                    sq.assert_whitted_records(got["whitted"], frames[100], "self-check", ref["scene"]["meshes"], mode100=got["shade"][100])


def test_whitted_reference_counts_turns_and_its_check_fails(pkg, oracle):
    """the mirror in front of chain B: the frames of the turns-only copy are black or white and monotone in max_bounces
    (whitted_reference asserts it), pixels on the mirror turn once and the others never; the check passes on its own reference
    and fails on one ulp, on a swapped inst and when the frames of the copy are not monotone"""
    sc = D.mirror_and_chain_b()
    cam = sc["camera"]
    w, h, bounces, seed = 24, 16, 2, 77
    world = {"oracle": oracle, "camera": (cam["position"], cam["matrix"]), "lights": sc["lights"]}
    assert sq.departs_from_mode_100(sc) and not sq.departs_from_mode_100(D.plate_and_chain_b())
    wref = sq.whitted_reference(world, sc, w, h, bounces, seed, "self-check")
    assert (wref["turns"] == 1).sum() > 50 and (wref["turns"] == 0).sum() > 50 and set(wref["turns"].tolist()) == {0, 1}
    on = np.flatnonzero(wref["turns"] == 1)
    assert not np.array_equal(wref["rgb"][0][on], wref["rgb"][bounces][on]), "a turn changes the colour"
    assert len(np.unique(wref["rgb"][bounces][on], axis=0)) > len(on) // 8, "the colour behind a turn depends on where the mirrored ray arrived"

    def outputs():
        runs = {}
        for B in (0, bounces):
            o = {"rgb": wref["rgb"][B].copy(), "t": wref["t"].copy(), "inst": wref["inst"].copy(), "prim": wref["prim"].copy()}
            o.update({key: np.zeros((w * h, 2 if key == "uv" else 3), np.float32) for key in ("normal", "albedo", "uv")})
            runs[B] = _forms(o, {})
        return {"chain": True, "bounces": bounces, "runs": runs}
    sq.assert_whitted_records(outputs(), wref, "self-check", sc["meshes"])
    got = outputs()
    _ulp_up(got["runs"][bounces]["device"]["rgb"], 3 * int(on[0]))
    with pytest.raises(AssertionError, match="mode 150 max_bounces=2 .device. rgb"):
        sq.assert_whitted_records(got, wref, "self-check", sc["meshes"])
    got = outputs()
    got["runs"][0]["host"]["inst"][on[0]] ^= 1
    with pytest.raises(AssertionError, match="inst"):
        sq.assert_whitted_records(got, wref, "self-check", sc["meshes"])
    white, black = np.ones((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
    assert sq.assert_turn_counts([black, white, white], "self-check").tolist() == [1] * (w * h)
    with pytest.raises(AssertionError, match="white at m and black at m . 1"):
        sq.assert_turn_counts([black, white, black], "self-check")
    with pytest.raises(AssertionError, match="other than 0 and 1"):
        sq.assert_turn_counts([black, white * np.float32(0.5), white], "self-check")


def test_a_constant_material_departs_from_mode_100(oracle, scenes):
    """the Cornell box as it is, its light CONSTANT: mode 150 ends there with the material's colour as mode 200 does, at no turn
    (include/crt_hip.h), so its reference is the chain's, which passes as device output, and the mode-100 frame is not: the
    check against it fails on the light's pixels"""
    sc = scenes.cornell_box()
    assert sq.departs_from_mode_100(sc)
    cam = sc["camera"]
    w, h, bounces, seed = 96, 64, 2, 99
    world = {"oracle": oracle, "camera": (cam["position"], cam["matrix"]), "lights": sc["lights"]}
    wref = sq.whitted_reference(world, sc, w, h, bounces, seed, "self-check")
    assert not wref["turns"].any(), "nothing turns in the Cornell box"
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
    lambert = O.render(cam["position"], cam["matrix"], 100, w, h)
    O.close()
    constant = [i for i, m in enumerate(sc["meshes"]) if sc["materials"][m["material_index"]]["type"] == 4]
    on = np.flatnonzero(np.isin(wref["inst"], constant))
    assert len(on) > 0, "the camera sees the light"
    assert np.all(wref["rgb"][0][on] == np.float32(sc["materials"][sc["meshes"][constant[0]]["material_index"]]["albedo"]))

    def outputs(chain):
        runs = {}
        for B in (0, bounces):
            o = {"rgb": wref["rgb"][B].copy(), "t": wref["t"].copy(), "inst": wref["inst"].copy(), "prim": wref["prim"].copy()}
            o.update({key: np.zeros((w * h, 2 if key == "uv" else 3), np.float32) for key in ("normal", "albedo", "uv")})
            runs[B] = _forms(o, {})
        return {"chain": chain, "bounces": bounces, "runs": runs}
    sq.assert_whitted_records(outputs(True), wref, "self-check", sc["meshes"])
    with pytest.raises(AssertionError, match="mode 150 max_bounces=0 .host. rgb"):
        sq.assert_whitted_records(outputs(False), lambert, "self-check", sc["meshes"])
