"""The assertion helpers of tests/shaded_query_checks.py can fail (CPU only): each is fed its own reference as "device output" and
passes, and fails when one float of rgb is moved by one ulp, when one inst is swapped, and when the id of an inert triangle is put
in -- into the reference as well, so that nothing but the inert check can notice.  Nothing on the GPU is broken on purpose."""
import copy

import numpy as np
import pytest

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
    sc = dict(sc, meshes=meshes)
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
    O.close()
    scene = {"meshes": sc["meshes"], "materials": sc["materials"], "textures": None}
    return {"scene": scene, "frames": frames, "centre": centre, "trace": trace, "poses": poses,
            "inert_id": (0, int(np.flatnonzero(inert[0])[0]))}


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
                "uv": uv.copy(), "inst": f["hit_inst"].reshape(-1).copy(), "prim": f["hit_prim"].reshape(-1).copy()}
    f = frames[200]
    guides = {"normal": normal.reshape(H, W, 3).copy(), "albedo": albedo.reshape(H, W, 3).copy(), "t": t.reshape(H, W).copy()}
    return {"centre": ref["centre"], "shade": {m: {form: shade(m) for form in sq.FORMS} for m in (3, 100)},
            "path": {"rgb": f["rgb"].reshape(-1, 3).copy(), "t": f["hit_t"].reshape(-1).copy(), "uv": uv.copy(),
                     "inst": f["hit_inst"].reshape(-1).copy(), "prim": f["hit_prim"].reshape(-1).copy()},
            "guides": guides, "guides_ref": {k: v.reshape(n, -1).copy() for k, v in guides.items()}}


def _arbitrary_outputs(ref):
    tr = ref["trace"]
    hits = {k: tr[k].copy() for k in sq.HIT_OUTPUTS}
    hit = tr["inst"] != MISS
    ones = np.where(hit[:, None], np.float32(0.5), np.float32(0.0)) * np.ones((1, 3), np.float32)
    return {"shade": dict(copy.deepcopy(hits), rgb=ones.copy(), normal=ones.copy(), albedo=ones.copy()), "path": dict(copy.deepcopy(hits), rgb=ones.copy())}


def _pose_outputs(ref):
    P = ref["poses"]
    return {"shade": {k: np.array(P[100][k]) for k in ("rgb", "t", "inst", "prim")}, "path": {k: np.array(P[200][k]) for k in ("rgb", "t", "inst", "prim")}}


def _check_frames(ref, got, frames=None):
    sq.assert_frame_records(got, frames or ref["frames"], W, H, "self-check", scene=ref["scene"])


def _check_arbitrary(ref, got, trace=None):
    sq.assert_arbitrary_records(got, trace or ref["trace"], "self-check", meshes=ref["scene"]["meshes"])


def _check_poses(ref, got, poses=None):
    sq.assert_pose_records(got, poses or ref["poses"], "self-check", meshes=ref["scene"]["meshes"])


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
