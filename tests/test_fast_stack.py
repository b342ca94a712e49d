"""The render kernel's pops (traversal.hip.h, Stack::popLds): an entry in the LDS part of the stack is read with an LDS load and
an entry in the spill arena with a global load, under a per-lane branch, where Stack::pop selects an address and loads through the
flat path.  Same entries in the same order, so small frames rendered with LDS parts of 1 .. 16 entries -- rays that live almost
entirely in the spill arena, rays that cross between the two parts again and again, rays that never leave LDS; wavefronts whose
lanes are on both sides of one pop -- must be the oracle's frame for frame and counter for counter, as in test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 96, 64
STACK_ENTRIES = (1, 3, 6, 7, 8, 12, 16)
NODE_DECISION_ROOM = 6  # LayLegacy::kStackPerLevel * NODE_STEPS
PATH_SPP, PATH_BOUNCES, PATH_SEED = 1, 2, 77
SCENES = ("heightfield", "soup")


def _scene(scenes, name):
    if name == "heightfield":
        return scenes.heightfield(n=64, n_lights=2, width=W, height=H)  # 8 194 triangles, two shadow rays per hit
    return scenes.icosphere_soup(n_spheres=120, subdiv=1, width=W, height=H)  # 9 602 triangles


@pytest.fixture(scope="module")
def refs(oracle, scenes):
    """per scene: the scene, the oracle's frames of modes 3, 100 and 200, and the deepest stack of every pixel's rays (mode 100:
    the primary ray and its shadow rays) in the oracle's own walk of the same 4-wide tree.  Computed once, never changed."""
    out = {}
    for name in SCENES:
        sc = _scene(scenes, name)
        cam = sc["camera"]
        O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
        frames = {mode: O.render(cam["position"], cam["matrix"], mode, W, H) for mode in (3,)}
        depth = np.zeros((H, W), dtype=np.uint32)
        oracle.lib().oracle_set_stack_output(depth.ctypes.data_as(C.c_void_p))
        try:
            frames[100] = O.render(cam["position"], cam["matrix"], 100, W, H)
        finally:
            oracle.lib().oracle_set_stack_output(None)
        oracle.set_path_params(PATH_SPP, PATH_BOUNCES, PATH_SEED)
        try:
            frames[200] = O.render(cam["position"], cam["matrix"], oracle.MODE_PATH, W, H, miss_rgb=(0.0, 0.0, 0.0))
        finally:
            oracle.set_path_params(4, 3, 1234)
        out[name] = {"scene": sc, "frames": frames, "depth": depth}
        O.close()
    return out


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _upload(renderer, sc):
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"])
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])


def _check(renderer, ref, what):
    """the plain kernel's frame and the counting kernel's frame and counters against the oracle's"""
    for counting in (False, True):
        renderer.set_counting(counting)
        got = renderer.render_frame(W, H)
        for k in ("hit_inst", "hit_prim", "hit_t", "rgba8"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s counting=%d" % (what, k, counting))
        assert np.array_equal(got["rgb"], ref["rgb"], equal_nan=True), "%s rgb counting=%d" % (what, counting)
        if counting:
            st, rs = got["stats"], ref["stats"]
            for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested"):
                assert st[k] == rs[k], "%s %s" % (what, k)


def _frames(pkg, renderer, ref, what):
    for mode in (3, 100):
        renderer.change_shading_mode(mode)
        _check(renderer, ref["frames"][mode], "%s mode %d" % (what, mode))
    renderer.change_shading_mode(pkg.MODE_PATH)
    renderer.set_path_params(PATH_SPP, PATH_BOUNCES, PATH_SEED)
    renderer.set_miss_color((0.0, 0.0, 0.0))
    try:
        _check(renderer, ref["frames"][200], "%s mode 200" % what)
    finally:
        renderer.set_path_params(4, 3, 1234)
        renderer.set_miss_color((0.0, 1.0, 1.0))


@pytest.mark.parametrize("name", SCENES)
def test_scenes_leave_the_lds_part(refs, name):
    """The oracle's own per-pixel stack depth: some ray needs more entries than the smallest LDS part used, so the frames below
    cannot pass without ever leaving the LDS part; some ray stands above 12 - 6 entries, so at 7, 8 and 12 entries there are rays
    with less than a node decision's room (kStackPerLevel * NODE_STEPS pushes) below the LDS part's end; 16 entries hold every ray."""
    depth = refs[name]["depth"]
    deepest = int(depth.max())
    print("%s: deepest stack %d, pixels deeper than 1: %d" % (name, deepest, int((depth > 1).sum())))
    assert deepest > min(STACK_ENTRIES)
    assert deepest > 12 - NODE_DECISION_ROOM
    assert deepest <= 16


@pytest.mark.parametrize("name", SCENES)
def test_frames_match_the_oracle_at_every_lds_depth(pkg, refs, renderer, name):
    ref = refs[name]
    _upload(renderer, ref["scene"])
    try:
        for entries in STACK_ENTRIES:
            renderer.set_option("stack_entries", entries)
            _frames(pkg, renderer, ref, "%s stack_entries=%d" % (name, entries))
    finally:
        renderer.set_counting(False)
        renderer.set_option("stack_entries", 0)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("inner_min", (1, 40))
def test_hand_over_in_node_and_leaf_phases(pkg, refs, renderer, name, inner_min):
    """inner_min = inner_min_any = 1: leaves wait until no lane stands on an inner node, so nearly every pop from the spill arena
    is a node step's; 40: leaves are served as soon as fewer than 40 lanes stand on inner nodes, so the pops that end a leaf phase
    often find lanes on both sides of the LDS part's end."""
    ref = refs[name]
    _upload(renderer, ref["scene"])
    try:
        renderer.set_option("inner_min", inner_min)
        renderer.set_option("inner_min_any", inner_min)
        for entries in (1, 3, 8):
            renderer.set_option("stack_entries", entries)
            _frames(pkg, renderer, ref, "%s inner_min=%d stack_entries=%d" % (name, inner_min, entries))
    finally:
        renderer.set_counting(False)
        for k, v in (("inner_min", -6), ("inner_min_any", -6), ("stack_entries", 0)):
            renderer.set_option(k, v)
