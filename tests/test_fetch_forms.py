"""The render kernel's fetch forms (traversal.hip.h, PAIR / NARROW of closestIteration / anyIteration): a leaf pair's six loads are
issued in front of their first wait, and a per-lane node or triangle record is addressed by a 32-bit byte offset from the
wave-uniform base unless the scene's arrays are too long for that (option "wide_offsets", crt::wideOffsets).  Neither touches a
ray's steps, so small frames rendered in either form -- with the stack in LDS and almost wholly in the spill arena, with packets
that have inactive lanes, by the plain and the counting kernel, whole and as a two-rank tile share -- must be the oracle's frame
for frame and counter for counter, as in test_fast_stack.py.  The SPLIT variant keeps the 64-bit form (its streams walk the tree
with the shared default traversal), so no split-packet launch is needed here; test_gpu_parity.py holds those to the oracle."""
import numpy as np
import pytest

SIZES = ((96, 64), (70, 50))  # the second leaves packets with inactive lanes
SCENES = ("heightfield", "soup")
SHADINGS = ((3, 0), (100, 0), (100, 300))  # (mode, phong_ks)


def _scene(scenes, name):
    if name == "heightfield":
        return scenes.heightfield(n=64, n_lights=2)  # 8 194 triangles, two shadow rays per hit
    return scenes.icosphere_soup(n_spheres=120, subdiv=1)  # 9 602 triangles


@pytest.fixture(scope="module")
def refs(oracle, scenes):
    """per scene: the scene, the oracle's tree (leaf size of every triangle record) and its frames of every size and shading.
    Computed once, never changed."""
    out = {}
    for name in SCENES:
        sc = _scene(scenes, name)
        cam = sc["camera"]
        O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
        frames = {}
        try:
            for (w, h) in SIZES:
                for mode, phong in SHADINGS:
                    oracle.set_phong(phong, 32)
                    frames[(w, h, mode, phong)] = O.render(cam["position"], cam["matrix"], mode, w, h)
        finally:
            oracle.set_phong(0, 32)
        ref4 = O.nodes4q()["ref"].reshape(-1)
        code = ~ref4[ref4 < 0].astype(np.int64) & 0xFFFFFFFF
        first, cnt = code >> 3, code & 7
        tris = O.tris()
        leaf_size = np.zeros(len(tris), dtype=np.uint32)
        for f, c in zip(first[cnt > 0], cnt[cnt > 0]):
            leaf_size[f:f + c] = c
        out[name] = {"scene": sc, "frames": frames, "leaf_sizes": sorted(set(int(c) for c in cnt if c > 0)), "leaf_size": leaf_size,
                     "tri_of": {(int(t["inst"]), int(t["prim"])): i for i, t in enumerate(tris)}}
        O.close()
    return out


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def test_scenes_mix_leaf_sizes_inside_a_packet(refs):
    """What the leaf-pair loop needs to be exercised: leaves with an odd and with an even number of triangles (a last trip with and
    without a second record), and an 8x8 packet whose lanes stand at leaves of different sizes, one of them odd and smaller than
    another -- then in the smaller leaf's last trip one lane has no second record (`two` false) while another has one.  From the
    oracle's tree and closest hits: the leaf a pixel's hit lies in is a leaf its ray tests."""
    sizes, mixed = set(), 0
    for name in SCENES:
        ref = refs[name]
        sizes |= set(ref["leaf_sizes"])
        w, h = SIZES[0]
        fr = ref["frames"][(w, h, 3, 0)]
        leaf = np.zeros((h, w), dtype=np.uint32)  # size of the leaf of the pixel's hit; 0 = miss
        for y, x in zip(*np.nonzero(fr["hit_inst"] != 0xFFFFFFFF)):
            leaf[y, x] = ref["leaf_size"][ref["tri_of"][(int(fr["hit_inst"][y, x]), int(fr["hit_prim"][y, x]))]]
        here = 0
        for y0 in range(0, h, 8):
            for x0 in range(0, w, 8):
                s = sorted(set(int(v) for v in leaf[y0:y0 + 8, x0:x0 + 8].reshape(-1)) - {0})
                here += any(a % 2 == 1 and a < s[-1] for a in s)
        print("%s: leaf sizes %s, packets with an odd leaf beside a larger one: %d" % (name, ref["leaf_sizes"], here))
        mixed += here
    assert any(s % 2 == 1 for s in sizes) and any(s % 2 == 0 for s in sizes), sorted(sizes)
    assert mixed > 0


def test_host_chooses_the_form_by_the_array_sizes(pkg):
    """crt::wideOffsets through crt_debug_wide_offsets: narrow while every record starts below 2^32 (64-byte nodes, 48-byte
    triangles), wide one record later, and wide whenever the option says so"""
    f = pkg.lib().crt_debug_wide_offsets
    assert "crt_debug_wide_offsets" in pkg.ABI_SYMBOLS
    assert f(1 << 26, 89478485, 0) == 0
    assert f((1 << 26) + 1, 89478485, 0) == 1
    assert f(1 << 26, 89478486, 0) == 1
    assert f((1 << 26) + 1, 89478486, 0) == 1
    assert f(0, 0, 0) == 0 and f(1, 1, 0) == 0
    assert f((1 << 28) - 1, (1 << 28) - 1, 0) == 1  # the builders' limit
    for n_nodes, n_tris in ((0, 0), (1, 1), (1 << 26, 89478485), ((1 << 26) + 1, 89478486)):
        assert f(n_nodes, n_tris, 1) == 1


def _check(got, ref, what, counting):
    for k in ("hit_inst", "hit_prim", "hit_t", "rgba8"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (what, k))
    assert np.array_equal(got["rgb"], ref["rgb"], equal_nan=True), "%s rgb" % what
    if counting:
        for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested"):
            assert got["stats"][k] == ref["stats"][k], "%s %s" % (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_frames_match_the_oracle_in_both_forms(pkg, oracle, refs, renderer, name, size):
    ref = refs[name]
    w, h = size
    sc = ref["scene"]
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"])
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
    try:
        for wide in (0, 1):
            renderer.set_option("wide_offsets", wide)
            for entries in (0, 1):
                renderer.set_option("stack_entries", entries)
                for mode, phong in SHADINGS:
                    renderer.change_shading_mode(mode)
                    renderer.set_option("phong_ks", phong)
                    for counting in (False, True):
                        renderer.set_counting(counting)
                        what = "%s %dx%d wide_offsets=%d stack_entries=%d mode %d phong %d counting=%d" % (name, w, h, wide, entries, mode, phong, counting)
                        _check(renderer.render_frame(w, h), ref["frames"][(w, h, mode, phong)], what, counting)
    finally:
        renderer.set_counting(False)
        for k, v in (("wide_offsets", 0), ("stack_entries", 0), ("phong_ks", 0)):
            renderer.set_option(k, v)
        renderer.change_shading_mode(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_two_rank_tile_share_matches_the_oracle_in_both_forms(pkg, refs, renderer, name):
    import torch
    ref = refs[name]
    w, h = SIZES[1]
    sc = ref["scene"]
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"])
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
    n = 2
    slots = pkg.tile_slots(w, h, n)
    try:
        renderer.change_shading_mode(100)
        for wide in (0, 1):
            renderer.set_option("wide_offsets", wide)
            gathered = torch.zeros(n * slots * 256, dtype=torch.int32, device="cuda")
            frame = torch.zeros(w * h, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for rank in range(n):
                renderer.render_tiles_device(w, h, rank, n, gathered.data_ptr() + rank * slots * 1024)
            renderer.untile_device(w, h, n, gathered.data_ptr(), frame.data_ptr())
            renderer.synchronize()
            np.testing.assert_array_equal(frame.cpu().numpy().view(np.uint32).reshape(h, w), ref["frames"][(w, h, 100, 0)]["rgba8"].view(np.uint32).reshape(h, w),
                                          err_msg="%s wide_offsets=%d" % (name, wide))
    finally:
        renderer.set_option("wide_offsets", 0)
        renderer.change_shading_mode(0)
