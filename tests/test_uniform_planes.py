"""The decoded plane table (render_kernels.h kPlaneStride, crt_bvh_export_planes4q) and the node steps that read it.

When every active lane of a wavefront stands on one node, the render kernel fetches the record through the scalar cache and,
for wavefronts whose rays share a direction octant, takes the 24 plane offsets from the table as floats instead of converting
the record's bytes per lane.  The table is built on the device from the uploaded nodes at every upload, for the host SAH tree
and the GPU-built LBVH alike.  These tests pin the table byte for byte and compare frames, hit ids, t and fetch counters with
the CPU oracle on scenes and cameras chosen so that packets take the scalar path in every octant and in mixed octants."""
import numpy as np
import pytest

GPU = pytest.mark.gpu


def _decoded(nodes4q):
    """float(q) of the 24 plane bytes of every record, then 8 zeros: the table's spec"""
    raw = np.frombuffer(nodes4q.tobytes(), dtype=np.uint8).reshape(-1, 64)
    out = np.zeros((len(nodes4q), 32), dtype=np.float32)
    out[:, :24] = raw[:, 24:48].astype(np.float32)
    return out


def _shell_scene(n, seed):
    """n small random triangles all around the origin (where the camera stands) and one light: rays in every direction hit
    something, shadow rays leave in all directions"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-6.0, 6.0, size=(n, 1, 3))
    c[np.linalg.norm(c[:, 0], axis=1) < 1.5] *= 3.0  # keep the camera's surroundings clear
    v = (c + rng.uniform(-0.6, 0.6, size=(n, 3, 3))).reshape(-1, 3).astype(np.float32)
    t = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)
    meshes = [{"vertices": v, "triangles": t, "material_index": 0}]
    return meshes, [((0.5, 7.0, 0.3), 900.0)], [{"albedo": (0.7, 0.6, 0.5), "type": 1}]


# the eight view directions along the diagonals: the central packets of a frame share the octant of their view direction,
# the packets near the frame's edges cross one or two axis planes (mixed-octant steps)
_VIEWS = [(yaw, pitch) for yaw in (45.0, 135.0, 225.0, 315.0) for pitch in (35.0, -35.0)]


def _packet_octants(scenes, yaw, pitch, w, h):
    """the direction octants of each 8x8 packet's rays (float64 restatement of rayDir, away from the axis planes only)"""
    rot = scenes.camera_matrix(yaw, pitch).astype(np.float64).reshape(3, 3)
    px, py = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    x = (2.0 * px / w - 1.0) * (w / h)
    y = 1.0 - 2.0 * py / h
    d = np.stack([x, y, -np.ones_like(x)], axis=-1) @ rot.T
    octs = set()
    single = set()
    for by in range(0, h, 8):
        for bx in range(0, w, 8):
            p = d[by:by + 8, bx:bx + 8].reshape(-1, 3)
            o = set(((p[:, 0] < 0) * 1 + (p[:, 1] < 0) * 2 + (p[:, 2] < 0) * 4).tolist())
            if len(o) == 1:
                single |= o
            else:
                octs.add(8)
    return single, octs


def test_plane_table_entry_point_rejects_missing_state(pkg):
    assert pkg.lib().crt_bvh_export_planes4q(None, None) == 5  # CRT_ESTATE


def test_diagonal_views_cover_every_octant_and_mixed_packets(scenes):
    """the camera set of the GPU tests below: uniform-octant packets in all eight octants, mixed packets in every view"""
    seen = set()
    for yaw, pitch in _VIEWS:
        single, mixed = _packet_octants(scenes, yaw, pitch, 96, 96)
        assert mixed == {8}
        seen |= single
    assert seen == set(range(8))


@GPU
@pytest.mark.parametrize("gpu_build", [0, 1])
def test_plane_table_is_the_decoded_planes_of_every_node(pkg, oracle, scenes, dragon, gpu_build):
    """float(q) for every plane byte of every node, for the SAH tree and the LBVH, rebuilt by every upload (a larger and a
    smaller tree after each other on one context)"""
    r = pkg.Renderer(0)
    try:
        r.set_option("gpu_build", gpu_build)
        for sc in (scenes.cornell_box(), dragon, scenes.displaced_sphere(), scenes.single_triangle()):
            r.upload(sc["meshes"], sc["lights"], sc["materials"])
            q = r.bvh_export4q()
            O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], build_mode=gpu_build)
            assert q.tobytes() == O.nodes4q().tobytes()
            p = r.bvh_export_planes4q()
            assert p.shape == (len(q), 32)
            assert p.tobytes() == _decoded(q).tobytes()
    finally:
        r.close()


@GPU
@pytest.mark.parametrize("gpu_build", [0, 1])
def test_scalar_path_steps_match_the_oracle_in_every_octant(pkg, oracle, scenes, gpu_build):
    """frames over a scene surrounding the camera, looking down each of the eight diagonals: every packet starts with a
    uniform descent from the root, in its own octant or (near the frame's edges) a mixed one; mode 3 (primary rays) and
    mode 100 (plus shadow rays), instrumented and plain kernels, against the oracle over the same tree"""
    meshes, lights, mats = _shell_scene(3000, 11)
    r = pkg.Renderer(0)
    try:
        r.set_option("gpu_build", gpu_build)
        r.upload(meshes, lights, mats)
        O = oracle.OracleScene(meshes, lights, mats, build_mode=gpu_build)
        assert r.bvh_export4q().tobytes() == O.nodes4q().tobytes()
        pos = np.float32([0.0, 0.0, 0.0])
        w = h = 96
        for yaw, pitch in _VIEWS:
            rot = scenes.camera_matrix(yaw, pitch)
            r.set_camera(pos, rot)
            for mode in (3, 100):
                r.change_shading_mode(mode)
                ref = O.render(pos, rot, mode, w, h)
                assert (ref["hit_inst"] != 0xFFFFFFFF).mean() > 0.5, "the view should mostly hit"
                for counting in (True, False):
                    r.set_counting(counting)
                    got = r.render_frame(w, h)
                    for k in ("hit_inst", "hit_prim", "hit_t", "rgba8"):
                        np.testing.assert_array_equal(got[k], ref[k], err_msg="view %s mode %d %s" % ((yaw, pitch), mode, k))
                    assert np.array_equal(got["rgb"], ref["rgb"], equal_nan=True)
                    if counting:
                        st, rs = got["stats"], ref["stats"]
                        assert (st["rays_shadow"], st["nodes_visited"], st["tris_tested"]) == \
                               (rs["rays_shadow"], rs["nodes_visited"], rs["tris_tested"]), (yaw, pitch, mode)
                r.set_counting(False)
    finally:
        r.close()


@GPU
def test_single_packet_frames(pkg, oracle, scenes):
    """an 8x8 frame = one packet = one wavefront: the scalar-path descent from the root and the steps that follow, with
    nothing else in flight.  Its rays span the whole field of view, so most of these packets take the mixed-octant form."""
    meshes, lights, mats = _shell_scene(1500, 23)
    r = pkg.Renderer(0)
    try:
        r.upload(meshes, lights, mats)
        O = oracle.OracleScene(meshes, lights, mats)
        pos = np.float32([0.0, 0.0, 0.0])
        for yaw, pitch in _VIEWS:
            rot = scenes.camera_matrix(yaw, pitch)
            r.set_camera(pos, rot)
            for mode in (3, 100):
                r.change_shading_mode(mode)
                r.set_counting(True)
                got = r.render_frame(8, 8)
                r.set_counting(False)
                ref = O.render(pos, rot, mode, 8, 8)
                for k in ("hit_inst", "hit_prim", "hit_t", "rgba8"):
                    np.testing.assert_array_equal(got[k], ref[k], err_msg="view %s mode %d %s" % ((yaw, pitch), mode, k))
                st, rs = got["stats"], ref["stats"]
                assert (st["rays_shadow"], st["nodes_visited"], st["tris_tested"]) == (rs["rays_shadow"], rs["nodes_visited"], rs["tris_tested"])
    finally:
        r.close()
