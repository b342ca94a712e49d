"""Frames through the triangle test's short reciprocal (traversal.hip.h rcpExact) and its division fallback.

The render kernel's closest-hit leaf tests take 1 / det from v_rcp_f32 and a Newton step; a wavefront with any lane whose
det lies outside the range where that is exact takes the division instead.  Frames over a dense scene surrounding the
camera, one view down each of the eight diagonals (every octant-specialised loop and the mixed-octant one), must equal the
oracle's: hit ids, t, colours and fetch counters, with counting on and off.  A second scene mixes in triangles so small
that the Moeller-Trumbore determinant is denormal or zero, so that wavefronts take the fallback."""
import numpy as np
import pytest

GPU = pytest.mark.gpu
_VIEWS = [(yaw, pitch) for yaw in (45.0, 135.0, 225.0, 315.0) for pitch in (35.0, -35.0)]


def _shell(n, seed, tiny=0.0):
    """n random triangles around the origin (the camera) and one light; a fraction `tiny` of them shrunk to 1e-20 of
    their size around their centre"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-8.0, 8.0, size=(n, 1, 3))
    c[np.linalg.norm(c[:, 0], axis=1) < 2.0] *= 3.0
    off = rng.uniform(-0.4, 0.4, size=(n, 3, 3))
    small = rng.random(n) < tiny
    off[small] *= 1e-20
    v = (c + off).reshape(-1, 3).astype(np.float32)
    t = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)
    meshes = [{"vertices": v, "triangles": t, "material_index": 0}]
    return meshes, [((0.5, 9.0, 0.3), 1500.0)], [{"albedo": (0.7, 0.6, 0.5), "type": 1}]


def _compare(pkg, oracle, scenes, meshes, lights, mats, w, h, gpu_build=0):
    r = pkg.Renderer(0)
    try:
        r.set_option("gpu_build", gpu_build)
        r.upload(meshes, lights, mats)
        O = oracle.OracleScene(meshes, lights, mats, build_mode=gpu_build)
        pos = np.float32([0.0, 0.0, 0.0])
        for yaw, pitch in _VIEWS:
            rot = scenes.camera_matrix(yaw, pitch)
            r.set_camera(pos, rot)
            for mode in (3, 100):
                r.change_shading_mode(mode)
                ref = O.render(pos, rot, mode, w, h)
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
@pytest.mark.parametrize("gpu_build", [0, 1])
def test_frames_match_the_oracle_in_every_octant(pkg, oracle, scenes, gpu_build):
    meshes, lights, mats = _shell(20000, 5)
    _compare(pkg, oracle, scenes, meshes, lights, mats, 160, 160, gpu_build)


@GPU
def test_degenerate_triangles_match_the_oracle(pkg, oracle, scenes):
    meshes, lights, mats = _shell(6000, 9, tiny=0.3)
    _compare(pkg, oracle, scenes, meshes, lights, mats, 96, 96)
