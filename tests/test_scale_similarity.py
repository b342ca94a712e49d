"""Every scene query at power-of-two scale (include/crt_hip.h, "scale").

Scene, records and incoming gradients are scaled by 2^k (tests/scale_similarity.py says what scales and by which exponent).
On the CPU each query's reference runs at k = -120 .. 120 in steps of 4 and at every k next to an end: the contiguous range
around 0 over which its outputs are those of k = 0 with the exponent shifted, bit for bit, is RANGES -- the figures of the
header and of DESIGN.md 5s -- and inside it no record is left out.  On the GPU, over the SAH, LBVH and PLOC trees of a dynamic
upload, every query equals its reference at scale k bit for bit at seven k per query -- 0, the middle of each half of the
range, the last k inside and the first k outside at each end, where intermediates are subnormal or overflow -- and inside the
range also its own k = 0 outputs, shifted."""
import numpy as np
import pytest

import grad_reference as G
import scale_similarity as ss
from test_gradients import refs as grefs  # noqa: F401  (the fixtures of the references)
from test_list_hits import ref as lref  # noqa: F401
from test_point_queries import TREES, ref as pref  # noqa: F401
from test_winding import wref  # noqa: F401

N = ss.N
# (first k, last k) of the similar range per query, measured by test_reference_ranges (-s prints them); DESIGN.md 5s
RANGES = {
    "trace_rays": (-34, 41), "occluded": (-43, 41), "count_hits": (-41, 41), "list_hits": (-34, 41),
    "closest_points": (-28, 30), "occupancy": (-45, 42),
    "winding_exact": (-118, 120),  # the ends of what the scene and the records can express, not of the arithmetic
    "winding_beta2": (-57, 58), "winding_beta8": (-58, 58),
    "trace_rays_backward": (-34, 41), "closest_points_backward": (-28, 30),
}
# exact mode must be similar at least here (the issue's figure for the open icosphere)
WINDING_EXACT_AT_LEAST = (-90, 90)


@pytest.fixture(scope="module")
def harness(pkg, oracle, scenes, pref, lref, wref, grefs):
    return ss.Harness(pkg, oracle, scenes, pref, lref, wref, grefs["f32"])


# ---- CPU

@pytest.mark.parametrize("query", ss.QUERIES)
def test_reference_ranges(harness, query):
    lo, hi, left_out, holes = ss.similar_range(harness, query)
    print("%-24s similar for k in [%d, %d], %d records left out inside" % (query, lo, hi, left_out))
    assert left_out == 0, "inside the range every record takes part"
    assert not holes, "not similar at k = %r inside the range" % holes
    assert (lo, hi) == RANGES[query]
    if query == "winding_exact":
        assert lo <= WINDING_EXACT_AT_LEAST[0] and hi >= WINDING_EXACT_AT_LEAST[1]


def test_host_builder_range(harness):
    """an observation, not a contract: the range of k over which the host SAH builder gives the wide tree of k = 0"""
    ref0 = harness.host_tree(0)[0]["ref"]
    same = [k for k in range(-120, 121) if np.array_equal(harness.host_tree(k)[0]["ref"], ref0)]
    lo = max(k for k in range(-120, 1) if k not in same) + 1 if any(k not in same for k in range(-120, 1)) else -120
    hi = min(k for k in range(0, 121) if k not in same) - 1 if any(k not in same for k in range(0, 121)) else 120
    print("host SAH builder: the child references of k = 0 for k in [%d, %d]" % (lo, hi))
    assert lo < 0 < hi


# ---- GPU

FAMILIES = {"rays": ("trace_rays", "occluded", "count_hits", "list_hits"), "points": ("closest_points", "occupancy"),
            "winding": ("winding_exact", "winding_beta2", "winding_beta8"), "gradients": ("trace_rays_backward", "closest_points_backward")}
TREE_DEPENDENT = ("trace_rays", "occluded", "winding_beta2", "winding_beta8")  # their references walk the exported tree
FLT_MAX = float(np.finfo(np.float32).max)


def scales(query):
    """0, the middle of each half of the range, the last k inside and the first k outside at each end"""
    lo, hi = RANGES[query]
    return (0, lo // 2, hi // 2, lo, hi, lo - 1, hi + 1)


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def trees(renderer):
    yield
    for k, v in (("gpu_build", 0), ("gpu_builder", 0)):
        renderer.set_option(k, v)


def _check_vertex_sums(got, scene, inst, prim, ref, what):
    """grad_xyz against the exact sum S of the reference's float32 contributions: |got - S| <= 2^-24 |S| + m 2^-52 A
    (tests/grad_reference.py) plus 2^-150, half the spacing of the subnormals a small sum is rounded into; components whose sum
    float32 cannot hold are not judged"""
    S, A, m = G.vertex_sums(scene, inst, prim, ref["contrib"].reshape(-1, 3, 3), ref["live"].astype(bool))
    got = np.asarray(got, np.float32).reshape(-1, 3)
    assert got.shape == S.shape, what
    bound = 2.0 ** -24 * np.abs(S) + m * 2.0 ** -52 * A + 2.0 ** -150
    judged = np.abs(S) + bound < FLT_MAX
    err = np.abs(got.astype(np.float64) - S)
    assert np.all(err[judged] <= bound[judged]), "%s: grad_xyz leaves the bound at %d components" % (what, int((err[judged] > bound[judged]).sum()))
    assert np.all(got.view(np.uint32)[m == 0] == 0), what + ": a vertex no live record touches is +0.0"


def _run(h, r, query, k):
    """the query on the GPU at scale k, in the layout of the reference's outputs (and grad_xyz beside the gradients)"""
    if query == "trace_rays":
        return r.trace_rays(h.rays(k))
    if query == "occluded":
        return {"occluded": r.occluded(h.rays(k)).astype(np.uint8)}
    if query == "count_hits":
        return {"count": r.count_hits(h.rays(k))}
    if query == "list_hits":
        return r.list_hits(h.rays(k))
    if query == "closest_points":
        return r.closest_points(h.points(k))
    if query == "occupancy":
        return {"inside": r.occupancy(h.points(k)).astype(np.uint8)}
    if query.startswith("winding"):
        return {"w": r.winding_numbers(h.points(k), 0.0 if query == "winding_exact" else float(query.split("_beta")[1]))}
    g = h.incoming(k)
    if query == "trace_rays_backward":
        hit = h.reference("trace_rays", k)
        out = r.trace_rays_backward(h.rays(k), hit["inst"], hit["prim"], hit["t"], hit["uv"], g["g_t"], g["g_uv"])
        return {"grad_o": out["grad_rays"][:, 0:4], "grad_d": out["grad_rays"][:, 4:8], "grad_xyz": out["grad_xyz"], "hit": hit}
    hit = h.reference("closest_points", k)
    out = r.closest_points_backward(h.points(k), hit["inst"], hit["prim"], hit["uv"], g["g_dist"])
    return {"grad_p": out["grad_points"], "grad_xyz": out["grad_xyz"], "hit": hit}


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_gpu_equals_the_reference_at_every_scale(harness, renderer, trees, family, tree):
    h = harness
    at_zero = {}
    for k in sorted({k for q in FAMILIES[family] for k in scales(q)}, key=abs):
        todo = [q for q in FAMILIES[family] if k in scales(q)]
        for name, v in TREES[tree].items():
            renderer.set_option(name, v)
        renderer.upload(h.meshes(k), [], [{"albedo": (1, 1, 1), "type": 1}], dynamic=True)
        exported = tuple(renderer.bvh_export()) + (renderer.bvh_export4q(),)
        if k == 0:
            tree_at_zero = exported[3]["ref"]
        same_tree = np.array_equal(exported[3]["ref"], tree_at_zero)
        if family == "winding":  # the moment table of k = 0 shifted: {p~, r} by k, N~ (an area) by 2 k, nothing rounded
            table = renderer.winding_moments()
            if k == 0:
                table_at_zero = table
            same_table = same_tree and bool((ss._exact(table_at_zero[:, :16], k).all() and ss._exact(table_at_zero[:, 16:], 2 * k).all()
                                             and ss.same_floats(table[:, :16], np.ldexp(table_at_zero[:, :16], k)).all()
                                             and ss.same_floats(table[:, 16:], np.ldexp(table_at_zero[:, 16:], 2 * k)).all()))
        for q in todo:
            what = "%s %s 2^%d" % (q, tree, k)
            got = _run(h, renderer, q, k)
            ref = h.reference(q, k, exported if q in TREE_DEPENDENT else None)
            bad = h.equal(got, {name: v for name, v in ref.items() if name in got})
            assert not bad, "%s: the GPU differs from the reference in %s" % (what, ", ".join(bad))
            if "grad_xyz" in got:
                _check_vertex_sums(got["grad_xyz"], h.scene_arrays(k), got["hit"]["inst"], got["hit"]["prim"], ref, what)
            if k == 0:
                at_zero[q] = got
            elif RANGES[q][0] <= k <= RANGES[q][1]:
                if q in ("winding_beta2", "winding_beta8"):
                    # other clusters, another w: the ranges are those of the host builder's tree.  A GPU builder forms other
                    # clusters, whose N~ may leave the normal floats sooner, or another tree altogether; then the table is
                    # not the table of k = 0 and only the reference at k is held to
                    assert same_tree or tree != "sah", what + ": the host builder's tree changed inside the range"
                    if tree != "sah" and not same_table:
                        continue
                base = {name: at_zero[q][name] for name in h.reference(q, 0) if name in got}
                ok, left_out = h.similar(q, got, k, base)
                assert ok and left_out == 0, "%s: not the GPU's own k = 0 outputs shifted (%d records left out)" % (what, left_out)
