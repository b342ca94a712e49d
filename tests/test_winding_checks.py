"""The inputs and checks of tests/winding_checks.py can see what the GPU tests claim (CPU only).  Over the expected tree of every
builder: the reference walks inert records to exactly nothing, its moment table holds against the float64 statement, the points
would show an inert triangle that was counted, the chains put the exact-mode walk past the LDS part of the stack, and the
reference stays within its error budget of float64 on every scene the GPU tests use.  assert_winding, fed the reference's own
output as "device output" by a stand-in, passes, and fails on each of five mutations.  Nothing on the GPU is broken on purpose.

Measured here (-s prints them).  Deepest stack of the exact-mode walk (exact_walk_depth), depth4 and the host's bound 3 * depth4 + 1:
    chain A             sah  36 (depth4 12, bound 37)    lbvh 50 (depth4 20, bound 61)    ploc 28 (depth4 11, bound 34)
    plate and chain B   sah  27 (depth4  9, bound 28)    lbvh 57 (depth4 19, bound 58)    ploc 30 (depth4 10, bound 31)
Largest |w - w_f64| per scene, the largest of its three trees (points_for's points no nearer to a finite triangle than 1 % of
the scene's size; the chains' 191 points and the spheres' 257 shell points as they are):
    scene                          exact     beta 1    beta 2    beta 4    beta 8
    probe100 (every kind)          8.4e-10   5.9e-3    6.3e-4    1.4e-4    1.9e-5
    probe2000                      9.1e-9    1.6e-2    2.1e-3    5.5e-4    1.5e-4
    cornell_first_last             1.8e-7    1.2e-1    1.4e-2    3.4e-4    1.8e-7
    cornell_whole_mesh             2.7e-7    1.3e-1    1.5e-2    1.9e-4    2.7e-7
    dragon_shared_vertex           2.6e-7    6.8e-2    2.2e-2    6.2e-3    1.5e-3
    heightfield_leaf               2.5e-7    1.6e-1    2.4e-2    7.0e-3    7.4e-4
    icosphere_pole                 7.2e-8    1.9e-1    2.3e-2    5.0e-3    7.1e-4
    finite_beside_inert            3.0e-8    1.1e-1    2.3e-2    2.5e-3    1.0e-4
    normals_and_uvs                2.5e-7    1.3e-1    1.7e-2    5.2e-4    2.5e-7
    tiny1 .. tiny5 (poisoned)      1.2e-7    2.1e-2    7.2e-4    2.1e-5    1.2e-7
    all_inert                      0         0         0         0         0
    chain A                        2.3e-6    6.8e-2    2.2e-3    2.0e-4    1.1e-5
    plate and chain B              1.0e-6    3.5e-2    1.5e-3    1.0e-4    8.0e-6
    sphere at 0 .. 131072          1.2e-7    1.5e-1    2.6e-2    4.0e-3    1.3e-4
    open sphere at 0 .. 131072     1.1e-7    1.4e-1    2.2e-2    3.6e-3    1.0e-4
The worst ratio of the exact mode's error to its budget n_tris * ATAN_BUDGET / (2 pi) is 0.39 (tiny2, two triangles); chain A is
at 0.06 and the shifted spheres at 0.003.  No ceiling is asserted for beta > 0: only that the error does not grow with beta,
except below the exact mode's budget.  """
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deep_stack_scenes as D  # noqa: E402
import test_deep_stacks as ds  # noqa: E402
import test_nonfinite_vertices as nf  # noqa: E402
import test_winding as tw  # noqa: E402
import winding_checks as wc  # noqa: E402
from test_nonfinite_vertices import case  # noqa: E402,F401  (fixture: the poisoned scenes)
from winding_checks import wref  # noqa: E402,F401  (fixture: tests/winding_reference.c)

TREES = ("sah", "lbvh", "ploc")
CASES = sorted(set(nf._GPU_PARAMS) | set(nf._DYNAMIC))
GROWTH_BETAS = (1.0, 2.0, 4.0, 8.0)
TWO_PI = 2.0 * math.pi


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clear_of_the_surface(records, pts):
    """the points no nearer to a finite triangle than 1 % of the size of the finite triangles' box: where tests/test_winding.py
    measures the reference against float64 (nearer to an edge the angle itself is ill conditioned in float32)"""
    alive = records[wc.finite_records(records)]
    if not len(alive):
        return pts
    v0, e1, e2 = (alive[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    corners = np.concatenate([v0, v0 + e1, v0 + e2])
    size = float(np.linalg.norm(corners.max(axis=0) - corners.min(axis=0)))
    keep = np.array([tw._min_distance(alive, p.astype(np.float64)) >= 0.01 * size for p in pts[:, 0:3]])
    assert keep.mean() >= 0.8, "too few points are clear of the surface"
    return np.ascontiguousarray(pts[keep])


def poisoned_tree(pkg, oracle, sc, tree):
    """(nodes4q, tris) a fresh upload of the poisoned scene over `tree` must export (test_nonfinite_vertices._expected_tree)"""
    nodes, tris, shade, O = nf._expected_tree(pkg, oracle, sc, tree)
    if O is None:
        O = nf._oracle_scene(oracle, sc)
        O.set_bvh(nodes, tris, shade)
    return O.nodes4q().copy(), np.ascontiguousarray(O.tris()).copy()


def chain_tree(pkg, oracle, sc, builder):
    O = ds.oracle_tree(pkg, oracle, sc, builder)
    try:
        return O.nodes4q().copy(), np.ascontiguousarray(O.tris()).copy(), O.depth4
    finally:
        O.close()


def reference_against_float64(wref, name, tree, nodes4q, tris, records, pts):
    """what test_winding.test_reference_exact_matches_float64 and test_reference_tree_matches_float64 assert, on pts (clear of
    the surface, no NaN): exact mode within n_tris * ATAN_BUDGET / (2 pi) of float64, the error at beta 1, 2, 4, 8 not growing except below that floor, and beta inf, 0, -1, NaN the exact bits"""
    alive = np.ascontiguousarray(records[wc.finite_records(records)])
    floor = len(records) * tw.ATAN_BUDGET / TWO_PI
    f64 = tw.winding_f64(alive, pts)
    exact = tw.ref_exact(wref, alive, pts)
    err0 = float(np.abs(exact.astype(np.float64) - f64).max())
    moments = tw.ref_moments(wref, nodes4q, tris)
    errs = []
    for beta in GROWTH_BETAS:
        w = tw.ref_tree(wref, nodes4q, tris, moments, beta, pts)
        assert np.isfinite(w).all(), (name, tree, beta)
        errs.append(float(np.abs(w.astype(np.float64) - f64).max()))
    print("%-28s %-4s max |w - f64|: exact %.2e (bound %.2e)  beta 1, 2, 4, 8: %s" % (name, tree, err0, floor, " ".join("%.2e" % e for e in errs)))
    assert err0 <= floor, "%s %s: exact mode is %.3e from float64, the budget is %.3e" % (name, tree, err0, floor)
    for lo, hi in zip(errs[1:], errs[:-1]):
        assert lo <= max(hi, floor), "%s %s: the error grows with beta: %r" % (name, tree, errs)
    for beta in (float("inf"), 0.0, -1.0, float("nan")):
        w = tw.ref_tree(wref, nodes4q, tris, moments, beta, pts)
        np.testing.assert_array_equal(_bits(w), _bits(exact), err_msg="%s %s beta %r" % (name, tree, beta))


# ---- the poisoned scenes

@pytest.mark.parametrize("name,kind", CASES, ids=["%s-%s" % p for p in CASES])
def test_reference_ignores_inert_records_and_the_points_would_show_one(pkg, oracle, wref, case, name, kind):
    sc = case(name, kind)
    pts = wc.points_for(sc, seed=len(name))
    assert len(pts) <= wc.MAX_POINTS and np.isnan(pts[:, 0:3]).any(axis=1).sum() == 1
    poisoned, clean = nf._records(pkg, sc["meshes"]), nf._records(pkg, sc["clean"])
    alive = wc.finite_records(poisoned)
    assert not alive.all() and wc.finite_records(clean).all()
    finite_only = tw.ref_exact(wref, np.ascontiguousarray(poisoned[alive]), pts)
    np.testing.assert_array_equal(_bits(tw.ref_exact(wref, poisoned, pts)), _bits(finite_only), err_msg="brute force over the NaN records")
    if not alive.any():
        assert not _bits(finite_only).any(), "nothing winds around a point of a scene without a finite triangle"
    # an inert triangle that was counted shows on some point
    counted = tw.ref_exact(wref, clean, pts)
    assert (_bits(counted) != _bits(finite_only)).any(), "%s %s: no point sees the inert triangles" % (name, kind)
    smooth = clear_of_the_surface(poisoned, pts[:-wc.N_SPECIAL])
    for tree in TREES:
        what = "%s %s %s" % (name, kind, tree)
        nodes4q, tris = poisoned_tree(pkg, oracle, sc, tree)
        assert np.array_equal(wc.finite_records(tris), alive[tris["gid"].astype(np.int64)]), what
        moments = tw.ref_moments(wref, nodes4q, tris)
        wc.assert_moments(wref, nodes4q, tris, moments, what)
        for beta in (0.0, -1.0, float("inf")):
            np.testing.assert_array_equal(_bits(tw.ref_tree(wref, nodes4q, tris, moments, beta, pts)), _bits(finite_only),
                                          err_msg="%s: the walk over the NaN records, beta %r" % (what, beta))
        reference_against_float64(wref, "%s-%s" % (name, kind), tree, nodes4q, tris, poisoned, smooth)


# ---- the stand-in: the reference's own output as "device output"

class ReferenceDevice:
    """what assert_winding asks of a renderer, answered by tests/winding_reference.c over a given tree; `walked` are the records
    the walk really reads (a faulty device may read others than it exports), `spoil` edits an answer before it is returned"""
    host_pointers = True

    def __init__(self, wref, nodes4q, tris, walked=None, spoil=None):
        self.wref, self.nodes4q, self.tris = wref, nodes4q, tris
        self.walked = tris if walked is None else walked
        self.spoil = spoil or (lambda kind, value: value)
        self.counting = False

    def bvh_export4q(self):
        return self.nodes4q.copy()

    def bvh_export(self):
        return None, self.tris.copy(), None

    def set_counting(self, on):
        self.counting = bool(on)

    def winding_moments(self):
        return self.spoil("moments", tw.ref_moments(self.wref, self.nodes4q, self.tris))

    def winding_numbers(self, pts, beta=2.0):
        moments = tw.ref_moments(self.wref, self.nodes4q, self.tris)
        return self.spoil("w", tw.ref_tree(self.wref, self.nodes4q, self.walked, moments, beta, pts))

    def winding_numbers_device(self, n, d_points, d_w, beta=2.0, stats=False):
        import ctypes as C
        pts = np.frombuffer((C.c_float * (4 * n)).from_address(d_points), dtype=np.float32).reshape(n, 4)
        np.frombuffer((C.c_float * n).from_address(d_w), dtype=np.float32)[:] = self.winding_numbers(pts, beta)
        st = {"rays_primary": n, "nodes_visited": 0, "tris_tested": 0}
        if self.counting and not 0.0 < beta < float("inf"):  # (the stand-in has no counters for the approximating walk)
            inner, fetched = wc.exact_walk_counts(self.nodes4q)
            m = int((~np.isnan(pts[:, 0:3]).any(axis=1)).sum())
            st.update(nodes_visited=m * inner, tris_tested=m * fetched)
        elif self.counting:
            st.update(nodes_visited=1, tris_tested=1)
        return self.spoil("stats", st) if stats else None


@pytest.fixture(scope="module")
def standin(pkg, oracle, wref, case):
    sc = case("cornell_first_last", "nan")
    nodes4q, tris = poisoned_tree(pkg, oracle, sc, "sah")
    return {"scene": sc, "nodes4q": nodes4q, "tris": tris, "records": nf._records(pkg, sc["meshes"]), "clean": nf._records(pkg, sc["clean"]),
            "points": wc.points_for(sc, seed=3)}


def _run(pkg, wref, s, **kw):
    r = ReferenceDevice(wref, s["nodes4q"], s["tris"], **kw)
    return wc.assert_winding(pkg, wref, r, s["scene"], s["records"], s["points"], "stand-in")


def test_assert_winding_passes_on_the_reference(pkg, wref, standin):
    out = _run(pkg, wref, standin)
    assert set(out["w"]) == set(wc.EXACT_BETAS + wc.TREE_BETAS) and set(out["counters"]) == set(out["w"])
    inner, fetched = wc.exact_walk_counts(standin["nodes4q"])
    assert inner > 1 and fetched == len(standin["tris"])
    assert (~wc.finite_records(standin["records"])).sum() >= 1


def _first_inner_slot(nodes4q, tris):
    """(node, slot) of a reachable non-root node's slot with a finite triangle below it"""
    f64 = wc.moments_f64(nodes4q, tris)
    for i in f64["reachable"][1:]:
        for k in range(4):
            if f64["n"][i, k]:
                return i, k
    raise AssertionError("the stand-in's tree has one node")


def test_assert_winding_fails_when_a_moment_line_is_zeroed(pkg, wref, standin):
    node, _ = _first_inner_slot(standin["nodes4q"], standin["tris"])

    def spoil(kind, v):
        if kind == "moments":
            v[node] = 0.0
        return v
    with pytest.raises(AssertionError, match="all zeros.*stopped short"):
        _run(pkg, wref, standin, spoil=spoil)


def test_assert_winding_fails_when_a_moment_moves_by_one_ulp(pkg, wref, standin):
    node, slot = _first_inner_slot(standin["nodes4q"], standin["tris"])

    def spoil(kind, v):
        if kind == "moments":
            word = 16 + 4 * slot + int(np.argmax(np.abs(v[node, 16 + 4 * slot:19 + 4 * slot])))
            v[node].view(np.uint32)[word] += 1
        return v
    with pytest.raises(AssertionError, match="differ from the reference"):
        _run(pkg, wref, standin, spoil=spoil)


def test_the_float64_table_fails_a_rule_both_sides_carry(pkg, wref, standin):
    """a table that counts the inert triangle (the reference's arithmetic over the clean records in leaf order) is what a rule
    wrong on both sides would export: bit-equal to a reference with the same flaw, and caught by moments_f64 alone"""
    nodes4q, tris = standin["nodes4q"], standin["tris"]
    wc.check_moments_f64(tw.ref_moments(wref, nodes4q, tris), nodes4q, tris, "as exported")
    counted = np.ascontiguousarray(standin["clean"][tris["gid"].astype(np.int64)])
    with pytest.raises(AssertionError, match="float64 gives"):
        wc.check_moments_f64(tw.ref_moments(wref, nodes4q, counted), nodes4q, tris, "inert counted")
    twice = tw.ref_moments(wref, nodes4q, tris)
    twice[0, 16:32] *= np.float32(2.0)
    with pytest.raises(AssertionError, match="float64 gives"):
        wc.check_moments_f64(twice, nodes4q, tris, "counted twice")
    short = tw.ref_moments(wref, nodes4q, tris)
    short[0, 3:16:4] *= np.float32(0.5)
    with pytest.raises(AssertionError, match="a vertex below it"):
        wc.check_moments_f64(short, nodes4q, tris, "r halved")


def test_assert_winding_fails_when_an_inert_triangle_is_counted(pkg, wref, standin):
    tris = standin["tris"]
    dead = np.flatnonzero(~wc.finite_records(tris))
    walked = tris.copy()
    walked[dead[0]] = standin["clean"][int(tris["gid"][dead[0]])]
    with pytest.raises(AssertionError, match="exact mode against brute force without the inert records"):
        _run(pkg, wref, standin, walked=walked)


def test_assert_winding_fails_when_a_winding_number_moves_by_one_ulp(pkg, wref, standin):
    for when in (0, 3):  # an exact-mode answer of the host form; a beta = 2 answer
        calls = []

        def spoil(kind, v):
            if kind == "w":
                calls.append(1)
                if len(calls) == when + 1:
                    v.view(np.uint32)[int(np.argmax(np.abs(v)))] += 1
            return v
        with pytest.raises(AssertionError, match="differ, first point"):
            _run(pkg, wref, standin, spoil=spoil)
    calls = []

    def late(kind, v):  # the device form alone
        if kind == "w":
            calls.append(1)
            if len(calls) == len(wc.EXACT_BETAS + wc.TREE_BETAS) + 1:
                v.view(np.uint32)[int(np.argmax(np.abs(v)))] += 1
        return v
    with pytest.raises(AssertionError, match="the device form"):
        _run(pkg, wref, standin, spoil=late)


def test_assert_winding_fails_when_the_counters_are_off_by_one(pkg, wref, standin):
    for key in ("nodes_visited", "tris_tested"):
        def spoil(kind, v):
            if kind == "stats" and v[key]:
                v = dict(v, **{key: v[key] + 1})
            return v
        with pytest.raises(AssertionError, match="fetched"):
            _run(pkg, wref, standin, spoil=spoil)

    def loud(kind, v):  # counters that run without counting
        return dict(v, nodes_visited=v["nodes_visited"] or 1) if kind == "stats" else v
    with pytest.raises(AssertionError, match="without counting"):
        _run(pkg, wref, standin, spoil=loud)


# ---- the chains: the exact-mode walk leaves the LDS part

def test_exact_mode_walks_leave_the_lds_part(pkg, oracle, wref):
    deepest = {}
    for name, sc in (("chain A", D.chain_a()), ("plate and chain B", D.plate_and_chain_b())):
        pts = ds.winding_points(pkg, sc, seed=9)
        records = ds.tp._tri_records(pkg, sc["meshes"])
        for b in ds.BUILDERS:
            nodes4q, tris, depth4 = chain_tree(pkg, oracle, sc, b)
            d = wc.exact_walk_depth(nodes4q)
            inner, fetched = wc.exact_walk_counts(nodes4q)
            print("%s, %s: depth4 %d, bound %d, the exact-mode walk holds %d entries; %d inner nodes, %d records" % (
                name, b, depth4, 3 * depth4 + 1, d, inner, fetched))
            assert d > ds.LDS_DEFAULT, (name, b, d)
            assert d <= 3 * depth4 + 1, (name, b, d, depth4)
            assert fetched == len(tris) == len(records)
            deepest[(name, b)] = d
            wc.assert_moments(wref, nodes4q, tris, tw.ref_moments(wref, nodes4q, tris), "%s %s" % (name, b))
            reference_against_float64(wref, name, b, nodes4q, tris, records, pts[:-1])
    assert deepest[("chain A", "lbvh")] > ds.LDS_MOST


# ---- far from the origin

@pytest.mark.parametrize("off", tw.FAR_OFFSETS)
def test_reference_holds_far_from_the_origin(pkg, oracle, scenes, wref, off):
    for kind in tw.FAR_SCENES:
        sc, pts, _ = tw.far_case(scenes, kind, off)
        records = ds.tp._tri_records(pkg, sc["meshes"])
        for b in TREES:
            nodes4q, tris, _ = chain_tree(pkg, oracle, sc, b)
            wc.assert_moments(wref, nodes4q, tris, tw.ref_moments(wref, nodes4q, tris), "%s at %g, %s" % (kind, off, b))
            reference_against_float64(wref, "%s at %g" % (kind, off), b, nodes4q, tris, records, pts)


def test_tiny_scenes_have_the_smallest_trees(pkg, oracle, wref):
    seen = set()
    for n in range(1, 6):
        sc = nf._tiny(n)
        pts = wc.points_for(sc, seed=n)
        records = ds.tp._tri_records(pkg, sc["meshes"])
        for b in TREES:
            nodes4q, tris, _ = chain_tree(pkg, oracle, sc, b)
            seen.add(len(nodes4q))
            wc.assert_moments(wref, nodes4q, tris, tw.ref_moments(wref, nodes4q, tris), "tiny%d %s" % (n, b))
            moments = tw.ref_moments(wref, nodes4q, tris)
            for beta in (0.0, float("inf")):  # (one to five triangles: n_tris * ATAN_BUDGET is no budget for a point 1 % from an edge)
                np.testing.assert_array_equal(_bits(tw.ref_tree(wref, nodes4q, tris, moments, beta, pts)), _bits(tw.ref_exact(wref, records, pts)))
    print("node counts of the tiny scenes' wide trees: %r" % sorted(seen))
    assert {1, 2} <= seen, "the one-leaf root and a two-node tree"
