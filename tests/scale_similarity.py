"""The scale-similarity harness of tests/test_scale_similarity.py: one scene, 257 ray and 257 point records, every length
of them scaled by 2^k with np.ldexp, and per query its reference run at scale k (the oracle's walk, tests/point_reference.c,
tests/list_hits_reference.c, tests/winding_reference.c, the float32 build of tests/grad_reference.c).

What scales: the vertices, ray origins, tmin / tmax, points and rmax by 2^k; directions stay.  Every float32 operation on
normal numbers commutes with that, so the outputs at scale k are the outputs at k = 0 with the exponent shifted by
SHIFT[name] * k.  The gradients take the loss as fixed: a derivative by a length carries 2^-k, so the incoming dL/dt and
dL/ddist are scaled by 2^-k and dL/d(u, v) is not.  From the header's formulas, lambda = (gt n + gu p + gv q) / det with
n = e1 x e2 ~ 2^2k, p = d x e2 and q = e1 x d ~ 2^k, det = -d . n ~ 2^2k: dL/do = lambda ~ 2^-k, dL/dd = t lambda ~ 2^0, the vertex
contributions -w lambda ~ 2^-k; for points s = g (p - c) / |p - c| ~ 2^-k and so are dL/dp and the contributions."""
import numpy as np

import grad_reference as G
import test_gradients as tg
import test_list_hits as tl
import test_point_queries as tp
import test_winding as tw
from test_query_direction_scale import _exact, base_rays

N = 257          # neither a multiple of 64 nor of 256
GRID = 12        # records sit on the grid 2^-12: a non-zero coordinate is at least 2^-12 and scales exactly down to 2^-137
QUERIES = ("trace_rays", "occluded", "count_hits", "list_hits", "closest_points", "occupancy", "winding_exact", "winding_beta2",
           "winding_beta8", "trace_rays_backward", "closest_points_backward")
# exponent of 2^k an output carries; names absent here are integers or bytes and do not change
SHIFT = {"t": 1, "dist": 1, "point": 1, "uv": 0, "w": 0, "grad_o": -1, "grad_d": 0, "grad_p": -1, "contrib": -1}
KINDS = {"trace_rays": "rays", "occluded": "rays", "count_hits": "rays", "list_hits": "rays", "trace_rays_backward": "rays"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _snap(x):
    """x rounded to the grid 2^-GRID (infinities and zeros stay)"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x), np.ldexp(np.round(np.ldexp(x, GRID)), -GRID), x).astype(np.float32)


def same_floats(a, b):
    """bitwise equality per element, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _ints(a):
    """ids and counts as int64, a 32-bit word read as unsigned (MISS is 0xFFFFFFFF whatever the array's type)"""
    a = np.ascontiguousarray(a)
    return (a.view(np.uint32) if a.dtype.itemsize == 4 else a).astype(np.int64)


class Harness:
    """the scene, the records and the references; reference(query, k) is cached"""

    def __init__(self, pkg, oracle, scenes, pref, lref, wref, gref):
        self.pkg, self.oracle, self.pref, self.lref, self.wref, self.gref = pkg, oracle, pref, lref, wref, gref
        self.meshes0 = [tw._sphere(scenes, keep=tw._not_first_octant), tg._quad()]
        sc = {"meshes": self.meshes0}
        rays = base_rays(pkg, sc, np.random.default_rng(71), N)
        rays[:, 0:3] = _snap(rays[:, 0:3])
        rays[:, [3, 7]] = _snap(rays[:, [3, 7]])
        self.rays0 = np.ascontiguousarray(rays)
        rng = np.random.default_rng(72)
        xyz = _snap(tw.shell_points(rng, N, tw.BANDS["open"]))
        self.points0 = np.ascontiguousarray(pkg.make_points(xyz, rmax=_snap(rng.choice([np.inf, 0.5, 2.0], size=N))))
        self.g_t = rng.normal(size=N).astype(np.float32)
        self.g_uv = rng.normal(size=(N, 2)).astype(np.float32)
        self.g_dist = rng.normal(size=N).astype(np.float32)
        self._cache = {}

    # ---- the inputs at scale k
    def meshes(self, k):
        return [dict(m, vertices=np.ldexp(np.asarray(m["vertices"], np.float32), k)) for m in self.meshes0]

    def rays(self, k):
        r = self.rays0.copy()
        r[:, 0:3] = np.ldexp(r[:, 0:3], k)
        r[:, [3, 7]] = np.ldexp(r[:, [3, 7]], k)
        return r

    def points(self, k):
        return np.ldexp(self.points0, k)

    def incoming(self, k):
        return {"g_t": np.ldexp(self.g_t, -k), "g_uv": self.g_uv, "g_dist": np.ldexp(self.g_dist, -k)}

    def scene_exact(self, k):
        return all(_exact(m["vertices"], k).all() for m in self.meshes0)

    def inputs_exact(self, query, k):
        """per record: its scaled inputs are exact and normal or zero"""
        if KINDS.get(query) == "rays":
            ok = _exact(self.rays0[:, 0:3], k).all(1) & _exact(self.rays0[:, 3], k) & _exact(self.rays0[:, 7], k)
            return ok & (_exact(self.g_t, -k) if query == "trace_rays_backward" else True)
        ok = _exact(self.points0, k).all(1)
        return ok & (_exact(self.g_dist, -k) if query == "closest_points_backward" else True)

    def scene_arrays(self, k):
        return G.SceneArrays([(m["vertices"], m["triangles"]) for m in self.meshes(k)])

    # ---- the references at scale k; `exported`: (nodes, tris, shade, nodes4q) of an upload, else the host SAH tree
    def reference(self, query, k, exported=None):
        key = (query, k)
        if exported is None and key in self._cache:
            return self._cache[key]
        out = getattr(self, "_ref_" + query.split("_beta")[0])(k, exported, *([float(query.split("_beta")[1])] if "_beta" in query else []))
        if exported is None:
            self._cache[key] = out
        return out

    def _oracle_scene(self, k, exported):
        S = self.oracle.OracleScene(self.meshes(k), [], tw.MATERIALS)
        if exported is not None:
            S.set_bvh(*exported[:3])
        return S

    def _ref_trace_rays(self, k, exported):
        S = self._oracle_scene(k, exported)
        try:
            res = self.oracle.trace_rays(S, self.rays(k))
        finally:
            S.close()
        return {q: res[q] for q in ("t", "uv", "inst", "prim")}

    def _ref_occluded(self, k, exported):
        S = self._oracle_scene(k, exported)
        try:
            return {"occluded": self.oracle.occluded_rays(S, self.rays(k))["occluded"].astype(np.uint8)}
        finally:
            S.close()

    def records(self, k):
        return tp._tri_records(self.pkg, self.meshes(k))

    def _ref_count_hits(self, k, exported):
        return {"count": tp.ref_count(self.pref, self.records(k), self.rays(k))}

    def _ref_list_hits(self, k, exported):
        return tl.ref_list(self.lref, self.records(k), self.rays(k))

    def _ref_closest_points(self, k, exported):
        return tp.ref_closest(self.pref, self.records(k), self.points(k))

    def _ref_occupancy(self, k, exported):
        return {"inside": tp.ref_occupancy(self.pref, self.records(k), self.points(k)).astype(np.uint8)}

    def _ref_winding_exact(self, k, exported):
        return {"w": tw.ref_exact(self.wref, self.records(k), self.points(k))}

    def host_tree(self, k):
        if ("tree", k) not in self._cache:
            self._cache[("tree", k)] = tw.host_tree(self.pkg, self.meshes(k))
        return self._cache[("tree", k)]

    def _ref_winding(self, k, exported, beta):
        nodes4q, tris = (exported[3], np.ascontiguousarray(exported[1])) if exported is not None else self.host_tree(k)
        return {"w": tw.ref_tree(self.wref, nodes4q, tris, tw.ref_moments(self.wref, nodes4q, tris), beta, self.points(k))}

    def _ref_trace_rays_backward(self, k, exported):
        hit = self.reference("trace_rays", k)
        g = self.incoming(k)
        grad, contrib, live = G.ray_reference(self.gref, self.scene_arrays(k), self.rays(k), hit["inst"], hit["prim"], hit["t"], hit["uv"], g["g_t"],
                                              g["g_uv"])
        return {"grad_o": grad[:, 0:4], "grad_d": grad[:, 4:8], "contrib": contrib.reshape(N, 9), "live": live.astype(np.uint8)}

    def _ref_closest_points_backward(self, k, exported):
        hit = self.reference("closest_points", k)
        grad, contrib, live = G.point_reference(self.gref, self.scene_arrays(k), self.points(k), hit["inst"], hit["prim"], hit["uv"],
                                                self.incoming(k)["g_dist"])
        return {"grad_p": grad, "contrib": contrib.reshape(N, 9), "live": live.astype(np.uint8)}

    # ---- the comparison
    def similar(self, query, got, k, base=None):
        """(the outputs `got` at scale k are those of k = 0 shifted, over the records that take part; how many records are left
        out).  A record takes part when its scaled inputs and its expected outputs are exact and normal or zero."""
        base = self.reference(query, 0) if base is None else base
        ok = self.inputs_exact(query, k) & self.scene_exact(k)
        per_hit = "offsets" in base
        if per_hit:  # list_hits: the lengths first, then every record of the rays that take part
            cnt0, cnt = np.diff(base["offsets"]), np.diff(np.asarray(got["offsets"], np.int64))
            if not np.array_equal(cnt0[ok], cnt[ok]):
                return False, int((~ok).sum())
        want = {}
        for name, v in base.items():
            if name == "offsets":
                continue
            rows = np.repeat(np.arange(N), cnt0) if per_hit else np.arange(N)
            if name in SHIFT:
                want[name] = np.ldexp(np.asarray(v, np.float32), SHIFT[name] * k)
                e = _exact(v, SHIFT[name] * k).reshape(len(rows), -1).all(1)
                np.logical_and.at(ok, rows[~e], False)
            else:
                want[name] = v
        good = True
        for name, w in want.items():
            if per_hit:
                sel0 = np.repeat(ok, cnt0)
                sel = np.repeat(ok, cnt)
                g, w = np.asarray(got[name])[sel], np.asarray(w)[sel0]
            else:
                g, w = np.asarray(got[name])[ok], np.asarray(w)[ok]
            good &= bool(same_floats(g, w).all()) if name in SHIFT else np.array_equal(_ints(g), _ints(w))
        return good, int((~ok).sum())

    def equal(self, got, want):
        """names of the outputs of `got` that differ from the reference `want` in any bit (a NaN equals a NaN)"""
        bad = []
        for name, w in want.items():
            g = np.asarray(got[name])
            w = np.asarray(w)
            if g.shape != w.shape:
                bad.append(name)
            elif w.dtype == np.float32:
                if not same_floats(g, w).all():
                    bad.append("%s (%d records)" % (name, int((~same_floats(g, w)).reshape(len(w), -1).any(1).sum()) if len(w) else 0))
            elif not np.array_equal(_ints(g), _ints(w)):
                bad.append(name)
        return bad


def similar_range(h, query, kmax=120, step=4):
    """the largest contiguous range of k around 0 over which `query`'s reference is similar, scanned in steps of `step` and then
    at every k between the last similar and the first dissimilar one; the most records left out at any k inside it; and
    the k inside it that are not similar after all (every k is looked at, not only the scanned ones).  The range
    also ends where a vertex of the scaled scene or a record is no longer a normal float32: less would be compared there"""
    def ok(k):
        return h.scene_exact(k) and h.similar(query, h.reference(query, k), k) == (True, 0)
    ends = []
    for sign in (-1, 1):
        last = 0
        for k in range(step, kmax + 1, step):
            if not ok(sign * k):
                break
            last = k
        end = last
        for k in range(last + 1, min(last + step, kmax + 1)):
            if not ok(sign * k):
                break
            end = k
        ends.append(sign * end)
    inside = {k: h.similar(query, h.reference(query, k), k) for k in range(ends[0], ends[1] + 1)}
    return ends[0], ends[1], max(n for _, n in inside.values()), [k for k, (good, _) in inside.items() if not good]
