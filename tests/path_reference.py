"""Float64 restatement of the mode-200 path spec (DESIGN.md section 3 "Path tracing", include/crt_hip.h CRT_MODE_PATH), for
the tests only.  It shares no arithmetic with the CPU oracle or the product: geometry is a brute-force closest hit over every
triangle, the RNG is the spec's integer hash chain on uint32, and every other quantity is float64.  Since it draws the same
random numbers as the kernels, a 1-spp pixel is one path, traced here without statistics.

Near a discontinuity (a ray grazing a triangle edge, two surfaces at nearly the same t, a shadow ray ending on an occluder,
a light at cos ~ 0, Snell's k ~ 0, a normal's z ~ 0 or a grazing hit) the float32 and float64 paths may legitimately take
different branches.  trace_paths records the margin of every such decision and flags the path when one falls below the
thresholds in MARGINS; the tests skip flagged paths and bound their share.

Textures.  The albedo of a hit is the material's, or its texture's when 0 <= texture < number of textures (any material type;
glass has no albedo term).  Kinds: albedo (colour a); edges (colour a where u, v or 1 - u - v of the hit's barycentrics is below
the width, else b); checker (width = trunc(1 / square_size), cells floor(c * width), a when the cell numbers' sum is even);
bitmap (c clamped to [0, 1], row trunc((1 - v) * (h - 1)), column trunc(u * (w - 1)), that texel / 255).  Checker and bitmap
take c = uv0 * w + uv1 * u + uv2 * v from the mesh's per-vertex uvs; a mesh without uvs has c = (0, 0).
Every lookup is a decision.  The float32 coordinate differs from c by the barycentrics' error, which MARGINS["bary"] bounds,
times the uv span of the triangle, |uv1 - uv0| + |uv2 - uv0|, plus three roundings (one product, two fmas) of at most
2^-24 max|uv| each: eps = 2e-5 * span + 3 * 2^-24 * max|uv| per axis.  A checker lookup is flagged when c * width lies within
eps * |width| + 2^-24 |c * width| (the product's rounding) of an integer; a bitmap lookup when c is within eps of a clamp it has
not clearly passed, or the texel coordinate within (eps + 2^-24) * (w - 1) + 2^-24 * coordinate of an integer (the extra 2^-24:
the rounding of 1 - v); a coordinate clamped on both sides gives an exact integer and w - 1 = 0 or h - 1 = 0 leaves nothing to
decide.  An edges lookup is flagged unless some barycentric is below width - MARGINS["bary"] or all are above width + it.
Confirmed in numpy float32 (Moeller-Trumbore, then the interpolation in the order above, on the 6 863 textured camera-ray hits
of the two textured scenes at pixel centres and with the jitter of the three seeds): the largest |float32 - float64| coordinate
difference is 7.8e-7, at most 12.3 % of eps; the largest barycentric difference 2.7e-6 against the margin's 2e-5.
Share of paths the reference alone flags, over max_bounces 0 / 1 / 2 / 5 and the three seeds: at most 0.49 % of a frame in
textured_room and 0.10 % in textured_glass (cap: 3 %); at pixel centres at most 0.10 %."""
import math
from collections import Counter

import numpy as np

RAY_TMIN, RAY_TMAX, BIAS = 0.001, 1e4, 1e-3
DIFFUSE, REFLECTIVE, REFRACTIVE, CONSTANT = 1, 2, 3, 4
MISS = 0xFFFFFFFF

# decision margins below which a path is not compared: barycentric (dimensionless), t (relative to 1 + t), cosines and k
MARGINS = {"bary": 2e-5, "t": 1e-4, "cos": 1e-5, "snell_k": 1e-4, "normal_z": 1e-6}

_U32 = np.uint32


def pcg_hash(v):
    """RXS-M-XS 32 on uint32 arrays (wrapping arithmetic)"""
    v = np.asarray(v, dtype=_U32)
    with np.errstate(over="ignore"):
        state = v * _U32(747796405) + _U32(2891336453)
        word = ((state >> ((state >> _U32(28)) + _U32(4))) ^ state) * _U32(277803737)
    return (word >> _U32(22)) ^ word


def rng_start(pix, sample, seed):
    """hash(pixel ^ hash(sample + hash(seed)))"""
    with np.errstate(over="ignore"):
        return pcg_hash(np.asarray(pix, dtype=_U32) ^ pcg_hash(np.asarray(sample, dtype=_U32) + pcg_hash(_U32(seed))))


def rng_next(state):
    """(new state, uniform in [0, 1) with 24 bits) -- exact in float32 and float64 alike"""
    state = pcg_hash(state)
    return state, (state >> _U32(8)).astype(np.float64) * 2.0 ** -24


def _norm(a):
    return a / np.sqrt(np.sum(a * a, axis=-1, keepdims=True))


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _cross(a, b):
    """a x b written as products and one subtraction per component: an exactly zero component gets the same sign of zero as
    the spec's fma(a.y, b.z, -(a.z * b.y)) (both are x + (-y) of the same exact products)"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def camera_dirs(rot, px, py, jx, jy, w, h):
    """ray_dir_j: pixel + jitter -> NDC -> normalize(x, y, -1) -> rotation (row-major, column vector) -> normalize"""
    x = (np.asarray(px, np.float64) + jx) / w
    y = (np.asarray(py, np.float64) + jy) / h
    x = (2.0 * x - 1.0) * (w / h)
    y = 1.0 - 2.0 * y
    dc = _norm(np.stack([x, y, -np.ones_like(x)], axis=-1))
    R = np.asarray(rot, np.float64).reshape(3, 3)
    return _norm(dc @ R.T)


_EPS32 = 2.0 ** -24
_KINDS = ("albedo", "edges", "checker", "bitmap")


def _parse_texture(t):
    """a texture dict of the tests -> float64: kind, colours a / b, scalar (edge width / square size), pixels (H, W, C)"""
    assert t["type"] in _KINDS
    T = {"kind": t["type"], "a": np.float32(t.get("color_a", (0, 0, 0))).astype(np.float64),
         "b": np.float32(t.get("color_b", (0, 0, 0))).astype(np.float64), "scalar": float(np.float32(t.get("scalar", 0.0)))}
    if T["kind"] == "checker":
        q = 1.0 / T["scalar"]
        T["width"] = int(math.trunc(q))
        # the number of squares is a decision too; the scenes keep 1 / square_size exact or well away from an integer
        assert q == round(q) == float(np.float32(1.0) / np.float32(T["scalar"])) or abs(q - round(q)) > 1e-3
    if T["kind"] == "bitmap":
        T["pixels"] = np.asarray(t["pixels"], np.uint8)
        assert T["pixels"].ndim == 3 and T["pixels"].shape[2] >= 3
    return T


def _from_integer(x):
    return np.abs(x - np.rint(x))


class Scene:
    """the scene dict of the tests (meshes / lights / materials), flattened to per-triangle float64 arrays"""

    def __init__(self, sc):
        v0, e1, e2, inst, prim, mat, nrm, uv = [], [], [], [], [], [], [], []
        for mi, m in enumerate(sc["meshes"]):
            v = np.asarray(m["vertices"], np.float32).astype(np.float64).reshape(-1, 3)
            t = np.asarray(m["triangles"], np.int64).reshape(-1, 3)
            v0.append(v[t[:, 0]])
            e1.append(v[t[:, 1]] - v[t[:, 0]])
            e2.append(v[t[:, 2]] - v[t[:, 0]])
            inst.append(np.full(len(t), mi))
            prim.append(np.arange(len(t)))
            mat.append(np.full(len(t), int(m.get("material_index", 0))))
            n = m.get("normals")
            n = np.zeros_like(v) if n is None else np.asarray(n, np.float32).astype(np.float64).reshape(-1, 3)
            nrm.append(np.stack([n[t[:, 0]], n[t[:, 1]], n[t[:, 2]]], axis=1))
            c = m.get("uvs")  # (u, v, unused) per vertex; a mesh without them has the coordinate (0, 0) everywhere
            c = np.zeros((len(v), 2)) if c is None else np.asarray(c, np.float32).astype(np.float64).reshape(-1, 3)[:, :2]
            uv.append(np.stack([c[t[:, 0]], c[t[:, 1]], c[t[:, 2]]], axis=1))
        self.v0, self.e1, self.e2 = np.concatenate(v0), np.concatenate(e1), np.concatenate(e2)
        self.inst, self.prim, self.nrm = np.concatenate(inst), np.concatenate(prim), np.concatenate(nrm)
        self.uv = np.concatenate(uv)
        self.textures = [_parse_texture(t) for t in (sc.get("textures") or ())]
        mats = list(sc["materials"])
        matidx = np.concatenate(mat)
        known = matidx < len(mats)  # a triangle without a material is white DIFFUSE
        self.albedo = np.ones((len(matidx), 3))
        self.mtype = np.full(len(matidx), DIFFUSE)
        self.smooth = np.zeros(len(matidx), bool)
        self.ior = np.ones(len(matidx))
        self.tex = np.full(len(matidx), -1)           # texture of the triangle's material, -1: its own albedo
        self.tex_past = np.zeros(len(matidx), bool)   # a texture index at or past the end of the table: ignored
        for k in range(len(matidx)):
            if known[k]:
                M = mats[matidx[k]]
                self.albedo[k] = np.float32(M.get("albedo", (1, 1, 1))).astype(np.float64)
                self.mtype[k] = int(M.get("type", 1))
                self.smooth[k] = bool(M.get("smooth_shading", False))
                self.ior[k] = float(np.float32(M.get("ior", 1.0)))
                ti = int(M.get("texture", -1))
                if 0 <= ti < len(self.textures):
                    self.tex[k] = ti
                self.tex_past[k] = ti >= len(self.textures)
        self.lights = [(np.float32(p).astype(np.float64), float(np.float32(i))) for p, i in sc["lights"]]

    def intersect(self, o, d):
        """Moeller-Trumbore of every ray with every triangle: t, u, v of shape (rays, triangles)"""
        p = _cross(d[:, None, :], self.e2[None])
        det = _dot(self.e1[None], p)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            s = o[:, None, :] - self.v0[None]
            u = _dot(s, p) * inv
            q = _cross(s, self.e1[None])
            v = _dot(d[:, None, :], q) * inv
            t = _dot(self.e2[None], q) * inv
        return t, u, v

    def closest(self, o, d, tmin, tmax=RAY_TMAX):
        """closest hit in (tmin, tmax), ties to the lower triangle: (hit, tri, t, u, v, robust)"""
        t, u, v = self.intersect(o, d)
        m = np.minimum(np.minimum(u, v), 1.0 - u - v)
        ok = np.isfinite(t) & np.isfinite(m)
        m = np.where(ok, m, -np.inf)
        t = np.where(ok, t, np.nan)
        hitm = (t > tmin) & (t < tmax) & (m >= 0.0)
        tt = np.where(hitm, t, np.inf)
        tri = np.argmin(tt, axis=1)
        rows = np.arange(len(o))
        tb = tt[rows, tri]
        hit = np.isfinite(tb)
        tref = np.where(hit, tb, 0.0)
        tol = MARGINS["t"] * (1.0 + np.abs(t))
        cand = (m > -MARGINS["bary"]) & (t > tmin - tol) & (t < tmax + tol)
        near_tmin = np.any(cand & (t <= tmin + tol), axis=1)
        others = cand.copy()
        others[rows, tri] &= ~hit
        rival = np.any(others & (t < tref[:, None] + MARGINS["t"] * (1.0 + tref[:, None])), axis=1)
        robust = np.where(hit, (m[rows, tri] >= MARGINS["bary"]) & ~rival & ~near_tmin, ~np.any(cand, axis=1))
        return hit, tri, tref, u[rows, tri], v[rows, tri], robust

    def occluded(self, o, d, dist):
        """any triangle in (0, dist): (occluded, robust)"""
        t, u, v = self.intersect(o, d)
        m = np.minimum(np.minimum(u, v), 1.0 - u - v)
        ok = np.isfinite(t) & np.isfinite(m)
        m = np.where(ok, m, -np.inf)
        t = np.where(ok, t, np.nan)
        D = dist[:, None]
        occ = np.any((m >= 0.0) & (t > 0.0) & (t < D), axis=1)
        tol = MARGINS["t"] * (1.0 + np.abs(t))
        edge = (np.abs(m) < MARGINS["bary"]) & (t > -tol) & (t < D + tol)
        ends = (m > -MARGINS["bary"]) & ((np.abs(t) < tol) | (np.abs(t - D) < tol))
        return occ, ~np.any(edge | ends, axis=1)

    def surface(self, o, d, tri, t, u, v):
        """hit point, unit normal facing the ray (interpolated for smooth materials), entering flag, robustness of the flip"""
        P = o + d * t[:, None]
        N = _cross(self.e1[tri], self.e2[tri])
        w = 1.0 - u - v
        n = self.nrm[tri]
        Ns = n[:, 0] * w[:, None] + n[:, 1] * u[:, None] + n[:, 2] * v[:, None]
        use = self.smooth[tri] & (_dot(Ns, Ns) > 0.0)
        N = _norm(np.where(use[:, None], Ns, N))
        nd = _dot(N, d)
        entering = ~(nd > 0.0)
        N = np.where(entering[:, None], N, -N)
        return P, N, entering, np.abs(nd) >= MARGINS["cos"]

    def albedo_at(self, tri, u, v, ev, all_diffuse=False, after_bounce=False):
        """albedo of hits (tri, u, v): the material's, or its texture's when the material names one inside the table.  The edges
        texture is a function of the hit's barycentrics, every other kind of uv0 * w + uv1 * u + uv2 * v.  Returns (rgb, robust):
        robust is False where a float32 evaluation could pick another cell / texel / side (module docstring, "Textures").
        Glass never uses its albedo, so its lookups decide nothing (unless all_diffuse: mode 100 shades every material alike)."""
        rgb = self.albedo[tri].copy()
        robust = np.ones(len(tri), bool)
        ti, mt = self.tex[tri], self.mtype[tri]
        w = 1.0 - u - v
        ev["tex_index_past_table"] += int(np.sum(self.tex_past[tri]))
        ev["tex_on_glass_or_mirror"] += int(np.sum((ti >= 0) & ((mt == REFLECTIVE) | (mt == REFRACTIVE))))
        plain = (mt != REFLECTIVE) & (mt != REFRACTIVE) & (mt != CONSTANT)
        if after_bounce:
            ev["tex_after_bounce"] += int(np.sum((ti >= 0) & plain))
        for k in np.unique(ti[ti >= 0]):
            sel = np.nonzero(ti == k)[0]
            T = self.textures[k]
            ev["tex_" + T["kind"]] += len(sel)
            ok = np.ones(len(sel), bool)
            if T["kind"] == "albedo":
                col = np.repeat(T["a"][None], len(sel), axis=0)
            elif T["kind"] == "edges":
                x = np.stack([u[sel], v[sel], w[sel]], axis=-1)
                edge = np.any(x < T["scalar"], axis=-1)
                m = MARGINS["bary"]
                ok = np.any(x < T["scalar"] - m, axis=-1) | np.all(x >= T["scalar"] + m, axis=-1)
                ev["edges_edge"] += int(edge.sum())
                ev["edges_inner"] += int(np.sum(~edge))
                col = np.where(edge[:, None], T["a"][None], T["b"][None])
            else:
                U = self.uv[tri[sel]]
                c = U[:, 0] * w[sel, None] + U[:, 1] * u[sel, None] + U[:, 2] * v[sel, None]
                # float32 coordinate - float64 coordinate: the barycentrics' error times the triangle's uv span + three roundings
                eps = (MARGINS["bary"] * (np.abs(U[:, 1] - U[:, 0]) + np.abs(U[:, 2] - U[:, 0]))
                       + 3.0 * _EPS32 * np.max(np.abs(U), axis=1))
                if T["kind"] == "checker":
                    x = c * T["width"]
                    ok = np.all(_from_integer(x) >= eps * abs(T["width"]) + _EPS32 * np.abs(x), axis=-1)
                    even = np.sum(np.floor(x), axis=-1) % 2.0 == 0.0
                    ev["checker_negative"] += int(np.sum(np.any(c < 0.0, axis=-1)))
                    ev["checker_above_1"] += int(np.sum(np.any(c > 1.0, axis=-1)))
                    col = np.where(even[:, None], T["a"][None], T["b"][None])
                else:
                    px = T["pixels"]
                    scale = np.array([px.shape[1] - 1.0, px.shape[0] - 1.0])
                    for ax, name in ((0, "u"), (1, "v")):
                        ev["bitmap_%s_low" % name] += int(np.sum(c[:, ax] < 0.0))
                        ev["bitmap_%s_high" % name] += int(np.sum(c[:, ax] > 1.0))
                    cc = np.clip(c, 0.0, 1.0)
                    x = np.stack([cc[:, 0], 1.0 - cc[:, 1]], axis=-1) * scale
                    clamped = (c <= -eps) | (c >= 1.0 + eps)  # 0 or 1 exactly on both sides: the texel index is an exact integer
                    inside = (c >= eps) & (c <= 1.0 - eps)
                    sure = inside & (_from_integer(x) >= (eps + _EPS32) * scale + _EPS32 * x)
                    ok = np.all(clamped | sure | (scale == 0.0), axis=-1)
                    at = np.trunc(x).astype(np.int64)
                    col = px[at[:, 1], at[:, 0], :3].astype(np.float64) / 255.0
            rgb[sel] = col
            robust[sel] = ok
        if not all_diffuse:
            robust |= mt == REFRACTIVE
        return rgb, robust

    def direct(self, Po, N, albedo, ev, view=None, ks=0.0, exponent=32):
        """sum over the lights of albedo * I / (4 pi r^2) * cos where the shadow ray (Po, L/r, 0, r) is clear; cos <= 0
        traces nothing.  view (mode 100): adds the white Phong term ks * I/(4 pi r^2) * max(0, R.view)^exponent."""
        rgb = np.zeros_like(Po)
        robust = np.ones(len(Po), bool)
        for lp, inten in self.lights:
            Lv = lp[None] - Po
            r2 = _dot(Lv, Lv)
            dist = np.sqrt(r2)
            Ld = Lv / dist[:, None]
            c = _dot(N, Ld)
            robust &= np.abs(c) >= MARGINS["cos"]
            lit = c > 0.0
            ev["light_behind"] += int(np.sum(~lit))
            occ = np.zeros(len(Po), bool)
            if lit.any():
                oc, rb = self.occluded(Po[lit], Ld[lit], dist[lit])
                occ[lit] = oc
                robust[lit] &= rb
            ev["shadowed"] += int(np.sum(lit & occ))
            ev["lit"] += int(np.sum(lit & ~occ))
            k = np.where(lit & ~occ, inten / (4.0 * math.pi * r2) * np.maximum(c, 0.0), 0.0)
            rgb += albedo * k[:, None]
            if view is not None and ks > 0.0:
                R = 2.0 * _dot(N, Ld)[:, None] * N - Ld
                rv = np.maximum(0.0, _dot(R, view))
                rgb += np.where(lit & ~occ, ks * inten / (4.0 * math.pi * r2) * rv ** exponent, 0.0)[:, None]
        return rgb, robust


def trace_paths(S, cam_pos, cam_rot, w, h, miss, max_bounces, seed, sample=0):
    """One path per pixel (sample index `sample`) of a w x h frame.  Returns a dict: rgb (h, w, 3), inst / prim / t of the
    camera ray's hit, segments (closest-hit rays per path), robust (h, w) and ev (Counter of what the paths did)."""
    n = w * h
    pix = np.arange(n, dtype=np.uint32)
    st = rng_start(pix, np.full(n, sample, np.uint32), seed)
    st, jx = rng_next(st)
    st, jy = rng_next(st)
    o = np.repeat(np.float32(cam_pos).astype(np.float64)[None], n, axis=0)
    d = camera_dirs(cam_rot, pix % w, pix // w, jx, jy, w, h)
    miss = np.float32(miss).astype(np.float64)
    L = np.zeros((n, 3))
    thr = np.ones((n, 3))
    robust = np.ones(n, bool)
    segs = np.zeros(n, np.int64)
    prev = np.zeros(n, np.int64)  # material of the last surface the path left (0 = camera)
    inst0, prim0, t0 = np.full(n, MISS, np.uint32), np.full(n, MISS, np.uint32), np.full(n, RAY_TMAX)
    ev = Counter()
    alive = np.arange(n)
    tmin = RAY_TMIN
    for bounce in range(max_bounces + 1):
        if len(alive) == 0:
            break
        segs[alive] += 1
        hit, tri, t, u, v, rb = S.closest(o[alive], d[alive], tmin)
        robust[alive] &= rb
        if bounce == 0:
            inst0[alive[hit]] = S.inst[tri[hit]]
            prim0[alive[hit]] = S.prim[tri[hit]]
            t0[alive[hit]] = t[hit]
        ms = alive[~hit]
        L[ms] += thr[ms] * miss
        ev["miss_direct" if bounce == 0 else "miss_after_bounce"] += len(ms)
        alive, tri, t, u, v = alive[hit], tri[hit], t[hit], u[hit], v[hit]
        if len(alive) == 0:
            break
        P, N, entering, rb = S.surface(o[alive], d[alive], tri, t, u, v)
        robust[alive] &= rb
        mt = S.mtype[tri]
        alb, rb = S.albedo_at(tri, u, v, ev, after_bounce=bounce > 0)
        robust[alive] &= rb
        nxt_o, nxt_d = np.zeros((len(alive), 3)), np.zeros((len(alive), 3))
        goes = np.zeros(len(alive), bool)
        cut = bounce == max_bounces

        k = mt == CONSTANT
        L[alive[k]] += thr[alive[k]] * alb[k]
        ev["emit_direct"] += int(np.sum(k & (prev[alive] == 0)))
        ev["emit_after_mirror"] += int(np.sum(k & (prev[alive] == REFLECTIVE)))
        ev["emit_after_diffuse"] += int(np.sum(k & (prev[alive] == DIFFUSE)))

        k = mt == REFLECTIVE
        ev["mirror_cut" if cut else "mirror"] += int(k.sum())
        if not cut and k.any():
            dd = d[alive[k]]
            kk = 2.0 * _dot(dd, N[k])
            nxt_d[k] = _norm(dd - kk[:, None] * N[k])
            nxt_o[k] = P[k] + N[k] * BIAS
            thr[alive[k]] *= alb[k]
            goes |= k

        k = mt == REFRACTIVE
        ev["refract_cut" if cut else "refract"] += int(k.sum())
        if not cut and k.any():
            dd, Nk = d[alive[k]], N[k]
            eta = np.where(entering[k], 1.0 / S.ior[tri[k]], S.ior[tri[k]])
            cosi = -_dot(dd, Nk)
            kq = 1.0 - eta * eta * (1.0 - cosi * cosi)
            robust[alive[k]] &= np.abs(kq) >= MARGINS["snell_k"]
            tir = kq < 0.0
            refl = dd - (2.0 * _dot(dd, Nk))[:, None] * Nk
            with np.errstate(invalid="ignore"):
                trans = eta[:, None] * dd + (eta * cosi - np.sqrt(np.maximum(kq, 0.0)))[:, None] * Nk
            nxt_d[k] = _norm(np.where(tir[:, None], refl, trans))
            nxt_o[k] = P[k] + Nk * np.where(tir, BIAS, -BIAS)[:, None]
            ev["tir"] += int(tir.sum())
            ev["enter"] += int(np.sum(~tir & entering[k]))
            ev["exit"] += int(np.sum(~tir & ~entering[k]))
            goes |= k

        k = (mt != CONSTANT) & (mt != REFLECTIVE) & (mt != REFRACTIVE)
        if k.any():
            Po = P[k] + N[k] * BIAS
            Ld, rb = S.direct(Po, N[k], alb[k], ev)
            robust[alive[k]] &= rb
            L[alive[k]] += thr[alive[k]] * Ld
            if not cut:
                ak = alive[k]
                st[ak], u1 = rng_next(st[ak])
                st[ak], u2 = rng_next(st[ak])
                rr, phi = np.sqrt(u1), 2.0 * math.pi * u2
                lx, ly, lz = rr * np.cos(phi), rr * np.sin(phi), np.sqrt(np.maximum(0.0, 1.0 - u1))
                Nk = N[k]
                nz = Nk[:, 2]
                robust[ak] &= (nz == 0.0) | (np.abs(nz) >= MARGINS["normal_z"])
                sg = np.copysign(1.0, nz)
                a = -1.0 / (sg + nz)
                b = Nk[:, 0] * Nk[:, 1] * a
                T = np.stack([1.0 + sg * Nk[:, 0] * Nk[:, 0] * a, sg * b, -sg * Nk[:, 0]], axis=-1)
                B = np.stack([b, sg + Nk[:, 1] * Nk[:, 1] * a, -Nk[:, 1]], axis=-1)
                nxt_d[k] = _norm(lx[:, None] * T + ly[:, None] * B + lz[:, None] * Nk)
                nxt_o[k] = Po
                thr[ak] *= alb[k]
                goes |= k
                ev["diffuse_bounce"] += int(k.sum())
                ev["basis_sg+"] += int(np.sum(sg > 0))
                ev["basis_sg-"] += int(np.sum(sg < 0))
                ev["basis_nz=+0"] += int(np.sum((nz == 0.0) & (sg > 0)))
                ev["basis_nz=-0"] += int(np.sum((nz == 0.0) & (sg < 0)))
        prev[alive] = mt
        o[alive[goes]] = nxt_o[goes]
        d[alive[goes]] = nxt_d[goes]
        alive = alive[goes]
        tmin = 0.0
    return {"rgb": L.reshape(h, w, 3), "inst": inst0.reshape(h, w), "prim": prim0.reshape(h, w), "t": t0.reshape(h, w),
            "segments": segs.reshape(h, w), "robust": robust.reshape(h, w), "ev": ev}


def shade_centres(S, cam_pos, cam_rot, w, h, mode, miss, ks=0.0, exponent=32, ev=None):
    """modes 3 (barycentric), 5 (distance) and 100 (Lambert + Phong) at pixel centres, float64: (rgb, robust, inst, prim, t);
    ev: a Counter that receives the texture events of mode 100"""
    n = w * h
    pix = np.arange(n)
    o = np.repeat(np.float32(cam_pos).astype(np.float64)[None], n, axis=0)
    d = camera_dirs(cam_rot, pix % w, pix // w, 0.5, 0.5, w, h)
    hit, tri, t, u, v, robust = S.closest(o, d, RAY_TMIN)
    rgb = np.repeat(np.float32(miss).astype(np.float64)[None], n, axis=0)
    if mode == 3:
        rgb[hit] = np.stack([1.0 - u - v, u, v], axis=-1)[hit]
    elif mode == 5:
        rgb[hit] = np.clip(t * 0.05, 0.0, 1.0)[hit, None]
    else:
        P, N, _, rb = S.surface(o[hit], d[hit], tri[hit], t[hit], u[hit], v[hit])
        robust[hit] &= rb
        alb, rb = S.albedo_at(tri[hit], u[hit], v[hit], Counter() if ev is None else ev, all_diffuse=True)
        robust[hit] &= rb
        c, rb = S.direct(P + N * BIAS, N, alb, Counter(), view=-d[hit], ks=ks, exponent=exponent)
        robust[hit] &= rb
        rgb[hit] = c
    inst = np.where(hit, S.inst[tri], MISS).astype(np.uint32)
    prim = np.where(hit, S.prim[tri], MISS).astype(np.uint32)
    return (rgb.reshape(h, w, 3), robust.reshape(h, w), inst.reshape(h, w), prim.reshape(h, w),
            np.where(hit, t, RAY_TMAX).reshape(h, w))


# ---- scenes: small (< 200 triangles), each aimed at places where the path code can go wrong

def _mesh(v, t, mat, normals=None):
    return {"vertices": np.asarray(v, np.float32).reshape(-1, 3), "triangles": np.asarray(t, np.uint32).reshape(-1, 3),
            "material_index": mat, "normals": None if normals is None else np.asarray(normals, np.float32).reshape(-1, 3)}


def quad(a, b, c, d, mat):
    """two triangles (a, b, c), (a, c, d): normal along (b - a) x (c - a)"""
    return _mesh([a, b, c, d], [(0, 1, 2), (0, 2, 3)], mat)


def box(lo, hi, mat):
    """closed box, every face wound so that (v1 - v0) x (v2 - v0) points out"""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    faces = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]
    tris = [t for a, b, c, d in faces for t in ((a, b, c), (a, c, d))]
    return _outward(_mesh(v, tris, mat))


def _outward(m):
    v = m["vertices"].astype(np.float64)
    ctr = v.mean(axis=0)
    for t in m["triangles"]:
        n = np.cross(v[t[1]] - v[t[0]], v[t[2]] - v[t[0]])
        assert np.dot(n, v[t].mean(axis=0) - ctr) > 0.0, "inward face"
    return m


def prism(x0, x1, z0, y0, y1, mat):
    """right prism along y; right angle at (x1, z0); legs facing +z (z = z0) and +x (x = x1), hypotenuse at 45 degrees from
    (x0, z0) to (x1, z0 - (x1 - x0)): a ray along -z through the +z leg meets the hypotenuse at 45 degrees"""
    z1 = z0 - (x1 - x0)
    cs = [(x0, z0), (x1, z0), (x1, z1)]
    v = [(x, y0, z) for x, z in cs] + [(x, y1, z) for x, z in cs]
    tris = [(0, 2, 1), (3, 4, 5)]  # caps
    for a, b in ((0, 1), (1, 2), (2, 0)):
        tris += [(a, b, b + 3), (a, b + 3, a + 3)]
    m = _mesh(v, tris, mat)
    vv = m["vertices"].astype(np.float64)
    ctr = vv.mean(axis=0)
    tt = m["triangles"].copy()
    for i, t in enumerate(tt):  # wind every face outward
        n = np.cross(vv[t[1]] - vv[t[0]], vv[t[2]] - vv[t[0]])
        if np.dot(n, vv[t].mean(axis=0) - ctr) < 0.0:
            tt[i] = t[[0, 2, 1]]
    m["triangles"] = tt
    return _outward(m)


def icosphere(scenes, centre, radius, subdiv, mat):
    v, f = scenes._icosphere(subdiv)
    v = (v * radius + np.asarray(centre)).astype(np.float32)
    m = _outward(_mesh(v, f, mat))
    m["normals"] = scenes.vertex_normals(m["vertices"], m["triangles"])
    return m


def _sc(meshes, lights, materials, pos, rot):
    return {"meshes": meshes, "lights": lights, "materials": materials,
            "camera": {"position": np.float32(pos), "matrix": np.float32(rot).reshape(9)}}


def _backdrop(floor_mat, wall_mat):
    return [quad((-6, -1, 3), (6, -1, 3), (6, -1, -8), (-6, -1, -8), floor_mat),
            quad((-6, -1, -8), (6, -1, -8), (6, 5, -8), (-6, 5, -8), wall_mat)]


def scene_room(scenes):
    """Closed room of diffuse walls facing +-x, +-y, +-z (the ceiling and the right wall wound outward, so their normals are
    flipped towards the ray: a zero normal z comes out as +0 on some walls and -0 on others), an oblique panel,
    a blocker box that shades part of the floor from light 0, and light 1 behind the panel's back and the blocker's far side.
    Albedos differ per channel."""
    mats = [{"albedo": a, "type": DIFFUSE} for a in
            ((0.8, 0.5, 0.3), (0.3, 0.7, 0.5), (0.6, 0.4, 0.9), (0.9, 0.8, 0.2), (0.4, 0.6, 0.8), (0.7, 0.3, 0.6),
             (0.5, 0.9, 0.4), (0.85, 0.75, 0.65))]
    x0, x1, y0, y1, z0, z1 = -2.0, 2.0, -1.5, 1.5, -6.0, 2.0
    meshes = [quad((x0, y0, z1), (x1, y0, z1), (x1, y0, z0), (x0, y0, z0), 0),   # floor, normal +y
              quad((x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0), 1),   # ceiling, wound +y (faces -y once flipped)
              quad((x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1), 2),   # left wall
              quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1), 3),   # right wall, wound +x (flipped)
              quad((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), 4),   # back wall, normal +z
              quad((x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1), 5)]   # wall behind the camera, normal -z
    c, r = np.array([0.9, -0.4, -3.6]), scenes.camera_matrix(35.0, 25.0).reshape(3, 3).astype(np.float64)
    pts = [c + r @ np.array(p) for p in ((-0.6, -0.5, 0), (0.6, -0.5, 0), (0.6, 0.5, 0), (-0.6, 0.5, 0))]
    meshes.append(quad(*pts, 6))
    meshes.append(box((-1.1, -1.5, -3.4), (-0.4, -0.8, -2.7), 7))
    lights = [((-0.7, 1.2, -3.0), 40.0), ((1.6, 0.3, -4.8), 25.0)]
    return _sc(meshes, lights, mats, (0.0, 0.0, 1.5), scenes.camera_matrix(0.0, -5.0))


def scene_mirrors(scenes):
    """Mirror floor and two facing mirror walls, a diffuse back wall, a CONSTANT ceiling panel (seen directly, in the mirrors
    and after diffuse bounces) and an open top and front: misses after bounces."""
    mats = [{"albedo": (0.9, 0.8, 0.7), "type": REFLECTIVE}, {"albedo": (0.95, 0.85, 0.6), "type": REFLECTIVE},
            {"albedo": (0.7, 0.5, 0.6), "type": DIFFUSE}, {"albedo": (1.6, 1.2, 0.6), "type": CONSTANT}]
    meshes = [quad((-1.2, -1, 1), (1.2, -1, 1), (1.2, -1, -5), (-1.2, -1, -5), 0),
              quad((-1.2, -1, -5), (-1.2, 2, -5), (-1.2, 2, 1), (-1.2, -1, 1), 1),
              quad((1.2, -1, 1), (1.2, 2, 1), (1.2, 2, -5), (1.2, -1, -5), 1),
              quad((-1.2, -1, -5), (1.2, -1, -5), (1.2, 2, -5), (-1.2, 2, -5), 2),
              quad((-0.6, 1.0, -2.0), (0.6, 1.0, -2.0), (0.6, 1.0, -4.0), (-0.6, 1.0, -4.0), 3)]
    lights = [((0.3, 1.6, -3.0), 30.0)]
    return _sc(meshes, lights, mats, (0.2, 0.1, 0.6), scenes.camera_matrix(12.0, 8.0))


_GLASS_MATS = [{"albedo": (0.6, 0.7, 0.8), "type": DIFFUSE}, {"albedo": (0.8, 0.6, 0.5), "type": DIFFUSE},
               {"albedo": (1.0, 1.0, 1.0), "type": REFRACTIVE, "ior": 1.5}]
_GLASS_LIGHTS = [((2.0, 3.0, 0.0), 60.0), ((-2.5, 2.0, -3.0), 40.0)]


def scene_slab(scenes):
    """a glass slab with outward winding seen obliquely: rays enter (eta = 1/ior) and exit (eta = ior)"""
    meshes = _backdrop(0, 1) + [box((-1.0, -0.9, -3.2), (1.0, 0.9, -2.6), 2)]
    return _sc(meshes, _GLASS_LIGHTS, _GLASS_MATS, (1.2, 0.8, 0.5), scenes.camera_matrix(25.0, -12.0))


def scene_prism(scenes):
    """a 45-degree glass prism: rays through the +z leg meet the hypotenuse beyond the critical angle (total internal
    reflection) or, further off axis, refract out of it"""
    meshes = _backdrop(0, 1) + [prism(-0.8, 0.8, -1.6, -0.9, 0.9, 2)]
    return _sc(meshes, _GLASS_LIGHTS, _GLASS_MATS, (0.0, 0.0, 0.4), scenes.camera_matrix(0.0, 0.0))


def scene_sphere(scenes):
    """a smooth-shaded low-poly glass icosphere (80 triangles): interpolated normals decide entering / exiting"""
    meshes = _backdrop(0, 1) + [icosphere(scenes, (0.0, -0.1, -2.6), 0.8, 1, 2)]
    mats = [dict(m) for m in _GLASS_MATS]
    mats[2]["smooth_shading"] = True
    return _sc(meshes, _GLASS_LIGHTS, mats, (0.0, 0.2, 0.4), scenes.camera_matrix(0.0, -4.0))



# ---- textured scenes: every texture kind, uvs below 0 and above 1, several bitmaps in one table

def _planar(m, pu, pv):
    """per-vertex uvs (u, v, unused) as affine functions of the position: pu, pv = (cx, cy, cz, offset)"""
    v = m["vertices"].astype(np.float64)
    uv = np.stack([v @ np.array(pu[:3]) + pu[3], v @ np.array(pv[:3]) + pv[3], np.zeros(len(v))], axis=1)
    m["uvs"] = uv.astype(np.float32)
    return m


def _bitmap(w, h, channels=3):
    """a w x h image without two equal neighbours in any channel; the fourth channel, where there is one, holds values that no
    colour channel takes at that texel"""
    yy, xx = np.mgrid[0:h, 0:w]
    ch = [(xx * 37 + yy * 11 + 20) % 256, (xx * 13 + yy * 53 + 90) % 256, (xx * 29 + yy * 31 + 160) % 256, (xx * 7 + yy * 3 + 5) % 256]
    return np.stack(ch[:channels], axis=-1).astype(np.uint8)


_CHK_A, _CHK_B = (0.85, 0.8, 0.7), (0.25, 0.3, 0.55)
_TEXTURES = [
    {"type": "checker", "color_a": _CHK_A, "color_b": _CHK_B, "scalar": 0.125},             # 0: 8 squares
    {"type": "checker", "color_a": (0.7, 0.85, 0.6), "color_b": (0.35, 0.2, 0.3), "scalar": 0.3},    # 1: 3
    {"type": "checker", "color_a": (0.6, 0.7, 0.9), "color_b": (0.5, 0.25, 0.2), "scalar": 0.07},    # 2: 14
    {"type": "checker", "color_a": (0.9, 0.6, 0.5), "color_b": (0.2, 0.5, 0.4), "scalar": 0.6},      # 3: 1
    {"type": "checker", "color_a": (0.55, 0.75, 0.65), "color_b": (0.9, 0.1, 0.1), "scalar": 2.0},   # 4: 0, all colour a
    {"type": "edges", "color_a": (0.95, 0.85, 0.2), "color_b": (0.6, 0.15, 0.1), "scalar": 0.04},    # 5
    {"type": "edges", "color_a": (0.1, 0.9, 0.9), "color_b": (0.5, 0.45, 0.8), "scalar": 0.0},       # 6: all inner
    {"type": "edges", "color_a": (0.8, 0.4, 0.7), "color_b": (0.1, 0.1, 0.9), "scalar": 0.5},        # 7: all edge
    {"type": "bitmap", "pixels": _bitmap(17, 13)},                                                  # 8
    {"type": "bitmap", "pixels": _bitmap(5, 3, 4)},                                                 # 9: RGBA
    {"type": "bitmap", "pixels": _bitmap(1, 9)},                                                    # 10: w - 1 = 0
    {"type": "bitmap", "pixels": _bitmap(9, 1)},                                                    # 11: h - 1 = 0
    {"type": "bitmap", "pixels": _bitmap(1, 1)[:, :, ::-1]},                                        # 12
    {"type": "albedo", "color_a": (0.3, 0.8, 0.45)},                                                # 13
]


def scene_textured_room(scenes):
    """scene_room's closed room with floor, ceiling and side walls cut into three strips along z, one texture per surface.
    Material i < 14 has texture i (and an albedo that no texture yields).  Floor: checkers on uvs from -0.8 to 1.4 and -1.7 to
    1.1.  Ceiling: bitmaps 17x13 and 9x1 with u from -0.3 to 1.3, and the albedo texture.  Left wall: the three edges textures,
    on a mesh whose uvs are far from any barycentric.  Right wall: RGBA, 1x9 and 1x1 bitmaps on rotated uvs (u along y, v along
    z, both leaving [0, 1]).  Back wall: the 14-square checker with u decreasing as x grows.  Behind the camera: the 1-square
    checker.  A panel without uvs whose bitmap is therefore read at (0, 0), a box with planar uvs, and a second panel whose
    material names texture 14 of 14: its own albedo."""
    n = len(_TEXTURES)
    own = [(0.31 + 0.04 * (i % 5), 0.62 - 0.05 * (i % 4), 0.43 + 0.06 * (i % 3)) for i in range(n)]
    mats = [{"albedo": own[i], "type": DIFFUSE, "texture": i} for i in range(n)]
    mats.append({"albedo": (0.75, 0.35, 0.55), "type": DIFFUSE, "texture": n})  # 14: index past the table
    x0, x1, y0, y1 = -2.0, 2.0, -1.5, 1.5
    zs = (2.0, -1.0, -3.5, -6.0)
    meshes = []
    for k, mat in enumerate((0, 1, 4)):  # floor, normal +y
        za, zb = zs[k], zs[k + 1]
        meshes.append(_planar(quad((x0, y0, za), (x1, y0, za), (x1, y0, zb), (x0, y0, zb), mat), (0.55, 0, 0, 0.3), (0, 0, 0.35, 0.4)))
    for k, mat in enumerate((8, 11, 13)):  # ceiling
        za, zb = zs[k], zs[k + 1]
        meshes.append(_planar(quad((x0, y1, za), (x1, y1, za), (x1, y1, zb), (x0, y1, zb), mat), (0.4, 0, 0, 0.5), (0, 0, -0.3, 0.2)))
    for k, mat in enumerate((5, 6, 7)):  # left wall
        za, zb = zs[k], zs[k + 1]
        meshes.append(_planar(quad((x0, y0, zb), (x0, y1, zb), (x0, y1, za), (x0, y0, za), mat), (0, 0.1, 0, 5.0), (0, 0, 0.1, 5.0)))
    for k, mat in enumerate((9, 10, 12)):  # right wall: u along y, v along z
        za, zb = zs[k], zs[k + 1]
        meshes.append(_planar(quad((x1, y0, zb), (x1, y1, zb), (x1, y1, za), (x1, y0, za), mat),
                              (0, 0.5, 0, 0.5), (0, 0, 1.5 / (zb - za), -0.25 - 1.5 * za / (zb - za))))
    meshes.append(_planar(quad((x0, y0, zs[3]), (x1, y0, zs[3]), (x1, y1, zs[3]), (x0, y1, zs[3]), 2), (-0.4, 0, 0, 0.5), (0, 0.5, 0, 0.6)))
    meshes.append(_planar(quad((x0, y0, zs[0]), (x0, y1, zs[0]), (x1, y1, zs[0]), (x1, y0, zs[0]), 3), (0.55, 0, 0, 0.3), (0, 0.5, 0, 0.4)))
    c, r = np.array([0.9, -0.4, -3.6]), scenes.camera_matrix(35.0, 25.0).reshape(3, 3).astype(np.float64)
    pts = [c + r @ np.array(p) for p in ((-0.6, -0.5, 0), (0.6, -0.5, 0), (0.6, 0.5, 0), (-0.6, 0.5, 0))]
    meshes.append(quad(*pts, 8))  # no uvs: texel (row 12, column 0) of the 17x13 bitmap
    meshes.append(_planar(box((-1.1, -1.5, -3.4), (-0.4, -0.8, -2.7), 8), (0.9, 0, 0.4, 2.3), (0, 1.1, 0.3, 2.4)))
    c = np.array([-0.2, -0.9, -2.0])
    pts = [c + r @ np.array(p) for p in ((-0.4, -0.3, 0), (0.4, -0.3, 0), (0.4, 0.3, 0), (-0.4, 0.3, 0))]
    meshes.append(_planar(quad(*pts, 14), (0.5, 0, 0, 0.5), (0, 0.5, 0, 0.5)))
    lights = [((-0.7, 1.2, -3.0), 40.0), ((1.6, 0.3, -4.8), 25.0)]
    sc = _sc(meshes, lights, mats, (0.0, 0.0, 1.5), scenes.camera_matrix(0.0, -5.0))
    sc["textures"] = [dict(t) for t in _TEXTURES]
    return sc


def scene_textured_glass(scenes):
    """scene_sphere's smooth glass icosphere over a 3-square checker floor (uvs from -1 to 2) in front of a 17x13 bitmap wall
    (u from -0.25 to 1.25, v up to 1.2), beside a mirror whose albedo is an albedo texture: textured surfaces are reached through
    refraction and after mirror bounces.  The glass names a texture too; it decides nothing (glass has no albedo term)."""
    floor, wall = _backdrop(0, 1)
    _planar(floor, (0.25, 0, 0, 0.5), (0, 0, 0.2, 1.0))
    _planar(wall, (0.125, 0, 0, 0.5), (0, 0.2, 0, 0.2))
    mirror = _planar(quad((-2.4, -1, -1.0), (-1.6, -1, -4.0), (-1.6, 1.5, -4.0), (-2.4, 1.5, -1.0), 3), (0, 0, 0.3, 1), (0, 0.4, 0, 0.4))
    meshes = [floor, wall, icosphere(scenes, (0.0, -0.1, -2.6), 0.8, 1, 2), mirror]
    mats = [dict(m) for m in _GLASS_MATS]
    mats[0]["texture"], mats[1]["texture"] = 0, 1
    mats[2].update(smooth_shading=True, texture=0)
    mats.append({"albedo": (0.5, 0.5, 0.5), "type": REFLECTIVE, "texture": 2})
    sc = _sc(meshes, _GLASS_LIGHTS, mats, (0.0, 0.2, 0.4), scenes.camera_matrix(0.0, -4.0))
    sc["textures"] = [dict(_TEXTURES[1]), dict(_TEXTURES[8]), {"type": "albedo", "color_a": (0.9, 0.7, 0.8)}]
    return sc


SCENES = {"room": scene_room, "mirrors": scene_mirrors, "slab": scene_slab, "prism": scene_prism, "sphere": scene_sphere,
          "textured_room": scene_textured_room, "textured_glass": scene_textured_glass}
MISS_RGB = (0.2, 0.35, 0.5)
