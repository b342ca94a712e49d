"""Float64 restatement of the mode-200 path spec (DESIGN.md section 3 "Path tracing", include/crt_hip.h CRT_MODE_PATH), for
the tests only.  It shares no arithmetic with the CPU oracle or the product: geometry is a brute-force closest hit over every
triangle, the RNG is the spec's integer hash chain on uint32, and every other quantity is float64.  Since it draws the same
random numbers as the kernels, a 1-spp pixel is one path, traced here without statistics.

Near a discontinuity (a ray grazing a triangle edge, two surfaces at nearly the same t, a shadow ray ending on an occluder,
a light at cos ~ 0, Snell's k ~ 0, a normal's z ~ 0 or a grazing hit) the float32 and float64 paths may legitimately take
different branches.  trace_paths records the margin of every such decision and flags the path when one falls below the
thresholds in MARGINS; the tests skip flagged paths and bound their share."""
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


class Scene:
    """the scene dict of the tests (meshes / lights / materials), flattened to per-triangle float64 arrays"""

    def __init__(self, sc):
        v0, e1, e2, inst, prim, mat, nrm = [], [], [], [], [], [], []
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
        self.v0, self.e1, self.e2 = np.concatenate(v0), np.concatenate(e1), np.concatenate(e2)
        self.inst, self.prim, self.nrm = np.concatenate(inst), np.concatenate(prim), np.concatenate(nrm)
        mats = list(sc["materials"])
        matidx = np.concatenate(mat)
        known = matidx < len(mats)  # a triangle without a material is white DIFFUSE
        self.albedo = np.ones((len(matidx), 3))
        self.mtype = np.full(len(matidx), DIFFUSE)
        self.smooth = np.zeros(len(matidx), bool)
        self.ior = np.ones(len(matidx))
        for k in range(len(matidx)):
            if known[k]:
                M = mats[matidx[k]]
                self.albedo[k] = np.float32(M.get("albedo", (1, 1, 1))).astype(np.float64)
                self.mtype[k] = int(M.get("type", 1))
                self.smooth[k] = bool(M.get("smooth_shading", False))
                self.ior[k] = float(np.float32(M.get("ior", 1.0)))
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
        alb = S.albedo[tri]
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


def shade_centres(S, cam_pos, cam_rot, w, h, mode, miss, ks=0.0, exponent=32):
    """modes 3 (barycentric), 5 (distance) and 100 (Lambert + Phong) at pixel centres, float64: (rgb, robust, inst, prim, t)"""
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
        c, rb = S.direct(P + N * BIAS, N, S.albedo[tri[hit]], Counter(), view=-d[hit], ks=ks, exponent=exponent)
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


SCENES = {"room": scene_room, "mirrors": scene_mirrors, "slab": scene_slab, "prism": scene_prism, "sphere": scene_sphere}
MISS_RGB = (0.2, 0.35, 0.5)
