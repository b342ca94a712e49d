"""Float64 restatement of the mode-150 contract (include/crt_hip.h, "Whitted shading"), for the tests only.  It is written over
path_reference.Scene -- the brute-force closest hit, the surface, the albedo, the direct light with its Phong term -- and shares
no arithmetic with the kernels.  The decision margins are path_reference.MARGINS: a record is flagged (robust False) when one
of its decisions, on any segment, falls below them, and the tests skip it and bound the share of such records.

A record carries a throughput T = (1, 1, 1) and a turn count k = 0.  At the end of a segment: a miss gives the miss colour
(times T after a turn); REFLECTIVE and REFRACTIVE turn the record as the mode-200 path turns, or end it black after max_bounces
turns; CONSTANT gives T x albedo; anything else is shaded as mode 100 shades: the direct light with Phong's view vector minus
the segment's direction, times T after a turn."""
import math
from collections import Counter

import numpy as np

import path_reference as R

# how a record ended
END_MISS, END_CONSTANT, END_CUT, END_LIT, END_SHADOWED, END_DARK = range(6)


def trace(S, o, d, miss, max_bounces, ks=0.0, exponent=32, tmin=R.RAY_TMIN, tmax=R.RAY_TMAX):
    """n records (o, d) over (tmin, tmax).  Returns a dict of flat arrays: rgb (n, 3), robust, segments (closest-hit rays of the
    record), turns, end (END_*; a lit surface counts as END_SHADOWED when an occluder took a light that faces it, as END_DARK
    when no light faces it), inst / prim / t of segment 0's hit, and ev, a Counter of what the records did."""
    n = len(o)
    o, d = np.array(o, np.float64), np.array(d, np.float64)
    miss = np.float32(miss).astype(np.float64)
    rgb, T = np.zeros((n, 3)), np.ones((n, 3))
    robust = np.ones(n, bool)
    segs, turns, end = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1)
    inst0, prim0, t0 = np.full(n, R.MISS, np.uint32), np.full(n, R.MISS, np.uint32), np.full(n, float(tmax))
    ev = Counter()
    alive = np.arange(n)
    for k in range(max_bounces + 1):
        if len(alive) == 0:
            break
        segs[alive] += 1
        turns[alive] = k
        if k == 0:
            hit, tri, t, u, v, rb = S.closest(o[alive], d[alive], tmin, tmax)
        else:
            hit, tri, t, u, v, rb = S.closest(o[alive], d[alive], 0.0)
        robust[alive] &= rb
        if k == 0:
            inst0[alive[hit]] = S.inst[tri[hit]]
            prim0[alive[hit]] = S.prim[tri[hit]]
            t0[alive[hit]] = t[hit]
        ms = alive[~hit]
        rgb[ms] = miss[None] if k == 0 else T[ms] * miss
        end[ms] = END_MISS
        ev["miss_direct" if k == 0 else "miss_after_turn"] += len(ms)
        alive, tri, t, u, v = alive[hit], tri[hit], t[hit], u[hit], v[hit]
        if len(alive) == 0:
            break
        P, N, entering, rb = S.surface(o[alive], d[alive], tri, t, u, v)
        robust[alive] &= rb
        mt = S.mtype[tri]
        alb, rb = S.albedo_at(tri, u, v, ev, after_bounce=k > 0)
        robust[alive] &= rb
        nxt_o, nxt_d = np.zeros((len(alive), 3)), np.zeros((len(alive), 3))
        goes = np.zeros(len(alive), bool)
        cut = k == max_bounces

        m = mt == R.CONSTANT
        rgb[alive[m]] = T[alive[m]] * alb[m]
        end[alive[m]] = END_CONSTANT
        ev["emit_direct" if k == 0 else "emit_after_turn"] += int(m.sum())

        m = mt == R.REFLECTIVE
        ev["mirror_cut" if cut else "mirror"] += int(m.sum())
        if cut:
            end[alive[m]] = END_CUT
        elif m.any():
            dd = d[alive[m]]
            kk = 2.0 * R._dot(dd, N[m])
            nxt_d[m] = R._norm(dd - kk[:, None] * N[m])
            nxt_o[m] = P[m] + N[m] * R.BIAS
            T[alive[m]] *= alb[m]
            goes |= m

        m = mt == R.REFRACTIVE
        ev["refract_cut" if cut else "refract"] += int(m.sum())
        if cut:
            end[alive[m]] = END_CUT
        elif m.any():
            dd, Nm = d[alive[m]], N[m]
            eta = np.where(entering[m], 1.0 / S.ior[tri[m]], S.ior[tri[m]])
            cosi = -R._dot(dd, Nm)
            kq = 1.0 - eta * eta * (1.0 - cosi * cosi)
            robust[alive[m]] &= np.abs(kq) >= R.MARGINS["snell_k"]
            tir = kq < 0.0
            refl = dd - (2.0 * R._dot(dd, Nm))[:, None] * Nm
            trans = eta[:, None] * dd + (eta * cosi - np.sqrt(np.maximum(kq, 0.0)))[:, None] * Nm
            nxt_d[m] = R._norm(np.where(tir[:, None], refl, trans))
            nxt_o[m] = P[m] + Nm * np.where(tir, R.BIAS, -R.BIAS)[:, None]
            ev["tir"] += int(tir.sum())
            ev["enter"] += int(np.sum(~tir & entering[m]))
            ev["exit"] += int(np.sum(~tir & ~entering[m]))
            goes |= m

        m = (mt != R.CONSTANT) & (mt != R.REFLECTIVE) & (mt != R.REFRACTIVE)
        if m.any():
            am = alive[m]
            Po = P[m] + N[m] * R.BIAS
            evd = Counter()
            L, rb = S.direct(Po, N[m], alb[m], evd, view=-d[am], ks=ks, exponent=exponent)
            robust[am] &= rb
            rgb[am] = L if k == 0 else T[am] * L
            # the same sums without occluders and without the Phong term: which records lost a light to a shadow
            lam, _ = S.direct(Po, N[m], alb[m], Counter()) if ks > 0.0 else (L, None)
            clear, facing = np.zeros_like(Po), np.zeros(len(Po), bool)
            for lp, inten in S.lights:
                Lv = lp[None] - Po
                r2 = R._dot(Lv, Lv)
                c = R._dot(N[m], Lv / np.sqrt(r2)[:, None])
                clear += alb[m] * np.where(c > 0.0, inten / (4.0 * math.pi * r2) * np.maximum(c, 0.0), 0.0)[:, None]
                facing |= c > 0.0
            shadowed = np.any(lam != clear, axis=1)
            end[am] = np.where(shadowed, END_SHADOWED, np.where(facing, END_LIT, END_DARK))
            after = "" if k == 0 else "_after_turn"
            for name in ("lit", "shadowed", "light_behind"):
                ev[name + after] += evd[name]
            ev["diffuse" + after] += int(m.sum())
        o[alive[goes]] = nxt_o[goes]
        d[alive[goes]] = nxt_d[goes]
        alive = alive[goes]
    assert np.all(end >= 0)
    return {"rgb": rgb, "robust": robust, "segments": segs, "turns": turns, "end": end, "inst": inst0, "prim": prim0, "t": t0, "ev": ev}


def centres(S, cam_pos, cam_rot, w, h, miss, max_bounces, ks=0.0, exponent=32):
    """trace() of the pixel-centre camera rays of a w x h frame, the arrays shaped (h, w[, 3])"""
    n = w * h
    pix = np.arange(n)
    o = np.repeat(np.float32(cam_pos).astype(np.float64)[None], n, axis=0)
    d = R.camera_dirs(cam_rot, pix % w, pix // w, 0.5, 0.5, w, h)
    out = trace(S, o, d, miss, max_bounces, ks, exponent)
    return {k: (a if k == "ev" else a.reshape((h, w) + a.shape[1:])) for k, a in out.items()}


def specular_only(sc):
    """a copy of the scene dict in which every material that is neither REFLECTIVE nor REFRACTIVE is an untextured white
    CONSTANT: a path through it is its specular chain and nothing else"""
    out = dict(sc)
    out["materials"] = [dict(m) if int(m.get("type", 1)) in (R.REFLECTIVE, R.REFRACTIVE) else {"albedo": (1.0, 1.0, 1.0), "type": R.CONSTANT}
                        for m in sc["materials"]]
    return out
