"""Reference of the edge-avoiding a-trous denoiser (crt_denoise*, include/crt_hip.h) in numpy, written from the contract's
formulas alone: every pass is 25 shifted-array terms, so a 64 x 64 image takes well under a second.  `dtype` selects the
arithmetic: float64 is the reference, float32 the yardstick for what rounding alone costs.  Also the synthetic test image of
tests/test_denoise.py."""
import numpy as np

H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
DEFAULTS = {"iterations": 5, "sigma_color": 4.0, "sigma_normal": 0.3, "sigma_depth": 0.05, "demodulate": 1}


def live_mask(rgb, normal, albedo, t):
    """(h, w) bool: all 10 inputs finite, a non-zero normal component, t > 0"""
    fin = np.isfinite(rgb).all(axis=2) & np.isfinite(normal).all(axis=2) & np.isfinite(albedo).all(axis=2) & np.isfinite(t)
    with np.errstate(invalid="ignore"):
        return fin & (normal != 0).any(axis=2) & (t > 0)


def _shifted(a, ox, oy, fill=0):
    """b[y, x] = a[y + oy, x + ox] where that lies inside the image, `fill` elsewhere; and the inside mask"""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((h, w), dtype=bool)
    if abs(ox) >= w or abs(oy) >= h:
        return b, inside
    ys, yd = (slice(oy, h), slice(0, h - oy)) if oy >= 0 else (slice(0, h + oy), slice(-oy, h))
    xs, xd = (slice(ox, w), slice(0, w - ox)) if ox >= 0 else (slice(0, w + ox), slice(-ox, w))
    b[yd, xd] = a[ys, xs]
    inside[yd, xd] = True
    return b, inside


def denoise(rgb, normal, albedo, t, iterations=5, sigma_color=4.0, sigma_normal=0.3, sigma_depth=0.05, demodulate=1, dtype=np.float64):
    """(h, w, 3) array of `dtype`: the filter of the contract.  Pixels that are not live come back as they went in (their bits,
    when dtype is float32)."""
    T = np.dtype(dtype).type
    src = np.asarray(rgb)
    live = live_mask(np.asarray(rgb), np.asarray(normal), np.asarray(albedo), np.asarray(t))
    L3 = live[:, :, None]
    # everything that is not live is replaced by harmless values: it never takes part
    c_in = np.where(L3, rgb, 0).astype(dtype)
    n = np.where(L3, normal, 0).astype(dtype)
    z = np.where(live, t, 1).astype(dtype)
    a = np.maximum(np.where(L3, albedo, 1).astype(dtype), T(1e-3)) if demodulate else np.ones_like(c_in)
    c = c_in / a
    inv_n2 = T(1.0) / (T(sigma_normal) * T(sigma_normal))
    inv_z2 = T(1.0) / ((T(sigma_depth) * z) * (T(sigma_depth) * z))
    for i in range(iterations):
        s = 1 << i
        sc = T(sigma_color) * T(2.0 ** -i)
        inv_c2 = T(1.0) / (sc * sc)
        num = np.zeros_like(c)
        den = np.zeros(c.shape[:2], dtype=dtype)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, inside = _shifted(c, s * dx, s * dy)
                nq, _ = _shifted(n, s * dx, s * dy)
                zq, _ = _shifted(z, s * dx, s * dy, fill=1)
                lq, _ = _shifted(live, s * dx, s * dy, fill=False)
                ok = inside & lq & live
                dc, dn, dz = c - cq, n - nq, z - zq
                e = (dc * dc).sum(axis=2) * inv_c2 + (dn * dn).sum(axis=2) * inv_n2 + dz * dz * inv_z2
                wgt = np.where(ok, T(H5[dx + 2]) * T(H5[dy + 2]) * np.exp(-e), T(0)).astype(dtype)
                num += wgt[:, :, None] * cq
                den += wgt
        c = np.where(L3, num / np.where(live, den, 1)[:, :, None], c)
    out = (c * a).astype(dtype)
    return np.where(L3, out, src.astype(dtype))


def deviation(x, ref64):
    """the metric of every comparison: |x - ref64| / max(|ref64|, 1e-3), elementwise (float64)"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    return np.abs(np.asarray(x, dtype=np.float64) - ref64) / np.maximum(np.abs(ref64), 1e-3)


def synthetic(w, h, edge=None, miss_at=None, seed=7):
    """The synthetic scene: two planes meeting at the vertical edge in column `edge` (default round(0.55 w)): normal (0, 0.6, 0.8)
    left, (0.8, 0, 0.6) right; t = 3 + 0.02 x + 0.01 y, plus 1.5 on the right; albedo a 4-pixel checker of (0.8, 0.2, 0.2) and
    (0.2, 0.7, 0.9); irradiance 1.0 left, 0.4 right; colour = albedo x irradiance x Gamma(4, 0.25) noise, one draw per pixel
    from default_rng(seed); a 3 x 2 block of miss pixels (normal 0, albedo 0, t 10000, colour (0, 1, 1)) with its corner at
    miss_at = (x, y) where it fits.  Returns float32 arrays and the clean image."""
    edge = int(round(0.55 * w)) if edge is None else edge
    y, x = np.mgrid[0:h, 0:w]
    right = x >= edge
    normal = np.where(right[:, :, None], np.float32([0.8, 0.0, 0.6]), np.float32([0.0, 0.6, 0.8])).astype(np.float32)
    t = (3.0 + 0.02 * x + 0.01 * y + np.where(right, 1.5, 0.0)).astype(np.float32)
    checker = ((x // 4 + y // 4) & 1).astype(bool)
    albedo = np.where(checker[:, :, None], np.float32([0.2, 0.7, 0.9]), np.float32([0.8, 0.2, 0.2])).astype(np.float32)
    irradiance = np.where(right, 0.4, 1.0)
    noise = np.random.default_rng(seed).gamma(4.0, 0.25, size=(h, w))
    clean = (albedo * irradiance[:, :, None]).astype(np.float32)
    rgb = (albedo * (irradiance * noise)[:, :, None]).astype(np.float32)
    miss = np.zeros((h, w), dtype=bool)
    if miss_at is None:
        miss_at = (min(5, max(w - 3, 0)), min(3, max(h - 2, 0)))
    mx, my = miss_at
    if w >= mx + 3 and h >= my + 2 and w * h > 6:
        miss[my:my + 2, mx:mx + 3] = True
        normal[miss] = 0.0
        albedo[miss] = 0.0
        t[miss] = 10000.0
        rgb[miss] = np.float32([0.0, 1.0, 1.0])
        clean[miss] = np.float32([0.0, 1.0, 1.0])
    return {"rgb": rgb, "normal": normal, "albedo": albedo, "t": t, "clean": clean, "miss": miss, "edge": edge, "right": right}
