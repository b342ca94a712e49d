"""Reference of the variance-guided a-trous filter (crt_denoise_variance*, include/crt_hip.h, "variance") in numpy, written from
the contract's formulas alone, in the manner of tests/denoise_reference.py: every pass is 9 + 25 shifted-array terms.  `dtype`
selects the arithmetic: float64 is the reference, float32 the yardstick for what rounding alone costs."""
import numpy as np

from denoise_reference import H5, _shifted, live_mask as guide_live_mask

K3 = (0.25, 0.5, 0.25)
DEFAULTS = {"iterations": 5, "sigma_luminance": 0.0625, "sigma_normal": 0.3, "sigma_depth": 0.05, "demodulate": 1}
LUMA = (0.2126, 0.7152, 0.0722)


def live_mask(rgb, normal, albedo, t, variance):
    """(h, w) bool: crt_denoise's rule, and the variance finite and >= 0"""
    v = np.asarray(variance)
    with np.errstate(invalid="ignore"):
        return guide_live_mask(np.asarray(rgb), np.asarray(normal), np.asarray(albedo), np.asarray(t)) & np.isfinite(v) & (v >= 0)


def luminance(c):
    T = c.dtype.type
    return T(LUMA[0]) * c[..., 0] + T(LUMA[1]) * c[..., 1] + T(LUMA[2]) * c[..., 2]


def denoise_variance(rgb, normal, albedo, t, variance, iterations=5, sigma_luminance=0.0625, sigma_normal=0.3, sigma_depth=0.05, demodulate=1,
                     dtype=np.float64, weights=None):
    """(out (h, w, 3), variance_out (h, w)) of `dtype`: the filter of the contract.  Pixels that are not live come back as they
    went in (their bits, when dtype is float32).  weights: None, or a list that receives per pass the (h, w) sum of the weights
    of the taps other than the centre (a debug return)."""
    T = np.dtype(dtype).type
    src, vsrc = np.asarray(rgb), np.asarray(variance)
    live = live_mask(rgb, normal, albedo, t, variance)
    L3 = live[:, :, None]
    # everything that is not live is replaced by harmless values: it never takes part
    c_in = np.where(L3, rgb, 0).astype(dtype)
    n = np.where(L3, normal, 0).astype(dtype)
    z = np.where(live, t, 1).astype(dtype)
    v = np.where(live, variance, 0).astype(dtype)
    a = np.maximum(np.where(L3, albedo, 1).astype(dtype), T(1e-3)) if demodulate else np.ones_like(c_in)
    c = c_in / a
    inv_n2 = T(1.0) / (T(sigma_normal) * T(sigma_normal))
    inv_z = T(1.0) / (T(sigma_depth) * z)
    for i in range(iterations):
        s = 1 << i
        # g_p: the 3 x 3 mean of the variance at stride 1
        gs = np.zeros(v.shape, dtype=dtype)
        gk = np.zeros(v.shape, dtype=dtype)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                vq, inside = _shifted(v, dx, dy)
                lq, _ = _shifted(live, dx, dy, fill=False)
                k = np.where(inside & lq & live, T(K3[dx + 1]) * T(K3[dy + 1]), T(0)).astype(dtype)
                gs += k * vq
                gk += k
        g = gs / np.where(live, gk, 1)
        if np.isinf(sigma_luminance):
            inv_d = np.zeros(v.shape, dtype=dtype)
        else:
            inv_d = T(1.0) / (T(sigma_luminance) * np.sqrt(g) + T(1e-4))
        lum = luminance(c)
        num = np.zeros_like(c)
        den = np.zeros(v.shape, dtype=dtype)
        vnum = np.zeros(v.shape, dtype=dtype)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, inside = _shifted(c, s * dx, s * dy)
                nq, _ = _shifted(n, s * dx, s * dy)
                zq, _ = _shifted(z, s * dx, s * dy, fill=1)
                vq, _ = _shifted(v, s * dx, s * dy)
                lq, _ = _shifted(live, s * dx, s * dy, fill=False)
                ok = inside & lq & live
                dn, dz = n - nq, (z - zq) * inv_z
                e = np.abs(lum - luminance(cq)) * inv_d + (dn * dn).sum(axis=2) * inv_n2 + dz * dz
                wgt = np.where(ok, T(H5[dx + 2]) * T(H5[dy + 2]) * np.exp(-e), T(0)).astype(dtype)
                num += wgt[:, :, None] * cq
                vnum += wgt * wgt * vq
                den += wgt
        if weights is not None:
            weights.append(np.where(live, den - T(H5[2] * H5[2]), 0))
        safe = np.where(live, den, 1)
        c = np.where(L3, num / safe[:, :, None], c)
        v = np.where(live, vnum / (safe * safe), v)
    out = (c * a).astype(dtype)
    return np.where(L3, out, src.astype(dtype)), np.where(live, v, vsrc.astype(dtype))
