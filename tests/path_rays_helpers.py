"""Helpers of tests/test_path_rays.py: a frame's jittered camera rays as ray records.

ray_dir_j restates the kernels' rayDirJ / the oracle's ray_dir_j in float32: numpy float32 operations (each correctly rounded)
and fmaf done exactly -- the rational a * b + c rounded once to the nearest float32, ties to even.  With the jitter of the
spec's hash chain a record built here is the camera ray of pixel (px, py) of a mode-200 frame, bit for bit, so a w x h oracle
frame at 1 spp is the reference of w * h records and a 1 x 1 frame (pixel 0, id 0) that of one arbitrary ray."""
from fractions import Fraction

import numpy as np

TMIN, TMAX = 0.001, 10000.0
F32 = np.float32


def _round_f32(x):
    """the float32 nearest to the Fraction x, ties to even (x != 0, well inside the normal range)"""
    near = F32(float(x))  # within one float32 step of x: the float64 is correctly rounded, the cast at worst a double rounding
    best = None
    for c in (np.nextafter(near, F32(-np.inf)), near, np.nextafter(near, F32(np.inf))):
        err = abs(Fraction(float(c)) - x)
        even = (int(np.array(c, dtype=F32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, c)
    return best[1]


def fmaf(a, b, c):
    """a * b + c of three float32 values with one rounding"""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        return F32(np.float64(a) * np.float64(b) + np.float64(c))  # (the product is exact in float64: the sign of zero is right)
    return _round_f32(exact)


def dot3(a, b):
    return fmaf(a[2], b[2], fmaf(a[1], b[1], F32(a[0] * b[0])))


def normalize3(a):
    inv = F32(1.0) / np.sqrt(dot3(a, a))
    return np.array([a[0] * inv, a[1] * inv, a[2] * inv], dtype=F32)


def ray_dir_j(rot, px, py, jx, jy, w, h):
    rot = np.asarray(rot, dtype=F32).reshape(9)
    width, height = F32(w), F32(h)
    x, y = F32(px) + F32(jx), F32(py) + F32(jy)
    x, y = x / width, y / height
    x = F32(2.0) * x - F32(1.0)
    y = F32(1.0) - F32(2.0) * y
    x = x * (width / height)
    dc = normalize3(np.array([x, y, F32(-1.0)], dtype=F32))
    dw = np.array([dot3(rot[0:3], dc), dot3(rot[3:6], dc), dot3(rot[6:9], dc)], dtype=F32)
    return normalize3(dw)


def camera_records(pos, rot, w, h, jx, jy):
    """(w * h, 8) float32 records of a frame's camera rays with per-pixel jitter jx, jy (w * h each); record i is pixel i"""
    rays = np.empty((w * h, 8), dtype=F32)
    rays[:, 0:3] = np.asarray(pos, dtype=F32)
    rays[:, 3], rays[:, 7] = TMIN, TMAX
    for i in range(w * h):
        rays[i, 4:7] = ray_dir_j(rot, i % w, i // w, jx[i], jy[i], w, h)
    return rays


def reference_jitter(R, ids, sample, seed):
    """the two draws after the path's start, from tests/path_reference.py's hash chain, as float32"""
    ids = np.asarray(ids, dtype=np.uint32)
    st = R.rng_start(ids, np.full(len(ids), sample, np.uint32), seed)
    st, jx = R.rng_next(st)
    st, jy = R.rng_next(st)
    return jx.astype(F32), jy.astype(F32)


def frame_records(R, cam, w, h, sample, seed):
    """the records of a frame's camera rays of one sample (ids = pixel numbers)"""
    jx, jy = reference_jitter(R, np.arange(w * h), sample, seed)
    return camera_records(cam["position"], cam["matrix"], w, h, jx, jy)


def pose_records(R, pos, rot, seed, sample=0):
    """one record per pose: the sample's camera ray of the 1 x 1 frame at that pose (pixel 0, so id 0)"""
    jx, jy = reference_jitter(R, np.zeros(1, np.uint32), sample, seed)
    rays = np.empty((len(pos), 8), dtype=F32)
    for k in range(len(pos)):
        rays[k, 0:3], rays[k, 3], rays[k, 7] = pos[k], TMIN, TMAX
        rays[k, 4:7] = ray_dir_j(rot[k], 0, 0, jx[0], jy[0], 1, 1)
    return rays
