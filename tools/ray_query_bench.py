#!/usr/bin/env python3
"""Batched ray queries (crt_trace_rays_device / crt_occluded_rays_device) on the C3 workload (BASELINE.json configs[2]:
scenes.heightfield(), 1 002 530 triangles, its camera, 1920x1080).  Legs, all seeded, alternating in order round by round:
  camera_rowmajor   the frame's 2 073 600 camera rays (numpy, not bit-exact to the kernel's), row-major, closest hit
  camera_8x8        the same rays in 8x8-block order (the render kernel's packet), closest hit
  frame_mode3       the mode-3 frame (primary rays only) that traces the same rays, for comparison
  ao_closest / ao_occluded   4 cosine-weighted hemisphere rays per primary hit, tmin 1e-3, tmax 2 % of the scene diagonal
  random_closest / random_occluded   2^22 rays, origins uniform in the scene box, directions uniform on the sphere, tmax inf
Each leg is issued back to back on one stream after a warm-up and timed with HIP events; ms per call = events / calls.
Prints one JSON object (and writes it to --out when given).

  python tools/ray_query_bench.py [--calls 10] [--warmup 3] [--rounds 4] [--legs a,b,...] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_dirs(rot, w, h):
    """the rayGen direction of every pixel centre (the kernel's formula in float32 numpy; fma and rounding may differ)"""
    x = (np.arange(w, dtype=np.float32) + np.float32(0.5)) / np.float32(w)
    y = (np.arange(h, dtype=np.float32) + np.float32(0.5)) / np.float32(h)
    x = (np.float32(2.0) * x - np.float32(1.0)) * np.float32(w / h)
    y = np.float32(1.0) - np.float32(2.0) * y
    X, Y = np.meshgrid(x, y)
    dc = np.stack([X, Y, -np.ones_like(X)], axis=-1).reshape(-1, 3)
    dc /= np.linalg.norm(dc, axis=1, keepdims=True)
    dw = dc @ np.asarray(rot, dtype=np.float32).reshape(3, 3).T
    return (dw / np.linalg.norm(dw, axis=1, keepdims=True)).astype(np.float32)


def block_order(w, h, b=8):
    """pixel indices in b x b-block order (blocks row-major, pixels row-major inside a block)"""
    y, x = np.divmod(np.arange(w * h), w)
    key = ((y // b) * ((w + b - 1) // b) + x // b) * (b * b) + (y % b) * b + (x % b)
    return np.argsort(key, kind="stable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="timed calls per leg and round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls before each leg's timed calls")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--legs", default=None, help="comma-separated subset of the legs (default: all)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as e
    pkg = e.load_package()
    scenes = importlib.import_module(e.PKG_NAME + ".scenes")
    W, H = 1920, 1080
    sc = scenes.heightfield()
    cam = sc["camera"]
    r = pkg.Renderer(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    r.set_camera(cam["position"], cam["matrix"])
    r.change_shading_mode(3)
    rng = np.random.default_rng(1234)
    verts = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))

    # camera rays, and the primary hits the AO rays start from (found by the query itself, closest hit)
    cam_rays = pkg.make_rays(np.asarray(cam["position"], dtype=np.float32), camera_dirs(cam["matrix"], W, H), tmin=0.001, tmax=10000.0)
    prim = r.trace_rays(cam_rays)
    hit = prim["inst"] != pkg.MISS
    tris = []
    for m in sc["meshes"]:
        v = np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3)
        t = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)
        tris.append((v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]))
    P = cam_rays[hit, 0:3] + cam_rays[hit, 4:7] * prim["t"][hit, None]
    N = np.zeros_like(P)
    for i, (v0, v1, v2) in enumerate(tris):
        sel = prim["inst"][hit] == i
        k = prim["prim"][hit][sel]
        n = np.cross(v1[k] - v0[k], v2[k] - v0[k])
        N[sel] = n / np.linalg.norm(n, axis=1, keepdims=True)
    N *= -np.sign(np.sum(N * cam_rays[hit, 4:7], axis=1, keepdims=True))  # facing the camera
    N = np.repeat(N, 4, axis=0)
    P = np.repeat(P, 4, axis=0)
    u1, u2 = rng.random(len(N)), rng.random(len(N))
    rr, ph = np.sqrt(u1), 2 * np.pi * u2
    lx, ly, lz = rr * np.cos(ph), rr * np.sin(ph), np.sqrt(1 - u1)  # cosine-weighted around +z
    helper = np.where(np.abs(N[:, 0:1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    T = np.cross(helper, N)
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    B = np.cross(N, T)
    ao_dirs = (T * lx[:, None] + B * ly[:, None] + N * lz[:, None]).astype(np.float32)
    ao_rays = pkg.make_rays(P.astype(np.float32), ao_dirs, tmin=1e-3, tmax=0.02 * diag)
    n_rand = 1 << 22
    d = rng.normal(size=(n_rand, 3))
    rand_rays = pkg.make_rays((lo + rng.random((n_rand, 3)) * (hi - lo)).astype(np.float32),
                              (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32), tmin=0.0, tmax=np.inf)

    sets = {"camera_rowmajor": cam_rays, "camera_8x8": np.ascontiguousarray(cam_rays[block_order(W, H)]), "ao": ao_rays, "random": rand_rays}
    dev = {k: torch.from_numpy(v).cuda() for k, v in sets.items()}
    nmax = max(len(v) for v in sets.values())
    d_t = torch.empty(nmax, dtype=torch.float32, device="cuda")
    d_uv = torch.empty((nmax, 2), dtype=torch.float32, device="cuda")
    d_inst = torch.empty(nmax, dtype=torch.int32, device="cuda")
    d_prim = torch.empty(nmax, dtype=torch.int32, device="cuda")
    d_occ = torch.empty(nmax, dtype=torch.bool, device="cuda")
    frame = torch.empty(W * H, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    r.set_stream(stream.cuda_stream)

    legs = {
        "camera_rowmajor": ("camera_rowmajor", False), "camera_8x8": ("camera_8x8", False), "frame_mode3": (None, False),
        "ao_closest": ("ao", False), "ao_occluded": ("ao", True), "random_closest": ("random", False), "random_occluded": ("random", True),
    }
    names = a.legs.split(",") if a.legs else list(legs)

    def call(name):
        src, occl = legs[name]
        if src is None:
            r.render_frame_device(W, H, frame.data_ptr())
            return
        n, p = len(sets[src]), dev[src].data_ptr()
        if occl:
            r.occluded_device(n, p, d_occ.data_ptr())
        else:
            r.trace_rays_device(n, p, d_t.data_ptr(), d_uv.data_ptr(), d_inst.data_ptr(), d_prim.data_ptr())

    def leg(name):
        for _ in range(a.warmup):
            call(name)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(a.calls):
            call(name)
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) / a.calls

    ms = {k: [] for k in names}
    for i in range(a.rounds):
        for k in (names if i % 2 == 0 else names[::-1]):  # alternate the order: no leg always follows the same one
            ms[k].append(leg(k))
    r.reset_stream()
    r.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    rays = {k: (len(sets[legs[k][0]]) if legs[k][0] else W * H) for k in names}
    out = {"workload": "C3: heightfield 708x708 quads + ground (1 002 530 triangles), 1920x1080 camera",
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "rays": rays, "ms": ms, "median_ms": med,
           "mray_per_s": {k: rays[k] / (med[k] * 1e3) for k in names},
           "primary_hit_fraction": float(hit.mean()), "ao_tmax": 0.02 * diag,
           "device": torch.cuda.get_device_name(0)}
    if "camera_8x8" in med and "frame_mode3" in med:
        out["camera_8x8_over_frame_mode3"] = med["camera_8x8"] / med["frame_mode3"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
