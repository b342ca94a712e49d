#!/usr/bin/env python3
"""Path-traced ray queries (crt_path_rays_device) on the C3 workload (BASELINE.json configs[2]: scenes.heightfield(),
1 002 530 triangles, its camera and light, 1920x1080) with max_bounces 3, one sample per record.  Ray sets, all seeded:
  camera     the frame's 2 073 600 sample-0 camera rays (jitter from path_jitter; the directions in numpy, not bit-exact to
             the kernel's), row-major, ids = pixel numbers
  shuffled   the same rays and ids in a random order
  random     2^21 rays from points of the scene's box (widened by a tenth) towards other points of it, ids = record numbers
`frame_mode200` is the mode-200 frame at 1 spp on the same context and view: the yardstick of the camera set (tile-private
queues, compaction between the stages, octant-specialised camera rays).
Every figure is the call's own kernel_ms (HIP events around all kernels of the call, crt_frame_stats); legs alternate in order
round by round; per leg the median and the spread (min, max) over rounds x calls.  Prints one JSON object (and writes it to
--out).

  python tools/path_rays_bench.py [--calls 5] [--warmup 2] [--rounds 4] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def jittered_camera_dirs(rot, w, h, jx, jy):
    """rayDirJ of every pixel (the kernel's formula in float32 numpy; fma and rounding may differ)"""
    f = np.float32
    px, py = np.meshgrid(np.arange(w, dtype=f), np.arange(h, dtype=f))
    x = (px.reshape(-1) + jx) / f(w)
    y = (py.reshape(-1) + jy) / f(h)
    x = (f(2.0) * x - f(1.0)) * f(w / h)
    y = f(1.0) - f(2.0) * y
    dc = np.stack([x, y, -np.ones_like(x)], axis=-1)
    dc /= np.linalg.norm(dc, axis=1, keepdims=True)
    dw = dc @ np.asarray(rot, dtype=f).reshape(3, 3).T
    return (dw / np.linalg.norm(dw, axis=1, keepdims=True)).astype(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5, help="timed calls per leg and round")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls before each leg's timed calls")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as e
    pkg = e.load_package()
    scenes = importlib.import_module(e.PKG_NAME + ".scenes")
    W, H, SEED, BOUNCES = 1920, 1080, 1234, 3
    sc = scenes.heightfield()
    cam = sc["camera"]
    r = pkg.Renderer(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    r.set_camera(cam["position"], cam["matrix"])
    r.change_shading_mode(200)
    r.set_path_params(1, BOUNCES, SEED)
    rng = np.random.default_rng(1234)
    verts = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    ext = hi - lo

    pix = np.arange(W * H, dtype=np.uint32)
    jx, jy = pkg.path_jitter(pix, 0, SEED)
    cam_rays = pkg.make_rays(np.asarray(cam["position"], dtype=np.float32), jittered_camera_dirs(cam["matrix"], W, H, jx, jy), tmin=0.001, tmax=10000.0)
    n_rand = 1 << 21
    o = lo - 0.1 * ext + rng.random((n_rand, 3)) * 1.2 * ext
    d = lo + rng.random((n_rand, 3)) * ext - o
    rand_rays = pkg.make_rays(o.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32), tmin=0.001, tmax=np.inf)
    perm = rng.permutation(len(cam_rays))
    sets = {"camera": (cam_rays, pix), "shuffled": (np.ascontiguousarray(cam_rays[perm]), np.ascontiguousarray(pix[perm])),
            "random": (rand_rays, np.arange(n_rand, dtype=np.uint32))}
    dev = {k: (torch.from_numpy(v[0]).cuda(), torch.from_numpy(v[1].view(np.int32)).cuda()) for k, v in sets.items()}
    nmax = max(len(v[0]) for v in sets.values())
    d_rgb = torch.empty((nmax, 3), dtype=torch.float32, device="cuda")
    d_inst = torch.empty(nmax, dtype=torch.int32, device="cuda")
    frame = torch.empty(W * H, dtype=torch.int32, device="cuda")

    def call(name):
        if name == "frame_mode200":
            return r.render_frame_device(W, H, frame.data_ptr(), stats=True)["kernel_ms"]
        rays, ids = dev[name]
        return r.path_rays_device(len(rays), rays.data_ptr(), d_ids=ids.data_ptr(), d_rgb=d_rgb.data_ptr(), d_inst=d_inst.data_ptr(), stats=True)["kernel_ms"]

    names = ["frame_mode200"] + list(sets)
    ms = {k: [] for k in names}
    for i in range(a.rounds):
        for k in (names if i % 2 == 0 else names[::-1]):  # alternate the order: no leg always follows the same one
            for _ in range(a.warmup):
                call(k)
            ms[k] += [call(k) for _ in range(a.calls)]

    # what the rays meet: hits, closest-hit and shadow rays per record (counting variant, one call per set)
    r.set_counting(True)
    mix = {}
    for s in sets:
        rays, ids = dev[s]
        st = r.path_rays_device(len(rays), rays.data_ptr(), d_ids=ids.data_ptr(), d_rgb=d_rgb.data_ptr(), d_inst=d_inst.data_ptr(), stats=True)
        hits = int((d_inst[:len(rays)] != -1).sum().item())
        mix[s] = {"rays": len(rays), "hit_fraction": hits / len(rays), "closest_rays": st["rays_primary"], "shadow_rays": st["rays_shadow"]}
    fs = r.render_frame_device(W, H, frame.data_ptr(), stats=True)
    mix["frame_mode200"] = {"rays": W * H, "closest_rays": fs["rays_primary"], "shadow_rays": fs["rays_shadow"]}
    r.set_counting(False)
    r.close()

    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"workload": "C3: heightfield 708x708 quads + ground (1 002 530 triangles), 1 light, 1920x1080 camera, mode 200, 1 spp, max_bounces 3",
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "sets": mix, "median_ms": med,
           "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
           "camera_over_frame": med["camera"] / med["frame_mode200"],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
