#!/usr/bin/env python3
"""Shaded ray queries (crt_shade_rays_device) in mode 100 on the C3 workload (BASELINE.json configs[2]: scenes.heightfield(),
1 002 530 triangles, its camera and light, 1920x1080).  Ray sets, all seeded:
  camera     the frame's 2 073 600 camera rays (numpy, not bit-exact to the kernel's), row-major
  shuffled   the same rays in a random order
  random     2^21 rays from points of the scene's box (widened by a tenth) towards other points of it
For every set three legs: `shade` (crt_shade_rays_device, rgb + normal + albedo + hit outputs), and the composition a caller has
without it, minus its own shading: `trace` (crt_trace_rays_device) and `occluded` (crt_occluded_rays_device) on the same rays.
`frame_mode100` is the frame kernel on the same context and view: the yardstick of the camera set.
Every figure is the call's own kernel_ms (HIP events around the kernel, crt_frame_stats); legs alternate in order round by
round; per leg the median and the spread (min, max) over rounds x calls.  Prints one JSON object (and writes it to --out).

  python tools/shade_rays_bench.py [--calls 5] [--warmup 2] [--rounds 4] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ray_query_bench import camera_dirs  # noqa: E402  (tools/ is the script directory)


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
    W, H = 1920, 1080
    sc = scenes.heightfield()
    cam = sc["camera"]
    r = pkg.Renderer(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    r.set_camera(cam["position"], cam["matrix"])
    r.change_shading_mode(100)
    rng = np.random.default_rng(1234)
    verts = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    ext = hi - lo

    cam_rays = pkg.make_rays(np.asarray(cam["position"], dtype=np.float32), camera_dirs(cam["matrix"], W, H), tmin=0.001, tmax=10000.0)
    n_rand = 1 << 21
    o = lo - 0.1 * ext + rng.random((n_rand, 3)) * 1.2 * ext
    d = lo + rng.random((n_rand, 3)) * ext - o
    rand_rays = pkg.make_rays(o.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32), tmin=0.001, tmax=np.inf)
    sets = {"camera": cam_rays, "shuffled": np.ascontiguousarray(cam_rays[rng.permutation(len(cam_rays))]), "random": rand_rays}
    dev = {k: torch.from_numpy(v).cuda() for k, v in sets.items()}
    nmax = max(len(v) for v in sets.values())
    d_rgb, d_nrm, d_alb = (torch.empty((nmax, 3), dtype=torch.float32, device="cuda") for _ in range(3))
    d_t = torch.empty(nmax, dtype=torch.float32, device="cuda")
    d_uv = torch.empty((nmax, 2), dtype=torch.float32, device="cuda")
    d_inst = torch.empty(nmax, dtype=torch.int32, device="cuda")
    d_prim = torch.empty(nmax, dtype=torch.int32, device="cuda")
    d_occ = torch.empty(nmax, dtype=torch.bool, device="cuda")
    frame = torch.empty(W * H, dtype=torch.int32, device="cuda")

    def call(name):
        if name == "frame_mode100":
            return r.render_frame_device(W, H, frame.data_ptr(), stats=True)["kernel_ms"]
        src, what = name.split("_")
        n, p = len(sets[src]), dev[src].data_ptr()
        if what == "shade":
            st = r.shade_rays_device(n, p, d_rgb.data_ptr(), d_nrm.data_ptr(), d_alb.data_ptr(), d_t.data_ptr(), d_uv.data_ptr(),
                                     d_inst.data_ptr(), d_prim.data_ptr(), stats=True)
        elif what == "trace":
            st = r.trace_rays_device(n, p, d_t.data_ptr(), d_uv.data_ptr(), d_inst.data_ptr(), d_prim.data_ptr(), stats=True)
        else:
            st = r.occluded_device(n, p, d_occ.data_ptr(), stats=True)
        return st["kernel_ms"]

    names = ["frame_mode100"] + ["%s_%s" % (s, w) for s in sets for w in ("shade", "trace", "occluded")]
    ms = {k: [] for k in names}
    for i in range(a.rounds):
        for k in (names if i % 2 == 0 else names[::-1]):  # alternate the order: no leg always follows the same one
            for _ in range(a.warmup):
                call(k)
            ms[k] += [call(k) for _ in range(a.calls)]

    # what the rays meet: hits, and shadow rays per record (counting variant, one call per set)
    r.set_counting(True)
    mix = {}
    for s in sets:
        st = r.shade_rays_device(len(sets[s]), dev[s].data_ptr(), d_rgb.data_ptr(), d_inst=d_inst.data_ptr(), stats=True)
        hits = int((d_inst[:len(sets[s])] != -1).sum().item())
        mix[s] = {"rays": len(sets[s]), "hit_fraction": hits / len(sets[s]), "shadow_rays": st["rays_shadow"]}
    r.set_counting(False)
    r.close()

    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"workload": "C3: heightfield 708x708 quads + ground (1 002 530 triangles), 1 light, 1920x1080 camera, mode 100",
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "sets": mix, "median_ms": med,
           "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
           "trace_plus_occluded_ms": {s: med[s + "_trace"] + med[s + "_occluded"] for s in sets},
           "shade_over_trace_plus_occluded": {s: med[s + "_shade"] / (med[s + "_trace"] + med[s + "_occluded"]) for s in sets},
           "camera_shade_over_frame": med["camera_shade"] / med["frame_mode100"],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
