#!/usr/bin/env python3
"""Gradients of the ray and closest-point queries (crt_trace_rays_backward_device, crt_closest_points_backward_device) on the C3
workload (BASELINE.json configs[2]: scenes.heightfield(), 1 002 530 triangles, its camera) uploaded as a dynamic scene, for the
1920x1080 pixel-centre camera rays (n = 2 073 600 records) and as many points half a unit above their hits.  Legs:
  trace_rays          the forward closest-hit query the ray backward follows
  rays_backward       grad_rays and grad_xyz: the record kernel with its nine float64 atomics per live record, the zeroing of the
                      sums before it and the rounding kernel behind it
  rays_records_only   grad_xyz = NULL: no atomics
  closest_points      the forward closest-point query
  points_backward     grad_points and grad_xyz
  copy_rays           a device-to-device copy that moves the ray backward's compulsory bytes per record: 64 B in (ray, inst, prim,
                      t, uv, grad_t, grad_uv), 32 B out; done as a copy of 48 B per record
  copy_points         the same for points: 36 B in, 16 B out, a copy of 26 B per record
and, on a scene of one triangle with 2^20 rays that all hit it (the worst contention: nine addresses take every atomic),
  one_trace_rays, one_rays_backward, one_rays_records_only
Every figure of a library call is the call's own kernel_ms (HIP events, crt_frame_stats); the copies are timed with HIP events
around torch's copy.  Legs alternate in order round by round; per leg the median and the spread (min, max) over rounds x calls.
No time is a pass condition.  Prints one JSON object (and writes it to --out).

  python tools/grad_bench.py [--calls 5] [--warmup 2] [--rounds 4] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def buffers(n, nv):
        return {"t": torch.empty(n, **f32), "uv": torch.empty((n, 2), **f32), "inst": torch.empty(n, **i32), "prim": torch.empty(n, **i32),
                "g_t": torch.randn(n, **f32), "g_uv": torch.randn((n, 2), **f32), "grad_rays": torch.empty((n, 8), **f32),
                "grad_xyz": torch.empty((nv, 3), **f32)}

    def ray_legs(r, n, d_rays, b, prefix=""):
        p = {k: v.data_ptr() for k, v in b.items()}
        return {
            prefix + "trace_rays": lambda: r.trace_rays_device(n, d_rays.data_ptr(), p["t"], p["uv"], p["inst"], p["prim"], stats=True)["kernel_ms"],
            prefix + "rays_backward": lambda: r.trace_rays_backward_device(n, d_rays.data_ptr(), p["inst"], p["prim"], p["t"], p["uv"], p["g_t"], p["g_uv"],
                                                                           p["grad_rays"], p["grad_xyz"], stats=True)["kernel_ms"],
            prefix + "rays_records_only": lambda: r.trace_rays_backward_device(n, d_rays.data_ptr(), p["inst"], p["prim"], p["t"], p["uv"], p["g_t"],
                                                                               p["g_uv"], p["grad_rays"], None, stats=True)["kernel_ms"]}

    def copy_leg(r, src, dst):
        def run():
            r.synchronize()
            ev0.record()
            dst.copy_(src)
            ev1.record()
            torch.cuda.synchronize()
            return ev0.elapsed_time(ev1)
        return run

    def measure(legs):
        names = list(legs)
        ms = {k: [] for k in names}
        for i in range(a.rounds):
            for k in (names if i % 2 == 0 else names[::-1]):  # alternate the order: no leg always follows the same one
                for _ in range(a.warmup):
                    legs[k]()
                ms[k] += [legs[k]() for _ in range(a.calls)]
        return {"median_ms": {k: statistics.median(v) for k, v in ms.items()}, "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()}}

    # ---- the C3 scene
    sc = scenes.heightfield()
    W, H = 1920, 1080
    n = W * H
    r = pkg.Renderer(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=True)
    r.set_camera(sc["camera"]["position"], np.asarray(sc["camera"]["matrix"], np.float32).reshape(9))
    nv = r._total_vertices()
    d_rays = torch.empty((n, 8), **f32)
    r.camera_rays_device(W, H, d_rays.data_ptr(), stats=True)
    b = buffers(n, nv)
    legs = ray_legs(r, n, d_rays, b)
    legs["trace_rays"]()
    hit = b["inst"] >= 0
    # points half a unit above the hits (misses: the ray origin), searched within 2 units
    d_pts = torch.empty((n, 4), **f32)
    d_pts[:, 0:3] = d_rays[:, 0:3] + d_rays[:, 4:7] * torch.where(hit, b["t"], torch.zeros_like(b["t"])).unsqueeze(1)
    d_pts[:, 1] += 0.5
    d_pts[:, 3] = 2.0
    pb = {"dist": torch.empty(n, **f32), "uv": torch.empty((n, 2), **f32), "inst": torch.empty(n, **i32), "prim": torch.empty(n, **i32),
          "grad_points": torch.empty((n, 4), **f32)}
    torch.cuda.synchronize()
    q = {k: v.data_ptr() for k, v in pb.items()}
    legs["closest_points"] = lambda: r.closest_points_device(n, d_pts.data_ptr(), q["dist"], None, q["uv"], q["inst"], q["prim"], stats=True)["kernel_ms"]
    legs["points_backward"] = lambda: r.closest_points_backward_device(n, d_pts.data_ptr(), q["inst"], q["prim"], q["uv"], b["g_t"].data_ptr(),
                                                                       q["grad_points"], b["grad_xyz"].data_ptr(), stats=True)["kernel_ms"]
    src48, dst48 = torch.empty(n * 48, dtype=torch.uint8, device="cuda"), torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    src26, dst26 = torch.empty(n * 26, dtype=torch.uint8, device="cuda"), torch.empty(n * 26, dtype=torch.uint8, device="cuda")
    legs["copy_rays"] = copy_leg(r, src48, dst48)
    legs["copy_points"] = copy_leg(r, src26, dst26)
    legs["closest_points"]()
    big = measure(legs)
    med = big["median_ms"]
    big.update(records=n, vertices=nv, hit_fraction=float(hit.float().mean().item()), point_hit_fraction=float((pb["inst"] >= 0).float().mean().item()),
               rays_backward_over_trace_rays=med["rays_backward"] / med["trace_rays"], rays_backward_over_copy=med["rays_backward"] / med["copy_rays"],
               rays_records_only_over_copy=med["rays_records_only"] / med["copy_rays"],
               points_backward_over_closest_points=med["points_backward"] / med["closest_points"],
               points_backward_over_copy=med["points_backward"] / med["copy_points"],
               atomic_gb_per_s={"rays_backward": 72.0 * float(hit.sum().item()) / ((med["rays_backward"] - med["rays_records_only"]) * 1e6)})
    r.close()
    del d_rays, d_pts, b, pb, src48, dst48, src26, dst26

    # ---- one triangle, every record on it
    m = 1 << 20
    tri = {"vertices": np.float32([(-1, -1, 0), (1.5, -1, 0.2), (-0.5, 1.5, -0.1)]), "triangles": np.uint32([(0, 1, 2)]), "material_index": 0,
           "normals": None}
    rng = np.random.default_rng(1)
    uv = rng.uniform(0.02, 0.48, size=(m, 2))
    V = tri["vertices"].astype(np.float64)
    target = V[0] + uv[:, :1] * (V[1] - V[0]) + uv[:, 1:] * (V[2] - V[0])
    o = target + np.stack([rng.uniform(-0.5, 0.5, m), rng.uniform(-0.5, 0.5, m), rng.uniform(2, 4, m)], -1)
    r = pkg.Renderer(0)
    r.upload([tri], [((0.0, 4.0, 2.0), 60.0)], [{"albedo": (0.8, 0.8, 0.8), "type": 1}], dynamic=True)
    d_rays = torch.from_numpy(pkg.make_rays(o, target - o)).cuda()
    b = buffers(m, 3)
    torch.cuda.synchronize()
    legs = ray_legs(r, m, d_rays, b, "one_")
    legs["one_trace_rays"]()
    all_hit = bool((b["inst"] == 0).all().item())
    one = measure(legs)
    med1 = one["median_ms"]
    one.update(records=m, all_hit=all_hit, rays_backward_over_trace_rays=med1["one_rays_backward"] / med1["one_trace_rays"],
               rays_backward_over_records_only=med1["one_rays_backward"] / med1["one_rays_records_only"],
               atomics_per_us=9.0 * m / ((med1["one_rays_backward"] - med1["one_rays_records_only"]) * 1e3))
    r.close()

    out = {"workload": "C3 as a dynamic scene: heightfield 708x708 quads + ground (1 002 530 triangles), the 1920x1080 camera rays; and one triangle hit by 2^20 rays",
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "c3": big, "one_triangle": one, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
