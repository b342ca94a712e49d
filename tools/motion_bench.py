#!/usr/bin/env python3
"""Motion for temporal reprojection (crt_motion_snapshot, crt_frame_motion_device, crt_previous_points_device,
crt_temporal_accumulate_motion_device) on the C3 workload (BASELINE.json configs[2]: scenes.heightfield(), 1 002 530 triangles, its
camera and light) uploaded as a dynamic scene, at 1920x1080 and 3840x2160.  After a snapshot every mesh is moved by a mesh
transform (0.05 up, 0.03 to the right), so every pixel that sees geometry has a previous point.  Legs:
  frame_guides      the guide buffers of the frame: the pass frame_motion is compared with (camera rays + shaded query)
  frame_motion      camera rays + closest-hit query + previous points
  previous_points   the previous-points kernel alone, on inst / prim / uv the caller already has (the cheaper route)
  temporal_plain    crt_temporal_accumulate_device against the history of the frame before the move
  temporal_motion   crt_temporal_accumulate_motion_device with the frame's previous points
  copy_bytes        a device-to-device copy that moves the motion call's compulsory bytes: 128 B per pixel (40 in: rgb, normal,
                    albedo, t; 12 of prev_point; 32 of history read; 32 written; 12 out), done as a copy of 64 B per pixel
Every figure of a library call is the call's own kernel_ms (HIP events, crt_frame_stats); the copy is timed with HIP events around
torch's copy.  Legs alternate in order round by round; per leg the median and the spread (min, max) over rounds x calls.  No time
is a pass condition.  Prints one JSON object (and writes it to --out).

  python tools/motion_bench.py [--calls 5] [--warmup 2] [--rounds 4] [--out FILE]"""
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
    sc = scenes.heightfield()
    cam = np.concatenate([np.asarray(sc["camera"]["position"], np.float32), np.asarray(sc["camera"]["matrix"], np.float32).reshape(9)])
    r = pkg.Renderer(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=True)
    r.set_camera(cam[:3], cam[3:])
    r.change_shading_mode(200)
    r.set_path_params(1, 3, 1234)
    move = np.float32([[1, 0, 0, 0.03], [0, 1, 0, 0.05], [0, 0, 1, 0]])

    results = {}
    for W, H in ((1920, 1080), (3840, 2160)):
        n = W * H
        f32 = dict(dtype=torch.float32, device="cuda")
        d_rgba = torch.empty(n, dtype=torch.int32, device="cuda")

        def frame():
            d = {"rgb": torch.empty((n, 3), **f32), "normal": torch.empty((n, 3), **f32), "albedo": torch.empty((n, 3), **f32), "t": torch.empty(n, **f32)}
            r.render_frame_device(W, H, d_rgba.data_ptr(), d_rgb=d["rgb"].data_ptr(), stats=True)
            r.frame_guides_device(W, H, d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(), stats=True)
            return d
        for m in range(len(sc["meshes"])):
            r.set_mesh_transform(m, None)
        before = frame()
        d_hist, d_next, d_out = torch.empty((n, 8), **f32), torch.empty((n, 8), **f32), torch.empty((n, 3), **f32)
        d_pp = torch.empty((n, 3), **f32)
        r.temporal_accumulate_device(W, H, cam, cam, before["rgb"].data_ptr(), before["normal"].data_ptr(), before["albedo"].data_ptr(),
                                     before["t"].data_ptr(), None, d_hist.data_ptr(), d_out.data_ptr(), stats=True)
        r.motion_snapshot()
        for m in range(len(sc["meshes"])):
            r.set_mesh_transform(m, move)
        now = frame()
        d_rays = torch.empty((n, 8), **f32)
        d_uv = torch.empty((n, 2), **f32)
        d_inst, d_prim = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        r.camera_rays_device(W, H, d_rays.data_ptr(), stats=True)
        r.trace_rays_device(n, d_rays.data_ptr(), None, d_uv.data_ptr(), d_inst.data_ptr(), d_prim.data_ptr(), stats=True)
        r.frame_motion_device(W, H, d_pp.data_ptr(), stats=True)
        d_src, d_dst = torch.empty(n * 32, dtype=torch.int16, device="cuda"), torch.empty(n * 32, dtype=torch.int16, device="cuda")  # 64 B per pixel
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def call(name):
            if name == "frame_guides":
                return r.frame_guides_device(W, H, now["normal"].data_ptr(), now["albedo"].data_ptr(), now["t"].data_ptr(), stats=True)["kernel_ms"]
            if name == "frame_motion":
                return r.frame_motion_device(W, H, d_pp.data_ptr(), stats=True)["kernel_ms"]
            if name == "previous_points":
                return r.previous_points_device(n, d_inst.data_ptr(), d_prim.data_ptr(), d_uv.data_ptr(), d_pp.data_ptr(), stats=True)["kernel_ms"]
            if name == "copy_bytes":
                r.synchronize()
                ev0.record()
                d_dst.copy_(d_src)
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1)
            return r.temporal_accumulate_device(W, H, cam, cam, now["rgb"].data_ptr(), now["normal"].data_ptr(), now["albedo"].data_ptr(),
                                                now["t"].data_ptr(), d_hist.data_ptr(), d_next.data_ptr(), d_out.data_ptr(), stats=True,
                                                d_prev_point=d_pp.data_ptr() if name == "temporal_motion" else None)["kernel_ms"]

        names = ["frame_guides", "frame_motion", "previous_points", "temporal_plain", "temporal_motion", "copy_bytes"]
        ms = {k: [] for k in names}
        for i in range(a.rounds):
            for k in (names if i % 2 == 0 else names[::-1]):  # alternate the order: no leg always follows the same one
                for _ in range(a.warmup):
                    call(k)
                ms[k] += [call(k) for _ in range(a.calls)]
        moved = int(torch.isfinite(d_pp).all(dim=1).sum().item())
        call("temporal_plain")
        kept_plain = int((d_next[:, 3] > 1).sum().item())
        call("temporal_motion")
        kept_motion = int((d_next[:, 3] > 1).sum().item())
        med = {k: statistics.median(v) for k, v in ms.items()}
        results["%dx%d" % (W, H)] = {
            "moved_fraction": moved / n, "with_history_fraction": {"temporal_plain": kept_plain / n, "temporal_motion": kept_motion / n},
            "median_ms": med, "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
            "frame_motion_over_frame_guides": med["frame_motion"] / med["frame_guides"],
            "temporal_motion_over_plain": med["temporal_motion"] / med["temporal_plain"],
            "temporal_motion_over_copy_bytes": med["temporal_motion"] / med["copy_bytes"],
            "gb_per_s_of_128_bytes": {k: 128.0 * n / (med[k] * 1e6) for k in ("temporal_motion", "copy_bytes")}}
        del d_rgba, before, now, d_hist, d_next, d_out, d_pp, d_rays, d_uv, d_inst, d_prim, d_src, d_dst
    r.close()
    out = {"workload": "C3 as a dynamic scene: heightfield 708x708 quads + ground (1 002 530 triangles), mode 200 at 1 spp; every mesh moved by a transform after the snapshot",
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "sizes": results, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
