#!/usr/bin/env python3
"""Temporal reprojection (crt_temporal_accumulate_device, defaults) on the C3 workload (BASELINE.json configs[2]:
scenes.heightfield(), 1 002 530 triangles, its camera and light) at 1920x1080 and 3840x2160.  Input: the mode-200 frame at 1 spp
with its guides, for two poses; the history is the accumulation's own output for the first pose.  Legs:
  static       cam_prev == cam_cur bitwise: the shortcut, a pixel's history is around its own record
  moving       the second pose (moved 0.05 to the right, yawed 1 degree) against the first pose's history: the projection
Two yardsticks on the same context:
  copy_bytes   a device-to-device copy that moves the call's compulsory bytes: 116 B per pixel (40 in: rgb, normal, albedo, t; 32
               of history read; 32 written; 12 out), done as a copy of 58 B per pixel (58 read + 58 written)
  frame_1spp   the mode-200 frame at 1 spp: the accumulation has to cost less than the samples it saves
Every figure of a library call is the call's own kernel_ms (HIP events around its kernel, crt_frame_stats); the copy is timed with
HIP events around torch's copy.  Legs alternate in order round by round; per leg the median and the spread (min, max) over rounds x
calls.  No time is a pass condition.  Prints one JSON object (and writes it to --out).

  python tools/temporal_bench.py [--calls 5] [--warmup 2] [--rounds 4] [--out FILE]"""
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
    cam = sc["camera"]
    pos0 = np.asarray(cam["position"], np.float32)
    poses = [np.concatenate([pos0, np.asarray(cam["matrix"], np.float32).reshape(9)]),
             np.concatenate([pos0 + np.float32([0.05, 0.0, 0.0]), scenes.camera_matrix(1.0, 60.0)])]
    r = pkg.Renderer(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    r.change_shading_mode(200)
    r.set_path_params(1, 3, 1234)

    results = {}
    for W, H in ((1920, 1080), (3840, 2160)):
        n = W * H
        f32 = dict(dtype=torch.float32, device="cuda")
        d_rgba = torch.empty(n, dtype=torch.int32, device="cuda")
        frames = []
        for c in poses:  # colour and guides of both poses
            d = {"rgb": torch.empty((n, 3), **f32), "normal": torch.empty((n, 3), **f32), "albedo": torch.empty((n, 3), **f32), "t": torch.empty(n, **f32)}
            r.set_camera(c[:3], c[3:])
            r.render_frame_device(W, H, d_rgba.data_ptr(), d_rgb=d["rgb"].data_ptr(), stats=True)
            r.frame_guides_device(W, H, d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(), stats=True)
            frames.append(d)
        d_hist, d_next, d_out = torch.empty((n, 8), **f32), torch.empty((n, 8), **f32), torch.empty((n, 3), **f32)
        d_src, d_dst = torch.empty(n * 29, dtype=torch.int16, device="cuda"), torch.empty(n * 29, dtype=torch.int16, device="cuda")  # 58 B per pixel
        torch.cuda.synchronize()

        def accumulate(k, prev, d_prev, d_to):
            d = frames[k]
            return r.temporal_accumulate_device(W, H, poses[k], poses[prev], d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(),
                                                d["t"].data_ptr(), d_prev, d_to.data_ptr(), d_out.data_ptr(), stats=True)["kernel_ms"]
        accumulate(0, 0, None, d_hist)  # the first pose's history
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def call(name):
            if name == "frame_1spp":
                return r.render_frame_device(W, H, d_rgba.data_ptr(), stats=True)["kernel_ms"]
            if name == "copy_bytes":
                r.synchronize()
                ev0.record()
                d_dst.copy_(d_src)
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1)
            return accumulate(0 if name == "static" else 1, 0, d_hist.data_ptr(), d_next)

        names = ["frame_1spp", "static", "moving", "copy_bytes"]
        ms = {k: [] for k in names}
        for i in range(a.rounds):
            for k in (names if i % 2 == 0 else names[::-1]):  # alternate the order: no leg always follows the same one
                for _ in range(a.warmup):
                    call(k)
                ms[k] += [call(k) for _ in range(a.calls)]
        call("moving")
        with_history = int((d_next[:, 3] > 1).sum().item())
        live = int((d_next[:, 3] > 0).sum().item())
        med = {k: statistics.median(v) for k, v in ms.items()}
        results["%dx%d" % (W, H)] = {
            "live_fraction": live / n, "moving_with_history_fraction_of_live": with_history / max(live, 1),
            "median_ms": med, "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
            "over_copy_bytes": {k: med[k] / med["copy_bytes"] for k in ("static", "moving")},
            "over_frame_1spp": {k: med[k] / med["frame_1spp"] for k in ("static", "moving")},
            "gb_per_s_of_116_bytes": {k: 116.0 * n / (med[k] * 1e6) for k in ("static", "moving", "copy_bytes")}}
        del d_rgba, frames, d_hist, d_next, d_out, d_src, d_dst
    r.close()
    out = {"workload": "C3: heightfield 708x708 quads + ground (1 002 530 triangles), 1 light, mode 200 at 1 spp, 3 bounces; temporal accumulation, defaults",
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "sizes": results, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
