#!/usr/bin/env python3
"""The variance calls (crt_temporal_variance_device, crt_denoise_variance_device, defaults) beside their parents on the C3 workload
(BASELINE.json configs[2]: scenes.heightfield(), 1 002 530 triangles, its camera and light) at 1920x1080 and 3840x2160.  Input: the
mode-200 frame at 1 spp with its guides, for two poses; prev_point is a buffer of NaN (nothing moved: the motion kernels run).  Legs:
  tv_first       crt_temporal_variance_device without history: every live pixel is short, the 7 x 7 window runs everywhere
  tv_converged   the second pose (moved 0.05 to the right, yawed 1 degree) against a history of six frames of the first pose: almost
                 every wavefront skips the window
  tm_first, tm_converged   crt_temporal_accumulate_motion_device on the same inputs
  dv             crt_denoise_variance_device, 5 iterations, on tv_converged's colour and variance
  dn             crt_denoise_device, 5 iterations, on the same colour
Yardsticks on the same context:
  copy_tv        a device-to-device copy of tv_converged's compulsory bytes: 148 B per pixel (40 in: rgb, normal, albedo, t; 12
                 prev_point; 32 + 8 of history and moments read; 32 + 8 + 4 written; 12 out), as a copy of 74 B per pixel
  copy_dv        the same for dv: 60 B per pixel (44 in, 12 + 4 out), as a copy of 30 B per pixel
  frame_1spp     the mode-200 frame at 1 spp
Every figure of a library call is the call's own kernel_ms (HIP events around its kernels, crt_frame_stats); the copies are timed
with HIP events around torch's copy.  Legs alternate in order round by round; per leg the median and the spread (min, max) over
rounds x calls.  No time is a pass condition.  Prints one JSON object (and writes it to --out).

--legs restricts the run to some legs (for a profiler's kernel trace of one leg); the ratios need all of them and are then left out.

  python tools/variance_bench.py [--calls 5] [--warmup 2] [--rounds 4] [--legs tv_converged,...] [--out FILE]"""
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
    ap.add_argument("--legs", default=None, help="comma-separated legs to run; default: all")
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

    results = {}
    for W, H in ((1920, 1080), (3840, 2160)):
        n = W * H
        f32 = dict(dtype=torch.float32, device="cuda")
        d_rgba = torch.empty(n, dtype=torch.int32, device="cuda")

        def render(k, seed):
            d = {"rgb": torch.empty((n, 3), **f32), "normal": torch.empty((n, 3), **f32), "albedo": torch.empty((n, 3), **f32), "t": torch.empty(n, **f32)}
            r.set_camera(poses[k][:3], poses[k][3:])
            r.set_path_params(1, 3, seed)
            r.render_frame_device(W, H, d_rgba.data_ptr(), d_rgb=d["rgb"].data_ptr(), stats=True)
            r.frame_guides_device(W, H, d["normal"].data_ptr(), d["albedo"].data_ptr(), d["t"].data_ptr(), stats=True)
            return d
        d_pp = torch.full((n, 3), float("nan"), **f32)
        hist = [torch.empty((n, 8), **f32) for _ in range(3)]
        mom = [torch.empty((n, 2), **f32) for _ in range(3)]
        d_var, d_out, d_filtered, d_vout = torch.empty(n, **f32), torch.empty((n, 3), **f32), torch.empty((n, 3), **f32), torch.empty(n, **f32)
        d_src, d_dst = torch.empty(n * 37, dtype=torch.int16, device="cuda"), torch.empty(n * 37, dtype=torch.int16, device="cuda")  # 74 B per pixel
        torch.cuda.synchronize()

        def variance(d, k, prev, at, to):
            return r.temporal_variance_device(W, H, poses[k], poses[prev], d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(),
                                              d["t"].data_ptr(), None if at is None else hist[at].data_ptr(), hist[to].data_ptr(),
                                              None if at is None else mom[at].data_ptr(), mom[to].data_ptr(), d_var.data_ptr(), d_out.data_ptr(),
                                              stats=True, d_prev_point=d_pp.data_ptr())["kernel_ms"]

        def motion(d, k, prev, at, to):
            return r.temporal_accumulate_device(W, H, poses[k], poses[prev], d["rgb"].data_ptr(), d["normal"].data_ptr(), d["albedo"].data_ptr(),
                                                d["t"].data_ptr(), None if at is None else hist[at].data_ptr(), hist[to].data_ptr(),
                                                d_out.data_ptr(), stats=True, d_prev_point=d_pp.data_ptr())["kernel_ms"]
        at = None
        for f in range(6):  # six frames of the first pose: hist[at], mom[at] with len 6
            to = 0 if at != 0 else 1
            variance(render(0, 1234 + f), 0, 0, at, to)
            at = to
        first, moving = render(0, 1234), render(1, 1240)
        variance(moving, 1, 0, at, 2)  # d_out, d_var: the filter's input
        d_acc, d_accvar = d_out.clone(), d_var.clone()
        short = int(((hist[2][:, 3] > 0) & (hist[2][:, 3] < 4)).sum().item())
        live = int((hist[2][:, 3] > 0).sum().item())
        # the share of the V6 kernel's 64 x 4 tiles that hold a short pixel and so fill their halo (W and H are multiples of the tile)
        is_short = ((hist[2][:, 3] > 0) & (hist[2][:, 3] < 4)).reshape(H // 4, 4, W // 64, 64)
        tiles_short = float(is_short.any(dim=3).any(dim=1).float().mean().item()) if H % 4 == 0 and W % 64 == 0 else None
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def copy(items):
            r.synchronize()
            ev0.record()
            d_dst[:items].copy_(d_src[:items])
            ev1.record()
            torch.cuda.synchronize()
            return ev0.elapsed_time(ev1)

        def call(name):
            if name == "frame_1spp":
                return r.render_frame_device(W, H, d_rgba.data_ptr(), stats=True)["kernel_ms"]
            if name == "copy_tv":
                return copy(n * 37)
            if name == "copy_dv":
                return copy(n * 15)
            if name == "tv_first":
                return variance(first, 0, 0, None, 2)
            if name == "tv_converged":
                return variance(moving, 1, 0, at, 2)
            if name == "tm_first":
                return motion(first, 0, 0, None, 2)
            if name == "tm_converged":
                return motion(moving, 1, 0, at, 2)
            g = moving
            if name == "dv":
                return r.denoise_variance_device(W, H, d_acc.data_ptr(), g["normal"].data_ptr(), g["albedo"].data_ptr(), g["t"].data_ptr(),
                                                 d_accvar.data_ptr(), d_filtered.data_ptr(), d_vout.data_ptr(), stats=True, iterations=5)["kernel_ms"]
            return r.denoise_device(W, H, d_acc.data_ptr(), g["normal"].data_ptr(), g["albedo"].data_ptr(), g["t"].data_ptr(), d_filtered.data_ptr(),
                                    stats=True, iterations=5)["kernel_ms"]

        names = ["frame_1spp", "tv_first", "tv_converged", "tm_first", "tm_converged", "dv", "dn", "copy_tv", "copy_dv"]
        if a.legs:
            if not set(a.legs.split(",")) <= set(names):
                ap.error("--legs takes some of " + ",".join(names))
            names = [k for k in names if k in a.legs.split(",")]
        ms = {k: [] for k in names}
        for i in range(a.rounds):
            for k in (names if i % 2 == 0 else names[::-1]):  # alternate the order: no leg always follows the same one
                for _ in range(a.warmup):
                    call(k)
                ms[k] += [call(k) for _ in range(a.calls)]
        med = {k: statistics.median(v) for k, v in ms.items()}
        results["%dx%d" % (W, H)] = {
            "live_fraction": live / n, "converged_short_fraction_of_live": short / max(live, 1), "converged_tiles_with_a_short_pixel": tiles_short,
            "median_ms": med, "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()}}
        if not a.legs:
            results["%dx%d" % (W, H)].update({
                "first_over_converged": med["tv_first"] / med["tv_converged"],
                "over_parent": {"tv_first": med["tv_first"] / med["tm_first"], "tv_converged": med["tv_converged"] / med["tm_converged"],
                                "dv": med["dv"] / med["dn"]},
                "over_copy": {"tv_first": med["tv_first"] / med["copy_tv"], "tv_converged": med["tv_converged"] / med["copy_tv"],
                              "dv": med["dv"] / med["copy_dv"]}})
        del d_rgba, hist, mom, d_var, d_out, d_filtered, d_vout, d_src, d_dst, d_pp, first, moving, d_acc, d_accvar
    r.close()
    out = {"workload": "C3: heightfield 708x708 quads + ground (1 002 530 triangles), 1 light, mode 200 at 1 spp, 3 bounces; variance calls, defaults",
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "sizes": results, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
