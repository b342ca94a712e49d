#!/usr/bin/env python3
"""The guide buffers (crt_frame_guides_device) and the a-trous denoiser (crt_denoise_device, 5 iterations, defaults) on the C3
workload (BASELINE.json configs[2]: scenes.heightfield(), 1 002 530 triangles, its camera and light) at 1920x1080 and
3840x2160.  Input: the mode-200 frame at 1 spp and at 4 spp with its guides.  Two yardsticks on the same context:
  copy_pass    a device-to-device copy of the bytes ONE pass must move: 32 B in (colour + guide of the centre) and 16 B out per
               pixel, done as a 32 B/pixel copy -- a pass cannot be faster than that, five passes not faster than five of them
  frame_1spp   the mode-200 frame at 1 spp: a denoiser has to cost less than the samples it stands in for
Every figure of a library call is the call's own kernel_ms (HIP events around its kernels, crt_frame_stats); the copy is timed
with HIP events around torch's copy.  Legs alternate in order round by round; per leg the median and the spread (min, max) over
rounds x calls.  Prints one JSON object (and writes it to --out).

  python tools/denoise_bench.py [--calls 5] [--warmup 2] [--rounds 4] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

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
    r = pkg.Renderer(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    r.set_camera(cam["position"], cam["matrix"])
    r.change_shading_mode(200)

    results = {}
    for W, H in ((1920, 1080), (3840, 2160)):
        n = W * H
        f32 = dict(dtype=torch.float32, device="cuda")
        d_rgba = torch.empty(n, dtype=torch.int32, device="cuda")
        d_rgb = {spp: torch.empty((n, 3), **f32) for spp in (1, 4)}
        d_nrm, d_alb, d_out = (torch.empty((n, 3), **f32) for _ in range(3))
        d_t = torch.empty(n, **f32)
        d_src, d_dst = torch.empty(n * 8, **f32), torch.empty(n * 8, **f32)  # 32 B per pixel each
        for spp in (1, 4):
            r.set_path_params(spp, 3, 1234)
            r.render_frame_device(W, H, d_rgba.data_ptr(), d_rgb=d_rgb[spp].data_ptr(), stats=True)
        r.set_path_params(1, 3, 1234)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def call(name):
            if name == "frame_1spp":
                return r.render_frame_device(W, H, d_rgba.data_ptr(), stats=True)["kernel_ms"]
            if name == "guides":
                return r.frame_guides_device(W, H, d_nrm.data_ptr(), d_alb.data_ptr(), d_t.data_ptr(), stats=True)["kernel_ms"]
            if name == "copy_pass":
                r.synchronize()
                ev0.record()
                d_dst.copy_(d_src)
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1)
            spp = int(name.split("_")[1][0])
            return r.denoise_device(W, H, d_rgb[spp].data_ptr(), d_nrm.data_ptr(), d_alb.data_ptr(), d_t.data_ptr(), d_out.data_ptr(), stats=True,
                                    iterations=5)["kernel_ms"]

        call("guides")  # the denoiser's input
        names = ["frame_1spp", "guides", "denoise_1spp", "denoise_4spp", "copy_pass"]
        ms = {k: [] for k in names}
        for i in range(a.rounds):
            for k in (names if i % 2 == 0 else names[::-1]):  # alternate the order: no leg always follows the same one
                for _ in range(a.warmup):
                    call(k)
                ms[k] += [call(k) for _ in range(a.calls)]
        live = int(((d_nrm != 0).any(dim=1) & (d_t > 0)).sum().item())
        med = {k: statistics.median(v) for k, v in ms.items()}
        results["%dx%d" % (W, H)] = {
            "live_fraction": live / n, "median_ms": med, "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
            "denoise_over_5_copy_passes": {s: med["denoise_" + s] / (5.0 * med["copy_pass"]) for s in ("1spp", "4spp")},
            "denoise_over_frame_1spp": {s: med["denoise_" + s] / med["frame_1spp"] for s in ("1spp", "4spp")},
            "guides_over_frame_1spp": med["guides"] / med["frame_1spp"]}
        del d_rgba, d_rgb, d_nrm, d_alb, d_out, d_t, d_src, d_dst
    r.close()
    out = {"workload": "C3: heightfield 708x708 quads + ground (1 002 530 triangles), 1 light, mode 200, 3 bounces; denoiser: 5 iterations, defaults",
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "sizes": results, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
