#!/usr/bin/env python3
"""Cost of progressive accumulation (crt_set_accumulation) on the C5 workload (BASELINE.json configs[4]: 5M triangles,
3840x2160, mode 200, 4 spp, 3 bounces).  In one process, three legs alternate round by round:
  off        accumulation off: the plain frame (what bench.py --config c5 measures)
  on         accumulation on, far from the limit: every frame reads and writes the per-pixel sums (four doubles each, 265 MB)
  saturated  accumulation at its limit: no ray traced, the stored sums resolved to RGBA8 (resolve-only kernel)
Frames are issued back to back on one stream (crt_render_frame_device) after a warm-up; ms/frame = HIP events around the leg's
frames / frames.  Prints one JSON object (and writes it to --out when given).

  python tools/accumulate_bench.py [--frames 10] [--warmup 3] [--rounds 4] [--out FILE]"""
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
    ap.add_argument("--frames", type=int, default=10, help="timed frames per leg and round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed frames before each leg's timed frames")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as e
    pkg = e.load_package()
    scenes = importlib.import_module(e.PKG_NAME + ".scenes")
    W, H, SPP = 3840, 2160, 4
    sc = scenes.heightfield(n=1581, n_lights=1)
    r = pkg.Renderer(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
    r.change_shading_mode(200)
    r.set_path_params(SPP, 3, 1234)
    frame = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    r.set_stream(stream.cuda_stream)

    def leg(name):
        if name == "off":
            r.set_accumulation(0)
        elif name == "on":
            r.set_accumulation(1 << 24)   # starts over; the limit is never reached here
        else:
            r.set_accumulation(SPP)       # the first warm-up frame fills the sums, every later frame only resolves them
        for _ in range(a.warmup):
            r.render_frame_device(W, H, frame.data_ptr())
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(a.frames):
            r.render_frame_device(W, H, frame.data_ptr())
        t1.record(stream)
        t1.synchronize()
        n = r.accumulated_samples()
        expect = 0 if name == "off" else (SPP if name == "saturated" else SPP * (a.warmup + a.frames))
        assert n == expect, (name, n, expect)
        return t0.elapsed_time(t1) / a.frames

    legs = ("off", "on", "saturated")
    ms = {k: [] for k in legs}
    for i in range(a.rounds):
        for k in (legs if i % 2 == 0 else legs[::-1]):  # alternate the order: no leg always follows the same one
            ms[k].append(leg(k))
    r.set_accumulation(0)
    r.reset_stream()
    r.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"workload": "C5: heightfield 1581x1581 quads + ground (4 999 124 triangles), %dx%d, mode 200, %d spp, 3 bounces" % (W, H, SPP),
           "frames_per_leg": a.frames, "warmup": a.warmup, "rounds": a.rounds, "ms_per_frame": ms, "median_ms": med,
           "accumulate_over_off": med["on"] / med["off"] - 1.0, "saturated_ms": med["saturated"],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
