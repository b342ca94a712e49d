#!/usr/bin/env python3
"""GPU rebuild (crt_rebuild) and the PLOC builder (option "gpu_builder" = 1, include/crt_hip.h) on the 1M-triangle scenes:
scenes.heightfield() and scenes.icosphere_soup(), uploaded with option "dynamic", mode 100 at 1920x1080.  Per scene and tree
(sah = host SAH upload, lbvh / ploc = "gpu_build" upload with that builder; a SAH scene's rebuilds use the LBVH):
  upload_ms / build_device_ms        crt_build_stats of the upload
  rebuild_device_ms / rebuild_wall_ms   crt_rebuild with nothing pending (median of 5): HIP-event time and wall time of the call
  frame_ms.{static, refit_rotated, rebuild_rotated}   kernel time (median of --frames) before any update, after a rigid
                                     10-degree rotation of every mesh carried in by crt_refit, and the same rotation carried in by
                                     crt_rebuild
  fetch.{static, refit_rotated, rebuild_rotated}   [nodes_visited, tris_tested] of one counting frame
Per-kernel times: run this under rocprofv3 --kernel-trace --stats (a run of its own).
Prints one JSON object (and writes it to --out when given).

  python tools/rebuild_bench.py [--frames 20] [--scenes heightfield,soup] [--trees sah,lbvh,ploc] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUILDERS = {"sah": (0, 0), "lbvh": (1, 0), "ploc": (1, 1)}  # tree -> ("gpu_build", "gpu_builder")


def frame_ms(r, buf, w, h, n):
    for _ in range(3):
        r.render_frame_device(w, h, buf.data_ptr(), stats=True)
    return statistics.median(r.render_frame_device(w, h, buf.data_ptr(), stats=True)["kernel_ms"] for _ in range(n))


def fetches(r, buf, w, h):
    r.set_counting(True)
    st = r.render_frame_device(w, h, buf.data_ptr(), stats=True)
    r.set_counting(False)
    return [st["nodes_visited"], st["tris_tested"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--scenes", default="heightfield,soup")
    ap.add_argument("--trees", default="sah,lbvh,ploc")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as e
    pkg = e.load_package()
    scenes = importlib.import_module(e.PKG_NAME + ".scenes")
    W, H = 1920, 1080
    makers = {"heightfield": scenes.heightfield, "soup": scenes.icosphere_soup}
    buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    ang = np.deg2rad(10.0)
    rot = np.float32([[np.cos(ang), 0, np.sin(ang), 0], [0, 1, 0, 0], [-np.sin(ang), 0, np.cos(ang), 0]])
    r = pkg.Renderer(0)
    out = {"frame": [W, H], "mode": 100, "legs": {}}
    try:
        for name in a.scenes.split(","):
            sc = makers[name]()
            for tree in a.trees.split(","):
                gb, builder = BUILDERS[tree]
                r.set_option("gpu_build", gb)
                r.set_option("gpu_builder", builder)
                r.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=True)
                r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
                r.change_shading_mode(100)
                leg = {"n_tris": sum(len(m["triangles"]) for m in sc["meshes"])}
                bs = r.build_stats()
                leg["upload_ms"], leg["build_device_ms"] = bs["upload_ms"], bs["device_build_ms"]
                fm = {"static": frame_ms(r, buf, W, H, a.frames)}
                fc = {"static": fetches(r, buf, W, H)}
                dev, wall = [], []
                for _ in range(5):
                    t0 = time.perf_counter()
                    dev.append(r.rebuild())
                    wall.append((time.perf_counter() - t0) * 1e3)
                leg["rebuild_device_ms"], leg["rebuild_wall_ms"] = statistics.median(dev), statistics.median(wall)
                # back to the uploaded tree, then the rotation through a refit
                r.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=True)
                r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
                for i in range(len(sc["meshes"])):
                    r.set_mesh_transform(i, rot)
                leg["refit_device_ms_rotated"] = r.refit()
                fm["refit_rotated"] = frame_ms(r, buf, W, H, a.frames)
                fc["refit_rotated"] = fetches(r, buf, W, H)
                t0 = time.perf_counter()
                leg["rebuild_device_ms_rotated"] = r.rebuild()
                leg["rebuild_wall_ms_rotated"] = (time.perf_counter() - t0) * 1e3
                fm["rebuild_rotated"] = frame_ms(r, buf, W, H, a.frames)
                fc["rebuild_rotated"] = fetches(r, buf, W, H)
                n4, d4 = r.bvh_export4()
                leg["nodes4_depth4_rebuilt"] = [len(n4), d4]
                leg["max_depth_rebuilt"] = r.bvh_info()["max_depth"]
                leg["frame_ms"], leg["fetch"] = fm, fc
                out["legs"]["%s/%s" % (name, tree)] = leg
                print(json.dumps({"%s/%s" % (name, tree): leg}), flush=True)
    finally:
        r.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
