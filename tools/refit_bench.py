#!/usr/bin/env python3
"""Dynamic geometry (crt_refit, include/crt_hip.h) on the 1M-triangle scenes: scenes.heightfield() (1 002 530 triangles) and
scenes.icosphere_soup() (1 000 002), each over the host SAH tree and the GPU LBVH tree (option "gpu_build"), uploaded with
option "dynamic".  Per scene and tree:
  upload_ms / build_device_ms   crt_build_stats of the dynamic upload (host SAH: wall time; LBVH: also the build kernels' time)
  refit_device_ms / refit_wall_ms   crt_refit after an identity update of the big mesh: HIP-event time of the refit, and the
                                    call's wall time (the collapse reads one count per wide level back to the host)
  frame_ms.{static, identity, wave, rotated}   mode 100 at 1920x1080, kernel time (HIP events, median of --frames) before any
                                    update, after an identity refit, after a small wave deformation of the big mesh and after
                                    a rigid 10-degree rotation of every mesh
  per_frame_update_ms / per_frame_static_ms   wall time per iteration of: new vertices (host form, two seeded wave phases
                                    alternating) + refit + frame, against frames alone -- geometry that changes every frame,
                                    so no launch order is reused
Per-kernel times of the refit stages: run this under rocprofv3 --kernel-trace --stats (a run of its own).
Prints one JSON object (and writes it to --out when given).

  python tools/refit_bench.py [--frames 20] [--scenes heightfield,soup] [--trees sah,lbvh] [--out FILE]"""
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


def frame_ms(r, torch, buf, w, h, n):
    for _ in range(3):
        r.render_frame_device(w, h, buf.data_ptr(), stats=True)
    return statistics.median(r.render_frame_device(w, h, buf.data_ptr(), stats=True)["kernel_ms"] for _ in range(n))


def wave(v, phase, amp):
    out = v.copy()
    out[:, 1] += (amp * np.sin(0.7 * v[:, 0] + 0.5 * v[:, 2] + phase)).astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--scenes", default="heightfield,soup")
    ap.add_argument("--trees", default="sah,lbvh")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as e
    pkg = e.load_package()
    scenes = importlib.import_module(e.PKG_NAME + ".scenes")
    W, H = 1920, 1080
    makers = {"heightfield": scenes.heightfield, "soup": scenes.icosphere_soup}
    buf = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    r = pkg.Renderer(0)
    out = {"frame": [W, H], "mode": 100, "legs": {}}
    try:
        for name in a.scenes.split(","):
            sc = makers[name]()
            big = int(np.argmax([len(m["triangles"]) for m in sc["meshes"]]))
            v0 = np.ascontiguousarray(sc["meshes"][big]["vertices"], dtype=np.float32)
            for tree in a.trees.split(","):
                r.set_option("gpu_build", 1 if tree == "lbvh" else 0)
                r.upload(sc["meshes"], sc["lights"], sc["materials"], dynamic=True)
                r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
                r.change_shading_mode(100)
                leg = {"n_tris": sum(len(m["triangles"]) for m in sc["meshes"])}
                bs = r.build_stats()
                leg["upload_ms"], leg["build_device_ms"] = bs["upload_ms"], bs["device_build_ms"]
                n4, d4 = r.bvh_export4()
                leg["nodes4_depth4_static"] = [len(n4), d4]
                fm = {"static": frame_ms(r, torch, buf, W, H, a.frames)}
                dev, wall = [], []
                for _ in range(5):
                    r.update_vertices(big, v0)
                    t0 = time.perf_counter()
                    dev.append(r.refit())
                    wall.append((time.perf_counter() - t0) * 1e3)
                leg["refit_device_ms"], leg["refit_wall_ms"] = statistics.median(dev), statistics.median(wall)
                fm["identity"] = frame_ms(r, torch, buf, W, H, a.frames)
                r.update_vertices(big, wave(v0, 0.0, 0.05))
                leg["refit_device_ms_wave"] = r.refit()
                fm["wave"] = frame_ms(r, torch, buf, W, H, a.frames)
                ang = np.deg2rad(10.0)
                rot = np.float32([[np.cos(ang), 0, np.sin(ang), 0], [0, 1, 0, 0], [-np.sin(ang), 0, np.cos(ang), 0]])
                for i in range(len(sc["meshes"])):
                    r.set_mesh_transform(i, rot)
                leg["refit_device_ms_rotated"] = r.refit()
                fm["rotated"] = frame_ms(r, torch, buf, W, H, a.frames)
                n4, d4 = r.bvh_export4()
                leg["nodes4_depth4_rotated"] = [len(n4), d4]
                leg["frame_ms"] = fm
                for i in range(len(sc["meshes"])):
                    r.set_mesh_transform(i, None)
                variants = [wave(v0, 0.0, 0.05), wave(v0, 1.0, 0.05)]
                r.update_vertices(big, variants[1])
                r.render_frame_device(W, H, buf.data_ptr(), stats=True)
                t0 = time.perf_counter()
                for k in range(a.frames):
                    r.update_vertices(big, variants[k % 2])
                    r.render_frame_device(W, H, buf.data_ptr())
                r.synchronize()
                leg["per_frame_update_ms"] = (time.perf_counter() - t0) * 1e3 / a.frames
                t0 = time.perf_counter()
                for k in range(a.frames):
                    r.render_frame_device(W, H, buf.data_ptr())
                r.synchronize()
                leg["per_frame_static_ms"] = (time.perf_counter() - t0) * 1e3 / a.frames
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
