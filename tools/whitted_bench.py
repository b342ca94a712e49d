#!/usr/bin/env python3
"""Shading mode 150 (Whitted: mode 100 seen through mirrors and glass) on the icosphere soup (scenes.icosphere_soup(): 3125
icospheres of 320 triangles over a ground quad, 1 000 002 triangles, its camera and light, 1920x1080), the spheres cut into
three meshes by sphere number.  Two scenes of the same geometry:
  diffuse    every material DIFFUSE: mode 150 does mode 100's work, so shade150 / shade100 is the job's overhead
  specular   the second third of the spheres REFLECTIVE, the last third REFRACTIVE (ior 1.5)
Legs, on the frame's 2 073 600 pixel-centre camera rays (crt_camera_rays_device):
  (a) diffuse_shade100, diffuse_shade150      crt_shade_rays_device (rgb + normal + albedo + hit outputs) in mode 100 / 150
  (b) specular_shade150                       the same in mode 150 on the specular scene: rays per second, and the counted
                                              turns and shadow rays per record
  (c) <scene>_frame100, <scene>_frame150      crt_render_frame_device (rgba8 + float colour)
      <scene>_rays + <scene>_shade150rgb      what a caller composes without the frame: crt_camera_rays_device, then
                                              crt_shade_rays_device (rgb, t, inst, prim); the frame adds the quantisation
Every figure is the call's own kernel_ms (HIP events around the kernels, crt_frame_stats); legs alternate in order round by
round; per leg the median and the spread (min, max) over rounds x calls.  Prints one JSON object (and writes it to --out).

  python tools/whitted_bench.py [--bounces 8] [--calls 5] [--warmup 2] [--rounds 4] [--spheres 3125] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def soup_in_thirds(scenes, n_spheres, specular):
    """the soup with its spheres as three meshes, materials 1..3; specular: the kinds of the second and the third"""
    sc = scenes.icosphere_soup(n_spheres=n_spheres)
    ground, soup = sc["meshes"]
    nv = len(scenes._icosphere(2)[0])
    v = np.asarray(soup["vertices"], dtype=np.float32).reshape(n_spheres, nv, 3)
    t = np.asarray(soup["triangles"], dtype=np.uint32).reshape(n_spheres, -1, 3) - (np.arange(n_spheres, dtype=np.uint32) * nv)[:, None, None]
    meshes = [ground]
    for g in range(3):
        pick = np.arange(g, n_spheres, 3)
        tri = t[pick] + (np.arange(len(pick), dtype=np.uint32) * nv)[:, None, None]
        meshes.append({"vertices": np.ascontiguousarray(v[pick].reshape(-1, 3)), "triangles": np.ascontiguousarray(tri.reshape(-1, 3)),
                       "material_index": 1 + g, "normals": None})
    sc["meshes"] = meshes
    sc["materials"] = [{"albedo": (0.8, 0.8, 0.8), "type": 1}, {"albedo": (0.6, 0.8, 0.9), "type": 1},
                       {"albedo": (0.9, 0.85, 0.7), "type": 2 if specular else 1}, {"albedo": (1.0, 1.0, 1.0), "type": 3 if specular else 1, "ior": 1.5}]
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bounces", type=int, default=8, help="option max_bounces: the turns a record may take")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per leg and round")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls before each leg's timed calls")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--spheres", type=int, default=3125)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as e
    pkg = e.load_package()
    scenes = importlib.import_module(e.PKG_NAME + ".scenes")
    W, H = 1920, 1080
    n = W * H
    R = {}
    triangles = 0
    for name in ("diffuse", "specular"):
        sc = soup_in_thirds(scenes, a.spheres, name == "specular")
        triangles = sum(len(m["triangles"]) for m in sc["meshes"])
        r = pkg.Renderer(0)
        r.upload(sc["meshes"], sc["lights"], sc["materials"])
        r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
        r.set_option("max_bounces", a.bounces)
        R[name] = r
    d_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    d_scratch = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    R["diffuse"].camera_rays_device(W, H, d_rays.data_ptr(), stats=True)  # (both scenes have the one camera)
    d_rgb, d_nrm, d_alb = (torch.empty((n, 3), dtype=torch.float32, device="cuda") for _ in range(3))
    d_t = torch.empty(n, dtype=torch.float32, device="cuda")
    d_uv = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    d_inst = torch.empty(n, dtype=torch.int32, device="cuda")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda")
    frame = torch.empty(n, dtype=torch.int32, device="cuda")

    def call(leg):
        scene, what = leg.split("_")
        r = R[scene]
        if what == "rays":
            return r.camera_rays_device(W, H, d_scratch.data_ptr(), stats=True)["kernel_ms"]
        r.change_shading_mode(100 if what.endswith("100") else 150)
        if what.startswith("frame"):
            return r.render_frame_device(W, H, frame.data_ptr(), d_rgb=d_rgb.data_ptr(), stats=True)["kernel_ms"]
        if what == "shade150rgb":
            return r.shade_rays_device(n, d_rays.data_ptr(), d_rgb.data_ptr(), d_t=d_t.data_ptr(), d_inst=d_inst.data_ptr(), d_prim=d_prim.data_ptr(),
                                       stats=True)["kernel_ms"]
        return r.shade_rays_device(n, d_rays.data_ptr(), d_rgb.data_ptr(), d_nrm.data_ptr(), d_alb.data_ptr(), d_t.data_ptr(), d_uv.data_ptr(),
                                   d_inst.data_ptr(), d_prim.data_ptr(), stats=True)["kernel_ms"]

    legs = ["diffuse_shade100", "diffuse_shade150", "specular_shade150"]
    for s in R:
        legs += [s + "_frame100", s + "_frame150", s + "_rays", s + "_shade150rgb"]
    ms = {k: [] for k in legs}
    for i in range(a.rounds):
        for k in (legs if i % 2 == 0 else legs[::-1]):  # alternate the order: no leg always follows the same one
            for _ in range(a.warmup):
                call(k)
            ms[k] += [call(k) for _ in range(a.calls)]

    # what the records do (counting variant, one call per scene and mode)
    mix = {}
    for s, r in R.items():
        r.set_counting(True)
        for mode in (100, 150):
            r.change_shading_mode(mode)
            st = r.shade_rays_device(n, d_rays.data_ptr(), d_rgb.data_ptr(), d_inst=d_inst.data_ptr(), stats=True)
            mix["%s_mode%d" % (s, mode)] = {"hit_fraction": int((d_inst != -1).sum().item()) / n, "turns_per_record": (st["rays_primary"] - n) / n,
                                           "shadow_rays_per_record": st["rays_shadow"] / n, "nodes_per_record": st["nodes_visited"] / n,
                                           "tris_per_record": st["tris_tested"] / n}
        r.set_counting(False)
        r.close()

    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"workload": "icosphere soup in three meshes + ground (%d triangles), 1 light, 1920x1080 camera rays, max_bounces %d" % (triangles, a.bounces),
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "records": n, "what_the_records_do": mix, "median_ms": med,
           "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
           "a_shade150_over_shade100_diffuse": med["diffuse_shade150"] / med["diffuse_shade100"],
           "b_specular_shade150_mrays_per_s": n / med["specular_shade150"] / 1e3,
           "c_frame150_over_frame100": {s: med[s + "_frame150"] / med[s + "_frame100"] for s in R},
           "c_frame150_over_rays_plus_shade": {s: med[s + "_frame150"] / (med[s + "_rays"] + med[s + "_shade150rgb"]) for s in R},
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
