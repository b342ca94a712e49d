#!/usr/bin/env python3
"""All-hits ray queries (crt_list_hits_device) beside crt_count_hits_device, in one process.  Legs, all seeded:
  c3      C3 height field (BASELINE.json configs[2], 1 002 530 triangles), 4 194 304 rays, origins uniform in the scene box,
          directions uniform on the sphere, tmax = inf: the hit-count leg of tools/point_query_bench.py
  soup    scenes.icosphere_soup() (3125 closed spheres, 1 000 000 triangles), 1 048 576 such rays: many closed surfaces per ray
  long    a stack of 1024 parallel two-triangle sheets, 32 768 oblique rays from below whose tmax clips the stack anywhere:
          list lengths uniform in 0 .. 1024.  The leg the sort's crossover ("list_short_max") is chosen on: --short-max a,b,c
          times the filling call at each value.
Per leg three calls, alternating in order round by round, each issued back to back on one stream after a warm-up and timed
with HIP events (ms per call = events / calls, the median over rounds; min and max show the spread):
  count    crt_count_hits_device
  offsets  crt_list_hits_device without record arrays (count + scan)
  fill     crt_list_hits_device with all four arrays and capacity = the total (count + scan + fill + sort)
phase_ms = where a filling call's time goes: HIP events the library records between its kernels when a call is given stats
(crt_debug_list_phases: count, scan, fill, sort + resolve), medians over rounds x calls such calls; share = each over their
sum.  Prints one JSON object.

  python tools/list_hits_bench.py [--calls 5] [--warmup 2] [--rounds 4] [--legs c3,soup,long] [--short-max 8,24,64] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT_MAX = 24  # the library's default "list_short_max", set explicitly below so that the figures say what they were taken with
sys.path.insert(0, ROOT)


def random_rays(pkg, rng, lo, hi, n):
    d = rng.normal(size=(n, 3))
    return pkg.make_rays((lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32),
                         (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32), tmin=0.0, tmax=np.inf)


def sheet_stack(rng, n_sheets, dz, half):
    z = (np.arange(n_sheets) * dz).astype(np.float32)
    v = np.zeros((n_sheets, 4, 3), np.float32)
    v[:, :, 0:2] = np.float32([[-half, -half], [half, -half], [half, half], [-half, half]])
    v[:, :, 2] = z[:, None]
    base = 4 * np.arange(n_sheets)[:, None]
    t = np.concatenate([base + np.array([0, 1, 2]), base + np.array([0, 2, 3])])
    return {"vertices": v.reshape(-1, 3), "triangles": t[rng.permutation(len(t))].astype(np.uint32), "material_index": 0, "normals": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--legs", default="c3,soup,long")
    ap.add_argument("--short-max", default=None, help="comma-separated list_short_max values to time the long leg's filling call at")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as e
    pkg = e.load_package()
    scenes = importlib.import_module(e.PKG_NAME + ".scenes")
    rng = np.random.default_rng(1234)
    r = pkg.Renderer(0)
    r.set_option("list_short_max", SHORT_MAX)
    stream = torch.cuda.current_stream()
    result = {"calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "legs": {}}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(a.calls):
            fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) / a.calls

    for leg in a.legs.split(","):
        if leg == "long":
            mesh = sheet_stack(rng, 1024, 0.01, 200.0)
            meshes, lights, mats = [mesh], [], [{"albedo": (1, 1, 1), "type": 1}]
            n = 1 << 15
            o = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(-2.0, -1.0, n)], axis=1).astype(np.float32)
            d = rng.normal(size=(n, 3)).astype(np.float32)
            d[:, 2] = np.abs(d[:, 2]) + 0.7
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            through = (10.24 + 2.0) / d[:, 2]  # beyond the top sheet
            rays = pkg.make_rays(o, d, tmin=0.0, tmax=(rng.random(n) * through).astype(np.float32))
        else:
            sc = scenes.heightfield() if leg == "c3" else scenes.icosphere_soup()
            meshes, lights, mats = sc["meshes"], sc["lights"], sc["materials"]
            verts = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in meshes])
            rays = random_rays(pkg, rng, verts.min(axis=0), verts.max(axis=0), 1 << (22 if leg == "c3" else 20))
        r.upload(meshes, lights, mats)
        n = len(rays)
        d_rays = torch.from_numpy(rays).cuda()
        d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        r.set_stream(stream.cuda_stream)
        total = r.list_hits_device(n, d_rays.data_ptr(), d_off.data_ptr(), 0, total=True)
        cap = max(total, 1)
        d_t = torch.empty(cap, dtype=torch.float32, device="cuda")
        d_uv = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        d_inst = torch.empty(cap, dtype=torch.int32, device="cuda")
        d_prim = torch.empty(cap, dtype=torch.int32, device="cuda")
        calls = {
            "count": lambda: r.count_hits_device(n, d_rays.data_ptr(), d_cnt.data_ptr()),
            "offsets": lambda: r.list_hits_device(n, d_rays.data_ptr(), d_off.data_ptr(), 0),
            "fill": lambda: r.list_hits_device(n, d_rays.data_ptr(), d_off.data_ptr(), cap, d_t.data_ptr(), d_uv.data_ptr(), d_inst.data_ptr(),
                                               d_prim.data_ptr()),
        }
        names = list(calls)
        ms = {k: [] for k in names}
        for i in range(a.rounds):
            for k in (names if i % 2 == 0 else names[::-1]):
                ms[k].append(timed(calls[k]))
        med = {k: statistics.median(v) for k, v in ms.items()}
        phases = {k: [] for k in ("count", "scan", "fill", "sort")}
        for _ in range(a.rounds * a.calls):
            r.list_hits_device(n, d_rays.data_ptr(), d_off.data_ptr(), cap, d_t.data_ptr(), d_uv.data_ptr(), d_inst.data_ptr(), d_prim.data_ptr(),
                               stats=True)
            for k, v in r.list_phases().items():
                phases[k].append(v)
        phase_ms = {k: statistics.median(v) for k, v in phases.items()}
        cnt = np.diff(d_off.cpu().numpy())
        out = {"rays": n, "triangles": int(sum(len(m["triangles"]) for m in meshes)), "hits": int(total), "hits_per_ray": total / n,
               "longest_list": int(cnt.max()), "short_max": SHORT_MAX, "lists_above_short_max": int((cnt > SHORT_MAX).sum()),
               "ms": ms, "median_ms": med, "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
               "mrays_per_s": {k: n / (med[k] * 1e3) for k in names},
               "ratio_to_count": {k: med[k] / med["count"] for k in names},
               "phase_ms": phase_ms, "share": {k: v / sum(phase_ms.values()) for k, v in phase_ms.items()}}
        if leg == "long" and a.short_max:
            sweep = {}
            values = [int(x) for x in a.short_max.split(",")]
            for i in range(a.rounds):
                for v in (values if i % 2 == 0 else values[::-1]):
                    r.set_option("list_short_max", v)
                    sweep.setdefault(v, []).append(timed(calls["fill"]))
            r.set_option("list_short_max", SHORT_MAX)
            out["short_max_ms"] = {str(v): statistics.median(x) for v, x in sweep.items()}
        r.reset_stream()
        torch.cuda.synchronize()
        result["legs"][leg] = out
    r.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
