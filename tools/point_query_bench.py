#!/usr/bin/env python3
"""Point queries (crt_closest_points_device / crt_occupancy_device / crt_count_hits_device) on the C3 workload (BASELINE.json
configs[2]: scenes.heightfield(), 1 002 530 triangles).  Legs, all seeded, alternating in order round by round:
  near_closest        2^20 points within ~0.05 of the height field's vertices, rmax = inf, closest point
  uniform_closest     2^20 points uniform in the scene box, rmax = inf
  uniform_closest_r1  the same points with rmax = 1 % of the scene diagonal
  occupancy_grid      occupancy of a 128^3 grid over the scene box (2 097 152 points, three rays each)
  count_random        hit counts of 2^22 rays, origins uniform in the scene box, directions uniform on the sphere, tmax inf
Each leg is issued back to back on one stream after a warm-up and timed with HIP events; ms per call = events / calls, the
median over rounds.  One extra counting call per leg gives nodes and triangles fetched per query.  Prints one JSON object
(and writes it to --out when given).

  python tools/point_query_bench.py [--calls 5] [--warmup 2] [--rounds 4] [--legs a,b,...] [--out FILE]"""
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
    ap.add_argument("--legs", default=None, help="comma-separated subset of the legs (default: all)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as e
    pkg = e.load_package()
    scenes = importlib.import_module(e.PKG_NAME + ".scenes")
    sc = scenes.heightfield()
    r = pkg.Renderer(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    rng = np.random.default_rng(1234)
    verts = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))

    n = 1 << 20
    hv = np.asarray(sc["meshes"][1]["vertices"], dtype=np.float32).reshape(-1, 3)
    near = hv[rng.integers(0, len(hv), size=n)] + rng.normal(size=(n, 3)).astype(np.float32) * np.float32(0.05)
    uni = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    g = (np.arange(128) + 0.5) / 128.0
    gx, gy, gz = np.meshgrid(g, g, g, indexing="ij")
    grid = (lo + np.stack([gx, gy, gz], axis=-1).reshape(-1, 3) * (hi - lo)).astype(np.float32)
    n_rand = 1 << 22
    d = rng.normal(size=(n_rand, 3))
    rand_rays = pkg.make_rays((lo + rng.random((n_rand, 3)) * (hi - lo)).astype(np.float32),
                              (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32), tmin=0.0, tmax=np.inf)
    sets = {"near": pkg.make_points(near), "uniform": pkg.make_points(uni), "uniform_r1": pkg.make_points(uni, rmax=0.01 * diag),
            "grid": pkg.make_points(grid), "random": rand_rays}
    dev = {k: torch.from_numpy(v).cuda() for k, v in sets.items()}
    nmax = max(len(v) for v in sets.values())
    d_dist = torch.empty(nmax, dtype=torch.float32, device="cuda")
    d_point = torch.empty((nmax, 3), dtype=torch.float32, device="cuda")
    d_uv = torch.empty((nmax, 2), dtype=torch.float32, device="cuda")
    d_inst = torch.empty(nmax, dtype=torch.int32, device="cuda")
    d_prim = torch.empty(nmax, dtype=torch.int32, device="cuda")
    d_cnt = torch.empty(nmax, dtype=torch.int32, device="cuda")
    d_occ = torch.empty(nmax, dtype=torch.bool, device="cuda")
    stream = torch.cuda.current_stream()
    r.set_stream(stream.cuda_stream)

    legs = {"near_closest": ("near", "closest"), "uniform_closest": ("uniform", "closest"), "uniform_closest_r1": ("uniform_r1", "closest"),
            "occupancy_grid": ("grid", "occupancy"), "count_random": ("random", "count")}
    names = a.legs.split(",") if a.legs else list(legs)

    def call(name, stats=False):
        src, kind = legs[name]
        k, p = len(sets[src]), dev[src].data_ptr()
        if kind == "closest":
            return r.closest_points_device(k, p, d_dist.data_ptr(), d_point.data_ptr(), d_uv.data_ptr(), d_inst.data_ptr(), d_prim.data_ptr(),
                                           stats=stats)
        if kind == "occupancy":
            return r.occupancy_device(k, p, d_occ.data_ptr(), stats=stats)
        return r.count_hits_device(k, p, d_cnt.data_ptr(), stats=stats)

    def leg(name):
        for _ in range(a.warmup):
            call(name)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(a.calls):
            call(name)
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) / a.calls

    ms = {k: [] for k in names}
    for i in range(a.rounds):
        for k in (names if i % 2 == 0 else names[::-1]):  # alternate the order: no leg always follows the same one
            ms[k].append(leg(k))
    r.set_counting(True)
    fetch = {}
    for k in names:
        st = call(k, stats=True)
        q = len(sets[legs[k][0]])
        fetch[k] = {"nodes_per_query": st["nodes_visited"] / q, "tris_per_query": st["tris_tested"] / q}
    r.set_counting(False)
    r.reset_stream()
    torch.cuda.synchronize()
    r.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    queries = {k: len(sets[legs[k][0]]) for k in names}
    out = {"workload": "C3: heightfield 708x708 quads + ground (1 002 530 triangles)",
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "queries": queries, "ms": ms, "median_ms": med,
           "mquery_per_s": {k: queries[k] / (med[k] * 1e3) for k in names}, "fetch": fetch, "rmax_r1": 0.01 * diag,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
