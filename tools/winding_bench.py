#!/usr/bin/env python3
"""Winding numbers (crt_winding_numbers_device) on the C3 workload (BASELINE.json configs[2]: scenes.heightfield(), 1 002 530
triangles), beside crt_occupancy_device on the same points and beside a device copy of the call's compulsory bytes (16 read
and 4 written per point).  Legs, all seeded, alternating in order round by round:
  winding_beta1 / _beta2 / _beta4   2^20 points uniform in the scene box at beta = 1, 2, 4
  winding_exact                     the first 4096 of them in exact mode (beta = 0: every triangle, 4 x 10^9 terms)
  occupancy                         crt_occupancy_device on the 2^20 points
  copy                              torch copy of 20 x 2^20 bytes
Each leg is issued back to back on one stream after a warm-up and timed with HIP events; ms per call = events / calls, the
median over rounds.  The moment table's build is timed once, as the wall time of the first query of 64 points (which builds
the table and waits for it) less that of the same query repeated.  One extra counting call per winding leg gives nodes and
triangles fetched per point.  Prints one JSON object (and writes it to --out when given).

  python tools/winding_bench.py [--calls 5] [--warmup 2] [--rounds 4] [--legs a,b,...] [--tree sah|lbvh|ploc] [--out FILE]"""
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
TREES = {"sah": {"gpu_build": 0}, "lbvh": {"gpu_build": 1, "gpu_builder": 0}, "ploc": {"gpu_build": 1, "gpu_builder": 1}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5, help="timed calls per leg and round")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls before each leg's timed calls")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--legs", default=None, help="comma-separated subset of the legs (default: all)")
    ap.add_argument("--tree", default="sah", choices=sorted(TREES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as e
    pkg = e.load_package()
    scenes = importlib.import_module(e.PKG_NAME + ".scenes")
    sc = scenes.heightfield()
    r = pkg.Renderer(0)
    for k, v in TREES[a.tree].items():
        r.set_option(k, v)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    rng = np.random.default_rng(1234)
    verts = np.concatenate([np.asarray(m["vertices"], dtype=np.float32).reshape(-1, 3) for m in sc["meshes"]])
    lo, hi = verts.min(axis=0), verts.max(axis=0)

    n, n_exact = 1 << 20, 4096
    pts = pkg.make_points((lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32))
    d_pts = torch.from_numpy(pts).cuda()
    d_w = torch.empty(n, dtype=torch.float32, device="cuda")
    d_occ = torch.empty(n, dtype=torch.bool, device="cuda")
    d_src = torch.empty(20 * n, dtype=torch.uint8, device="cuda")
    d_dst = torch.empty_like(d_src)
    stream = torch.cuda.current_stream()
    r.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()

    def tiny():
        t0 = time.perf_counter()
        r.winding_numbers_device(64, d_pts.data_ptr(), d_w.data_ptr(), 2.0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    first = tiny()
    again = statistics.median(tiny() for _ in range(5))

    legs = {"winding_beta1": (n, 1.0), "winding_beta2": (n, 2.0), "winding_beta4": (n, 4.0), "winding_exact": (n_exact, 0.0),
            "occupancy": (n, None), "copy": (n, None)}
    names = a.legs.split(",") if a.legs else list(legs)

    def call(name, stats=False):
        k, beta = legs[name]
        if name == "copy":
            d_dst.copy_(d_src)
            return None
        if name == "occupancy":
            return r.occupancy_device(k, d_pts.data_ptr(), d_occ.data_ptr(), stats=stats)
        return r.winding_numbers_device(k, d_pts.data_ptr(), d_w.data_ptr(), beta, stats=stats)

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
        if k != "copy":
            st = call(k, stats=True)
            fetch[k] = {"nodes_per_query": st["nodes_visited"] / legs[k][0], "tris_per_query": st["tris_tested"] / legs[k][0]}
    r.set_counting(False)
    r.reset_stream()
    torch.cuda.synchronize()
    info = r.bvh_info()
    r.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    queries = {k: legs[k][0] for k in names}
    out = {"workload": "C3: heightfield 708x708 quads + ground (1 002 530 triangles)", "tree": a.tree, "n_tris": info["n_tris"],
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "queries": queries, "ms": ms, "median_ms": med,
           "mquery_per_s": {k: queries[k] / (med[k] * 1e3) for k in names}, "fetch": fetch,
           "first_query_wall_ms": first, "repeated_query_wall_ms": again, "moments_build_wall_ms": first - again,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
