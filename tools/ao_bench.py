#!/usr/bin/env python3
"""Shading mode 120 (ambient occlusion: sky visibility per hit) on the 1M-triangle height field (scenes.heightfield(n_lights=1):
708 x 708 quads over a ground quad, its camera and light), on the 2 073 600 pixel-centre camera rays of a 1920x1080 frame.
  (a) shade120_K, K = 16 and 64     crt_shade_rays_device (rgb) in mode 120, "ao_radius" 0, "ao_sky" 0: the closest hit, then K
                                    occlusion rays per hit drawn in registers
      occluded_K_bysample / _byrecord   the yardstick: crt_occluded_rays_device on the same hits x K rays, written to HBM
                                    beforehand (the contract's origins and directions restated with torch) -- sample-major,
                                    neighbouring records side by side as the mode-120 lanes hold them, and record-major, a
                                    record's K rays side by side
      trace                         crt_trace_rays_device (t, inst): the closest hit alone, for scale
      Occlusion samples per second = hits x K / kernel time; with counting on, the node and triangle fetches of each.
  (b) frame120_16, frame200_16      crt_render_frame_device (rgba8 + float colour) in mode 120 with K = 16, and in mode 200
                                    with "spp" 16 and "max_bounces" 1: the only way to this picture without mode 120
  (c) few_4096x4096                 4096 records (every 506th pixel) at K = 4096: one lane per record, a grid of 64 wavefronts
Every figure is the call's own kernel_ms (HIP events around the kernels, crt_frame_stats); legs alternate in order round by
round; per leg the median and the spread (min, max) over rounds x calls.  Prints one JSON object (and writes it to --out).

  python tools/ao_bench.py [--calls 5] [--warmup 2] [--rounds 3] [--quads 708] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M32 = 0xFFFFFFFF


def pcg_hash(v):
    """int64 tensors holding 32-bit values"""
    state = (v * 747796405 + 2891336453) & M32
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
    return ((word >> 22) ^ word) & M32


def directions(torch, ids, s, seed, N):
    """the contract's direction of sample s for the records ids (int64) with normals N (float32, n x 3)"""
    hs = pcg_hash(torch.tensor([seed & M32], dtype=torch.int64, device=ids.device))
    st = pcg_hash(pcg_hash(pcg_hash(ids ^ pcg_hash(hs + s))))
    st = pcg_hash(st)
    u1 = (st >> 8).to(torch.float32) * 2.0 ** -24
    st = pcg_hash(st)
    u2 = (st >> 8).to(torch.float32) * 2.0 ** -24
    rr, phi = torch.sqrt(u1), 6.28318530717958648 * u2
    lx, ly, lz = rr * torch.cos(phi), rr * torch.sin(phi), torch.sqrt(torch.clamp(1.0 - u1, min=0.0))
    nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
    sg = torch.where(nz >= 0, torch.ones_like(nz), -torch.ones_like(nz))
    a = -1.0 / (sg + nz)
    b = nx * ny * a
    T = torch.stack([1.0 + sg * nx * nx * a, sg * b, -sg * nx], dim=1)
    B = torch.stack([b, sg + ny * ny * a, -ny], dim=1)
    d = lx[:, None] * T + ly[:, None] * B + lz[:, None] * N
    return d / torch.linalg.norm(d, dim=1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5, help="timed calls per leg and round")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls before each leg's timed calls")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quads", type=int, default=708, help="the height field's side in quads")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import __graft_entry__ as e
    pkg = e.load_package()
    scenes = importlib.import_module(e.PKG_NAME + ".scenes")
    W, H = 1920, 1080
    n = W * H
    seed = 1234
    sc = scenes.heightfield(n=a.quads, n_lights=1)
    triangles = sum(len(m["triangles"]) for m in sc["meshes"])
    r = pkg.Renderer(0)
    r.upload(sc["meshes"], sc["lights"], sc["materials"])
    r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
    r.set_option("seed", seed)
    r.set_option("max_bounces", 1)
    r.set_option("spp", 16)

    d_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    r.camera_rays_device(W, H, d_rays.data_ptr(), stats=True)
    d_rgb, d_nrm = (torch.empty((n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    d_t = torch.empty(n, dtype=torch.float32, device="cuda")
    d_inst = torch.empty(n, dtype=torch.int32, device="cuda")
    frame = torch.empty(n, dtype=torch.int32, device="cuda")
    r.change_shading_mode(100)
    r.shade_rays_device(n, d_rays.data_ptr(), d_normal=d_nrm.data_ptr(), d_t=d_t.data_ptr(), d_inst=d_inst.data_ptr(), stats=True)
    ids = torch.nonzero(d_inst != -1).reshape(-1)
    hits = int(ids.numel())
    N = d_nrm[ids]
    Po = d_rays[ids, 0:3] + d_rays[ids, 4:7] * d_t[ids, None] + 1e-3 * N

    # the yardstick's rays, materialised: probes[K]["bysample"][s * hits + i], ["byrecord"][i * K + s]
    probes = {}
    for K in (16, 64):
        by_sample = torch.zeros((K, hits, 8), dtype=torch.float32, device="cuda")
        for s in range(K):
            by_sample[s, :, 0:3] = Po
            by_sample[s, :, 4:7] = directions(torch, ids, s, seed, N)
        by_sample[:, :, 7] = 10000.0
        probes[K] = {"bysample": by_sample.reshape(-1, 8), "byrecord": by_sample.transpose(0, 1).contiguous().reshape(-1, 8)}
    d_occ = torch.empty(hits * 64, dtype=torch.uint8, device="cuda")
    few = torch.arange(0, n, n // 4096, device="cuda")[:4096]
    d_few = d_rays[few].contiguous()
    torch.cuda.synchronize()

    def ao(K):
        r.set_option("ao_samples", K)
        r.set_option("ao_radius", 0)
        r.set_option("ao_sky", 0)
        r.change_shading_mode(120)

    def call(leg):
        what, _, arg = leg.partition("_")
        if what == "trace":
            return r.trace_rays_device(n, d_rays.data_ptr(), d_t=d_t.data_ptr(), d_inst=d_inst.data_ptr(), stats=True)
        if what == "shade120":
            ao(int(arg))
            return r.shade_rays_device(n, d_rays.data_ptr(), d_rgb.data_ptr(), stats=True)
        if what == "occluded":
            K, layout = arg.split("_")
            return r.occluded_device(hits * int(K), probes[int(K)][layout].data_ptr(), d_occ.data_ptr(), stats=True)
        if what == "frame120":
            ao(int(arg))
            return r.render_frame_device(W, H, frame.data_ptr(), d_rgb=d_rgb.data_ptr(), stats=True)
        if what == "frame200":
            r.change_shading_mode(200)
            return r.render_frame_device(W, H, frame.data_ptr(), d_rgb=d_rgb.data_ptr(), stats=True)
        ao(4096)  # few_4096x4096
        return r.shade_rays_device(4096, d_few.data_ptr(), d_rgb.data_ptr(), stats=True)

    legs = ["trace", "shade120_16", "occluded_16_bysample", "occluded_16_byrecord", "shade120_64", "occluded_64_bysample", "occluded_64_byrecord",
            "frame120_16", "frame200_16", "few_4096x4096"]
    ms = {k: [] for k in legs}
    for i in range(a.rounds):
        for k in (legs if i % 2 == 0 else legs[::-1]):  # alternate the order: no leg always follows the same one
            for _ in range(a.warmup):
                call(k)
            ms[k] += [call(k)["kernel_ms"] for _ in range(a.calls)]

    # where the time goes (counting variant, one call per leg)
    r.set_counting(True)
    fetch = {}
    for k in legs:
        st = call(k)
        fetch[k] = {"rays_primary": st["rays_primary"], "rays_shadow": st["rays_shadow"], "nodes_visited": st["nodes_visited"], "tris_tested": st["tris_tested"]}
    r.set_counting(False)
    visible = float(d_rgb[:4096, 0].mean().item())
    r.close()

    med = {k: statistics.median(v) for k, v in ms.items()}
    few_hits = fetch["few_4096x4096"]["rays_shadow"] // 4096
    out = {"workload": "height field %d x %d quads + ground (%d triangles), 1 light, 1920x1080 camera rays, seed %d" % (a.quads, a.quads, triangles, seed),
           "calls_per_leg": a.calls, "warmup": a.warmup, "rounds": a.rounds, "records": n, "hits": hits, "median_ms": med,
           "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()}, "counted": fetch,
           "a_msamples_per_s": {k: hits * int(k.split("_")[1]) / med[k] / 1e3 for k in legs if k.startswith(("shade120", "occluded"))},
           "a_shade120_over_occluded": {"%d_%s" % (K, lay): med["occluded_%d_%s" % (K, lay)] / med["shade120_%d" % K]
                                        for K in (16, 64) for lay in ("bysample", "byrecord")},
           "a_shade120_minus_trace_over_occluded": {"%d_%s" % (K, lay): med["occluded_%d_%s" % (K, lay)] / (med["shade120_%d" % K] - med["trace"])
                                                    for K in (16, 64) for lay in ("bysample", "byrecord")},
           "b_frame200_over_frame120": med["frame200_16"] / med["frame120_16"],
           "c_few_msamples_per_s": few_hits * 4096 / med["few_4096x4096"] / 1e3, "c_few_hit_records": few_hits, "c_few_mean_visibility": visible,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
