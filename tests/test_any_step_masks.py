"""The render kernel's any-hit node step on lane masks (traversal.hip.h, the RENDER form of LayLegacy::anyStep): the three push
conditions and the "nothing hit" condition of a shadow ray's step are formed on the scalar unit from the four slab compares' lane
masks and handed back as branch masks, instead of being widened to 0 / 1 registers and combined there.  No stack operation moves,
so mode 100 frames -- with the LDS part of the stack at 1, 5 and 16 entries, with narrow and wide fetch offsets, with and without
the Phong term, by the plain and the counting kernel -- must be the oracle's frame for frame and counter for counter.

A frame says nothing about a pattern of hit children its shadow rays never meet.  So before the GPU is used,
test_shadow_ray_steps_meet_every_pattern walks the oracle's wide tree with a float32 numpy restatement of the kernels' slab test
for every shadow ray of every scene's frame and asserts that the any-hit steps meet all 16 combinations of hit children, on
stacks on both sides of each LDS size, and that the scene with its light among the geometry has packets of mixed direction signs
(the generic loop).  That walk is a coverage check only: a borderline ray counted on the wrong side does not matter."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deep_stack_scenes import plate_and_chain_b  # noqa: E402

W, H = 64, 64
ENTRIES = (1, 5, 16)
PHONGS = (0, 300)
SCENES = ("heightfield", "soup", "inside", "plates", "deep")
MISS = 0xFFFFFFFF
K_SHADOW_BIAS = np.float32(1e-3)
K_SLAB_PAD = np.float32(2.0 ** -21)
K_CULL_PAD = np.float32(1.0 + 2.0 ** -18)
K_DIR_EPS = np.float32(1e-20)
K_DONE = -(1 << 31)


def _mesh(v, t, material=0):
    return {"vertices": np.asarray(v, dtype=np.float32).reshape(-1, 3), "triangles": np.asarray(t, dtype=np.uint32).reshape(-1, 3),
            "material_index": material, "normals": None}


def _plates_scene(scenes):
    """A floor seen from above, a light high over it, and between them groups of four separated plates side by side, each plate of
    a few triangles: the shadow rays of the floor's pixels rise through the groups, and by where a ray starts it crosses the boxes
    of none, any one or several of a group's four plates -- a node of four separated children under a light, origins on a grid
    below."""
    rng = np.random.default_rng(77)
    meshes = [_mesh([(-6, 0, 6), (6, 0, 6), (-6, 0, -6), (6, 0, -6)], [(0, 1, 2), (3, 2, 1)], 0)]
    v, t = [], []
    for gx in range(-1, 2):
        for gz in range(-1, 2):
            for k in range(4):  # four overlapping-in-projection plates at four heights
                cx, cz = 3.0 * gx + rng.uniform(-0.5, 0.5), 3.0 * gz + rng.uniform(-0.5, 0.5)
                y = 1.0 + 0.6 * k + rng.uniform(0.0, 0.2)
                sx, sz = rng.uniform(0.8, 1.6, 2)
                n = 3  # n x n quads
                xs, zs = np.linspace(cx - sx, cx + sx, n + 1), np.linspace(cz - sz, cz + sz, n + 1)
                base = len(v)
                v += [(x, y + 0.05 * np.sin(3 * x + 2 * z), z) for x in xs for z in zs]
                for i in range(n):
                    for j in range(n):
                        a = base + i * (n + 1) + j
                        t += [(a, a + 1, a + n + 1), (a + n + 2, a + n + 1, a + 1)]
    meshes.append(_mesh(v, t, 1))
    return {"meshes": meshes, "lights": [((0.5, 14.0, 0.3), 4000.0), ((-7.0, 6.0, 5.0), 1500.0)],
            "materials": [{"albedo": (0.8, 0.8, 0.8), "type": 1}, {"albedo": (0.9, 0.5, 0.4), "type": 1}],
            "camera": {"position": np.array((0.0, 16.0, 3.0), dtype=np.float32), "matrix": scenes.camera_matrix(0.0, 80.0)}}


def _scene(scenes, name):
    if name == "heightfield":
        return scenes.heightfield(n=32, n_lights=2)  # 2 050 triangles, two shadow rays per hit
    if name == "soup":
        return scenes.icosphere_soup(n_spheres=40, subdiv=1, extent=6.0)  # 3 202 triangles, close together
    if name == "inside":  # one light among the geometry, just over the middle of the terrain: shadow rays run towards it from all sides
        sc = scenes.heightfield(n=32, n_lights=1)
        return dict(sc, lights=[((0.3, 1.9, -0.4), 60.0)])
    if name == "plates":
        return _plates_scene(scenes)
    return plate_and_chain_b()  # tests/deep_stack_scenes.py: shadow rays walk chain B in slot order, three pushes per level


@pytest.fixture(scope="module")
def scenes(pkg):
    """the package's scene generators, loaded by path under a name of this module's own.  (Importing them as the package's
    submodule binds the name `scenes` in the package, and tests/test_binding_surface.py, which runs after this file and without
    a GPU has no other user of the scenes before it, reads every name bound there as public surface.)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("any_step_masks_scenes", os.path.join(os.path.dirname(pkg.__file__), "scenes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def refs(oracle, scenes):
    """per scene: the scene, the oracle's wide tree and triangles, and its mode 100 frames without and with the Phong term.
    Computed once, never changed."""
    out = {}
    for name in SCENES:
        sc = _scene(scenes, name)
        cam = sc["camera"]
        O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
        frames = {}
        try:
            for phong in PHONGS:
                oracle.set_phong(phong, 32)
                frames[phong] = O.render(cam["position"], cam["matrix"], 100, W, H)
        finally:
            oracle.set_phong(0, 32)
        dirs = np.zeros((H, W, 3), dtype=np.float32)
        for y in range(H):
            for x in range(W):
                dirs[y, x] = oracle.ray_dir(cam["matrix"], x, y, W, H)
        out[name] = {"scene": sc, "frames": frames, "nodes4q": O.nodes4q(), "tris": O.tris(), "dirs": dirs}
        O.close()
    return out


# ---- float32 restatement of the shadow rays and of the any-hit walk (traversal.hip.h makeRay, slab, anyStep)
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _dot(a, b):
    return _fma(a[:, 2], b[:, 2], _fma(a[:, 1], b[:, 1], a[:, 0] * b[:, 0]))


def _cross(a, b):
    return np.stack([_fma(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])), _fma(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2])),
                     _fma(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]))], 1)


def _shadow_rays(ref):
    """origin, unit direction, length and pixel of every shadow ray of the frame: per hit pixel and light with a positive cosine,
    from the hit point moved 1e-3 along the normal facing the viewer (flat normals: none of these scenes has vertex normals)"""
    sc, fr, tris = ref["scene"], ref["frames"][0], ref["tris"]
    tri_of = {(int(t["inst"]), int(t["prim"])): i for i, t in enumerate(tris)}
    ys, xs = np.nonzero(fr["hit_inst"] != MISS)
    idx = np.array([tri_of[(int(fr["hit_inst"][y, x]), int(fr["hit_prim"][y, x]))] for y, x in zip(ys, xs)], dtype=np.int64)
    d = ref["dirs"][ys, xs]
    o = np.asarray(sc["camera"]["position"], dtype=np.float32)[None, :]
    P = _fma(d, fr["hit_t"][ys, xs][:, None], o)
    N = _cross(tris["e1"][idx], tris["e2"][idx])
    N = N * (np.float32(1.0) / np.sqrt(_dot(N, N)))[:, None]
    N = np.where((_dot(N, d) > 0)[:, None], -N, N)
    Po = _fma(N, K_SHADOW_BIAS, P)
    O_, D_, T_, PIX = [], [], [], []
    for (lp, _) in sc["lights"]:
        Lv = np.asarray(lp, dtype=np.float32)[None, :] - Po
        dist = np.sqrt(_dot(Lv, Lv))
        Ld = Lv * (np.float32(1.0) / dist)[:, None]
        lit = _dot(N, Ld) > 0
        O_.append(Po[lit]); D_.append(Ld[lit]); T_.append(dist[lit]); PIX.append(np.stack([xs[lit], ys[lit]], 1))
    return np.concatenate(O_), np.concatenate(D_), np.concatenate(T_), np.concatenate(PIX)


def _walk_any(nodes4q, tris, o, d, tmax):
    """every ray's any-hit walk in the kernels' order (children in slot order, the first hit one next, the others pushed last slot
    first; a leaf ends the ray if one of its triangles lies in (0, tmax)).  Returns the number of node steps per pattern
    h0 | h1 << 1 | h2 << 2 | h3 << 3, the same split by the stack height in front of the step's pushes, and occluded per ray."""
    n = len(o)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ds = np.where(np.abs(d) < K_DIR_EPS, np.copysign(K_DIR_EPS, d), d)
        idir = np.float32(1.0) / ds
        noid = -(o * idir)
        noidn = noid - np.abs(noid) * K_SLAB_PAD
        neg = np.signbit(d)
        tcull = tmax * K_CULL_PAD
        cur = np.zeros(n, dtype=np.int64) if len(nodes4q) else np.full(n, K_DONE, dtype=np.int64)
        stack = np.zeros((n, 128), dtype=np.int64)
        sp = np.zeros(n, dtype=np.int64)
        occluded = np.zeros(n, dtype=bool)
        patterns = np.zeros(16, dtype=np.int64)
        by_height = {}
        qlo = np.stack([nodes4q["qlo_x"], nodes4q["qlo_y"], nodes4q["qlo_z"]], 1)
        qhi = np.stack([nodes4q["qhi_x"], nodes4q["qhi_y"], nodes4q["qhi_z"]], 1)
        while True:
            inner = np.nonzero(cur >= 0)[0]
            if len(inner):
                nd = cur[inner]
                a = nodes4q["s"][nd] * idir[inner]
                bn = _fma(nodes4q["lo"][nd], idir[inner], noidn[inner])
                bf = _fma(np.abs(noidn[inner]), np.float32(2.0) * K_SLAB_PAD, bn)
                hit = np.zeros((len(inner), 4), dtype=bool)
                for k in range(4):
                    lo = ((qlo[nd] >> (8 * k)) & 0xFF).astype(np.float32)
                    hi = ((qhi[nd] >> (8 * k)) & 0xFF).astype(np.float32)
                    near, far = np.where(neg[inner], hi, lo), np.where(neg[inner], lo, hi)
                    tn, tf = _fma(near, a, bn), _fma(far, a, bf)
                    t_n = np.maximum(np.maximum(tn[:, 0], tn[:, 1]), np.maximum(tn[:, 2], np.float32(0.0)))
                    t_f = np.minimum(np.minimum(tf[:, 0], tf[:, 1]), np.minimum(tf[:, 2], tcull[inner]))
                    hit[:, k] = t_n <= t_f
                pat = hit[:, 0] * 1 + hit[:, 1] * 2 + hit[:, 2] * 4 + hit[:, 3] * 8
                patterns += np.bincount(pat, minlength=16)
                for hgt in np.unique(sp[inner]):
                    by_height.setdefault(int(hgt), np.zeros(16, dtype=np.int64))
                    by_height[int(hgt)] += np.bincount(pat[sp[inner] == hgt], minlength=16)
                refs = nodes4q["ref"][nd].astype(np.int64)
                first = np.argmax(hit, axis=1)
                nxt = refs[np.arange(len(inner)), first]
                none = pat == 0
                pop = none & (sp[inner] > 0)
                sp[inner[pop]] -= 1
                nxt[pop] = stack[inner[pop], sp[inner[pop]]]
                nxt[none & ~pop] = K_DONE
                for k in (3, 2, 1):
                    push = hit[:, k] & (first < k) & ~none
                    stack[inner[push], sp[inner[push]]] = refs[push, k]
                    sp[inner[push]] += 1
                cur[inner] = nxt
                continue
            leaf = np.nonzero((cur < 0) & (cur != K_DONE))[0]
            if not len(leaf):
                break
            code = ~cur[leaf] & 0xFFFFFFFF
            first, cnt = code >> 3, code & 7
            for i in range(int(cnt.max()) if len(cnt) else 0):
                live = np.nonzero((i < cnt) & ~occluded[leaf])[0]
                if not len(live):
                    break
                ray, T = leaf[live], tris[first[live] + i]
                p = _cross(d[ray], T["e2"])
                inv = np.float32(1.0) / _dot(T["e1"], p)
                s = o[ray] - T["v0"]
                u = _dot(s, p) * inv
                q = _cross(s, T["e1"])
                v = _dot(d[ray], q) * inv
                t = _dot(T["e2"], q) * inv
                occluded[ray] |= (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < tmax[ray])
            done = occluded[leaf] | (sp[leaf] == 0)
            sp[leaf[~done]] -= 1
            cur[leaf] = np.where(done, K_DONE, stack[leaf, sp[leaf]])
    return patterns, by_height, occluded


@pytest.fixture(scope="module")
def walks(refs):
    out = {}
    for name in SCENES:
        o, d, tmax, pix = _shadow_rays(refs[name])
        patterns, by_height, occluded = _walk_any(refs[name]["nodes4q"], refs[name]["tris"], o, d, tmax)
        out[name] = {"patterns": patterns, "by_height": by_height, "occluded": occluded, "d": d, "pix": pix}
    return out


def test_shadow_ray_steps_meet_every_pattern(walks):
    """All 16 combinations of hit children, overall and in every scene but the chain (whose rays are aimed down one axis); steps
    whose first push lands below and at or above every tested LDS size (the pushes of one step land at heights h .. h + 2, so
    steps straddle the boundary too); occluded and unoccluded rays; and in the scene with its light among the geometry, 8x8
    packets whose shadow rays disagree on a direction sign."""
    total = np.zeros(16, dtype=np.int64)
    for name in SCENES:
        w = walks[name]
        print("%s: %d shadow rays, %d occluded, steps per pattern %s, deepest stack in front of a step %d"
              % (name, len(w["d"]), int(w["occluded"].sum()), w["patterns"].tolist(), max(w["by_height"])))
        total += w["patterns"]
        if name != "deep":  # (behind the chain every shadow ray is occluded, and its steps hit the last two or three children)
            assert 0 < w["occluded"].sum() < len(w["d"]), name
            assert (w["patterns"] > 0).all(), "%s: patterns never met: %s" % (name, np.nonzero(w["patterns"] == 0)[0].tolist())
    assert (total > 0).all()
    pushing = [p for p in range(16) if bin(p).count("1") >= 2]
    for entries in ENTRIES:
        below = sum(int(h[pushing].sum()) for name in SCENES for hgt, h in walks[name]["by_height"].items() if hgt < entries)
        above = sum(int(h[pushing].sum()) for name in SCENES for hgt, h in walks[name]["by_height"].items() if hgt >= entries)
        print("stack_entries %d: pushing steps whose first push lands in the LDS part %d, in the arena %d" % (entries, below, above))
        assert below > 0 and above > 0, entries
    w = walks["inside"]
    packet = (w["pix"][:, 1] // 8) * (W // 8) + w["pix"][:, 0] // 8
    mixed = 0
    for p in np.unique(packet):
        s = np.signbit(w["d"][packet == p])
        mixed += bool((s.any(axis=0) & ~s.all(axis=0)).any())
    print("inside: %d of %d packets with shadow rays of mixed direction signs" % (mixed, len(np.unique(packet))))
    assert mixed > 0


def test_walk_agrees_with_the_oracle_on_occlusion(oracle, scenes, refs, walks):
    """the restated walk is the kernels' walk: its shadow rays are occluded where the oracle's any-hit query says so, but for a
    handful of borderline rays (the restated origins are the oracle's to within rounding, not bit for bit)"""
    for name in ("heightfield", "plates"):
        sc = refs[name]["scene"]
        o, d, tmax, _ = _shadow_rays(refs[name])
        O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"])
        rays = np.concatenate([o, np.zeros((len(o), 1), np.float32), d, tmax[:, None]], 1).astype(np.float32)
        want = oracle.occluded_rays(O, rays)["occluded"].astype(bool)
        O.close()
        differ = int((want != walks[name]["occluded"]).sum())
        print("%s: %d of %d rays differ" % (name, differ, len(o)))
        assert differ <= len(o) // 100


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


def _check(got, ref, what, counting):
    for k in ("hit_inst", "hit_prim", "hit_t", "rgba8"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (what, k))
    if counting:
        for k in ("rays_primary", "rays_shadow", "nodes_visited", "tris_tested"):
            assert got["stats"][k] == ref["stats"][k], "%s %s: %d, oracle %d" % (what, k, got["stats"][k], ref["stats"][k])


@pytest.mark.gpu
@pytest.mark.parametrize("entries", ENTRIES)
@pytest.mark.parametrize("name", SCENES)
def test_frames_match_the_oracle(refs, renderer, name, entries):
    ref = refs[name]
    sc = ref["scene"]
    renderer.upload(sc["meshes"], sc["lights"], sc["materials"])
    renderer.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
    renderer.change_shading_mode(100)
    try:
        renderer.set_option("stack_entries", entries)
        for wide in (0, 1):
            renderer.set_option("wide_offsets", wide)
            for phong in PHONGS:
                renderer.set_option("phong_ks", phong)
                for counting in (False, True):
                    renderer.set_counting(counting)
                    what = "%s stack_entries=%d wide_offsets=%d phong %d counting=%d" % (name, entries, wide, phong, counting)
                    _check(renderer.render_frame(W, H), ref["frames"][phong], what, counting)
    finally:
        renderer.set_counting(False)
        for k, v in (("wide_offsets", 0), ("stack_entries", 0), ("phong_ks", 0)):
            renderer.set_option(k, v)
        renderer.change_shading_mode(0)
