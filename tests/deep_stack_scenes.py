"""Scenes whose rays hold far more stack entries than the LDS part of the kernels' per-lane stack ("How deep a
stack gets"), for tests/test_deep_stacks.py.

A chain is n plates: triangle k is (-a, -a, z) (3a, -a, z) (-a, 3a, z) with a = 0.6 s_k, z = sign * s_k and s_k = s0 * r**k, each
repeated `dup` times as coincident copies.  The geometric growth makes the SAH, Morton and PLOC hierarchies peel the plates off one
group per level, so a ray from the apex finds the continuing child nearest at every wide node while the other three children are
hit as well: three pushes per wide level.  Chain A (sign = -1) lies in front of the identity camera at the origin; chain B
(sign = +1) lies behind it and is deep for the walks that take children in slot order (any hit, counts, lists)."""
import numpy as np

IDENTITY = np.eye(3, dtype=np.float32)
TMIN, TMAX = 0.001, 10000.0  # the frames' ray interval: every s_k must lie inside it
LIGHT = ((0.001, 0.002, 9000.0), 1.0e8)  # behind chain B, a little off the axis: shadow rays cross the whole chain


def plates(n, r, s0, dup=1, sign=-1.0):
    """one mesh of n * dup triangles; vertices float32, three of their own per triangle"""
    s = s0 * float(r) ** np.arange(n, dtype=np.float64)
    assert TMIN < s.min() and s.max() < TMAX
    a = 0.6 * s
    z = sign * s
    tri = np.stack([np.stack([-a, -a, z], 1), np.stack([3 * a, -a, z], 1), np.stack([-a, 3 * a, z], 1)], 1)  # (n, 3, 3)
    v = np.repeat(tri, dup, axis=0).reshape(-1, 3).astype(np.float32)
    return {"vertices": v, "triangles": np.arange(len(v), dtype=np.uint32).reshape(-1, 3), "material_index": 0, "normals": None}


def even_plates(n_tris, z0=-1.0, z1=-40.0):
    """n_tris plates of one size at even spacing: a shallow tree over as many triangles as a deep chain has"""
    z = np.linspace(z0, z1, n_tris)
    a = np.full(n_tris, 30.0)
    tri = np.stack([np.stack([-a, -a, z], 1), np.stack([3 * a, -a, z], 1), np.stack([-a, 3 * a, z], 1)], 1)
    v = tri.reshape(-1, 3).astype(np.float32)
    return {"vertices": v, "triangles": np.arange(len(v), dtype=np.uint32).reshape(-1, 3), "material_index": 0, "normals": None}


def _scene(meshes, lights=()):
    return {"meshes": meshes, "lights": list(lights), "materials": [{"albedo": (0.8, 0.7, 0.6), "type": 1}],
            "camera": {"position": np.zeros(3, dtype=np.float32), "matrix": IDENTITY.copy()}}


def chain_a(n=34, r=1.5, s0=0.01, dup=7):
    """chain A alone: camera rays are deep (238 triangles; over the LBVH tree depth4 is 20 and a lane holds 60 entries)"""
    return _scene([plates(n, r, s0, dup, -1.0)])


def plate_and_chain_b(n=30, dup=4):
    """one plate in front of the camera, chain B behind it and a light behind chain B: the camera rays hold nothing, the shadow
    rays walk chain B in slot order, and the bounce rays off the plate walk it nearest child first"""
    return _scene([plates(1, 1.5, 0.01, 1, -1.0), plates(n, 1.5, 0.02, dup, 1.0)], [LIGHT])


MIRROR = {"albedo": (0.9, 0.9, 0.9), "type": 2}  # REFLECTIVE
BACKDROP_Z = 3000.0  # behind the largest plate of chain B (s = 2557), within the frames' ray interval along every mirrored ray
APEX_LIGHT = ((0.0005, 0.001, 0.005), 3.0e8)  # between the mirror and chain B, next to the apex


def _quad(lo, hi, z, material):
    v = np.float32([[lo, lo, z], [hi, lo, z], [hi, hi, z], [lo, hi, z]])
    return {"vertices": v, "triangles": np.uint32([[0, 1, 3], [1, 2, 3]]), "material_index": material, "normals": None}


def mirror_and_chain_b(n=30, dup=4):
    """plate_and_chain_b with a mirror for its front plate (a second material; chain B stays diffuse), a diffuse backdrop behind
    chain B and a second light next to the apex.  The mirror is the whole square the front plate is half of, so the camera
    rays, which hold nothing, are mirrored into chain B in two kinds: those inside the plates' triangle end on the first plate,
    those in the other half of the square (x + y > 1.2 z) cross every box of the chain, miss every plate and end on the
    backdrop.  Both walk the chain nearest child first.  The backdrop faces the apex light through the whole chain, so the
    shadow ray that follows such a turn walks the chain in slot order, and its light depends on where the mirrored ray arrived"""
    sc = plate_and_chain_b(n, dup)
    a = 0.6 * 0.01
    sc["materials"] = sc["materials"] + [dict(MIRROR)]
    sc["meshes"] = [_quad(-a, 3 * a, -0.01, 1), sc["meshes"][1], _quad(-0.7 * BACKDROP_Z, 2.0 * BACKDROP_Z, BACKDROP_Z, 0)]
    sc["lights"] = sc["lights"] + [APEX_LIGHT]
    return sc


def shallow_like(sc):
    """per mesh of sc, evenly spaced plates of the same triangle count (same buffers' sizes, a shallow tree)"""
    meshes = []
    for i, m in enumerate(sc["meshes"]):
        sign = -1.0 if i == 0 else 1.0
        meshes.append(even_plates(len(m["triangles"]), sign * 1.0, sign * 40.0))
    return dict(sc, meshes=meshes)


def apex_rays(make_rays, n, seed, towards=+1.0, tmin=0.0, tmax=np.inf):
    """n seeded rays from near the apex into the chain on the `towards` side of z: directions inside the cone every plate covers
    (|x|, |y| < 0.5 |z|; the plates reach from -0.6 to about 1.2 on both axes), origins within 1e-4 of the origin"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1e-4, 1e-4, (n, 3)).astype(np.float32)
    d = np.empty((n, 3), dtype=np.float32)
    d[:, 0:2] = rng.uniform(-0.5, 0.5, (n, 2))
    d[:, 2] = towards
    d *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)  # not normalised: t in units of |d|
    return make_rays(o, d, tmin=tmin, tmax=tmax)
