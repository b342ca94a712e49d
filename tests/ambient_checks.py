"""The ambient-occlusion contract (include/crt_hip.h "ambient occlusion", shading mode 120) composed on the CPU, shared by
tests/test_occlusion_mode.py and tests/shaded_query_checks.py: the loader of tests/ao_reference.c, and the steps of the contract
over arrays -- the biased origin and the K directions of every hit record as probe records, the reach R from an exported root
node, the colour from the number of probes that escape.  Nothing here touches a GPU: who holds the hits, the normals and the
probes' occlusion (other GPU queries in test_occlusion_mode.py, the oracle and brute force in shaded_query_checks.py) passes
them in."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNBOUNDED = np.float32(10000.0)  # the reach of "ao_radius" = 0

_lib = None
_dir = None  # the temporary directory the library lives in, kept for the life of the process


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def build_reference(out):
    """tests/ao_reference.c compiled to the shared library `out`, loaded, with its argument types"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for tests/ao_reference.c")
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(ROOT, "tests", "ao_reference.c"),
                           "-o", out, "-lm"])
    L = C.CDLL(out)
    vp, u32 = C.c_void_p, C.c_uint32
    L.ao_ref_bounce.argtypes = [u32, vp, vp, vp, vp]
    L.ao_ref_origins.argtypes = [u32, vp, vp, vp, vp]
    L.ao_ref_directions.argtypes = [u32, vp, u32, u32, vp, vp]
    L.ao_ref_radius.argtypes = [u32, vp]
    L.ao_ref_radius.restype = C.c_float
    L.ao_ref_colour.argtypes = [u32, vp, u32, C.c_int, vp, vp, vp, vp]
    for f in (L.ao_ref_bounce, L.ao_ref_origins, L.ao_ref_directions, L.ao_ref_colour):
        f.restype = None
    return L


def reference():
    """the library, built once per process"""
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="ao_reference")
        _lib = build_reference(os.path.join(_dir.name, "libao_reference.so"))
    return _lib


@pytest.fixture(scope="module")
def ref():
    return reference()


def radius(L, v, nodes):
    """the reach R of option "ao_radius" = v: 10000 for 0, else v thousandths of the diagonal of the box of node 0 of
    crt_bvh_export (`nodes`: what bvh_export() returned first, read when the check runs)"""
    if v == 0:
        return UNBOUNDED
    if len(nodes) == 0:
        return np.float32(0.0)
    node0 = np.ascontiguousarray(nodes[:1]).view(np.float32)[:12].copy()
    return np.float32(L.ao_ref_radius(int(v), node0.ctypes.data))


def probe_records(L, rays, t, normal, ids, k, seed, R):
    """steps 2 and 3: for every hit record (`rays` its 8 floats, `t` its hit distance, `normal` the unit normal the query
    returns, `ids` its index in the call) the k probes {Po, 0, direction, R} as ray records, (len(rays) * k, 8), record-major"""
    n = len(rays)
    records, t, normal = _f32(rays).reshape(-1, 8), _f32(t).reshape(-1), _f32(normal).reshape(-1, 3)
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    assert len(t) == n and len(normal) == n and len(ids) == n
    po = np.zeros((n, 3), dtype=np.float32)
    dirs = np.zeros((n, k, 3), dtype=np.float32)
    if n:
        L.ao_ref_origins(n, records.ctypes.data, t.ctypes.data, normal.ctypes.data, po.ctypes.data)
        L.ao_ref_directions(n, ids.ctypes.data, int(k), int(seed), normal.ctypes.data, dirs.ctypes.data)
    probes = np.zeros((n * k, 8), dtype=np.float32)
    probes[:, 0:3] = np.repeat(po, k, axis=0)
    probes[:, 4:7] = dirs.reshape(-1, 3)
    probes[:, 7] = R
    return probes


def composed_rgb(L, n, hit, visible, k, sky, albedo, miss, direct):
    """steps 4 and 5: the colour of n records of which those at the indices `hit` hit, `visible[j]` of the k probes of hit j
    escaped; albedo and direct (mode 100's colour) per hit; the others hold the miss colour"""
    miss = _f32(miss).reshape(3)
    visible = np.ascontiguousarray(visible, dtype=np.uint32).reshape(-1)
    albedo, direct = _f32(albedo).reshape(-1, 3), _f32(direct).reshape(-1, 3)
    assert len(visible) == len(hit) and len(albedo) == len(hit) and len(direct) == len(hit)
    rgb = np.tile(miss, (n, 1))
    part = np.zeros((len(hit), 3), dtype=np.float32)
    if len(hit):
        L.ao_ref_colour(len(hit), visible.ctypes.data, int(k), int(sky), albedo.ctypes.data, miss.ctypes.data, direct.ctypes.data, part.ctypes.data)
    rgb[hit] = part
    return rgb
