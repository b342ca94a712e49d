"""directx-raytracer_amd -- Python binding (ctypes) of libcrt_hip.so, the MI355X-native render loop.

The product is the C-ABI shared library (include/crt_hip.h; sources in csrc/).  This module is the thin
test/bench harness on top of it: `Scene` wraps the crt_scene_* scene layer (CRTScene / CRTCamera surface),
`Renderer` wraps the crt_ctx renderer (DXRTRenderer surface: upload, set camera, changeShadingMode, renderFrame).
There is no CPU fallback: if the library or a HIP device is missing, construction raises.

The directory name contains a hyphen, so it is loaded by path (see __graft_entry__.load_package()).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CRT_HIP_LIBRARY") or os.path.join(_HERE, "libcrt_hip.so")  # the override is for A/B builds (tools/variant_build.sh)
MISS = 0xFFFFFFFF
MODE_LAMBERT = 100
MODE_PATH = 200
TILE = 16

NODE_DTYPE = np.dtype([("lx0", "f4"), ("lx1", "f4"), ("ly0", "f4"), ("ly1", "f4"),
                       ("rx0", "f4"), ("rx1", "f4"), ("ry0", "f4"), ("ry1", "f4"),
                       ("lz0", "f4"), ("lz1", "f4"), ("rz0", "f4"), ("rz1", "f4"),
                       ("left", "i4"), ("right", "i4"), ("pad0", "i4"), ("pad1", "i4")])
NODE4_DTYPE = np.dtype([("minx", "f4", 4), ("maxx", "f4", 4), ("miny", "f4", 4), ("maxy", "f4", 4), ("minz", "f4", 4), ("maxz", "f4", 4),
                        ("ref", "i4", 4), ("pad", "i4", 4)])
NODE4Q_DTYPE = np.dtype([("lo", "f4", 3), ("s", "f4", 3), ("qlo_x", "u4"), ("qhi_x", "u4"), ("qlo_y", "u4"), ("qhi_y", "u4"), ("qlo_z", "u4"), ("qhi_z", "u4"), ("ref", "i4", 4)])
assert NODE4Q_DTYPE.itemsize == 64
BVH_EMPTY = -1
TRI_DTYPE = np.dtype([("v0", "f4", 3), ("inst", "u4"), ("e1", "f4", 3), ("prim", "u4"),
                      ("e2", "f4", 3), ("gid", "u4")])
SHADE_DTYPE = np.dtype([("n0", "f4", 3), ("n1", "f4", 3), ("n2", "f4", 3), ("material", "u4"), ("pad", "u4", 2)])


class CrtError(RuntimeError):
    pass


class MeshView(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("idx", C.c_void_p), ("normals", C.c_void_p), ("uvs", C.c_void_p),
                ("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32), ("material_index", C.c_int32)]


class Light(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("intensity", C.c_float)]


class Material(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("type", C.c_uint32), ("smooth", C.c_uint32), ("ior", C.c_float), ("texture", C.c_int32)]


class Texture(C.Structure):
    _fields_ = [("type", C.c_uint32), ("color_a", C.c_float * 3), ("color_b", C.c_float * 3), ("scalar", C.c_float),
                ("pixels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32)]


TEXTURE_TYPES = {"albedo": 0, "edges": 1, "checker": 2, "bitmap": 3}
UV_DTYPE = np.dtype([("uv0", "f4", 2), ("uv1", "f4", 2), ("uv2", "f4", 2)])


class FrameStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("rays_primary", C.c_uint64),
                ("rays_shadow", C.c_uint64), ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


SAMPLE_CENTRE = 0xFFFFFFFF  # CRT_SAMPLE_CENTRE: the pixel-centre camera rays of modes 0..100


class DenoiseParams(C.Structure):
    """crt_denoise_params; the defaults are the header's"""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("demodulate", C.c_uint32)]

    def __init__(self, iterations=5, sigma_color=4.0, sigma_normal=0.3, sigma_depth=0.05, demodulate=1):
        super().__init__(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_depth), int(demodulate))


class TemporalParams(C.Structure):
    """crt_temporal_params; the defaults are the header's"""
    _fields_ = [("alpha", C.c_float), ("depth_tolerance", C.c_float), ("normal_threshold", C.c_float), ("max_history", C.c_uint32),
                ("demodulate", C.c_uint32)]

    def __init__(self, alpha=0.1, depth_tolerance=0.01, normal_threshold=0.9, max_history=64, demodulate=1):
        super().__init__(float(alpha), float(depth_tolerance), float(normal_threshold), int(max_history), int(demodulate))


class TemporalVarianceParams(C.Structure):
    """crt_temporal_variance_params: crt_temporal_params, then alpha_moments and min_history; the defaults are the header's"""
    _fields_ = [("base", TemporalParams), ("alpha_moments", C.c_float), ("min_history", C.c_uint32)]

    def __init__(self, alpha_moments=0.2, min_history=4, **base):
        super().__init__(TemporalParams(**base), float(alpha_moments), int(min_history))


class DenoiseVarianceParams(C.Structure):
    """crt_denoise_variance_params; the defaults are the header's"""
    _fields_ = [("iterations", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("demodulate", C.c_uint32)]

    def __init__(self, iterations=5, sigma_luminance=0.0625, sigma_normal=0.3, sigma_depth=0.05, demodulate=1):
        super().__init__(int(iterations), float(sigma_luminance), float(sigma_normal), float(sigma_depth), int(demodulate))


def build(force=False):
    """Compile libcrt_hip.so (g++ host code + hipcc --offload-arch=gfx950 kernels) in-tree."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", csrc, "-j8", "all"], stdout=subprocess.DEVNULL)
    return LIB_PATH


# ---- the C ABI: every symbol include/crt_hip.h declares -> (restype, argtypes), stated once (tests/test_abi.py checks the table
# against the header and the library); lib() applies it, ABI_SYMBOLS lists it
_vp, _u32, _i32, _flt, _int = C.c_void_p, C.c_uint32, C.c_int32, C.c_float, C.c_int
_ABI = {
    "crt_abi_version": (_u32, []),
    "crt_create": (_int, [C.POINTER(_vp), _int]),
    "crt_destroy": (None, [_vp]),
    "crt_last_error": (C.c_char_p, [_vp]),
    "crt_upload_scene": (_int, [_vp, _vp, _u32, _vp, _u32, _vp, _u32]),
    "crt_set_camera": (_int, [_vp, _vp, _vp]),
    "crt_set_textures": (_int, [_vp, _vp, _u32]),
    "crt_bvh_export_uv": (_int, [_vp, _vp, C.POINTER(_int)]),
    "crt_scene_texture_color": (_int, [_vp, _u32, _flt, _flt, _vp]),
    "crt_scene_add_texture": (_int, [_vp, C.c_char_p, C.c_char_p, _vp, _vp, _flt, C.c_char_p]),
    "crt_scene_set_material_texture": (_int, [_vp, _u32, C.c_char_p]),
    "crt_scene_set_mesh_uvs": (_int, [_vp, _u32, _vp]),
    "crt_set_shading_mode": (_int, [_vp, _u32]),
    "crt_set_miss_color": (_int, [_vp, _vp]),
    "crt_set_counting": (_int, [_vp, _int]),
    "crt_set_option": (_int, [_vp, C.c_char_p, _int]),
    "crt_debug_read_timeline": (_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "crt_debug_read_counters": (_int, [_vp, _vp]),
    "crt_debug_check_rcp": (_int, [_int, _vp]),
    "crt_debug_wide_offsets": (_int, [C.c_ulonglong, C.c_ulonglong, _int]),
    "crt_tile_count": (_u32, [_u32, _u32]),
    "crt_tile_slots": (_u32, [_u32, _u32, _u32]),
    "crt_render_tiles_device": (_int, [_vp, _u32, _u32, _u32, _u32, _vp, _vp]),
    "crt_untile_batch_device": (_int, [_vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "crt_render_frames_batch_device": (_int, [_vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "crt_render_tiles_batch_device": (_int, [_vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "crt_untile_device": (_int, [_vp, _u32, _u32, _u32, _vp, _vp]),
    "crt_set_stream": (_int, [_vp, _vp]),
    "crt_reset_stream": (_int, [_vp]),
    "crt_synchronize": (_int, [_vp]),
    "crt_bvh_info": (_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "crt_bvh_export": (_int, [_vp, _vp, _vp, _vp]),
    "crt_bvh_build_host": (_int, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u32), C.POINTER(_vp), C.POINTER(_vp),
                                  C.POINTER(_u32), C.POINTER(_u32)]),
    "crt_free": (None, [_vp]),
    "crt_host_alloc": (_vp, [C.c_size_t]),
    "crt_host_free": (None, [_vp]),
    "crt_bvh_info4": (_int, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "crt_build_stats": (_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "crt_bvh_export4": (_int, [_vp, _vp]),
    "crt_bvh_export4q": (_int, [_vp, _vp]),
    "crt_bvh_export_planes4q": (_int, [_vp, _vp]),
    "crt_comm_unique_id": (_int, [_vp]),
    "crt_comm_init": (_int, [_vp, _u32, _u32, _vp]),
    "crt_comm_init_host": (_int, [_vp, _u32, _u32, C.c_char_p]),
    "crt_comm_destroy": (_int, [_vp]),
    "crt_comm_info": (_int, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "crt_render_frame_distributed": (_int, [_vp, _u32, _u32, _vp, _vp, C.POINTER(FrameStats)]),
    "crt_bvh_quantize4": (_int, [_vp, _u32, _vp]),
    "crt_bvh_build_host4": (_int, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u32), C.POINTER(_u32)]),
    "crt_scene_load": (_int, [C.c_char_p, C.POINTER(_vp), C.c_char_p, C.c_size_t]),
    "crt_scene_new": (_int, [C.POINTER(_vp)]),
    "crt_scene_save": (_int, [_vp, C.c_char_p, C.c_char_p, C.c_size_t]),
    "crt_scene_free": (None, [_vp]),
    "crt_scene_add_mesh": (_int, [_vp, _vp, _u32, _vp, _u32, _i32]),
    "crt_scene_add_light": (_int, [_vp, _vp, _flt]),
    "crt_scene_add_material": (_int, [_vp, _vp]),
    "crt_scene_mesh_count": (_u32, [_vp]),
    "crt_scene_mesh": (_int, [_vp, _u32, _vp]),
    "crt_scene_light_count": (_u32, [_vp]),
    "crt_scene_light": (_int, [_vp, _u32, _vp]),
    "crt_scene_material_count": (_u32, [_vp]),
    "crt_scene_material": (_int, [_vp, _u32, _vp]),
    "crt_scene_texture_count": (_u32, [_vp]),
    "crt_scene_settings": (_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), _vp]),
    "crt_scene_camera_get": (_int, [_vp, _vp, _vp]),
    "crt_scene_camera_set": (_int, [_vp, _vp, _vp]),
    "crt_scene_camera_rotate": (_int, [_vp, _flt, _flt]),
    "crt_scene_camera_zoom": (_int, [_vp, _flt]),
    "crt_scene_camera_move_forward": (_int, [_vp, _flt]),
    "crt_scene_camera_move_right": (_int, [_vp, _flt]),
    "crt_scene_camera_pan": (_int, [_vp, _flt]),
    "crt_scene_camera_tilt": (_int, [_vp, _flt]),
    "crt_scene_camera_roll": (_int, [_vp, _flt]),
    "crt_scene_camera_pan_around_target": (_int, [_vp, _flt, _vp]),
    "crt_upload_scene_from": (_int, [_vp, _vp]),
    "crt_set_camera_from": (_int, [_vp, _vp]),
    "crt_set_accumulation": (_int, [_vp, _u32]),
    "crt_reset_accumulation": (_int, [_vp]),
    "crt_accumulated_samples": (_int, [_vp, C.POINTER(_u32)]),
    "crt_winding_moments_export": (_int, [_vp, _vp]),
    "crt_set_mesh_transform": (_int, [_vp, _u32, _vp]),
    "crt_refit": (_int, [_vp, C.POINTER(C.c_double)]),
    "crt_mesh_vertices": (_int, [_vp, _u32, _vp, _vp]),
    "crt_rebuild": (_int, [_vp, C.POINTER(C.c_double)]),
    "crt_debug_list_phases": (_int, [_vp, _vp]),
    "crt_motion_snapshot": (_int, [_vp]),
}


def _host_and_device(rows):
    """the entry points that come as crt_x (host buffers) and crt_x_device (device pointers) with one argument list"""
    return {name + suffix: sig for name, sig in rows.items() for suffix in ("", "_device")}


_ABI.update(_host_and_device({
    "crt_render_frame": (_int, [_vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crt_trace_rays": (_int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crt_occluded_rays": (_int, [_vp, _u32, _vp, _vp, _vp]),
    "crt_closest_points": (_int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crt_count_hits": (_int, [_vp, _u32, _vp, _vp, _vp]),
    "crt_occupancy": (_int, [_vp, _u32, _vp, _vp, _vp]),
    "crt_winding_numbers": (_int, [_vp, _u32, _vp, _flt, _vp, _vp]),
    "crt_update_vertices": (_int, [_vp, _u32, _u32, _vp, _vp]),
    "crt_list_hits": (_int, [_vp, _u32, _vp, _vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crt_shade_rays": (_int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crt_path_rays": (_int, [_vp, _u32, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crt_camera_rays": (_int, [_vp, _u32, _u32, _u32, _vp, _vp]),
    "crt_frame_guides": (_int, [_vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "crt_denoise": (_int, [_vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crt_temporal_accumulate": (_int, [_vp, _u32, _u32] + [_vp] * 11),
    "crt_previous_points": (_int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "crt_frame_motion": (_int, [_vp, _u32, _u32, _vp, _vp]),
    "crt_temporal_accumulate_motion": (_int, [_vp, _u32, _u32] + [_vp] * 12),
    "crt_temporal_variance": (_int, [_vp, _u32, _u32] + [_vp] * 15),
    "crt_denoise_variance": (_int, [_vp, _u32, _u32] + [_vp] * 9),
    "crt_trace_rays_backward": (_int, [_vp, _u32] + [_vp] * 10),
    "crt_closest_points_backward": (_int, [_vp, _u32] + [_vp] * 8),
}))
ABI_SYMBOLS = list(_ABI)

_lib = None


def lib():
    """Load the shared library; never builds implicitly and never falls back to anything else."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CrtError("libcrt_hip.so is missing (%s): run __graft_entry__.build() / make -C csrc; "
                       "there is no CPU fallback" % LIB_PATH)
    # One HIP runtime per process: libcrt_hip.so needs libamdhip64.so.7 and takes whichever copy the process has
    # already loaded.  PyTorch bundles its own (torch/lib, same SONAME); if ours (/opt/rocm) were loaded first torch
    # would end up with a mixed runtime and report "No HIP GPUs".  So when torch is around, let it load first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in _ABI.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _f32(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert n is None or a.size == n
    return a


def make_rays(origins, directions, tmin=0.0, tmax=np.inf):
    """(N, 8) float32 ray records {ox, oy, oz, tmin, dx, dy, dz, tmax} for Renderer.trace_rays / occluded.  origins and
    directions are (N, 3) or (3,) (broadcast against each other); tmin / tmax are scalars or length-N arrays."""
    o = np.asarray(origins, dtype=np.float32)
    d = np.asarray(directions, dtype=np.float32)
    if o.shape[-1:] != (3,) or d.shape[-1:] != (3,) or o.ndim > 2 or d.ndim > 2:
        raise ValueError("origins and directions must be (N, 3) or (3,)")
    n = max(o.reshape(-1, 3).shape[0], d.reshape(-1, 3).shape[0])
    o = np.broadcast_to(o.reshape(-1, 3), (n, 3))
    d = np.broadcast_to(d.reshape(-1, 3), (n, 3))
    out = np.empty((n, 8), dtype=np.float32)
    out[:, 0:3] = o
    out[:, 3] = np.broadcast_to(np.asarray(tmin, dtype=np.float32), (n,))
    out[:, 4:7] = d
    out[:, 7] = np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,))
    return out


def _pcg_hash(v):
    """the integer hash of the path tracer's RNG on uint32 arrays"""
    state = v * np.uint32(747796405) + np.uint32(2891336453)
    word = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
    return (word >> np.uint32(22)) ^ word


def path_jitter(ids, sample, seed):
    """(jx, jy), float32 arrays in [0, 1): the two draws the path of (id, sample) takes before its first bounce draw -- in a
    frame the jitter of pixel `id` inside its pixel; Renderer.path_rays leaves them unused (include/crt_hip.h, "sample
    indexing").  ids: uint32 array (or scalar); sample and seed: integers.  Pure numpy."""
    with np.errstate(over="ignore"):
        ids = np.atleast_1d(np.asarray(ids, dtype=np.uint32))
        seed_h = _pcg_hash(np.asarray([int(seed) & 0xFFFFFFFF], dtype=np.uint32))
        st = _pcg_hash(ids ^ _pcg_hash(np.asarray([int(sample) & 0xFFFFFFFF], dtype=np.uint32) + seed_h))
        st = _pcg_hash(st)
        jx = (st >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        st = _pcg_hash(st)
        jy = (st >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return jx, jy


def make_points(xyz, rmax=np.inf):
    """(N, 4) float32 point records {x, y, z, rmax} for Renderer.closest_points / occupancy / signed_distance.  xyz is (N, 3)
    or (3,); rmax is a scalar or a length-N array (the search radius of the closest-point query; occupancy ignores it)."""
    p = np.asarray(xyz, dtype=np.float32)
    if p.shape[-1:] != (3,) or p.ndim > 2:
        raise ValueError("xyz must be (N, 3) or (3,)")
    p = p.reshape(-1, 3)
    n = p.shape[0]
    out = np.empty((n, 4), dtype=np.float32)
    out[:, 0:3] = p
    out[:, 3] = np.broadcast_to(np.asarray(rmax, dtype=np.float32), (n,))
    return out


def tile_count(w, h):
    return ((w + TILE - 1) // TILE) * ((h + TILE - 1) // TILE)


def tile_slots(w, h, n_ranks):
    return (tile_count(w, h) + n_ranks - 1) // n_ranks


def untile_host(gathered, w, h, n_ranks, n_frames=1, frame=0):
    """numpy statement of the tile-major -> row-major de-interleave (crt_untile_device's layout contract):
    gathered = uint32[n_ranks, n_frames, slots, 16, 16]; macro tile k (row-major) of frame f lives at rank k % n_ranks,
    frame f, slot k // n_ranks (n_frames = 1: one frame per all-gather)."""
    slots = tile_slots(w, h, n_ranks)
    g = np.asarray(gathered, dtype=np.uint32).reshape(n_ranks, n_frames, slots, TILE, TILE)[:, frame]
    tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    k = np.arange(tx * ty)
    tiles = g[k % n_ranks, k // n_ranks]                       # [k, 16, 16]
    full = tiles.reshape(ty, tx, TILE, TILE).transpose(0, 2, 1, 3).reshape(ty * TILE, tx * TILE)
    return np.ascontiguousarray(full[:h, :w])


def tile_host(frame_u32, w, h, rank, n_ranks):
    """inverse for one rank: the staging buffer crt_render_tiles_device fills (pixels outside the frame = 0)."""
    slots = tile_slots(w, h, n_ranks)
    tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    pad = np.zeros((ty * TILE, tx * TILE), dtype=np.uint32)
    pad[:h, :w] = np.asarray(frame_u32, dtype=np.uint32).reshape(h, w)
    tiles = pad.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(tx * ty, TILE, TILE)
    out = np.zeros((slots, TILE, TILE), dtype=np.uint32)
    mine = np.arange(rank, tx * ty, n_ranks)
    out[:len(mine)] = tiles[mine]
    return out


class Scene:
    """crt_scene handle: CRTScene / CRTSceneParser / CRTCamera surface (host only, no GPU needed)."""

    def __init__(self, path=None):
        L = lib()
        h = C.c_void_p()
        if path is None:
            rc = L.crt_scene_new(C.byref(h))
            if rc:
                raise CrtError("crt_scene_new rc=%d" % rc)
        else:
            err = C.create_string_buffer(512)
            rc = L.crt_scene_load(os.fsencode(path), C.byref(h), err, len(err))
            if rc:
                raise CrtError("crt_scene_load(%s) rc=%d: %s" % (path, rc, err.value.decode()))
        self.h = h

    @classmethod
    def from_arrays(cls, sc):
        """sc: dict as produced by scenes.py (meshes / lights / materials / camera)."""
        s = cls()
        for m in sc["meshes"]:
            s.add_mesh(m["vertices"], m["triangles"], m.get("material_index", 0))
        for pos, inten in sc.get("lights", []):
            s.add_light(pos, inten)
        for m in sc.get("materials", []):
            s.add_material(m.get("albedo", (1, 1, 1)), m.get("type", 1), m.get("smooth_shading", False), m.get("ior", 1.0))
        for i, m in enumerate(sc["meshes"]):
            if m.get("uvs") is not None:
                s.set_mesh_uvs(i, m["uvs"])
        cam = sc.get("camera")
        if cam is not None:
            s.set_camera(cam["position"], cam["matrix"])
        return s

    def close(self):
        if getattr(self, "h", None):
            lib().crt_scene_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ok(self, rc, what):
        if rc:
            raise CrtError("%s rc=%d" % (what, rc))

    def _call(self, name, *args):
        """the entry point `name` with the scene's handle in front, reported under its own name (the camera methods below report
        under the reference's method names, so they call _ok themselves)"""
        self._ok(getattr(lib(), name)(self.h, *args), name)

    def save(self, path):
        """binary cache (.crtbin)"""
        err = C.create_string_buffer(512)
        rc = lib().crt_scene_save(self.h, os.fsencode(path), err, len(err))
        if rc:
            raise CrtError("crt_scene_save(%s) rc=%d: %s" % (path, rc, err.value.decode()))

    def add_mesh(self, vertices, triangles, material_index=0):
        v = _f32(vertices).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        self._call("crt_scene_add_mesh", v.ctypes.data, len(v), t.ctypes.data, len(t), int(material_index))

    def add_light(self, pos, intensity):
        p = _f32(pos, 3)
        self._call("crt_scene_add_light", p.ctypes.data, float(intensity))

    def add_material(self, albedo=(1, 1, 1), type=1, smooth_shading=False, ior=1.0):
        m = Material((C.c_float * 3)(*[float(x) for x in albedo]), int(type), int(bool(smooth_shading)), float(ior), -1)
        self._call("crt_scene_add_material", C.byref(m))

    def add_texture(self, name, type, color_a=(0, 0, 0), color_b=(0, 0, 0), scalar=0.0, file_path=None):
        a, b = _f32(color_a, 3), _f32(color_b, 3)
        self._call("crt_scene_add_texture", name.encode(), type.encode(), a.ctypes.data, b.ctypes.data, float(scalar),
                   os.fsencode(file_path) if file_path else None)

    def set_material_texture(self, material, texture_name):
        self._call("crt_scene_set_material_texture", int(material), texture_name.encode())

    def set_mesh_uvs(self, mesh, uvs):
        u = _f32(uvs).reshape(-1, 3)
        self._call("crt_scene_set_mesh_uvs", int(mesh), u.ctypes.data)

    def texture_color(self, i, u, v):
        out = np.zeros(3, dtype=np.float32)
        self._call("crt_scene_texture_color", int(i), float(np.float32(u)), float(np.float32(v)), out.ctypes.data)
        return out

    # ---- getters (CRTScene::getObjects / getLights / getMaterials / getTextures / getSettings)
    @property
    def mesh_count(self):
        return lib().crt_scene_mesh_count(self.h)

    def mesh(self, i):
        mv = MeshView()
        self._call("crt_scene_mesh", i, C.byref(mv))

        def arr(ptr, n, dt):
            if not ptr or n == 0:
                return None
            buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt).copy()
        v = arr(mv.xyz, mv.n_vertices * 3, np.float32)
        t = arr(mv.idx, mv.n_triangles * 3, np.uint32)
        n = arr(mv.normals, mv.n_vertices * 3, np.float32)
        uv = arr(mv.uvs, mv.n_vertices * 3, np.float32)
        return {"uvs": uv.reshape(-1, 3) if uv is not None else None, "vertices": v.reshape(-1, 3) if v is not None else np.zeros((0, 3), np.float32),
                "triangles": t.reshape(-1, 3) if t is not None else np.zeros((0, 3), np.uint32),
                "normals": n.reshape(-1, 3) if n is not None else None, "material_index": mv.material_index}

    def meshes(self):
        return [self.mesh(i) for i in range(self.mesh_count)]

    def lights(self):
        out = []
        for i in range(lib().crt_scene_light_count(self.h)):
            l = Light()
            self._call("crt_scene_light", i, C.byref(l))
            out.append((tuple(l.pos), l.intensity))
        return out

    def materials(self):
        out = []
        for i in range(lib().crt_scene_material_count(self.h)):
            m = Material()
            self._call("crt_scene_material", i, C.byref(m))
            out.append({"albedo": tuple(m.albedo), "type": m.type, "smooth_shading": bool(m.smooth), "ior": m.ior, "texture": m.texture})
        return out

    @property
    def texture_count(self):
        return lib().crt_scene_texture_count(self.h)

    def settings(self):
        w, h = C.c_uint32(), C.c_uint32()
        bg = np.zeros(3, dtype=np.float32)
        self._call("crt_scene_settings", C.byref(w), C.byref(h), bg.ctypes.data)
        return {"width": w.value, "height": h.value, "background_color": tuple(bg)}

    # ---- camera (CRTCamera)
    def camera(self):
        pos = np.zeros(3, dtype=np.float32)
        rot = np.zeros(9, dtype=np.float32)
        self._call("crt_scene_camera_get", pos.ctypes.data, rot.ctypes.data)
        return pos, rot

    def set_camera(self, pos=None, rot=None):
        p = _f32(pos, 3) if pos is not None else None
        r = _f32(rot, 9) if rot is not None else None
        self._call("crt_scene_camera_set", p.ctypes.data if p is not None else None, r.ctypes.data if r is not None else None)

    def rotate(self, dyaw, dpitch):
        self._ok(lib().crt_scene_camera_rotate(self.h, dyaw, dpitch), "rotate")

    def zoom(self, a):
        self._ok(lib().crt_scene_camera_zoom(self.h, a), "zoom")

    def move_forward(self, d):
        self._ok(lib().crt_scene_camera_move_forward(self.h, d), "moveForward")

    def move_right(self, d):
        self._ok(lib().crt_scene_camera_move_right(self.h, d), "moveRight")

    def pan(self, deg):
        self._ok(lib().crt_scene_camera_pan(self.h, deg), "pan")

    def tilt(self, deg):
        self._ok(lib().crt_scene_camera_tilt(self.h, deg), "tilt")

    def roll(self, deg):
        self._ok(lib().crt_scene_camera_roll(self.h, deg), "roll")

    def pan_around_target(self, deg, target):
        t = _f32(target, 3)
        self._ok(lib().crt_scene_camera_pan_around_target(self.h, deg, t.ctypes.data), "panAroundTarget")


class TemporalHistory:
    """Frame-to-frame state of Renderer.temporal_accumulate_device: two torch CUDA history buffers of (h, w, 8) float32 that swap
    every push, and the camera of the last push.  The renderer's context keeps none of it.  With variance=True the pushes go
    through Renderer.temporal_variance_device: two (h, w, 2) moment buffers swap beside the history buffers, .variance is the
    (h, w) variance of the last push, and params may hold alpha_moments and min_history too."""

    def __init__(self, renderer, width, height, variance=False, **params):
        import torch
        self.renderer, self.w, self.h, self.params = renderer, int(width), int(height), params
        self.hist = [torch.zeros((self.h, self.w, 8), dtype=torch.float32, device="cuda") for _ in range(2)]
        self.mom = [torch.zeros((self.h, self.w, 2), dtype=torch.float32, device="cuda") for _ in range(2)] if variance else None
        self.variance = torch.zeros((self.h, self.w), dtype=torch.float32, device="cuda") if variance else None
        self.at = 0          # hist[at] holds the previous frame's records
        self.camera = None   # the camera of the previous push; None = no history

    def reset(self):
        """drop the history (after a cut, or after geometry moved when no prev_point is given): the next push starts over"""
        self.camera = None

    def push(self, rgb, normal, albedo, t, camera=None, prev_point=None):
        """rgb, normal, albedo (h, w, 3) and t (h, w): numpy arrays or torch CUDA tensors of this frame; camera: 12 floats
        {pos, rot}, None = the one last given to the renderer's set_camera / set_camera_from; prev_point: None, or the (h, w, 3)
        previous points of this frame (Renderer.frame_motion) when meshes moved.  Returns the accumulated image, of the kind rgb
        is (numpy in, numpy out), and swaps the buffers."""
        import torch
        if camera is None:
            camera = getattr(self.renderer, "camera", None)
            if camera is None:
                raise ValueError("no camera: pass camera= or call the renderer's set_camera first")
        cam = _f32(camera, 12).copy()
        shapes = ((self.h, self.w, 3), (self.h, self.w, 3), (self.h, self.w, 3), (self.h, self.w), (self.h, self.w, 3))
        dev = []
        for a, shape in zip((rgb, normal, albedo, t) + (() if prev_point is None else (prev_point,)), shapes):
            d = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
            if tuple(d.shape) != shape or d.dtype != torch.float32 or not d.is_cuda:
                raise ValueError("expected float32 buffers of shape %r" % (shape,))
            dev.append(d.contiguous())
        out = torch.empty((self.h, self.w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # torch fills its tensors on its own stream
        have = self.camera is not None
        if self.mom is not None:
            self.renderer.temporal_variance_device(self.w, self.h, cam, self.camera if have else cam, dev[0].data_ptr(), dev[1].data_ptr(),
                                                   dev[2].data_ptr(), dev[3].data_ptr(), self.hist[self.at].data_ptr() if have else None,
                                                   self.hist[self.at ^ 1].data_ptr(), self.mom[self.at].data_ptr() if have else None,
                                                   self.mom[self.at ^ 1].data_ptr(), self.variance.data_ptr(), out.data_ptr(),
                                                   d_prev_point=None if prev_point is None else dev[4].data_ptr(), **self.params)
        else:
            self.renderer.temporal_accumulate_device(self.w, self.h, cam, self.camera if have else cam, dev[0].data_ptr(), dev[1].data_ptr(),
                                                     dev[2].data_ptr(), dev[3].data_ptr(), self.hist[self.at].data_ptr() if have else None,
                                                     self.hist[self.at ^ 1].data_ptr(), out.data_ptr(),
                                                     d_prev_point=None if prev_point is None else dev[4].data_ptr(), **self.params)
        self.renderer.synchronize()
        self.at ^= 1
        self.camera = cam
        return out if isinstance(rgb, torch.Tensor) else out.cpu().numpy()

    @property
    def records(self):
        """the history records of the last push, (h, w, 8) torch CUDA tensor {c.rgb, len, n.xyz, t}"""
        return self.hist[self.at]

    @property
    def moments(self):
        """the luminance moments of the last push, (h, w, 2) torch CUDA tensor {m1, m2}; None without variance=True"""
        return None if self.mom is None else self.mom[self.at]


def _mesh_views(meshes, keep):
    arr = (MeshView * max(1, len(meshes)))()
    for i, m in enumerate(meshes):
        v = _f32(m["vertices"]).reshape(-1, 3)
        t = np.ascontiguousarray(m["triangles"], dtype=np.uint32).reshape(-1, 3)
        n = m.get("normals")
        if n is not None:
            n = _f32(n).reshape(-1, 3)
        uv = m.get("uvs")
        if uv is not None:
            uv = _f32(uv).reshape(-1, 3)
        keep += [v, t, n, uv]
        arr[i].xyz = v.ctypes.data
        arr[i].idx = t.ctypes.data
        arr[i].normals = n.ctypes.data if n is not None else None
        arr[i].uvs = uv.ctypes.data if uv is not None else None
        arr[i].n_vertices = len(v)
        arr[i].n_triangles = len(t)
        arr[i].material_index = int(m.get("material_index", 0))
    return arr


def build_bvh_host(meshes):
    """crt_bvh_build_host: the product's BVH builder, host only (no GPU). Returns nodes, tris, shade, max_depth."""
    L = lib()
    keep = []
    mv = _mesh_views(meshes, keep)
    pn, pt, ps = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nn, nt, md = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = L.crt_bvh_build_host(mv, len(meshes), C.byref(pn), C.byref(nn), C.byref(pt), C.byref(ps), C.byref(nt), C.byref(md))
    if rc:
        raise CrtError("crt_bvh_build_host rc=%d: %s" % (rc, L.crt_last_error(None).decode()))

    def take(p, n, dt):
        if n == 0:
            out = np.zeros(0, dtype=dt)
        else:
            out = np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(p.value), dtype=dt).copy()
        L.crt_free(p)
        return out
    return take(pn, nn.value, NODE_DTYPE), take(pt, nt.value, TRI_DTYPE), take(ps, nt.value, SHADE_DTYPE), md.value


def build_bvh4_host(meshes):
    """crt_bvh_build_host4: binary build + collapse to the 4-wide tree the kernels traverse. Returns nodes4, depth4."""
    L = lib()
    keep = []
    mv = _mesh_views(meshes, keep)
    pn, nn, d4 = C.c_void_p(), C.c_uint32(), C.c_uint32()
    rc = L.crt_bvh_build_host4(mv, len(meshes), C.byref(pn), C.byref(nn), C.byref(d4))
    if rc:
        raise CrtError("crt_bvh_build_host4 rc=%d: %s" % (rc, L.crt_last_error(None).decode()))
    out = np.zeros(0, dtype=NODE4_DTYPE) if nn.value == 0 else \
        np.frombuffer((C.c_char * (nn.value * 128)).from_address(pn.value), dtype=NODE4_DTYPE).copy()
    L.crt_free(pn)
    return out, d4.value


def quantize4(nodes4):
    """crt_bvh_quantize4: wide nodes -> the 64-byte quantised nodes the kernels traverse (host only)"""
    nodes4 = np.ascontiguousarray(nodes4, dtype=NODE4_DTYPE)
    out = np.zeros(len(nodes4), dtype=NODE4Q_DTYPE)
    rc = lib().crt_bvh_quantize4(nodes4.ctypes.data, len(nodes4), out.ctypes.data)
    if rc != 0:
        raise CrtError("crt_bvh_quantize4 failed rc=%d" % rc)
    return out


def inside_length(offsets, t):
    """Per ray of a hit list (Renderer.list_hits: offsets (N + 1,), t (total,) ascending inside a ray), the sum over k of
    float64(t[2k+1]) - float64(t[2k]): the length between its 1st and 2nd, 3rd and 4th, ... hit; an odd last hit is ignored.
    (N,) float64, pure numpy."""
    off = np.asarray(offsets, dtype=np.int64)
    t64 = np.asarray(t, dtype=np.float64)
    n = len(off) - 1
    cnt = np.diff(off)
    ray = np.repeat(np.arange(n), cnt)
    k = np.arange(len(t64)) - off[:-1][ray]  # position inside the ray's list
    paired = k < (cnt[ray] & ~1)
    out = np.zeros(n, dtype=np.float64)
    # interval by interval (not a signed sum over all records): t[2k+1] - t[2k] first, then the sum in list order
    hi = paired & ((k & 1) == 1)
    seg = t64[hi] - t64[np.flatnonzero(hi) - 1]
    np.add.at(out, ray[hi], seg)
    return out


_torch_fns = None


def _torch_functions():
    """(ray function, point function): the torch.autograd.Functions behind Renderer.trace_rays_torch / closest_points_torch, made at
    the first call -- torch is not needed to import this package"""
    global _torch_fns
    if _torch_fns is not None:
        return _torch_fns
    import torch

    def records(a, width, what):
        if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and a.dim() == 2 and a.shape[1] == width):
            raise ValueError("%s must be an (N, %d) float32 CUDA tensor" % (what, width))
        return a.detach().contiguous()

    def forward_setup(ctx, renderer, meshes, verts):
        shapes = getattr(renderer, "_mesh_shapes", [])
        if len(set(meshes)) != len(meshes) or any(not 0 <= m < len(shapes) for m in meshes):
            raise ValueError("vertices: the keys must be distinct mesh ordinals of the uploaded scene")
        for m, v in zip(meshes, verts):
            if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (shapes[m][0], 3)):
                raise ValueError("vertices[%d] must be a (%d, 3) float32 CUDA tensor" % (m, shapes[m][0]))
        torch.cuda.current_stream().synchronize()  # the inputs are ready
        for m, v in zip(meshes, verts):
            renderer.update_vertices(m, v.detach().contiguous())
        ctx.renderer, ctx.meshes = renderer, meshes
        ctx.set_materialize_grads(False)

    def ptr(a):
        return None if a is None else a.data_ptr()

    def grad_in(g, like):
        return None if g is None else g.to(torch.float32).expand_as(like).contiguous()

    def vertex_grads(ctx, grad_xyz):
        """per mesh of the forward call the rest-vertex gradient: its rows of grad_xyz times the transposed 3x3 of its transform"""
        r = ctx.renderer
        starts = np.cumsum([0] + [nv for nv, _ in r._mesh_shapes])
        out = []
        for k, m in enumerate(ctx.meshes):
            if grad_xyz is None or not ctx.needs_input_grad[3 + k]:
                out.append(None)
                continue
            g = grad_xyz[starts[m]:starts[m + 1]]
            tr = r._mesh_transforms[m]
            if tr is not None:  # world = M rest + t: dL/drest = M^T dL/dworld, row by row g M
                g = g @ torch.from_numpy(np.ascontiguousarray(tr[:, :3])).to(g.device)
            out.append(g)
        return out

    def check_serial(ctx):
        if ctx.serial != ctx.renderer._geom_serial:
            raise CrtError("backward: the scene's vertices or transforms changed since the forward pass")

    class RayFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, rays, meshes, *verts):
            r = records(rays, 8, "rays")
            forward_setup(ctx, renderer, meshes, verts)
            n = r.shape[0]
            t = torch.empty(n, dtype=torch.float32, device=r.device)
            uv = torch.empty((n, 2), dtype=torch.float32, device=r.device)
            inst = torch.empty(n, dtype=torch.int32, device=r.device)
            prim = torch.empty(n, dtype=torch.int32, device=r.device)
            renderer.trace_rays_device(n, ptr(r), ptr(t), ptr(uv), ptr(inst), ptr(prim))
            renderer.synchronize()
            ctx.serial = renderer._geom_serial
            ctx.save_for_backward(r, t, uv, inst, prim)
            ctx.mark_non_differentiable(inst, prim)
            return t, uv, inst, prim

        @staticmethod
        def backward(ctx, g_t, g_uv, _g_inst, _g_prim):
            r, t, uv, inst, prim = ctx.saved_tensors
            n = r.shape[0]
            none = (None, None, None) + (None,) * len(ctx.meshes)
            want_rays, want_xyz = ctx.needs_input_grad[1], any(ctx.needs_input_grad[3:])
            if (g_t is None and g_uv is None) or not (want_rays or want_xyz):
                return none
            check_serial(ctx)
            g_t, g_uv = grad_in(g_t, t), grad_in(g_uv, uv)
            grad_rays = torch.zeros((n, 8), dtype=torch.float32, device=r.device) if want_rays else None
            grad_xyz = torch.zeros((ctx.renderer._total_vertices(), 3), dtype=torch.float32, device=r.device) if want_xyz else None
            torch.cuda.current_stream().synchronize()  # the incoming gradients are ready
            ctx.renderer.trace_rays_backward_device(n, ptr(r), ptr(inst), ptr(prim), ptr(t), ptr(uv), ptr(g_t), ptr(g_uv), ptr(grad_rays),
                                                    ptr(grad_xyz))
            ctx.renderer.synchronize()
            return (None, grad_rays, None) + tuple(vertex_grads(ctx, grad_xyz))

    class PointFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, points, meshes, *verts):
            p = records(points, 4, "points")
            forward_setup(ctx, renderer, meshes, verts)
            n = p.shape[0]
            dist = torch.empty(n, dtype=torch.float32, device=p.device)
            point = torch.empty((n, 3), dtype=torch.float32, device=p.device)
            uv = torch.empty((n, 2), dtype=torch.float32, device=p.device)
            inst = torch.empty(n, dtype=torch.int32, device=p.device)
            prim = torch.empty(n, dtype=torch.int32, device=p.device)
            renderer.closest_points_device(n, ptr(p), ptr(dist), ptr(point), ptr(uv), ptr(inst), ptr(prim))
            renderer.synchronize()
            ctx.serial = renderer._geom_serial
            ctx.save_for_backward(p, uv, inst, prim)
            ctx.mark_non_differentiable(point, uv, inst, prim)
            return dist, point, uv, inst, prim

        @staticmethod
        def backward(ctx, g_dist, *_rest):
            p, uv, inst, prim = ctx.saved_tensors
            n = p.shape[0]
            none = (None, None, None) + (None,) * len(ctx.meshes)
            want_points, want_xyz = ctx.needs_input_grad[1], any(ctx.needs_input_grad[3:])
            if g_dist is None or not (want_points or want_xyz):
                return none
            check_serial(ctx)
            g_dist = grad_in(g_dist, p[:, 0])
            grad_points = torch.zeros((n, 4), dtype=torch.float32, device=p.device) if want_points else None
            grad_xyz = torch.zeros((ctx.renderer._total_vertices(), 3), dtype=torch.float32, device=p.device) if want_xyz else None
            torch.cuda.current_stream().synchronize()
            ctx.renderer.closest_points_backward_device(n, ptr(p), ptr(inst), ptr(prim), ptr(uv), ptr(g_dist), ptr(grad_points), ptr(grad_xyz))
            ctx.renderer.synchronize()
            return (None, grad_points, None) + tuple(vertex_grads(ctx, grad_xyz))

    _torch_fns = (RayFunction, PointFunction)
    return _torch_fns


# ---- what Renderer's wrappers share: the layout of every output field, and the coercion of every kind of input
# per record of a query (n records) or per pixel of a frame (h x w pixels): the field's trailing shape and its dtype
_FIELDS = {
    "t": ((), np.float32), "uv": ((2,), np.float32), "inst": ((), np.uint32), "prim": ((), np.uint32),
    "rgb": ((3,), np.float32), "normal": ((3,), np.float32), "albedo": ((3,), np.float32),
    "dist": ((), np.float32), "point": ((3,), np.float32),
    "grad_rays": ((8,), np.float32), "grad_points": ((4,), np.float32), "grad_xyz": ((3,), np.float32),
    "hit_inst": ((), np.uint32), "hit_prim": ((), np.uint32), "hit_t": ((), np.float32),
}


def _outputs(keys, want, lead):
    """(out, pointers): out holds a zeroed array of shape lead + the field's for every key of `keys` that is in `want`, in the order of
    `keys`; pointers has one entry per key in that order, the array's address or None (NULL: not wanted)"""
    out = {k: np.zeros(tuple(lead) + _FIELDS[k][0], dtype=_FIELDS[k][1]) for k in keys if k in want}
    return out, [out[k].ctypes.data if k in out else None for k in keys]


def _ptr(a):
    return None if a is None else a.ctypes.data


def _ray_records(rays):
    return np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)


def _point_records(points):
    return np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)


def _points_or_records(points):
    """(N, 4) records as they are, (N, 3) coordinates as records with rmax = inf"""
    pts = np.asarray(points, dtype=np.float32)
    return make_points(pts) if pts.shape[-1:] == (3,) else _point_records(pts)


def _ids(a):
    return np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)


def _sample_index(sample):
    return SAMPLE_CENTRE if sample is None else int(sample)


def _one_per_record(n, what, *arrays):
    """the shared check of the *_backward host forms: every array that is given holds n records"""
    if not all(len(a) == n for a in arrays if a is not None):
        raise ValueError("%s must hold one record per %s" % what)


_FRAME_TRAIL = {"hist_prev": (8,), "mom_prev": (2,), "variance": ()}  # floats per pixel of a frame buffer; every other one has 3


def _frame_buffers(t, optional=(), **buffers):
    """(h, w, t, buffers): t as a contiguous float32 (h, w) plane and every named buffer as contiguous float32 of (h, w) + its
    trailing shape (_FRAME_TRAIL), in the order given; one named in `optional` may be None and stays None"""
    t = np.ascontiguousarray(t, dtype=np.float32)
    if t.ndim != 2:
        raise ValueError("t must be (h, w)")
    got = []
    for name, a in buffers.items():
        if a is not None or name not in optional:
            a = np.ascontiguousarray(a, dtype=np.float32)
            trail = _FRAME_TRAIL.get(name, (3,))
            if a.shape != t.shape + trail:
                raise ValueError("%s must be (h, w%s) where t is (h, w)" % (name, "".join(", %d" % k for k in trail)))
        got.append(a)
    return t.shape[0], t.shape[1], t, got


class Renderer:
    """crt_ctx handle: the DXRTRenderer surface over HIP. Raises CrtError when no MI355X / HIP device is usable."""

    def __init__(self, device=0):
        L = lib()
        h = C.c_void_p()
        rc = L.crt_create(C.byref(h), int(device))
        if rc:
            raise CrtError("crt_create rc=%d: %s" % (rc, L.crt_last_error(None).decode()))
        self.h = h
        self._keep = []
        self._geom_serial = 0  # bumped whenever vertices or transforms may have changed (the torch layer's backward checks it)

    def close(self):
        if getattr(self, "h", None):
            self._free_pinned()
            lib().crt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args, on=None):
        """the entry point `name` with the context's handle in front (on: another handle, a scene's); a return code other than
        zero raises CrtError with the context's last error"""
        rc = getattr(lib(), name)(self.h if on is None else on, *args)
        if rc:
            raise CrtError("%s rc=%d: %s" % (name, rc, lib().crt_last_error(self.h).decode()))

    def _call_stats(self, name, *args, stats=True):
        """_call for an entry point whose last argument is a crt_frame_stats*: NULL unless stats; returns the dict, or None"""
        st = FrameStats() if stats else None
        self._call(name, *args, C.byref(st) if stats else None)
        return st.as_dict() if stats else None

    def set_textures(self, textures):
        """textures: list of dicts {type: albedo|edges|checker|bitmap, color_a, color_b, scalar, pixels (H,W,C uint8)}"""
        keep = []
        arr = (Texture * max(1, len(textures)))()
        for i, t in enumerate(textures):
            arr[i].type = TEXTURE_TYPES[t["type"]]
            arr[i].color_a = (C.c_float * 3)(*[float(c) for c in t.get("color_a", (0, 0, 0))])
            arr[i].color_b = (C.c_float * 3)(*[float(c) for c in t.get("color_b", (0, 0, 0))])
            arr[i].scalar = float(t.get("scalar", 0.0))
            px = t.get("pixels")
            if px is not None:
                px = np.ascontiguousarray(px, dtype=np.uint8)
                keep.append(px)
                arr[i].pixels = px.ctypes.data
                arr[i].height, arr[i].width, arr[i].channels = px.shape
        self._call("crt_set_textures", arr, len(textures))

    def bvh_export_uv(self):
        info = self.bvh_info()
        uv = np.zeros(info["n_tris"], dtype=UV_DTYPE)
        has = C.c_int()
        self._call("crt_bvh_export_uv", uv.ctypes.data, C.byref(has))
        return uv if has.value else None

    def upload(self, meshes, lights=(), materials=(), textures=None, dynamic=False):
        """dynamic=True keeps what update_vertices / set_mesh_transform / refit need (include/crt_hip.h, dynamic geometry)"""
        self.set_option("dynamic", int(bool(dynamic)))
        keep = []
        mv = _mesh_views(meshes, keep)
        larr = (Light * max(1, len(lights)))()
        for i, (p, inten) in enumerate(lights):
            larr[i].pos = (C.c_float * 3)(*[float(x) for x in p])
            larr[i].intensity = float(inten)
        marr = (Material * max(1, len(materials)))()
        for i, m in enumerate(materials):
            marr[i].albedo = (C.c_float * 3)(*[float(x) for x in m.get("albedo", (1, 1, 1))])
            marr[i].type = int(m.get("type", 1))
            marr[i].smooth = int(bool(m.get("smooth_shading", False)))
            marr[i].ior = float(m.get("ior", 1.0))
            marr[i].texture = int(m.get("texture", -1))
        self._call("crt_upload_scene", mv, len(meshes), larr, len(lights), marr, len(materials))
        self._mesh_shapes = [(int(mv[i].n_vertices), bool(mv[i].normals)) for i in range(len(meshes))]
        self._geom_serial += 1
        self._mesh_transforms = [None] * len(meshes)  # per mesh the 3x4 of set_mesh_transform (None = identity), for the torch layer
        self.set_textures(list(textures) if textures else [])

    def upload_scene(self, scene, dynamic=False):
        self.set_option("dynamic", int(bool(dynamic)))
        self._call("crt_upload_scene_from", scene.h)
        shapes = []
        for i in range(scene.mesh_count):
            mv = MeshView()
            self._call("crt_scene_mesh", i, C.byref(mv), on=scene.h)
            shapes.append((int(mv.n_vertices), bool(mv.normals)))
        self._mesh_shapes = shapes
        self._mesh_transforms = [None] * len(shapes)
        self._geom_serial += 1

    # ---- dynamic geometry (include/crt_hip.h): scenes uploaded with dynamic=True
    def update_vertices(self, mesh, xyz, normals=None):
        """new rest vertices (and normals) of a mesh: numpy arrays (host), or contiguous float32 torch tensors on the GPU (device
        form; made ready on the current stream first).  Applied by the next refit."""
        self._geom_serial += 1
        try:
            import torch
            on_device = isinstance(xyz, torch.Tensor) and xyz.is_cuda
        except ImportError:
            on_device = False
        if on_device:
            for a in (xyz, normals):
                if a is not None and (a.dtype != torch.float32 or not a.is_contiguous() or not a.is_cuda or a.numel() % 3):
                    raise ValueError("update_vertices: device arrays must be contiguous float32 CUDA tensors of n x 3 floats")
            torch.cuda.current_stream().synchronize()
            self._call("crt_update_vertices_device", int(mesh), xyz.numel() // 3, xyz.data_ptr(),
                       normals.data_ptr() if normals is not None else None)
            return
        v = _f32(xyz).reshape(-1, 3)
        n = _f32(normals).reshape(-1, 3) if normals is not None else None
        self._call("crt_update_vertices", int(mesh), len(v), v.ctypes.data, _ptr(n))

    def set_mesh_transform(self, mesh, m):
        """m: 3x4 row-major, or 4x4 whose last row is 0 0 0 1; None = identity"""
        if m is None:
            self._call("crt_set_mesh_transform", int(mesh), None)
            self._remember_transform(mesh, None)
            return
        a = np.asarray(m, dtype=np.float32)
        if a.shape == (4, 4):
            if not np.array_equal(a[3], np.float32([0, 0, 0, 1])):
                raise ValueError("set_mesh_transform: a 4x4 matrix must end in the row 0 0 0 1")
            a = a[:3]
        if a.shape != (3, 4):
            raise ValueError("set_mesh_transform: 3x4 or 4x4 matrix expected, got %s" % (a.shape,))
        a = np.ascontiguousarray(a)
        self._call("crt_set_mesh_transform", int(mesh), a.ctypes.data)
        self._remember_transform(mesh, None if np.array_equal(a, np.eye(3, 4, dtype=np.float32)) else a.copy())

    def _remember_transform(self, mesh, m):
        """the Python side's copy of a mesh's 3x4 (None = identity): trace_rays_torch / closest_points_torch turn world-vertex
        gradients into rest-vertex gradients with it"""
        self._geom_serial += 1
        kept = getattr(self, "_mesh_transforms", None)
        if kept is not None and 0 <= int(mesh) < len(kept):
            kept[int(mesh)] = m

    def refit(self):
        """apply pending updates now; returns the refit's device time in ms (0 when nothing was pending)"""
        ms = C.c_double()
        self._call("crt_refit", C.byref(ms))
        return ms.value

    def rebuild(self):
        """apply pending updates and build a new tree on the GPU from the world vertices (builder: option "gpu_builder", 0 = LBVH,
        1 = PLOC); returns the rebuild's device time in ms"""
        ms = C.c_double()
        self._call("crt_rebuild", C.byref(ms))
        return ms.value

    def mesh_vertices(self, mesh):
        """(xyz, normals or None): world-space vertices of a mesh as they are traced, float32 (n, 3)"""
        shapes = getattr(self, "_mesh_shapes", [])
        if not 0 <= int(mesh) < len(shapes):
            raise CrtError("mesh_vertices: mesh %d out of range" % int(mesh))
        nv, has_n = shapes[int(mesh)]
        xyz = np.zeros((nv, 3), dtype=np.float32)
        nrm = np.zeros((nv, 3), dtype=np.float32) if has_n else None
        self._call("crt_mesh_vertices", int(mesh), xyz.ctypes.data, _ptr(nrm))
        return xyz, nrm

    def set_camera(self, pos, rot):
        p, r = _f32(pos, 3), _f32(rot, 9)
        self._call("crt_set_camera", p.ctypes.data, r.ctypes.data)
        self.camera = np.concatenate([p.reshape(3), r.reshape(9)])  # the 12 floats of the batch entry points (TemporalHistory.push)

    def set_camera_from(self, scene):
        self._call("crt_set_camera_from", scene.h)
        self.camera = np.concatenate(scene.camera())

    def change_shading_mode(self, mode):
        self._call("crt_set_shading_mode", int(mode))

    def set_miss_color(self, rgb):
        c = _f32(rgb, 3)
        self._call("crt_set_miss_color", c.ctypes.data)

    def set_counting(self, on):
        self._call("crt_set_counting", int(bool(on)))

    def set_path_params(self, spp=4, max_bounces=3, seed=1234):
        """mode 200 (path tracing) parameters"""
        self.set_option("spp", spp)
        self.set_option("max_bounces", max_bounces)
        self.set_option("seed", seed)

    def set_option(self, name, value):
        self._call("crt_set_option", name.encode(), int(value))

    def set_accumulation(self, max_samples):
        """mode 200: frames add their samples to per-pixel sums while the view holds still, up to max_samples per pixel
        (0 = off); always starts over (include/crt_hip.h)"""
        self._call("crt_set_accumulation", int(max_samples))

    def reset_accumulation(self):
        self._call("crt_reset_accumulation")

    def accumulated_samples(self):
        """samples per pixel in the current sums (0 when accumulation is off or was reset)"""
        n = C.c_uint32()
        self._call("crt_accumulated_samples", C.byref(n))
        return n.value

    # ---- batched ray queries (include/crt_hip.h): records of 8 floats {ox, oy, oz, tmin, dx, dy, dz, tmax}, see make_rays
    def trace_rays(self, rays, want=("t", "uv", "inst", "prim")):
        """closest hit of every ray (host buffers, synchronous).  Returns a dict of the wanted arrays -- t (N,) float32, uv (N, 2)
        float32, inst / prim (N,) uint32 (MISS on a miss, t = the ray's tmax) -- plus 'stats'."""
        r = _ray_records(rays)
        out, ptrs = _outputs(("t", "uv", "inst", "prim"), want, (len(r),))
        out["stats"] = self._call_stats("crt_trace_rays", len(r), r.ctypes.data, *ptrs)
        return out

    def trace_rays_device(self, n, d_rays, d_t=None, d_uv=None, d_inst=None, d_prim=None, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_trace_rays_device", int(n), d_rays, d_t, d_uv, d_inst, d_prim, stats=stats)

    def occluded(self, rays):
        """occlusion of every ray on (tmin, tmax): bool array (host buffers, synchronous)"""
        r = _ray_records(rays)
        out = np.zeros(len(r), dtype=np.bool_)
        self._call("crt_occluded_rays", len(r), r.ctypes.data, out.ctypes.data, None)
        return out

    def occluded_device(self, n, d_rays, d_occluded, stats=False):
        return self._call_stats("crt_occluded_rays_device", int(n), d_rays, d_occluded, stats=stats)

    def count_hits(self, rays):
        """number of triangles every ray crosses in (tmin, tmax): (N,) uint32 (host buffers, synchronous; rays as make_rays)"""
        r = _ray_records(rays)
        out = np.zeros(len(r), dtype=np.uint32)
        self._call("crt_count_hits", len(r), r.ctypes.data, out.ctypes.data, None)
        return out

    def count_hits_device(self, n, d_rays, d_count, stats=False):
        return self._call_stats("crt_count_hits_device", int(n), d_rays, d_count, stats=stats)

    # ---- shaded ray queries (include/crt_hip.h): the closest hit of every record shaded in the current mode (0..100)
    def shade_rays(self, rays, want=("rgb", "normal", "albedo", "t", "uv", "inst", "prim")):
        """colour, shading normal and albedo at the closest hit of every ray (host buffers, synchronous).  Returns a dict of the
        wanted arrays -- rgb / normal / albedo (N, 3) float32 (miss: the miss colour, zero, zero) and the arrays of trace_rays
        -- plus 'stats'."""
        r = _ray_records(rays)
        out, ptrs = _outputs(("rgb", "normal", "albedo", "t", "uv", "inst", "prim"), want, (len(r),))
        out["stats"] = self._call_stats("crt_shade_rays", len(r), r.ctypes.data, *ptrs)
        return out

    def shade_rays_device(self, n, d_rays, d_rgb=None, d_normal=None, d_albedo=None, d_t=None, d_uv=None, d_inst=None, d_prim=None,
                          stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_shade_rays_device", int(n), d_rays, d_rgb, d_normal, d_albedo, d_t, d_uv, d_inst, d_prim, stats=stats)

    # ---- path-traced ray queries (include/crt_hip.h): mode-200 radiance of every record, whatever the current mode
    def path_rays(self, rays, ids=None, first_sample=0, n_samples=1, sums=None, want=("rgb", "t", "uv", "inst", "prim")):
        """the frames' path tracing for caller-supplied rays (host buffers, synchronous): n_samples paths per record, samples
        first_sample .. first_sample + n_samples - 1 of path id ids[i] (None: i).  sums: None, or an (N, 3) float64 array that
        carries the per-record sample sums from call to call (read when first_sample > 0, always written; rgb is then the mean
        over first_sample + n_samples samples).  Returns a dict of the wanted arrays -- rgb (N, 3) float32 and the arrays of
        trace_rays -- plus 'stats'."""
        r = _ray_records(rays)
        n = len(r)
        out, (rgb, *hit) = _outputs(("rgb", "t", "uv", "inst", "prim"), want, (n,))
        i = None
        if ids is not None:
            i = _ids(ids)
            if len(i) != n:
                raise ValueError("ids must hold one uint32 per ray")
        if sums is not None and (not isinstance(sums, np.ndarray) or sums.dtype != np.float64 or sums.shape != (n, 3)
                                 or not sums.flags.c_contiguous or not sums.flags.writeable):
            raise ValueError("sums must be a writeable C-contiguous (N, 3) float64 array")
        out["stats"] = self._call_stats("crt_path_rays", n, r.ctypes.data, _ptr(i), int(first_sample), int(n_samples), rgb, _ptr(sums), *hit)
        return out

    def path_rays_device(self, n, d_rays, d_ids=None, first_sample=0, n_samples=1, d_rgb=None, d_sums=None, d_t=None, d_uv=None,
                         d_inst=None, d_prim=None, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_path_rays_device", int(n), d_rays, d_ids, int(first_sample), int(n_samples), d_rgb, d_sums, d_t, d_uv,
                                d_inst, d_prim, stats=stats)

    # ---- camera rays, guide buffers and the denoiser (include/crt_hip.h)
    def camera_rays(self, w, h, sample=None):
        """the frames' camera rays of a w x h frame as (w * h, 8) float32 records, record py * w + px (host buffer, synchronous).
        sample None: the pixel-centre rays of modes 0..100; an integer below 2^24: the jittered rays a mode-200 frame traces for
        that frame sample index with the context's seed."""
        rays = np.zeros((int(w) * int(h), 8), dtype=np.float32)
        self._call("crt_camera_rays", int(w), int(h), _sample_index(sample), rays.ctypes.data, None)
        return rays

    def camera_rays_device(self, w, h, d_rays, sample=None, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_camera_rays_device", int(w), int(h), _sample_index(sample), d_rays, stats=stats)

    def frame_guides(self, w, h, want=("normal", "albedo", "t")):
        """the guide buffers of a w x h frame (host buffers, synchronous): per pixel the shading normal and the albedo, (h, w, 3)
        float32, and t, (h, w) float32, of the pixel-centre camera ray (miss: zero, zero, 10000), in any shading mode.  Returns a
        dict of the wanted arrays plus 'stats'."""
        w, h = int(w), int(h)
        out, ptrs = _outputs(("normal", "albedo", "t"), want, (h, w))
        out["stats"] = self._call_stats("crt_frame_guides", w, h, *ptrs)
        return out

    def frame_guides_device(self, w, h, d_normal=None, d_albedo=None, d_t=None, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_frame_guides_device", int(w), int(h), d_normal, d_albedo, d_t, stats=stats)

    def denoise(self, rgb, normal, albedo, t, **params):
        """the edge-avoiding a-trous filter (host buffers, synchronous): rgb, normal, albedo (h, w, 3) and t (h, w) float32, e.g. a
        mode-200 frame's 'rgb' and frame_guides' arrays.  params: the fields of DenoiseParams (iterations, sigma_color,
        sigma_normal, sigma_depth, demodulate).  Returns the filtered (h, w, 3) float32 image."""
        h, w, t, (rgb, normal, albedo) = _frame_buffers(t, rgb=rgb, normal=normal, albedo=albedo)
        out = np.zeros((h, w, 3), dtype=np.float32)
        prm = DenoiseParams(**params)
        self._call("crt_denoise", w, h, rgb.ctypes.data, normal.ctypes.data, albedo.ctypes.data, t.ctypes.data, out.ctypes.data,
                   C.byref(prm), None)
        return out

    def denoise_device(self, w, h, d_rgb, d_normal, d_albedo, d_t, d_out, stats=False, **params):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); d_out may equal d_rgb; asynchronous on the context's
        stream unless stats"""
        prm = DenoiseParams(**params)
        return self._call_stats("crt_denoise_device", int(w), int(h), d_rgb, d_normal, d_albedo, d_t, d_out, C.byref(prm), stats=stats)

    # ---- temporal reprojection (include/crt_hip.h): cameras are 12 floats {pos[3], rot3x3 row-major[9]}
    def _temporal(self, name, w, h, cam_cur, cam_prev, pointers, prm, stats):
        """what the temporal entry points share: w, h, the two cameras as 12 floats each, the pointers, the parameter struct, stats"""
        cc, cp = _f32(cam_cur, 12), _f32(cam_prev, 12)
        return self._call_stats(name, int(w), int(h), cc.ctypes.data, cp.ctypes.data, *pointers, C.byref(prm), stats=stats)

    def _temporal_accumulate(self, form, w, h, cam_cur, cam_prev, frame, prev_point, history, stats, params):
        """crt_temporal_accumulate + form ("" or "_device"), or its _motion twin when prev_point is given: frame = the pointers
        rgb, normal, albedo, t; history = hist_prev, hist_next, out; prev_point goes between the two"""
        motion = [] if prev_point is None else [prev_point]
        return self._temporal("crt_temporal_accumulate" + ("_motion" if motion else "") + form, w, h, cam_cur, cam_prev,
                              (*frame, *motion, *history), TemporalParams(**params), stats)

    def temporal_accumulate(self, cam_cur, cam_prev, rgb, normal, albedo, t, hist_prev=None, want_out=True, prev_point=None, **params):
        """one frame blended with the reprojected history (host buffers, synchronous): rgb, normal, albedo (h, w, 3) and t (h, w)
        float32 of this frame (albedo may be None with demodulate=0), hist_prev None or the (h, w, 8) float32 records an earlier
        call returned, taken with camera cam_prev.  prev_point: None, or (h, w, 3) float32 previous points (frame_motion): the
        call then goes to crt_temporal_accumulate_motion.  params: the fields of TemporalParams.  Returns (hist_next, out): the
        new records and the accumulated (h, w, 3) image (None when not want_out)."""
        h, w, t, bufs = _frame_buffers(t, optional=("rgb", "normal", "albedo", "hist_prev", "prev_point"), rgb=rgb, normal=normal,
                                       albedo=albedo, hist_prev=hist_prev, prev_point=prev_point)
        rgb, normal, albedo, hp, pp = map(_ptr, bufs)
        hist = np.zeros((h, w, 8), dtype=np.float32)
        out = np.zeros((h, w, 3), dtype=np.float32) if want_out else None
        self._temporal_accumulate("", w, h, cam_cur, cam_prev, (rgb, normal, albedo, t.ctypes.data), pp, (hp, hist.ctypes.data, _ptr(out)),
                                  False, params)
        return hist, out

    def temporal_accumulate_device(self, w, h, cam_cur, cam_prev, d_rgb, d_normal, d_albedo, d_t, d_hist_prev, d_hist_next, d_out=None,
                                   stats=False, d_prev_point=None, **params):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); the cameras are host arrays of 12 floats; d_hist_prev None =
        no history; d_out may equal d_rgb or be None; d_prev_point: None, or the previous points of the frame
        (frame_motion_device; the call then goes to crt_temporal_accumulate_motion_device); asynchronous on the context's stream
        unless stats"""
        return self._temporal_accumulate("_device", w, h, cam_cur, cam_prev, (d_rgb, d_normal, d_albedo, d_t), d_prev_point,
                                         (d_hist_prev, d_hist_next, d_out), stats, params)

    # ---- variance (include/crt_hip.h): luminance moments beside the history, and the filter their variance steers
    def temporal_variance(self, cam_cur, cam_prev, rgb, normal, albedo, t, hist_prev=None, mom_prev=None, want_out=True, prev_point=None,
                          **params):
        """temporal_accumulate with luminance moments (host buffers, synchronous): mom_prev None or the (h, w, 2) float32 moments
        an earlier call returned, given exactly when hist_prev is.  params: the fields of TemporalVarianceParams (TemporalParams'
        and alpha_moments, min_history).  Returns (hist_next, mom_next, variance, out): (h, w, 8), (h, w, 2), (h, w) and the
        accumulated (h, w, 3) image (None when not want_out)."""
        h, w, t, bufs = _frame_buffers(t, optional=("rgb", "normal", "albedo", "prev_point", "hist_prev", "mom_prev"), rgb=rgb, normal=normal,
                                       albedo=albedo, prev_point=prev_point, hist_prev=hist_prev, mom_prev=mom_prev)
        rgb, normal, albedo, pp, hp, mp = map(_ptr, bufs)
        hist = np.zeros((h, w, 8), dtype=np.float32)
        mom = np.zeros((h, w, 2), dtype=np.float32)
        var = np.zeros((h, w), dtype=np.float32)
        out = np.zeros((h, w, 3), dtype=np.float32) if want_out else None
        self._temporal("crt_temporal_variance", w, h, cam_cur, cam_prev, (rgb, normal, albedo, t.ctypes.data, pp, hp, hist.ctypes.data, mp,
                                                                          mom.ctypes.data, var.ctypes.data, _ptr(out)),
                       TemporalVarianceParams(**params), False)
        return hist, mom, var, out

    def temporal_variance_device(self, w, h, cam_cur, cam_prev, d_rgb, d_normal, d_albedo, d_t, d_hist_prev, d_hist_next, d_mom_prev,
                                 d_mom_next, d_variance, d_out=None, stats=False, d_prev_point=None, **params):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); the cameras are host arrays of 12 floats; d_hist_prev and
        d_mom_prev None = no history; d_out may equal d_rgb or be None; d_prev_point: None, or the previous points of the frame;
        asynchronous on the context's stream unless stats"""
        return self._temporal("crt_temporal_variance_device", w, h, cam_cur, cam_prev, (d_rgb, d_normal, d_albedo, d_t, d_prev_point, d_hist_prev,
                                                                                        d_hist_next, d_mom_prev, d_mom_next, d_variance, d_out),
                              TemporalVarianceParams(**params), stats)

    def denoise_variance(self, rgb, normal, albedo, t, variance, want_variance=False, **params):
        """the a-trous filter with a variance-driven luminance weight (host buffers, synchronous): denoise's buffers and the
        (h, w) float32 variance of temporal_variance.  params: the fields of DenoiseVarianceParams; demodulate must be the
        temporal call's.  Returns the filtered (h, w, 3) float32 image, with want_variance (image, filtered variance)."""
        h, w, t, (rgb, normal, albedo, var) = _frame_buffers(t, rgb=rgb, normal=normal, albedo=albedo, variance=variance)
        out = np.zeros((h, w, 3), dtype=np.float32)
        vout = np.zeros((h, w), dtype=np.float32) if want_variance else None
        prm = DenoiseVarianceParams(**params)
        self._call("crt_denoise_variance", w, h, rgb.ctypes.data, normal.ctypes.data, albedo.ctypes.data, t.ctypes.data, var.ctypes.data,
                   out.ctypes.data, _ptr(vout), C.byref(prm), None)
        return (out, vout) if want_variance else out

    def denoise_variance_device(self, w, h, d_rgb, d_normal, d_albedo, d_t, d_variance, d_out, d_variance_out=None, stats=False, **params):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); d_out may equal d_rgb, d_variance_out may equal d_variance
        or be None; asynchronous on the context's stream unless stats"""
        prm = DenoiseVarianceParams(**params)
        return self._call_stats("crt_denoise_variance_device", int(w), int(h), d_rgb, d_normal, d_albedo, d_t, d_variance, d_out,
                                d_variance_out, C.byref(prm), stats=stats)

    # ---- motion (include/crt_hip.h): previous positions of hits on a dynamic scene whose meshes move
    def motion_snapshot(self):
        """remember the current world vertices as "previous" (after a frame is rendered, before the meshes are moved)"""
        self._call("crt_motion_snapshot")

    def previous_points(self, inst, prim, uv):
        """where the hits (inst, prim, uv) of trace_rays / shade_rays / list_hits were at the last snapshot: (N, 3) float32, NaN
        for a miss and for a triangle that did not move (host buffers, synchronous)"""
        i, q = _ids(inst), _ids(prim)
        u = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        if not len(i) == len(q) == len(u):
            raise ValueError("inst, prim and uv must hold one record per hit")
        out = np.zeros((len(i), 3), dtype=np.float32)
        self._call("crt_previous_points", len(i), i.ctypes.data, q.ctypes.data, u.ctypes.data, out.ctypes.data, None)
        return out

    def previous_points_device(self, n, d_inst, d_prim, d_uv, d_point, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_previous_points_device", int(n), d_inst, d_prim, d_uv, d_point, stats=stats)

    def frame_motion(self, w, h):
        """the previous points of a w x h frame's pixel-centre camera rays, (h, w, 3) float32: what temporal_accumulate and
        TemporalHistory.push take as prev_point (host buffer, synchronous)"""
        out = np.zeros((int(h), int(w), 3), dtype=np.float32)
        self._call("crt_frame_motion", int(w), int(h), out.ctypes.data, None)
        return out

    def frame_motion_device(self, w, h, d_prev_point, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_frame_motion_device", int(w), int(h), d_prev_point, stats=stats)

    # ---- point queries (include/crt_hip.h): records of 4 floats {x, y, z, rmax}, see make_points
    def closest_points(self, points, want=("dist", "point", "uv", "inst", "prim")):
        """closest surface point of every point within its rmax (host buffers, synchronous).  Returns a dict of the wanted
        arrays -- dist (N,) float32, point (N, 3) float32, uv (N, 2) float32, inst / prim (N,) uint32 (MISS on a miss, dist =
        the record's rmax, point = the query point) -- plus 'stats'."""
        pts = _point_records(points)
        out, ptrs = _outputs(("dist", "point", "uv", "inst", "prim"), want, (len(pts),))
        out["stats"] = self._call_stats("crt_closest_points", len(pts), pts.ctypes.data, *ptrs)
        return out

    def closest_points_device(self, n, d_points, d_dist=None, d_point=None, d_uv=None, d_inst=None, d_prim=None, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_closest_points_device", int(n), d_points, d_dist, d_point, d_uv, d_inst, d_prim, stats=stats)

    def occupancy(self, points):
        """inside / outside of every point (majority of three crossing parities): (N,) bool (host buffers, synchronous).
        points: (N, 4) records (make_points) or (N, 3) coordinates."""
        pts = _points_or_records(points)
        out = np.zeros(len(pts), dtype=np.bool_)
        self._call("crt_occupancy", len(pts), pts.ctypes.data, out.ctypes.data, None)
        return out

    def occupancy_device(self, n, d_points, d_inside, stats=False):
        return self._call_stats("crt_occupancy_device", int(n), d_points, d_inside, stats=stats)

    def signed_distance(self, points, sign="parity", beta=2.0, threshold=0.5):
        """distance to the closest surface point, negated where the point is inside: (N,) float32.  sign = "parity": inside by
        occupancy (closed meshes); "winding": inside by inside_winding(points, beta, threshold) (open meshes and soups too).
        points: (N, 4) records (make_points; rmax bounds the search) or (N, 3) coordinates (rmax = inf)."""
        if sign not in ("parity", "winding"):
            raise ValueError("sign must be 'parity' or 'winding'")
        pts = _points_or_records(points)
        d = self.closest_points(pts, want=("dist",))["dist"]
        inside = self.occupancy(pts) if sign == "parity" else self.inside_winding(pts, beta, threshold)
        return np.where(inside, -d, d).astype(np.float32)

    # ---- winding numbers (include/crt_hip.h): the inside test for open meshes and triangle soups
    def winding_numbers(self, points, beta=2.0):
        """generalised winding number of every point: (N,) float32 (host buffers, synchronous).  beta > 0: clusters farther than
        beta x their radius are taken by their dipole; beta <= 0: exact, the sum over every triangle.
        points: (N, 4) records (make_points; rmax is ignored) or (N, 3) coordinates."""
        pts = _points_or_records(points)
        out = np.zeros(len(pts), dtype=np.float32)
        self._call("crt_winding_numbers", len(pts), pts.ctypes.data, float(beta), out.ctypes.data, None)
        return out

    def winding_numbers_device(self, n, d_points, d_w, beta=2.0, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_winding_numbers_device", int(n), d_points, float(beta), d_w, stats=stats)

    def winding_moments(self):
        """the moment table the winding walk reads: (n_nodes4, 32) float32, {p~, r} of child slots 0..3, then {N~, 0} of slots 0..3"""
        n4 = C.c_uint32(0)
        self._call("crt_bvh_info4", C.byref(n4), None)
        out = np.zeros((n4.value, 32), dtype=np.float32)
        if n4.value:
            self._call("crt_winding_moments_export", out.ctypes.data)
        return out

    def inside_winding(self, points, beta=2.0, threshold=0.5):
        """inside / outside of every point by its winding number: (N,) bool, winding_numbers(points, beta) > threshold"""
        return self.winding_numbers(points, beta) > np.float32(threshold)

    # ---- gradients (include/crt_hip.h, "gradients"): the backward pass of trace_rays and closest_points; dynamic scenes only
    def _total_vertices(self):
        return sum(nv for nv, _ in getattr(self, "_mesh_shapes", []))

    def _grad_outputs(self, per_record, n, want):
        """_outputs of the two gradients of a *_backward host form: `per_record` over n records, grad_xyz over all vertices"""
        out, ptrs = _outputs((per_record,), want, (n,))
        xyz, xyz_ptrs = _outputs(("grad_xyz",), want, (self._total_vertices(),))
        return {**out, **xyz}, ptrs + xyz_ptrs

    def trace_rays_backward(self, rays, inst, prim, t, uv, grad_t=None, grad_uv=None, want=("grad_rays", "grad_xyz")):
        """gradients of a loss on the hits (inst, prim, t, uv) of `rays` (host buffers, synchronous).  grad_t (N,) and grad_uv
        (N, 2) are dL/dt and dL/d(u, v); one of them may be None (zeros).  Returns a dict of the wanted arrays: grad_rays (N, 8)
        float32 {dL/do, 0, dL/dd, 0} and grad_xyz (total vertices, 3) float32, the gradient with respect to the world vertices of
        all meshes back to back in upload order."""
        r = _ray_records(rays)
        n = len(r)
        i, q = _ids(inst), _ids(prim)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
        u = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        gt = None if grad_t is None else np.ascontiguousarray(grad_t, dtype=np.float32).reshape(-1)
        gu = None if grad_uv is None else np.ascontiguousarray(grad_uv, dtype=np.float32).reshape(-1, 2)
        _one_per_record(n, ("rays, inst, prim, t, uv and the gradients", "ray"), i, q, tt, u, gt, gu)
        out, ptrs = self._grad_outputs("grad_rays", n, want)
        self._call("crt_trace_rays_backward", n, r.ctypes.data, i.ctypes.data, q.ctypes.data, tt.ctypes.data, u.ctypes.data, _ptr(gt), _ptr(gu),
                   *ptrs, None)
        return out

    def trace_rays_backward_device(self, n, d_rays, d_inst, d_prim, d_t, d_uv, d_grad_t=None, d_grad_uv=None, d_grad_rays=None, d_grad_xyz=None,
                                   stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_trace_rays_backward_device", int(n), d_rays, d_inst, d_prim, d_t, d_uv, d_grad_t, d_grad_uv, d_grad_rays,
                                d_grad_xyz, stats=stats)

    def closest_points_backward(self, points, inst, prim, uv, grad_dist, want=("grad_points", "grad_xyz")):
        """gradients of a loss on the distances of `points` to their closest surface points (inst, prim, uv) (host buffers,
        synchronous).  grad_dist (N,) is dL/ddist.  Returns a dict of the wanted arrays: grad_points (N, 4) float32 {dL/dp, 0} and
        grad_xyz as trace_rays_backward."""
        pts = _point_records(points)
        n = len(pts)
        i, q = _ids(inst), _ids(prim)
        u = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        g = np.ascontiguousarray(grad_dist, dtype=np.float32).reshape(-1)
        _one_per_record(n, ("points, inst, prim, uv and grad_dist", "point"), i, q, u, g)
        out, ptrs = self._grad_outputs("grad_points", n, want)
        self._call("crt_closest_points_backward", n, pts.ctypes.data, i.ctypes.data, q.ctypes.data, u.ctypes.data, g.ctypes.data, *ptrs, None)
        return out

    def closest_points_backward_device(self, n, d_points, d_inst, d_prim, d_uv, d_grad_dist, d_grad_points=None, d_grad_xyz=None, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); asynchronous on the context's stream unless stats"""
        return self._call_stats("crt_closest_points_backward_device", int(n), d_points, d_inst, d_prim, d_uv, d_grad_dist, d_grad_points,
                                d_grad_xyz, stats=stats)

    def trace_rays_torch(self, rays, vertices):
        """trace_rays with a torch.autograd graph behind it.  rays: (N, 8) float32 CUDA tensor (may require grad); vertices: dict
        {mesh: (nv, 3) float32 CUDA tensor} of REST vertices (may require grad); the scene was uploaded with dynamic=True.  The
        forward pass hands every entry to update_vertices and traces; it returns (t, uv, inst, prim): t (N,) and uv (N, 2) carry
        the graph, inst / prim are int32 (a miss reads -1, t = the ray's tmax) and do not.  backward() gives the rays' gradient
        (tmin / tmax columns zero) and, per mesh named in `vertices`, the gradient with respect to its rest vertices (the world
        gradient times the transposed 3x3 of the mesh's transform).  Misses get zero gradient.  Call backward() before the
        vertices or transforms change again: it reads the scene as it stands."""
        return _torch_functions()[0].apply(self, rays, tuple(int(m) for m in vertices), *vertices.values())

    def closest_points_torch(self, points, vertices):
        """closest_points with a torch.autograd graph behind it.  points: (N, 4) float32 CUDA tensor {x, y, z, rmax} (may require
        grad); vertices as trace_rays_torch.  Returns (dist, point, uv, inst, prim); only dist carries the graph (multiply it by a
        constant sign for a signed distance).  backward() gives the points' gradient (rmax column zero) and the rest-vertex
        gradients as trace_rays_torch."""
        return _torch_functions()[1].apply(self, points, tuple(int(m) for m in vertices), *vertices.values())

    # ---- all-hits ray queries (include/crt_hip.h): every crossing of a ray as a CSR list sorted by distance
    def list_hits(self, rays, want=("t", "uv", "inst", "prim"), capacity=None):
        """every triangle each ray crosses in (tmin, tmax), in ascending t (host buffers, synchronous).  Returns a dict:
        offsets (N + 1,) int64 -- the hits of ray i are records offsets[i] .. offsets[i + 1] - 1 --, ray (total,) uint32 (the ray
        of every record), the wanted arrays t (total,) float32, uv (total, 2) float32, inst / prim (total,) uint32, and 'stats'
        of the last call.  Without `capacity` one offsets-only call learns the total first; with it that call is made only
        when the guess was too small."""
        r = _ray_records(rays)
        n = len(r)
        off = np.zeros(n + 1, dtype=np.uint64)
        tot = C.c_uint64(0)
        st = FrameStats()
        keys = ("t", "uv", "inst", "prim")
        wanted = [k for k in keys if k in want]

        def call(cap, want):
            out, ptrs = _outputs(keys, want, (cap,))
            self._call("crt_list_hits", n, r.ctypes.data, off.ctypes.data, cap, *ptrs, C.byref(tot), C.byref(st))
            return out
        out = {}
        if capacity is None or not wanted:
            call(0, ())
            capacity = tot.value
        if wanted:
            out = call(int(capacity), wanted)
            if tot.value > capacity:  # the guess was too small
                out = call(tot.value, wanted)
            out = {k: v[:tot.value] for k, v in out.items()}
        out["offsets"] = off.astype(np.int64)
        out["ray"] = np.repeat(np.arange(n, dtype=np.uint32), np.diff(out["offsets"]))
        out["stats"] = st.as_dict()
        return out

    def list_hits_device(self, n, d_rays, d_offsets, capacity, d_t=None, d_uv=None, d_inst=None, d_prim=None, total=False, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr()); d_offsets holds n + 1 int64.  Asynchronous on the
        context's stream unless total or stats.  Returns None, the total, the stats, or (total, stats)."""
        tot = C.c_uint64(0) if total else None
        st = self._call_stats("crt_list_hits_device", int(n), d_rays, d_offsets, int(capacity), d_t, d_uv, d_inst, d_prim,
                              C.byref(tot) if total else None, stats=stats)
        if total and stats:
            return tot.value, st
        return tot.value if total else st

    def list_phases(self):
        """HIP-event ms of count / scan / fill / sort of the last list_hits* call that was given stats"""
        buf = np.zeros(4, dtype=np.float64)
        self._call("crt_debug_list_phases", buf.ctypes.data)
        return dict(zip(("count", "scan", "fill", "sort"), buf.tolist()))

    def inside_length(self, rays):
        """per ray, the length (in units of |d|) between its 1st and 2nd, 3rd and 4th, ... hit: the chord through closed meshes"""
        got = self.list_hits(rays, want=("t",))
        return inside_length(got["offsets"], got["t"])

    def read_counters(self):
        buf = np.zeros(32, dtype=np.uint64)
        self._call("crt_debug_read_counters", buf.ctypes.data)
        return buf

    def read_timeline(self, max_words=1 << 22):
        buf = np.zeros(max_words, dtype=np.uint64)
        n = C.c_size_t()
        self._call("crt_debug_read_timeline", buf.ctypes.data, max_words, C.byref(n))
        return buf[:n.value].reshape(-1, 3)

    def set_stream(self, stream_ptr):
        """run on an external hipStream_t handle (0 / None = HIP's default stream, which is torch's default)"""
        self._call("crt_set_stream", stream_ptr)

    def reset_stream(self):
        self._call("crt_reset_stream")

    def synchronize(self):
        self._call("crt_synchronize")

    def bvh_info(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._call("crt_bvh_info", C.byref(a), C.byref(b), C.byref(c))
        return {"n_nodes": a.value, "n_tris": b.value, "max_depth": c.value}

    def bvh_export(self):
        info = self.bvh_info()
        nodes = np.zeros(info["n_nodes"], dtype=NODE_DTYPE)
        tris = np.zeros(info["n_tris"], dtype=TRI_DTYPE)
        shade = np.zeros(info["n_tris"], dtype=SHADE_DTYPE)
        self._call("crt_bvh_export", nodes.ctypes.data, tris.ctypes.data, shade.ctypes.data)
        return nodes, tris, shade

    def build_stats(self):
        a, b = C.c_double(), C.c_double()
        self._call("crt_build_stats", C.byref(a), C.byref(b))
        return {"upload_ms": a.value, "device_build_ms": b.value}

    def bvh_export4(self):
        a, b = C.c_uint32(), C.c_uint32()
        self._call("crt_bvh_info4", C.byref(a), C.byref(b))
        nodes4 = np.zeros(a.value, dtype=NODE4_DTYPE)
        self._call("crt_bvh_export4", nodes4.ctypes.data)
        return nodes4, b.value

    # native RCCL frame assembly (crt_comm_*): no torch involved
    def comm_init(self, rank, n_ranks, unique_id=None):
        """rank 0 may pass unique_id=None to create one; returns the 128-byte id (to be handed to the other ranks)"""
        if unique_id is None:
            buf = C.create_string_buffer(128)
            rc = lib().crt_comm_unique_id(buf)
            if rc != 0:
                raise CrtError("crt_comm_unique_id failed rc=%d: %s" % (rc, lib().crt_last_error(None).decode()))
            unique_id = buf.raw
        self._call("crt_comm_init", rank, n_ranks, C.create_string_buffer(unique_id, 128))
        return unique_id

    def comm_init_host(self, rank, n_ranks, name):
        """the same frame assembly with a POSIX shared-memory object ("/name") as the transport: ranks that share one GPU (rehearsal)"""
        self._call("crt_comm_init_host", rank, n_ranks, name.encode())

    def comm_destroy(self):
        self._call("crt_comm_destroy")

    def render_frame_distributed(self, w, h, d_rgba8=None, host=False, stats=False):
        out = np.zeros((h, w, 4), dtype=np.uint8) if host else None
        st = FrameStats()
        self._call("crt_render_frame_distributed", w, h, d_rgba8, _ptr(out), C.byref(st) if stats else None)
        res = {"stats": st.as_dict()} if stats else {}
        if host:
            res["rgba8"] = out
        return res

    def bvh_export4q(self):
        """the quantised 64-byte nodes as they sit in HBM"""
        a = C.c_uint32()
        self._call("crt_bvh_info4", C.byref(a), None)
        q = np.zeros(a.value, dtype=NODE4Q_DTYPE)
        self._call("crt_bvh_export4q", q.ctypes.data)
        return q

    def bvh_export_planes4q(self):
        """the decoded plane table: one row of 32 floats per quantised node, float(q) of its 24 plane bytes + 8 zeros"""
        a = C.c_uint32()
        self._call("crt_bvh_info4", C.byref(a), None)
        p = np.zeros((a.value, 32), dtype=np.float32)
        self._call("crt_bvh_export_planes4q", p.ctypes.data)
        return p

    def pinned_frame(self, w, h):
        """RGBA8 frame buffer in page-locked host memory (crt_host_alloc), reused across calls of render_frame(pinned=True)."""
        key = (w, h)
        if getattr(self, "_pinned_key", None) != key:
            self._free_pinned()
            ptr = lib().crt_host_alloc(w * h * 4)
            if not ptr:
                raise CrtError("crt_host_alloc failed")
            self._pinned_ptr, self._pinned_key = ptr, key
            self._pinned = np.ctypeslib.as_array((C.c_uint8 * (w * h * 4)).from_address(ptr)).reshape(h, w, 4)
        return self._pinned

    def _free_pinned(self):
        if getattr(self, "_pinned_ptr", None):
            self._pinned = None
            lib().crt_host_free(self._pinned_ptr)
            self._pinned_ptr, self._pinned_key = None, None

    def render_frame(self, w, h, want=("rgba8", "hit_inst", "hit_prim", "hit_t", "rgb"), pinned=False):
        """renderFrame with host outputs. Returns dict of arrays + 'stats'. pinned=True: rgba8 lands in a reused page-locked
        buffer (valid until the next such call)."""
        rgba8 = self.pinned_frame(w, h) if pinned else np.zeros((h, w, 4), dtype=np.uint8)  # always filled, wanted or not
        out, ptrs = _outputs(("hit_inst", "hit_prim", "hit_t", "rgb"), want, (h, w))
        out = {"rgba8": rgba8, **out}
        out["stats"] = self._call_stats("crt_render_frame", w, h, rgba8.ctypes.data, *ptrs)
        return out

    def render_frame_device(self, w, h, d_rgba8, d_hit_inst=None, d_hit_prim=None, d_hit_t=None, d_rgb=None, stats=False):
        """device pointers are integers (e.g. torch.Tensor.data_ptr())."""
        return self._call_stats("crt_render_frame_device", w, h, d_rgba8, d_hit_inst, d_hit_prim, d_hit_t, d_rgb, stats=stats)

    def render_tiles_device(self, w, h, rank, n_ranks, d_staging, stats=False):
        return self._call_stats("crt_render_tiles_device", w, h, rank, n_ranks, d_staging, stats=stats)

    @staticmethod
    def _batch_args(cameras, d_out):
        n = len(d_out)
        outs = (C.c_void_p * n)(*[int(x) for x in d_out])
        cams = None
        if cameras is not None:
            cams = np.ascontiguousarray(np.concatenate([np.concatenate([_f32(p, 3), _f32(r, 9)]) for p, r in cameras]), dtype=np.float32)
            assert cams.size == 12 * n
        return n, cams, outs

    def render_frames_batch_device(self, w, h, d_rgba8_list, cameras=None, stats=False):
        """several frames in ONE launch; cameras = [(pos, rot3x3), ...] per frame or None (current camera for all)."""
        n, cams, outs = self._batch_args(cameras, d_rgba8_list)
        return self._call_stats("crt_render_frames_batch_device", w, h, n, _ptr(cams), outs, stats=stats)

    def render_tiles_batch_device(self, w, h, rank, n_ranks, d_staging_list, cameras=None, stats=False):
        n, cams, outs = self._batch_args(cameras, d_staging_list)
        return self._call_stats("crt_render_tiles_batch_device", w, h, rank, n_ranks, n, _ptr(cams), outs, stats=stats)

    def untile_batch_device(self, w, h, n_ranks, n_frames, frame, d_gathered, d_frame):
        self._call("crt_untile_batch_device", w, h, n_ranks, n_frames, frame, d_gathered, d_frame)

    def untile_device(self, w, h, n_ranks, d_gathered, d_frame):
        self._call("crt_untile_device", w, h, n_ranks, d_gathered, d_frame)
