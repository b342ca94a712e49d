"""Snapshot of the Python binding for tests/test_binding_surface.py; no GPU involved.

snapshot(pkg, install) returns three sections:

  surface  every public name of the package: its kind, constants by value (ABI_SYMBOLS as a sorted list: its order carries no
           meaning; LIB_PATH as present only), numpy dtypes by descr, ctypes structures by field names and types, functions and
           the public methods and properties of every class (__init__ included) by signature and a hash of the docstring
  abi      per symbol of the header the names of the restype and argtypes lib() set on the real library
  calls    a fixed script of Renderer calls made against a stand-in for the library that records every C call: the symbol, and
           per argument a scalar / bytes / NULL verbatim, a byref as the type it refers to (a parameter struct with its field
           values), a host address as in:<argument> or out:<key> of the arrays that went in and came back, tmp otherwise; then
           the layout of what the wrapper returned, or the type of what it raised

The stand-in returns 0 from every call, b"" from crt_last_error and a buffer it keeps from crt_host_alloc; it writes 3 into every
integer and 1.5 into every double it is handed by reference, so that wrappers which size their outputs from such a value go on
(crt_list_hits also gets offsets that agree with that total).
Handles stay NULL: close() and __del__ never reach the real crt_destroy.

    python tests/binding_pin.py --write     rewrites tests/golden/binding_surface.json
"""
import ctypes as C
import hashlib
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "binding_surface.json")
N, W, H = 3, 4, 3   # records per query, frame width and height of the script
NOT_SCRIPTED = {"trace_rays_torch", "closest_points_torch"}   # they take CUDA tensors: the GPU suite has them
# these compute their result from what other wrappers returned: none of its arrays was handed to C, so an address of theirs that
# is no input is tmp (a result allocated after the C calls may sit where a buffer of those calls was freed)
DERIVED = {"signed_distance", "inside_winding", "inside_length"}


# ---------------------------------------------------------------- surface
def _doc(o):
    return hashlib.sha1((o.__doc__ or "").encode()).hexdigest()[:12]


def _function(f):
    return {"signature": str(inspect.signature(f)), "doc": _doc(f)}


def _members(cls):
    out = {}
    for name, v in vars(cls).items():
        if name.startswith("_") and name != "__init__":
            continue
        if isinstance(v, (staticmethod, classmethod)):
            out[name] = dict(_function(v.__func__), kind=type(v).__name__)
        elif isinstance(v, property):
            out[name] = {"kind": "property", "doc": _doc(v)}
        elif inspect.isfunction(v):
            out[name] = dict(_function(v), kind="method")
    return out


def _plain(v):
    """tuples as lists, all the way down (what JSON would make of them anyway)"""
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    return v


def surface(pkg):
    out = {}
    for name in sorted(n for n in vars(pkg) if not n.startswith("_")):
        v = getattr(pkg, name)
        if name == "LIB_PATH":
            out[name] = {"kind": type(v).__name__, "present": True}
        elif name == "ABI_SYMBOLS":
            out[name] = {"kind": type(v).__name__, "sorted": sorted(v)}
        elif inspect.ismodule(v):
            out[name] = {"kind": "module", "module": v.__name__}
        elif isinstance(v, np.dtype):
            out[name] = {"kind": "dtype", "descr": _plain(v.descr), "itemsize": v.itemsize}
        elif inspect.isclass(v):
            out[name] = {"kind": "class", "bases": [b.__name__ for b in v.__bases__], "doc": _doc(v), "members": _members(v)}
            if issubclass(v, C.Structure):
                out[name]["fields"] = [[f[0], f[1].__name__] for f in v._fields_]
        elif inspect.isfunction(v):
            out[name] = dict(_function(v), kind="function")
        else:
            out[name] = {"kind": type(v).__name__, "value": _plain(v)}
    return out


def abi(pkg):
    L = pkg.lib()

    def name(t):
        return "None" if t is None else t.__name__
    return {s: {"restype": name(getattr(L, s).restype), "argtypes": [name(t) for t in getattr(L, s).argtypes]} for s in pkg.ABI_SYMBOLS}


# ---------------------------------------------------------------- the stand-in
class _Addr(int):
    """a host address among recorded arguments, named once the call has returned"""


def _scalar(v):
    if v is None:
        return "NULL"
    if isinstance(v, int) and not isinstance(v, bool) and v >= 1 << 16 and v != 0xFFFFFFFF:
        return _Addr(v)   # the script's own integers are small, but for CRT_SAMPLE_CENTRE; no array sits at that odd address
    if isinstance(v, np.generic):
        return "%s:%r" % (type(v).__name__, v.item())
    return repr(v)


def _ctypes_value(o):
    t = type(o).__name__
    if isinstance(o, C.Structure):
        return [t, [[f[0], _ctypes_value(getattr(o, f[0])) if isinstance(getattr(o, f[0]), (C.Structure, C.Array)) else _scalar(getattr(o, f[0]))]
                    for f in o._fields_]]
    if isinstance(o, C.Array):
        if issubclass(o._type_, C.c_char):
            return [t, hashlib.sha1(o.raw).hexdigest()[:12]]
        return [t, [_ctypes_value(x) if isinstance(x, (C.Structure, C.Array)) else _scalar(x) for x in o]]
    return [t, _scalar(o.value)]


def _encode(a):
    """one argument of a C call, as it stands while the call is made"""
    if type(a).__name__ == "CArgObject":   # C.byref(...)
        o = a._obj
        if isinstance(o, C.Structure) and "__init__" in vars(type(o)):   # a parameter struct: its values are input
            return ["byref"] + _ctypes_value(o)
        return "byref:" + type(o).__name__
    if isinstance(a, (C.Structure, C.Array, C._SimpleCData)):
        return _ctypes_value(a)
    return _scalar(a)


class Recorder:
    """stands in for the loaded library: every crt_* attribute is a function that records its call"""

    def __init__(self):
        self.log = []
        self.buffers = []

    def __getattr__(self, symbol):
        if not symbol.startswith("crt_"):
            raise AttributeError(symbol)

        def fn(*args):
            self.log.append([symbol, [_encode(a) for a in args]])
            for a in args:
                o = getattr(a, "_obj", None) if type(a).__name__ == "CArgObject" else None
                if isinstance(o, (C.c_uint32, C.c_uint64, C.c_int32, C.c_size_t)):
                    o.value = 3
                elif isinstance(o, C.c_double):
                    o.value = 1.5
            if symbol == "crt_list_hits":   # offsets that agree with the total of 3: every hit on the last ray
                (C.c_uint64 * (args[1] + 1)).from_address(args[3])[args[1]] = 3
            if symbol == "crt_last_error":
                return b""
            if symbol == "crt_host_alloc":
                self.buffers.append(C.create_string_buffer(args[0]))
                return C.addressof(self.buffers[-1])
            return 0
        return fn


# ---------------------------------------------------------------- the script
def _arrays(path, v, out):
    if isinstance(v, np.ndarray):
        out[v.ctypes.data] = path
    elif isinstance(v, dict):
        for k, x in v.items():
            _arrays("%s.%s" % (path, k) if path else str(k), x, out)
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            _arrays("%s[%d]" % (path, i), x, out)


def _named(v, names):
    if isinstance(v, _Addr):
        return names.get(int(v), "tmp")
    if isinstance(v, list):
        return [_named(x, names) for x in v]
    return v


def _layout(v):
    if isinstance(v, np.ndarray):
        return "ndarray %s %r" % (v.dtype.name, v.shape)
    if isinstance(v, dict):
        return ["dict"] + [[k, _layout(x)] for k, x in v.items()]   # a list: the key order is part of the surface
    if isinstance(v, (list, tuple)):
        return [type(v).__name__] + [_layout(x) for x in v]
    if isinstance(v, (bytes, str, bool)) or v is None:
        return repr(v)
    return "%s %r" % (type(v).__name__, v)


def _given(v):
    if isinstance(v, np.ndarray):
        return "ndarray %s %r" % (v.dtype.name, v.shape)
    if isinstance(v, dict):
        return {str(k): _given(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_given(x) for x in v]
    if isinstance(v, (int, float, str, bytes, bool)) or v is None:
        return repr(v)
    return type(v).__name__


def f32(*shape):
    return np.zeros(shape, dtype=np.float32)


def u32(*shape):
    return np.zeros(shape, dtype=np.uint32)


def dev(k, first=101):
    """k distinct device pointers"""
    return list(range(first, first + k))


def calls(pkg, fake):
    """run the script; `fake` is a Recorder the caller has installed as pkg._lib"""
    assert pkg.lib() is fake
    steps = []
    r = pkg.Renderer(0)
    scene = pkg.Scene()
    assert not r.h and not scene.h
    fake.log.clear()

    def call(method, *args, **kw):
        f = getattr(r, method)
        bound = inspect.signature(f).bind(*args, **kw)
        ins = {}
        _arrays("", dict(bound.arguments), ins)
        step = {"call": method, "given": {k: _given(v) for k, v in bound.arguments.items()}}
        try:
            got = f(*args, **kw)
        except Exception as e:
            step["raised"] = type(e).__name__
            got = None
        else:
            step["returned"] = _layout(got)
        names = {}
        if method not in DERIVED:
            _arrays("", dict(enumerate(got)) if isinstance(got, tuple) else got, names)
        names = {a: "out:" + str(p) for a, p in names.items()}
        names.update({a: "in:" + p for a, p in ins.items()})
        step["abi"] = [[s, _named(a, names)] for s, a in fake.log]
        fake.log.clear()
        steps.append(step)
        return got

    tri = {"vertices": f32(3, 3), "triangles": u32(1, 3)}
    full = {"vertices": f32(4, 3), "triangles": u32(2, 3), "normals": f32(4, 3), "uvs": f32(4, 3), "material_index": 1}
    cam = lambda: f32(12)                      # noqa: E731
    img = lambda: f32(H, W, 3)                 # noqa: E731
    plane = lambda: f32(H, W)                  # noqa: E731
    rays = lambda n=N: f32(n, 8)               # noqa: E731
    pts = lambda n=N: f32(n, 4)                # noqa: E731

    # ---- scene, geometry, state
    call("set_textures", [])
    call("set_textures", [{"type": "checker", "color_a": (1, 0, 0), "color_b": (0, 0, 1), "scalar": 8.0},
                          {"type": "bitmap", "pixels": np.zeros((2, 3, 4), dtype=np.uint8)}])
    call("upload", [tri])
    call("upload", [tri, full], lights=[((1, 2, 3), 40.0)], materials=[{}, {"albedo": (0.5, 0.25, 1), "type": 2, "smooth_shading": True, "ior": 1.5,
                                                                            "texture": 0}],
         textures=[{"type": "albedo", "color_a": (1, 1, 1)}], dynamic=True)
    call("bvh_export_uv")
    call("update_vertices", 0, f32(3, 3))
    call("update_vertices", 1, f32(4, 3), normals=f32(4, 3))
    call("set_mesh_transform", 0, None)
    call("set_mesh_transform", 1, np.eye(3, 4, dtype=np.float32) * 2)
    call("set_mesh_transform", 1, np.eye(4, dtype=np.float32))
    call("set_mesh_transform", 1, np.ones((4, 4), dtype=np.float32))
    call("set_mesh_transform", 1, f32(2, 2))
    call("refit")
    call("rebuild")
    call("mesh_vertices", 0)
    call("mesh_vertices", 1)
    call("mesh_vertices", 2)
    call("upload_scene", scene)
    call("upload_scene", scene, dynamic=True)
    call("upload", [tri, full], dynamic=True)   # the gradients' grad_xyz is sized from the last upload
    call("set_camera", f32(3), f32(9))
    call("set_camera_from", scene)
    call("change_shading_mode", 100)
    call("set_miss_color", f32(3))
    call("set_counting", True)
    call("set_counting", 0)
    call("set_path_params")
    call("set_path_params", spp=2, max_bounces=5, seed=7)
    call("set_option", "spp", 3)
    call("set_accumulation", 16)
    call("reset_accumulation")
    call("accumulated_samples")

    # ---- ray queries
    call("trace_rays", rays())
    call("trace_rays", rays(), want=("prim", "t"))
    call("occluded", rays())
    call("trace_rays_device", N, 101)
    call("trace_rays_device", N, *dev(5), stats=True)
    call("occluded_device", N, 101, 102)
    call("occluded_device", N, 101, 102, stats=True)
    call("shade_rays", rays())
    call("shade_rays", rays(), want=("albedo", "rgb", "inst"))
    call("shade_rays_device", N, 101)
    call("shade_rays_device", N, *dev(8), stats=True)
    call("path_rays", rays())
    call("path_rays", rays(), ids=u32(N), first_sample=2, n_samples=4, sums=np.zeros((N, 3)), want=("rgb", "uv"))
    call("path_rays", rays(), ids=u32(N + 1))
    call("path_rays", rays(), sums=f32(N, 3))
    call("path_rays_device", N, 101)
    call("path_rays_device", N, 101, 102, 2, 4, *dev(6, 103), stats=True)
    call("count_hits", rays())
    call("count_hits_device", N, 101, 102)
    call("count_hits_device", N, 101, 102, stats=True)
    call("list_hits", rays())
    call("list_hits", rays(), want=("inst", "t"), capacity=5)
    call("list_hits", rays(), want=())
    call("list_hits_device", N, 101, 102, 5)
    call("list_hits_device", N, 101, 102, 5, *dev(4, 103), total=True)
    call("list_hits_device", N, 101, 102, 5, *dev(4, 103), stats=True)
    call("list_hits_device", N, 101, 102, 5, *dev(4, 103), total=True, stats=True)
    call("list_phases")
    call("inside_length", rays())

    # ---- frames: camera rays, guides, denoiser, temporal reprojection, variance, motion
    call("camera_rays", W, H)
    call("camera_rays", W, H, sample=5)
    call("camera_rays_device", W, H, 101)
    call("camera_rays_device", W, H, 101, sample=5, stats=True)
    call("frame_guides", W, H)
    call("frame_guides", W, H, want=("t", "normal"))
    call("frame_guides_device", W, H)
    call("frame_guides_device", W, H, *dev(3), stats=True)
    call("denoise", img(), img(), img(), plane())
    call("denoise", img(), img(), img(), plane(), iterations=2, sigma_color=1.5, sigma_normal=0.5, sigma_depth=0.25, demodulate=0)
    call("denoise", img(), img(), img(), f32(H * W))
    call("denoise", img(), f32(H, W, 2), img(), plane())
    call("denoise_device", W, H, *dev(5))
    call("denoise_device", W, H, *dev(5), stats=True, iterations=2, demodulate=0)
    call("temporal_accumulate", cam(), cam(), img(), img(), img(), plane())
    call("temporal_accumulate", cam(), cam(), img(), img(), None, plane(), hist_prev=f32(H, W, 8), want_out=False, prev_point=img(), alpha=0.5,
         depth_tolerance=0.125, normal_threshold=0.75, max_history=8, demodulate=0)
    call("temporal_accumulate", cam(), cam(), img(), img(), img(), plane(), hist_prev=f32(H, W, 8))
    call("temporal_accumulate", cam(), cam(), img(), img(), img(), f32(H * W))
    call("temporal_accumulate", cam(), cam(), img(), f32(W, H, 3), img(), plane())
    call("temporal_accumulate", cam(), cam(), img(), img(), img(), plane(), hist_prev=f32(H, W, 3))
    call("temporal_accumulate", cam(), cam(), img(), img(), img(), plane(), prev_point=f32(H, W, 2))
    call("temporal_accumulate_device", W, H, cam(), cam(), *dev(4), None, 106)
    call("temporal_accumulate_device", W, H, cam(), cam(), *dev(7), stats=True, d_prev_point=108, alpha=0.5, max_history=8)
    call("temporal_variance", cam(), cam(), img(), img(), img(), plane())
    call("temporal_variance", cam(), cam(), img(), img(), None, plane(), hist_prev=f32(H, W, 8), mom_prev=f32(H, W, 2), want_out=False,
         prev_point=img(), alpha_moments=0.25, min_history=2, alpha=0.5, demodulate=0)
    call("temporal_variance", cam(), cam(), img(), img(), img(), f32(H * W))
    call("temporal_variance", cam(), cam(), img(), img(), img(), plane(), prev_point=f32(H, W, 2))
    call("temporal_variance", cam(), cam(), img(), img(), img(), plane(), hist_prev=f32(H, W, 3))
    call("temporal_variance", cam(), cam(), img(), img(), img(), plane(), mom_prev=f32(H, W, 3))
    call("temporal_variance_device", W, H, cam(), cam(), *dev(4), None, 106, None, 108, 109)
    call("temporal_variance_device", W, H, cam(), cam(), *dev(10), stats=True, d_prev_point=111, alpha_moments=0.25, min_history=2, alpha=0.5)
    call("denoise_variance", img(), img(), img(), plane(), plane())
    call("denoise_variance", img(), img(), img(), plane(), plane(), want_variance=True, iterations=2, sigma_luminance=0.5, sigma_normal=0.5,
         sigma_depth=0.25, demodulate=0)
    call("denoise_variance", img(), img(), img(), f32(H * W), plane())
    call("denoise_variance", img(), img(), f32(H, W), plane(), plane())
    call("denoise_variance", img(), img(), img(), plane(), f32(W, H))
    call("denoise_variance_device", W, H, *dev(6))
    call("denoise_variance_device", W, H, *dev(7), stats=True, iterations=2)
    call("motion_snapshot")
    call("previous_points", u32(N), u32(N), f32(N, 2))
    call("previous_points", u32(N), u32(N + 1), f32(N, 2))
    call("previous_points_device", N, *dev(4))
    call("previous_points_device", N, *dev(4), stats=True)
    call("frame_motion", W, H)
    call("frame_motion_device", W, H, 101)
    call("frame_motion_device", W, H, 101, stats=True)

    # ---- point queries, winding numbers, gradients
    call("closest_points", pts())
    call("closest_points", pts(), want=("point", "dist"))
    call("closest_points", f32(4, 3))   # records only: twelve floats are three records, not four coordinates
    call("closest_points_device", N, 101)
    call("closest_points_device", N, *dev(6), stats=True)
    call("occupancy", pts())
    call("occupancy", f32(N, 3))
    call("occupancy_device", N, 101, 102)
    call("occupancy_device", N, 101, 102, stats=True)
    call("signed_distance", pts())
    call("signed_distance", f32(N, 3), sign="winding", beta=3, threshold=0.25)
    call("signed_distance", "not points", sign="nearest")
    call("winding_numbers", pts())
    call("winding_numbers", f32(N, 3), beta=3)
    call("winding_numbers_device", N, 101, 102)
    call("winding_numbers_device", N, 101, 102, beta=3, stats=True)
    call("winding_moments")
    call("inside_winding", pts())
    call("inside_winding", f32(N, 3), beta=3, threshold=0.25)
    call("trace_rays_backward", rays(), u32(N), u32(N), f32(N), f32(N, 2))
    call("trace_rays_backward", rays(), u32(N), u32(N), f32(N), f32(N, 2), grad_t=f32(N), grad_uv=f32(N, 2), want=("grad_xyz",))
    call("trace_rays_backward", rays(), u32(N), u32(N), f32(N + 1), f32(N, 2))
    call("trace_rays_backward", rays(), u32(N), u32(N), f32(N), f32(N, 2), grad_uv=f32(N + 1, 2))
    call("trace_rays_backward_device", N, *dev(5))
    call("trace_rays_backward_device", N, *dev(9), stats=True)
    call("closest_points_backward", pts(), u32(N), u32(N), f32(N, 2), f32(N))
    call("closest_points_backward", pts(), u32(N), u32(N), f32(N, 2), f32(N), want=("grad_points",))
    call("closest_points_backward", pts(), u32(N), u32(N), f32(N, 2), f32(N + 1))
    call("closest_points_backward_device", N, *dev(5))
    call("closest_points_backward_device", N, *dev(7), stats=True)

    # ---- debug reads, streams, tree export
    call("read_counters")
    call("read_timeline", max_words=6)
    call("set_stream", 101)
    call("set_stream", None)
    call("reset_stream")
    call("synchronize")
    call("bvh_info")
    call("bvh_export")
    call("build_stats")
    call("bvh_export4")
    call("bvh_export4q")
    call("bvh_export_planes4q")

    # ---- frames and their assembly across ranks
    call("comm_init", 0, 2)
    call("comm_init", 1, 2, unique_id=bytes(range(128)))
    call("comm_init_host", 1, 2, "/crt_pin")
    call("comm_destroy")
    call("render_frame_distributed", W, H)
    call("render_frame_distributed", W, H, d_rgba8=101, host=True, stats=True)
    call("render_frame_distributed", W, H, host=True)
    call("pinned_frame", W, H)
    call("pinned_frame", W, H)
    call("pinned_frame", W, 2 * H)
    call("render_frame", W, H)
    call("render_frame", W, H, want=("rgb", "hit_prim"), pinned=True)
    call("render_frame_device", W, H, 101)
    call("render_frame_device", W, H, *dev(5), stats=True)
    call("render_tiles_device", W, H, 1, 2, 101)
    call("render_tiles_device", W, H, 1, 2, 101, stats=True)
    call("render_frames_batch_device", W, H, [101, 102])
    call("render_frames_batch_device", W, H, [101, 102], cameras=[(f32(3), f32(9)), (f32(3), f32(9))], stats=True)
    call("render_tiles_batch_device", W, H, 1, 2, [101, 102])
    call("render_tiles_batch_device", W, H, 1, 2, [101, 102], cameras=[(f32(3), f32(9)), (f32(3), f32(9))], stats=True)
    call("untile_batch_device", W, H, 2, 3, 1, 101, 102)
    call("untile_device", W, H, 2, 101, 102)
    call("close")
    scene.close()
    return steps


def scripted_methods(steps):
    return {s["call"] for s in steps}


def public_methods(pkg):
    return {n for n, v in vars(pkg.Renderer).items() if not n.startswith("_") and inspect.isfunction(v)}


def snapshot(pkg, install):
    """install(fake) makes `fake` the package's _lib (the test hands monkeypatch.setattr in)"""
    out = {"surface": surface(pkg), "abi": abi(pkg)}
    fake = Recorder()
    install(fake)
    out["calls"] = calls(pkg, fake)
    return out


def dumps(snap):
    return json.dumps(snap, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    real = pkg.lib()
    try:
        text = dumps(snapshot(pkg, lambda fake: setattr(pkg, "_lib", fake)))
    finally:
        pkg._lib = real
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w") as f:
            f.write(text)
        print("wrote %s (%d bytes)" % (FIXTURE, len(text)))
    else:
        print("the fixture is %s" % ("up to date" if open(FIXTURE).read() == text else "STALE: run with --write"))
