"""The texture functions at the edges of their domain, and every way a uv record reaches leaf order.

Float to int in the texture functions follows one rule (include/crt_hip.h, "texture conversions"): truncate towards zero, saturate
to [INT_MIN, INT_MAX], NaN -> 0; the checker's colour is the parity of the wrapped sum of its two cell numbers.  `rule_colour`
below restates that rule in Python integers and numpy float32, sharing no code with the kernels, the oracle or the host scene
layer, and HAND holds colours worked out on paper from it.

CPU: the oracle's texture_color and the host layer's Scene.texture_color at the nominal (u, v) of every row.
GPU: a probe frame.  There is no device entry point that evaluates a texture at a given (u, v), so every row becomes a small quad
facing the camera under one pixel centre, all of its vertices carrying the row's uv, lit by one light at the eye in mode 100.  The
pixel divided by the same pixel of a frame with plain white materials is the texture's colour.  The pixel centre meets its quad
at barycentrics of about (1/3, 1/3), so the interpolated coordinate is the row's uv only to within a rounding or two: the
expectation is computed on uv0 * w + uv1 * u + uv2 * v formed in float32 in the documented order from the barycentrics of a mode-3
frame of the same scene (its float colour is (1 - u - v, u, v)).  HAND rows are chosen away from every cell boundary, so for them
the nominal and the interpolated coordinate give the same colour.

Measured on the MI355X before the rule was stated (plain casts on the CPU sides): see DESIGN.md section 7."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import path_reference as R
import shaded_query_checks as sq
import test_path_reference as T

f32 = np.float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
A, B = (0.75, 0.5, 0.25), (0.125, 0.375, 0.625)  # exact in float32, no zero channel
INF, NAN = float("inf"), float("nan")


def _near(x):
    x = f32(x)
    return [float(np.nextafter(x, f32(-INF))), float(x), float(np.nextafter(x, f32(INF)))]


UV = [-INF, -3e38, -1e12, -1.5, -1.0, -2.0 ** -149, -0.0, 0.0, 2.0 ** -149, 3e-10, 0.05, 0.2, 0.3, 0.5, 1.0 - 2.0 ** -24, 1.0,
      1.0 + 2.0 ** -23, 1.5, 1e12, 3e38, INF, NAN]
for _w in (1, 3, 8):
    UV += _near(-2.0 ** 31 / _w) + _near((2.0 ** 31 - 128) / _w)
UV = [float(f32(x)) for x in UV]
V05, V03 = float(f32(0.05)), float(f32(0.3))  # the fixed coordinate of a row
SQUARES = [0.0, 2.0 ** -149, 1e-10, 0.125, 1.0 / 3.0, 0.3, 1.0, 1.0 + 2.0 ** -23, 2.0, 1e30, INF, -0.3, NAN]
EDGE_WIDTHS = [-1.0, 0.0, 1.0 / 3.0, 0.5, 1.0, NAN]
BITMAPS = [(1, 1, 3), (1, 2, 3), (2, 1, 3), (1, 255, 3), (255, 1, 3), (2, 2, 4), (255, 1, 4), (1, 255, 4)]  # (w, h, channels)


def _pixels(w, h, c):
    """every texel differs from every other in each colour channel (w * h <= 255); alpha holds other values still"""
    k = np.arange(w * h).reshape(h, w)
    ch = [(k * 1 + 1) % 256, (k * 1 + 1) % 256 ^ 0x55, 255 - k, (k * 7 + 3) % 256]
    return np.stack(ch[:c], axis=-1).astype(np.uint8)


# ---- the rule, restated

def sat_int(x):
    """float32 -> int: NaN -> 0, saturate, truncate"""
    x = float(x)
    if x != x:
        return 0
    if x >= 2.0 ** 31:
        return INT_MAX
    if x <= -2.0 ** 31:
        return INT_MIN
    return int(x)


def rule_colour(tex, u, v):
    """colour of texture dict `tex` at float32 (u, v) (edges: at barycentrics (u, v)), as a tuple of float32"""
    u, v = f32(u), f32(v)
    a, b = tuple(f32(tex.get("color_a", (0, 0, 0)))), tuple(f32(tex.get("color_b", (0, 0, 0))))
    s = f32(tex.get("scalar", 0.0))
    with np.errstate(all="ignore"):
        if tex["type"] == "albedo":
            return a
        if tex["type"] == "edges":
            return a if (u < s or v < s or (f32(1.0) - u - v) < s) else b
        if tex["type"] == "checker":
            width = f32(sat_int(f32(1.0) / s))
            u2, v2 = sat_int(np.floor(u * width)), sat_int(np.floor(v * width))
            return a if (u2 + v2) % 2 == 0 else b  # Python integers: no overflow, the parity of the wrapped sum is the same
        px = tex["pixels"]
        u = f32(0.0) if u != u else min(max(u, f32(0.0)), f32(1.0))
        v = f32(0.0) if v != v else min(max(v, f32(0.0)), f32(1.0))
        row = sat_int((f32(1.0) - v) * f32(px.shape[0] - 1))
        col = sat_int(u * f32(px.shape[1] - 1))
        return tuple(f32(px[row, col, :3]) / f32(255.0))


def _round32(q):
    """a Fraction to the nearest float32, ties to even (for finite results inside the float32 range)"""
    c = f32(float(q))
    best = None
    for x in (np.nextafter(c, f32(-INF)), c, np.nextafter(c, f32(INF))):
        if not np.isfinite(x):
            continue
        d = abs(Fraction(float(x)) - q)
        even = (int(np.float32(x).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, x)
    return f32(best[1])


def fma32(a, b, c):
    """fmaf: a * b + c with one rounding"""
    a, b, c = f32(a), f32(b), f32(c)
    with np.errstate(all="ignore"):
        plain = f32(f32(a * b) + c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)) or not np.isfinite(plain):
        return plain  # infinities and NaN come out the same with one rounding or two
    q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if q == 0:
        return plain  # keeps the sign of zero
    return _round32(q)


def interpolate(c, bw, bu, bv):
    """uv0 * w + uv1 * u + uv2 * v in the documented order, all three uvs equal to c"""
    with np.errstate(all="ignore"):
        return fma32(c, bv, fma32(c, bu, f32(c) * f32(bw)))


# ---- rows: (texture index, u, v) over one table; bitmaps sit second and later in it, so their texel offsets are not 0

def table_and_rows():
    tex = [{"type": "checker", "color_a": A, "color_b": B, "scalar": s} for s in SQUARES]
    rows = []
    for i in range(len(SQUARES)):
        for x in UV:
            rows += [(i, x, V05), (i, V05, x)]
    for w, h, c in BITMAPS:
        tex.append({"type": "bitmap", "pixels": _pixels(w, h, c)})
        for x in UV:
            rows += [(len(tex) - 1, x, V03), (len(tex) - 1, V03, x)]
    for ew in EDGE_WIDTHS:
        tex.append({"type": "edges", "color_a": A, "color_b": B, "scalar": ew})
        rows += [(len(tex) - 1, 0.5, 0.5), (len(tex) - 1, NAN, INF)]
    tex.append({"type": "albedo", "color_a": A})
    rows += [(len(tex) - 1, NAN, -INF), (len(tex) - 1, 0.5, 0.5)]
    return tex, rows


# colours worked out on paper from the rule; v = 0.05 puts the second cell number at an even value for every width used here
# (0.05 * 8 = 0.4 -> 0; 0.05 * 3 -> 0; 0.05f * 2^31 = 13421773 * 8; 0.05 * -3 = -0.15 -> -1, the one odd case)
HAND_CHECKER = [
    # square_size, u, colour
    (0.125, 0.5, "A"),      # 4
    (0.125, 0.3, "A"),      # 2.4 -> 2
    (0.125, 0.2, "B"),      # 1.6 -> 1
    (0.125, 1e12, "B"),     # 8e12 saturates to INT_MAX, odd
    (0.125, INF, "B"),
    (0.125, 3e38, "B"),     # the product overflows to +inf
    (0.125, -1e12, "A"),    # INT_MIN, even
    (0.125, -INF, "A"),
    (0.125, -3e38, "A"),
    (0.125, NAN, "A"),      # NaN -> 0
    (0.125, 0.0, "A"),
    (0.125, -0.0, "A"),     # floor(-0) = -0 -> 0
    (0.125, 2.0 ** -149, "A"),
    (0.125, 3e-10, "A"),
    (0.0, 3e-10, "A"),      # width = INT_MAX -> 2^31 as a float; 3e-10 * 2^31 = 0.64 -> 0
    (0.0, 0.5, "A"),        # 2^30, even
    (0.0, 1e12, "B"),
    (0.0, -1e12, "A"),
    (0.0, NAN, "A"),
    (2.0 ** -149, 3e-10, "A"),  # 1 / s overflows to +inf like 1 / 0
    (1e-10, 3e-10, "A"),    # 1e10 saturates
    (0.3, 0.5, "B"),        # width 3: 1.5 -> 1
    (0.3, 0.2, "A"),        # 0.6 -> 0
    (1.0 / 3.0, 0.5, "B"),  # 1 / fl(1/3) rounds to 3.0 in float32
    (1.0, 0.5, "A"),
    (1.0, 1.5, "B"),
    (1.0, -1.5, "A"),       # -2
    (1.0 + 2.0 ** -23, 1.5, "A"),  # width 0: every coordinate in cell 0
    (2.0, 1.5, "A"),
    (1e30, 1e12, "A"),
    (INF, -1.5, "A"),
    (NAN, 1.5, "A"),        # NaN -> width 0
    (-0.3, 0.5, "B"),       # width -3: -1.5 -> -2 even, v: -0.15 -> -1 odd
    (-0.3, 0.2, "A"),       # -0.6 -> -1 odd, v odd: even sum
    (-0.3, 1e12, "B"),      # INT_MIN even, v odd
]
# bitmap (w, h): u (v = 0.3) -> texel column; v (u = 0.3) -> texel row
HAND_BITMAP = [
    ((2, 1), "u", 0.3, 0), ((2, 1), "u", 1.5, 1), ((2, 1), "u", INF, 1), ((2, 1), "u", -INF, 0), ((2, 1), "u", NAN, 0),
    ((2, 1), "u", -1.5, 0), ((2, 1), "u", 1e12, 1), ((255, 1), "u", 0.3, 76), ((255, 1), "u", 0.2, 50), ((255, 1), "u", 3e38, 254),
    ((255, 1), "u", NAN, 0), ((1, 2), "v", 0.3, 0), ((1, 2), "v", 1.5, 0), ((1, 2), "v", -1.5, 1), ((1, 2), "v", NAN, 1),
    ((1, 2), "v", INF, 0), ((1, 2), "v", -INF, 1), ((1, 255), "v", 0.3, 177), ((1, 255), "v", 0.2, 203), ((1, 255), "v", -1e12, 254),
    ((1, 1), "u", NAN, 0), ((1, 1), "v", INF, 0),
]
HAND_EDGES = {-1.0: "B", 0.0: "B", 0.5: "A", 1.0: "A", "nan": "B"}  # at barycentrics near (1/3, 1/3); NaN compares false


def _hand_expectations(tex, rows):
    """row number -> colour, for the rows that HAND covers"""
    name = {"A": tuple(f32(A)), "B": tuple(f32(B))}
    out = {}
    for n, (i, u, v) in enumerate(rows):
        t = tex[i]
        if t["type"] == "checker" and v == V05:
            for s, hu, col in HAND_CHECKER:
                same_s = (s != s and t["scalar"] != t["scalar"]) or float(f32(s)) == float(f32(t["scalar"]))
                if same_s and ((hu != hu and u != u) or (float(f32(hu)) == u and math.copysign(1, hu) == math.copysign(1, u))):
                    out[n] = name[col]
        elif t["type"] == "bitmap" and t["pixels"].shape[2] == 3:
            h, w = t["pixels"].shape[:2]
            for (bw, bh), axis, x, at in HAND_BITMAP:
                val, other = (u, v) if axis == "u" else (v, u)
                if (bw, bh) == (w, h) and other == V03 and ((x != x and val != val) or float(f32(x)) == val):
                    px = t["pixels"][0, at] if axis == "u" else t["pixels"][at, 0]
                    out[n] = tuple(f32(px[:3]) / f32(255.0))
        elif t["type"] == "edges" and u == 0.5:
            key = "nan" if t["scalar"] != t["scalar"] else t["scalar"]
            if key in HAND_EDGES:
                out[n] = name[HAND_EDGES[key]]
        elif t["type"] == "albedo":
            out[n] = name["A"]
    return out


def _ppm(path, px):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (px.shape[1], px.shape[0]))
        f.write(np.ascontiguousarray(px[:, :, :3]).tobytes())


def _host_scene(pkg, tex, tmp_path):
    """the table in the host scene layer; 4-channel images cannot be handed to it as PPM files and get None"""
    s = pkg.Scene()
    index = []
    for i, t in enumerate(tex):
        if t["type"] == "bitmap":
            if t["pixels"].shape[2] != 3:
                index.append(None)
                continue
            p = os.path.join(str(tmp_path), "t%d.ppm" % i)
            _ppm(p, t["pixels"])
            s.add_texture("t%d" % i, "bitmap", file_path=p)
        else:
            s.add_texture("t%d" % i, t["type"], t.get("color_a", (0, 0, 0)), t.get("color_b", (0, 0, 0)), t.get("scalar", 0.0))
        index.append(s.texture_count - 1)
    return s, index


def test_hand_table_agrees_with_the_restated_rule():
    """the paper answers and rule_colour are two statements of one rule; fma32 rounds once"""
    tex, rows = table_and_rows()
    hand = _hand_expectations(tex, rows)
    assert len(hand) >= len(HAND_CHECKER) + len(HAND_BITMAP) + len(HAND_EDGES) + 2
    for n, exp in hand.items():
        i, u, v = rows[n]
        if tex[i]["type"] == "edges":
            u = v = 1.0 / 3.0
        assert rule_colour(tex[i], u, v) == exp, "row %d: %r at (%r, %r)" % (n, tex[i].get("scalar"), u, v)
    x = f32(1.0 + 2.0 ** -12)  # x * x = 1 + 2^-11 + 2^-24 loses its last bit when rounded on its own
    assert float(fma32(x, x, f32(-1.0))) == 2.0 ** -11 + 2.0 ** -24 and float(f32(x * x) - f32(1.0)) == 2.0 ** -11
    assert float(fma32(f32(3.0), f32(1.0 / 3.0), f32(-1.0))) == float(Fraction(float(f32(1.0 / 3.0))) * 3 - 1)
    assert sat_int(f32(2.0 ** 31 - 128)) == 2 ** 31 - 128 and sat_int(f32(2.0 ** 31)) == INT_MAX and sat_int(-INF) == INT_MIN


def test_oracle_and_host_layer_follow_the_conversion_rule(pkg, oracle, tmp_path):
    """every row at its nominal (u, v): oracle texture_color == host Scene.texture_color == the restated rule, bit for bit,
    and == the paper answers where there is one"""
    tex, rows = table_and_rows()
    hand = _hand_expectations(tex, rows)
    host, index = _host_scene(pkg, tex, tmp_path)
    bad = []
    for n, (i, u, v) in enumerate(rows):
        if tex[i]["type"] == "edges":  # a function of barycentrics: feed it some
            u, v = (1.0 / 3.0, 1.0 / 3.0) if u == 0.5 else (u, v)
        exp = rule_colour(tex[i], u, v)
        if n in hand:
            assert exp == hand[n]
        got_o = tuple(oracle.texture_color(tex[i], u, v))
        got_h = tuple(host.texture_color(index[i], u, v)) if index[i] is not None else exp
        if got_o != exp or got_h != exp:
            bad.append((tex[i]["type"], tex[i].get("scalar"), u, v, exp, got_o, got_h))
    assert not bad, "%d of %d rows off the rule (kind, scalar, u, v, rule, oracle, host), first: %r" % (len(bad), len(rows), bad[:5])


# ---- GPU: the probe frame

def probe_scene(tex, rows, textured=True):
    """K x K quads at z = -4 facing the camera at the origin, one per pixel of a K x K frame; the pixel centre meets quad n at the
    centroid of its first triangle; every vertex of quad n carries row n's uv; material i has texture i"""
    n = len(rows)
    K = int(math.ceil(math.sqrt(n)))
    sp = 8.0 / K
    e = 0.6 * sp
    meshes = []
    for k in range(K * K):
        i, u, v = rows[k] if k < n else (len(tex) - 1, 0.0, 0.0)
        px, py = k % K, k // K
        cx, cy = 4.0 * (2.0 * (px + 0.5) / K - 1.0), 4.0 * (1.0 - 2.0 * (py + 0.5) / K)
        x0, y0 = cx - 2.0 * e / 3.0, cy - e / 3.0
        m = R.quad((x0, y0, -4.0), (x0 + e, y0, -4.0), (x0 + e, y0 + e, -4.0), (x0, y0 + e, -4.0), i)
        m["uvs"] = np.tile(f32([u, v, 0.0]), (4, 1))
        meshes.append(m)
    mats = [{"albedo": (1.0, 1.0, 1.0), "type": 1, "texture": i if textured else -1} for i in range(len(tex))]
    return K, meshes, [((0.0, 0.0, 0.0), 100.0)], mats


def _identify(ratio, candidates):
    d = np.abs(np.asarray(candidates, np.float64) - np.asarray(ratio, np.float64)[None]).max(axis=1)
    k = int(np.argmin(d))
    assert d[k] < 1e-5, "colour %r is none of the texture's" % (ratio,)
    return tuple(f32(candidates[k]))


@pytest.fixture(scope="module")
def renderer(pkg):
    r = pkg.Renderer(0)
    yield r
    r.close()


@pytest.mark.gpu
def test_device_textures_follow_the_conversion_rule(pkg, oracle, renderer, scenes, tmp_path):
    """probe frame: device == oracle bit for bit; the colour each pixel identifies == the restated rule == the host layer on the
    interpolated coordinate, and == the paper answers"""
    tex, rows = table_and_rows()
    hand = _hand_expectations(tex, rows)
    K, meshes, lights, mats = probe_scene(tex, rows)
    _, _, _, white = probe_scene(tex, rows, textured=False)
    host, index = _host_scene(pkg, tex, tmp_path)
    pos, rot = f32([0, 0, 0]), scenes.IDENTITY
    r = renderer
    r.set_accumulation(0)
    r.set_option("phong_ks", 0)
    frames = {}
    for key, mm, tt, mode in (("tex", mats, tex, 100), ("white", white, None, 100), ("bary", white, None, 3)):
        r.upload(meshes, lights, mm, tt)
        r.set_camera(pos, rot)
        r.change_shading_mode(mode)
        frames[key] = r.render_frame(K, K)
    O = oracle.OracleScene(meshes, lights, mats, textures=tex)
    ref = O.render(pos, rot, 100, K, K)
    n = len(rows)
    inst = frames["tex"]["hit_inst"].reshape(-1)
    np.testing.assert_array_equal(inst, np.arange(K * K), err_msg="a pixel centre does not meet its own quad")
    np.testing.assert_array_equal(frames["tex"]["hit_prim"].reshape(-1), 0)
    dev = frames["tex"]["rgb"].reshape(-1, 3)
    differ = np.nonzero(np.any(dev.view(np.uint32) != ref["rgb"].reshape(-1, 3).view(np.uint32), axis=1))[0]
    differ = [int(k) for k in differ if k < n]
    msg = ["row %d %s scalar %r uv (%r, %r): device %s, oracle %s" % (k, tex[rows[k][0]]["type"], tex[rows[k][0]].get("scalar"),
                                                                     rows[k][1], rows[k][2], dev[k], ref["rgb"].reshape(-1, 3)[k])
           for k in differ[:8]]
    print("probe frame %dx%d, %d rows, %d differ from the oracle" % (K, K, n, len(differ)))
    assert not differ, "device and oracle differ on %d rows:\n%s" % (len(differ), "\n".join(msg))
    with np.errstate(all="ignore"):
        ratio = dev.astype(np.float64) / frames["white"]["rgb"].reshape(-1, 3).astype(np.float64)
    bary = frames["bary"]["rgb"].reshape(-1, 3)
    bad = []
    for k, (i, u, v) in enumerate(rows):
        t = tex[i]
        bw, bu, bv = bary[k]
        assert abs(bu - 1 / 3) < 1e-3 and abs(bv - 1 / 3) < 1e-3
        if t["type"] == "edges":
            tu, tv = bu, bv
        else:
            tu, tv = interpolate(u, bw, bu, bv), interpolate(v, bw, bu, bv)
        exp = rule_colour(t, tu, tv)
        if t["type"] == "bitmap":
            cands = (t["pixels"][:, :, :3].reshape(-1, 3).astype(np.float32) / f32(255.0)).tolist()
        else:
            cands = [f32(t.get("color_a", (0, 0, 0))).tolist(), f32(t.get("color_b", (0, 0, 0))).tolist()]
        got = _identify(ratio[k], cands)
        got_h = tuple(host.texture_color(index[i], float(tu), float(tv))) if index[i] is not None else exp
        if got != exp or got_h != exp or (k in hand and hand[k] != exp):
            bad.append((k, t["type"], t.get("scalar"), u, v, float(tu), float(tv), got, exp, got_h, hand.get(k)))
    assert not bad, ("%d rows (row, kind, scalar, u, v, interpolated u, v, device, rule, host, paper), first: %r" % (len(bad), bad[:5]))


# ---- GPU: every way a uv record reaches leaf order, against the float64 reference

LBVH, PLOC = 0, 1
ROUTES = ["host_sah", "gpu_build_lbvh", "gpu_build_ploc", "rebuild_lbvh", "rebuild_ploc", "transform_refit"]


def _moved(name):
    """(mesh, 3x4 transform) of a textured mesh that stays inside its scene"""
    if name == "textured_room":
        return 13, f32([[1, 0, 0, 0.3], [0, 1, 0, 0.2], [0, 0, 1, 0.4]])  # the box with planar uvs
    c, s = math.cos(0.2), math.sin(0.2)
    return 1, f32([[c, 0, s, 0.0], [0, 1, 0, 0.0], [-s, 0, c, -0.3]])   # the bitmap wall, turned about y


ROUTE_PATH_PARAMS = (1, 2, 1234)


def _oracle_frames(oracle, sc, cam):
    """the oracle's frames of the scene in modes 3, 100 and 200 (ROUTE_PATH_PARAMS) with the float64 reference's miss colour:
    the bit-exact yardstick test_path_reference pins to the float64 reference on these scenes"""
    O = oracle.OracleScene(sc["meshes"], sc["lights"], sc["materials"], textures=sc.get("textures", ()))
    oracle.set_path_params(*ROUTE_PATH_PARAMS)
    try:
        return {m: O.render(cam["position"], cam["matrix"], m, T.W, T.H, miss_rgb=R.MISS_RGB) for m in (3, 100, 200)}
    finally:
        oracle.set_path_params(4, 3, 1234)
        O.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", T.TEXTURED)
def test_gpu_uv_records_reach_leaf_order(pkg, oracle, scenes, name, route):
    """mode 100 at pixel centres and one mode-200 frame per pipeline, against the float64 reference, after each kind of upload or
    tree change.  The reference knows per-vertex uvs only, so a uv record attached to the wrong triangle, or in the wrong
    vertex order, moves the texture.  Then the same frame through camera_rays, shade_rays, path_rays and frame_guides, which
    read the uv records through their own parameter block, against the oracle's frames bit for bit; the guide albedo of a
    textured hit is the oracle's texture_color at the hit's interpolated uv."""
    sc = R.SCENES[name](scenes)
    meshes = [dict(m) for m in sc["meshes"]]
    cam = sc["camera"]
    r = pkg.Renderer(0)
    try:
        r.set_accumulation(0)
        r.set_option("gpu_build", 0 if route in ("host_sah", "transform_refit") else 1)
        r.set_option("gpu_builder", PLOC if route.endswith("ploc") else LBVH)
        dynamic = route.startswith("rebuild") or route == "transform_refit"
        r.upload(meshes, sc["lights"], sc["materials"], sc.get("textures"), dynamic=dynamic)
        if dynamic:
            mesh, M = _moved(name)
            r.set_mesh_transform(mesh, M)
            if route == "transform_refit":
                r.refit()
            else:
                r.rebuild()
            meshes[mesh]["vertices"] = np.asarray(r.mesh_vertices(mesh)[0], np.float32).reshape(-1, 3).copy()
            v = sc["meshes"][mesh]["vertices"].astype(np.float64)
            np.testing.assert_allclose(meshes[mesh]["vertices"], v @ M[:, :3].astype(np.float64).T + M[:, 3], rtol=0, atol=1e-5)
            nrm = r.mesh_vertices(mesh)[1]
            if nrm is not None:
                meshes[mesh]["normals"] = np.asarray(nrm, np.float32).reshape(-1, 3).copy()
        S = R.Scene(dict(sc, meshes=meshes))
        r.set_camera(cam["position"], cam["matrix"])
        r.set_miss_color(R.MISS_RGB)
        r.change_shading_mode(100)
        r.set_option("phong_ks", 250)
        r.set_option("phong_exponent", 16)
        T.compare_centres(r.render_frame(T.W, T.H), S, cam, 100, R.MISS_RGB, 0.25, 16)
        r.set_option("phong_ks", 0)
        r.change_shading_mode(200)
        ref = R.trace_paths(S, cam["position"], cam["matrix"], T.W, T.H, R.MISS_RGB, 2, 1234)
        for pipeline in (0, 1):
            r.set_option("path_pipeline", pipeline)
            r.set_path_params(1, 2, 1234)
            T.compare_path_frame(r.render_frame(T.W, T.H), ref, "%s %s pipeline=%d" % (name, route, pipeline))
        r.set_option("path_pipeline", 0)
        now = dict(sc, meshes=meshes)
        got = sq.frame_records_equal_frames(r, _oracle_frames(oracle, now, cam), T.W, T.H, ROUTE_PATH_PARAMS, "%s %s" % (name, route),
                                            scene=now, texture_color=oracle.texture_color,
                                            world={"oracle": oracle, "camera": (cam["position"], cam["matrix"]), "lights": sc["lights"], "miss": R.MISS_RGB})
        hit = got["guides"]["t"] != f32(sq.TMAX)
        assert len(np.unique(got["guides"]["albedo"][hit], axis=0)) >= 4, "the textures show in the albedo guide"
    finally:
        r.close()


def _upload_over_route(pkg, sc, name, route, moved=None):
    """a context holding the scene with its textured mesh moved (_moved), reached over `route`: the three dynamic routes upload the
    rest pose and move the mesh; the three static ones upload `moved`, the meshes as a dynamic route traced them"""
    r = pkg.Renderer(0)
    try:
        r.set_accumulation(0)
        r.set_option("gpu_build", 0 if route in ("host_sah", "transform_refit") else 1)
        r.set_option("gpu_builder", PLOC if route.endswith("ploc") else LBVH)
        dynamic = route.startswith("rebuild") or route == "transform_refit"
        r.upload(sc["meshes"] if dynamic else moved, sc["lights"], sc["materials"], sc.get("textures"), dynamic=dynamic)
        if dynamic:
            mesh, M = _moved(name)
            r.set_mesh_transform(mesh, M)
            if route == "transform_refit":
                r.refit()
            else:
                r.rebuild()
        r.set_camera(sc["camera"]["position"], sc["camera"]["matrix"])
        r.set_miss_color(R.MISS_RGB)
        r.change_shading_mode(100)
        return r
    except Exception:
        r.close()
        raise


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.TEXTURED)
def test_gpu_guide_albedo_is_the_same_over_every_route(pkg, scenes, name):
    """One geometry (the scene with its textured mesh moved), one camera, the six routes: the albedo guide, and with it normal
    and t, have the same bits over every route.  The frames read the uv records through fillParams and are compared route by
    route above; the guides read them through the shaded queries' parameter block, so a stale uv pointer or an ungathered uv
    record after crt_rebuild shows here."""
    sc = R.SCENES[name](scenes)
    mesh, _ = _moved(name)
    guides, moved = {}, None
    for route in ["transform_refit"] + [x for x in ROUTES if x != "transform_refit"]:
        r = _upload_over_route(pkg, sc, name, route, moved)
        try:
            if route.startswith("rebuild") or route == "transform_refit":  # (crt_mesh_vertices reads dynamic scenes only)
                xyz, nrm = r.mesh_vertices(mesh)
                if moved is None:
                    moved = [dict(m) for m in sc["meshes"]]
                    moved[mesh]["vertices"] = np.asarray(xyz, np.float32).reshape(-1, 3).copy()
                    if nrm is not None:
                        moved[mesh]["normals"] = np.asarray(nrm, np.float32).reshape(-1, 3).copy()
                assert np.array_equal(sq._bits(xyz).reshape(-1), sq._bits(moved[mesh]["vertices"]).reshape(-1)), "%s %s: the traced vertices" % (name, route)
            guides[route] = r.frame_guides(T.W, T.H)
            ref = r.shade_rays(r.camera_rays(T.W, T.H), want=("normal", "albedo", "t"))
            for k in ("normal", "albedo", "t"):
                assert np.array_equal(sq._bits(guides[route][k]).reshape(-1), sq._bits(ref[k]).reshape(-1)), "%s %s: guide %s against shade_rays" % (name, route, k)
        finally:
            r.close()
    first = guides["transform_refit"]
    hit = first["t"] != f32(sq.TMAX)
    assert hit.sum() > T.W * T.H // 4 and len(np.unique(first["albedo"][hit], axis=0)) >= 4, "the camera sees the textures"
    for route in ROUTES:
        for k in ("albedo", "normal", "t"):
            assert np.array_equal(sq._bits(guides[route][k]), sq._bits(first[k])), "%s: guide %s over %s differs from transform_refit" % (name, k, route)
