// Device-side ray generation and shading shared by the render kernel and the path-tracing pipeline: rayGen, the reference's
// closest-hit colour functions (modes 0..6), textures, the surface at a hit, direct light (Lambert + optional Phong, shadow
// rays), the counter-based RNG.  Internal to the including translation unit.
#pragma once

#include "traversal.hip.h"

namespace crt {
namespace {

// rayGen (hlsl:21-55) with width/height as parameters instead of the literals 1920/1080 (hlsl:24-25)
__device__ __forceinline__ F3 rayDirJ(const float* rot, uint32_t px, uint32_t py, float jx, float jy, float width, float height)
{
    float x = static_cast<float>(px), y = static_cast<float>(py);
    x += jx; // 0.5 in the reference (hlsl:35-36); the path tracer jitters inside the pixel
    y += jy;
    x /= width;
    y /= height;
    x = (2.0f * x) - 1.0f;
    y = 1.0f - (2.0f * y);
    x *= width / height;
    const F3 dc = normalize3(f3(x, y, -1.0f));
    const F3 dw = f3(dot3(f3(rot[0], rot[1], rot[2]), dc), dot3(f3(rot[3], rot[4], rot[5]), dc),
                     dot3(f3(rot[6], rot[7], rot[8]), dc));
    return normalize3(dw);
}

__device__ __forceinline__ F3 rayDir(const float* rot, uint32_t px, uint32_t py, float width, float height)
{
    return rayDirJ(rot, px, py, 0.5f, 0.5f, width, height);
}

__device__ __forceinline__ F3 objectBaseColour(uint32_t inst) // hlsl:97-101,117-121
{
    const float f = static_cast<float>(inst);
    return f3(hashSin(f * 12.9898f, 43758.5453f), hashSin(f * 78.233f, 12345.6789f), hashSin(f * 39.425f, 34567.8901f));
}

// closestHit, modes 0..6 (hlsl:78-169)
__device__ __forceinline__ F3 shadeDebug(uint32_t mode, uint32_t inst, uint32_t prim, float t, float u, float v, F3 o, F3 d)
{
    const F3 wp = f3(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);
    if (mode == 0) {
        const float f = static_cast<float>(prim);
        return f3(hashSin(f * 12.9898f, 43758.5453f), hashSin(f * 78.233f, 43758.5453f), hashSin(f * 45.164f, 43758.5453f));
    }
    if (mode == 1) {
        const F3 base = objectBaseColour(inst);
        const int cx = static_cast<int>(floorf(wp.x / 2.0f)), cy = static_cast<int>(floorf(wp.y / 2.0f)),
                  cz = static_cast<int>(floorf(wp.z / 2.0f));
        const uint32_t hash = (static_cast<uint32_t>(cx) * 73856093u) ^ (static_cast<uint32_t>(cy) * 19349663u) ^
                              (static_cast<uint32_t>(cz) * 83492791u);
        const float variation = hashSin(static_cast<float>(hash) * 12.9898f, 43758.5453f);
        return f3(lerp1(base.x * 0.7f, base.x * 1.3f, variation), lerp1(base.y * 0.7f, base.y * 1.3f, variation),
                  lerp1(base.z * 0.7f, base.z * 1.3f, variation));
    }
    if (mode == 2) {
        const F3 base = objectBaseColour(inst);
        const float shade = hashSin(static_cast<float>(prim) * 12.9898f, 43758.5453f);
        const float k = lerp1(0.6f, 1.0f, shade);
        return f3(base.x * k, base.y * k, base.z * k);
    }
    if (mode == 3) return f3(1.0f - u - v, u, v);
    if (mode == 4) {
        const float h = saturate1((wp.y + 10.0f) / 20.0f);
        return f3(lerp1(0.1f, 0.9f, h), lerp1(0.2f, 0.9f, h), lerp1(0.6f, 0.9f, h));
    }
    if (mode == 5) {
        const float c = saturate1(t * 0.05f);
        return f3(c, c, c);
    }
    const int checker = (static_cast<int>(floorf(wp.x)) ^ static_cast<int>(floorf(wp.z))) & 1;
    const float c = checker ? 0.9f : 0.2f;
    return f3(c, c, c);
}

struct LightRec { float x, y, z, intensity; };
struct MaterialRec { float r, g, b; uint32_t type; uint32_t smooth; float ior; int texture; };

// CRTTexture::getColor restated (R/CRTTexture*.cpp; oracle: texture_color)
__device__ __forceinline__ F3 textureColor(const TextureRec& t, const unsigned char* texels, float u, float v)
{
    const F3 A = f3(t.a[0], t.a[1], t.a[2]), B = f3(t.b[0], t.b[1], t.b[2]);
    if (t.type == 1u) return (u < t.scalar || v < t.scalar || (1.0f - u - v) < t.scalar) ? A : B; // edges
    if (t.type == 2u) { // checker
        // float -> int as include/crt_hip.h states it ("texture conversions"): v_cvt_i32_f32 truncates, saturates and turns NaN
        // into 0, which is the rule; the oracle and the host scene layer spell it out (tex_int / texInt)
        const int width = static_cast<int>(1.0f / t.scalar);
        const int u2 = static_cast<int>(floorf(u * static_cast<float>(width)));
        const int v2 = static_cast<int>(floorf(v * static_cast<float>(width)));
        return (((static_cast<uint32_t>(u2) + static_cast<uint32_t>(v2)) & 1u) == 0u) ? A : B; // parity of the wrapped sum (the CPU sides: (u2 ^ v2) & 1)
    }
    if (t.type == 3u) { // bitmap: nearest texel, v flipped
        if (t.channels < 3u || t.width == 0u) return f3(0.0f, 0.0f, 0.0f);
        u = fminf(fmaxf(u, 0.0f), 1.0f);
        v = fminf(fmaxf(v, 0.0f), 1.0f);
        const int row = static_cast<int>((1.0f - v) * static_cast<float>(static_cast<int>(t.height) - 1));
        const int col = static_cast<int>(u * static_cast<float>(static_cast<int>(t.width) - 1));
        const unsigned char* px = texels + t.texel_offset + (static_cast<size_t>(row) * t.width + static_cast<size_t>(col)) * t.channels;
        return f3(static_cast<float>(px[0]) / 255.0f, static_cast<float>(px[1]) / 255.0f, static_cast<float>(px[2]) / 255.0f);
    }
    return A; // albedo texture
}

// Surface at a closest hit (oracle: surface_at): hit point, shading normal flipped to face the ray, material
struct Surface {
    F3 P, N, albedo;
    uint32_t mtype;
    bool entering;
    float ior;
};

// P: the parameter block holding the scene's shading tables (RenderParams; ShadeQueryParams of the shaded ray queries).  Of r
// only o and d are read.
// NARROW: the triangle and shading records (48 bytes each) at a 32-bit byte offset from their bases (LayLegacy::triPtr)
template <bool NARROW = false, class P>
__device__ __forceinline__ Surface surfaceAt(const P& p, const float4* tris, const Ray& r, const Hit& h)
{
    Surface sf;
    const float4* T = LayLegacy::triPtr<NARROW>(tris, h.tri);
    const float4 tb = T[1], tc = T[2];
    const float* S = reinterpret_cast<const float*>(LayLegacy::triPtr<NARROW>(reinterpret_cast<const float4*>(p.shade), h.tri)); // shading / uv record: leaf order, 48 bytes as well
    const uint32_t material = __float_as_uint(S[9]);
    sf.P = f3(r.o.x + r.d.x * h.t, r.o.y + r.d.y * h.t, r.o.z + r.d.z * h.t);
    sf.albedo = f3(1.0f, 1.0f, 1.0f);
    sf.mtype = 1u;
    sf.ior = 1.0f;
    bool smooth = false;
    if (material < p.n_mats) {
        const MaterialRec* M = reinterpret_cast<const MaterialRec*>(p.mats) + material;
        sf.albedo = f3(M->r, M->g, M->b);
        smooth = M->smooth != 0;
        sf.mtype = M->type;
        sf.ior = M->ior;
        if (M->texture >= 0 && static_cast<uint32_t>(M->texture) < p.n_textures) {
            // CRTMaterial::isTexture: albedo from the texture; edges on the hit's barycentrics, the rest on the mesh uvs
            const TextureRec tx = reinterpret_cast<const TextureRec*>(p.textures)[M->texture];
            float tu = h.u, tv = h.v;
            if (tx.type != 1u) {
                tu = 0.0f;
                tv = 0.0f;
                if (p.uvs) {
                    const float* U = reinterpret_cast<const float*>(p.uvs) + 6 * static_cast<size_t>(h.tri);
                    const float w = 1.0f - h.u - h.v;
                    tu = fmaf(U[4], h.v, fmaf(U[2], h.u, U[0] * w));
                    tv = fmaf(U[5], h.v, fmaf(U[3], h.u, U[1] * w));
                }
            }
            sf.albedo = textureColor(tx, p.texels, tu, tv);
        }
    }
    F3 N = cross3(f3(tb.x, tb.y, tb.z), f3(tc.x, tc.y, tc.z));
    if (smooth) {
        const float w = 1.0f - h.u - h.v;
        const F3 Ns = f3(fmaf(S[6], h.v, fmaf(S[3], h.u, S[0] * w)), fmaf(S[7], h.v, fmaf(S[4], h.u, S[1] * w)),
                         fmaf(S[8], h.v, fmaf(S[5], h.u, S[2] * w)));
        if (dot3(Ns, Ns) > 0.0f) N = Ns;
    }
    N = normalize3(N);
    sf.entering = true;
    if (dot3(N, r.d) > 0.0f) {
        N = f3(-N.x, -N.y, -N.z);
        sf.entering = false;
    }
    sf.N = N;
    return sf;
}

__device__ __forceinline__ F3 biasPoint(F3 P, F3 N, float bias)
{
    return f3(fmaf(N.x, bias, P.x), fmaf(N.y, bias, P.y), fmaf(N.z, bias, P.z));
}

// x^n by square and multiply in the oracle's order (pow_uint)
__device__ __forceinline__ float powUint(float x, uint32_t n)
{
    float result = 1.0f, base = x;
    while (n) {
        if (n & 1u) result *= base;
        base *= base;
        n >>= 1;
    }
    return result;
}

// One light seen from Po with normal N: squared distance, distance, unit direction, clamped cosine.  A shadow ray is traced
// only for cosv > 0: origin Po, direction Ld, interval (0, dist).
struct LightTerm {
    F3 Ld;
    float r2, dist, cosv;
};
__device__ __forceinline__ LightTerm lightTerm(const LightRec& Lt, F3 Po, F3 N)
{
    LightTerm lt;
    const F3 Lv = sub3(f3(Lt.x, Lt.y, Lt.z), Po);
    lt.r2 = dot3(Lv, Lv);
    lt.dist = sqrtf(lt.r2);
    const float invr = 1.0f / lt.dist;
    lt.Ld = f3(Lv.x * invr, Lv.y * invr, Lv.z * invr);
    lt.cosv = fmaxf(0.0f, dot3(N, lt.Ld));
    return lt;
}

// An unoccluded light's contribution added to rgb: Lambert, and with PHONG (mode 100 only) the specular term
// ks * I / (4 pi r^2) * max(0, R . view)^n, R = the light direction mirrored about N.  P: the parameter block (phong_ks,
// phong_exp).  The one statement of the per-light arithmetic: directLight below and the shaded ray queries
// (shade_kernels.hip) both add a light through here.
template <bool PHONG, class P>
__device__ __forceinline__ void addLight(const P& p, const LightRec& Lt, const LightTerm& lt, F3 N, F3 albedo, F3 view, F3& rgb)
{
    const float k = (Lt.intensity / (kFourPi * lt.r2)) * lt.cosv;
    rgb.x = fmaf(albedo.x, k, rgb.x);
    rgb.y = fmaf(albedo.y, k, rgb.y);
    rgb.z = fmaf(albedo.z, k, rgb.z);
    if constexpr (PHONG) { // (a parameter block without the Phong options -- the path-traced ray queries' -- never gets here)
        if (p.phong_ks > 0.0f) {
            const float nl2 = 2.0f * dot3(N, lt.Ld);
            const F3 R = f3(fmaf(nl2, N.x, -lt.Ld.x), fmaf(nl2, N.y, -lt.Ld.y), fmaf(nl2, N.z, -lt.Ld.z));
            const float rv = fmaxf(0.0f, dot3(R, view));
            const float sp = (p.phong_ks * (Lt.intensity / (kFourPi * lt.r2))) * powUint(rv, p.phong_exp);
            rgb.x += sp; rgb.y += sp; rgb.z += sp;
        }
    }
}

// direct light at Po: one any-hit shadow ray per light with a positive cosine (oracle: direct_light)
template <bool COUNT, bool PHONG, bool NARROW = false>
__device__ __forceinline__ F3 directLight(const RenderParams& p, const float4* nodes, const float4* tris, F3 Po, F3 N, F3 albedo, F3 view,
                                          Stack& stack, uint32_t& iters, uint32_t& cntNodes, uint32_t& cntTris, uint32_t& cntShadow)
{
    F3 rgb = f3(0.0f, 0.0f, 0.0f);
    const LightRec* lights = reinterpret_cast<const LightRec*>(p.lights);
    for (uint32_t li = 0; li < p.n_lights; li++) {
        const LightRec Lt = lights[li];
        const LightTerm lt = lightTerm(Lt, Po, N);
        if (lt.cosv > 0.0f) {
            const Ray sr = makeRay(Po, lt.Ld);
            if (COUNT) cntShadow++;
            const bool occluded = traceAny<COUNT, true, NARROW>(nodes, tris, p.n_nodes, sr, 0.0f, lt.dist, stack, static_cast<int>(p.tune_inner_min_any), iters, cntNodes, cntTris, p.planes);
            if (!occluded) addLight<PHONG>(p, Lt, lt, N, albedo, view, rgb);
        }
    }
    return rgb;
}

// mode 100: Lambert (+ optional Phong highlight) + one shadow ray per light, every material treated as diffuse (oracle: shade_lambert)
template <bool COUNT, bool PHONG, bool NARROW = false>
__device__ __forceinline__ F3 shadeLambert(const RenderParams& p, const float4* nodes, const float4* tris, const Ray& r,
                                           const Hit& h, Stack& stack, uint32_t& iters, uint32_t& cntNodes, uint32_t& cntTris, uint32_t& cntShadow)
{
    const Surface sf = surfaceAt<NARROW>(p, tris, r, h);
    return directLight<COUNT, PHONG, NARROW>(p, nodes, tris, biasPoint(sf.P, sf.N, kShadowBias), sf.N, sf.albedo, f3(-r.d.x, -r.d.y, -r.d.z), stack, iters, cntNodes, cntTris, cntShadow);
}

// ---- mode 200: path tracing (oracle: trace_path). Counter-based RNG keyed by (pixel, sample, seed).
__device__ __forceinline__ uint32_t pcgHash(uint32_t v)
{
    const uint32_t state = v * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
__device__ __forceinline__ float rngNext(uint32_t& st)
{
    st = pcgHash(st);
    return static_cast<float>(st >> 8) * 0x1p-24f;
}

// ---- The path's directions at a surface: the mirror direction, the Snell branch and the cosine-weighted bounce (oracle:
// trace_path).  The one statement of each: streamShade (path_kernels.hip) and the path-traced ray queries
// (path_query_kernels.hip) both go through here.
__device__ __forceinline__ F3 mirrorDir(F3 d, F3 N) // not normalised
{
    const float k = 2.0f * dot3(d, N);
    return f3(fmaf(-k, N.x, d.x), fmaf(-k, N.y, d.y), fmaf(-k, N.z, d.z));
}
// The direction behind a REFRACTIVE surface, not normalised: Snell's, with Po (the point the path goes on from) moved to the
// far side of the surface; on total internal reflection the mirror direction, and Po stays
__device__ __forceinline__ F3 refractDir(F3 d, const Surface& sf, F3& Po)
{
    const float eta = sf.entering ? 1.0f / sf.ior : sf.ior;
    const float cosi = -dot3(d, sf.N);
    const float k = 1.0f - eta * eta * (1.0f - cosi * cosi);
    if (k < 0.0f) return mirrorDir(d, sf.N);
    const float m2 = eta * cosi - sqrtf(k);
    const F3 t = f3(fmaf(m2, sf.N.x, eta * d.x), fmaf(m2, sf.N.y, eta * d.y), fmaf(m2, sf.N.z, eta * d.z));
    Po = biasPoint(sf.P, sf.N, -kShadowBias);
    return t;
}
__device__ __forceinline__ F3 diffuseBounce(F3 N, float u1, float u2)
{
    const float rr = sqrtf(u1), phi = 6.28318530717958648f * u2;
    const float lx = rr * sinContract(phi + 1.57079632679489662f), ly = rr * sinContract(phi), lz = sqrtf(fmaxf(0.0f, 1.0f - u1));
    const float sg = copysignf(1.0f, N.z);
    const float a = -1.0f / (sg + N.z);
    const float b = N.x * N.y * a;
    const F3 T = f3(1.0f + sg * N.x * N.x * a, sg * b, -sg * N.x);
    const F3 Bv = f3(b, sg + N.y * N.y * a, -N.y);
    const F3 d = f3(fmaf(lz, N.x, fmaf(ly, Bv.x, lx * T.x)), fmaf(lz, N.y, fmaf(ly, Bv.y, lx * T.y)), fmaf(lz, N.z, fmaf(ly, Bv.z, lx * T.z)));
    return normalize3(d);
}

// Sample sums of one pixel (path_kernels.hip) or one record (path_query_kernels.hip): float64, one sample added at a time in
// sample order, resolved once as (float)(sum / total).  oracle_render sums and divides the same way.  loadSum / storeSum: the
// frames' layout, {x, y}, {z, 0} (two 16-byte words per pixel, index i -> words 2i, 2i + 1).
struct D3 { double x, y, z; };
__device__ __forceinline__ D3 loadSum(const void* sums, size_t i)
{
    const double2 a = static_cast<const double2*>(sums)[2u * i], b = static_cast<const double2*>(sums)[2u * i + 1u];
    return D3{ a.x, a.y, b.x };
}
__device__ __forceinline__ void storeSum(void* sums, size_t i, const D3& a)
{
    static_cast<double2*>(sums)[2u * i] = make_double2(a.x, a.y);
    static_cast<double2*>(sums)[2u * i + 1u] = make_double2(a.z, 0.0);
}
__device__ __forceinline__ D3 addSample(const D3& a, const float4& s)
{
    return D3{ a.x + static_cast<double>(s.x), a.y + static_cast<double>(s.y), a.z + static_cast<double>(s.z) };
}
__device__ __forceinline__ F3 sumMean(const D3& a, uint32_t total)
{
    const double n = static_cast<double>(total);
    return f3(static_cast<float>(a.x / n), static_cast<float>(a.y / n), static_cast<float>(a.z / n));
}

__device__ __forceinline__ uint32_t waveSum(uint32_t v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

} // namespace
} // namespace crt
