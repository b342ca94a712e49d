// HIP kernels for gfx950 (MI355X): the variance half of the SVGF pair (the contracts are stated in include/crt_hip.h, "variance",
// the reasons in DESIGN.md section 5j).  Pure image-space passes: they read the caller's buffers and know nothing of the scene.
//
// temporalVarianceKernel   step V6 of crt_temporal_variance*, launched behind temporalKernel<., MOMENTS> (temporal_kernels.hip),
//               whose records {c.rgb, len}, {n.xyz, t} and {m1, m2} it reads.  One thread per pixel, a wavefront = 64 consecutive
//               x of one row, a workgroup = 4 rows.  A pixel with a long history needs its own record only.  A pixel with a short
//               one needs the 7 x 7 window, and every tap of it a ray direction: so the workgroup computes each pixel of its 70 x
//               10 halo once into LDS -- the world point Pq = o_cur + rayDirJ * t, the normal and the moments, two float4 -- and
//               the 49 taps run out of LDS.  A record that may not be a tap (outside the image, len not > 0, a non-finite value)
//               gets a NaN normal there, which fails the normal test; the centre always counts and takes its own normal from its
//               registers.  A workgroup without a short pixel skips the halo, a wavefront without one skips the window: after a
//               few frames that is almost all of them.
// packVariance / passVariance   crt_denoise_variance*: the shape of denoise_kernels.hip, with the variance in the colour plane's
//               fourth component ({c.rgb, v}; v < 0: not live -- a live variance is never negative), so a tap stays at two float4
//               loads.  The 3 x 3 prefilter of the variance adds eight stride-1 loads of that component per pass.
// No atomics: a pixel's sums run over its taps in a fixed order, so the same input gives the same bits.
//
// Arithmetic: float32, -ffp-contract=off; fused multiply-adds only where fmaf is written.  temporalVarianceKernel is bit for bit
// tests/variance_reference.c; nothing of the ray generation is restated: the directions are rayDirJ (shading.hip.h), called as the
// frame kernels call it.  The filter uses the library's expf and sqrtf and is held to a float64 reference by a deviation bound.
#include "shading.hip.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace crt {
namespace {

constexpr uint32_t kVrTileX = 64, kVrTileY = 4; // pixels of a workgroup: one wavefront per row
constexpr uint32_t kVrMaxGrid = 1u << 20;       // workgroups of a launch; the kernels stride over what is left
constexpr int kVrRadius = 3;                    // the 7 x 7 window of step V6
constexpr uint32_t kVrHaloX = kVrTileX + 2u * kVrRadius, kVrHaloY = kVrTileY + 2u * kVrRadius; // 70 x 10

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= FLT_MAX; } // false for NaN

__global__ __launch_bounds__(256) void temporalVarianceKernel(const TemporalParams p)
{
    __shared__ float4 haloP[kVrHaloX * kVrHaloY]; // {Pq.xyz, m1}
    __shared__ float4 haloN[kVrHaloX * kVrHaloY]; // {n.xyz (x = NaN: never a tap), m2}
    const float4* __restrict__ hist = reinterpret_cast<const float4*>(p.histNext);
    const float2* __restrict__ mom = reinterpret_cast<const float2*>(p.momNext);
    const float fw = static_cast<float>(p.width), fh = static_cast<float>(p.height);
    const uint32_t tilesX = (p.width + kVrTileX - 1u) / kVrTileX, tilesY = (p.height + kVrTileY - 1u) / kVrTileY;
    const uint32_t nTiles = tilesX * tilesY; // < 2^28 for width * height <= 2^28
    const uint32_t lx = threadIdx.x & 63u, ly = threadIdx.x >> 6;
    const F3 oCur = f3(p.posCur[0], p.posCur[1], p.posCur[2]);
    for (uint32_t tile = blockIdx.x; tile < nTiles; tile += gridDim.x) { // (uniform over the workgroup: the barriers below are safe)
        const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
        const uint32_t x = tx * kVrTileX + lx, y = ty * kVrTileY + ly;
        const bool inImage = x < p.width && y < p.height;
        const size_t pi = inImage ? static_cast<size_t>(y) * p.width + x : 0u;
        float4 hc = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hg = hc;
        float2 mp = make_float2(0.0f, 0.0f);
        if (inImage) {
            hc = hist[2u * pi];
            hg = hist[2u * pi + 1u];
            mp = mom[pi];
        }
        const float len = hc.w;
        const bool live = inImage && len > 0.0f; // a live pixel was written with len >= 1, any other with 0
        const bool isShort = live && !(len >= p.minHistory);
        float var = live ? fmaxf(mp.y - mp.x * mp.x, 0.0f) : 0.0f; // the long branch
        if (__syncthreads_or(isShort ? 1 : 0)) {
            const int hx0 = static_cast<int>(tx * kVrTileX) - kVrRadius, hy0 = static_cast<int>(ty * kVrTileY) - kVrRadius;
            for (uint32_t e = threadIdx.x; e < kVrHaloX * kVrHaloY; e += 256u) {
                const uint32_t ey = e / kVrHaloX, ex = e - ey * kVrHaloX;
                const int qx = hx0 + static_cast<int>(ex), qy = hy0 + static_cast<int>(ey);
                float4 hp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hn = make_float4(NAN, 0.0f, 0.0f, 0.0f);
                if ((static_cast<uint32_t>(qx) < p.width) & (static_cast<uint32_t>(qy) < p.height)) {
                    const size_t qi = static_cast<size_t>(qy) * p.width + static_cast<size_t>(qx);
                    const float4 qc = hist[2u * qi], qg = hist[2u * qi + 1u];
                    const float2 qm = mom[qi];
                    const bool tap = qc.w > 0.0f && finite1(qc.x) && finite1(qc.y) && finite1(qc.z) && finite1(qc.w) && finite1(qg.x) &&
                                     finite1(qg.y) && finite1(qg.z) && finite1(qg.w) && finite1(qm.x) && finite1(qm.y);
                    const F3 d = rayDirJ(p.rotCur, static_cast<uint32_t>(qx), static_cast<uint32_t>(qy), 0.5f, 0.5f, fw, fh);
                    hp = make_float4(oCur.x + d.x * qg.w, oCur.y + d.y * qg.w, oCur.z + d.z * qg.w, qm.x);
                    hn = make_float4(tap ? qg.x : NAN, qg.y, qg.z, qm.y);
                }
                haloP[e] = hp;
                haloN[e] = hn;
            }
            __syncthreads();
            if (__any(isShort ? 1 : 0)) { // (uniform over the wavefront)
                const uint32_t ce = (ly + kVrRadius) * kVrHaloX + lx + kVrRadius;
                const float4 cP = haloP[ce];
                const F3 P = f3(cP.x, cP.y, cP.z), n = f3(hg.x, hg.y, hg.z);
                const float limit = p.depthTolerance * hg.w;
                float N = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
                for (int dy = -kVrRadius; dy <= kVrRadius; dy++) {
#pragma unroll
                    for (int dx = -kVrRadius; dx <= kVrRadius; dx++) {
                        const uint32_t qe = static_cast<uint32_t>(static_cast<int>(ce) + dy * static_cast<int>(kVrHaloX) + dx);
                        const float4 qP = haloP[qe], qN = haloN[qe];
                        const float plane = fabsf(dot3(n, sub3(f3(qP.x, qP.y, qP.z), P)));
                        const float nn = dot3(n, f3(qN.x, qN.y, qN.z));
                        const bool ok = (dx == 0 && dy == 0) || ((plane <= limit) & (nn >= p.normalThreshold)); // (a NaN fails either test)
                        N = N + (ok ? 1.0f : 0.0f);
                        a1 = a1 + (ok ? qP.w : 0.0f);
                        a2 = a2 + (ok ? qN.w : 0.0f);
                    }
                }
                const float M1 = a1 / N, M2 = a2 / N;
                const float spatial = fmaxf(M2 - M1 * M1, 0.0f) * (p.minHistory / len);
                var = isShort ? spatial : var;
            }
            __syncthreads(); // the next tile refills the halo
        }
        if (inImage) p.variance[pi] = var;
    }
}

// ---- crt_denoise_variance*

__global__ __launch_bounds__(256) void packVarianceKernel(const DenoiseVarianceParams p)
{
    const size_t n = static_cast<size_t>(p.width) * p.height;
    float4* colour = reinterpret_cast<float4*>(p.colour[0]);
    float4* guide = reinterpret_cast<float4*>(p.guide);
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256u) {
        const float r = p.rgb[3u * i], g = p.rgb[3u * i + 1u], b = p.rgb[3u * i + 2u];
        const float nx = p.normal[3u * i], ny = p.normal[3u * i + 1u], nz = p.normal[3u * i + 2u];
        const float ar = p.albedo[3u * i], ag = p.albedo[3u * i + 1u], ab = p.albedo[3u * i + 2u];
        const float t = p.t[i], v = p.variance[i];
        const bool finite = finite1(r) && finite1(g) && finite1(b) && finite1(nx) && finite1(ny) && finite1(nz) && finite1(ar) && finite1(ag) &&
                            finite1(ab) && finite1(t) && finite1(v);
        const bool live = finite && (nx != 0.0f || ny != 0.0f || nz != 0.0f) && t > 0.0f && v >= 0.0f;
        float4 c = make_float4(r, g, b, -1.0f);
        if (live) {
            c.w = v + 0.0f; // (-0 becomes +0: live is w >= 0)
            if (p.demodulate) {
                c.x = r / fmaxf(ar, 1e-3f);
                c.y = g / fmaxf(ag, 1e-3f);
                c.z = b / fmaxf(ab, 1e-3f);
            }
        }
        colour[i] = c;
        guide[i] = make_float4(nx, ny, nz, t);
    }
}

// h (x) h of h = (1/16, 1/4, 3/8, 1/4, 1/16); every product is exact in float
__device__ __forceinline__ constexpr float kernelWeight(int d)
{
    return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

__device__ __forceinline__ float luminance(float r, float g, float b) { return fmaf(0.0722f, b, fmaf(0.7152f, g, 0.2126f * r)); }

template <bool LAST>
__global__ __launch_bounds__(256) void passVarianceKernel(const DenoiseVarianceParams p, const float4* __restrict__ src, float4* __restrict__ dst,
                                                          int stride)
{
    const float4* __restrict__ guide = reinterpret_cast<const float4*>(p.guide);
    const uint32_t tilesX = (p.width + kVrTileX - 1u) / kVrTileX, tilesY = (p.height + kVrTileY - 1u) / kVrTileY;
    const uint32_t nTiles = tilesX * tilesY; // < 2^28 for width * height <= 2^28
    const uint32_t lx = threadIdx.x & 63u, ly = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
        const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
        const uint32_t x = tx * kVrTileX + lx, y = ty * kVrTileY + ly;
        if (x >= p.width || y >= p.height) continue;
        const size_t pi = static_cast<size_t>(y) * p.width + x;
        const float4 cp = src[pi];
        float rx = cp.x, ry = cp.y, rz = cp.z, rv = cp.w; // a pixel that is not live: its rgb bits as they came
        const bool live = cp.w >= 0.0f;
        if (live) {
            const float4 gp = guide[pi];
            // the 3 x 3 mean of the variance, stride 1: k3 = (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4) over the taps inside and live
            float gs = 0.25f * cp.w, gk = 0.25f;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    if (dx == 0 && dy == 0) continue;
                    const int qx = static_cast<int>(x) + dx, qy = static_cast<int>(y) + dy;
                    const bool inside = (static_cast<uint32_t>(qx) < p.width) & (static_cast<uint32_t>(qy) < p.height);
                    const size_t qi = inside ? static_cast<size_t>(qy) * p.width + static_cast<size_t>(qx) : pi;
                    const float vq = src[qi].w;
                    const bool ok = inside & (vq >= 0.0f);
                    const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
                    gs = fmaf(ok ? k : 0.0f, ok ? vq : 0.0f, gs);
                    gk += ok ? k : 0.0f;
                }
            }
            // 1 / d_p, once per pixel; +inf switches the term off, and so does a variance so large that d_p overflows
            const float dP = fmaf(p.sigma_luminance, sqrtf(gs / gk), 1e-4f);
            const float invD = p.sigma_luminance > FLT_MAX ? 0.0f : 1.0f / dP;
            const float invZ = fminf(1.0f / (p.sigma_depth * gp.w), FLT_MAX); // 1 / (sigma_depth t_p)
            const float lp = luminance(cp.x, cp.y, cp.z);
            constexpr float kCentre = 0.375f * 0.375f;
            float sx = kCentre * cp.x, sy = kCentre * cp.y, sz = kCentre * cp.z, sw = kCentre, sv = (kCentre * kCentre) * cp.w;
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    if (dx == 0 && dy == 0) continue;
                    const int qx = static_cast<int>(x) + dx * stride, qy = static_cast<int>(y) + dy * stride;
                    const bool inside = (static_cast<uint32_t>(qx) < p.width) & (static_cast<uint32_t>(qy) < p.height);
                    const size_t qi = inside ? static_cast<size_t>(qy) * p.width + static_cast<size_t>(qx) : pi;
                    const float4 cq = src[qi], gq = guide[qi];
                    const bool ok = inside & (cq.w >= 0.0f);
                    const float dl = fabsf(lp - luminance(cq.x, cq.y, cq.z));
                    const float dnx = gp.x - gq.x, dny = gp.y - gq.y, dnz = gp.z - gq.z;
                    const float dz = (gp.w - gq.w) * invZ;
                    float e = dl * invD;
                    e = fmaf(fmaf(dnz, dnz, fmaf(dny, dny, dnx * dnx)), p.inv_sigma_normal2, e);
                    e = fmaf(dz, dz, e);
                    const float k = kernelWeight(dx) * kernelWeight(dy); // (a constant once unrolled)
                    const float w = ok ? k * expf(-e) : 0.0f; // (a tap that is not live may hold anything, NaN included)
                    sx = fmaf(w, ok ? cq.x : 0.0f, sx);
                    sy = fmaf(w, ok ? cq.y : 0.0f, sy);
                    sz = fmaf(w, ok ? cq.z : 0.0f, sz);
                    sv = fmaf(w * w, ok ? cq.w : 0.0f, sv);
                    sw += w;
                }
            }
            rx = sx / sw; // sw >= 9/64
            ry = sy / sw;
            rz = sz / sw;
            rv = sv / (sw * sw);
        }
        if (LAST) {
            if (live && p.demodulate) {
                rx *= fmaxf(p.albedo[3u * pi], 1e-3f);
                ry *= fmaxf(p.albedo[3u * pi + 1u], 1e-3f);
                rz *= fmaxf(p.albedo[3u * pi + 2u], 1e-3f);
            }
            if (p.varianceOut != nullptr) p.varianceOut[pi] = live ? rv : p.variance[pi]; // not live: its bits as they came
            p.out[3u * pi] = rx;
            p.out[3u * pi + 1u] = ry;
            p.out[3u * pi + 2u] = rz;
        } else {
            dst[pi] = make_float4(rx, ry, rz, rv);
        }
    }
}

} // namespace

int launchTemporalVariance(const TemporalParams& p, ihipStream_t* stream)
{
    const size_t tiles = static_cast<size_t>((p.width + kVrTileX - 1u) / kVrTileX) * ((p.height + kVrTileY - 1u) / kVrTileY);
    if (tiles == 0u) return static_cast<int>(hipSuccess);
    const dim3 g(static_cast<uint32_t>(std::min<size_t>(tiles, kVrMaxGrid))), block(256);
    hipLaunchKernelGGL(temporalVarianceKernel, g, block, 0, stream, p);
    return static_cast<int>(hipGetLastError());
}

int launchDenoiseVariance(const DenoiseVarianceParams& p, ihipStream_t* stream)
{
    const size_t n = static_cast<size_t>(p.width) * p.height;
    if (n == 0u || p.iterations == 0u) return static_cast<int>(hipSuccess);
    const dim3 block(256);
    const dim3 gPack(static_cast<uint32_t>(std::min<size_t>((n + 255u) / 256u, kVrMaxGrid)));
    hipLaunchKernelGGL(packVarianceKernel, gPack, block, 0, stream, p);
    const size_t tiles = static_cast<size_t>((p.width + kVrTileX - 1u) / kVrTileX) * ((p.height + kVrTileY - 1u) / kVrTileY);
    const dim3 g(static_cast<uint32_t>(std::min<size_t>(tiles, kVrMaxGrid)));
    for (uint32_t i = 0; i < p.iterations; i++) {
        const float4* src = static_cast<const float4*>(p.colour[i & 1u]);
        float4* dst = static_cast<float4*>(p.colour[(i & 1u) ^ 1u]);
        const int stride = 1 << i;
        if (i + 1u == p.iterations) hipLaunchKernelGGL((passVarianceKernel<true>), g, block, 0, stream, p, src, dst, stride);
        else hipLaunchKernelGGL((passVarianceKernel<false>), g, block, 0, stream, p, src, dst, stride);
    }
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
