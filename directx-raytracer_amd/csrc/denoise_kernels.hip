// HIP kernels for gfx950 (MI355X): the edge-avoiding a-trous wavelet filter of crt_denoise* (Dammertz et al. 2010) and its
// variance-guided form of crt_denoise_variance* (SVGF).  The contracts are stated in include/crt_hip.h, the reasons in DESIGN.md
// sections 5g and 5j.  A pure image-space filter: it reads the caller's colour and guide buffers and knows nothing of the scene.
// One pack kernel and one pass kernel, instantiated with VARIANCE uniformly over the launch (variance != nullptr).
//
//   pack        one thread per pixel: the strided dwords a tap would need (rgb, normal, t, variance) become two float4 planes,
//               colour {c.rgb, v} and guide {n.xyz, t}, c = rgb / max(albedo, 1e-3) when demodulating.  v >= 0: live -- the
//               variance, which is never negative, or 0 for the plain filter; a pixel that is not live keeps its rgb bits in
//               the colour plane with v = -1 and is carried through every pass untouched.
//   pass i      the walk of image_space.hip.h: every tap of every stride is a contiguous 1 KiB row segment per plane.  The 24
//               taps around a live centre are unrolled; a tap outside the image reads the centre's own address and gets weight 0,
//               a tap that is not live gets weight 0: the weights are predicated, no lane branches inside the tap loop.  One
//               exponential per tap, of the summed exponent.  The centre tap's exponent is 0 by definition: its weight is the
//               constant 9/64.  The variants differ in the exponent's first term -- |dc|^2 / sigma_color^2, halved per pass on
//               the host, against |d lum| / (sigma_luminance sqrt(3 x 3 mean of v) + 1e-4), eight more stride-1 loads of the
//               fourth component per pass -- and in the fifth sum, the variance under the squared weights.
//   last pass   the same, its result multiplied back by the albedo factor and written as 3 floats (and the variance) per pixel.
// The colour planes ping-pong; the guide plane is read-only after the pack.  No atomics: a pixel's sum runs over its taps in a
// fixed order, so the same input gives the same bits.
//
// Arithmetic: float32, -ffp-contract=off; fused multiply-adds where fmaf is written; expf and sqrtf are the library's.  Not
// bit-exact against any CPU form (exp has no such contract): the tests bound the deviation from a float64 reference.
#include "image_space.hip.h"
#include "render_kernels.h"

#include <cmath>

namespace crt {
namespace {

template <bool VARIANCE>
__global__ __launch_bounds__(256) void denoisePackKernel(const DenoiseParams p)
{
    const size_t n = static_cast<size_t>(p.width) * p.height;
    float4* colour = reinterpret_cast<float4*>(p.colour[0]);
    float4* guide = reinterpret_cast<float4*>(p.guide);
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256u) {
        const float r = p.rgb[3u * i], g = p.rgb[3u * i + 1u], b = p.rgb[3u * i + 2u];
        const float nx = p.normal[3u * i], ny = p.normal[3u * i + 1u], nz = p.normal[3u * i + 2u];
        const float ar = p.albedo[3u * i], ag = p.albedo[3u * i + 1u], ab = p.albedo[3u * i + 2u];
        const float t = p.t[i], v = VARIANCE ? p.variance[i] : 0.0f;
        const bool finite = finite1(r) && finite1(g) && finite1(b) && finite1(nx) && finite1(ny) && finite1(nz) && finite1(ar) && finite1(ag) &&
                            finite1(ab) && finite1(t) && finite1(v);
        const bool live = finite && guideLive(nx, ny, nz, t) && v >= 0.0f;
        float4 c = make_float4(r, g, b, -1.0f);
        if (live) {
            c.w = v + 0.0f; // (-0 becomes +0: live is w >= 0)
            if (p.demodulate) {
                c.x = r / albedoFloor(ar);
                c.y = g / albedoFloor(ag);
                c.z = b / albedoFloor(ab);
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

// invSc2: 1 / sigma_color^2 of this pass (the plain filter's first term; unused with VARIANCE)
template <bool VARIANCE, bool LAST>
__global__ __launch_bounds__(256) void denoisePassKernel(const DenoiseParams p, const float4* __restrict__ src, float4* __restrict__ dst, int stride,
                                                         float invSc2)
{
    const float4* __restrict__ guide = reinterpret_cast<const float4*>(p.guide);
    const TileWalk walk(p.width, p.height);
    for (uint32_t tile = blockIdx.x; tile < walk.nTiles; tile += gridDim.x) {
        const uint2 o = walk.origin(tile);
        const uint32_t x = o.x + walk.lx, y = o.y + walk.ly;
        if (x >= p.width || y >= p.height) continue;
        const size_t pi = static_cast<size_t>(y) * p.width + x;
        const float4 cp = src[pi];
        float rx = cp.x, ry = cp.y, rz = cp.z, rv = cp.w; // a pixel that is not live: its rgb bits as they came
        const bool live = cp.w >= 0.0f;
        if (live) {
            const float4 gp = guide[pi];
            float invD = 0.0f;
            if (VARIANCE) {
                // the 3 x 3 mean of the variance, stride 1: k3 = (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4) over the taps inside and live
                float gs = 0.25f * cp.w, gk = 0.25f;
#pragma unroll
                for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        if (dx == 0 && dy == 0) continue;
                        const int qx = static_cast<int>(x) + dx, qy = static_cast<int>(y) + dy;
                        const bool inside = tapInside(p.width, p.height, qx, qy);
                        const float vq = src[inside ? pixelIndex(p.width, qx, qy) : pi].w;
                        const bool ok = inside & (vq >= 0.0f);
                        const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
                        gs = fmaf(ok ? k : 0.0f, ok ? vq : 0.0f, gs);
                        gk += ok ? k : 0.0f;
                    }
                }
                // 1 / d_p, once per pixel; +inf switches the term off, and so does a variance so large that d_p overflows
                const float dP = fmaf(p.sigma_first, sqrtf(gs / gk), 1e-4f);
                invD = p.sigma_first > FLT_MAX ? 0.0f : 1.0f / dP;
            }
            const float invZ = fminf(1.0f / (p.sigma_depth * gp.w), FLT_MAX); // 1 / (sigma_depth t_p), once per pixel
            const float lp = luminance(cp.x, cp.y, cp.z); // (lp, invD and the fifth sum sv: dead code without VARIANCE)
            constexpr float kCentre = 0.375f * 0.375f;
            float sx = kCentre * cp.x, sy = kCentre * cp.y, sz = kCentre * cp.z, sw = kCentre, sv = (kCentre * kCentre) * cp.w;
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    if (dx == 0 && dy == 0) continue;
                    const int qx = static_cast<int>(x) + dx * stride, qy = static_cast<int>(y) + dy * stride;
                    const bool inside = tapInside(p.width, p.height, qx, qy);
                    const size_t qi = inside ? pixelIndex(p.width, qx, qy) : pi;
                    const float4 cq = src[qi], gq = guide[qi];
                    const bool ok = inside & (cq.w >= 0.0f);
                    const float dcx = cp.x - cq.x, dcy = cp.y - cq.y, dcz = cp.z - cq.z;
                    const float dnx = gp.x - gq.x, dny = gp.y - gq.y, dnz = gp.z - gq.z;
                    const float dz = (gp.w - gq.w) * invZ;
                    float e = VARIANCE ? fabsf(lp - luminance(cq.x, cq.y, cq.z)) * invD : fmaf(dcz, dcz, fmaf(dcy, dcy, dcx * dcx)) * invSc2;
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
            if (VARIANCE) rv = sv / (sw * sw);
        }
        if (LAST) {
            if (live && p.demodulate) {
                rx *= albedoFloor(p.albedo[3u * pi]);
                ry *= albedoFloor(p.albedo[3u * pi + 1u]);
                rz *= albedoFloor(p.albedo[3u * pi + 2u]);
            }
            if (VARIANCE && p.varianceOut != nullptr) p.varianceOut[pi] = live ? rv : p.variance[pi]; // not live: its bits as they came
            p.out[3u * pi] = rx;
            p.out[3u * pi + 1u] = ry;
            p.out[3u * pi + 2u] = rz;
        } else {
            dst[pi] = make_float4(rx, ry, rz, rv);
        }
    }
}

// pack, iterations - 1 passes, and the last pass fused with the multiply-back
template <bool VARIANCE>
int launchFilter(const DenoiseParams& p, ihipStream_t* stream)
{
    const size_t n = static_cast<size_t>(p.width) * p.height;
    if (n == 0u || p.iterations == 0u) return static_cast<int>(hipSuccess);
    const dim3 block(256), g(tileGrid(p.width, p.height));
    hipLaunchKernelGGL(denoisePackKernel<VARIANCE>, dim3(cappedGrid((n + 255u) / 256u)), block, 0, stream, p);
    for (uint32_t i = 0; i < p.iterations; i++) {
        const float4* src = static_cast<const float4*>(p.colour[i & 1u]);
        float4* dst = static_cast<float4*>(p.colour[(i & 1u) ^ 1u]);
        const float invSc2 = VARIANCE ? 0.0f : std::fmin(std::ldexp(p.sigma_first, 2 * static_cast<int>(i)), FLT_MAX); // sigma_color halves every pass
        const int stride = 1 << i;
        if (i + 1u == p.iterations) hipLaunchKernelGGL((denoisePassKernel<VARIANCE, true>), g, block, 0, stream, p, src, dst, stride, invSc2);
        else hipLaunchKernelGGL((denoisePassKernel<VARIANCE, false>), g, block, 0, stream, p, src, dst, stride, invSc2);
    }
    return static_cast<int>(hipGetLastError());
}

} // namespace

int launchDenoise(const DenoiseParams& p, ihipStream_t* stream)
{
    return p.variance != nullptr ? launchFilter<true>(p, stream) : launchFilter<false>(p, stream);
}

} // namespace crt
