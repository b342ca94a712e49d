// HIP kernels for gfx950 (MI355X): the edge-avoiding a-trous wavelet filter of crt_denoise* (Dammertz et al. 2010; the contract
// is stated in include/crt_hip.h, the reasons in DESIGN.md section 5g).  A pure image-space filter: it reads the caller's
// colour and guide buffers and knows nothing of the scene.
//
//   pack        one thread per pixel: the seven strided dwords a tap would need (rgb, normal, t) become two float4 planes,
//               colour {c.rgb, live} and guide {n.xyz, t}, c = rgb / max(albedo, 1e-3) when demodulating.  A pixel that is
//               not live keeps its rgb bits in the colour plane with live = 0 and is carried through every pass untouched.
//   pass i      one thread per pixel, a wavefront = 64 consecutive x of one row, a workgroup = 4 rows: every tap of every
//               stride is then a contiguous 1 KiB row segment per plane.  The 24 taps around a live centre are unrolled; a tap
//               outside the image reads the centre's own address and gets weight 0, a tap that is not live gets weight 0: the
//               weights are predicated, no lane branches inside the tap loop.  One exponential per tap, of the summed exponent.
//               The centre tap's exponent is 0 by definition: its weight is the constant 9/64.
//   last pass   the same, its result multiplied back by the albedo factor and written as 3 floats per pixel.
// The colour planes ping-pong; the guide plane is read-only after the pack.  No atomics: a pixel's sum runs over its taps in a
// fixed order, so the same input gives the same bits.
//
// Arithmetic: float32, -ffp-contract=off; fused multiply-adds where fmaf is written; expf is the library's.  Not bit-exact
// against any CPU form (exp has no such contract): the tests bound the deviation from a float64 reference.
#include "render_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace crt {
namespace {

constexpr uint32_t kDnTileX = 64, kDnTileY = 4; // pixels of a workgroup: one wavefront per row
constexpr uint32_t kDnMaxGrid = 1u << 20;       // workgroups of a launch; the kernels stride over what is left

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= FLT_MAX; } // false for NaN

__global__ __launch_bounds__(256) void denoisePackKernel(const DenoiseParams p)
{
    const size_t n = static_cast<size_t>(p.width) * p.height;
    float4* colour = reinterpret_cast<float4*>(p.colour[0]);
    float4* guide = reinterpret_cast<float4*>(p.guide);
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256u) {
        const float r = p.rgb[3u * i], g = p.rgb[3u * i + 1u], b = p.rgb[3u * i + 2u];
        const float nx = p.normal[3u * i], ny = p.normal[3u * i + 1u], nz = p.normal[3u * i + 2u];
        const float ar = p.albedo[3u * i], ag = p.albedo[3u * i + 1u], ab = p.albedo[3u * i + 2u];
        const float t = p.t[i];
        const bool finite = finite1(r) && finite1(g) && finite1(b) && finite1(nx) && finite1(ny) && finite1(nz) && finite1(ar) && finite1(ag) &&
                            finite1(ab) && finite1(t);
        const bool live = finite && (nx != 0.0f || ny != 0.0f || nz != 0.0f) && t > 0.0f;
        float4 c = make_float4(r, g, b, 0.0f);
        if (live) {
            c.w = 1.0f;
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

template <bool LAST>
__global__ __launch_bounds__(256) void denoisePassKernel(const DenoiseParams p, const float4* __restrict__ src, float4* __restrict__ dst, int stride,
                                                         float invSc2)
{
    const float4* __restrict__ guide = reinterpret_cast<const float4*>(p.guide);
    const uint32_t tilesX = (p.width + kDnTileX - 1u) / kDnTileX, tilesY = (p.height + kDnTileY - 1u) / kDnTileY;
    const uint32_t nTiles = tilesX * tilesY; // < 2^28 for width * height <= 2^28
    const uint32_t lx = threadIdx.x & 63u, ly = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
        const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
        const uint32_t x = tx * kDnTileX + lx, y = ty * kDnTileY + ly;
        if (x >= p.width || y >= p.height) continue;
        const size_t pi = static_cast<size_t>(y) * p.width + x;
        const float4 cp = src[pi];
        float rx = cp.x, ry = cp.y, rz = cp.z; // a pixel that is not live: its rgb bits as they came
        const bool live = cp.w != 0.0f;
        if (live) {
            const float4 gp = guide[pi];
            const float invZ = fminf(1.0f / (p.sigma_depth * gp.w), FLT_MAX); // 1 / (sigma_depth t_p), once per pixel
            constexpr float kCentre = 0.375f * 0.375f;
            float sx = kCentre * cp.x, sy = kCentre * cp.y, sz = kCentre * cp.z, sw = kCentre;
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    if (dx == 0 && dy == 0) continue;
                    const int qx = static_cast<int>(x) + dx * stride, qy = static_cast<int>(y) + dy * stride;
                    const bool inside = (static_cast<uint32_t>(qx) < p.width) & (static_cast<uint32_t>(qy) < p.height);
                    const size_t qi = inside ? static_cast<size_t>(qy) * p.width + static_cast<size_t>(qx) : pi;
                    const float4 cq = src[qi], gq = guide[qi];
                    const bool ok = inside & (cq.w != 0.0f);
                    const float dcx = cp.x - cq.x, dcy = cp.y - cq.y, dcz = cp.z - cq.z;
                    const float dnx = gp.x - gq.x, dny = gp.y - gq.y, dnz = gp.z - gq.z;
                    const float dz = (gp.w - gq.w) * invZ;
                    float e = fmaf(dcz, dcz, fmaf(dcy, dcy, dcx * dcx)) * invSc2;
                    e = fmaf(fmaf(dnz, dnz, fmaf(dny, dny, dnx * dnx)), p.inv_sigma_normal2, e);
                    e = fmaf(dz, dz, e);
                    const float k = kernelWeight(dx) * kernelWeight(dy); // (a constant once unrolled)
                    const float w = ok ? k * expf(-e) : 0.0f; // (a tap that is not live may hold anything, NaN included)
                    sx = fmaf(w, ok ? cq.x : 0.0f, sx);
                    sy = fmaf(w, ok ? cq.y : 0.0f, sy);
                    sz = fmaf(w, ok ? cq.z : 0.0f, sz);
                    sw += w;
                }
            }
            rx = sx / sw; // sw >= 9/64
            ry = sy / sw;
            rz = sz / sw;
        }
        if (LAST) {
            if (live && p.demodulate) {
                rx *= fmaxf(p.albedo[3u * pi], 1e-3f);
                ry *= fmaxf(p.albedo[3u * pi + 1u], 1e-3f);
                rz *= fmaxf(p.albedo[3u * pi + 2u], 1e-3f);
            }
            p.out[3u * pi] = rx;
            p.out[3u * pi + 1u] = ry;
            p.out[3u * pi + 2u] = rz;
        } else {
            dst[pi] = make_float4(rx, ry, rz, cp.w);
        }
    }
}

} // namespace

int launchDenoise(const DenoiseParams& p, ihipStream_t* stream)
{
    const size_t n = static_cast<size_t>(p.width) * p.height;
    if (n == 0u || p.iterations == 0u) return static_cast<int>(hipSuccess);
    const dim3 block(256);
    const dim3 gPack(static_cast<uint32_t>(std::min<size_t>((n + 255u) / 256u, kDnMaxGrid)));
    hipLaunchKernelGGL(denoisePackKernel, gPack, block, 0, stream, p);
    const size_t tiles = static_cast<size_t>((p.width + kDnTileX - 1u) / kDnTileX) * ((p.height + kDnTileY - 1u) / kDnTileY);
    const dim3 g(static_cast<uint32_t>(std::min<size_t>(tiles, kDnMaxGrid)));
    for (uint32_t i = 0; i < p.iterations; i++) {
        const float4* src = static_cast<const float4*>(p.colour[i & 1u]);
        float4* dst = static_cast<float4*>(p.colour[(i & 1u) ^ 1u]);
        const float invSc2 = std::fmin(std::ldexp(p.inv_sigma_color2, 2 * static_cast<int>(i)), FLT_MAX); // sigma_color halves every pass
        const int stride = 1 << i;
        if (i + 1u == p.iterations) hipLaunchKernelGGL((denoisePassKernel<true>), g, block, 0, stream, p, src, dst, stride, invSc2);
        else hipLaunchKernelGGL((denoisePassKernel<false>), g, block, 0, stream, p, src, dst, stride, invSc2);
    }
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
