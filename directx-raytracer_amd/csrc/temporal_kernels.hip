// HIP kernel for gfx950 (MI355X): temporal reprojection of crt_temporal_accumulate* (the contract is stated step by step in
// include/crt_hip.h, the reasons in DESIGN.md section 5h).  A pure image-space pass: it reads the caller's colour, guide and
// history buffers and two camera poses, and knows nothing of the scene.
//
//   one thread per pixel, a wavefront = 64 consecutive x of one row, a workgroup = 4 rows; the kernel strides over tiles.
//   The pixel's world point P = o_cur + rayDirJ(rot_cur, p) t is projected into the previous camera by inverting rayDirJ's
//   camera model; the four history records around that position are read as two float4 each, {c.rgb, len} and {n.xyz, t},
//   and weighted bilinearly.  Validity is predicated: a tap outside the image -- and every tap of a pixel that has no
//   position in the previous frame -- reads the centre's own record with weight 0, a tap that fails a test gets weight 0 and
//   its values are replaced by 0 before they are used, so no lane branches around a load and no NaN of a dead record
//   travels.  The only branch around the taps is uniform over the launch: no history buffer at all.
// No atomics, no LDS, no scratch: a pixel's sums run over its taps in a fixed order, so the same input gives the same bits.
//
// Arithmetic: float32, -ffp-contract=off; fused multiply-adds only where fmaf is written (dot3, the blend); / and sqrtf are
// correctly rounded.  Bit for bit tests/temporal_reference.c.  Nothing of the ray generation is restated: the directions are
// rayDirJ (shading.hip.h), called as the frame kernels call it.
//
// The motion variant (crt_temporal_accumulate_motion*, steps 4', 5', 7' and 9') is the same kernel instantiated with MOTION:
// a pixel whose prevPoint is finite projects that point instead of its own world point, always (the static-camera shortcut
// becomes a per-lane select), and its plane test is taken at that point.  The choice is uniform over the launch, so the plain
// entry point runs the instruction stream it ran before.
//
// The variance variant (crt_temporal_variance*, steps V1 to V5; section 5j) is the same kernel instantiated with MOMENTS: a tap
// grows by one 8-byte load, the luminance moments {m1, m2} of its record, which ride on the tap's weight.  Again uniform over
// the launch: the instantiations without MOMENTS compile to what they were.  Step V6, the variance itself, reads the records
// this kernel wrote for a pixel's neighbours and is a kernel of its own (variance_kernels.hip), launched behind this one.
#include "shading.hip.h"

#include <algorithm>
#include <cfloat>

namespace crt {
namespace {

constexpr uint32_t kTpTileX = 64, kTpTileY = 4; // pixels of a workgroup: one wavefront per row
constexpr uint32_t kTpMaxGrid = 1u << 20;       // workgroups of a launch; the kernel strides over what is left

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= FLT_MAX; } // false for NaN

template <bool MOTION, bool MOMENTS>
__global__ __launch_bounds__(256) void temporalKernel(const TemporalParams p)
{
    const float4* __restrict__ hist = reinterpret_cast<const float4*>(p.histPrev);
    float4* __restrict__ next = reinterpret_cast<float4*>(p.histNext);
    const float2* __restrict__ mom = reinterpret_cast<const float2*>(p.momPrev); // null exactly when hist is
    float2* __restrict__ momNext = reinterpret_cast<float2*>(p.momNext);
    const float fw = static_cast<float>(p.width), fh = static_cast<float>(p.height);
    const uint32_t tilesX = (p.width + kTpTileX - 1u) / kTpTileX, tilesY = (p.height + kTpTileY - 1u) / kTpTileY;
    const uint32_t nTiles = tilesX * tilesY; // < 2^28 for width * height <= 2^28
    const uint32_t lx = threadIdx.x & 63u, ly = threadIdx.x >> 6;
    const F3 oCur = f3(p.posCur[0], p.posCur[1], p.posCur[2]), oPrev = f3(p.posPrev[0], p.posPrev[1], p.posPrev[2]);
    for (uint32_t tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
        const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
        const uint32_t x = tx * kTpTileX + lx, y = ty * kTpTileY + ly;
        if (x >= p.width || y >= p.height) continue;
        const size_t pi = static_cast<size_t>(y) * p.width + x;
        const float r = p.rgb[3u * pi], g = p.rgb[3u * pi + 1u], b = p.rgb[3u * pi + 2u];
        const F3 n = f3(p.normal[3u * pi], p.normal[3u * pi + 1u], p.normal[3u * pi + 2u]);
        const float t = p.t[pi];
        float ar = 1.0f, ag = 1.0f, ab = 1.0f;
        bool live = finite1(r) && finite1(g) && finite1(b) && finite1(n.x) && finite1(n.y) && finite1(n.z) && finite1(t) &&
                    (n.x != 0.0f || n.y != 0.0f || n.z != 0.0f) && t > 0.0f;
        if (p.demodulate) {
            const float qr = p.albedo[3u * pi], qg = p.albedo[3u * pi + 1u], qb = p.albedo[3u * pi + 2u];
            live = live && finite1(qr) && finite1(qg) && finite1(qb);
            ar = fmaxf(qr, 1e-3f);
            ag = fmaxf(qg, 1e-3f);
            ab = fmaxf(qb, 1e-3f);
        }
        const float cr = r / ar, cg = g / ag, cb = b / ab;
        float outR = cr, outG = cg, outB = cb, outLen = 1.0f; // a live pixel without history
        float m1 = 0.0f, m2 = 0.0f, lum = 0.0f, lum2 = 0.0f;
        if (MOMENTS) { // step V1
            lum = fmaf(0.0722f, cb, fmaf(0.7152f, cg, 0.2126f * cr));
            lum2 = lum * lum;
            m1 = lum;
            m2 = lum2;
        }
        if (hist != nullptr) {
            // steps 4-7: where the pixel's world point was on the previous frame's screen
            const F3 d = rayDirJ(p.rotCur, x, y, 0.5f, 0.5f, fw, fh);
            const F3 P = f3(oCur.x + d.x * t, oCur.y + d.y * t, oCur.z + d.z * t);
            float fx = static_cast<float>(x), fy = static_cast<float>(y);
            bool proj = live;
            F3 Pm = P;         // step 4': where the pixel's surface element was in the previous frame
            bool moved = false;
            if (MOTION) {
                const F3 m = f3(p.prevPoint[3u * pi], p.prevPoint[3u * pi + 1u], p.prevPoint[3u * pi + 2u]);
                moved = finite1(m.x) && finite1(m.y) && finite1(m.z);
                Pm = moved ? m : P;
            }
            if (MOTION || !p.staticCamera) {
                const F3 v = sub3(Pm, oPrev);
                const float pcx = dot3(f3(p.rotPrev[0], p.rotPrev[3], p.rotPrev[6]), v);
                const float pcy = dot3(f3(p.rotPrev[1], p.rotPrev[4], p.rotPrev[7]), v);
                const float pcz = dot3(f3(p.rotPrev[2], p.rotPrev[5], p.rotPrev[8]), v);
                const float s = -pcz;
                const float sx = ((pcx / s) / (fw / fh) + 1.0f) * 0.5f * fw - 0.5f;
                const float sy = (1.0f - pcy / s) * 0.5f * fh - 0.5f;
                if (MOTION) { // step 7': a pixel that did not move under equal cameras keeps its own position
                    const bool shortcut = p.staticCamera && !moved;
                    const bool on = s > 0.0f && sx > -1.0f && sx < fw && sy > -1.0f && sy < fh; // (a NaN fails)
                    proj = proj && (shortcut || on);
                    fx = (proj && !shortcut) ? sx : fx;
                    fy = (proj && !shortcut) ? sy : fy;
                } else {
                    proj = proj && s > 0.0f && sx > -1.0f && sx < fw && sy > -1.0f && sy < fh; // (a NaN fails)
                    fx = proj ? sx : fx;
                    fy = proj ? sy : fy;
                }
            }
            // steps 8-10: the four taps
            const float x0 = floorf(fx), y0 = floorf(fy);
            const float wx = fx - x0, wy = fy - y0;
            const int ix = static_cast<int>(x0), iy = static_cast<int>(y0); // -1 .. width - 1, -1 .. height - 1
            const float limit = p.depthTolerance * t;
            float W = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f, sm1 = 0.0f, sm2 = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int qx = ix + (k & 1), qy = iy + (k >> 1);
                const float bk = ((k & 1) ? wx : 1.0f - wx) * ((k >> 1) ? wy : 1.0f - wy);
                const bool inside = proj & (static_cast<uint32_t>(qx) < p.width) & (static_cast<uint32_t>(qy) < p.height);
                const size_t qi = inside ? static_cast<size_t>(qy) * p.width + static_cast<size_t>(qx) : pi;
                const float4 hc = hist[2u * qi], hg = hist[2u * qi + 1u];
                bool usable = finite1(hc.x) && finite1(hc.y) && finite1(hc.z) && finite1(hc.w) && finite1(hg.x) && finite1(hg.y) &&
                              finite1(hg.z) && finite1(hg.w) && hc.w > 0.0f;
                float2 mq = make_float2(0.0f, 0.0f);
                if (MOMENTS) { // step V3
                    mq = mom[qi];
                    usable = usable && finite1(mq.x) && finite1(mq.y);
                }
                const F3 dq = rayDirJ(p.rotPrev, inside ? static_cast<uint32_t>(qx) : x, inside ? static_cast<uint32_t>(qy) : y, 0.5f, 0.5f, fw, fh);
                const F3 Pq = f3(oPrev.x + dq.x * hg.w, oPrev.y + dq.y * hg.w, oPrev.z + dq.z * hg.w);
                const float plane = fabsf(dot3(n, sub3(Pq, Pm)));
                const float nn = dot3(n, f3(hg.x, hg.y, hg.z));
                const bool ok = inside & usable & (plane <= limit) & (nn >= p.normalThreshold); // (a NaN fails either test)
                const float wk = ok ? bk : 0.0f;
                W = W + wk;
                sr = sr + wk * (ok ? hc.x : 0.0f);
                sg = sg + wk * (ok ? hc.y : 0.0f);
                sb = sb + wk * (ok ? hc.z : 0.0f);
                sl = sl + wk * (ok ? hc.w : 0.0f);
                if (MOMENTS) { // step V4
                    sm1 = sm1 + wk * (ok ? mq.x : 0.0f);
                    sm2 = sm2 + wk * (ok ? mq.y : 0.0f);
                }
            }
            if (W >= 0.01f) { // step 11
                const float hr = sr / W, hgn = sg / W, hb = sb / W, L = sl / W;
                const float at = fmaxf(p.alpha, 1.0f / (L + 1.0f));
                outR = fmaf(at, cr - hr, hr);
                outG = fmaf(at, cg - hgn, hgn);
                outB = fmaf(at, cb - hb, hb);
                outLen = fminf(L + 1.0f, p.maxHistory);
                if (MOMENTS) { // step V5
                    const float am = fmaxf(p.alphaMoments, 1.0f / (L + 1.0f));
                    const float h1 = sm1 / W, h2 = sm2 / W;
                    m1 = fmaf(am, lum - h1, h1);
                    m2 = fmaf(am, lum2 - h2, h2);
                }
            }
        }
        if (live) {
            next[2u * pi] = make_float4(outR, outG, outB, outLen);
            outR *= ar;
            outG *= ag;
            outB *= ab;
        } else { // step 3: its rgb bits as they came; never a tap
            next[2u * pi] = make_float4(r, g, b, 0.0f);
            outR = r;
            outG = g;
            outB = b;
        }
        next[2u * pi + 1u] = make_float4(n.x, n.y, n.z, t);
        if (MOMENTS) momNext[pi] = live ? make_float2(m1, m2) : make_float2(0.0f, 0.0f); // step V2
        if (p.out != nullptr) {
            p.out[3u * pi] = outR;
            p.out[3u * pi + 1u] = outG;
            p.out[3u * pi + 2u] = outB;
        }
    }
}

} // namespace

int launchTemporal(const TemporalParams& p, ihipStream_t* stream)
{
    const size_t tiles = static_cast<size_t>((p.width + kTpTileX - 1u) / kTpTileX) * ((p.height + kTpTileY - 1u) / kTpTileY);
    if (tiles == 0u) return static_cast<int>(hipSuccess);
    const dim3 g(static_cast<uint32_t>(std::min<size_t>(tiles, kTpMaxGrid))), block(256);
    if (p.momNext != nullptr) {
        if (p.prevPoint != nullptr) hipLaunchKernelGGL((temporalKernel<true, true>), g, block, 0, stream, p);
        else hipLaunchKernelGGL((temporalKernel<false, true>), g, block, 0, stream, p);
        if (const hipError_t e = hipGetLastError()) return static_cast<int>(e);
        return launchTemporalVariance(p, stream); // step V6, behind the records it reads
    }
    if (p.prevPoint != nullptr) hipLaunchKernelGGL((temporalKernel<true, false>), g, block, 0, stream, p);
    else hipLaunchKernelGGL((temporalKernel<false, false>), g, block, 0, stream, p);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
