// HIP kernels for gfx950 (MI355X): temporal reprojection of crt_temporal_accumulate* and crt_temporal_variance* (the contracts are
// stated step by step in include/crt_hip.h, the reasons in DESIGN.md sections 5h and 5j).  Pure image-space passes: they read the
// caller's colour, guide and history buffers and two camera poses, and know nothing of the scene.  Both kernels walk the image
// as image_space.hip.h says: one thread per pixel, a wavefront = 64 consecutive x of one row, a workgroup = 4 rows.
//
// temporalKernel   The pixel's world point P = o_cur + rayDirJ(rot_cur, p) t is projected into the previous camera by inverting
//   rayDirJ's camera model; the four history records around that position are read as two float4 each, {c.rgb, len} and
//   {n.xyz, t}, and weighted bilinearly.  Validity is predicated: a tap outside the image -- and every tap of a pixel that has no
//   position in the previous frame -- reads the centre's own record with weight 0, a tap that fails a test gets weight 0 and
//   its values are replaced by 0 before they are used, so no lane branches around a load and no NaN of a dead record
//   travels.  The only branch around the taps is uniform over the launch: no history buffer at all.  No LDS, no scratch.
//
//   The motion variant (crt_temporal_accumulate_motion*, steps 4', 5', 7' and 9') is the same kernel instantiated with MOTION:
//   a pixel whose prevPoint is finite projects that point instead of its own world point, always (the static-camera shortcut
//   becomes a per-lane select), and its plane test is taken at that point.  The choice is uniform over the launch, so the plain
//   entry point runs the instruction stream it ran before.
//
//   The variance variant (crt_temporal_variance*, steps V1 to V5) is the same kernel instantiated with MOMENTS: a tap grows by
//   one 8-byte load, the luminance moments {m1, m2} of its record, which ride on the tap's weight.  Again uniform over the
//   launch: the instantiations without MOMENTS compile to what they were.
//
// temporalVarianceKernel   step V6, the variance itself, launched behind temporalKernel<., MOMENTS>, whose records {c.rgb, len},
//   {n.xyz, t} and {m1, m2} it reads for a pixel's neighbours.  A pixel with a long history needs its own record only.  A pixel
//   with a short one needs the 7 x 7 window, and every tap of it a ray direction: so the workgroup computes each pixel of its
//   70 x 10 halo once into LDS (22 KiB) -- the world point Pq = o_cur + rayDirJ * t, the normal and the moments, two
//   float4 -- and the 49 taps run out of LDS.  A record that may not be a tap (outside the image, len not > 0, a non-finite
//   value) gets a NaN normal there, which fails the normal test; the centre always counts and takes its own normal from its
//   registers.  A workgroup without a short pixel skips the halo, a wavefront without one skips the window: after a few frames
//   that is almost all of them.
// No atomics: a pixel's sums run over its taps in a fixed order, so the same input gives the same bits.
//
// Arithmetic: float32, -ffp-contract=off; fused multiply-adds only where fmaf is written (dot3, the blend, the luminance); / and
// sqrtf are correctly rounded.  Bit for bit tests/temporal_reference.c and tests/variance_reference.c.  Nothing of the ray
// generation is restated: the directions are rayDirJ (shading.hip.h), called as the frame kernels call it.
#include "image_space.hip.h"
#include "shading.hip.h"

namespace crt {
namespace {

constexpr int kVrRadius = 3; // the 7 x 7 window of step V6
constexpr uint32_t kVrHaloX = kTileX + 2u * kVrRadius, kVrHaloY = kTileY + 2u * kVrRadius; // 70 x 10

template <bool MOTION, bool MOMENTS>
__global__ __launch_bounds__(256) void temporalKernel(const TemporalParams p)
{
    const float4* __restrict__ hist = reinterpret_cast<const float4*>(p.histPrev);
    float4* __restrict__ next = reinterpret_cast<float4*>(p.histNext);
    const float2* __restrict__ mom = reinterpret_cast<const float2*>(p.momPrev); // null exactly when hist is
    float2* __restrict__ momNext = reinterpret_cast<float2*>(p.momNext);
    const float fw = static_cast<float>(p.width), fh = static_cast<float>(p.height);
    const TileWalk walk(p.width, p.height);
    const F3 oCur = f3(p.posCur[0], p.posCur[1], p.posCur[2]), oPrev = f3(p.posPrev[0], p.posPrev[1], p.posPrev[2]);
    for (uint32_t tile = blockIdx.x; tile < walk.nTiles; tile += gridDim.x) {
        const uint2 o = walk.origin(tile);
        const uint32_t x = o.x + walk.lx, y = o.y + walk.ly;
        if (x >= p.width || y >= p.height) continue;
        const size_t pi = static_cast<size_t>(y) * p.width + x;
        const float r = p.rgb[3u * pi], g = p.rgb[3u * pi + 1u], b = p.rgb[3u * pi + 2u];
        const F3 n = f3(p.normal[3u * pi], p.normal[3u * pi + 1u], p.normal[3u * pi + 2u]);
        const float t = p.t[pi];
        float ar = 1.0f, ag = 1.0f, ab = 1.0f;
        bool live = finite1(r) && finite1(g) && finite1(b) && finite1(n.x) && finite1(n.y) && finite1(n.z) && finite1(t) &&
                    guideLive(n.x, n.y, n.z, t);
        if (p.demodulate) {
            const float qr = p.albedo[3u * pi], qg = p.albedo[3u * pi + 1u], qb = p.albedo[3u * pi + 2u];
            live = live && finite1(qr) && finite1(qg) && finite1(qb);
            ar = albedoFloor(qr);
            ag = albedoFloor(qg);
            ab = albedoFloor(qb);
        }
        const float cr = r / ar, cg = g / ag, cb = b / ab;
        float outR = cr, outG = cg, outB = cb, outLen = 1.0f; // a live pixel without history
        float m1 = 0.0f, m2 = 0.0f, lum = 0.0f, lum2 = 0.0f;
        if (MOMENTS) { // step V1
            lum = luminance(cr, cg, cb);
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
                const bool inside = tapInside(p.width, p.height, qx, qy, proj);
                const size_t qi = inside ? pixelIndex(p.width, qx, qy) : pi;
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

// step V6 of crt_temporal_variance*
__global__ __launch_bounds__(256) void temporalVarianceKernel(const TemporalParams p)
{
    __shared__ float4 haloP[kVrHaloX * kVrHaloY]; // {Pq.xyz, m1}
    __shared__ float4 haloN[kVrHaloX * kVrHaloY]; // {n.xyz (x = NaN: never a tap), m2}
    const float4* __restrict__ hist = reinterpret_cast<const float4*>(p.histNext);
    const float2* __restrict__ mom = reinterpret_cast<const float2*>(p.momNext);
    const float fw = static_cast<float>(p.width), fh = static_cast<float>(p.height);
    const TileWalk walk(p.width, p.height);
    const uint32_t lx = walk.lx, ly = walk.ly;
    const F3 oCur = f3(p.posCur[0], p.posCur[1], p.posCur[2]);
    for (uint32_t tile = blockIdx.x; tile < walk.nTiles; tile += gridDim.x) { // (uniform over the workgroup: the barriers below are safe)
        const uint2 o = walk.origin(tile);
        const uint32_t x = o.x + lx, y = o.y + ly;
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
            const int hx0 = static_cast<int>(o.x) - kVrRadius, hy0 = static_cast<int>(o.y) - kVrRadius;
            for (uint32_t e = threadIdx.x; e < kVrHaloX * kVrHaloY; e += 256u) {
                const uint32_t ey = e / kVrHaloX, ex = e - ey * kVrHaloX;
                const int qx = hx0 + static_cast<int>(ex), qy = hy0 + static_cast<int>(ey);
                float4 hp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hn = make_float4(NAN, 0.0f, 0.0f, 0.0f);
                if (tapInside(p.width, p.height, qx, qy)) {
                    const size_t qi = pixelIndex(p.width, qx, qy);
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

} // namespace

int launchTemporal(const TemporalParams& p, ihipStream_t* stream)
{
    const dim3 g(tileGrid(p.width, p.height)), block(256);
    if (g.x == 0u) return static_cast<int>(hipSuccess);
    if (p.momNext != nullptr) {
        if (p.prevPoint != nullptr) hipLaunchKernelGGL((temporalKernel<true, true>), g, block, 0, stream, p);
        else hipLaunchKernelGGL((temporalKernel<false, true>), g, block, 0, stream, p);
        if (const hipError_t e = hipGetLastError()) return static_cast<int>(e);
        hipLaunchKernelGGL(temporalVarianceKernel, g, block, 0, stream, p); // behind the records it reads
    } else if (p.prevPoint != nullptr) {
        hipLaunchKernelGGL((temporalKernel<true, false>), g, block, 0, stream, p);
    } else {
        hipLaunchKernelGGL((temporalKernel<false, false>), g, block, 0, stream, p);
    }
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
