// HIP kernel for gfx950 (MI355X): shaded ray queries on caller-supplied rays (crt_shade_rays*) -- the closest hit of
// ray_kernels.hip carried on through the frames' shading (shading.hip.h): the seven reference modes, or mode 100's Lambert /
// Phong sum with one any-hit shadow ray per light.  What DXR allows from any shader (TraceRay, then shade the result) and the
// reference only does from its own rayGen (R/HLSL/ray_tracing_shaders.hlsl:21-169).
//
// One job of runQuery (query.hip.h) on the phase machine of lit_job.hip.h, and the plainest: one segment, then the lights.
//   end of the closest hit   the hit outputs (t, uv, inst, prim), the surface (surfaceAt: normal, albedo) and, in a debug mode or
//                 on a miss, the colour are written and the record is finished.  In mode 100 on a hit the lane goes on to
//                 its shadow rays
//   after the last light the colour is written and the record ends.
// The shading functions get the record's own origin and direction and the unscaled t (LitJob::segment0): what the frame kernels
// hand them for a camera ray.  So a record that holds a frame's camera ray gives that pixel's rgb_f32 bit for bit.
//
// Arithmetic contract: identical, operation for operation, to oracle/crt_oracle.c (compiled with -ffp-contract=off).
#include "lit_job.hip.h"

namespace crt {
namespace {

// Register budget (DESIGN.md sections 5e, 5x): 5 wavefronts per SIMD -- 91 VGPRs (93 counting), nothing spilled, no scratch.
// At 6 (80 VGPRs) VGPRs spill inside the loop.
constexpr int kShadeWaves = 5;

template <bool CNT>
struct ShadeJob : LitJob<ShadeJob<CNT>, ShadeQueryParams, CNT> {
    using Base = LitJob<ShadeJob<CNT>, ShadeQueryParams, CNT>;
    using Base::q; using Base::cur; using Base::light; using Base::idx; using Base::kIdle; using Base::kN;
    using Base::kAlbedo; using Base::kRgb; using Base::hit; using Base::vec; using Base::setVec; using Base::store3;
    using Base::nextLight;

    __device__ __forceinline__ explicit ShadeJob(const ShadeQueryParams& params) : Base(params) {}
    __device__ __forceinline__ ~ShadeJob() { this->addCounts(); }
    // the record ends with this colour
    __device__ __forceinline__ void finish(F3 colour)
    {
        if (q.out.rgb) store3(q.out.rgb, idx, colour);
        light = kIdle;
        cur = LayLegacy::kDone;
    }
    __device__ __forceinline__ void afterLights(F3) { finish(vec(kRgb)); }
    static constexpr bool kPhong = true; // Phong's view vector: minus the record's direction
    __device__ __forceinline__ F3 viewVector() const { return this->recordView(); }
    // the closest-hit traversal has ended (or never began): hit outputs, surface, colour or the first shadow ray
    __device__ __forceinline__ void endClosest()
    {
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        Hit h = hit();
        Ray rec; // the record as the caller wrote it
        rec.idir = rec.noidn = f3(0.0f, 0.0f, 0.0f);
        uint32_t inst = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
        const bool isHit = this->segment0(idx, h, rec);
        const bool lambert = q.mode >= 100u;
        F3 colour = f3(q.miss[0], q.miss[1], q.miss[2]), nrm = f3(0.0f, 0.0f, 0.0f), alb = f3(0.0f, 0.0f, 0.0f), Po = nrm;
        if (isHit) {
            inst = this->hitId(h, 0);
            prim = this->hitId(h, 1);
            if (lambert || q.out.normal || q.out.albedo) {
                const Surface sf = surfaceAt(q, tris, rec, h);
                nrm = sf.N;
                alb = sf.albedo;
                Po = biasPoint(sf.P, sf.N, kShadowBias);
            }
            if (!lambert) colour = shadeDebug(q.mode, inst, prim, h.t, h.u, h.v, rec.o, rec.d);
        }
        Base::storeHit(q.out, idx, h, inst, prim);
        if (q.out.normal) store3(q.out.normal, idx, nrm);
        if (q.out.albedo) store3(q.out.albedo, idx, alb);
        if (isHit & lambert) {
            setVec(kN, nrm);
            setVec(kAlbedo, alb);
            setVec(kRgb, f3(0.0f, 0.0f, 0.0f));
            nextLight(0u, Po);
        } else finish(colour);
    }
};

template <bool COUNT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kShadeWaves, 8))) void shadeQueryKernel(const ShadeQueryParams q)
{
    runQuery<COUNT, ShadeJob<COUNT>>(q);
}

} // namespace

// the kind of this file for launchQuery (render_kernels.h)
QueryKernel kKernelShade = { reinterpret_cast<const void*>(&shadeQueryKernel<false>), reinterpret_cast<const void*>(&shadeQueryKernel<true>), 1u };

} // namespace crt
