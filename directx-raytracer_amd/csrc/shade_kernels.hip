// HIP kernel for gfx950 (MI355X): shaded ray queries on caller-supplied rays (crt_shade_rays*) -- the closest hit of
// ray_kernels.hip carried on through the frames' shading (shading.hip.h): the seven reference modes, or mode 100's Lambert /
// Phong sum with one any-hit shadow ray per light.  What DXR allows from any shader (TraceRay, then shade the result) and the
// reference only does from its own rayGen (R/HLSL/ray_tracing_shaders.hlsl:21-169).
//
// One job of runQuery (query.hip.h).  A lane's record goes through phases inside step():
//   closest hit   the record prescaled by 2^e (queryRay), exactly the traversal of crt_trace_rays
//   end of it     the hit outputs (t, uv, inst, prim), the surface (surfaceAt: normal, albedo) and, in a debug mode or on a
//                 miss, the colour are written and the record is finished.  In mode 100 on a hit the lane goes on:
//   shadow ray    for each light with a positive cosine, in light order, the lane becomes an any-hit traversal from the root
//                 with an empty stack: the frames' shadow ray (unit direction, not prescaled); when it ends the light is
//                 added (addLight, the code directLight adds it with) and the next light set up
//   after the last light the colour is written and only then `cur` becomes kDone, so that runQuery refills the lane.
// The shading functions get the record's own origin and direction (read again from the buffer when the closest hit ends: the
// prescaled direction may have lost low bits of small components) and the unscaled t = t' 2^-e: what the frame kernels hand
// them for a camera ray.  So a record that holds a frame's camera ray gives that pixel's rgb_f32 bit for bit.
//
// A wavefront holds lanes of both populations at once.  step() runs one scheduling decision of each: closestIteration for
// the lanes in their closest phase, then anyIteration for those on a shadow ray (each with its own node-step threshold over
// its own population).  Every ray, primary or shadow, is still walked by one lane in its own fixed order, so results and
// fetch counts do not depend on which lanes share a wavefront.
//
// Arithmetic contract: identical, operation for operation, to oracle/crt_oracle.c (compiled with -ffp-contract=off).
#include "query.hip.h"
#include "shading.hip.h"

namespace crt {
namespace {

// Register budget: 5 wavefronts per SIMD -- 91 VGPRs (95 counting), nothing spilled, no scratch.  At 6
// (80 VGPRs) 11 VGPRs spill inside the loop (19 counting).
constexpr int kShadeWaves = 5;

template <bool CNT>
struct ShadeJob {
    static constexpr int kClosest = -1; // `light` while the record's own ray is walked
    static constexpr int kIdle = -2;    // no record, or a finished one

    const ShadeQueryParams& q;
    Stack stack;
    Ray r;    // closest phase: the prescaled record; shadow phase: the shadow ray (r.o = the biased hit point)
    int cur;
    int light = kIdle;  // >= 0: the light whose shadow ray is being walked
    uint32_t idx = 0;   // the record
    float tmin = 0.0f, tmax = 0.0f, tcull = 0.0f; // closest phase: the prescaled interval (queryRay); shadow phase: (0, dist)
    // One set of registers for the two phases, which never need both: in the closest phase the best hit {t', u, v, tri, gid}
    // (w[0..4]), in the shadow phases the normal, the albedo and the running colour (w[0..2], [3..5], [6..8]).  As members of
    // their own the nine floats of the shadow phases stay allocated through the closest-hit loop (another lane of the
    // wavefront may be in a shadow phase) and the kernel does not fit 5 wavefronts per SIMD without spilling.
    float w[9];
    __device__ __forceinline__ Hit hit() const { return Hit{ w[0], w[1], w[2], __float_as_uint(w[3]), __float_as_uint(w[4]) }; }
    __device__ __forceinline__ void setHit(const Hit& h) { w[0] = h.t; w[1] = h.u; w[2] = h.v; w[3] = __uint_as_float(h.tri); w[4] = __uint_as_float(h.gid); }
    __device__ __forceinline__ F3 vec(int k) const { return f3(w[3 * k], w[3 * k + 1], w[3 * k + 2]); }
    __device__ __forceinline__ void setVec(int k, F3 v) { w[3 * k] = v.x; w[3 * k + 1] = v.y; w[3 * k + 2] = v.z; }
    static constexpr int kN = 0, kAlbedo = 1, kRgb = 2;
    uint32_t iters = 0;
    uint32_t cntShadow = 0;

    __device__ __forceinline__ explicit ShadeJob(const ShadeQueryParams& params) : q(params)
    {
        r = makeRay(f3(0.0f, 0.0f, 0.0f), f3(0.0f, 0.0f, 1.0f));
        for (float& x : w) x = 0.0f;
    }
    // (counting) the wavefront's shadow rays: runQuery adds the fetch counts itself and knows nothing of this one.  Runs when
    // runQuery's loop has ended, every lane active
    __device__ __forceinline__ ~ShadeJob()
    {
        if (CNT) {
            const uint32_t s = waveTotal(cntShadow);
            if ((threadIdx.x & 63u) == 0u) atomicAdd(&q.c.counters[2], static_cast<unsigned long long>(s));
        }
    }
    // everything is written where it becomes known (inside step): nothing of a finished record is held for this
    __device__ __forceinline__ void retire(uint32_t) {}
    __device__ __forceinline__ void start(uint32_t i)
    {
        const float4* rays = reinterpret_cast<const float4*>(q.c.records);
        const float4 a = rays[2u * static_cast<size_t>(i)], b = rays[2u * static_cast<size_t>(i) + 1u];
        idx = i;
        queryRay(a, b, r, tmin, tmax);
        setHit(Hit{ tmax, 0.0f, 0.0f, 0u, 0u });
        tcull = cullBound(tmax);
        light = kClosest;
        // a record with a NaN or an empty interval is not traced: step() finishes it as a miss
        cur = (queryRayOk(a, b, tmin, tmax) & (q.c.n_nodes != 0u)) ? LayLegacy::kRoot : LayLegacy::kDone;
    }
    static __device__ __forceinline__ void store3(float* out, uint32_t i, F3 v)
    {
        float* o = out + 3u * static_cast<size_t>(i);
        o[0] = v.x; o[1] = v.y; o[2] = v.z;
    }
    __device__ __forceinline__ void finish(F3 colour)
    {
        if (q.rgb) store3(q.rgb, idx, colour);
        light = kIdle;
        cur = LayLegacy::kDone;
    }
    // the shadow ray of the first light from `from` on that sees the surface from its front, or the end of the record
    __device__ __forceinline__ void nextLight(uint32_t from, F3 Po)
    {
        const LightRec* lights = reinterpret_cast<const LightRec*>(q.lights);
        for (uint32_t li = from; li < q.n_lights; li++) {
            const LightTerm lt = lightTerm(lights[li], Po, vec(kN));
            if (lt.cosv > 0.0f) {
                r = makeRay(Po, lt.Ld);
                tmin = 0.0f;
                tmax = lt.dist;
                tcull = lt.dist * kCullPad;
                stack.sp = 0;
                cur = LayLegacy::kRoot;
                light = static_cast<int>(li);
                if (CNT) cntShadow++;
                return;
            }
        }
        finish(vec(kRgb));
    }
    // the closest-hit traversal has ended (or never began): hit outputs, surface, colour or the first shadow ray
    __device__ __forceinline__ void endClosest()
    {
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        const float4* rays = reinterpret_cast<const float4*>(q.c.records);
        const float4 a = rays[2u * static_cast<size_t>(idx)], b = rays[2u * static_cast<size_t>(idx) + 1u];
        // the record's scale exponent and prescaled tmax again rather than carried (queryRay on the same record: the same bits)
        Ray scaled;
        float tminRec, tmaxRec;
        const int e = queryRay(a, b, scaled, tminRec, tmaxRec);
        const Hit h = hit();
        const bool isHit = h.t < tmaxRec;
        const bool lambert = q.mode >= 100u;
        uint32_t inst = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
        F3 colour = f3(q.miss[0], q.miss[1], q.miss[2]), nrm = f3(0.0f, 0.0f, 0.0f), alb = f3(0.0f, 0.0f, 0.0f), Po = nrm;
        const float t = isHit ? __builtin_amdgcn_ldexpf(h.t, -e) : b.w;
        if (isHit) { // (an empty scene has no triangle record to read)
            const float4* T = LayLegacy::triPtr(tris, h.tri);
            inst = __float_as_uint(T[0].w); // v0.w = mesh ordinal
            prim = __float_as_uint(T[1].w); // e1.w = triangle of the mesh
            Ray rec; // the record as the caller wrote it
            rec.o = f3(a.x, a.y, a.z);
            rec.d = f3(b.x, b.y, b.z);
            rec.idir = rec.noidn = f3(0.0f, 0.0f, 0.0f);
            Hit hr = h;
            hr.t = t;
            if (lambert || q.normal || q.albedo) {
                const Surface sf = surfaceAt(q, tris, rec, hr);
                nrm = sf.N;
                alb = sf.albedo;
                Po = biasPoint(sf.P, sf.N, kShadowBias);
            }
            if (!lambert) colour = shadeDebug(q.mode, inst, prim, t, h.u, h.v, rec.o, rec.d);
        }
        if (q.t) q.t[idx] = t;
        if (q.uv) reinterpret_cast<float2*>(q.uv)[idx] = make_float2(h.u, h.v);
        if (q.inst) q.inst[idx] = inst;
        if (q.prim) q.prim[idx] = prim;
        if (q.normal) store3(q.normal, idx, nrm);
        if (q.albedo) store3(q.albedo, idx, alb);
        if (isHit & lambert) {
            setVec(kN, nrm);
            setVec(kAlbedo, alb);
            setVec(kRgb, f3(0.0f, 0.0f, 0.0f));
            nextLight(0u, Po);
        } else finish(colour);
    }
    // a shadow ray has ended: its light's contribution, then the next light
    __device__ __forceinline__ void endShadow(bool occluded)
    {
        if (!occluded) {
            const LightRec Lt = reinterpret_cast<const LightRec*>(q.lights)[light];
            const LightTerm lt = lightTerm(Lt, r.o, vec(kN)); // (again rather than carried: the same inputs, the same bits)
            F3 view = f3(0.0f, 0.0f, 0.0f);
            if (q.phong_ks > 0.0f) { // Phong's view vector: minus the record's direction
                const float4 b = reinterpret_cast<const float4*>(q.c.records)[2u * static_cast<size_t>(idx) + 1u];
                view = f3(-b.x, -b.y, -b.z);
            }
            F3 rgb = vec(kRgb);
            addLight<true>(q, Lt, lt, vec(kN), vec(kAlbedo), view, rgb);
            setVec(kRgb, rgb);
        }
        nextLight(static_cast<uint32_t>(light) + 1u, r.o);
    }
    template <bool COUNT>
    __device__ __forceinline__ void step(uint32_t& cntNodes, uint32_t& cntTris)
    {
        static_assert(COUNT == CNT, "ShadeJob<COUNT> runs under runQuery<COUNT>");
        const float4* nodes = reinterpret_cast<const float4*>(q.c.nodes);
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        if (light == kClosest) {
            Hit h = hit();
            closestIteration<COUNT, 8>(nodes, tris, r, tmin, tcull, stack, static_cast<int>(q.c.inner_min), h, cur, iters, cntNodes, cntTris);
            setHit(h);
            tcull = cullBound(h.t); // (closestIteration sets t * kCullPad on an accepted hit: the same value for t >= 0)
            if (cur == LayLegacy::kDone) endClosest();
        } else if (light >= 0) {
            bool occluded = false; // (set by the leaf step that also ends the traversal: nothing to carry)
            anyIteration<COUNT, 8>(nodes, tris, r, tmin, tmax, tcull, stack, static_cast<int>(q.inner_min_any), occluded, cur, iters, cntNodes, cntTris);
            if (cur == LayLegacy::kDone) endShadow(occluded);
        }
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
