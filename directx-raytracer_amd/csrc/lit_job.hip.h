// The phase machine of the four lit-ray jobs of runQuery (query.hip.h): ShadeJob (shade_kernels.hip, modes 0..100), AmbientJob
// (ao_kernels.hip, mode 120), WhittedJob (whitted_kernels.hip, mode 150) and PathJob (path_query_kernels.hip, mode 200).  A lane's
// record goes through phases inside step():
//   closest hit   `light` = kClosest: a closest-hit traversal.  Segment 0 is the record prescaled by 2^e (queryRay), exactly the
//                 traversal of crt_trace_rays; a job that goes on behind a surface walks plain unit-direction rays (its goOn)
//   end of it     the job's endClosest(): segment 0 gives the hit outputs (segment0, hitId, storeHit); then the surface, and the
//                 record ends, goes on, or is lit (nextLight(0, biased hit point))
//   shadow ray    `light` >= 0: for each light with a positive cosine, in light order, the lane becomes an any-hit traversal from
//                 the root with an empty stack: the frames' shadow ray (unit direction, not prescaled); when it ends the light
//                 is added (endShadow: lightTerm and addLight, the code directLight adds it with) and the next light set up
//   after the last light the job's afterLights().  `cur` becomes kDone only when the job has written what it keeps of the
//   record, so that runQuery refills the lane then and retire() has nothing to do.
// A wavefront holds lanes of both populations at once.  step() runs one scheduling decision of each: closestIteration for
// the lanes in their closest phase, then anyIteration for those on an any-hit ray (each with its own node-step threshold over
// its own population).  Every ray is still walked by one lane in its own fixed order, so results and fetch counts do not
// depend on which lanes share a wavefront.
//
// A job derives from LitJob<Job, its parameter struct, CNT> and supplies, as plain members found through static_cast (no
// virtuals):
//   endClosest()      a closest-hit traversal has ended (or, for an untraced record, never began)
//   afterLights(Po)   every light has been asked
//   kPhong            whether addLight takes the Phong term, and then viewVector(): Phong's view vector
//   ~Job()            calls addCounts
// and may replace start() (runQuery's: PathJob, whose work items are not records; WhittedJob adds its slot word) and anyHit() /
// endAny(), to walk any-hit rays of its own beside the shadow rays (AmbientJob).
//
// The order of the members is part of the device code: the compiler names registers in it.  So are the shapes of the helpers
// of segment 0 -- results by value and by reference as they stand, the triangle record asked inside the job's own `if (isHit)`:
// one helper returning a struct, or ids handed back through references, moved instructions in every kernel (DESIGN.md
// section 5x).
#pragma once

#include "query.hip.h"
#include "shading.hip.h"

namespace crt {
namespace {

template <class Derived, class Params, bool CNT>
struct LitJob {
    static constexpr int kClosest = -1; // `light` while a closest-hit ray (the record's own, or a later segment's) is walked
    static constexpr int kIdle = -2;    // no record, or a finished one

    const Params& q;
    Stack stack;
    Ray r;    // closest phase: segment 0 the prescaled record, later the job's ray; any-hit phase: that ray (r.o = the biased hit point)
    int cur;
    int light = kIdle;  // >= 0: the light whose shadow ray is being walked
    uint32_t idx = 0;   // the record (PathJob: the work item and the bounce count)
    float tlim = 0.0f;  // closest phase: tmin (segment 0: the record's, prescaled; later 0); any-hit phase: tmax = the light's distance
    // (tmax of a closest phase: the record's again at its end, kTMax later; the cull bound follows from the best hit or from
    // the distance)
    // One set of registers for the two phases, which never need both: in the closest phase the best hit {t', u, v, tri, gid}
    // (w[0..4]), in the any-hit phases the normal, the albedo and the light gathered so far (w[0..2], [3..5], [6..8]).  As
    // members of their own the nine floats of the any-hit phases stay allocated through the closest-hit loop (another lane of
    // the wavefront may be in an any-hit phase) and the kernels do not fit 5 wavefronts per SIMD without spilling.
    float w[9];
    __device__ __forceinline__ Hit hit() const { return Hit{ w[0], w[1], w[2], __float_as_uint(w[3]), __float_as_uint(w[4]) }; }
    __device__ __forceinline__ void setHit(const Hit& h) { w[0] = h.t; w[1] = h.u; w[2] = h.v; w[3] = __uint_as_float(h.tri); w[4] = __uint_as_float(h.gid); }
    __device__ __forceinline__ F3 vec(int k) const { return f3(w[3 * k], w[3 * k + 1], w[3 * k + 2]); }
    __device__ __forceinline__ void setVec(int k, F3 v) { w[3 * k] = v.x; w[3 * k + 1] = v.y; w[3 * k + 2] = v.z; }
    static constexpr int kN = 0, kAlbedo = 1, kRgb = 2;
    uint32_t extra = 0; // a word for the job's own phases (AmbientJob: its sample number and count); unused, it costs nothing
    uint32_t iters = 0;
    uint32_t cntShadow = 0;

    __device__ __forceinline__ Derived& self() { return static_cast<Derived&>(*this); }

    __device__ __forceinline__ explicit LitJob(const Params& params) : q(params)
    {
        r = makeRay(f3(0.0f, 0.0f, 0.0f), f3(0.0f, 0.0f, 1.0f));
        for (float& x : w) x = 0.0f;
    }
    // (counting) the wavefront's shadow rays to counters[2] and, for a job that counts a second kind of ray, those to
    // counters[3]: runQuery adds the fetch counts itself and knows nothing of these.  For the job's destructor, which runs when
    // runQuery's loop has ended, every lane active
    template <bool OTHER = false>
    __device__ __forceinline__ void addCounts(uint32_t cntOther = 0u)
    {
        if (CNT) {
            const uint32_t s = waveTotal(cntShadow), b = OTHER ? waveTotal(cntOther) : 0u;
            if ((threadIdx.x & 63u) == 0u) {
                atomicAdd(&q.c.counters[2], static_cast<unsigned long long>(s));
                if (OTHER) atomicAdd(&q.c.counters[3], static_cast<unsigned long long>(b));
            }
        }
    }
    // Segment 0 of record i: the prescaled ray, its tmax as the best hit, and whether it is walked at all.  (PathJob has its
    // own: a work item is not a record)
    __device__ __forceinline__ void start(uint32_t i)
    {
        const float4* rays = reinterpret_cast<const float4*>(q.c.records);
        const float4 a = rays[2u * static_cast<size_t>(i)], b = rays[2u * static_cast<size_t>(i) + 1u];
        idx = i;
        float tmax;
        queryRay(a, b, r, tlim, tmax);
        setHit(Hit{ tmax, 0.0f, 0.0f, 0u, 0u });
        light = kClosest;
        // a record with a NaN or an empty interval is not traced: step() finishes it as a miss
        cur = (queryRayOk(a, b, tlim, tmax) & (q.c.n_nodes != 0u)) ? LayLegacy::kRoot : LayLegacy::kDone;
    }
    // everything is written where it becomes known (inside step): nothing of a finished record is held for this
    __device__ __forceinline__ void retire(uint32_t) {}
    static __device__ __forceinline__ void store3(float* out, uint32_t i, F3 v)
    {
        float* o = out + 3u * static_cast<size_t>(i);
        o[0] = v.x; o[1] = v.y; o[2] = v.z;
    }
    // The end of segment 0 of record `rec` with best hit h: seg.o / seg.d become the record as the caller wrote it (read again
    // from the buffer: the prescaled direction may have lost low bits of small components) and h.t the unscaled t = t' 2^-e,
    // on a miss the record's tmax; returns whether it is a hit.  The scale exponent and the prescaled tmax again rather than
    // carried (queryRay on the same record: the same bits).  What the frame kernels hand the shading for a camera ray: a
    // record that holds one gives that pixel's bits.
    __device__ __forceinline__ bool segment0(uint32_t rec, Hit& h, Ray& seg) const
    {
        const float4* rays = reinterpret_cast<const float4*>(q.c.records);
        const float4 a = rays[2u * static_cast<size_t>(rec)], b = rays[2u * static_cast<size_t>(rec) + 1u];
        Ray scaled;
        float tminRec, tmaxRec;
        const int e = queryRay(a, b, scaled, tminRec, tmaxRec);
        const bool isHit = h.t < tmaxRec;
        seg.o = f3(a.x, a.y, a.z);
        seg.d = f3(b.x, b.y, b.z);
        h.t = isHit ? __builtin_amdgcn_ldexpf(h.t, -e) : b.w;
        return isHit;
    }
    // a hit's mesh ordinal (k = 0: v0.w) or triangle of the mesh (k = 1: e1.w), from its triangle record.  (An empty scene has
    // no triangle record to read: ask on a hit only; a miss writes 0xFFFFFFFF)
    __device__ __forceinline__ uint32_t hitId(const Hit& h, int k) const
    {
        return __float_as_uint(LayLegacy::triPtr(reinterpret_cast<const float4*>(q.c.tris), h.tri)[k].w);
    }
    // the hit outputs of record `rec`, each nullable.  out: what holds them (ShadedOutputs, or PathQueryParams itself)
    template <class Out>
    static __device__ __forceinline__ void storeHit(const Out& out, uint32_t rec, const Hit& h, uint32_t inst, uint32_t prim)
    {
        if (out.t) out.t[rec] = h.t;
        if (out.uv) reinterpret_cast<float2*>(out.uv)[rec] = make_float2(h.u, h.v);
        if (out.inst) out.inst[rec] = inst;
        if (out.prim) out.prim[rec] = prim;
    }
    // the shadow ray of the first light from `from` on that sees the surface from its front, or what follows the last light
    __device__ __forceinline__ void nextLight(uint32_t from, F3 Po)
    {
        const LightRec* lights = reinterpret_cast<const LightRec*>(q.lights);
        for (uint32_t li = from; li < q.n_lights; li++) {
            const LightTerm lt = lightTerm(lights[li], Po, vec(kN));
            if (lt.cosv > 0.0f) {
                r = makeRay(Po, lt.Ld);
                tlim = lt.dist;
                stack.sp = 0;
                cur = LayLegacy::kRoot;
                light = static_cast<int>(li);
                if (CNT) cntShadow++;
                return;
            }
        }
        self().afterLights(Po);
    }
    // a shadow ray has ended: its light's contribution, then the next light
    __device__ __forceinline__ void endShadow(bool occluded)
    {
        if (!occluded) {
            const LightRec Lt = reinterpret_cast<const LightRec*>(q.lights)[light];
            const LightTerm lt = lightTerm(Lt, r.o, vec(kN)); // (again rather than carried: the same inputs, the same bits)
            F3 view = f3(0.0f, 0.0f, 0.0f);
            if constexpr (Derived::kPhong) {
                if (q.phong_ks > 0.0f) view = self().viewVector();
            }
            F3 rgb = vec(kRgb);
            addLight<Derived::kPhong>(q, Lt, lt, vec(kN), vec(kAlbedo), view, rgb);
            setVec(kRgb, rgb);
        }
        nextLight(static_cast<uint32_t>(light) + 1u, r.o);
    }
    // Phong's view vector of a job that shades segment 0 only: minus the record's direction
    __device__ __forceinline__ F3 recordView() const
    {
        const float4 b = reinterpret_cast<const float4*>(q.c.records)[2u * static_cast<size_t>(idx) + 1u];
        return f3(-b.x, -b.y, -b.z);
    }
    // the lanes of the any-hit population, and what ends their traversal
    __device__ __forceinline__ bool anyHit() const { return light >= 0; }
    __device__ __forceinline__ void endAny(bool occluded) { endShadow(occluded); }
    template <bool COUNT>
    __device__ __forceinline__ void step(uint32_t& cntNodes, uint32_t& cntTris)
    {
        static_assert(COUNT == CNT, "a job<COUNT> runs under runQuery<COUNT>");
        const float4* nodes = reinterpret_cast<const float4*>(q.c.nodes);
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        if (light == kClosest) {
            Hit h = hit();
            float tcull = cullBound(h.t); // (closestIteration sets t * kCullPad on an accepted hit: the same value for t >= 0)
            closestIteration<COUNT, 8>(nodes, tris, r, tlim, tcull, stack, static_cast<int>(q.c.inner_min), h, cur, iters, cntNodes, cntTris);
            setHit(h);
            if (cur == LayLegacy::kDone) self().endClosest();
        } else if (self().anyHit()) { // one any-hit population, one node-step threshold
            bool occluded = false; // (set by the leaf step that also ends the traversal: nothing to carry)
            anyIteration<COUNT, 8>(nodes, tris, r, 0.0f, tlim, tlim * kCullPad, stack, static_cast<int>(q.inner_min_any), occluded, cur, iters, cntNodes, cntTris);
            if (cur == LayLegacy::kDone) self().endAny(occluded);
        }
    }
};

} // namespace
} // namespace crt
