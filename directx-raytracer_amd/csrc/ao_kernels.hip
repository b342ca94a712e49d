// HIP kernel for gfx950 (MI355X): ambient occlusion on caller-supplied rays -- crt_shade_rays* and the frames in mode 120
// (include/crt_hip.h CRT_MODE_AMBIENT): the cosine-weighted share of the hemisphere that the hit point sees within a radius,
// as a grey value or as a sky of the miss colour on top of mode 100's point lights.
//
// One job of runQuery (query.hip.h), ShadeJob (shade_kernels.hip) with one more phase.  A lane's record goes through phases
// inside step():
//   closest hit   the record prescaled by 2^e (queryRay), exactly the traversal of crt_trace_rays
//   end of it     the hit outputs (t, uv, inst, prim, normal, albedo) are written.  A miss gets the miss colour and ends;
//   shadow ray    (option "ao_sky" only) for each light with a positive cosine, in light order, an any-hit traversal from the
//                 root (lightTerm, addLight<true>: the code ShadeJob adds a light with); the sum is mode 100's rgb
//   occlusion     K = "ao_samples" any-hit traversals from the biased hit point over (0, R), one after another: sample s goes
//                 in the first bounce direction of the mode-200 path of (record, s, seed) -- PathJob's hash chain and its
//                 diffuseBounce (path_query_kernels.hip).  The number of samples that escape is counted in a register
//   after the last sample the colour is written and only then `cur` becomes kDone, so that runQuery refills the lane.
// Drawing a direction costs several hundred instructions (seven hashes, two double-precision sines, three square roots, the
// ray's reciprocals) and a wavefront pays that for all 64 lanes whenever one lane does it.  So a lane whose sample has ended waits
// (kWait) and the wavefront draws for all waiting lanes at once, when kStartMin of them wait or nobody else has a ray to walk
// -- runQuery's refill rule once more, one level down.  Started lane by lane, the moment each sample ended, the kernel ran at
// 0.36 to 0.39 of the speed of crt_occluded_rays on the same rays with the same fetch counts.
// The order of the two any-hit phases does not show in the result: the light sum and the count meet in one fmaf at the end.
// Lights come first because their running sum then sits where ShadeJob keeps it and simply stays through the samples.
//
// Everything lives in registers: the nine floats of ShadeJob (normal, albedo, light sum; during the closest phase the best
// hit) and one word holding the sample number and the count.  No scratch slot, no atomics on results.
//
// Arithmetic contract: every function called here is the one the frames, ShadeJob and PathJob call (shading.hip.h).
#include "query.hip.h"
#include "shading.hip.h"

namespace crt {
namespace {

// Register budget: 5 wavefronts per SIMD, nothing spilled, no scratch.
// (A macro, as path_query_kernels.hip's: tools/kernel_regs.sh ao_kernels.hip "-DCRT_AO_WAVES=4" shows another budget.)
#ifndef CRT_AO_WAVES
#define CRT_AO_WAVES 5
#endif
constexpr int kAmbientWaves = CRT_AO_WAVES;
// waiting lanes a wavefront collects before it draws their next directions
#ifndef CRT_AO_START_MIN
#define CRT_AO_START_MIN 16
#endif
constexpr int kStartMin = CRT_AO_START_MIN;

template <bool CNT>
struct AmbientJob {
    static constexpr int kClosest = -1; // `light` while the record's own ray is walked
    static constexpr int kIdle = -2;    // no record, or a finished one
    static constexpr int kSample = -3;  // an occlusion sample is walked
    static constexpr int kWait = -4;    // the next occlusion sample is to be drawn: r.o holds the biased hit point, `cur` is not read

    const AmbientQueryParams& q;
    Stack stack;
    Ray r;    // closest phase: the prescaled record; any-hit phases: the shadow or occlusion ray (r.o = the biased hit point)
    int cur;
    int light = kIdle;  // >= 0: the light whose shadow ray is being walked
    uint32_t idx = 0;   // the record
    float tlim = 0.0f;  // closest phase: tmin (the record's, prescaled); any-hit phases: tmax = the light's distance, or R
    // One set of registers for the phases, as ShadeJob's: closest phase the best hit {t', u, v, tri, gid} (w[0..4]), any-hit
    // phases the normal, the albedo and the light gathered (w[0..2], [3..5], [6..8])
    float w[9];
    __device__ __forceinline__ Hit hit() const { return Hit{ w[0], w[1], w[2], __float_as_uint(w[3]), __float_as_uint(w[4]) }; }
    __device__ __forceinline__ void setHit(const Hit& h) { w[0] = h.t; w[1] = h.u; w[2] = h.v; w[3] = __uint_as_float(h.tri); w[4] = __uint_as_float(h.gid); }
    __device__ __forceinline__ F3 vec(int k) const { return f3(w[3 * k], w[3 * k + 1], w[3 * k + 2]); }
    __device__ __forceinline__ void setVec(int k, F3 v) { w[3 * k] = v.x; w[3 * k + 1] = v.y; w[3 * k + 2] = v.z; }
    static constexpr int kN = 0, kAlbedo = 1, kRgb = 2;
    // the sample being walked (low half) and the samples that escaped so far (high half): K <= 4096
    uint32_t sv = 0;
    static constexpr uint32_t kVisibleOne = 1u << 16, kSampleMask = kVisibleOne - 1u;
    uint32_t iters = 0;
    uint32_t cntShadow = 0;

    __device__ __forceinline__ explicit AmbientJob(const AmbientQueryParams& params) : q(params)
    {
        r = makeRay(f3(0.0f, 0.0f, 0.0f), f3(0.0f, 0.0f, 1.0f));
        for (float& x : w) x = 0.0f;
    }
    // (counting) the wavefront's shadow and occlusion rays: runQuery adds the fetch counts itself.  Runs when runQuery's loop
    // has ended, every lane active
    __device__ __forceinline__ ~AmbientJob()
    {
        if (CNT) {
            const uint32_t s = waveTotal(cntShadow);
            if ((threadIdx.x & 63u) == 0u) atomicAdd(&q.c.counters[2], static_cast<unsigned long long>(s));
        }
    }
    __device__ __forceinline__ void retire(uint32_t) {}
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
    // the lane waits for its next occlusion sample (`cur` stays off kDone: the record is not finished)
    __device__ __forceinline__ void wait(F3 Po)
    {
        r.o = Po;
        cur = LayLegacy::kRoot;
        light = kWait;
    }
    // occlusion sample s = sv's low half from Po: the first bounce of the mode-200 path of (idx, s, seed) at a diffuse surface
    // with this normal (PathJob::start's hash chain, the two draws of the pixel jitter skipped, then afterLights' two draws)
    __device__ __forceinline__ void startSample(F3 Po)
    {
        const uint32_t s = sv & kSampleMask;
        uint32_t st = pcgHash(pcgHash(pcgHash(idx ^ pcgHash(s + pcgHash(q.seed)))));
        const float u1 = rngNext(st), u2 = rngNext(st);
        r = makeRay(Po, diffuseBounce(vec(kN), u1, u2));
        tlim = q.radius;
        stack.sp = 0;
        cur = LayLegacy::kRoot; // (a record that gets here has hit a triangle: the tree is not empty)
        light = kSample;
        if (CNT) cntShadow++;
    }
    // an occlusion sample has ended: the next one, or the colour
    __device__ __forceinline__ void endSample(bool occluded)
    {
        sv += occluded ? 1u : 1u + kVisibleOne;
        if ((sv & kSampleMask) != q.samples) {
            wait(r.o);
            return;
        }
        const float v = static_cast<float>(static_cast<double>(sv >> 16) / static_cast<double>(q.samples));
        F3 colour = f3(v, v, v);
        if (q.sky) { // point lights plus a sky of the miss colour
            const F3 a = vec(kAlbedo), direct = vec(kRgb);
            colour = f3(fmaf(a.x * q.miss[0], v, direct.x), fmaf(a.y * q.miss[1], v, direct.y), fmaf(a.z * q.miss[2], v, direct.z));
        }
        finish(colour);
    }
    // the shadow ray of the first light from `from` on that sees the surface from its front, or the first occlusion sample
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
        wait(Po);
    }
    // the closest-hit traversal has ended (or never began): hit outputs, surface, then the lights or the samples
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
        uint32_t inst = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
        F3 nrm = f3(0.0f, 0.0f, 0.0f), alb = f3(0.0f, 0.0f, 0.0f), Po = nrm;
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
            const Surface sf = surfaceAt(q, tris, rec, hr);
            nrm = sf.N;
            alb = sf.albedo;
            Po = biasPoint(sf.P, sf.N, kShadowBias);
        }
        if (q.t) q.t[idx] = t;
        if (q.uv) reinterpret_cast<float2*>(q.uv)[idx] = make_float2(h.u, h.v);
        if (q.inst) q.inst[idx] = inst;
        if (q.prim) q.prim[idx] = prim;
        if (q.normal) store3(q.normal, idx, nrm);
        if (q.albedo) store3(q.albedo, idx, alb);
        if (!isHit) {
            finish(f3(q.miss[0], q.miss[1], q.miss[2]));
            return;
        }
        setVec(kN, nrm);
        setVec(kAlbedo, alb);
        setVec(kRgb, f3(0.0f, 0.0f, 0.0f));
        sv = 0u;
        if (q.sky) nextLight(0u, Po);
        else wait(Po);
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
        static_assert(COUNT == CNT, "AmbientJob<COUNT> runs under runQuery<COUNT>");
        const float4* nodes = reinterpret_cast<const float4*>(q.c.nodes);
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        if (light == kClosest) {
            Hit h = hit();
            float tcull = cullBound(h.t); // (closestIteration sets t * kCullPad on an accepted hit: the same value for t >= 0)
            closestIteration<COUNT, 8>(nodes, tris, r, tlim, tcull, stack, static_cast<int>(q.c.inner_min), h, cur, iters, cntNodes, cntTris);
            setHit(h);
            if (cur == LayLegacy::kDone) endClosest();
        } else if ((light >= 0) | (light == kSample)) { // a shadow ray or an occlusion sample: one any-hit population, one node-step threshold
            bool occluded = false; // (set by the leaf step that also ends the traversal: nothing to carry)
            anyIteration<COUNT, 8>(nodes, tris, r, 0.0f, tlim, tlim * kCullPad, stack, static_cast<int>(q.inner_min_any), occluded, cur, iters, cntNodes, cntTris);
            if (cur == LayLegacy::kDone) {
                if (light == kSample) endSample(occluded);
                else endShadow(occluded);
            }
        }
        // the waiting lanes' next samples, together
        const unsigned long long waiting = __ballot(light == kWait);
        if (waiting != 0ull) {
            const unsigned long long walking = __ballot((light != kWait) & (light != kIdle));
            if ((walking == 0ull) | (static_cast<int>(__popcll(waiting)) >= kStartMin)) {
                if (light == kWait) startSample(r.o);
            }
        }
    }
};

template <bool COUNT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kAmbientWaves, 8))) void ambientQueryKernel(const AmbientQueryParams q)
{
    runQuery<COUNT, AmbientJob<COUNT>>(q);
}

} // namespace

// the kind of this file for launchQuery (render_kernels.h)
QueryKernel kKernelAmbient = { reinterpret_cast<const void*>(&ambientQueryKernel<false>), reinterpret_cast<const void*>(&ambientQueryKernel<true>), 1u };

} // namespace crt
