// HIP kernels for gfx950 (MI355X): Whitted ray queries on caller-supplied rays -- crt_shade_rays* and the frames in mode 150
// (include/crt_hip.h CRT_MODE_WHITTED): mode 100 seen through mirrors and glass.  A record follows the deterministic specular
// chain of the mode-200 paths (PathJob, path_query_kernels.hip: REFLECTIVE turns by mirrorDir, REFRACTIVE by refractDir, no
// Fresnel split, no random numbers) and is shaded as ShadeJob (shade_kernels.hip) shades in mode 100 at the first surface that
// is neither: one any-hit shadow ray per light with a positive cosine, addLight<true>.
//
// One job of runQuery (query.hip.h), joined from the phases of those two.  A lane's record goes through phases inside step():
//   closest hit   segment 0: the record prescaled by 2^e (queryRay), exactly the traversal of crt_trace_rays; after a turn: the
//                 plain unit-direction ray over (0, 10000), PathJob's bounce ray (goOn)
//   end of it     segment 0 writes the hit outputs (t, uv, inst, prim, normal, albedo).  A miss gives T x miss colour and
//                 CONSTANT T x albedo, and the record ends; REFLECTIVE / REFRACTIVE turn the lane into the next closest-hit
//                 traversal at once, or end the record black after max_bounces turns; anything else goes on to its lights:
//   shadow ray    for each light with a positive cosine, in light order, an any-hit traversal from the root (lightTerm,
//                 addLight<true>: the code ShadeJob adds a light with)
//   after the last light T x the gathered light is written and only then `cur` becomes kDone, so that runQuery refills the lane.
// T is the product of the mirrors' albedos so far and k the number of turns.  With k = 0 every colour is written as it stands,
// without the product: a record that meets no mirror and no glass gives ShadeJob's mode-100 bits.
//
// T, k and Phong's view vector (minus the direction of the segment that reached the lit surface: the shadow phase holds the
// shadow ray in `r` and cannot have it again) are touched once per surface, never inside a traversal, and seven more registers
// would not fit.  They live in the record's scratch slot of two float4, as PathJob keeps an item's
// throughput and radiance.  (A slot per lane of the grid would be smaller, but its address needs the lane index, which the
// compiler computes once in front of the loop and then holds: tried, 95 VGPRs, and 4 spilled in the counting variant.)
//
// Arithmetic contract: every function called here is the one the frames, ShadeJob and PathJob call (shading.hip.h).
#include "query.hip.h"
#include "shading.hip.h"

namespace crt {
namespace {

// Register budget: 5 wavefronts per SIMD, nothing spilled, no scratch.
// (A macro, as path_query_kernels.hip's: tools/kernel_regs.sh whitted_kernels.hip "-DCRT_WHITTED_WAVES=4" shows another budget.)
#ifndef CRT_WHITTED_WAVES
#define CRT_WHITTED_WAVES 5
#endif
constexpr int kWhittedWaves = CRT_WHITTED_WAVES;

template <bool CNT>
struct WhittedJob {
    static constexpr int kClosest = -1; // `light` while a closest-hit ray (the record's own, or a turn's) is walked
    static constexpr int kIdle = -2;    // no record, or a finished one

    const WhittedQueryParams& q;
    Stack stack;
    Ray r;    // closest phase: segment 0 the prescaled record, later the turn's ray; shadow phase: the shadow ray (r.o = the biased hit point)
    int cur;
    int light = kIdle;  // >= 0: the light whose shadow ray is being walked
    // Registers are what limits this kernel, as PathJob: nothing is held that can be had again
    uint32_t idx = 0;   // the record
    float tlim = 0.0f;  // closest phase: tmin (segment 0: the record's, prescaled; later 0); shadow phase: tmax = the light's distance
    // One set of registers for the two phases, as ShadeJob's: closest phase the best hit {t, u, v, tri, gid} (w[0..4]), shadow
    // phases the normal, the albedo and the light gathered so far (w[0..2], [3..5], [6..8])
    float w[9];
    __device__ __forceinline__ Hit hit() const { return Hit{ w[0], w[1], w[2], __float_as_uint(w[3]), __float_as_uint(w[4]) }; }
    __device__ __forceinline__ void setHit(const Hit& h) { w[0] = h.t; w[1] = h.u; w[2] = h.v; w[3] = __uint_as_float(h.tri); w[4] = __uint_as_float(h.gid); }
    __device__ __forceinline__ F3 vec(int k) const { return f3(w[3 * k], w[3 * k + 1], w[3 * k + 2]); }
    __device__ __forceinline__ void setVec(int k, F3 v) { w[3 * k] = v.x; w[3 * k + 1] = v.y; w[3 * k + 2] = v.z; }
    static constexpr int kN = 0, kAlbedo = 1, kRgb = 2;
    uint32_t iters = 0;
    uint32_t cntShadow = 0, cntTurn = 0;

    __device__ __forceinline__ explicit WhittedJob(const WhittedQueryParams& params) : q(params)
    {
        r = makeRay(f3(0.0f, 0.0f, 0.0f), f3(0.0f, 0.0f, 1.0f));
        for (float& x : w) x = 0.0f;
    }
    // (counting) the wavefront's shadow and turn rays: runQuery adds the fetch counts itself.  Runs when runQuery's loop has
    // ended, every lane active
    __device__ __forceinline__ ~WhittedJob()
    {
        if (CNT) {
            const uint32_t s = waveTotal(cntShadow), b = waveTotal(cntTurn);
            if ((threadIdx.x & 63u) == 0u) {
                atomicAdd(&q.c.counters[2], static_cast<unsigned long long>(s));
                atomicAdd(&q.c.counters[3], static_cast<unsigned long long>(b));
            }
        }
    }
    __device__ __forceinline__ void retire(uint32_t) {}
    // The record's scratch slot: [0] = {T.rgb, k | kHasT}, [1] = {view.xyz, 0}.  T is stored by the first mirror and stands for
    // (1, 1, 1) until then (kHasT clear): start() writes the one word.  (Written as the constant {1, 1, 1, 0} there, the four
    // registers of that constant stayed allocated through the traversal loops and the kernel spilled.)
    static constexpr uint32_t kHasT = 0x80000000u, kTurns = 0xFFu; // (max_bounces <= 64)
    static __device__ __forceinline__ F3 throughput(const float4 Tk)
    {
        const bool has = (__float_as_uint(Tk.w) & kHasT) != 0u;
        return f3(has ? Tk.x : 1.0f, has ? Tk.y : 1.0f, has ? Tk.z : 1.0f);
    }
    __device__ __forceinline__ float4* slot() const { return static_cast<float4*>(q.state) + 2u * static_cast<size_t>(idx); }
    __device__ __forceinline__ void start(uint32_t i)
    {
        const float4* rays = reinterpret_cast<const float4*>(q.c.records);
        const float4 a = rays[2u * static_cast<size_t>(i)], b = rays[2u * static_cast<size_t>(i) + 1u];
        idx = i;
        float tmax;
        queryRay(a, b, r, tlim, tmax);
        setHit(Hit{ tmax, 0.0f, 0.0f, 0u, 0u });
        light = kClosest;
        reinterpret_cast<uint32_t*>(slot())[3] = 0u; // k = 0, T = (1, 1, 1)
        // a record with a NaN or an empty interval is not traced: step() finishes it as a miss
        cur = (queryRayOk(a, b, tlim, tmax) & (q.c.n_nodes != 0u)) ? LayLegacy::kRoot : LayLegacy::kDone;
    }
    static __device__ __forceinline__ void store3(float* out, uint32_t i, F3 v)
    {
        float* o = out + 3u * static_cast<size_t>(i);
        o[0] = v.x; o[1] = v.y; o[2] = v.z;
    }
    // the record ends with light L reaching its last surface (or the miss colour, or an emitter's albedo): L itself before the
    // first turn, T x L after it
    __device__ __forceinline__ void finish(F3 L)
    {
        const float4 Tk = slot()[0];
        if ((__float_as_uint(Tk.w) & kTurns) != 0u) {
            const F3 T = throughput(Tk);
            L = f3(fmaf(T.x, L.x, 0.0f), fmaf(T.y, L.y, 0.0f), fmaf(T.z, L.z, 0.0f));
        }
        if (q.rgb) store3(q.rgb, idx, L);
        light = kIdle;
        cur = LayLegacy::kDone;
    }
    // the record goes on from Po in direction nd: PathJob's bounce ray
    __device__ __forceinline__ void goOn(F3 Po, F3 nd)
    {
        r = makeRay(Po, nd);
        tlim = 0.0f;
        setHit(Hit{ kTMax, 0.0f, 0.0f, 0u, 0u });
        stack.sp = 0;
        cur = LayLegacy::kRoot; // (a record that goes on has hit a triangle: the tree is not empty)
        light = kClosest;
        if (CNT) cntTurn++;
    }
    // the shadow ray of the first light from `from` on that sees the surface from its front, or the end of the record
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
        finish(vec(kRgb));
    }
    // a closest-hit traversal has ended (or, for an untraced record, never began)
    __device__ __forceinline__ void endClosest()
    {
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        const bool first = (reinterpret_cast<const uint32_t*>(slot())[3] & kTurns) == 0u; // segment 0: no turn yet
        Hit h = hit();
        bool isHit = h.t < kTMax;
        Ray seg = r; // what the shading sees: origin, direction (of seg only o and d are read) and h.t
        if (first) {
            // the record as the caller wrote it and the unscaled t (ShadeJob::endClosest), and the hit outputs
            const float4* rays = reinterpret_cast<const float4*>(q.c.records);
            const float4 a = rays[2u * static_cast<size_t>(idx)], b = rays[2u * static_cast<size_t>(idx) + 1u];
            Ray scaled;
            float tminRec, tmaxRec;
            const int e = queryRay(a, b, scaled, tminRec, tmaxRec);
            isHit = h.t < tmaxRec;
            seg.o = f3(a.x, a.y, a.z);
            seg.d = f3(b.x, b.y, b.z);
            h.t = isHit ? __builtin_amdgcn_ldexpf(h.t, -e) : b.w;
            uint32_t inst = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
            if (isHit) { // (an empty scene has no triangle record to read)
                const float4* T = LayLegacy::triPtr(tris, h.tri);
                inst = __float_as_uint(T[0].w); // v0.w = mesh ordinal
                prim = __float_as_uint(T[1].w); // e1.w = triangle of the mesh
            }
            if (q.t) q.t[idx] = h.t;
            if (q.uv) reinterpret_cast<float2*>(q.uv)[idx] = make_float2(h.u, h.v);
            if (q.inst) q.inst[idx] = inst;
            if (q.prim) q.prim[idx] = prim;
            if (!isHit) {
                if (q.normal) store3(q.normal, idx, f3(0.0f, 0.0f, 0.0f));
                if (q.albedo) store3(q.albedo, idx, f3(0.0f, 0.0f, 0.0f));
            }
        }
        if (!isHit) {
            finish(f3(q.miss[0], q.miss[1], q.miss[2]));
            return;
        }
        const Surface sf = surfaceAt(q, tris, seg, h);
        const float4 Tk = slot()[0]; // (k again rather than carried through the surface evaluation)
        const uint32_t k = __float_as_uint(Tk.w) & kTurns;
        const F3 T = throughput(Tk);
        if (k == 0u) {
            if (q.normal) store3(q.normal, idx, sf.N);
            if (q.albedo) store3(q.albedo, idx, sf.albedo);
        }
        F3 Po = biasPoint(sf.P, sf.N, kShadowBias);
        if (sf.mtype == 4u) { // CONSTANT: emits and ends.  T x albedo before the first turn too, as a path's first segment
            if (q.rgb) store3(q.rgb, idx, f3(fmaf(T.x, sf.albedo.x, 0.0f), fmaf(T.y, sf.albedo.y, 0.0f), fmaf(T.z, sf.albedo.z, 0.0f)));
            light = kIdle;
            cur = LayLegacy::kDone;
        } else if (sf.mtype == 2u || sf.mtype == 3u) {
            if (k == q.max_bounces) { // the chain is cut: black, as a path's
                if (q.rgb) store3(q.rgb, idx, f3(0.0f, 0.0f, 0.0f));
                light = kIdle;
                cur = LayLegacy::kDone;
            } else if (sf.mtype == 2u) { // REFLECTIVE
                const F3 nd = normalize3(mirrorDir(seg.d, sf.N));
                slot()[0] = make_float4(T.x * sf.albedo.x, T.y * sf.albedo.y, T.z * sf.albedo.z, __uint_as_float((k + 1u) | kHasT));
                goOn(Po, nd);
            } else { // REFRACTIVE (T stays)
                const F3 d = refractDir(seg.d, sf, Po);
                reinterpret_cast<uint32_t*>(slot())[3] = __float_as_uint(Tk.w) + 1u;
                goOn(Po, normalize3(d));
            }
        } else { // DIFFUSE, INVALID, no material: mode 100's shading here
            if (q.phong_ks > 0.0f) slot()[1] = make_float4(-seg.d.x, -seg.d.y, -seg.d.z, 0.0f); // Phong's view vector
            setVec(kN, sf.N);
            setVec(kAlbedo, sf.albedo);
            setVec(kRgb, f3(0.0f, 0.0f, 0.0f));
            nextLight(0u, Po);
        }
    }
    // a shadow ray has ended: its light's contribution, then the next light
    __device__ __forceinline__ void endShadow(bool occluded)
    {
        if (!occluded) {
            const LightRec Lt = reinterpret_cast<const LightRec*>(q.lights)[light];
            const LightTerm lt = lightTerm(Lt, r.o, vec(kN)); // (again rather than carried: the same inputs, the same bits)
            F3 view = f3(0.0f, 0.0f, 0.0f);
            if (q.phong_ks > 0.0f) {
                const float4 v = slot()[1];
                view = f3(v.x, v.y, v.z);
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
        static_assert(COUNT == CNT, "WhittedJob<COUNT> runs under runQuery<COUNT>");
        const float4* nodes = reinterpret_cast<const float4*>(q.c.nodes);
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        if (light == kClosest) {
            Hit h = hit();
            float tcull = cullBound(h.t); // (closestIteration sets t * kCullPad on an accepted hit: the same value for t >= 0)
            closestIteration<COUNT, 8>(nodes, tris, r, tlim, tcull, stack, static_cast<int>(q.c.inner_min), h, cur, iters, cntNodes, cntTris);
            setHit(h);
            if (cur == LayLegacy::kDone) endClosest();
        } else if (light >= 0) {
            bool occluded = false; // (set by the leaf step that also ends the traversal: nothing to carry)
            anyIteration<COUNT, 8>(nodes, tris, r, 0.0f, tlim, tlim * kCullPad, stack, static_cast<int>(q.inner_min_any), occluded, cur, iters, cntNodes, cntTris);
            if (cur == LayLegacy::kDone) endShadow(occluded);
        }
    }
};

template <bool COUNT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kWhittedWaves, 8))) void whittedQueryKernel(const WhittedQueryParams q)
{
    runQuery<COUNT, WhittedJob<COUNT>>(q);
}

// One thread per pixel of a mode-150 frame: the float colour the query wrote, quantised as every frame kernel quantises its own
__global__ __launch_bounds__(256) void whittedPackKernel(const float* __restrict__ rgb, uint32_t* __restrict__ rgba8, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x; // n <= 2^28
    if (i >= n) return;
    const float* c = rgb + 3u * static_cast<size_t>(i);
    rgba8[i] = unorm8(c[0]) | (unorm8(c[1]) << 8) | (unorm8(c[2]) << 16) | 0xFF000000u;
}

} // namespace

// the kind of this file for launchQuery (render_kernels.h)
QueryKernel kKernelWhitted = { reinterpret_cast<const void*>(&whittedQueryKernel<false>), reinterpret_cast<const void*>(&whittedQueryKernel<true>), 1u };

int launchWhittedPack(const float* rgb, uint32_t* rgba8, uint32_t n, ihipStream_t* stream)
{
    if (n == 0u) return static_cast<int>(hipSuccess);
    const dim3 g((n + 255u) / 256u), block(256);
    hipLaunchKernelGGL(whittedPackKernel, g, block, 0, stream, rgb, rgba8, n);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
