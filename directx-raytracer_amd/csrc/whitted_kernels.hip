// HIP kernels for gfx950 (MI355X): Whitted ray queries on caller-supplied rays -- crt_shade_rays* and the frames in mode 150
// (include/crt_hip.h CRT_MODE_WHITTED): mode 100 seen through mirrors and glass.  A record follows the deterministic specular
// chain of the mode-200 paths (PathJob, path_query_kernels.hip: REFLECTIVE turns by mirrorDir, REFRACTIVE by refractDir, no
// Fresnel split, no random numbers) and is shaded as ShadeJob (shade_kernels.hip) shades in mode 100 at the first surface that
// is neither: one any-hit shadow ray per light with a positive cosine, addLight<true>.
//
// One job of runQuery (query.hip.h) on the phase machine of lit_job.hip.h.  What it adds:
//   closest hit   after a turn: the plain unit-direction ray over (0, 10000), PathJob's bounce ray (goOn)
//   end of it     segment 0 writes the hit outputs (t, uv, inst, prim, normal, albedo).  A miss gives T x miss colour and
//                 CONSTANT T x albedo, and the record ends; REFLECTIVE / REFRACTIVE turn the lane into the next closest-hit
//                 traversal at once, or end the record black after max_bounces turns; anything else goes on to its lights
//   after the last light T x the gathered light is written and the record ends.
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
#include "lit_job.hip.h"

namespace crt {
namespace {

// Register budget: 5 wavefronts per SIMD, nothing spilled, no scratch.
// (A macro, as path_query_kernels.hip's: tools/kernel_regs.sh whitted_kernels.hip "-DCRT_WHITTED_WAVES=4" shows another budget.)
#ifndef CRT_WHITTED_WAVES
#define CRT_WHITTED_WAVES 5
#endif
constexpr int kWhittedWaves = CRT_WHITTED_WAVES;

template <bool CNT>
struct WhittedJob : LitJob<WhittedJob<CNT>, WhittedQueryParams, CNT> {
    using Base = LitJob<WhittedJob<CNT>, WhittedQueryParams, CNT>;
    using Base::q; using Base::stack; using Base::r; using Base::cur; using Base::light; using Base::idx; using Base::tlim;
    using Base::kClosest; using Base::kIdle; using Base::kN; using Base::kAlbedo; using Base::kRgb; using Base::hit;
    using Base::setHit; using Base::vec; using Base::setVec; using Base::store3; using Base::nextLight;
    // Registers are what limits this kernel, as PathJob: nothing is held that can be had again
    uint32_t cntTurn = 0;

    __device__ __forceinline__ explicit WhittedJob(const WhittedQueryParams& params) : Base(params) {}
    __device__ __forceinline__ ~WhittedJob() { this->template addCounts<true>(cntTurn); } // the shadow and the turn rays
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
        Base::start(i);
        reinterpret_cast<uint32_t*>(slot())[3] = 0u; // k = 0, T = (1, 1, 1)
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
        if (q.out.rgb) store3(q.out.rgb, idx, L);
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
    __device__ __forceinline__ void afterLights(F3) { finish(vec(kRgb)); }
    // Phong's view vector: minus the direction of the segment that reached the lit surface, from the scratch slot
    static constexpr bool kPhong = true;
    __device__ __forceinline__ F3 viewVector() const
    {
        const float4 v = slot()[1];
        return f3(v.x, v.y, v.z);
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
            isHit = this->segment0(idx, h, seg);
            uint32_t inst = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
            if (isHit) {
    inst = this->hitId(h, 0);
    prim = this->hitId(h, 1);
}
            Base::storeHit(q.out, idx, h, inst, prim); // the record as the caller wrote it, the unscaled t; the hit outputs
            if (!isHit) {
                if (q.out.normal) store3(q.out.normal, idx, f3(0.0f, 0.0f, 0.0f));
                if (q.out.albedo) store3(q.out.albedo, idx, f3(0.0f, 0.0f, 0.0f));
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
            if (q.out.normal) store3(q.out.normal, idx, sf.N);
            if (q.out.albedo) store3(q.out.albedo, idx, sf.albedo);
        }
        F3 Po = biasPoint(sf.P, sf.N, kShadowBias);
        if (sf.mtype == 4u) { // CONSTANT: emits and ends.  T x albedo before the first turn too, as a path's first segment
            if (q.out.rgb) store3(q.out.rgb, idx, f3(fmaf(T.x, sf.albedo.x, 0.0f), fmaf(T.y, sf.albedo.y, 0.0f), fmaf(T.z, sf.albedo.z, 0.0f)));
            light = kIdle;
            cur = LayLegacy::kDone;
        } else if (sf.mtype == 2u || sf.mtype == 3u) {
            if (k == q.max_bounces) { // the chain is cut: black, as a path's
                if (q.out.rgb) store3(q.out.rgb, idx, f3(0.0f, 0.0f, 0.0f));
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
};

template <bool COUNT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kWhittedWaves, 8))) void whittedQueryKernel(const WhittedQueryParams q)
{
    runQuery<COUNT, WhittedJob<COUNT>>(q);
}

// One thread per pixel of a mode-150 or mode-120 frame: the float colour the query wrote, quantised as every frame kernel quantises its own
__global__ __launch_bounds__(256) void rgbToRgba8Kernel(const float* __restrict__ rgb, uint32_t* __restrict__ rgba8, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x; // n <= 2^28
    if (i >= n) return;
    const float* c = rgb + 3u * static_cast<size_t>(i);
    rgba8[i] = unorm8(c[0]) | (unorm8(c[1]) << 8) | (unorm8(c[2]) << 16) | 0xFF000000u;
}

} // namespace

// the kind of this file for launchQuery (render_kernels.h)
QueryKernel kKernelWhitted = { reinterpret_cast<const void*>(&whittedQueryKernel<false>), reinterpret_cast<const void*>(&whittedQueryKernel<true>), 1u };

int launchRgbToRgba8(const float* rgb, uint32_t* rgba8, uint32_t n, ihipStream_t* stream)
{
    if (n == 0u) return static_cast<int>(hipSuccess);
    const dim3 g((n + 255u) / 256u), block(256);
    hipLaunchKernelGGL(rgbToRgba8Kernel, g, block, 0, stream, rgb, rgba8, n);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
