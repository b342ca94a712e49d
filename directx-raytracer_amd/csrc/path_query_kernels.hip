// HIP kernels for gfx950 (MI355X): path-traced ray queries on caller-supplied rays (crt_path_rays*) -- the frames' mode-200
// path (path_kernels.hip; specification: oracle trace_path) from its first segment on, for records instead of pixels.
//
// One job of runQuery (query.hip.h) on the phase machine of lit_job.hip.h.  A work item is a (record, sample) pair, numbered
// sample-major inside a pass (item = sample-in-pass * records + record), so neighbouring lanes hold neighbouring records of
// the same sample and one record at thousands of samples still fills the machine.  What it adds:
//   closest hit   later bounces: the plain unit-direction ray over (0, 10000), the frames' bounce ray (goOn)
//   end of it     bounce 0 of the call's first sample writes the hit outputs.  A miss adds throughput x miss colour and ends
//                 the path; CONSTANT emits and ends it; REFLECTIVE / REFRACTIVE turn the lane into the next closest-hit
//                 traversal at once; DIFFUSE goes on to its lights (addLight<false>)
//   after the last light the gathered light joins the radiance, the cosine-weighted bounce is drawn and the lane becomes a
//   closest-hit traversal again -- where ShadeJob ends the record.  A path that ends leaves its radiance in the item's slot
//   of the scratch array; `cur` becomes kDone only then, so that runQuery refills the lane.
// pathResolveKernel then adds a pass's samples per record in sample order into float64 sums (addSample) and, after the
// call's last pass, writes the mean (sumMean).  No atomics on floating-point data.
//
// Throughput and radiance live in the item's scratch slot (two float4), as the frames keep them in q.thr / q.done: they are
// touched once per surface, never inside a traversal, and six more registers would not fit.  The
// directions at a surface (mirrorDir, refractDir, diffuseBounce) and the sample sums (addSample, sumMean) are the functions of
// shading.hip.h that the frames' streamShade and pathKernel go through.
//
// Arithmetic contract: identical, operation for operation, to oracle/crt_oracle.c (compiled with -ffp-contract=off).
#include "lit_job.hip.h"

namespace crt {
namespace {

// Register budget: 5 wavefronts per SIMD -- 93 VGPRs (96 counting), nothing spilled, no scratch.
// (A macro, as path_kernels.hip's: tools/kernel_regs.sh path_query_kernels.hip "-DCRT_PATH_QUERY_WAVES=4" shows another budget.)
#ifndef CRT_PATH_QUERY_WAVES
#define CRT_PATH_QUERY_WAVES 5
#endif
constexpr int kPathQueryWaves = CRT_PATH_QUERY_WAVES;

template <bool CNT>
struct PathJob : LitJob<PathJob<CNT>, PathQueryParams, CNT> {
    using Base = LitJob<PathJob<CNT>, PathQueryParams, CNT>;
    using Base::q; using Base::stack; using Base::r; using Base::cur; using Base::light; using Base::tlim;
    using Base::kClosest; using Base::kIdle; using Base::kN; using Base::kAlbedo; using Base::hit; using Base::setHit;
    using Base::vec; using Base::setVec; using Base::nextLight;
    // Registers are what limits this kernel, so nothing is held that can be had again.  The base's
    // record word is the work item of the pass = its scratch slot (<= 2^25 items a pass), the bounce count above it; the RNG
    // state travels in the w of the item's throughput slot: only a diffuse bounce draws
    static constexpr uint32_t kItemBits = 25u, kItemMask = (1u << kItemBits) - 1u;
    __device__ __forceinline__ uint32_t item() const { return Base::idx & kItemMask; }
    __device__ __forceinline__ uint32_t bounce() const { return Base::idx >> kItemBits; }
    static constexpr int kAux = Base::kRgb; // the direct light gathered so far
    uint32_t cntBounce = 0;

    __device__ __forceinline__ explicit PathJob(const PathQueryParams& params) : Base(params) {}
    __device__ __forceinline__ ~PathJob() { this->template addCounts<true>(cntBounce); } // the shadow and the bounce rays
    // the item's slot of a scratch array (q.rad, q.thr)
    __device__ __forceinline__ float4 load4(const void* a) const { return static_cast<const float4*>(a)[item()]; }
    __device__ __forceinline__ F3 load3(const void* a) const { const float4 v = load4(a); return f3(v.x, v.y, v.z); }
    __device__ __forceinline__ void store3(void* a, F3 v, uint32_t w4 = 0u) const { static_cast<float4*>(a)[item()] = make_float4(v.x, v.y, v.z, __uint_as_float(w4)); }
    __device__ __forceinline__ void start(uint32_t i)
    {
        const float4* rays = reinterpret_cast<const float4*>(q.c.records);
        const uint32_t sl = i / q.n_records, rec = i - sl * q.n_records;
        const float4 a = rays[2u * static_cast<size_t>(rec)], b = rays[2u * static_cast<size_t>(rec) + 1u];
        Base::idx = i; // bounce 0
        float tmax;
        queryRay(a, b, r, tlim, tmax);
        setHit(Hit{ tmax, 0.0f, 0.0f, 0u, 0u });
        light = kClosest;
        // the frames' start for pixel `id` and this sample, then the two draws a frame spends on the pixel jitter
        const uint32_t id = q.ids ? q.ids[rec] : q.id_base + rec;
        const uint32_t rng = pcgHash(id ^ pcgHash((q.sample0 + sl) + pcgHash(q.seed)));
        store3(q.rad, f3(0.0f, 0.0f, 0.0f));
        store3(q.thr, f3(1.0f, 1.0f, 1.0f), pcgHash(pcgHash(rng)));
        // a record with a NaN or an empty interval is not traced: step() finishes it as a miss
        cur = (queryRayOk(a, b, tlim, tmax) & (q.c.n_nodes != 0u)) ? LayLegacy::kRoot : LayLegacy::kDone;
    }
    __device__ __forceinline__ void finish()
    {
        light = kIdle;
        cur = LayLegacy::kDone;
    }
    // the path goes on from Po in direction nd: the frames' bounce ray
    __device__ __forceinline__ void goOn(F3 Po, F3 nd)
    {
        Base::idx += 1u << kItemBits;
        r = makeRay(Po, nd);
        tlim = 0.0f;
        setHit(Hit{ kTMax, 0.0f, 0.0f, 0u, 0u });
        stack.sp = 0;
        cur = LayLegacy::kRoot; // (a path that goes on has hit a triangle: the tree is not empty)
        light = kClosest;
        if (CNT) cntBounce++;
    }
    // DIFFUSE, every light asked: the direct light joins the radiance, then the cosine-weighted bounce
    __device__ __forceinline__ void afterLights(F3 Po)
    {
        const float4 thr = load4(q.thr);
        const F3 Lr = load3(q.rad), aux = vec(kAux), albedo = vec(kAlbedo), N = vec(kN);
        store3(q.rad, f3(fmaf(thr.x, aux.x, Lr.x), fmaf(thr.y, aux.y, Lr.y), fmaf(thr.z, aux.z, Lr.z)));
        if (bounce() != q.max_bounces) {
            uint32_t rng = __float_as_uint(thr.w);
            const float u1 = rngNext(rng), u2 = rngNext(rng);
            const F3 nd = diffuseBounce(N, u1, u2);
            store3(q.thr, f3(thr.x * albedo.x, thr.y * albedo.y, thr.z * albedo.z), rng);
            goOn(Po, nd);
        } else finish();
    }
    static constexpr bool kPhong = false; // addLight<false>: no view vector
    // a closest-hit traversal has ended (or, for an untraced record, never began)
    __device__ __forceinline__ void endClosest()
    {
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        Hit h = hit();
        bool isHit = h.t < kTMax;
        Ray seg = r; // what the shading sees: origin, direction (of seg only o and d are read) and h.t
        if (bounce() == 0u) {
            // the record as the caller wrote it and the unscaled t.  The hit outputs do not depend on the sample: the pass's
            // first one writes them (NULL in later passes)
            const uint32_t sl = item() / q.n_records, rec = item() - sl * q.n_records;
            isHit = this->segment0(rec, h, seg);
            if (sl == 0u) {
                uint32_t inst = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
                if (isHit) {
    inst = this->hitId(h, 0);
    prim = this->hitId(h, 1);
}
                Base::storeHit(q, rec, h, inst, prim);
            }
        }
        if (!isHit) { // throughput x miss colour, and the path ends
            const F3 thr = load3(q.thr), Lr = load3(q.rad);
            store3(q.rad, f3(fmaf(thr.x, q.miss[0], Lr.x), fmaf(thr.y, q.miss[1], Lr.y), fmaf(thr.z, q.miss[2], Lr.z)));
            finish();
            return;
        }
        const Surface sf = surfaceAt(q, tris, seg, h);
        F3 Po = biasPoint(sf.P, sf.N, kShadowBias);
        if (sf.mtype == 4u) { // CONSTANT: emits and ends
            const F3 thr = load3(q.thr), Lr = load3(q.rad);
            store3(q.rad, f3(fmaf(thr.x, sf.albedo.x, Lr.x), fmaf(thr.y, sf.albedo.y, Lr.y), fmaf(thr.z, sf.albedo.z, Lr.z)));
            finish();
        } else if (sf.mtype == 2u) { // REFLECTIVE
            if (bounce() != q.max_bounces) {
                const F3 nd = normalize3(mirrorDir(seg.d, sf.N));
                const float4 thr = load4(q.thr);
                store3(q.thr, f3(thr.x * sf.albedo.x, thr.y * sf.albedo.y, thr.z * sf.albedo.z), __float_as_uint(thr.w));
                goOn(Po, nd);
            } else finish();
        } else if (sf.mtype == 3u) { // REFRACTIVE (the throughput stays)
            if (bounce() != q.max_bounces) {
                const F3 d = refractDir(seg.d, sf, Po);
                goOn(Po, normalize3(d));
            } else finish();
        } else { // DIFFUSE
            setVec(kN, sf.N);
            setVec(kAlbedo, sf.albedo);
            setVec(kAux, f3(0.0f, 0.0f, 0.0f));
            nextLight(0u, Po);
        }
    }
};

template <bool COUNT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kPathQueryWaves, 8))) void pathQueryKernel(const PathQueryParams q)
{
    runQuery<COUNT, PathJob<COUNT>>(q);
}

// One thread per record: the pass's samples join the running sums in sample order (the frames' addSample); `in` NULL starts
// from zero, `out` and `rgb` NULL are not written.  Sums: 3 float64 per record.
__global__ __launch_bounds__(256) void pathResolveKernel(const float4* __restrict__ rad, uint32_t nRecords, uint32_t nSamples,
                                                         const double* in, double* out, float* rgb, uint32_t total)
{
    const size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= nRecords) return;
    D3 acc{ 0.0, 0.0, 0.0 };
    if (in) acc = D3{ in[3u * i], in[3u * i + 1u], in[3u * i + 2u] };
    for (uint32_t sl = 0; sl < nSamples; sl++) acc = addSample(acc, rad[static_cast<size_t>(sl) * nRecords + i]);
    if (out) {
        out[3u * i] = acc.x;
        out[3u * i + 1u] = acc.y;
        out[3u * i + 2u] = acc.z;
    }
    if (rgb) {
        const F3 m = sumMean(acc, total);
        rgb[3u * i] = m.x;
        rgb[3u * i + 1u] = m.y;
        rgb[3u * i + 2u] = m.z;
    }
}

} // namespace

// the kind of this file for launchQuery (render_kernels.h)
QueryKernel kKernelPath = { reinterpret_cast<const void*>(&pathQueryKernel<false>), reinterpret_cast<const void*>(&pathQueryKernel<true>), 1u };

int launchPathResolve(const void* rad, uint32_t n_records, uint32_t n_samples, const double* in, double* out, float* rgb, uint32_t total,
                      ihipStream_t* stream)
{
    if (n_records == 0u) return static_cast<int>(hipSuccess);
    const dim3 g((n_records + 255u) / 256u), block(256);
    hipLaunchKernelGGL(pathResolveKernel, g, block, 0, stream, static_cast<const float4*>(rad), n_records, n_samples, in, out, rgb, total);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
