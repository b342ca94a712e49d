// HIP kernel for gfx950 (MI355X): ambient occlusion on caller-supplied rays -- crt_shade_rays* and the frames in mode 120
// (include/crt_hip.h CRT_MODE_AMBIENT): the cosine-weighted share of the hemisphere that the hit point sees within a radius,
// as a grey value or as a sky of the miss colour on top of mode 100's point lights.
//
// One job of runQuery (query.hip.h) on the phase machine of lit_job.hip.h, with one more phase:
//   end of the closest hit   the hit outputs (t, uv, inst, prim, normal, albedo) are written.  A miss gets the miss colour and ends;
//   shadow rays   (option "ao_sky" only) the base's; the sum is mode 100's rgb
//   occlusion     K = "ao_samples" any-hit traversals from the biased hit point over (0, R), one after another: sample s goes
//                 in the first bounce direction of the mode-200 path of (record, s, seed) -- PathJob's hash chain and its
//                 diffuseBounce (path_query_kernels.hip).  The number of samples that escape is counted in a register.  They
//                 are lanes of the base's any-hit population (anyHit, endAny)
//   after the last sample the colour is written and the record ends.
// Drawing a direction costs several hundred instructions (seven hashes, two double-precision sines, three square roots, the
// ray's reciprocals) and a wavefront pays that for all 64 lanes whenever one lane does it.  So a lane whose sample has ended waits
// (kWait) and the wavefront draws for all waiting lanes at once, when kStartMin of them wait or nobody else has a ray to walk
// -- runQuery's refill rule once more, one level down.  Started lane by lane, the moment each sample ended, the kernel ran at
// 0.36 to 0.39 of the speed of crt_occluded_rays on the same rays with the same fetch counts.
// The order of the two any-hit phases does not show in the result: the light sum and the count meet in one fmaf at the end.
// Lights come first because their running sum then sits where ShadeJob keeps it and simply stays through the samples.
//
// Everything lives in registers: the nine floats of the base (normal, albedo, light sum; during the closest phase the best
// hit) and its extra word, holding the sample number and the count.  No scratch slot, no atomics on results.
//
// Arithmetic contract: every function called here is the one the frames, ShadeJob and PathJob call (shading.hip.h).
#include "lit_job.hip.h"

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
struct AmbientJob : LitJob<AmbientJob<CNT>, AmbientQueryParams, CNT> {
    using Base = LitJob<AmbientJob<CNT>, AmbientQueryParams, CNT>;
    using Base::q; using Base::stack; using Base::r; using Base::cur; using Base::light; using Base::idx; using Base::tlim;
    using Base::kIdle; using Base::kN; using Base::kAlbedo; using Base::kRgb; using Base::hit; using Base::vec;
    using Base::setVec; using Base::store3; using Base::nextLight;
    static constexpr int kSample = -3;  // `light` while an occlusion sample is walked
    static constexpr int kWait = -4;    // the next occlusion sample is to be drawn: r.o holds the biased hit point, `cur` is not read
    // the base's extra word: the sample being walked (low half) and the samples that escaped so far (high half): K <= 4096
    using Base::extra;
    static constexpr uint32_t kVisibleOne = 1u << 16, kSampleMask = kVisibleOne - 1u;

    __device__ __forceinline__ explicit AmbientJob(const AmbientQueryParams& params) : Base(params) {}
    __device__ __forceinline__ ~AmbientJob() { this->addCounts(); } // the shadow and the occlusion rays
    __device__ __forceinline__ void finish(F3 colour)
    {
        if (q.out.rgb) store3(q.out.rgb, idx, colour);
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
    // occlusion sample s = extra's low half from Po: the first bounce of the mode-200 path of (idx, s, seed) at a diffuse surface
    // with this normal (PathJob::start's hash chain, the two draws of the pixel jitter skipped, then afterLights' two draws)
    __device__ __forceinline__ void startSample(F3 Po)
    {
        const uint32_t s = extra & kSampleMask;
        uint32_t st = pcgHash(pcgHash(pcgHash(idx ^ pcgHash(s + pcgHash(q.seed)))));
        const float u1 = rngNext(st), u2 = rngNext(st);
        r = makeRay(Po, diffuseBounce(vec(kN), u1, u2));
        tlim = q.radius;
        stack.sp = 0;
        cur = LayLegacy::kRoot; // (a record that gets here has hit a triangle: the tree is not empty)
        light = kSample;
        if (CNT) this->cntShadow++;
    }
    // an occlusion sample has ended: the next one, or the colour
    __device__ __forceinline__ void endSample(bool occluded)
    {
        extra += occluded ? 1u : 1u + kVisibleOne;
        if ((extra & kSampleMask) != q.samples) {
            wait(r.o);
            return;
        }
        const float v = static_cast<float>(static_cast<double>(extra >> 16) / static_cast<double>(q.samples));
        F3 colour = f3(v, v, v);
        if (q.sky) { // point lights plus a sky of the miss colour
            const F3 a = vec(kAlbedo), direct = vec(kRgb);
            colour = f3(fmaf(a.x * q.miss[0], v, direct.x), fmaf(a.y * q.miss[1], v, direct.y), fmaf(a.z * q.miss[2], v, direct.z));
        }
        finish(colour);
    }
    // after the last light: the first occlusion sample
    __device__ __forceinline__ void afterLights(F3 Po) { wait(Po); }
    static constexpr bool kPhong = true; // Phong's view vector: minus the record's direction
    __device__ __forceinline__ F3 viewVector() const { return this->recordView(); }
    // the closest-hit traversal has ended (or never began): hit outputs, surface, then the lights or the samples
    __device__ __forceinline__ void endClosest()
    {
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        Hit h = hit();
        Ray rec; // the record as the caller wrote it
        rec.idir = rec.noidn = f3(0.0f, 0.0f, 0.0f);
        uint32_t inst = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
        const bool isHit = this->segment0(idx, h, rec);
        F3 nrm = f3(0.0f, 0.0f, 0.0f), alb = f3(0.0f, 0.0f, 0.0f), Po = nrm;
        if (isHit) {
            inst = this->hitId(h, 0);
            prim = this->hitId(h, 1);
            const Surface sf = surfaceAt(q, tris, rec, h);
            nrm = sf.N;
            alb = sf.albedo;
            Po = biasPoint(sf.P, sf.N, kShadowBias);
        }
        Base::storeHit(q.out, idx, h, inst, prim);
        if (q.out.normal) store3(q.out.normal, idx, nrm);
        if (q.out.albedo) store3(q.out.albedo, idx, alb);
        if (!isHit) {
            finish(f3(q.miss[0], q.miss[1], q.miss[2]));
            return;
        }
        setVec(kN, nrm);
        setVec(kAlbedo, alb);
        setVec(kRgb, f3(0.0f, 0.0f, 0.0f));
        extra = 0u;
        if (q.sky) nextLight(0u, Po);
        else wait(Po);
    }
    // a shadow ray or an occlusion sample: one any-hit population
    __device__ __forceinline__ bool anyHit() const { return (light >= 0) | (light == kSample); }
    __device__ __forceinline__ void endAny(bool occluded)
    {
        if (light == kSample) endSample(occluded);
        else this->endShadow(occluded);
    }
    template <bool COUNT>
    __device__ __forceinline__ void step(uint32_t& cntNodes, uint32_t& cntTris)
    {
        Base::template step<COUNT>(cntNodes, cntTris);
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
