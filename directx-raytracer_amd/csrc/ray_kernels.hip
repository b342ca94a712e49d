// HIP kernel for gfx950 (MI355X): batched ray queries on caller-supplied rays (crt_trace_rays* / crt_occluded_rays*) -- the
// DXR TraceRay of any ray, which the reference only issues from its own rayGen shader (R/HLSL/ray_tracing_shaders.hlsl:21-69).
//
// A ray record is 8 floats {ox, oy, oz, tmin, dx, dy, dz, tmax} (32 B, two dwordx4 loads).  User rays are arbitrary: one may be
// a node step long, its neighbour a grazing ray hundreds of steps long, so a wavefront that traced a fixed chunk of 64 would run
// as long as its slowest ray.  Here the grid is persistent (what the chip holds at once) and every lane holds one ray: a lane
// whose traversal has ended retires its ray (writes the requested outputs) and takes the next record as soon as CRT_REFILL_MIN
// lanes are idle -- the streamClosest idea of path_kernels.hip applied to a user buffer.  That loop is runQuery (query.hip.h),
// shared with the point queries and the listing.  Records are handed out from a global
// cursor in chunks of `chunk` rays per atomic.  Every ray is still traced by one lane in its own fixed order with the per-lane
// tmin / tmax of its record, so results and fetch counts are those of the oracle's traversal of the same ray, whatever the
// order of the buffer, the refill timing or the wave scheduling.
//
// A record is traced prescaled by a power of two (queryRay, query.hip.h): results do not depend on |d|.
// Arithmetic contract: identical, operation for operation, to oracle/crt_oracle.c (compiled with -ffp-contract=off).
#include "query.hip.h"

namespace crt {
namespace {

// Register budget: the closest-hit form is given 6 wavefronts per SIMD (76 VGPRs, nothing spilled); at the frames' 7 it spilled
// 4 VGPRs inside the loop and ran 9 / 8 / 15 % slower on the camera / AO / random legs of tools/ray_query_bench.py.
constexpr int kRayWavesClosest = 6;

// The ray query's job for runQuery (query.hip.h).  OCCL = false: closest hit (t, uv, inst, prim, each optional); true: any
// hit in (tmin, tmax), one byte per ray.  Output pointers are kernel arguments, so their null tests are scalar branches.
// The generic octant loop (OCT = 8): refilled lanes mix direction octants.
template <bool OCCL>
struct RayJob {
    const RayQueryParams& q;
    Stack stack;
    Ray r;
    int cur;
    float tmin = 0.0f, tmax = 0.0f, tcull = 0.0f; // the prescaled interval (queryRay)
    float tmaxRec = 0.0f;                         // the record's own tmax: a miss reports it
    int e = 0;                                    // the record's scale exponent: a hit reports t * 2^-e
    Hit h;
    bool occluded = false;
    uint32_t iters = 0;

    __device__ __forceinline__ explicit RayJob(const RayQueryParams& params) : q(params)
    {
        r = makeRay(f3(0.0f, 0.0f, 0.0f), f3(0.0f, 0.0f, 1.0f));
        h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.tri = 0; h.gid = 0;
    }
    __device__ __forceinline__ void retire(uint32_t my)
    {
        if (OCCL) {
            q.occluded[my] = occluded ? 1u : 0u;
            return;
        }
        const bool hit = h.t < tmax;
        if (q.t) q.t[my] = hit ? __builtin_amdgcn_ldexpf(h.t, -e) : tmaxRec;
        if (q.uv) reinterpret_cast<float2*>(q.uv)[my] = make_float2(h.u, h.v);
        if (q.inst || q.prim) {
            uint32_t inst = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
            if (hit) { // (an empty scene has no triangle record to read)
                const uint32_t* T = reinterpret_cast<const uint32_t*>(LayLegacy::triPtr(reinterpret_cast<const float4*>(q.c.tris), h.tri));
                inst = T[3]; // v0.w = mesh ordinal
                prim = T[7]; // e1.w = triangle of the mesh
            }
            if (q.inst) q.inst[my] = inst;
            if (q.prim) q.prim[my] = prim;
        }
    }
    __device__ __forceinline__ void start(uint32_t idx)
    {
        const float4* rays = reinterpret_cast<const float4*>(q.c.records);
        const float4 a = rays[2u * static_cast<size_t>(idx)], b = rays[2u * static_cast<size_t>(idx) + 1u];
        e = queryRay(a, b, r, tmin, tmax);
        tmaxRec = b.w;
        h.t = tmax; h.u = 0.0f; h.v = 0.0f; h.tri = 0; h.gid = 0;
        occluded = false;
        tcull = cullBound(tmax);
        // a record with a NaN or an empty interval is not traced: it reports a miss
        cur = (queryRayOk(a, b, tmin, tmax) & (q.c.n_nodes != 0u)) ? LayLegacy::kRoot : LayLegacy::kDone;
    }
    template <bool COUNT>
    __device__ __forceinline__ void step(uint32_t& cntNodes, uint32_t& cntTris)
    {
        const float4* nodes = reinterpret_cast<const float4*>(q.c.nodes);
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        const int innerMin = static_cast<int>(q.c.inner_min);
        if (OCCL) anyIteration<COUNT, 8>(nodes, tris, r, tmin, tmax, tcull, stack, innerMin, occluded, cur, iters, cntNodes, cntTris);
        else {
            closestIteration<COUNT, 8>(nodes, tris, r, tmin, tcull, stack, innerMin, h, cur, iters, cntNodes, cntTris);
            tcull = cullBound(h.t); // (closestIteration sets t * kCullPad on an accepted hit: the same value for t >= 0)
        }
    }
};

template <bool COUNT, bool OCCL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(OCCL ? LayLegacy::kWavesPerEu : kRayWavesClosest, 8))) void rayQueryKernel(const RayQueryParams q)
{
    runQuery<COUNT, RayJob<OCCL>>(q);
}

// Exhaustive check of rcpExact (traversal.hip.h) against the compiled correctly rounded 1.0f / d: wavefront w takes the
// 64 * kRcpPerThread consecutive bit patterns from w * 64 * kRcpPerThread, 64 neighbouring patterns (one per lane) per
// round.  out: [0] rcpExact mismatches, [1] inputs checked, [2..5] mismatches of the unguarded rcpNewton form among
// the inputs with biased exponent 0 / 253..255 / 1..252 and an all-ones significand (the class Markstein's theorem leaves
// out) / all others -- rcpFastOk accepts the last two, [6] smallest mismatching input of rcpExact (or ~0).  NaN results
// match any NaN.
constexpr uint32_t kRcpPerThread = 256;
__device__ __forceinline__ bool sameRcp(float a, float b) { return (__float_as_uint(a) == __float_as_uint(b)) | ((a != a) & (b != b)); }

__global__ void __launch_bounds__(256) rcpCheckKernel(unsigned long long* out)
{
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    uint32_t bad = 0, badClass[4] = { 0, 0, 0, 0 }, first = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < kRcpPerThread; k++) {
        const uint32_t bits = (wave * kRcpPerThread + k) * 64u + lane;
        const float d = __uint_as_float(bits);
        const float ref = 1.0f / d;
        if (!sameRcp(rcpExact(d), ref)) { bad++; first = min(first, bits); }
        const uint32_t e = (bits >> 23) & 0xFFu;
        const int cls = e == 0u ? 0 : (e >= 253u ? 1 : ((bits & 0x7FFFFFu) == 0x7FFFFFu ? 2 : 3));
        if (!sameRcp(rcpNewton(d), ref)) badClass[cls]++;
    }
    if (bad) { atomicAdd(&out[0], static_cast<unsigned long long>(bad)); atomicMin(&out[6], static_cast<unsigned long long>(first)); }
    for (int c = 0; c < 4; c++)
        if (badClass[c]) atomicAdd(&out[2 + c], static_cast<unsigned long long>(badClass[c]));
    atomicAdd(&out[1], static_cast<unsigned long long>(kRcpPerThread));
}

} // namespace

// the kinds of this file for launchQuery (render_kernels.h)
QueryKernel kKernelClosestHit = { reinterpret_cast<const void*>(&rayQueryKernel<false, false>), reinterpret_cast<const void*>(&rayQueryKernel<true, false>), 1u };
QueryKernel kKernelOcclusion = { reinterpret_cast<const void*>(&rayQueryKernel<false, true>), reinterpret_cast<const void*>(&rayQueryKernel<true, true>), 1u };

int launchRcpCheck(unsigned long long* out, ihipStream_t* stream)
{
    // 2^32 inputs: 2^24 threads of kRcpPerThread inputs each
    const uint32_t blocks = static_cast<uint32_t>((1ull << 32) / (256ull * kRcpPerThread));
    hipLaunchKernelGGL(rcpCheckKernel, dim3(blocks), dim3(256), 0, stream, out);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt

// The query kernels are instantiated here, in the order the code object has listed them since each had a launcher of its own
// (tools/kernel_diff.sh compares listings line by line)
template __global__ void crt::rayQueryKernel<false, true>(const crt::RayQueryParams);
template __global__ void crt::rayQueryKernel<false, false>(const crt::RayQueryParams);
template __global__ void crt::rayQueryKernel<true, true>(const crt::RayQueryParams);
template __global__ void crt::rayQueryKernel<true, false>(const crt::RayQueryParams);
