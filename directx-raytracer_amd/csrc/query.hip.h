// Device-side skeleton of the persistent query kernels (ray_kernels.hip, point_kernels.hip, list_kernels.hip, winding_kernels.hip
// and, through the phase machine of lit_job.hip.h, shade_kernels.hip, ao_kernels.hip, whitted_kernels.hip, path_query_kernels.hip):
// every lane holds one caller record, a wavefront refills its idle lanes from a
// chunked global cursor.  The record window (RayTap), the driver loop every query kernel runs (runQuery) and the every-hit
// traversal of the hit counts and the listing.  Device code only: the sizing of the persistent grid and the launch are
// query_launch.cpp.  No frame kernel includes this.  (The refill threshold CRT_REFILL_MIN and lanesBelow are in
// traversal.hip.h: the path pipeline's streamClosest refills by the same rule.)
#pragma once

#include "traversal.hip.h"

namespace crt {
namespace {

// The box-cull bound of a ray whose current bound (tmax, then the best hit) is b.  Slab distances and the Moeller-Trumbore t
// round differently, so boxes are culled against b widened by 2^-18 of |b| (traversal.hip.h kCullPad): b * (1 + 2^-18) for
// b >= 0, as the frames do, and b * (1 - 2^-18) for b < 0, where the frames' factor would narrow the bound instead and reject
// boxes holding triangles strictly inside (tmin, tmax).  Frames never see a negative bound (tmin = 0.001).
constexpr float kCullPadNeg = 0.999996185302734375f; // 1 - 2^-18
__device__ __forceinline__ float cullBound(float b) { return b * (b >= 0.0f ? kCullPad : kCullPadNeg); }

// The ray of a query record {ox, oy, oz, tmin} {dx, dy, dz, tmax} (crt_trace_rays*, crt_occluded_rays*, crt_count_hits*: any
// direction magnitude), prescaled by a power of two as the oracle's query_setup does: (o, tmin 2^e, d 2^-e, tmax 2^e), e the
// exponent of the largest |d_i|, which lands in [1, 2) (frexp's exponent is 0 for a zero or non-finite input: e = -1 there).
// The scaling is exact, so every slab distance, pad, cull bound and Moeller-Trumbore value of the scaled ray is that of the
// record scaled by 2^-e, the hit's t is t' 2^-e, and kDirEps clamps only components below 1e-20 of the largest instead of
// every component below 1e-20.  The frames' rays have unit length and do not come through here.
__device__ __forceinline__ int queryRay(const float4 a, const float4 b, Ray& r, float& tmin, float& tmax)
{
    const int e = __builtin_amdgcn_frexp_expf(fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fabsf(b.z))) - 1;
    r = makeRay(f3(a.x, a.y, a.z), f3(__builtin_amdgcn_ldexpf(b.x, -e), __builtin_amdgcn_ldexpf(b.y, -e), __builtin_amdgcn_ldexpf(b.z, -e)));
    tmin = __builtin_amdgcn_ldexpf(a.w, e);
    tmax = __builtin_amdgcn_ldexpf(b.w, e);
    return e;
}

// a ray record is traced when it holds no NaN and its interval is not empty (a, b: the record, tmin / tmax: of queryRay)
__device__ __forceinline__ bool queryRayOk(const float4 a, const float4 b, float tmin, float tmax)
{
    return (a.x == a.x) & (a.y == a.y) & (a.z == a.z) & (b.x == b.x) & (b.y == b.y) & (b.z == b.z) & (tmin < tmax);
}

__device__ __forceinline__ uint32_t waveTotal(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// A wavefront's window [next, end) on the record buffer.  The first chunk is the wavefront's own (chunk number blockIdx.x, no
// atomic); later ones come from the cursor, which counts the chunks behind the grid's own.  Everything here is wave-uniform.
struct RayTap {
    uint32_t next, end;
    bool dry; // the cursor has passed the end of the buffer
    __device__ __forceinline__ void begin(uint32_t n, uint32_t chunk)
    {
        const uint64_t first = static_cast<uint64_t>(blockIdx.x) * chunk;
        next = static_cast<uint32_t>(first < n ? first : n);
        end = static_cast<uint32_t>(first + chunk < n ? first + chunk : n);
        dry = false;
    }
    __device__ __forceinline__ bool more() const { return (next < end) | !dry; }
    // records for the lanes of `mask` (call in wave-uniform control flow); a lane's record is valid if `valid`
    __device__ __forceinline__ uint32_t take(uint32_t* cursor, uint32_t n, uint32_t chunk, unsigned long long mask, bool& valid)
    {
        const uint32_t want = static_cast<uint32_t>(__popcll(mask)), avail = end - next;
        uint32_t nb = 0u, nbEnd = 0u;
        if ((want > avail) & !dry) {
            uint32_t k = 0u;
            if ((threadIdx.x & 63u) == 0u) k = atomicAdd(cursor, 1u);
            const uint64_t start = (static_cast<uint64_t>(gridDim.x) + __builtin_amdgcn_readfirstlane(k)) * chunk;
            if (start >= n) dry = true;
            else {
                nb = static_cast<uint32_t>(start);
                nbEnd = static_cast<uint32_t>(start + chunk < n ? start + chunk : n);
            }
        }
        const uint32_t pre = lanesBelow(mask);
        const uint32_t idx = pre < avail ? next + pre : nb + (pre - avail);
        valid = (pre < avail) | (idx < nbEnd);
        if (want > avail) {
            next = nbEnd ? min(nb + (want - avail), nbEnd) : end;
            end = nbEnd ? nbEnd : end;
        } else {
            next += want;
        }
        return idx;
    }
};

// The persistent loop of every query kernel.  A lane whose traversal has ended (job.cur == kDone) is idle; once every lane is,
// or CRT_REFILL_MIN are while the buffer still has records, the finished records are retired and the idle lanes take the next
// ones; then the wavefront runs one scheduling decision.  It ends when the buffer is exhausted and every record retired, and
// (COUNT) adds its fetch counts to q.counters[0] (nodes) and [1] (triangles).  Every record is still walked by one lane in its
// own fixed order, so results and counts do not depend on the order of the buffer, the refill timing or the wave scheduling.
//
// A job holds the per-lane state of one kind of query and says what differs between the kinds.  It is built here from the
// kernel's parameters (params.c: the QueryCommon part) -- as a local of this function, not a reference handed in by the kernel:
// handed in, the occlusion, hit-count and closest-point kernels came out 7 to 8 VGPRs larger and one wavefront per SIMD short
// (tools/kernel_regs.sh), whatever the order of the members or the spelling of the refill block.
//   stack          a Stack (or a type derived from it); set up here: LDS part `stack_entries` deep in the workgroup's dynamic
//                  shared memory, the rest in the lane's slice of the spill arena.  Emptied here before every start()
//   cur            the lane's current node or leaf reference; kDone: nothing left to do
//   retire(my)     writes the outputs of the lane's finished record `my`
//   start(idx)     loads record idx, resets the state and sets cur to kRoot -- or to kDone when the record is not to be walked
//   step<COUNT>(cntNodes, cntTris)   one scheduling decision for the whole wavefront
template <bool COUNT, class Job, class Params>
__device__ __forceinline__ void runQuery(const Params& params)
{
    const QueryCommon& q = params.c;
    Job job(params);
    extern __shared__ int s_stack[]; // stack_entries x (ints per entry) x 64 dwords
    const uint32_t lane = threadIdx.x & 63u;
    Stack& stack = job.stack;
    stack.lds = s_stack + lane;
    stack.spill = q.spill + (static_cast<size_t>(blockIdx.x) * 64u + lane) * q.spill_stride;
    stack.cap = static_cast<int>(q.stack_entries);
    stack.sp = 0;
    job.cur = LayLegacy::kDone;
    bool have = false; // this lane holds a record (being walked, or finished and not yet retired)
    uint32_t my = 0;   // its index in the buffer
    uint32_t cntNodes = 0, cntTris = 0;
    RayTap tap;
    tap.begin(q.n, q.chunk);
    const unsigned long long all = __ballot(true);
    for (;;) {
        const bool idle = job.cur == LayLegacy::kDone;
        const unsigned long long idleMask = __ballot(idle);
        if (idleMask == all || (tap.more() && static_cast<uint32_t>(__popcll(idleMask)) >= static_cast<uint32_t>(CRT_REFILL_MIN))) {
            if (idle & have) job.retire(my);
            bool valid = false;
            const uint32_t idx = tap.take(q.cursor, q.n, q.chunk, idleMask, valid);
            if (idle) {
                have = valid;
                if (valid) {
                    my = idx;
                    stack.sp = 0;
                    job.start(idx);
                }
            }
            if (__ballot(have) == 0ull && !tap.more()) break;
        }
        job.template step<COUNT>(cntNodes, cntTris);
    }
    if (COUNT) {
        const uint32_t a = waveTotal(cntNodes), c = waveTotal(cntTris);
        if (lane == 0) {
            atomicAdd(&q.counters[0], static_cast<unsigned long long>(a));
            atomicAdd(&q.counters[1], static_cast<unsigned long long>(c));
        }
    }
}

// The scheduling decision of closestIteration / anyIteration (traversal.hip.h, where the reasons and the measurements are) for
// the query kernels' own traversals: true = node steps.  innerMin > 0: while at least that many lanes stand on inner nodes
// (innerMask) or nobody waits at a leaf (leafMask); innerMin <= 0 (adaptive): while at least (live lanes * -innerMin) / 8 do.
// A macro, to stand in an `if` as the frame traversals' copy does: as a function returning bool the two tests become selects
// before they are inlined, and closestPointKernel then needs 81 VGPRs instead of 73 (5 wavefronts per SIMD instead of 6).
// (The two frame traversals keep their copy: the frame kernels' code is not to change.)
#define CRT_NODE_STEPS_NEXT(innerMask, leafMask, innerMin)                                                                      \
    ((innerMask) != 0ull &&                                                                                                    \
     ((leafMask) == 0ull || static_cast<int>(__popcll(innerMask)) >=                                                           \
                                ((innerMin) > 0 ? (innerMin) : (static_cast<int>(__popcll((innerMask) | (leafMask))) * -(innerMin) + 7) / 8)))

// One scheduling decision of the every-hit traversal (hit counts, occupancy, the listing's fill): anyIteration's node steps; a
// leaf hands every triangle the Moeller-Trumbore test accepts in (tmin, tmax) to onHit(t, triangle record) and the lane goes
// on with its stack (no early exit).  crt_list_hits* sizes a ray's segment by a count and fills it by a second traversal, and
// relies on the two accepting exactly the same triangles: both are this function, with another onHit.
template <bool COUNT, class OnHit>
__device__ __forceinline__ void everyHitIteration(const float4* __restrict__ nodes, const float4* __restrict__ tris, const Ray& r, float tmin,
                                                  float tmax, float tcull, Stack& stack, int innerMin, int& cur, uint32_t& cntNodes,
                                                  uint32_t& cntTris, OnHit onHit)
{
    constexpr int OCT = 8; // refilled lanes mix direction octants: the generic slab test, no plane table
    const float* planes = nullptr;
    const unsigned long long innerMask = __ballot(LayLegacy::inner(cur));
    const unsigned long long leafMask = __ballot(LayLegacy::leaf(cur));
    if ((innerMask | leafMask) == 0ull) return;
    if (CRT_NODE_STEPS_NEXT(innerMask, leafMask, innerMin)) {
        CRT_NODE_STEPS(anyStep)
        return;
    }
    if (LayLegacy::leaf(cur)) {
        uint32_t first, cnt;
        LayLegacy::leafRange(cur, first, cnt);
        for (uint32_t i = 0; i < cnt; i++) {
            const uint32_t id = LayLegacy::triId(first, i);
            const float4* T = LayLegacy::triPtr(tris, id);
            const float4 a = T[0], b = T[1], c = T[2];
            if (COUNT) cntTris++;
            float t, u, v;
            if (triTest<false>(r, a, b, c, tmin, t, u, v) & (t < tmax)) onHit(t, id);
        }
        cur = stack.sp == 0 ? LayLegacy::kDone : stack.pop();
    }
}

} // namespace
} // namespace crt
