// HIP kernels for gfx950 (MI355X): generalised winding numbers of caller-supplied points (crt_winding_numbers*,
// include/crt_hip.h) -- the inside test that is defined for open meshes and triangle soups.
//
// The walk is a job for the persistent driver the other point queries share (runQuery, query.hip.h).  A node step reads the
// four child references of the quantised node and the node's line of the moment table, {p~, r} per child: a child farther
// from the point than beta x r contributes its dipole 0.5 N~ . (p~ - q) / |p~ - q|^3 and is not entered, the others are
// entered or pushed; the boxes are never decoded.  A leaf adds every triangle's half solid angle.  Every contribution goes
// into a per-lane 64-bit fixed-point sum, so the result does not depend on the order of the walk.
//
// The moment table is built bottom-up, one launch per depth level of the wide tree, deepest first, the kernel boundary the
// only synchronisation (as refitLevelKernel).  The levels come from a top-down pass of the same shape that writes every
// node's depth: the wide tree of a static scene has no level lists in HBM (only a dynamic scene keeps those of its binary
// tree), and this way one road serves every scene and every builder.
//
// Arithmetic contract: operation for operation the order written in include/crt_hip.h (tests/winding_reference.c restates it
// on the host, compiled with -ffp-contract=off like this file).
#include "query.hip.h"
#include "../../include/crt_hip.h"

namespace crt {
namespace {

// ---- crtAtan2 and the per-triangle term (include/crt_hip.h gives the order in words)

constexpr float kPi = 0x1.921fb6p+1f, kHalfPi = 0x1.921fb6p+0f;
constexpr double kTwoPi = 6.283185307179586;
constexpr double kFixScale = 0x1p36, kFixInv = 0x1p-36;
constexpr float kClusterMax = 4096.0f; // a dipole's contribution is clamped to +-2^12 before it is converted

__device__ __forceinline__ float crtAtan2(float y, float x)
{
    const float ay = fabsf(y), ax = fabsf(x);
    const bool swap = ay > ax;
    const float mx = swap ? ay : ax, mn = swap ? ax : ay;
    const bool ok = (y == y) & (x == x) & (mx > 0.0f) & (mx < __builtin_inff());
    const float t = mn / mx, s = t * t;
    float p = CRT_ATAN_C6;
    p = fmaf(p, s, CRT_ATAN_C5);
    p = fmaf(p, s, CRT_ATAN_C4);
    p = fmaf(p, s, CRT_ATAN_C3);
    p = fmaf(p, s, CRT_ATAN_C2);
    p = fmaf(p, s, CRT_ATAN_C1);
    p = fmaf(p, s, CRT_ATAN_C0);
    float r = fmaf(t, s * p, t);
    if (swap) r = kHalfPi - r;
    if (x < 0.0f) r = kPi - r;
    if (!ok) r = 0.0f;
    return y < 0.0f ? -r : r;
}

// the contract's expo(m): the frexp exponent of m, 0 when m is zero or not finite (a NaN is never the largest: m is none)
__device__ __forceinline__ int expo(float m)
{
    int e;
    (void)frexpf(m, &e);
    return ((m > 0.0f) & (m < __builtin_inff())) ? e : 0;
}

__device__ __forceinline__ float maxAbs(float m, float x)
{
    const float ax = fabsf(x);
    return ax > m ? ax : m;
}
__device__ __forceinline__ float maxAbs3(float m, F3 v) { return maxAbs(maxAbs(maxAbs(m, v.x), v.y), v.z); }
__device__ __forceinline__ F3 scale3(F3 v, int s) { return f3(ldexpf(v.x, s), ldexpf(v.y, s), ldexpf(v.z, s)); }

// half the signed solid angle of the record {v0, e1, e2} seen from q
__device__ __forceinline__ float halfAngle(F3 q, F3 v0, F3 e1, F3 e2)
{
    const F3 a0 = sub3(v0, q);
    const F3 b0 = f3(a0.x + e1.x, a0.y + e1.y, a0.z + e1.z), c0 = f3(a0.x + e2.x, a0.y + e2.y, a0.z + e2.z);
    // everything below is dimensionless: the triangle as seen from q, brought to unit size by an exact power of two
    const int s = -expo(maxAbs3(maxAbs3(maxAbs3(0.0f, a0), b0), c0));
    const F3 a = scale3(a0, s);
    e1 = scale3(e1, s);
    e2 = scale3(e2, s);
    const F3 b = f3(a.x + e1.x, a.y + e1.y, a.z + e1.z), c = f3(a.x + e2.x, a.y + e2.y, a.z + e2.z);
    const F3 n = f3(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
    const float det = dot3(a, n);
    const float la = sqrtf(dot3(a, a)), lb = sqrtf(dot3(b, b)), lc = sqrtf(dot3(c, c));
    const float m = (la * lb) * lc;
    const float den = ((m + dot3(a, b) * lc) + dot3(b, c) * la) + dot3(c, a) * lb;
    return m == 0.0f ? 0.0f : crtAtan2(det, den);
}

__device__ __forceinline__ long long toFixed(float h) { return __double2ll_rn(static_cast<double>(h) * kFixScale); }

// The winding-number job for runQuery (query.hip.h)
struct WindingJob {
    const WindingQueryParams& q;
    Stack stack;
    int cur;
    F3 p = { 0.0f, 0.0f, 0.0f };
    long long sum = 0;

    __device__ __forceinline__ explicit WindingJob(const WindingQueryParams& params) : q(params) {}
    __device__ __forceinline__ void retire(uint32_t my) { q.w[my] = static_cast<float>(static_cast<double>(sum) * kFixInv / kTwoPi); }
    __device__ __forceinline__ void start(uint32_t idx)
    {
        const float4 r = reinterpret_cast<const float4*>(q.c.records)[idx];
        p = f3(r.x, r.y, r.z);
        sum = 0;
        // a record with a NaN is not walked: w = 0
        const bool ok = (r.x == r.x) & (r.y == r.y) & (r.z == r.z);
        cur = (ok & (q.c.n_nodes != 0u)) ? LayLegacy::kRoot : LayLegacy::kDone;
    }
    template <bool COUNT>
    __device__ __forceinline__ void nodeStep(uint32_t& cntNodes)
    {
        const int4 refs = *reinterpret_cast<const int4*>(reinterpret_cast<const float4*>(q.c.nodes) + 4 * static_cast<size_t>(cur) + 3);
        const float4* M = reinterpret_cast<const float4*>(q.moments) + (kMomentStride / 4u) * static_cast<size_t>(cur);
        if (COUNT) cntNodes++;
        const float beta = q.beta;
        const bool approx = beta > 0.0f;
        int next = 0;
        bool have = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int ref = k == 0 ? refs.x : (k == 1 ? refs.y : (k == 2 ? refs.z : refs.w));
            if (ref == CRT_BVH_EMPTY) continue;
            const float4 c = M[k];
            const F3 d0 = sub3(f3(c.x, c.y, c.z), p);
            const int s = -expo(maxAbs3(0.0f, d0)); // the dipole in units of 2^-s, so that |d| is of order 1
            const F3 d = scale3(d0, s);
            const float d2 = dot3(d, d), br = beta * ldexpf(c.w, s);
            if (approx & (d2 > br * br)) {
                const float4 N = M[4 + k]; // only an accepted child's second line is touched
                float h = ldexpf((0.5f * dot3(f3(N.x, N.y, N.z), d)) / (d2 * sqrtf(d2)), 2 * s);
                h = h == h ? h : 0.0f;
                h = h > kClusterMax ? kClusterMax : (h < -kClusterMax ? -kClusterMax : h);
                sum += toFixed(h);
            } else if (have) {
                stack.push(ref);
            } else {
                next = ref;
                have = true;
            }
        }
        cur = have ? next : (stack.sp == 0 ? LayLegacy::kDone : stack.pop());
    }
    template <bool COUNT>
    __device__ __forceinline__ void leafStep(uint32_t& cntTris)
    {
        const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
        uint32_t first, cnt;
        LayLegacy::leafRange(cur, first, cnt);
        for (uint32_t i = 0; i < cnt; i++) {
            const float4* T = LayLegacy::triPtr(tris, LayLegacy::triId(first, i));
            const float4 a = T[0], e1 = T[1], e2 = T[2];
            if (COUNT) cntTris++;
            sum += toFixed(halfAngle(p, f3(a.x, a.y, a.z), f3(e1.x, e1.y, e1.z), f3(e2.x, e2.y, e2.z)));
        }
        cur = stack.sp == 0 ? LayLegacy::kDone : stack.pop();
    }
    // as closestIteration: node steps while enough lanes stand on inner nodes, else the leaves
    template <bool COUNT>
    __device__ __forceinline__ void step(uint32_t& cntNodes, uint32_t& cntTris)
    {
        const unsigned long long innerMask = __ballot(LayLegacy::inner(cur));
        const unsigned long long leafMask = __ballot(LayLegacy::leaf(cur));
        const int innerMin = static_cast<int>(q.c.inner_min);
        if (CRT_NODE_STEPS_NEXT(innerMask, leafMask, innerMin)) {
#pragma unroll
            for (int rep = 0; rep < NODE_STEPS; rep++)
                if (LayLegacy::inner(cur)) nodeStep<COUNT>(cntNodes);
        } else if (LayLegacy::leaf(cur)) {
            leafStep<COUNT>(cntTris);
        }
    }
};

template <bool COUNT>
__global__ __launch_bounds__(64) void windingKernel(const WindingQueryParams q)
{
    runQuery<COUNT, WindingJob>(q);
}

// ---- the moment table

constexpr uint32_t kNoDepth = 0xFFFFFFFFu;

struct MomentSum { // float64 sums over a triangle set: N~ = sum of area vectors, A = sum of areas, A p~ = sum of area x centroid
    double n[3], a, ap[3];
};

__global__ __launch_bounds__(256) void windingDepthInitKernel(uint32_t* __restrict__ depth, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) depth[i] = i == 0u ? 0u : kNoDepth;
}

// every node of depth `level` names its inner children's depth (a node has one parent: no two threads write one word)
__global__ __launch_bounds__(256) void windingDepthKernel(const crt_bvh_node4q* __restrict__ nodes, uint32_t n, uint32_t* __restrict__ depth, uint32_t level)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || depth[i] != level) return;
    for (int k = 0; k < 4; k++) {
        const int32_t ref = nodes[i].ref[k];
        if (ref > 0 && static_cast<uint32_t>(ref) < n) depth[ref] = level + 1u;
    }
}

__device__ __forceinline__ bool finite3(const float* v) { return (v[0] - v[0] == 0.0f) & (v[1] - v[1] == 0.0f) & (v[2] - v[2] == 0.0f); }

// Every node of depth `level`: the sums and the moments of its four child slots.  An inner child's sums are its node's total,
// written by the launch of the level below; a leaf's are folded over its triangles in leaf order.  Float64, no fused
// multiply-add (-ffp-contract=off), rounded to float32 once at the end.
__global__ __launch_bounds__(256) void windingMomentsKernel(const crt_bvh_node4q* __restrict__ nodes, const crt_bvh_tri* __restrict__ tris, uint32_t n,
                                                            const uint32_t* __restrict__ depth, uint32_t level, MomentSum* __restrict__ sums,
                                                            float* __restrict__ moments)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || depth[i] != level) return;
    const crt_bvh_node4q N = nodes[i];
    const uint32_t qlo[3] = { N.qlo_x, N.qlo_y, N.qlo_z }, qhi[3] = { N.qhi_x, N.qhi_y, N.qhi_z };
    MomentSum total = { { 0.0, 0.0, 0.0 }, 0.0, { 0.0, 0.0, 0.0 } };
    float* out = moments + static_cast<size_t>(kMomentStride) * i;
    for (int k = 0; k < 4; k++) {
        const int32_t ref = N.ref[k];
        MomentSum s = { { 0.0, 0.0, 0.0 }, 0.0, { 0.0, 0.0, 0.0 } };
        float pt[3] = { 0.0f, 0.0f, 0.0f }, r = 0.0f;
        if (ref != CRT_BVH_EMPTY) {
            if (ref >= 0) {
                if (static_cast<uint32_t>(ref) < n) s = sums[ref];
            } else {
                const uint32_t leaf = static_cast<uint32_t>(~ref), first = leaf >> 3, cnt = leaf & 7u;
                for (uint32_t j = 0; j < cnt; j++) {
                    const crt_bvh_tri T = tris[first + j];
                    if (!finite3(T.v0) || !finite3(T.e1) || !finite3(T.e2)) continue; // an inert triangle
                    const double e1[3] = { T.e1[0], T.e1[1], T.e1[2] }, e2[3] = { T.e2[0], T.e2[1], T.e2[2] };
                    const double nx = 0.5 * (e1[1] * e2[2] - e1[2] * e2[1]), ny = 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]),
                                 nz = 0.5 * (e1[0] * e2[1] - e1[1] * e2[0]);
                    const double area = __dsqrt_rn((nx * nx + ny * ny) + nz * nz);
                    s.n[0] += nx; s.n[1] += ny; s.n[2] += nz;
                    s.a += area;
                    for (int a = 0; a < 3; a++) s.ap[a] += area * (static_cast<double>(T.v0[a]) + (e1[a] + e2[a]) / 3.0);
                }
            }
            float lo[3], hi[3];
            const float base[3] = { N.lo[0], N.lo[1], N.lo[2] };
            float rr[3];
            for (int a = 0; a < 3; a++) {
                lo[a] = fmaf(static_cast<float>((qlo[a] >> (8 * k)) & 0xFFu), N.s[a], base[a]);
                hi[a] = fmaf(static_cast<float>((qhi[a] >> (8 * k)) & 0xFFu), N.s[a], base[a]);
                pt[a] = s.a > 0.0 ? static_cast<float>(s.ap[a] / s.a) : 0.5f * (lo[a] + hi[a]);
                const float d0 = pt[a] - lo[a], d1 = hi[a] - pt[a];
                const float q0 = d0 * d0, q1 = d1 * d1;
                rr[a] = q0 > q1 ? q0 : q1;
            }
            r = sqrtf((rr[0] + rr[1]) + rr[2]);
        }
        out[4 * k + 0] = pt[0]; out[4 * k + 1] = pt[1]; out[4 * k + 2] = pt[2]; out[4 * k + 3] = r;
        out[16 + 4 * k + 0] = static_cast<float>(s.n[0]); out[16 + 4 * k + 1] = static_cast<float>(s.n[1]);
        out[16 + 4 * k + 2] = static_cast<float>(s.n[2]); out[16 + 4 * k + 3] = 0.0f;
        for (int a = 0; a < 3; a++) { total.n[a] += s.n[a]; total.ap[a] += s.ap[a]; }
        total.a += s.a;
    }
    sums[i] = total;
}

size_t depthBytes(uint32_t n) { return (sizeof(uint32_t) * static_cast<size_t>(n) + 255u) & ~static_cast<size_t>(255u); }

} // namespace

// the kind of this file for launchQuery (render_kernels.h)
QueryKernel kKernelWinding = { reinterpret_cast<const void*>(&windingKernel<false>), reinterpret_cast<const void*>(&windingKernel<true>), 1u };

size_t windingScratchBytes(uint32_t n_nodes4) { return depthBytes(n_nodes4) + sizeof(MomentSum) * static_cast<size_t>(n_nodes4 ? n_nodes4 : 1u); }

int launchWindingMoments(const void* nodes4q, const void* tris, uint32_t n, uint32_t levels, float* moments, void* scratch, ihipStream_t* stream)
{
    if (n == 0u) return static_cast<int>(hipSuccess);
    uint32_t* depth = static_cast<uint32_t*>(scratch);
    MomentSum* sums = reinterpret_cast<MomentSum*>(static_cast<unsigned char*>(scratch) + depthBytes(n));
    const crt_bvh_node4q* nodes = static_cast<const crt_bvh_node4q*>(nodes4q);
    const dim3 grid((n + 255u) / 256u), blk(256);
    hipLaunchKernelGGL(windingDepthInitKernel, grid, blk, 0, stream, depth, n);
    for (uint32_t L = 0; L < levels; L++) hipLaunchKernelGGL(windingDepthKernel, grid, blk, 0, stream, nodes, n, depth, L);
    for (uint32_t L = levels + 1u; L-- > 0u;)
        hipLaunchKernelGGL(windingMomentsKernel, grid, blk, 0, stream, nodes, static_cast<const crt_bvh_tri*>(tris), n, depth, L, sums, moments);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt

// The query kernels are instantiated here, in the order the code object has listed them since each had a launcher of its own
// (tools/kernel_diff.sh compares listings line by line)
template __global__ void crt::windingKernel<true>(const crt::WindingQueryParams);
template __global__ void crt::windingKernel<false>(const crt::WindingQueryParams);
