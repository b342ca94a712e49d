// HIP kernels for gfx950 (MI355X): point queries on caller-supplied records (crt_closest_points* / crt_count_hits* /
// crt_occupancy*, include/crt_hip.h) -- the closest surface point of a point, the number of surfaces a ray crosses, and
// whether a point lies inside the geometry.
//
// Both kernels are persistent like rayQueryKernel (ray_kernels.hip): a job each for the driver they share (runQuery,
// query.hip.h).
//
// Closest point: a best-first descent of the quantised 4-wide tree.  A node step decodes the four child boxes, takes the
// squared distance from the point to each box as a lower bound, descends into the nearest child and pushes the others
// with their bound (a second LDS word per stack entry), so that a popped entry is culled against the best distance found
// since, without a fetch.  Pruning is conservative (dcullOf): a box is skipped only when no triangle
// in it can produce a computed d2 <= the best so far, so the result is the brute-force minimum over all triangles whatever
// the tree.
//
// Hit counts and occupancy: the any-hit node step of the ray queries with a per-lane counter and no early exit; occupancy
// traces its three rays one after the other in the same lane.
//
// Arithmetic contract: operation for operation the order written in include/crt_hip.h (tests/point_reference.c restates it
// on the host, compiled with -ffp-contract=off).
#include "query.hip.h"
#include "../../include/crt_hip.h"

namespace crt {
namespace {

// ---- closest point on one triangle (include/crt_hip.h gives the order in words)

constexpr float kSliver = 0x1p-10f; // face branch: s <= 2^-10 |ab|^2 |ac|^2 (the angle at a below 1.8 degrees) also tries the edges

__device__ __forceinline__ float clamp01(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; } // NaN -> 0, -0 -> +0

// squared distance from p to a + u ab + v ac, from ap = p - a: r = ap - u ab - v ac by two fma per component
__device__ __forceinline__ float dist2At(F3 ap, F3 ab, F3 ac, float u, float v)
{
    const F3 r = f3(fmaf(-v, ac.x, fmaf(-u, ab.x, ap.x)), fmaf(-v, ac.y, fmaf(-u, ab.y, ap.y)), fmaf(-v, ac.z, fmaf(-u, ab.z, ap.z)));
    return dot3(r, r);
}

// the nearest of the three edges (degenerate triangles, rounding at a region border); the first smallest candidate wins
__device__ __noinline__ float nearestEdge(F3 ap, F3 bp, F3 ab, F3 ac, float& u, float& v)
{
    const F3 bc = sub3(ac, ab);
    const float eab = dot3(ab, ab), eac = dot3(ac, ac), ebc = dot3(bc, bc);
    const float tab = eab > 0.0f ? clamp01(dot3(ap, ab) / eab) : 0.0f;
    const float tac = eac > 0.0f ? clamp01(dot3(ap, ac) / eac) : 0.0f;
    const float tbc = ebc > 0.0f ? clamp01(dot3(bp, bc) / ebc) : 0.0f;
    u = tab; v = 0.0f;
    float d2 = dist2At(ap, ab, ac, u, v);
    const float dac = dist2At(ap, ab, ac, 0.0f, tac);
    if (dac < d2) { u = 0.0f; v = tac; d2 = dac; }
    const float ubc = 1.0f - tbc;
    const float dbc = dist2At(ap, ab, ac, ubc, tbc);
    if (dbc < d2) { u = ubc; v = tbc; d2 = dbc; }
    return d2;
}

// Ericson's region method on (a, ab, ac) with ap = p - a: barycentrics (u, v) of the closest point and its squared distance
__device__ __forceinline__ float closestOnTri(F3 ap, F3 ab, F3 ac, float& u, float& v)
{
    const F3 bp = sub3(ap, ab), cp = sub3(ap, ac);
    const float d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    const float d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    const float d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e = d4 - d3, f = d5 - d6, s = (va + vb) + vc;
    if ((d1 <= 0.0f) & (d2 <= 0.0f)) { u = 0.0f; v = 0.0f; }
    else if ((d3 >= 0.0f) & (d4 <= d3)) { u = 1.0f; v = 0.0f; }
    else if ((vc <= 0.0f) & (d1 >= 0.0f) & (d3 <= 0.0f) & (d1 - d3 > 0.0f)) { u = d1 / (d1 - d3); v = 0.0f; }
    else if ((d6 >= 0.0f) & (d5 <= d6)) { u = 0.0f; v = 1.0f; }
    else if ((vb <= 0.0f) & (d2 >= 0.0f) & (d6 <= 0.0f) & (d2 - d6 > 0.0f)) { u = 0.0f; v = d2 / (d2 - d6); }
    else if ((va <= 0.0f) & (e >= 0.0f) & (f >= 0.0f) & (e + f > 0.0f)) { v = e / (e + f); u = 1.0f - v; }
    else if ((va > 0.0f) & (vb > 0.0f) & (vc > 0.0f) & (s < __builtin_inff())) {
        u = vb / s; v = vc / s;
        const float d = dist2At(ap, ab, ac, u, v);
        if (s > kSliver * (dot3(ab, ab) * dot3(ac, ac))) return d;
        // a sliver (s = |ab x ac|^2 in exact arithmetic): the face's barycentrics lose their precision, so the nearest of the
        // face point and the three edges
        float ue, ve;
        const float de = nearestEdge(ap, bp, ab, ac, ue, ve);
        if (de < d) { u = ue; v = ve; return de; }
        return d;
    }
    else return nearestEdge(ap, bp, ab, ac, u, v);
    return dist2At(ap, ab, ac, u, v);
}

// The box-cull bound of a closest-point search whose best squared distance is b: a box whose computed
// squared distance exceeds (sqrt(b) (1 + 2^-18) + pad)^2 (1 + 2^-18) holds no triangle whose computed d2 is <= b.  pad =
// 2^-18 x the diagonal of the root box.  +inf stays +inf.
constexpr float kDistPad = 1.00000381469726562f; // 1 + 2^-18
__device__ __forceinline__ float dcullOf(float b, float pad)
{
    const float r = fmaf(sqrtf(b), kDistPad, pad);
    return (r * r) * kDistPad;
}

// Per-lane stack of (reference, key) pairs on the fields of Stack: entry e of lane l at dwords 2e*64+l and (2e+1)*64+l of LDS
// for e < cap, then in the lane's slice of the spill arena.  key = the order key of the entry's box (its squared-distance bound
// with the two low bits replaced by the child slot: a float <= the bound, so comparing it with the cull bound is conservative).
struct PointStack : Stack {
    __device__ __forceinline__ void push(int ref, uint32_t key)
    {
        if (sp < cap) { lds[2 * sp * 64] = ref; lds[(2 * sp + 1) * 64] = static_cast<int>(key); }
        else { spill[2 * (sp - cap)] = ref; spill[2 * (sp - cap) + 1] = static_cast<int>(key); }
        sp++;
    }
    // the next entry whose bound is within dcull, or kDone
    __device__ __forceinline__ int popWithin(float dcull)
    {
        while (sp > 0) {
            sp--;
            int ref;
            uint32_t key;
            if (sp < cap) { ref = lds[2 * sp * 64]; key = static_cast<uint32_t>(lds[(2 * sp + 1) * 64]); }
            else { ref = spill[2 * (sp - cap)]; key = static_cast<uint32_t>(spill[2 * (sp - cap) + 1]); }
            if (__uint_as_float(key & ~3u) <= dcull) return ref;
        }
        return LayLegacy::kDone;
    }
};

// One closest-point node step: the four child boxes of node `cur`, nearest first
template <bool COUNT>
__device__ __forceinline__ void pointNodeStep(const float4* __restrict__ nodes, F3 p, float dcull, PointStack& stack, int& cur, uint32_t& cntNodes)
{
    const LayLegacy::Node nd = LayLegacy::load(nodes, cur);
    if (COUNT) cntNodes++;
    const float lox = nd.q0.x, loy = nd.q0.y, loz = nd.q0.z, sx = nd.q0.w, sy = nd.q1.x, sz = nd.q1.y;
    const uint32_t lx = __float_as_uint(nd.q1.z), hx = __float_as_uint(nd.q1.w), ly = __float_as_uint(nd.q2.x), hy = __float_as_uint(nd.q2.y),
                   lz = __float_as_uint(nd.q2.z), hz = __float_as_uint(nd.q2.w);
    const int4 refs = nd.refs;
    uint32_t key[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        // the child box as the contract decodes it (fma(q, s, lo): it contains the child's triangles), and the point's
        // per-axis gap to it
        const float gx = fmaxf(fmaxf(fmaf(ubyteToFloat(lx, k), sx, lox) - p.x, p.x - fmaf(ubyteToFloat(hx, k), sx, lox)), 0.0f);
        const float gy = fmaxf(fmaxf(fmaf(ubyteToFloat(ly, k), sy, loy) - p.y, p.y - fmaf(ubyteToFloat(hy, k), sy, loy)), 0.0f);
        const float gz = fmaxf(fmaxf(fmaf(ubyteToFloat(lz, k), sz, loz) - p.z, p.z - fmaf(ubyteToFloat(hz, k), sz, loz)), 0.0f);
        const float b = dot3(f3(gx, gy, gz), f3(gx, gy, gz));
        const int ref = k == 0 ? refs.x : (k == 1 ? refs.y : (k == 2 ? refs.z : refs.w));
        key[k] = ((ref != CRT_BVH_EMPTY) & (b <= dcull)) ? ((__float_as_uint(b) & ~3u) | static_cast<uint32_t>(k)) : 0xFFFFFFFFu;
    }
#define CRT_CSWAP(a, b) { const uint32_t lo = min(key[a], key[b]), hi = max(key[a], key[b]); key[a] = lo; key[b] = hi; }
    CRT_CSWAP(0, 1) CRT_CSWAP(2, 3) CRT_CSWAP(0, 2) CRT_CSWAP(1, 3) CRT_CSWAP(1, 2)
#undef CRT_CSWAP
    if (key[0] == 0xFFFFFFFFu) {
        cur = stack.popWithin(dcull);
        return;
    }
    cur = pick4(refs, key[0] & 3u);
    if (key[3] != 0xFFFFFFFFu) stack.push(pick4(refs, key[3] & 3u), key[3]); // farthest first: the nearest pending child pops first
    if (key[2] != 0xFFFFFFFFu) stack.push(pick4(refs, key[2] & 3u), key[2]);
    if (key[1] != 0xFFFFFFFFu) stack.push(pick4(refs, key[1] & 3u), key[1]);
}

// Best triangle so far: d2, global id (~0: none), record, barycentrics
struct PointBest {
    float d2, u, v;
    uint32_t gid, tri;
};

template <bool COUNT>
__device__ __forceinline__ void pointLeafStep(const float4* __restrict__ tris, F3 p, float pad, PointBest& b, float& dcull, PointStack& stack,
                                              int& cur, uint32_t& cntTris)
{
    uint32_t first, cnt;
    LayLegacy::leafRange(cur, first, cnt);
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t id = LayLegacy::triId(first, i);
        const float4* T = LayLegacy::triPtr(tris, id);
        const float4 a = T[0], e1 = T[1], e2 = T[2];
        if (COUNT) cntTris++;
        float u, v;
        const float d2 = closestOnTri(sub3(p, f3(a.x, a.y, a.z)), f3(e1.x, e1.y, e1.z), f3(e2.x, e2.y, e2.z), u, v);
        const uint32_t gid = __float_as_uint(e2.w);
        if ((d2 < b.d2) | ((d2 == b.d2) & (gid < b.gid))) {
            b.d2 = d2; b.u = u; b.v = v; b.gid = gid; b.tri = id;
            dcull = dcullOf(d2, pad);
        }
    }
    cur = stack.popWithin(dcull);
}

// The closest-point job for runQuery (query.hip.h)
struct ClosestPointJob {
    const PointQueryParams& q;
    PointStack stack;
    int cur;
    F3 p = { 0.0f, 0.0f, 0.0f };
    float rmax = 0.0f, dcull = 0.0f;
    PointBest b = { 0.0f, 0.0f, 0.0f, 0xFFFFFFFFu, 0u };

    __device__ __forceinline__ explicit ClosestPointJob(const PointQueryParams& params) : q(params) {}
    __device__ __forceinline__ void retire(uint32_t my)
    {
        const bool hit = b.gid != 0xFFFFFFFFu;
        if (q.dist) q.dist[my] = hit ? sqrtf(b.d2) : rmax;
        if (q.uv) reinterpret_cast<float2*>(q.uv)[my] = make_float2(b.u, b.v);
        if (q.point || q.inst || q.prim) {
            F3 x = p;
            uint32_t inst = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
            if (hit) { // (an empty scene has no triangle record to read)
                const float4* T = LayLegacy::triPtr(reinterpret_cast<const float4*>(q.c.tris), b.tri);
                const float4 a = T[0], e1 = T[1], e2 = T[2];
                x = f3(fmaf(b.v, e2.x, fmaf(b.u, e1.x, a.x)), fmaf(b.v, e2.y, fmaf(b.u, e1.y, a.y)), fmaf(b.v, e2.z, fmaf(b.u, e1.z, a.z)));
                inst = __float_as_uint(a.w);  // v0.w = mesh ordinal
                prim = __float_as_uint(e1.w); // e1.w = triangle of the mesh
            }
            if (q.point) { q.point[3u * static_cast<size_t>(my)] = x.x; q.point[3u * static_cast<size_t>(my) + 1u] = x.y; q.point[3u * static_cast<size_t>(my) + 2u] = x.z; }
            if (q.inst) q.inst[my] = inst;
            if (q.prim) q.prim[my] = prim;
        }
    }
    __device__ __forceinline__ void start(uint32_t idx)
    {
        const float4 r = reinterpret_cast<const float4*>(q.c.records)[idx];
        p = f3(r.x, r.y, r.z);
        rmax = r.w;
        b.d2 = rmax * rmax; b.u = 0.0f; b.v = 0.0f; b.gid = 0xFFFFFFFFu; b.tri = 0u;
        dcull = dcullOf(b.d2, q.pad);
        // a record with a NaN or a negative rmax is not searched: it reports a miss
        const bool ok = (r.x == r.x) & (r.y == r.y) & (r.z == r.z) & (rmax >= 0.0f);
        cur = (ok & (q.c.n_nodes != 0u)) ? LayLegacy::kRoot : LayLegacy::kDone;
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
                if (LayLegacy::inner(cur)) pointNodeStep<COUNT>(reinterpret_cast<const float4*>(q.c.nodes), p, dcull, stack, cur, cntNodes);
        } else if (LayLegacy::leaf(cur)) {
            pointLeafStep<COUNT>(reinterpret_cast<const float4*>(q.c.tris), p, q.pad, b, dcull, stack, cur, cntTris);
        }
    }
};

template <bool COUNT>
__global__ __launch_bounds__(64) void closestPointKernel(const PointQueryParams q)
{
    runQuery<COUNT, ClosestPointJob>(q);
}

__device__ __forceinline__ F3 occupancyDir(uint32_t k)
{
    constexpr float d0[3] = { CRT_OCCUPANCY_DIR0 }, d1[3] = { CRT_OCCUPANCY_DIR1 }, d2[3] = { CRT_OCCUPANCY_DIR2 };
    return f3(k == 0u ? d0[0] : (k == 1u ? d1[0] : d2[0]), k == 0u ? d0[1] : (k == 1u ? d1[1] : d2[1]), k == 0u ? d0[2] : (k == 1u ? d1[2] : d2[2]));
}

// The job of the hit counts and of occupancy for runQuery: the every-hit traversal (query.hip.h) with a per-lane counter.
// OCC = false: hit count of every ray record (one uint32 each); true: occupancy of every point record (one byte each), its
// three rays traced one after the other by the same lane
template <bool OCC>
struct HitCountJob {
    const PointQueryParams& q;
    Stack stack;
    int cur;
    Ray r;
    float tmin = 0.0f, tmax = 0.0f, tcull = 0.0f;
    uint32_t hits = 0, odd = 0;
    uint32_t dir = 2; // occupancy: the direction being traced; 2 = the last one (also: no record), nothing to follow

    __device__ __forceinline__ explicit HitCountJob(const PointQueryParams& params) : q(params) { r = makeRay(f3(0.0f, 0.0f, 0.0f), f3(0.0f, 0.0f, 1.0f)); }
    __device__ __forceinline__ void retire(uint32_t my)
    {
        if (OCC) q.inside[my] = (odd + (hits & 1u)) >= 2u ? 1u : 0u;
        else q.count[my] = hits;
    }
    __device__ __forceinline__ void start(uint32_t idx)
    {
        const float4* recs = reinterpret_cast<const float4*>(q.c.records);
        hits = 0; odd = 0;
        bool ok;
        if (OCC) {
            const float4 a = recs[idx];
            r = makeRay(f3(a.x, a.y, a.z), occupancyDir(0u));
            tmin = 0.0f;
            tmax = __builtin_inff();
            tcull = cullBound(__builtin_inff());
            ok = (a.x == a.x) & (a.y == a.y) & (a.z == a.z);
        } else {
            const float4 a = recs[2u * static_cast<size_t>(idx)], b = recs[2u * static_cast<size_t>(idx) + 1u];
            queryRay(a, b, r, tmin, tmax); // prescaled, as the ray queries
            tcull = cullBound(tmax);
            ok = queryRayOk(a, b, tmin, tmax);
        }
        // a record with a NaN (or an empty interval) is not traced: no crossings
        ok = ok & (q.c.n_nodes != 0u);
        dir = ok ? 0u : 2u;
        cur = ok ? LayLegacy::kRoot : LayLegacy::kDone;
    }
    template <bool COUNT>
    __device__ __forceinline__ void step(uint32_t& cntNodes, uint32_t& cntTris)
    {
        everyHitIteration<COUNT>(reinterpret_cast<const float4*>(q.c.nodes), reinterpret_cast<const float4*>(q.c.tris), r, tmin, tmax, tcull, stack,
                                 static_cast<int>(q.c.inner_min), cur, cntNodes, cntTris, [&](float, uint32_t) { hits++; });
        if (OCC && (cur == LayLegacy::kDone) && (dir < 2u)) { // this direction is done: the next one of the same point
            odd += hits & 1u;
            hits = 0;
            dir++;
            r = makeRay(r.o, occupancyDir(dir));
            stack.sp = 0;
            cur = LayLegacy::kRoot;
        }
    }
};

template <bool COUNT, bool OCC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LayLegacy::kWavesPerEu, 8))) void hitCountKernel(const PointQueryParams q)
{
    runQuery<COUNT, HitCountJob<OCC>>(q);
}

} // namespace

// the kinds of this file for launchQuery (render_kernels.h); the closest-point stack keeps each entry's box bound beside its reference
QueryKernel kKernelClosestPoint = { reinterpret_cast<const void*>(&closestPointKernel<false>), reinterpret_cast<const void*>(&closestPointKernel<true>), 2u };
QueryKernel kKernelCount = { reinterpret_cast<const void*>(&hitCountKernel<false, false>), reinterpret_cast<const void*>(&hitCountKernel<true, false>), 1u };
QueryKernel kKernelOccupancy = { reinterpret_cast<const void*>(&hitCountKernel<false, true>), reinterpret_cast<const void*>(&hitCountKernel<true, true>), 1u };

} // namespace crt

// The query kernels are instantiated here, in the order the code object has listed them since each had a launcher of its own
// (tools/kernel_diff.sh compares listings line by line)
template __global__ void crt::closestPointKernel<true>(const crt::PointQueryParams);
template __global__ void crt::closestPointKernel<false>(const crt::PointQueryParams);
template __global__ void crt::hitCountKernel<true, false>(const crt::PointQueryParams);
template __global__ void crt::hitCountKernel<false, false>(const crt::PointQueryParams);
template __global__ void crt::hitCountKernel<true, true>(const crt::PointQueryParams);
template __global__ void crt::hitCountKernel<false, true>(const crt::PointQueryParams);
