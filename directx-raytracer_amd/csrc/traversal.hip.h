// Device-side traversal shared by the render kernel (render_kernels.hip) and the path-tracing pipeline (path_kernels.hip):
// vector helpers, the ray, Moeller-Trumbore, the per-lane LDS stack, the quantised wide-node step and the wave-scheduled
// closest-hit / any-hit traversals.  Everything is internal to the including translation unit (anonymous namespace).
//
// Arithmetic contract: identical, operation for operation, to oracle/crt_oracle.c (compiled with
// -ffp-contract=off; fused multiply-adds only where fmaf()/fma() is written; correctly rounded / and sqrt).
#pragma once

#include "render_kernels.h"

#include <hip/hip_runtime.h>

#include <climits>

namespace crt {
namespace {


constexpr float kTMin = 0.001f;   // hlsl:51
constexpr float kTMax = 10000.0f; // hlsl:52
constexpr float kDirEps = 1e-20f;
constexpr float kCullPad = 1.00000381469726562f; // 1 + 2^-18, see oracle trace_closest
constexpr float kSlabPad = 0x1p-21f;              // slab pads: near offsets 2^-21 |o * idir| down, far ones 2^-20 |noidn| up
constexpr float kShadowBias = 1e-3f;
constexpr float kFourPi = 12.566370614359172f;
constexpr int kBlock = 256;
constexpr uint32_t kBoostAfter = 300; // traversal-loop iterations after which a wavefront raises its issue priority
#ifndef NODE_STEPS
#define NODE_STEPS 2
#endif
#ifndef CRT_PROF
#define CRT_PROF 0
#endif
// diagnostics that change what a frame does or costs (per-workgroup timeline stamps, dropping the most expensive
// packets): only in the diagnostic builds of tools/diag_build.sh / tools/prof_build.sh, never in the product
#ifndef CRT_DIAG
#define CRT_DIAG CRT_PROF
#endif
// Register budget: the primary/shadow-ray variant is asked for 7 wavefronts per SIMD (<= 72 VGPRs; nothing spilled in the
// headline variant since the pixel position is recomputed after the traversal, render_kernels.hip).  With the 64-byte quantised nodes a node in flight is 16 registers instead of 28, and with the LDS
// stack at 16 entries (4 KB per wavefront) the CU holds those 28 wavefronts: 0.295 ms against 0.306 at 6 per SIMD;
// 8 per SIMD (64 VGPRs) spills inside the loops (0.37).  The path-tracing variant keeps the compiler's choice.
#ifndef CRT_WAVES_PER_EU
#define CRT_WAVES_PER_EU 7
#endif
#define CRT_OCCUPANCY_ATTR __attribute__((amdgpu_waves_per_eu(CRT_WAVES_PER_EU, 8)))
// The forms every traversal is built with, each settled by a measurement and no longer a build switch: records a whole
// wavefront shares come through the scalar cache (LayLegacy::loadUniform) -- in the descent from the root, in any node step
// whose lanes agree, and in leaves; closest-hit leaves take their triangles two per trip; the next node's record is requested
// before the current step's pushes (closestStep); one copy of the traversal loops per direction octant for packets whose rays
// agree on it.  The render kernel's own forms are template parameters (RENDER and NARROW of closestIteration).

// idle lanes a wavefront of a streaming traversal (streamClosest of path_kernels.hip, runQuery of query.hip.h) collects before
// it retires their rays and fetches new work for them, while there is any
#ifndef CRT_REFILL_MIN
#define CRT_REFILL_MIN 16
#endif
constexpr uint32_t kGroupMax = 16; // grid padding unit: tiles per XCD group never exceed this

// the lanes of mask m below the calling lane: its place among them when work is handed out to the lanes of m
__device__ __forceinline__ uint32_t lanesBelow(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
}

struct F3 { float x, y, z; };

__device__ __forceinline__ F3 f3(float x, float y, float z) { return F3{ x, y, z }; }
__device__ __forceinline__ F3 sub3(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float dot3(F3 a, F3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ F3 cross3(F3 a, F3 b)
{
    return f3(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)));
}
__device__ __forceinline__ F3 normalize3(F3 a)
{
    const float inv = 1.0f / sqrtf(dot3(a, a));
    return f3(a.x * inv, a.y * inv, a.z * inv);
}
__device__ __forceinline__ float frac1(float x) { return x - floorf(x); }
__device__ __forceinline__ float saturate1(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ float lerp1(float a, float b, float t) { return a + t * (b - a); }

// sin() with the operation sequence of oracle_sinf: Cody-Waite reduction by 2*pi in double, odd Taylor
// polynomial to r^23 (Horner, fma), one rounding to float.  fp64 runs at full rate on CDNA4.
__device__ __forceinline__ float sinContract(float x)
{
    const double xd = static_cast<double>(x);
    const double k = rint(xd * 0x1.45f306dc9c883p-3);
    double r = fma(-k, 0x1.921fb54442d18p+2, xd);
    r = fma(-k, 0x1.1a62633145c07p-52, r);
    const double r2 = r * r;
    double p = -0x1.761b41316381ap-75;
    p = fma(p, r2, 0x1.71b8ef6dcf572p-66);
    p = fma(p, r2, -0x1.2f49b46814157p-57);
    p = fma(p, r2, 0x1.952c77030ad4ap-49);
    p = fma(p, r2, -0x1.ae7f3e733b81fp-41);
    p = fma(p, r2, 0x1.6124613a86d09p-33);
    p = fma(p, r2, -0x1.ae64567f544e4p-26);
    p = fma(p, r2, 0x1.71de3a556c734p-19);
    p = fma(p, r2, -0x1.a01a01a01a01ap-13);
    p = fma(p, r2, 0x1.1111111111111p-7);
    p = fma(p, r2, -0x1.5555555555555p-3);
    p = p * r2;
    return static_cast<float>(fma(p, r, r));
}
__device__ __forceinline__ float hashSin(float x, float k) { return frac1(sinContract(x) * k); }

__device__ __forceinline__ uint32_t unorm8(float c) { return static_cast<uint32_t>(saturate1(c) * 255.0f + 0.5f); }

// noidn: -(o * idir) moved down by 2^-21 of its magnitude, the offset of the near slab distances of the ray.  A node step turns
// it into the near offset bn = fma(lo, idir, noidn) and the far offset fma(|noidn|, 2^-20, bn) of each axis, so the far
// distances sit about 2^-21 |o * idir| above the plain ones and the near distances as far below.  The rounding of
// fma(plane, idir, -(o * idir)) has an absolute part of about 2^-23 |o * idir| that does not shrink with t; the pads cover it,
// so that a box the ray enters is never culled however far from the origin it lies.  No register more
// than the plain offset: the far pad is an fma operand with an absolute-value modifier.
struct Ray {
    F3 o, d;
    F3 idir, noidn;
};

__device__ __forceinline__ float safeRcp(float d)
{
    const float ds = (fabsf(d) < kDirEps) ? copysignf(kDirEps, d) : d;
    return 1.0f / ds;
}

// the far offset of a slab axis from its near offset bn: 2^-20 |noidn| higher (see Ray)
__device__ __forceinline__ float farOffset(float bn, float noidn) { return fmaf(fabsf(noidn), 2.0f * kSlabPad, bn); }

__device__ __forceinline__ Ray makeRay(F3 o, F3 d)
{
    Ray r;
    r.o = o;
    r.d = d;
    r.idir = f3(safeRcp(d.x), safeRcp(d.y), safeRcp(d.z));
    const F3 noid = f3(-(o.x * r.idir.x), -(o.y * r.idir.y), -(o.z * r.idir.z));
    r.noidn = f3(noid.x - fabsf(noid.x) * kSlabPad, noid.y - fabsf(noid.y) * kSlabPad, noid.z - fabsf(noid.z) * kSlabPad);
    return r;
}

// Correctly rounded 1 / d without the IEEE division sequence (2 v_div_scale, v_rcp, 6 fma / mul, v_div_fmas, v_div_fixup):
// v_rcp_f32 (1 ulp) and one Newton step written out, fmaf(-d, y, 1) then fmaf(e, y, y).  rcpFastOk names the inputs on
// which that form is bit for bit the division: biased exponent 1..252 (no zero, denormal, inf or NaN, and |d| < 2^126, so
// that 1 / d is normal).  Decided by comparing all 2^32 inputs with the device's 1.0f / d (crt_debug_check_rcp,
// tests/test_rcp_exact.py): outside that range the Newton form differs, inside it never does -- the all-ones significands
// included.  A wavefront with any lane outside the range takes the division for all its lanes: a
// wave-uniform branch, not a per-lane select (which would run both forms).
__device__ __forceinline__ bool rcpFastOk(float d)
{
    return (__float_as_uint(d) << 1) - 0x01000000u < 0xFC000000u;
}
__device__ __forceinline__ float rcpNewton(float d)
{
    const float y = __builtin_amdgcn_rcpf(d);
    const float e = fmaf(-d, y, 1.0f);
    return fmaf(e, y, y);
}
__device__ __forceinline__ float rcpExact(float d)
{
    // the division is the cold path: laid out away from the loops (inline, the icosphere soup frame lost 1.8 %)
    if (__builtin_expect(__ballot(!rcpFastOk(d)) == 0ull, 1)) return rcpNewton(d);
    return 1.0f / d;
}

// Moeller-Trumbore, two sided; u = weight of v1, v = weight of v2.  NaN/inf from det == 0 fail the compares.
// SHORT: 1 / det by rcpExact or by the division.  Only the render kernel's closest-hit leaves (RENDER) take the short form;
// any-hit leaves, the path kernel and the ray queries keep the division (measured, DESIGN section 5: the short form gained
// nothing there -- shadow rays: 5M-triangle frame +3 %, path tracing +0.9 %).
template <bool SHORT>
__device__ __forceinline__ bool triTest(const Ray& r, const float4 a, const float4 b, const float4 c, float tmin,
                                        float& t, float& u, float& v)
{
    const F3 e1 = f3(b.x, b.y, b.z), e2 = f3(c.x, c.y, c.z);
    const F3 p = cross3(r.d, e2);
    const float det = dot3(e1, p);
    const float inv = SHORT ? rcpExact(det) : 1.0f / det; // = 1.0f / det, bit for bit
    const F3 s = sub3(r.o, f3(a.x, a.y, a.z));
    u = dot3(s, p) * inv;
    const F3 q = cross3(s, e1);
    v = dot3(r.d, q) * inv;
    t = dot3(e2, q) * inv;
    return (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f) & (t > tmin);
}

// Per-lane traversal stack.  The first `cap` entries live in LDS (entry e of lane l at dword e*64+l: conflict free); cap
// is chosen so that the 28 wavefronts per CU the register budget allows fit its 160 KB (16 entries = 4 KB per wavefront).  No ray
// of the bench scenes ever holds more than 15 entries while the trees are 24..26 deep, but the builder allows depth 32, so deeper
// entries spill to a per-lane slice of a global arena that is never touched otherwise: any tree stays correct with the small LDS
// footprint.  Every push and every pop decides per lane where its entry is.
// pop() is `lds : spill` as one load: the compiler selects between the two 64-bit addresses (nine vector instructions, most
// of them half rate) and loads through the flat path, so an entry in LDS still goes through the vector-memory address unit.
// popLds() is the same pop as two loads under a branch, the LDS one through an LDS pointer: v_add, v_cmp, v_lshl_add_u32 and
// ds_read_b32 plus four scalar instructions for the lanes in the LDS part, and the global load of the others is jumped over
// when there are none.  Same entry, same order: only the instructions differ.  The render kernel's traversals take it
// (RENDER of traceClosest / traceAny); what DESIGN section 5 measured for it and for the unchecked stack it replaced is there.
struct Stack {
    int* lds;    // s_stack + lane
    int* spill;  // arena slice of this lane: spill_stride = 3 * depth4 + 1 - cap entries (the host's bound, reached to within one entry)
    int cap;     // wave-uniform
    int sp;
#if CRT_PROF // diagnostic build (tools/prof_build.sh): where a wavefront's cycles go, never compiled into the product
    unsigned long long tNode = 0, tLeaf = 0;
    uint32_t itNode = 0, itLeaf = 0, lanesNode = 0, lanesLeaf = 0;
    // divergent (per-lane fetched) steps: how many, lanes in them, runs of consecutive lanes on the same record, distinct records
    uint32_t dvN = 0, dvNLanes = 0, dvNRuns = 0, dvNDistinct = 0, dvL = 0, dvLLanes = 0, dvLRuns = 0, dvLDistinct = 0, unN = 0, unL = 0;
    // wave-level node steps by kind [0 closest hit, 1 any hit]: scalar path (record through the scalar cache), divergent first
    // step of a scheduling decision, follow-on steps (early-fetched, per lane); lane-steps on the scalar path.  Counted once
    // per wavefront (by its first active lane), so a sum over lanes counts wavefront steps.
    uint32_t wsU[2] = { 0, 0 }, wsD[2] = { 0, 0 }, wsF[2] = { 0, 0 }, lsU[2] = { 0, 0 };
    // follow-on steps whose active lanes all stand on one node (could take the scalar path)
    uint32_t wsFA[2] = { 0, 0 };
    __device__ __forceinline__ void agreeStat(int cur, int kind)
    {
        if (__ballot(cur != __builtin_amdgcn_readfirstlane(cur)) == 0ull) stepStat(wsFA, kind);
    }
    __device__ __forceinline__ void stepStat(uint32_t* ws, int kind)
    {
        const uint32_t lane = threadIdx.x & 63u;
        if (lane == static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(lane))) ws[kind]++;
    }
    __device__ __forceinline__ void divStats(int cur, uint32_t& steps, uint32_t& lanes, uint32_t& runs, uint32_t& distinct)
    {
        const unsigned long long act = __ballot(true);
        const int prev = __shfl_up(cur, 1, 64);
        const uint32_t lane = threadIdx.x & 63u;
        const bool prevActive = lane > 0 && ((act >> (lane - 1)) & 1ull);
        runs += __popcll(__ballot(!prevActive || prev != cur));
        steps++;
        lanes += __popcll(act);
        unsigned long long rest = act;
        while (rest) {
            const int first = __ffsll(static_cast<long long>(rest)) - 1;
            const int v = __shfl(cur, first, 64);
            rest &= ~__ballot(cur == v);
            distinct++;
        }
    }
#endif
    __device__ __forceinline__ void push(int v)
    {
        if (sp < cap) lds[sp * 64] = v;
        else spill[sp - cap] = v;
        sp++;
    }
    __device__ __forceinline__ int pop()
    {
        sp--;
        return sp < cap ? lds[sp * 64] : spill[sp - cap];
    }
    __device__ __forceinline__ int popLds()
    {
        sp--;
        int v;
        if (sp < cap) v = ((const __attribute__((address_space(3))) int*)lds)[sp * 64]; // two address spaces: never merged into one flat load
        else v = spill[sp - cap];
        return v;
    }
    template <bool RENDER> __device__ __forceinline__ int popAs()
    {
        if constexpr (RENDER) return popLds();
        else return pop();
    }
};

struct Hit {
    float t, u, v;
    uint32_t tri; // triangle record: leaf-order index into the triangle array, also the shading / uv record
    uint32_t gid;
};

__device__ __forceinline__ float ubyteToFloat(uint32_t w, int k) { return static_cast<float>((w >> (8 * k)) & 0xFFu); } // v_cvt_f32_ubyteK

typedef float f4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) f4v* ConstQuadPtr; // constant address space + wave-uniform address = scalar loads
__device__ __forceinline__ float4 quadOf(const f4v a) { return make_float4(a.x, a.y, a.z, a.w); }

__device__ __forceinline__ int pick4(const int4& v, uint32_t i) // v[i], i in 0..3, without dynamic register indexing
{
    const int lo = (i & 1u) ? v.y : v.x, hi = (i & 1u) ? v.w : v.z;
    return (i & 2u) ? hi : lo;
}

// =====================================================================================================================
// Tree layout.  The layout (LayLegacy) says what a reference is, how a node record is fetched and how one node step turns
// it into the next current reference plus pushes; the wave-level scheduling, leaves and the octant dispatch use only that.
//
// LayLegacy: 4-wide, node = crt_bvh_node4q, 64 bytes = four dwordx4 loads:
//   {lo.x lo.y lo.z s.x} {s.y s.z qlo_x qhi_x} {qlo_y qhi_y qlo_z qhi_z} {ref[4]}
// separate triangle array; references are signed (>= 0 node index, < 0 leaf ~((first << 3) | count)).
//
// The child planes are 8-bit offsets from the node's own minimum corner: plane = fma(q, s, lo).  A per-lane fetch
// request costs this kernel far more than vector arithmetic does (24 / 48 extra dependent VALU per step measured +9 % /
// +21 %, one extra 4-byte touch per pushed child +29 %), so records are kept to as few requests per lane as possible and
// decoded in registers.  The decode is folded into the slab test: t(q) = fma(q, s * idir, b) with b = fma(lo, idir, noidn) in
// the near distances and b = farOffset(that, noidn) in the far ones (Ray: three more fma per step, none per child);
// monotonic in q with the sign of idir, so for a known direction octant (OCT < 8) the near plane of each axis is a fixed
// member of the (qlo, qhi) pair and the min/max pairs of the generic form (OCT = 8) disappear -- bit for bit the same values.
// An unused child slot is the leaf of no triangles with a point box (qlo = qhi = 0): the slab test rejects it, there is no
// test of the reference.  (Not an inverted box: the min/max form of the mixed-octant path would turn that into the whole
// node and visit the empty leaf every time.)
// =====================================================================================================================

// the slab tests of children 2j and 2j + 1 of a node whose planes sit in bytes 2j, 2j + 1 of the six given words
// (Round 3, measured and not kept: one v_perm_b32 per plane PAIR building two halfs 1024 + q (0x6400 | q) that v_fma_mix_f32
// multiplies directly, instead of one v_cvt_f32_ubyte per plane: 12 instructions fewer per node step and 0.311 vs 0.284 ms.
// tools/micro/valu_cost.hip has the reason: v_fma_mix_f32 and v_perm_b32 issue at half the rate of v_fma_f32 -- as do
// v_cvt_f32_ubyte, float and integer min / max, compares, selects and everything VOP3-only or SDWA: 4.2 against 2.5 cycles per
// wavefront instruction -- so a conversion folded into a mixed-precision fma costs what the pair it replaces cost.)
template <int OCT>
__device__ __forceinline__ void slabPair(uint32_t lx, uint32_t hx, uint32_t ly, uint32_t hy, uint32_t lz, uint32_t hz, int pair, const Ray& r,
                                         float ax, float ay, float az, float bxn, float byn, float bzn, float bxf, float byf, float bzf,
                                         float tmin, float tcull, float tn[2], bool hit[2])
{
    // near / far member of each (qlo, qhi) pair: fixed by the template octant, or picked per lane from the direction's sign
    // bits (mixed-octant wavefronts: bounce rays) -- six selects instead of the twelve min/max of the textbook form, and
    // the same values: t is monotonic in q with the sign of idir
    const bool sx = (OCT < 8) ? (OCT & 1) != 0 : (__float_as_uint(r.d.x) >> 31) != 0u;
    const bool sy = (OCT < 8) ? (OCT & 2) != 0 : (__float_as_uint(r.d.y) >> 31) != 0u;
    const bool sz = (OCT < 8) ? (OCT & 4) != 0 : (__float_as_uint(r.d.z) >> 31) != 0u;
    const uint32_t nxw = sx ? hx : lx, fxw = sx ? lx : hx, nyw = sy ? hy : ly, fyw = sy ? ly : hy, nzw = sz ? hz : lz, fzw = sz ? lz : hz;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int byte = 2 * pair + i;
        const float t_n = fmaxf(fmaxf(fmaf(ubyteToFloat(nxw, byte), ax, bxn), fmaf(ubyteToFloat(nyw, byte), ay, byn)), fmaxf(fmaf(ubyteToFloat(nzw, byte), az, bzn), tmin));
        const float t_f = fminf(fminf(fmaf(ubyteToFloat(fxw, byte), ax, bxf), fmaf(ubyteToFloat(fyw, byte), ay, byf)), fminf(fmaf(ubyteToFloat(fzw, byte), az, bzf), tcull));
        tn[i] = t_n;
        hit[i] = t_n <= t_f;
    }
}

struct LayLegacy {
    static constexpr int kWidth = 4;
    static constexpr int kDone = INT_MIN; // traversal finished (not a valid leaf reference)
    static constexpr int kRoot = 0;
    static constexpr int kStackPerLevel = 3;
    static constexpr int kWavesPerEu = CRT_WAVES_PER_EU;
    struct Node {
        float4 q0, q1, q2;
        int4 refs;
    };
    // A record fetched through the scalar cache together with its row of the plane table: the 24 plane bytes as floats, so
    // that each plane is one v_fma_f32 with a scalar operand instead of a v_cvt_f32_ubyte (half rate) and the fma.
    struct NodeU {
        float4 q0;  // lo.xyz, s.x
        float sy, sz;
        int4 refs;
        float p[24]; // float(q): qlo_x[4] qhi_x[4] qlo_y[4] qhi_y[4] qlo_z[4] qhi_z[4] -- bytes 24..47 of the record, in order
    };
    static __device__ __forceinline__ bool inner(int c) { return c >= 0; }
    static __device__ __forceinline__ bool leaf(int c) { return (c < 0) & (c != kDone); }
    // NARROW: the record's byte offset is computed in 32 bits and added to the wave-uniform base, so that the loads take the
    // scalar-base form (one v_lshlrev_b32 instead of a 64-bit shift and add, and the reference needs no sign-extended upper
    // half).  Valid while 64 * n_nodes <= 2^32 and 48 * n_tris <= 2^32: the host's choice, wideOffsets() of render_kernels.h.
    template <bool NARROW = false>
    static __device__ __forceinline__ Node load(const float4* __restrict__ nodes, int ref)
    {
        const float4* N;
        if constexpr (NARROW) N = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(nodes) + (static_cast<uint32_t>(ref) << 6));
        else N = nodes + 4 * static_cast<size_t>(ref);
        Node nd;
        nd.q0 = N[0]; nd.q1 = N[1]; nd.q2 = N[2];
        nd.refs = *reinterpret_cast<const int4*>(N + 3);
        return nd;
    }
    static __device__ __forceinline__ Node loadUniform(const float4* nodes, int ref)
    {
        ConstQuadPtr C = (ConstQuadPtr)(reinterpret_cast<uintptr_t>(nodes + 4 * static_cast<size_t>(ref)));
        const f4v a = C[0], b = C[1], c = C[2], g = C[3];
        Node nd;
        nd.q0 = quadOf(a); nd.q1 = quadOf(b); nd.q2 = quadOf(c);
        nd.refs = make_int4(__float_as_int(g.x), __float_as_int(g.y), __float_as_int(g.z), __float_as_int(g.w));
        return nd;
    }
    static __device__ __forceinline__ NodeU loadUniformDecoded(const float4* nodes, const float* planes, int ref)
    {
        const Node nd = loadUniform(nodes, ref);
        ConstQuadPtr P = (ConstQuadPtr)(reinterpret_cast<uintptr_t>(planes + kPlaneStride * static_cast<size_t>(ref)));
        NodeU u;
        u.q0 = nd.q0; u.sy = nd.q1.x; u.sz = nd.q1.y; u.refs = nd.refs;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const f4v v = P[k];
            u.p[4 * k + 0] = v.x; u.p[4 * k + 1] = v.y; u.p[4 * k + 2] = v.z; u.p[4 * k + 3] = v.w;
        }
        return u;
    }
    // leaf reference -> first triangle and count; triangle i of the leaf: its record and the id kept in Hit::tri
    static __device__ __forceinline__ void leafRange(int c, uint32_t& first, uint32_t& cnt)
    {
        const uint32_t code = static_cast<uint32_t>(~c);
        first = code >> 3;
        cnt = code & 7u;
    }
    static __device__ __forceinline__ uint32_t triId(uint32_t first, uint32_t i) { return first + i; }
    template <bool NARROW = false>
    static __device__ __forceinline__ const float4* triPtr(const float4* __restrict__ tris, uint32_t id)
    {
        if constexpr (NARROW) return reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tris) + id * 48u);
        else return tris + 3 * static_cast<size_t>(id);
    }
    // the second record of a leaf pair, id1 = two ? id + 1 : id.  NARROW: the first record's offset plus 48 or 0, a select and an
    // add where id1 * 48 is a full 32-bit multiply (the first offset is the loop's induction variable)
    template <bool NARROW = false>
    static __device__ __forceinline__ const float4* triPtrSecond(const float4* __restrict__ tris, uint32_t id, uint32_t id1, bool two)
    {
        if constexpr (NARROW) return reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tris) + (id * 48u + (two ? 48u : 0u)));
        else return triPtr(tris, id1);
    }

    template <int OCT>
    static __device__ __forceinline__ void slab(const Node& nd, const Ray& r, float tmin, float tcull, float tn[4], bool hit[4])
    {
        const float ax = nd.q0.w * r.idir.x, ay = nd.q1.x * r.idir.y, az = nd.q1.y * r.idir.z;
        const float bxn = fmaf(nd.q0.x, r.idir.x, r.noidn.x), byn = fmaf(nd.q0.y, r.idir.y, r.noidn.y), bzn = fmaf(nd.q0.z, r.idir.z, r.noidn.z);
        const float bxf = farOffset(bxn, r.noidn.x), byf = farOffset(byn, r.noidn.y), bzf = farOffset(bzn, r.noidn.z);
        const uint32_t lx = __float_as_uint(nd.q1.z), hx = __float_as_uint(nd.q1.w), ly = __float_as_uint(nd.q2.x), hy = __float_as_uint(nd.q2.y),
                       lz = __float_as_uint(nd.q2.z), hz = __float_as_uint(nd.q2.w);
#pragma unroll
        for (int j = 0; j < 2; j++) slabPair<OCT>(lx, hx, ly, hy, lz, hz, j, r, ax, ay, az, bxn, byn, bzn, bxf, byf, bzf, tmin, tcull, tn + 2 * j, hit + 2 * j);
    }
    // the same slab tests on a scalar record with decoded planes: the octant names the near / far plane of every axis at
    // compile time, and fmaf(float(q), a, b) is the value slabPair computes (float(q) is exact for q <= 255).  Known octants
    // only: the mixed-octant form would pick between two scalar planes per lane, two moves and a select on this ISA (one
    // scalar operand per vector instruction), which costs more than the conversion it replaces; it keeps the record (Node).
    template <int OCT>
    static __device__ __forceinline__ void slab(const NodeU& nd, const Ray& r, float tmin, float tcull, float tn[4], bool hit[4])
    {
        static_assert(OCT < 8, "decoded planes: octant-specialised steps only");
        const float ax = nd.q0.w * r.idir.x, ay = nd.sy * r.idir.y, az = nd.sz * r.idir.z;
        const float bxn = fmaf(nd.q0.x, r.idir.x, r.noidn.x), byn = fmaf(nd.q0.y, r.idir.y, r.noidn.y), bzn = fmaf(nd.q0.z, r.idir.z, r.noidn.z);
        const float bxf = farOffset(bxn, r.noidn.x), byf = farOffset(byn, r.noidn.y), bzf = farOffset(bzn, r.noidn.z);
        constexpr int nx = (OCT & 1) ? 4 : 0, ny = (OCT & 2) ? 12 : 8, nz = (OCT & 4) ? 20 : 16; // near member of each pair
        constexpr int fx = 4 - nx, fy = 20 - ny, fz = 36 - nz;                                   // far member
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float t_n = fmaxf(fmaxf(fmaf(nd.p[nx + k], ax, bxn), fmaf(nd.p[ny + k], ay, byn)), fmaxf(fmaf(nd.p[nz + k], az, bzn), tmin));
            const float t_f = fminf(fminf(fmaf(nd.p[fx + k], ax, bxf), fmaf(nd.p[fy + k], ay, byf)), fminf(fmaf(nd.p[fz + k], az, bzf), tcull));
            tn[k] = t_n;
            hit[k] = t_n <= t_f;
        }
    }

    // closest hit: visit the hit children nearest first.  Order key = (bits(t_near) & 0x7FFFFFFC) | slot: t_near >= 0 so its
    // bit pattern orders like the float, the two low bits hold the slot (keys are unique, order is total and identical in
    // the oracle); misses get 0xFFFFFFFF.  Five min/max pairs sort the four keys.
    // EARLY (the step is followed by another node step of the same scheduling decision): the nearest hit child -- or the
    // popped entry of a lane that hit nothing -- is known after two of the network's min levels, so its record is requested
    // right there into ndNext, and the rest of the ordering and the pushes of the other hit children run under that fetch
    // instead of in front of it.  Same stack operations per lane in the same order, so results and counters are unchanged.
    // (Round 3, measured and not kept: ordering only the NEAREST child and pushing the others in slot order -- no network, no
    // select chain per pushed child; 0.2 % more node visits on the 1M-triangle frame by the oracle's count.  Shaded frame
    // 0.2803 vs 0.2854 ms, icosphere soup 0.246 vs 0.255, but primary rays only 0.201 vs 0.192 and the 5M-triangle frame
    // 0.368 vs 0.361: the network runs under the early fetch, off the step's dependent chain, so removing it frees issue
    // slots nobody was waiting for.)
    // (N: Node, or NodeU on the scalar path with the plane table)
    // (RENDER: the pop is Stack::popLds; NARROW: the early fetch is load<true>)
    template <bool COUNT, int OCT, bool EARLY, bool RENDER = false, bool NARROW = false, class N>
    static __device__ __forceinline__ void closestStep(const N& nd, const Ray& r, float tmin, float tcull, Stack& stack,
                                                       int& cur, uint32_t& cntNodes, const float4* __restrict__ nodes, Node& ndNext)
    {
        const int4 refs = nd.refs;
        if (COUNT) cntNodes++;
        float tn[4];
        bool hit[4];
        slab<OCT>(nd, r, tmin, tcull, tn, hit);
        uint32_t key[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            key[k] = hit[k] ? ((__float_as_uint(tn[k]) & 0x7FFFFFFCu) | static_cast<uint32_t>(k)) : 0xFFFFFFFFu;
        const uint32_t nearest = min(min(key[0], key[1]), min(key[2], key[3])); // = key[0] after the network
        const bool any = nearest != 0xFFFFFFFFu;
        cur = any ? pick4(refs, nearest & 3u) : (stack.sp == 0 ? kDone : stack.popAs<RENDER>()); // a lane pops or pushes, never both
        if (EARLY) {
            if (cur >= 0) ndNext = load<NARROW>(nodes, cur);
        }
#define CRT_CSWAP(a, b) { const uint32_t lo = min(key[a], key[b]), hi = max(key[a], key[b]); key[a] = lo; key[b] = hi; }
        CRT_CSWAP(0, 1) CRT_CSWAP(2, 3) CRT_CSWAP(0, 2) CRT_CSWAP(1, 3) CRT_CSWAP(1, 2)
#undef CRT_CSWAP
        if (key[1] != 0xFFFFFFFFu) {
            if (key[3] != 0xFFFFFFFFu) stack.push(pick4(refs, key[3] & 3u)); // farthest first: the nearest pending child pops first
            if (key[2] != 0xFFFFFFFFu) stack.push(pick4(refs, key[2] & 3u));
            stack.push(pick4(refs, key[1] & 3u));
        }
    }

    // any hit: order independent, children taken in slot order
    // RENDER: the same step with its conditions formed on lane masks.  `bool & bool` is integer arithmetic, and the compiler
    // takes it literally: each compare mask becomes a 0/1 register (v_cndmask_b32 0, 1), the or / and run in vector registers,
    // a v_cmp turns each result back into a mask, and the "nothing hit" branch gets second, negated compares -- 13 vector
    // instructions per step, most of them half rate, for four scalar instructions' worth of work.  (`&&` / `||` fare no
    // better: two of the three conditions come out widened all the same.)  A ballot of a compare IS its mask, in an SGPR
    // pair; the masks are combined as 64-bit integers on the scalar unit and handed back as branch masks by the inverse
    // ballot.  One compare per child; same selects, same pop, the same three push blocks in the same order, so every
    // stack operation, result and counter is what the form below gives.  DESIGN section 5 has the listings and the timing.
    template <bool COUNT, int OCT, bool EARLY, bool RENDER = false, bool NARROW = false, class N>
    static __device__ __forceinline__ void anyStep(const N& nd, const Ray& r, float tmin, float tcull, Stack& stack,
                                                   int& cur, uint32_t& cntNodes, const float4* __restrict__ nodes, Node& ndNext)
    {
        const int4 refs = nd.refs;
        if (COUNT) cntNodes++;
        float tn[4];
        bool hit[4];
        slab<OCT>(nd, r, tmin, tcull, tn, hit);
        const bool h0 = hit[0], h1 = hit[1], h2 = hit[2], h3 = hit[3];
        if constexpr (RENDER) {
            const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1), m2 = __ballot(h2), m3 = __ballot(h3);
            const unsigned long long m01 = m0 | m1, m012 = m01 | m2;
            if constexpr (COUNT) {
                // the counting variants keep the last select behind the pop: with three selects in front of it the chain's value
                // lives across the pop's branches, and the counting Phong variant with wide offsets -- four counters more
                // to hold -- then reloads its arena pointer inside the loops (22 spilled registers instead of 11)
                cur = h0 ? refs.x : (h1 ? refs.y : (h2 ? refs.z : (__builtin_amdgcn_inverse_ballot_w64(m012 | m3) ? refs.w : (stack.sp == 0 ? kDone : stack.popLds()))));
            } else {
                cur = h0 ? refs.x : (h1 ? refs.y : (h2 ? refs.z : refs.w));
                if (__builtin_amdgcn_inverse_ballot_w64(~(m012 | m3))) cur = stack.sp == 0 ? kDone : stack.popLds(); // a lane pops or pushes, never both
            }
            if (EARLY) {
                if (cur >= 0) ndNext = load<NARROW>(nodes, cur);
            }
            if (__builtin_amdgcn_inverse_ballot_w64(m3 & m012)) stack.push(refs.w);
            if (__builtin_amdgcn_inverse_ballot_w64(m2 & m01)) stack.push(refs.z);
            if (__builtin_amdgcn_inverse_ballot_w64(m1 & m0)) stack.push(refs.y);
        } else {
            cur = h0 ? refs.x : (h1 ? refs.y : (h2 ? refs.z : (h3 ? refs.w : (stack.sp == 0 ? kDone : stack.popAs<RENDER>()))));
            if (EARLY) {
                if (cur >= 0) ndNext = load<NARROW>(nodes, cur);
            }
            // first hit slot became current; later hit slots are pushed, last slot first
            if (h3 & (h0 | h1 | h2)) stack.push(refs.w);
            if (h2 & (h0 | h1)) stack.push(refs.z);
            if (h1 & h0) stack.push(refs.y);
        }
    }
};

// The record of a scalar-path step: with the plane table (RENDER) and a known octant its planes come
// decoded (LayLegacy::NodeU), otherwise it is the plain record.  Per-lane steps always fetch the plain 64-byte record: a
// second fetch per lane costs more than the conversions it would save (section 5 of DESIGN.md).
template <int OCT, bool RENDER>
__device__ __forceinline__ auto loadUniformStep(const float4* nodes, const float* planes, int ref)
{
    if constexpr (RENDER && OCT < 8) return LayLegacy::loadUniformDecoded(nodes, planes, ref);
    else return LayLegacy::loadUniform(nodes, ref);
}

// The step macros below expand inside a traversal function and read its names: COUNT, OCT, nodes, planes, r, tmin, tcull,
// stack, cur, cntNodes.  Their RENDER and NARROW arguments are the traversal's (see closestIteration).
// Uniform descent: the rays of an 8x8 packet start at the root and usually agree on the first few nodes.  While every
// active lane stands on the SAME inner node its record is fetched once through the scalar cache (the node address is
// wave-uniform, so the loads become s_load) instead of 64 identical per-lane vector fetches; each lane still runs its own
// slab tests, ordering and pushes, so results and counters are exactly those of the per-lane loop that follows.
#define CRT_UNIFORM_DESCENT(STEP, RENDER, NARROW)                                                                              \
    for (;;) {                                                                                                                 \
        const int c0 = __builtin_amdgcn_readfirstlane(cur);                                                                    \
        if (!LayLegacy::inner(c0) || __ballot(cur != c0) != 0ull) break;                                                       \
        LayLegacy::Node ndUnused;                                                                                              \
        CRT_UNIFORM_STEP_STAT(STEP)                                                                                            \
        LayLegacy::STEP<COUNT, OCT, false, RENDER, NARROW>(loadUniformStep<OCT, RENDER>(nodes, planes, c0), r, tmin, tcull, stack, cur, cntNodes, nodes, ndUnused); \
    }
#define CRT_STEP_KIND_closestStep 0
#define CRT_STEP_KIND_anyStep 1
#if CRT_PROF
#define CRT_DIV_STATS_NODE stack.divStats(cur, stack.dvN, stack.dvNLanes, stack.dvNRuns, stack.dvNDistinct);
#define CRT_DIV_STATS_LEAF stack.divStats(cur, stack.dvL, stack.dvLLanes, stack.dvLRuns, stack.dvLDistinct);
#define CRT_STEP_STAT(WS, STEP) stack.stepStat(stack.WS, CRT_STEP_KIND_##STEP);
#define CRT_UNIFORM_STEP_STAT(STEP) CRT_STEP_STAT(wsU, STEP) stack.lsU[CRT_STEP_KIND_##STEP]++;
#define CRT_AGREE_STAT(STEP) stack.agreeStat(cur, CRT_STEP_KIND_##STEP);
#else
#define CRT_DIV_STATS_NODE
#define CRT_DIV_STATS_LEAF
#define CRT_STEP_STAT(WS, STEP)
#define CRT_UNIFORM_STEP_STAT(STEP)
#define CRT_AGREE_STAT(STEP)
#endif
// One node step of the lanes standing on inner nodes (called with exactly those lanes active): through the scalar cache
// when they all stand on the same node, per lane otherwise.
// (Measured and rejected: fetching the DISTINCT nodes of a divergent step once each -- 6.6 distinct nodes among 50 wanting
// lanes on the 1M-triangle frame -- by the first lanes of the wavefront and handing them out through LDS: a scalar loop
// peels the distinct values, fetchers load and ds_write, every lane ds_reads its slot.  Bit-exact, a seventh of the
// per-lane requests, and 0.49 ms instead of 0.31: the peeling loop and two LDS round trips per step cost far more than
// the requests they save.)
// CRT_NODE_STEPS: the NODE_STEPS node steps of one scheduling decision.  The first fetches its record here; every step
// but the last requests the next record itself (see closestStep), per lane.
#define CRT_FIRST_NODE_STEP(STEP, EARLY, RENDER, NARROW)                                                                       \
    {                                                                                                                          \
        const int c0 = __builtin_amdgcn_readfirstlane(cur);                                                                    \
        if (__ballot(cur != c0) == 0ull) {                                                                                     \
            CRT_UNIFORM_STEP_STAT(STEP)                                                                                        \
            LayLegacy::STEP<COUNT, OCT, EARLY, RENDER, NARROW>(loadUniformStep<OCT, RENDER>(nodes, planes, c0), r, tmin, tcull, stack, cur, cntNodes, nodes, ndNext); \
        } else {                                                                                                               \
            CRT_DIV_STATS_NODE                                                                                                 \
            CRT_STEP_STAT(wsD, STEP)                                                                                           \
            LayLegacy::STEP<COUNT, OCT, EARLY, RENDER, NARROW>(LayLegacy::load<NARROW>(nodes, cur), r, tmin, tcull, stack, cur, cntNodes, nodes, ndNext); \
        }                                                                                                                      \
    }
#define CRT_NODE_STEPS_AS(STEP, RENDER, NARROW)                                                                                \
    if (LayLegacy::inner(cur)) {                                                                                               \
        LayLegacy::Node ndNext;                                                                                                \
        CRT_FIRST_NODE_STEP(STEP, (NODE_STEPS > 1), RENDER, NARROW)                                                            \
        _Pragma("unroll") for (int rep = 1; rep < NODE_STEPS; rep++) {                                                         \
            if (LayLegacy::inner(cur)) {                                                                                       \
                CRT_STEP_STAT(wsF, STEP)                                                                                       \
                CRT_AGREE_STAT(STEP)                                                                                           \
                const LayLegacy::Node ndCur = ndNext;                                                                          \
                if (rep + 1 < NODE_STEPS) LayLegacy::STEP<COUNT, OCT, true, RENDER, NARROW>(ndCur, r, tmin, tcull, stack, cur, cntNodes, nodes, ndNext); \
                else LayLegacy::STEP<COUNT, OCT, false, RENDER, NARROW>(ndCur, r, tmin, tcull, stack, cur, cntNodes, nodes, ndNext); \
            }                                                                                                                  \
        }                                                                                                                      \
    }
#define CRT_NODE_STEPS(STEP) CRT_NODE_STEPS_AS(STEP, false, false)

__device__ __forceinline__ void loadTriUniform(const float4* T, float4& a, float4& b, float4& c)
{
    ConstQuadPtr C = (ConstQuadPtr)(reinterpret_cast<uintptr_t>(T));
    a = quadOf(C[0]); b = quadOf(C[1]); c = quadOf(C[2]);
}

// A candidate hit replaces the lane's closest one if it is nearer, or as near with the smaller triangle gid (the tie-break
// that makes the result independent of the visiting order); boxes are culled against the new distance from then on.
__device__ __forceinline__ void acceptHit(Hit& h, float& tcull, float t, float u, float v, uint32_t id, uint32_t gid)
{
    if ((t < h.t) | ((t == h.t) & (gid < h.gid))) {
        h.t = t; h.u = u; h.v = v; h.tri = id; h.gid = gid;
        tcull = t * kCullPad;
    }
}

// Wave-level scheduling shared by both traversals.  Every lane walks its own ray in its own fixed order (so results
// and counters do not depend on what the other lanes do), but WHEN a lane's next step runs is decided per wavefront:
// node steps are issued while at least `innerMin` lanes still stand on inner nodes (or nobody waits at a leaf); then the
// lanes waiting at leaves intersect their triangles.  innerMin = 1 is the classic while-while loop (leaves wait until
// every lane has one: 47 % of the lanes active on the 1M-triangle frame); a fixed 32 was the setting of rounds 1 and 2 (first
// measurement: 0.67 vs 1.10 ms).  Round 3: the threshold follows the wavefront's LIVE lanes -- three quarters of them -- because
// late in a packet's life most rays have finished, fewer than 32 lanes are left on inner nodes whatever happens, and a fixed 32
// then serves every single lane that reaches a leaf at once, a whole pass of the wavefront for one or two lanes: primary rays only
// 0.193 -> 0.172 ms, soup 0.256 -> 0.231, the longest packets shorten most (lone launch of an 8-rank share of primary rays 141 -> 126 us).
// One scheduling decision of the closest-hit traversal for the whole wavefront: NODE_STEPS node steps of the lanes standing
// on inner nodes, or the leaf step of the lanes waiting at leaves.  Per-lane state (cur, stack, h, tcull) lives in the
// caller, so a caller may retire finished rays and start new ones between two calls (streamClosest).  Returns false when
// no lane has anything left to do.
// RENDER: the render kernel's forms, which its two traversals take together and the others leave off.  Scalar-path steps read
// the decoded plane table (planes: kPlaneStride floats per node, render_kernels.h; without RENDER there is no table), pops
// are Stack::popLds, closest-hit leaves take the short reciprocal (triTest) and the six loads of a leaf pair are issued in
// front of their first wait (see the leaf loop below).  NARROW: per-lane node and triangle fetches take a 32-bit byte
// offset from the wave-uniform base (LayLegacy::load) -- the render kernel's narrow variants, the host's choice per scene.
template <bool COUNT, int OCT, bool RENDER = false, bool NARROW = false>
__device__ __forceinline__ bool closestIteration(const float4* __restrict__ nodes, const float4* __restrict__ tris, const Ray& r, float tmin,
                                                 float& tcull, Stack& stack, int innerMin, Hit& h, int& cur, uint32_t& iters,
                                                 uint32_t& cntNodes, uint32_t& cntTris, const float* __restrict__ planes = nullptr)
{
    const unsigned long long innerMask = __ballot(LayLegacy::inner(cur));
    const unsigned long long leafMask = __ballot(LayLegacy::leaf(cur));
    if ((innerMask | leafMask) == 0ull) return false;
    if (++iters == kBoostAfter) __builtin_amdgcn_s_setprio(3); // a wavefront on a long critical path stops queueing behind the others
    // innerMin > 0: node steps while at least that many lanes stand on inner nodes; innerMin <= 0 (adaptive): while at least
    // (live lanes * -innerMin) / 8 do (live = lanes with anything left to do), so that a wavefront whose rays have mostly finished
    // does not fall back to serving every single waiting leaf at once
    const int wantNode = innerMin > 0 ? innerMin : (static_cast<int>(__popcll(innerMask | leafMask)) * -innerMin + 7) / 8;
    if (innerMask != 0ull && (leafMask == 0ull || static_cast<int>(__popcll(innerMask)) >= wantNode)) {
#if CRT_PROF
        const unsigned long long ts0 = __builtin_amdgcn_s_memtime();
#endif
        CRT_NODE_STEPS_AS(closestStep, RENDER, NARROW) // several node steps per scheduling decision: fewer ballots/branches
#if CRT_PROF
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        stack.tNode += __builtin_amdgcn_s_memtime() - ts0; stack.itNode++; stack.lanesNode += __popcll(innerMask);
#endif
        return true;
    }
#if CRT_PROF
    const unsigned long long tl0 = __builtin_amdgcn_s_memtime();
    stack.itLeaf++; stack.lanesLeaf += __popcll(leafMask);
#endif
    if (LayLegacy::leaf(cur)) {
        uint32_t first, cnt;
        LayLegacy::leafRange(cur, first, cnt);
        const int lc0 = __builtin_amdgcn_readfirstlane(cur);
        if (__ballot(cur != lc0) == 0ull) {
            // every waiting lane stands on the same leaf: its triangles come through the scalar cache, once per wavefront
            uint32_t ufirst, ucnt;
            LayLegacy::leafRange(lc0, ufirst, ucnt);
            for (uint32_t i = 0; i < ucnt; i++) {
                const uint32_t id = LayLegacy::triId(ufirst, i);
                float4 a, b, c;
                loadTriUniform(LayLegacy::triPtr(tris, id), a, b, c);
                if (COUNT) cntTris++;
                float t, u, v;
                if (triTest<RENDER>(r, a, b, c, tmin, t, u, v)) acceptHit(h, tcull, t, u, v, id, __float_as_uint(c.w));
            }
        } else {
            CRT_DIV_STATS_LEAF
            // two triangles per trip, same test order, so that the second record's loads overlap the first's.  The source order
            // alone does not get that: the compiler issues the first record's three loads, waits for the first of them, starts
            // the triangle test and only then computes the second address and issues the second record's loads -- two memory
            // latencies one after the other.  RENDER: a scheduling barrier behind the six loads keeps every instruction on its
            // side, so both addresses are computed first, the six loads go out back to back and the first wait follows them:
            // one round trip per pair (listings and times in DESIGN section 5).
            for (uint32_t i = 0; i < cnt; i += 2) {
                const bool two = i + 1 < cnt;
                const uint32_t id = LayLegacy::triId(first, i), id1 = LayLegacy::triId(first, two ? i + 1 : i);
                const float4* T = LayLegacy::triPtr<NARROW>(tris, id);
                const float4* T1 = LayLegacy::triPtrSecond<NARROW>(tris, id, id1, two);
                const float4 a = T[0], b = T[1], c = T[2];
                const float4 a1 = T1[0], b1 = T1[1], c1 = T1[2];
                if constexpr (RENDER) __builtin_amdgcn_sched_barrier(0);
                if (COUNT) cntTris += two ? 2u : 1u;
                float t, u, v;
                if (triTest<RENDER>(r, a, b, c, tmin, t, u, v)) acceptHit(h, tcull, t, u, v, id, __float_as_uint(c.w));
                if (two & triTest<RENDER>(r, a1, b1, c1, tmin, t, u, v)) acceptHit(h, tcull, t, u, v, id1, __float_as_uint(c1.w));
            }
        }
        cur = stack.sp == 0 ? LayLegacy::kDone : stack.popAs<RENDER>();
    }
#if CRT_PROF
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    stack.tLeaf += __builtin_amdgcn_s_memtime() - tl0;
#endif
    return true;
}

template <bool COUNT, int OCT, bool RENDER, bool NARROW>
__device__ __forceinline__ void traceClosestOct(const float4* __restrict__ nodes, const float4* __restrict__ tris,
                                             uint32_t n_nodes, const Ray& r, float tmin, float tmax, Stack& stack, int innerMin,
                                             Hit& h, uint32_t& iters, uint32_t& cntNodes, uint32_t& cntTris, const float* __restrict__ planes)
{
    h.t = tmax; h.u = 0.0f; h.v = 0.0f; h.tri = 0; h.gid = 0;
    int cur = n_nodes ? LayLegacy::kRoot : LayLegacy::kDone;
    stack.sp = 0;
    float tcull = tmax * kCullPad; // boxes are culled against best_t * pad; changes only when a hit is accepted
    CRT_UNIFORM_DESCENT(closestStep, RENDER, NARROW)
    while (closestIteration<COUNT, OCT, RENDER, NARROW>(nodes, tris, r, tmin, tcull, stack, innerMin, h, cur, iters, cntNodes, cntTris, planes)) {}
}

// One scheduling decision of the any-hit traversal (see closestIteration); tmax / tcull / occluded are per-lane state of the caller
template <bool COUNT, int OCT, bool RENDER = false, bool NARROW = false>
__device__ __forceinline__ bool anyIteration(const float4* __restrict__ nodes, const float4* __restrict__ tris, const Ray& r, float tmin, float tmax,
                                             float tcull, Stack& stack, int innerMin, bool& occluded, int& cur, uint32_t& iters,
                                             uint32_t& cntNodes, uint32_t& cntTris, const float* __restrict__ planes = nullptr)
{
    const unsigned long long innerMask = __ballot(LayLegacy::inner(cur));
    const unsigned long long leafMask = __ballot(LayLegacy::leaf(cur));
    if ((innerMask | leafMask) == 0ull) return false;
    if (++iters == kBoostAfter) __builtin_amdgcn_s_setprio(3);
    // innerMin > 0: node steps while at least that many lanes stand on inner nodes; innerMin <= 0 (adaptive): while at least
    // (live lanes * -innerMin) / 8 do (live = lanes with anything left to do), so that a wavefront whose rays have mostly finished
    // does not fall back to serving every single waiting leaf at once
    const int wantNode = innerMin > 0 ? innerMin : (static_cast<int>(__popcll(innerMask | leafMask)) * -innerMin + 7) / 8;
    if (innerMask != 0ull && (leafMask == 0ull || static_cast<int>(__popcll(innerMask)) >= wantNode)) {
#if CRT_PROF
        const unsigned long long ts0 = __builtin_amdgcn_s_memtime();
#endif
        CRT_NODE_STEPS_AS(anyStep, RENDER, NARROW) // several node steps per scheduling decision: fewer ballots/branches
#if CRT_PROF
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        stack.tNode += __builtin_amdgcn_s_memtime() - ts0; stack.itNode++; stack.lanesNode += __popcll(innerMask);
#endif
        return true;
    }
#if CRT_PROF
    const unsigned long long tl0 = __builtin_amdgcn_s_memtime();
    stack.itLeaf++; stack.lanesLeaf += __popcll(leafMask);
#endif
    if (LayLegacy::leaf(cur)) {
        uint32_t first, cnt;
        LayLegacy::leafRange(cur, first, cnt);
        const int lc0 = __builtin_amdgcn_readfirstlane(cur);
        if (__ballot(cur != lc0) == 0ull) {
            uint32_t ufirst, ucnt;
            LayLegacy::leafRange(lc0, ufirst, ucnt);
            for (uint32_t i = 0; i < ucnt; i++) {
                float4 a, b, c;
                loadTriUniform(LayLegacy::triPtr(tris, LayLegacy::triId(ufirst, i)), a, b, c);
                if (COUNT) cntTris++;
                float t, u, v;
                if (triTest<false>(r, a, b, c, tmin, t, u, v) & (t < tmax)) {
                    occluded = true;
                    break;
                }
            }
        } else {
            for (uint32_t i = 0; i < cnt; i++) {
                const float4* T = LayLegacy::triPtr<NARROW>(tris, LayLegacy::triId(first, i));
                const float4 a = T[0], b = T[1], c = T[2];
                if (COUNT) cntTris++;
                float t, u, v;
                if (triTest<false>(r, a, b, c, tmin, t, u, v) & (t < tmax)) {
                    occluded = true;
                    break;
                }
            }
        }
        if constexpr (RENDER) { // the pop condition on lane masks, as in anyStep: no 0/1 register and no 16-bit or
            cur = LayLegacy::kDone;
            if (__builtin_amdgcn_inverse_ballot_w64(~(__ballot(occluded) | __ballot(stack.sp == 0)))) cur = stack.popLds();
        } else {
            cur = (occluded | (stack.sp == 0)) ? LayLegacy::kDone : stack.popAs<RENDER>();
        }
    }
#if CRT_PROF
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    stack.tLeaf += __builtin_amdgcn_s_memtime() - tl0;
#endif
    return true;
}

template <bool COUNT, int OCT, bool RENDER, bool NARROW>
__device__ __forceinline__ bool traceAnyOct(const float4* __restrict__ nodes, const float4* __restrict__ tris,
                                         uint32_t n_nodes, const Ray& r, float tmin, float tmax, Stack& stack, int innerMin,
                                         uint32_t& iters, uint32_t& cntNodes, uint32_t& cntTris, const float* __restrict__ planes)
{
    bool occluded = false;
    int cur = n_nodes ? LayLegacy::kRoot : LayLegacy::kDone;
    stack.sp = 0;
    const float tcull = tmax * kCullPad;
    CRT_UNIFORM_DESCENT(anyStep, RENDER, NARROW)
    while (anyIteration<COUNT, OCT, RENDER, NARROW>(nodes, tris, r, tmin, tmax, tcull, stack, innerMin, occluded, cur, iters, cntNodes, cntTris, planes)) {}
    return occluded;
}

// Pick the traversal loop specialised for the wavefront's direction octant when all its active lanes share one (nearly
// every 8x8 camera packet and every packet of shadow rays towards one light does); otherwise the generic loop.
__device__ __forceinline__ uint32_t octantOf(const Ray& r)
{
    return (__float_as_uint(r.d.x) >> 31) | ((__float_as_uint(r.d.y) >> 31) << 1) | ((__float_as_uint(r.d.z) >> 31) << 2);
}

template <bool COUNT, bool RENDER = false, bool NARROW = false>
__device__ __forceinline__ void traceClosest(const float4* __restrict__ nodes, const float4* __restrict__ tris,
                                             uint32_t n_nodes, const Ray& r, float tmin, float tmax, Stack& stack, int innerMin,
                                             Hit& h, uint32_t& iters, uint32_t& cntNodes, uint32_t& cntTris, const float* __restrict__ planes = nullptr)
{
    const uint32_t oct = octantOf(r);
    const uint32_t o0 = __builtin_amdgcn_readfirstlane(oct);
    if (__ballot(oct != o0) == 0ull) {
        switch (o0) {
#define CRT_CASE(k) case k: traceClosestOct<COUNT, k, RENDER, NARROW>(nodes, tris, n_nodes, r, tmin, tmax, stack, innerMin, h, iters, cntNodes, cntTris, planes); return;
            CRT_CASE(0) CRT_CASE(1) CRT_CASE(2) CRT_CASE(3) CRT_CASE(4) CRT_CASE(5) CRT_CASE(6) CRT_CASE(7)
#undef CRT_CASE
        }
    }
    traceClosestOct<COUNT, 8, RENDER, NARROW>(nodes, tris, n_nodes, r, tmin, tmax, stack, innerMin, h, iters, cntNodes, cntTris, planes);
}

template <bool COUNT, bool RENDER = false, bool NARROW = false>
__device__ __forceinline__ bool traceAny(const float4* __restrict__ nodes, const float4* __restrict__ tris,
                                         uint32_t n_nodes, const Ray& r, float tmin, float tmax, Stack& stack, int innerMin,
                                         uint32_t& iters, uint32_t& cntNodes, uint32_t& cntTris, const float* __restrict__ planes = nullptr)
{
    const uint32_t oct = octantOf(r);
    const uint32_t o0 = __builtin_amdgcn_readfirstlane(oct);
    if (__ballot(oct != o0) == 0ull) {
        switch (o0) {
#define CRT_CASE(k) case k: return traceAnyOct<COUNT, k, RENDER, NARROW>(nodes, tris, n_nodes, r, tmin, tmax, stack, innerMin, iters, cntNodes, cntTris, planes);
            CRT_CASE(0) CRT_CASE(1) CRT_CASE(2) CRT_CASE(3) CRT_CASE(4) CRT_CASE(5) CRT_CASE(6) CRT_CASE(7)
#undef CRT_CASE
        }
    }
    return traceAnyOct<COUNT, 8, RENDER, NARROW>(nodes, tris, n_nodes, r, tmin, tmax, stack, innerMin, iters, cntNodes, cntTris, planes);
}

} // namespace
} // namespace crt
