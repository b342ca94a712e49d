// HIP kernels for gfx950 (MI355X): the backward pass of the closest-hit and the closest-point query (crt_trace_rays_backward*,
// crt_closest_points_backward*; the contract is in include/crt_hip.h "gradients", the derivation in DESIGN.md section 5p).  A hit
// names its triangle by (inst, prim); a dynamic scene keeps the world vertices by vertex (refit.h DynamicScene::dWorldXyz) and the
// mesh-local indices (dIdx), so the gradient of a loss on t / u / v (or on dist) with respect to the record and to the triangle's
// three world vertices is a gather, a 3x3 solve in closed form and a scatter-add -- whatever tree was built, refitted or rebuilt.
//
//   one lane per record, a grid-stride loop over 256-lane workgroups, as previousPointsKernel; no LDS, no scratch memory.
//   The scatter: every float32 contribution is widened to float64 and added to a context-owned array of 3 doubles per vertex with
//   the hardware float64 atomic add (global_atomic_add_f64, no compare-and-swap loop; the array is coarse-grained hipMalloc
//   memory); gradFinalizeKernel rounds each sum to float32 once.  No atomics at all when the caller wants no vertex gradient.
//
// Arithmetic per record: float32, -ffp-contract=off, in the operation order the header fixes; bit for bit tests/grad_reference.c.
#include "mesh_table.hip.h"
#include "render_kernels.h"

#include <algorithm>
#include <cfloat>

namespace crt {
namespace {

constexpr uint32_t kGradBlock = 256;
constexpr uint32_t kGradMaxGrid = 1u << 20; // workgroups of a launch; the kernels stride over what is left

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= FLT_MAX; } // false for NaN

// the three vertices of (inst, prim) as offsets into the by-vertex arrays; false: the ids name no triangle (CRT_MISS is
// 0xFFFFFFFF: no mesh has that ordinal).  The indices were checked against the mesh's vertex count at upload
__device__ __forceinline__ bool triangleOf(const MeshEntry* __restrict__ table, uint32_t nMeshes, const uint32_t* __restrict__ idx, uint32_t inst,
                                           uint32_t prim, size_t at[3])
{
    if (inst >= nMeshes) return false;
    const uint32_t triStart = table[inst].triStart, vertStart = table[inst].vertStart;
    if (prim >= table[inst + 1u].triStart - triStart) return false;
    const size_t g = 3u * (static_cast<size_t>(triStart) + prim);
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++) at[k] = 3u * (static_cast<size_t>(vertStart) + idx[g + k]);
    return true;
}

// vertex sums += -(w s), -(u s), -(v s) for the triangle's a, b, c
__device__ __forceinline__ void scatter(double* __restrict__ sums, const size_t at[3], float u, float v, const float s[3])
{
    const float w = (1.0f - u) - v;
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++) {
        unsafeAtomicAdd(sums + at[0] + k, static_cast<double>(-(w * s[k])));
        unsafeAtomicAdd(sums + at[1] + k, static_cast<double>(-(u * s[k])));
        unsafeAtomicAdd(sums + at[2] + k, static_cast<double>(-(v * s[k])));
    }
}

__global__ __launch_bounds__(256) void rayGradKernel(const RayGradParams p)
{
    const MeshEntry* __restrict__ table = static_cast<const MeshEntry*>(p.table);
    const float4* __restrict__ rays = reinterpret_cast<const float4*>(p.rays);
    const float2* __restrict__ uvs = reinterpret_cast<const float2*>(p.uv);
    const float2* __restrict__ gradUv = reinterpret_cast<const float2*>(p.gradUv);
    float4* __restrict__ out = reinterpret_cast<float4*>(p.gradRays);
    const size_t stride = static_cast<size_t>(gridDim.x) * kGradBlock;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kGradBlock + threadIdx.x; i < p.n; i += stride) {
        float lam[3] = { 0.0f, 0.0f, 0.0f }, tl[3] = { 0.0f, 0.0f, 0.0f };
        size_t at[3];
        bool live = false;
        const float2 uv = uvs[i];
        if (triangleOf(table, p.nMeshes, p.idx, p.inst[i], p.prim[i], at)) {
            const float t = p.t[i];
            const float gt = p.gradT ? p.gradT[i] : 0.0f;
            const float2 guv = gradUv ? gradUv[i] : make_float2(0.0f, 0.0f);
            if (finite1(t) && finite1(uv.x) && finite1(uv.y) && finite1(gt) && finite1(guv.x) && finite1(guv.y)) {
                const float4 dr = rays[2u * i + 1u];
                const float d[3] = { dr.x, dr.y, dr.z };
                float e1[3], e2[3];
#pragma unroll
                for (uint32_t k = 0; k < 3u; k++) {
                    const float a = p.world[at[0] + k];
                    e1[k] = p.world[at[1] + k] - a;
                    e2[k] = p.world[at[2] + k] - a;
                }
                const float nn[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] }; // e1 x e2
                const float pp[3] = { d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0] };       // d x e2
                const float qq[3] = { e1[1] * d[2] - e1[2] * d[1], e1[2] * d[0] - e1[0] * d[2], e1[0] * d[1] - e1[1] * d[0] };       // e1 x d
                const float det = -((d[0] * nn[0] + d[1] * nn[1]) + d[2] * nn[2]);
                live = true;
#pragma unroll
                for (uint32_t k = 0; k < 3u; k++) {
                    const float num = (gt * nn[k] + guv.x * pp[k]) + guv.y * qq[k];
                    lam[k] = num / det;
                    tl[k] = t * lam[k];
                    live = live && finite1(lam[k]) && finite1(tl[k]);
                }
            }
        }
        if (!live) lam[0] = lam[1] = lam[2] = tl[0] = tl[1] = tl[2] = 0.0f;
        if (out) {
            out[2u * i] = make_float4(lam[0], lam[1], lam[2], 0.0f);
            out[2u * i + 1u] = make_float4(tl[0], tl[1], tl[2], 0.0f);
        }
        if (live && p.sums) scatter(p.sums, at, uv.x, uv.y, lam);
    }
}

__global__ __launch_bounds__(256) void pointGradKernel(const PointGradParams p)
{
    const MeshEntry* __restrict__ table = static_cast<const MeshEntry*>(p.table);
    const float4* __restrict__ points = reinterpret_cast<const float4*>(p.points);
    const float2* __restrict__ uvs = reinterpret_cast<const float2*>(p.uv);
    float4* __restrict__ out = reinterpret_cast<float4*>(p.gradPoints);
    const size_t stride = static_cast<size_t>(gridDim.x) * kGradBlock;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kGradBlock + threadIdx.x; i < p.n; i += stride) {
        float s[3] = { 0.0f, 0.0f, 0.0f };
        size_t at[3];
        bool live = false;
        const float2 uv = uvs[i];
        if (triangleOf(table, p.nMeshes, p.idx, p.inst[i], p.prim[i], at)) {
            const float g = p.gradDist[i];
            if (finite1(uv.x) && finite1(uv.y) && finite1(g)) {
                const float4 pt = points[i];
                const float x[3] = { pt.x, pt.y, pt.z };
                float r[3];
#pragma unroll
                for (uint32_t k = 0; k < 3u; k++) {
                    const float a = p.world[at[0] + k];
                    const float e1 = p.world[at[1] + k] - a, e2 = p.world[at[2] + k] - a;
                    r[k] = x[k] - fmaf(uv.y, e2, fmaf(uv.x, e1, a));
                }
                const float len = sqrtf((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
                live = len > 0.0f && finite1(len); // false for NaN
#pragma unroll
                for (uint32_t k = 0; k < 3u; k++) {
                    s[k] = g * (r[k] / len);
                    live = live && finite1(s[k]);
                }
            }
        }
        if (!live) s[0] = s[1] = s[2] = 0.0f;
        if (out) out[i] = make_float4(s[0], s[1], s[2], 0.0f);
        if (live && p.sums) scatter(p.sums, at, uv.x, uv.y, s);
    }
}

__global__ __launch_bounds__(256) void gradFinalizeKernel(const double* __restrict__ sums, float* __restrict__ out, size_t n)
{
    const size_t stride = static_cast<size_t>(gridDim.x) * kGradBlock;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kGradBlock + threadIdx.x; i < n; i += stride) out[i] = static_cast<float>(sums[i]);
}

dim3 gradGrid(uint64_t n)
{
    const uint64_t blocks = (n + kGradBlock - 1u) / kGradBlock;
    return dim3(static_cast<uint32_t>(std::min<uint64_t>(blocks, kGradMaxGrid)));
}

} // namespace

int launchRayGrad(const RayGradParams& p, ihipStream_t* stream)
{
    if (p.n == 0u) return static_cast<int>(hipSuccess);
    hipLaunchKernelGGL(rayGradKernel, gradGrid(p.n), dim3(kGradBlock), 0, stream, p);
    return static_cast<int>(hipGetLastError());
}

int launchPointGrad(const PointGradParams& p, ihipStream_t* stream)
{
    if (p.n == 0u) return static_cast<int>(hipSuccess);
    hipLaunchKernelGGL(pointGradKernel, gradGrid(p.n), dim3(kGradBlock), 0, stream, p);
    return static_cast<int>(hipGetLastError());
}

int launchGradFinalize(const double* sums, float* out, size_t n, ihipStream_t* stream)
{
    if (n == 0u) return static_cast<int>(hipSuccess);
    hipLaunchKernelGGL(gradFinalizeKernel, gradGrid(n), dim3(kGradBlock), 0, stream, sums, out, n);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
