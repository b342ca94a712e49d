// HIP kernel for gfx950 (MI355X): where the hit of a ray query was one snapshot ago (crt_previous_points*, crt_frame_motion*; the
// contract is in include/crt_hip.h, the reasons in DESIGN.md section 5i).  A dynamic scene keeps its world vertices in HBM by
// vertex (refit.h DynamicScene::dWorldXyz) and, since crt_motion_snapshot, a copy of them as they were then (dPrevXyz).  A hit
// names its triangle by (inst, prim) and its place in it by (u, v); the triangle's three vertex numbers are fixed at upload, so
// the same barycentrics over the snapshot's vertices are the point the surface element came from -- whatever tree was built,
// refitted or rebuilt in between.
//
//   one lane per record, a grid-stride loop over 256-lane workgroups; 16 B of ids and barycentrics in, 12 B out, and three
//   index and up to 72 B of vertex reads gathered through the mesh table.  No LDS, no atomics, no scratch.
//   "Not moved / unknown" is three quiet NaNs (0x7FC00000), written as integers so that no NaN payload rule applies.
//
// Arithmetic: float32, -ffp-contract=off: per component fmaf(v, q2 - q0, fmaf(u, q1 - q0, q0)), each difference rounded once --
// the form crt_closest_points uses for its point.  Bit for bit tests/motion_reference.c.
#include "mesh_table.hip.h"
#include "render_kernels.h"

#include <algorithm>
#include <cfloat>

namespace crt {
namespace {

constexpr uint32_t kMotionBlock = 256;
constexpr uint32_t kMotionMaxGrid = 1u << 20; // workgroups of a launch; the kernel strides over what is left
constexpr uint32_t kQuietNan = 0x7FC00000u;

__global__ __launch_bounds__(256) void previousPointsKernel(const PreviousPointsParams p)
{
    const MeshEntry* __restrict__ table = static_cast<const MeshEntry*>(p.table);
    const float2* __restrict__ uvs = reinterpret_cast<const float2*>(p.uv);
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(p.point);
    const size_t stride = static_cast<size_t>(gridDim.x) * kMotionBlock;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kMotionBlock + threadIdx.x; i < p.n; i += stride) {
        const uint32_t inst = p.inst[i], prim = p.prim[i];
        const float2 uv = uvs[i];
        uint32_t r[3] = { kQuietNan, kQuietNan, kQuietNan };
        // CRT_MISS is 0xFFFFFFFF: no mesh has that ordinal
        if (p.prev != nullptr && inst < p.nMeshes && uv.x == uv.x && uv.y == uv.y) {
            const uint32_t triStart = table[inst].triStart, vertStart = table[inst].vertStart;
            if (prim < table[inst + 1u].triStart - triStart) {
                const size_t g = 3u * (static_cast<size_t>(triStart) + prim);
                const size_t a = 3u * (static_cast<size_t>(vertStart) + p.idx[g]), b = 3u * (static_cast<size_t>(vertStart) + p.idx[g + 1u]),
                             c = 3u * (static_cast<size_t>(vertStart) + p.idx[g + 2u]);
                bool same = true, finite = true;
                float res[3];
#pragma unroll
                for (uint32_t k = 0; k < 3u; k++) {
                    const float q0 = p.prev[a + k], q1 = p.prev[b + k], q2 = p.prev[c + k];
                    same = same && __float_as_uint(q0) == __float_as_uint(p.world[a + k]) && __float_as_uint(q1) == __float_as_uint(p.world[b + k]) &&
                           __float_as_uint(q2) == __float_as_uint(p.world[c + k]);
                    const float e1 = q1 - q0, e2 = q2 - q0;
                    res[k] = fmaf(uv.y, e2, fmaf(uv.x, e1, q0));
                    finite = finite && fabsf(res[k]) <= FLT_MAX; // false for NaN
                }
                if (!same && finite) {
#pragma unroll
                    for (uint32_t k = 0; k < 3u; k++) r[k] = __float_as_uint(res[k]);
                }
            }
        }
        out[3u * i] = r[0];
        out[3u * i + 1u] = r[1];
        out[3u * i + 2u] = r[2];
    }
}

} // namespace

int launchPreviousPoints(const PreviousPointsParams& p, ihipStream_t* stream)
{
    if (p.n == 0u) return static_cast<int>(hipSuccess);
    const uint64_t blocks = (static_cast<uint64_t>(p.n) + kMotionBlock - 1u) / kMotionBlock;
    const dim3 g(static_cast<uint32_t>(std::min<uint64_t>(blocks, kMotionMaxGrid))), block(kMotionBlock);
    hipLaunchKernelGGL(previousPointsKernel, g, block, 0, stream, p);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
