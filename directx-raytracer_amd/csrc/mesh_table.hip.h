// The meshes as they sit in HBM back to back, for the kernels that read vertices by triangle (bvh_gpu.hip: the GPU build;
// refit_kernels.hip: the refit of a dynamic scene).  One entry per mesh plus a terminator holding the totals.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace crt {

struct MeshEntry {
    uint32_t triStart, vertStart, nVerts, material;
    uint32_t hasNormals, hasUvs, pad0, pad1;
};

#ifdef __HIPCC__
// the mesh of global triangle g: the largest m with triStart[m] <= g (meshes without triangles are skipped by the <=)
__device__ __forceinline__ uint32_t meshOf(const MeshEntry* __restrict__ table, uint32_t n_meshes, uint32_t g)
{
    uint32_t lo = 0, hi = n_meshes;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (table[mid].triStart <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}
#endif

} // namespace crt
