// The meshes as they sit in HBM back to back, for the kernels that read vertices by triangle (bvh_gpu.hip: the GPU build;
// refit_kernels.hip: the refit of a dynamic scene).  One entry per mesh plus a terminator holding the totals.
#pragma once

#include "../../include/crt_hip.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace crt {

struct MeshEntry {
    uint32_t triStart, vertStart, nVerts, material;
    uint32_t hasNormals, hasUvs, pad0, pad1;
};

// the table of `meshes` on the host: one entry per mesh and the terminator (its triStart / vertStart are the totals, as 64-bit
// sums truncated: the callers check the limits)
inline std::vector<MeshEntry> makeMeshTable(const crt_mesh_view* meshes, uint32_t n_meshes)
{
    std::vector<MeshEntry> table(n_meshes + 1u);
    uint64_t t0 = 0, v0 = 0;
    for (uint32_t m = 0; m <= n_meshes; m++) {
        MeshEntry& E = table[m];
        E = MeshEntry{ static_cast<uint32_t>(t0), static_cast<uint32_t>(v0), 0u, 0u, 0u, 0u, 0u, 0u };
        if (m == n_meshes) break;
        const crt_mesh_view& M = meshes[m];
        E.nVerts = M.n_vertices;
        E.material = static_cast<uint32_t>(M.material_index);
        E.hasNormals = M.normals ? 1u : 0u;
        E.hasUvs = M.uvs ? 1u : 0u;
        t0 += M.n_triangles;
        v0 += M.n_vertices;
    }
    return table;
}

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
