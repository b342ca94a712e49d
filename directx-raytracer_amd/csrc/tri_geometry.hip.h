// The per-triangle rules of the device-side geometry code, each written once: how a triangle is fetched through the mesh table
// (mesh_table.hip.h), which triangle is inert, its box, the geometric part of its record and its vertex normals, the selects
// boxes are folded with and the Morton quantisation (the leaf reference: bvh_wide.h, with the host builder).  Both GPU builders (bvh_gpu.hip, bvh_ploc.hip), the
// refit and the rebuild (refit_kernels.hip) are callers, which is what makes them write the same bytes; flattenMeshes
// (bvh_build.cpp) is the host statement of the same rules.  Everything is force-inlined and the files are built with
// -ffp-contract=off: the order of operations of every expression here, and the direction of every select, is part of the contract.
#pragma once

#include "../../include/crt_hip.h"
#include "bvh_wide.h" // leafRef: the leaf reference, shared with the host builder
#include "mesh_table.hip.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace crt {

struct Box6 { float mn[3], mx[3]; };

// "a < b ? a : b" picks the last of equal values (and b when either is NaN): the oracle's aabb_grow
__host__ __device__ __forceinline__ float minSel(float a, float b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ float maxSel(float a, float b) { return a > b ? a : b; }

__host__ __device__ __forceinline__ Box6 unionBox(const Box6& a, const Box6& b)
{
    Box6 u;
    for (int k = 0; k < 3; k++) {
        u.mn[k] = minSel(a.mn[k], b.mn[k]);
        u.mx[k] = maxSel(a.mx[k], b.mx[k]);
    }
    return u;
}

// ---- 30-bit Morton codes: 10 bits per axis, cubic cells sized by the longest extent of the centroid bounds
__host__ __device__ __forceinline__ uint32_t expandBits10(uint32_t v)
{
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__host__ __device__ __forceinline__ uint32_t quant10(float f) { return f >= 0.0f ? (f < 1024.0f ? static_cast<uint32_t>(f) : 1023u) : 0u; }
__host__ __device__ __forceinline__ float mortonScale(float longestExtent) { return longestExtent > 0.0f ? 1024.0f / longestExtent : 0.0f; }

#ifdef __HIPCC__
// Global triangle g as the mesh arrays give it.  An inert triangle (crt_hip.h: some corner is not finite) keeps its place in
// the records and the leaves but has the box of the point (0, 0, 0) and a record of nine quiet NaNs.
struct TriFetch {
    uint32_t mesh;    // ordinal of its mesh
    MeshEntry M;      // that mesh's entry
    uint32_t v[3];    // global vertex numbers
    float p[3][3];    // the corners (zeros when !inRange)
    bool inRange;     // every index < M.nVerts (looked at only when asked for: kCheckIndices)
    bool finite;      // every corner coordinate x has x - x == 0
};

template <bool kCheckIndices = false>
__device__ __forceinline__ TriFetch fetchTri(const MeshEntry* __restrict__ table, uint32_t n_meshes, const float* __restrict__ xyz,
                                             const uint32_t* __restrict__ idx, uint32_t g)
{
    TriFetch t;
    t.mesh = meshOf(table, n_meshes, g);
    t.M = table[t.mesh];
    const uint32_t i0 = idx[3 * static_cast<size_t>(g)], i1 = idx[3 * static_cast<size_t>(g) + 1], i2 = idx[3 * static_cast<size_t>(g) + 2];
    t.v[0] = t.M.vertStart + i0;
    t.v[1] = t.M.vertStart + i1;
    t.v[2] = t.M.vertStart + i2;
    t.inRange = !kCheckIndices || !(i0 >= t.M.nVerts || i1 >= t.M.nVerts || i2 >= t.M.nVerts);
    t.finite = t.inRange;
    if (!t.inRange) {
        for (int c = 0; c < 3; c++)
            for (int k = 0; k < 3; k++) t.p[c][k] = 0.0f;
        return t;
    }
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < 3; k++) t.p[c][k] = xyz[3 * static_cast<size_t>(t.v[c]) + k];
    for (int k = 0; k < 3; k++)
        t.finite &= t.p[0][k] - t.p[0][k] == 0.0f && t.p[1][k] - t.p[1][k] == 0.0f && t.p[2][k] - t.p[2][k] == 0.0f; // x - x == 0: finite
    return t;
}

__device__ __forceinline__ Box6 triBox(const TriFetch& t)
{
    Box6 b;
    for (int k = 0; k < 3; k++) {
        b.mn[k] = t.finite ? minSel(minSel(t.p[0][k], t.p[1][k]), t.p[2][k]) : 0.0f;
        b.mx[k] = t.finite ? maxSel(maxSel(t.p[0][k], t.p[1][k]), t.p[2][k]) : 0.0f;
    }
    return b;
}

// the geometric part of a crt_bvh_tri: v0, e1 = v1 - v0, e2 = v2 - v0
__device__ __forceinline__ void triRecord(const TriFetch& t, float v0[3], float e1[3], float e2[3])
{
    const float qnan = __uint_as_float(0x7FC00000u); // the one bit pattern of an inert triangle's record
    for (int k = 0; k < 3; k++) {
        v0[k] = t.finite ? t.p[0][k] : qnan;
        e1[k] = t.finite ? t.p[1][k] - t.p[0][k] : qnan;
        e2[k] = t.finite ? t.p[2][k] - t.p[0][k] : qnan;
    }
}

// the vertex normals of a crt_bvh_shade; left as they are for a mesh without normals
__device__ __forceinline__ void triNormals(const TriFetch& t, const float* __restrict__ normals, float n0[3], float n1[3], float n2[3])
{
    if (!t.M.hasNormals) return;
    for (int k = 0; k < 3; k++) {
        n0[k] = normals[3 * static_cast<size_t>(t.v[0]) + k];
        n1[k] = normals[3 * static_cast<size_t>(t.v[1]) + k];
        n2[k] = normals[3 * static_cast<size_t>(t.v[2]) + k];
    }
}
#endif

} // namespace crt
