// Host BVH builder of the product: stands in for BuildRaytracingAccelerationStructure
// (R/DXRTRenderer.cpp:548-806; driver-built BLAS per mesh + TLAS with identity transforms => one flat
// world-space hierarchy here).  Deterministic binned SAH, spec in DESIGN.md "BVH build".
#pragma once

#include "../../include/crt_hip.h"

#include "hip_own.h"

#include <cstddef>
#include <cstdint>
#include <vector>

struct ihipStream_t;

namespace crt {

constexpr int kLeafMax = 4;       // triangles per leaf
constexpr int kLbvhLeafMax = 2;   // GPU LBVH: a Karras node over at most this many triangles becomes a leaf (oracle: LBVH_LEAF_MAX)
constexpr int kMaxDepth = 32;     // leaves at depth <= kMaxDepth => traversal stack <= kMaxDepth entries
constexpr int kBins = 16;
constexpr float kTravCost = 1.0f; // SAH cost of an inner-node visit, in triangle tests

// bytes in HBM of n leaf-ordered records of `each` bytes / of n quantised wide nodes: a speculative wide load of the last record
// may reach past it, so every such buffer ends in slack.  These two are the only statements of how much.
inline size_t recordBytes(size_t each, size_t n) { return each * n + 64; }
inline size_t quantisedBytes(size_t n) { return sizeof(crt_bvh_node4q) * n + 128; }

// A tree in HBM and its leaf-ordered records, owned: what it still holds is freed with it.  Move-only.
struct DeviceTree {
    DeviceBuffer nodes;    // binary nodes, DFS pre-order (empty for a host-built tree nobody will refit)
    DeviceBuffer nodes4;   // wide nodes (idem)
    DeviceBuffer nodes4q;  // quantised wide nodes: what the kernels traverse (quantisedBytes)
    DeviceBuffer tris, shade, uvs; // leaf order (recordBytes); uvs empty when no mesh has any
    uint32_t nNodes = 0, nNodes4 = 0, nTris = 0, depth4 = 0, maxDepth = 0;
};

struct Bvh {
    std::vector<crt_bvh_node> nodes;   // binary tree, 64 B each, DFS pre-order, node 0 = root (builder output, host only)
    std::vector<crt_bvh_node4> nodes4; // wide tree collapsed from it, 128 B each, DFS pre-order: what is uploaded and traversed
    std::vector<crt_bvh_node4q> nodes4q; // its 64-byte quantised form (quantizeBvh4): what is uploaded and traversed
    uint32_t depth4 = 0;               // levels of the wide tree
    std::vector<crt_bvh_tri> tris;     // 48 B each, leaf order
    std::vector<crt_bvh_shade> shade;  // 48 B each, leaf order
    std::vector<crt_bvh_uv> uvs;       // 24 B each, leaf order; empty when no mesh has uvs
    uint32_t maxDepth = 0;
    uint32_t nTris = 0;                // triangles; = tris.size() unless the tree and its records exist in HBM only:
    DeviceTree dev;                    // a tree the GPU builders made (the host vectors above then stay empty), until someone takes it
};

// meshes in InstanceID order; triangle gid = running ordinal over meshes. Throws std::runtime_error on bad input.
void buildBvh(const crt_mesh_view* meshes, uint32_t n_meshes, Bvh& out);
// shared first step of both builders (see bvh_build.cpp)
void flattenMeshes(const crt_mesh_view* meshes, uint32_t n_meshes, std::vector<crt_bvh_tri>& inTri, std::vector<crt_bvh_shade>& inShade,
                   std::vector<float>& boxCent);
// the GPU builders (option "gpu_builder"): Karras LBVH (bvh_gpu.hip) or PLOC (bvh_ploc.hip)
constexpr int kGpuBuilderLbvh = 0;
constexpr int kGpuBuilderPloc = 1;
// GPU build (bvh_gpu.hip): same output layout as buildBvh, lower quality, much faster; throws std::runtime_error on HIP errors
void buildBvhGpu(const crt_mesh_view* meshes, uint32_t n_meshes, Bvh& out, struct ihipStream_t* stream, double* device_ms,
                 int builder = kGpuBuilderLbvh);
// meshes already in HBM, as mesh_table.hip.h lays them out: the input of a rebuild (crt_rebuild)
struct GpuMeshes {
    const void* table = nullptr;     // MeshEntry per mesh + terminator
    uint32_t nMeshes = 0, n = 0;     // meshes, triangles
    const float* xyz = nullptr;      // 3 per vertex, world space
    const uint32_t* idx = nullptr;   // 3 per triangle, mesh-local
    const float* normals = nullptr;  // 3 per vertex or NULL
    const float* uvsIn = nullptr;    // 3 per vertex (u, v, unused) or NULL: no uv records
};
// the same build from meshes in HBM (n > kLeafMax)
DeviceTree rebuildBvhGpu(const GpuMeshes& in, int builder, struct ihipStream_t* stream, double* device_ms);
// A host tree goes to HBM (synchronous copies).  withBinaryAndWide: also the binary and the full-precision wide nodes (what a refit
// starts from and the exports of a dynamic scene read); otherwise what the kernels traverse only.
DeviceTree uploadTree(const Bvh& host, bool withBinaryAndWide);
// exclusive prefix sum of n uint32 counts on the device (gpu_sort.hip.h, whose kernels live in bvh_gpu.hip); tileSums holds
// deviceScanScratchBytes(n); returns the first launch error (a hipError_t)
int deviceExclusiveSum(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* tileSums, struct ihipStream_t* stream);
size_t deviceScanScratchBytes(uint32_t n);
// PLOC's tree (bvh_ploc.hip) from the Morton-sorted keys (gid in the low dword) and the per-gid triangle boxes (min xyz, max xyz):
// the binary nodes in DFS pre-order in `nodes` (allocated here, returned count) and the keys in leaf order at leafKeys[0..n)
uint32_t plocBuildGpu(const unsigned long long* sortedKeys, const float* triBoxes, uint32_t n, unsigned long long* leafKeys, DeviceBuffer& nodes,
                      struct ihipStream_t* stream);
// per-triangle uvs in input (gid) order, empty when no mesh has any; and their permutation to leaf order
void flattenUvs(const crt_mesh_view* meshes, uint32_t n_meshes, std::vector<crt_bvh_uv>& inUv);
void reorderUvs(const std::vector<crt_bvh_uv>& inUv, Bvh& bvh);
// binary -> wide collapse (DESIGN.md "BVH4"); called by both builders
void collapseBvh4(Bvh& bvh);
// the same collapse + quantisation on the device (bvh_gpu.hip), shared by the GPU builder and the refit of a dynamic scene
size_t collapseScratchBytes(uint32_t nBinary);
void collapseWideGpu(const crt_bvh_node* nodes, uint32_t nBinary, void* scratch, void* nodes4, void* nodes4q, DeviceTree* fresh,
                     struct ihipStream_t* stream, uint32_t* nWide, uint32_t* depth4, uint32_t* maxDepth);
// (the collapse and quantisation rules themselves: bvh_wide.h, shared with the GPU builder)

} // namespace crt
