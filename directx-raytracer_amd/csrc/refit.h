// Dynamic geometry (option "dynamic"): what a scene keeps in HBM so that moved vertices can be refitted into the uploaded tree
// instead of rebuilding it (refit_kernels.hip; DESIGN.md "Dynamic geometry"), or a new tree built from them on the GPU
// (dynamicRebuild).  The topology -- triangles, indices, uvs, materials -- is fixed at upload, the binary tree's
// shape and leaf order until a rebuild; a refit rewrites the vertices' world positions, the
// leaf-ordered triangle and shading records, the binary boxes and, by collapsing again, the wide tree and its plane table.
#pragma once

#include "../../include/crt_hip.h"
#include "bvh_build.h"

#include <cstdint>
#include <vector>

struct ihipStream_t;

namespace crt {

struct DynamicMesh {
    uint32_t vertStart = 0, nVerts = 0;
    bool hasNormals = false;
    bool identity = true; // transform bitwise equal to the identity: world data = rest data, no arithmetic
    float m[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 }; // row-major 3x4
    float nm[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };          // inverse transpose of its 3x3 (for normals), row-major
    bool dirty = false;   // rest data or transform changed since the last refit
};

struct DynamicScene {
    std::vector<DynamicMesh> meshes;
    uint32_t nVerts = 0, nTris = 0, nBinary = 0;
    void* dTable = nullptr;           // MeshEntry per mesh + terminator (mesh_table.hip.h)
    float* dRestXyz = nullptr;        // 3 floats per vertex, all meshes back to back
    float* dRestNormals = nullptr;    // idem (zeros for meshes without normals); NULL when no mesh has normals
    float* dWorldXyz = nullptr;
    float* dWorldNormals = nullptr;
    float* dPrevXyz = nullptr;        // crt_motion_snapshot: dWorldXyz as it was at the last snapshot (by vertex); NULL before the first
    uint32_t* dIdx = nullptr;         // 3 per triangle, mesh-local vertex indices
    uint32_t* dLevelNodes = nullptr;  // binary inner nodes by depth: level k = dLevelNodes[levelStart[k] .. levelStart[k + 1])
    std::vector<uint32_t> levelStart;
    void* dScratch = nullptr;         // collapseWideGpu scratch
    EventPair timer;                  // device_ms of a refit or a rebuild
    bool pending = false;             // some mesh is dirty

    DynamicScene() = default;
    DynamicScene(const DynamicScene&) = delete;
    DynamicScene& operator=(const DynamicScene&) = delete;
    ~DynamicScene();
};

// Everything a refit rewrites (all in HBM, capacities: nodes4 / nodes4q / planes hold one record per binary inner node)
struct RefitTargets {
    crt_bvh_node* binNodes;
    crt_bvh_tri* tris;
    crt_bvh_shade* shade;
    void* nodes4;
    void* nodes4q;
    float* planes;
};

// At upload: copies the meshes (rest = world = as given) and the per-level lists of the binary tree (hostNodes, or read back
// from binNodes when the tree exists on the device only).  Throws std::runtime_error on HIP errors.
void dynamicInit(DynamicScene& d, const crt_mesh_view* meshes, uint32_t n_meshes, const crt_bvh_node* hostNodes, const crt_bvh_node* binNodes,
                 uint32_t nBinary, ihipStream_t* stream);
// The refit of all pending updates, on `stream`; returns when it is done.  *nWide / *depth4: the re-collapsed wide tree;
// *device_ms: HIP-event time from the first transform to the plane table.  Throws std::runtime_error on HIP errors.
void dynamicRefit(DynamicScene& d, const RefitTargets& t, ihipStream_t* stream, uint32_t* nWide, uint32_t* depth4, double* device_ms);

// The rebuild (crt_rebuild; d.nTris > 0): the pending updates applied, then a new tree from the world vertices in HBM with the GPU
// builder `builder` (bvh_build.h kGpuBuilder*).  Returns the tree, its wide and quantised forms and the leaf-ordered records, all in
// HBM (for <= kLeafMax triangles the builders' one-leaf tree is made on the host and uploaded: uploadTree).  oldTris / oldUvs: the
// current leaf-ordered records; when oldUvs is set, the tree's uvs hold the uv records permuted to the new leaf order by gid.  The
// level lists and the collapse scratch follow the new tree.  Throws std::runtime_error on HIP errors.
DeviceTree dynamicRebuild(DynamicScene& d, int builder, const crt_bvh_tri* oldTris, const void* oldUvs, ihipStream_t* stream, double* device_ms);

} // namespace crt
