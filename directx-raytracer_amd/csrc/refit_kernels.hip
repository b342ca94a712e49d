// Refit of a dynamic scene (refit.h; DESIGN.md "Dynamic geometry"): moved vertices go into the tree uploaded with them, with the
// same bytes a fresh build of the moved meshes writes for every record whose place in the tree did not change.
//   1. transformKernel: world = transform . rest, one thread per vertex, for meshes whose transform is not the identity
//      (an identity mesh's world data is a copy of its rest data: no arithmetic, -0.0 stays -0.0)
//   2. recordsKernel: the leaf-ordered triangle / shading records from the world vertices, by triRecord / triNormals
//      (tri_geometry.hip.h), which the GPU build's gatherKernel calls too
//   3. refitLevelKernel: the binary boxes bottom-up, one launch per depth level, deepest first -- the kernel boundary is the
//      only synchronisation (no atomics, no hand-off between XCDs); a leaf's box from its triangles' triBox, as the GPU build's
//      triBoxKernel, an inner node's from grow(left, right) with minSel / maxSel, the selects of the oracle's aabb_grow
//   4. collapseWideGpu (bvh_gpu.hip, shared with the GPU build) and the plane table (launchDecodePlanes)
#include "refit.h"

#include "bvh_build.h"
#include "hip_own.h"
#include "render_kernels.h"
#include "tri_geometry.hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

namespace crt {
namespace {

struct Xform {
    float m[12];
    float nm[9];
};

// x' = ((m0*x + m1*y) + m2*z) + m3 per row (the file is built with -ffp-contract=off: no fused multiply-add); normals by the
// inverse transpose, no translation, not renormalised
__global__ __launch_bounds__(256) void transformKernel(const float* __restrict__ rest, const float* __restrict__ restN, float* __restrict__ world,
                                                       float* __restrict__ worldN, uint32_t n, Xform X)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float x = rest[3 * static_cast<size_t>(i)], y = rest[3 * static_cast<size_t>(i) + 1], z = rest[3 * static_cast<size_t>(i) + 2];
    for (int r = 0; r < 3; r++) world[3 * static_cast<size_t>(i) + r] = ((X.m[4 * r] * x + X.m[4 * r + 1] * y) + X.m[4 * r + 2] * z) + X.m[4 * r + 3];
    if (restN) {
        const float a = restN[3 * static_cast<size_t>(i)], b = restN[3 * static_cast<size_t>(i) + 1], c = restN[3 * static_cast<size_t>(i) + 2];
        for (int r = 0; r < 3; r++) worldN[3 * static_cast<size_t>(i) + r] = (X.nm[3 * r] * a + X.nm[3 * r + 1] * b) + X.nm[3 * r + 2] * c;
    }
}

// leaf position i: the record's gid names the triangle; v0 / e1 / e2 and the vertex normals rewritten in place (inst, prim, gid,
// the material and a mesh without normals' zeros stay)
__global__ __launch_bounds__(256) void recordsKernel(const MeshEntry* __restrict__ table, uint32_t n_meshes, const float* __restrict__ xyz,
                                                     const float* __restrict__ normals, const uint32_t* __restrict__ idx, uint32_t n,
                                                     crt_bvh_tri* __restrict__ tris, crt_bvh_shade* __restrict__ shade)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const TriFetch t = fetchTri(table, n_meshes, xyz, idx, tris[i].gid);
    triRecord(t, tris[i].v0, tris[i].e1, tris[i].e2);
    triNormals(t, normals, shade[i].n0, shade[i].n1, shade[i].n2);
}

// Every node of one depth level: both child boxes.  An inner child's box is the union of ITS two child boxes (written by the
// launch of the level below); a leaf's the union of its triangles' boxes in leaf order.  Both builders fold boxes with the same
// selects from +inf / -inf, and "a < b ? a : b" picks the last of equal values whichever way a fold is bracketed, so these are
// the builders' boxes bit for bit.  The empty leaf beside a one-leaf root takes its sibling's box, as the builders give it.
__global__ __launch_bounds__(256) void refitLevelKernel(const uint32_t* __restrict__ level, uint32_t count, crt_bvh_node* __restrict__ nodes,
                                                        const crt_bvh_tri* __restrict__ tris, const MeshEntry* __restrict__ table, uint32_t n_meshes,
                                                        const float* __restrict__ xyz, const uint32_t* __restrict__ idx)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    const uint32_t b = level[t];
    crt_bvh_node N = nodes[b];
    Box6 box[2];
    bool empty[2] = { false, false };
    for (int c = 0; c < 2; c++) {
        const int32_t ref = c == 0 ? N.left : N.right;
        Box6& B = box[c];
        if (ref >= 0) {
            const crt_bvh_node C = nodes[ref];
            B.mn[0] = minSel(C.lx0, C.rx0); B.mx[0] = maxSel(C.lx1, C.rx1);
            B.mn[1] = minSel(C.ly0, C.ry0); B.mx[1] = maxSel(C.ly1, C.ry1);
            B.mn[2] = minSel(C.lz0, C.rz0); B.mx[2] = maxSel(C.lz1, C.rz1);
            continue;
        }
        const uint32_t leaf = static_cast<uint32_t>(~ref), first = leaf >> 3, cnt = leaf & 7u;
        empty[c] = cnt == 0u;
        for (int a = 0; a < 3; a++) { B.mn[a] = INFINITY; B.mx[a] = -INFINITY; }
        for (uint32_t k = 0; k < cnt; k++) B = unionBox(B, triBox(fetchTri(table, n_meshes, xyz, idx, tris[first + k].gid)));
    }
    if (empty[1]) box[1] = box[0];
    else if (empty[0]) box[0] = box[1];
    N.lx0 = box[0].mn[0]; N.lx1 = box[0].mx[0]; N.ly0 = box[0].mn[1]; N.ly1 = box[0].mx[1]; N.lz0 = box[0].mn[2]; N.lz1 = box[0].mx[2];
    N.rx0 = box[1].mn[0]; N.rx1 = box[1].mx[0]; N.ry0 = box[1].mn[1]; N.ry1 = box[1].mx[1]; N.rz0 = box[1].mn[2]; N.rz1 = box[1].mx[2];
    nodes[b] = N;
}

// rebuild: the uv records follow their triangles -- scattered by gid from the old leaf order, gathered in the new one
__global__ __launch_bounds__(256) void uvScatterKernel(const crt_bvh_tri* __restrict__ tris, const crt_bvh_uv* __restrict__ uvs, uint32_t n,
                                                       crt_bvh_uv* __restrict__ byGid)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) byGid[tris[i].gid] = uvs[i];
}

__global__ __launch_bounds__(256) void uvGatherKernel(const crt_bvh_tri* __restrict__ tris, const crt_bvh_uv* __restrict__ byGid, uint32_t n,
                                                      crt_bvh_uv* __restrict__ uvs)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) uvs[i] = byGid[tris[i].gid];
}

} // namespace

// per-level lists of the binary inner nodes (the tree's shape changes only with a rebuild) and the collapse scratch for nBinary
// nodes (hostNodes, or read back from binNodes when the tree exists on the device only)
static void setLevels(DynamicScene& d, const crt_bvh_node* hostNodes, const crt_bvh_node* binNodes, uint32_t nBinary, ihipStream_t* stream)
{
    std::vector<crt_bvh_node> readBack;
    if (!hostNodes && nBinary) {
        readBack.resize(nBinary);
        HIP_THROW(hipMemcpyAsync(readBack.data(), binNodes, sizeof(crt_bvh_node) * nBinary, hipMemcpyDeviceToHost, stream));
        HIP_THROW(hipStreamSynchronize(stream));
        hostNodes = readBack.data();
    }
    std::vector<uint32_t> order;
    d.levelStart.clear();
    if (nBinary) {
        order.reserve(nBinary);
        order.push_back(0);
        size_t begin = 0;
        while (begin < order.size()) {
            const size_t end = order.size();
            d.levelStart.push_back(static_cast<uint32_t>(begin));
            for (size_t k = begin; k < end; k++) {
                const crt_bvh_node& N = hostNodes[order[k]];
                for (int32_t ch : { N.left, N.right })
                    if (ch >= 0) {
                        if (static_cast<uint32_t>(ch) >= nBinary || order.size() >= nBinary) throw std::runtime_error("binary tree: bad child reference");
                        order.push_back(static_cast<uint32_t>(ch));
                    }
            }
            begin = end;
        }
        d.levelStart.push_back(static_cast<uint32_t>(order.size()));
    }
    if (d.dLevelNodes) (void)hipFree(d.dLevelNodes);
    d.dLevelNodes = nullptr;
    if (d.dScratch) (void)hipFree(d.dScratch);
    d.dScratch = nullptr;
    d.nBinary = nBinary;
    HIP_THROW(hipMalloc(reinterpret_cast<void**>(&d.dLevelNodes), sizeof(uint32_t) * (order.empty() ? 1 : order.size())));
    if (!order.empty())
        HIP_THROW(hipMemcpyAsync(d.dLevelNodes, order.data(), sizeof(uint32_t) * order.size(), hipMemcpyHostToDevice, stream));
    HIP_THROW(hipMalloc(&d.dScratch, collapseScratchBytes(nBinary)));
    HIP_THROW(hipStreamSynchronize(stream)); // the host arrays above die with this call
}

// world = transform . rest for every dirty mesh (step 1 of the refit and of the rebuild)
static void applyTransforms(DynamicScene& d, ihipStream_t* stream)
{
    const dim3 blk(256);
    for (DynamicMesh& D : d.meshes) {
        if (!D.dirty || D.nVerts == 0) continue;
        const size_t off = 3 * static_cast<size_t>(D.vertStart), bytes = sizeof(float) * 3 * D.nVerts;
        if (D.identity) {
            HIP_THROW(hipMemcpyAsync(d.dWorldXyz + off, d.dRestXyz + off, bytes, hipMemcpyDeviceToDevice, stream));
            if (D.hasNormals) HIP_THROW(hipMemcpyAsync(d.dWorldNormals + off, d.dRestNormals + off, bytes, hipMemcpyDeviceToDevice, stream));
        } else {
            Xform X;
            std::memcpy(X.m, D.m, sizeof(X.m));
            std::memcpy(X.nm, D.nm, sizeof(X.nm));
            hipLaunchKernelGGL(transformKernel, dim3((D.nVerts + 255) / 256), blk, 0, stream, d.dRestXyz + off, D.hasNormals ? d.dRestNormals + off : nullptr,
                               d.dWorldXyz + off, D.hasNormals ? d.dWorldNormals + off : nullptr, D.nVerts, X);
        }
    }
}

DynamicScene::~DynamicScene()
{
    void* ptrs[] = { dTable, dRestXyz, dRestNormals, dWorldXyz, dWorldNormals, dPrevXyz, dIdx, dLevelNodes, dScratch };
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
}

void dynamicInit(DynamicScene& d, const crt_mesh_view* meshes, uint32_t n_meshes, const crt_bvh_node* hostNodes, const crt_bvh_node* binNodes,
                 uint32_t nBinary, ihipStream_t* stream)
{
    uint64_t nv = 0, nt = 0;
    bool anyNormals = false;
    d.meshes.resize(n_meshes);
    const std::vector<MeshEntry> table = makeMeshTable(meshes, n_meshes);
    for (uint32_t m = 0; m < n_meshes; m++) {
        DynamicMesh& D = d.meshes[m];
        D.vertStart = table[m].vertStart;
        D.nVerts = meshes[m].n_vertices;
        D.hasNormals = meshes[m].normals != nullptr;
        anyNormals |= D.hasNormals && D.nVerts > 0;
        nv += meshes[m].n_vertices;
        nt += meshes[m].n_triangles;
    }
    if (nv >= (1ull << 32)) throw std::runtime_error("too many vertices");
    d.nVerts = static_cast<uint32_t>(nv);
    d.nTris = static_cast<uint32_t>(nt);
    const size_t vb = sizeof(float) * 3 * (nv ? nv : 1);
    HIP_THROW(hipMalloc(&d.dTable, sizeof(MeshEntry) * table.size()));
    HIP_THROW(hipMalloc(reinterpret_cast<void**>(&d.dRestXyz), vb));
    HIP_THROW(hipMalloc(reinterpret_cast<void**>(&d.dWorldXyz), vb));
    if (anyNormals) {
        HIP_THROW(hipMalloc(reinterpret_cast<void**>(&d.dRestNormals), vb));
        HIP_THROW(hipMalloc(reinterpret_cast<void**>(&d.dWorldNormals), vb));
        HIP_THROW(hipMemsetAsync(d.dRestNormals, 0, vb, stream));
    }
    HIP_THROW(hipMalloc(reinterpret_cast<void**>(&d.dIdx), sizeof(uint32_t) * 3 * (nt ? nt : 1)));
    HIP_THROW(hipMemcpyAsync(d.dTable, table.data(), sizeof(MeshEntry) * table.size(), hipMemcpyHostToDevice, stream));
    for (uint32_t m = 0; m < n_meshes; m++) {
        const crt_mesh_view& M = meshes[m];
        const size_t off = 3 * static_cast<size_t>(table[m].vertStart);
        if (M.n_vertices && M.xyz) HIP_THROW(hipMemcpyAsync(d.dRestXyz + off, M.xyz, sizeof(float) * 3 * M.n_vertices, hipMemcpyHostToDevice, stream));
        if (M.n_vertices && M.normals)
            HIP_THROW(hipMemcpyAsync(d.dRestNormals + off, M.normals, sizeof(float) * 3 * M.n_vertices, hipMemcpyHostToDevice, stream));
        if (M.n_triangles)
            HIP_THROW(hipMemcpyAsync(d.dIdx + 3 * static_cast<size_t>(table[m].triStart), M.idx, sizeof(uint32_t) * 3 * static_cast<size_t>(M.n_triangles),
                                     hipMemcpyHostToDevice, stream));
    }
    HIP_THROW(hipMemcpyAsync(d.dWorldXyz, d.dRestXyz, vb, hipMemcpyDeviceToDevice, stream));
    if (anyNormals) HIP_THROW(hipMemcpyAsync(d.dWorldNormals, d.dRestNormals, vb, hipMemcpyDeviceToDevice, stream));

    setLevels(d, hostNodes, binNodes, nBinary, stream);
    HIP_THROW(hipStreamSynchronize(stream)); // the host arrays above die with this call
}

void dynamicRefit(DynamicScene& d, const RefitTargets& t, ihipStream_t* stream, uint32_t* nWide, uint32_t* depth4, double* device_ms)
{
    const dim3 blk(256);
    d.timer.start(stream);
    applyTransforms(d, stream);
    const uint32_t nMeshes = static_cast<uint32_t>(d.meshes.size());
    const MeshEntry* table = static_cast<const MeshEntry*>(d.dTable);
    if (d.nTris)
        hipLaunchKernelGGL(recordsKernel, dim3((d.nTris + 255) / 256), blk, 0, stream, table, nMeshes, d.dWorldXyz, d.dWorldNormals, d.dIdx, d.nTris,
                           t.tris, t.shade);
    for (size_t L = d.levelStart.size() - (d.levelStart.empty() ? 0 : 1); L-- > 0;) {
        const uint32_t first = d.levelStart[L], count = d.levelStart[L + 1] - first;
        hipLaunchKernelGGL(refitLevelKernel, dim3((count + 255) / 256), blk, 0, stream, d.dLevelNodes + first, count, t.binNodes, t.tris, table,
                           nMeshes, d.dWorldXyz, d.dIdx);
    }
    HIP_THROW(hipGetLastError());
    *nWide = 0;
    *depth4 = 0;
    if (d.nBinary) {
        collapseWideGpu(t.binNodes, d.nBinary, d.dScratch, t.nodes4, t.nodes4q, nullptr, stream, nWide, depth4, nullptr);
        HIP_THROW(static_cast<hipError_t>(launchDecodePlanes(t.nodes4q, *nWide, t.planes, stream)));
    }
    const double ms = d.timer.stopAndWait(stream);
    if (device_ms) *device_ms = ms;
    for (DynamicMesh& D : d.meshes) D.dirty = false;
    d.pending = false;
}

} // namespace crt

namespace crt {

DeviceTree dynamicRebuild(DynamicScene& d, int builder, const crt_bvh_tri* oldTris, const void* oldUvs, ihipStream_t* stream, double* device_ms)
{
    DeviceTree out;
    if (device_ms) *device_ms = 0.0;
    if (d.nTris == 0) throw std::logic_error("dynamicRebuild: a scene without triangles");
    d.timer.start(stream);
    applyTransforms(d, stream);
    const uint32_t nMeshes = static_cast<uint32_t>(d.meshes.size());
    if (d.nTris > static_cast<uint32_t>(kLeafMax)) {
        GpuMeshes in;
        in.table = d.dTable;
        in.nMeshes = nMeshes;
        in.n = d.nTris;
        in.xyz = d.dWorldXyz;
        in.idx = d.dIdx;
        in.normals = d.dWorldNormals;
        out = rebuildBvhGpu(in, builder, stream, nullptr);
    } else {
        // a handful of triangles: the builders' one-leaf tree is made on the host (bvh_gpu.hip), from the world vertices read back
        std::vector<MeshEntry> table(nMeshes + 1u);
        std::vector<float> xyz(3 * static_cast<size_t>(d.nVerts)), nrm(d.dWorldNormals ? 3 * static_cast<size_t>(d.nVerts) : 0);
        std::vector<uint32_t> idx(3 * static_cast<size_t>(d.nTris));
        HIP_THROW(hipMemcpyAsync(table.data(), d.dTable, sizeof(MeshEntry) * table.size(), hipMemcpyDeviceToHost, stream));
        if (!xyz.empty()) HIP_THROW(hipMemcpyAsync(xyz.data(), d.dWorldXyz, sizeof(float) * xyz.size(), hipMemcpyDeviceToHost, stream));
        if (!nrm.empty()) HIP_THROW(hipMemcpyAsync(nrm.data(), d.dWorldNormals, sizeof(float) * nrm.size(), hipMemcpyDeviceToHost, stream));
        HIP_THROW(hipMemcpyAsync(idx.data(), d.dIdx, sizeof(uint32_t) * idx.size(), hipMemcpyDeviceToHost, stream));
        HIP_THROW(hipStreamSynchronize(stream));
        std::vector<crt_mesh_view> views(nMeshes);
        for (uint32_t m = 0; m < nMeshes; m++) {
            const MeshEntry& E = table[m];
            crt_mesh_view& V = views[m];
            std::memset(&V, 0, sizeof(V));
            V.n_vertices = E.nVerts;
            V.n_triangles = table[m + 1].triStart - E.triStart;
            V.xyz = E.nVerts ? xyz.data() + 3 * static_cast<size_t>(E.vertStart) : nullptr;
            V.idx = V.n_triangles ? idx.data() + 3 * static_cast<size_t>(E.triStart) : nullptr;
            V.normals = E.hasNormals && E.nVerts ? nrm.data() + 3 * static_cast<size_t>(E.vertStart) : nullptr;
            V.material_index = static_cast<int32_t>(E.material);
        }
        Bvh host;
        buildBvhGpu(views.data(), nMeshes, host, stream, nullptr, builder);
        out = uploadTree(host, true);
    }
    if (oldUvs) {
        const dim3 blk(256), grd((d.nTris + 255) / 256);
        DeviceBuffer byGid(sizeof(crt_bvh_uv) * d.nTris);
        out.uvs = DeviceBuffer(recordBytes(sizeof(crt_bvh_uv), d.nTris));
        hipLaunchKernelGGL(uvScatterKernel, grd, blk, 0, stream, oldTris, static_cast<const crt_bvh_uv*>(oldUvs), d.nTris, byGid.as<crt_bvh_uv>());
        hipLaunchKernelGGL(uvGatherKernel, grd, blk, 0, stream, out.tris.as<const crt_bvh_tri>(), byGid.as<const crt_bvh_uv>(), d.nTris,
                           out.uvs.as<crt_bvh_uv>());
        HIP_THROW(hipGetLastError());
        HIP_THROW(hipStreamSynchronize(stream)); // byGid dies with this scope
    }
    const double ms = d.timer.stopAndWait(stream);
    if (device_ms) *device_ms = ms;
    setLevels(d, nullptr, out.nodes.as<const crt_bvh_node>(), out.nNodes, stream);
    for (DynamicMesh& D : d.meshes) D.dirty = false;
    d.pending = false;
    return out;
}

} // namespace crt
