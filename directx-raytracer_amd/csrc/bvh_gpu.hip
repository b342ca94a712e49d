// GPU BVH build: stands in for BuildRaytracingAccelerationStructure, which the reference
// runs on the GPU at init (R/DXRTRenderer.cpp:548-806).  LBVH: 30-bit Morton codes of the quantised box centroids,
// radix sort, Karras 2012 hierarchy, bottom-up exact box fitting, ranges of <= 2 triangles collapsed to leaves, then --
// still on the device -- the collapse to the 4-wide tree (level by level, bvh_wide.h wideSlots) and its quantisation.
// Specification = oracle/crt_oracle.c build_lbvh(); the two produce byte-identical trees (tests/test_gpu_parity.py).
// The meshes go up as they are (vertices, indices, normals, uvs: 18 MB for 1M triangles instead of 130 MB of flattened
// records); triangle boxes, the leaf-ordered triangle / shading / uv records, the binary nodes, the wide nodes and their
// quantised form are produced on the device and STAY there (the context adopts the buffers; crt_bvh_export* read them back
// on demand).  Nothing but a few counters comes back to the host.
// Cubic Morton cells and leaves of at most 2 triangles (per-axis scaling and the SAH builder's 4-triangle leaves measured +36 %
// node fetches and +94 % triangle tests against the SAH tree on the 1M-triangle frame; now +18 % / -13 %).  It is the fast
// option (option "gpu_build": 8.7 ms against 360 ms at 1M triangles), not the default.
// Option "gpu_builder" = 1 swaps the Karras hierarchy for PLOC (bvh_ploc.hip) on the same sorted keys; buildFromDevice holds
// both and starts from meshes already in HBM, so the rebuild of a dynamic scene (crt_rebuild) runs the same code as an upload.
#include "bvh_build.h"
#include "bvh_wide.h"
#include "hip_own.h"
#include "render_kernels.h"
#include "tri_geometry.hip.h"

#include <hip/hip_runtime.h>
#include "gpu_sort.hip.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>

namespace crt {
namespace {

struct KNode { // Karras internal node
    int left, right;   // >= 0 internal index, < 0: ~sorted leaf position
    uint32_t lo, hi;   // range of sorted positions covered
};

// float <-> int such that signed int order == float order (for atomicMin/atomicMax on floats)
__device__ __forceinline__ int orderedInt(float f)
{
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float fromOrderedInt(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }

__global__ void initBoundsKernel(int* bounds)
{
    if (threadIdx.x < 3) bounds[threadIdx.x] = INT_MAX;      // min
    else if (threadIdx.x < 6) bounds[threadIdx.x] = INT_MIN; // max
}

// centroid bounds: a fixed grid strides over the centroids, wave reduction, one atomic pair per wavefront and axis
// (one wavefront per 64 centroids meant 94 k atomics on the same six words at 1M triangles: 1.1 ms, most of it queueing)
constexpr uint32_t kBoundsBlocks = 256;
__global__ __launch_bounds__(256) void boundsKernel(const float* __restrict__ cent, uint32_t n, int* bounds)
{
    int mn[3] = { INT_MAX, INT_MAX, INT_MAX }, mx[3] = { INT_MIN, INT_MIN, INT_MIN };
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += kBoundsBlocks * 256u)
        for (int a = 0; a < 3; a++) {
            const int v = orderedInt(cent[3 * static_cast<size_t>(i) + a]);
            mn[a] = min(mn[a], v);
            mx[a] = max(mx[a], v);
        }
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; a++) {
            mn[a] = min(mn[a], __shfl_xor(mn[a], off, 64));
            mx[a] = max(mx[a], __shfl_xor(mx[a], off, 64));
        }
    if ((threadIdx.x & 63u) == 0)
        for (int a = 0; a < 3; a++) {
            atomicMin(&bounds[a], mn[a]);
            atomicMax(&bounds[3 + a], mx[a]);
        }
}

__global__ __launch_bounds__(256) void mortonKernel(const float* __restrict__ cent, uint32_t n, const int* __restrict__ bounds,
                                                    unsigned long long* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t q[3];
    float extm = 0.0f; // one cell size for all three axes (that of the longest extent): cubic cells
    for (int a = 0; a < 3; a++) {
        const float ext = fromOrderedInt(bounds[3 + a]) - fromOrderedInt(bounds[a]);
        if (ext > extm) extm = ext;
    }
    const float scale = mortonScale(extm);
    for (int a = 0; a < 3; a++) q[a] = quant10((cent[3 * static_cast<size_t>(i) + a] - fromOrderedInt(bounds[a])) * scale);
    const uint32_t code = (expandBits10(q[0]) << 2) | (expandBits10(q[1]) << 1) | expandBits10(q[2]);
    keys[i] = (static_cast<unsigned long long>(code) << 32) | i;
}

__device__ __forceinline__ int delta64(const unsigned long long* __restrict__ keys, long long n, long long i, long long j)
{
    if (j < 0 || j >= n) return -1;
    return __clzll(static_cast<long long>(keys[i] ^ keys[j]));
}

// Karras 2012, one thread per internal node
__global__ __launch_bounds__(256) void hierarchyKernel(const unsigned long long* __restrict__ keys, uint32_t n, KNode* __restrict__ K,
                                                       int* __restrict__ parentOfInternal, int* __restrict__ parentOfLeaf)
{
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const long long N = n;
    if (i >= N - 1) return;
    const int d = (delta64(keys, N, i, i + 1) - delta64(keys, N, i, i - 1)) < 0 ? -1 : 1;
    const int dmin = delta64(keys, N, i, i - d);
    long long lmax = 2;
    while (delta64(keys, N, i, i + lmax * d) > dmin) lmax *= 2;
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (delta64(keys, N, i, i + (l + t) * d) > dmin) l += t;
    const long long j = i + l * d;
    const int dnode = delta64(keys, N, i, j);
    long long sp = 0;
    for (long long t = (l + 1) / 2;; t = (t + 1) / 2) {
        if (delta64(keys, N, i, i + (sp + t) * d) > dnode) sp += t;
        if (t == 1) break;
    }
    const long long gamma = i + sp * d + (d < 0 ? -1 : 0);
    const long long lo = i < j ? i : j, hi = i < j ? j : i;
    KNode k;
    k.lo = static_cast<uint32_t>(lo);
    k.hi = static_cast<uint32_t>(hi);
    if (lo == gamma) { k.left = ~static_cast<int>(gamma); parentOfLeaf[gamma] = static_cast<int>(i); }
    else { k.left = static_cast<int>(gamma); parentOfInternal[gamma] = static_cast<int>(i); }
    if (hi == gamma + 1) { k.right = ~static_cast<int>(gamma + 1); parentOfLeaf[gamma + 1] = static_cast<int>(i); }
    else { k.right = static_cast<int>(gamma + 1); parentOfInternal[gamma + 1] = static_cast<int>(i); }
    K[i] = k;
    if (i == 0) parentOfInternal[0] = -1;
}

// bottom-up exact boxes: the second thread to arrive at a node unions its children and moves on.  A node whose triangle
// range lies inside the 256 leaves of one workgroup is only ever touched by that workgroup: arrival counter and fences at
// workgroup scope, which cost nothing.  A node spanning workgroups hands boxes between XCDs through memory, so those hops
// are fenced at agent scope on both sides (MI355X: per-XCD L2s are not coherent; cdna_hip_programming.md Guideline 16) --
// an agent-scope fence per hop for EVERY node was 6.4 of the build's 8.9 ms of kernel time at 1M triangles.
__global__ __launch_bounds__(256) void fitKernel(const KNode* __restrict__ K, const Box6* __restrict__ pbox, const unsigned long long* __restrict__ keys,
                                                 uint32_t n, const int* __restrict__ parentOfInternal, const int* __restrict__ parentOfLeaf,
                                                 Box6* nodeBox, unsigned int* flags)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t blockLo = blockIdx.x * 256u, blockHi = blockLo + 255u;
    int p = parentOfLeaf[i];
    while (p >= 0) {
        const KNode k = K[p];
        unsigned int earlier;
        if ((k.lo >= blockLo) & (k.hi <= blockHi)) {
            // release what this thread wrote below, announce arrival, acquire the sibling's boxes: all inside the workgroup
            earlier = __hip_atomic_fetch_add(&flags[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            earlier = __hip_atomic_fetch_add(&flags[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (earlier == 0u) return; // first arrival: the sibling subtree is not finished yet
        Box6 b;
        for (int c = 0; c < 2; c++) {
            const int ref = c == 0 ? k.left : k.right;
            Box6 cb;
            if (ref < 0) cb = pbox[static_cast<uint32_t>(keys[~ref] & 0xFFFFFFFFull)];
            else {
                const volatile Box6* src = nodeBox + ref; // written by another thread during this launch: do not cache in registers early
                for (int a = 0; a < 3; a++) { cb.mn[a] = src->mn[a]; cb.mx[a] = src->mx[a]; }
            }
            if (c == 0) b = cb;
            else b = unionBox(b, cb); // same selects as the oracle's aabb_grow(l, r)
        }
        // write-through stores: an agent-scope release writes this XCD's dirty L2 lines back, and it is far cheaper when
        // the 24 MB of boxes this kernel produces are not sitting there dirty
        for (int a = 0; a < 3; a++) {
            __hip_atomic_store(&nodeBox[p].mn[a], b.mn[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&nodeBox[p].mx[a], b.mx[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        p = parentOfInternal[p];
    }
}

__global__ __launch_bounds__(256) void keptKernel(const KNode* __restrict__ K, uint32_t nInternal, uint32_t* __restrict__ kept)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nInternal) kept[i] = (K[i].hi - K[i].lo + 1u > static_cast<uint32_t>(kLbvhLeafMax)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void emitKernel(const KNode* __restrict__ K, const uint32_t* __restrict__ kept, const uint32_t* __restrict__ rank,
                                                  const Box6* __restrict__ nodeBox, const Box6* __restrict__ pbox,
                                                  const unsigned long long* __restrict__ keys, uint32_t nInternal, crt_bvh_node* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nInternal || !kept[i]) return;
    const KNode k = K[i];
    Box6 b[2];
    int ref[2];
    for (int c = 0; c < 2; c++) {
        const int ch = c == 0 ? k.left : k.right;
        if (ch < 0) {
            b[c] = pbox[static_cast<uint32_t>(keys[~ch] & 0xFFFFFFFFull)];
            ref[c] = leafRef(static_cast<uint32_t>(~ch), 1u);
        } else {
            b[c] = nodeBox[ch];
            const uint32_t cnt = K[ch].hi - K[ch].lo + 1u;
            ref[c] = cnt <= static_cast<uint32_t>(kLbvhLeafMax) ? leafRef(K[ch].lo, cnt) : static_cast<int>(rank[ch]);
        }
    }
    crt_bvh_node N;
    N.lx0 = b[0].mn[0]; N.lx1 = b[0].mx[0]; N.ly0 = b[0].mn[1]; N.ly1 = b[0].mx[1]; N.lz0 = b[0].mn[2]; N.lz1 = b[0].mx[2];
    N.rx0 = b[1].mn[0]; N.rx1 = b[1].mx[0]; N.ry0 = b[1].mn[1]; N.ry1 = b[1].mx[1]; N.rz0 = b[1].mn[2]; N.rz1 = b[1].mx[2];
    N.left = ref[0]; N.right = ref[1]; N.pad0 = 0; N.pad1 = 0;
    out[rank[i]] = N;
}

// per input triangle (global ordinal g): bounds and centroid, exactly as flattenMeshes computes them on the host
__global__ __launch_bounds__(256) void triBoxKernel(const MeshEntry* __restrict__ table, uint32_t n_meshes, const float* __restrict__ xyz,
                                                    const uint32_t* __restrict__ idx, uint32_t n, Box6* __restrict__ box, float* __restrict__ cent,
                                                    int* __restrict__ badIndex)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    const TriFetch t = fetchTri<true>(table, n_meshes, xyz, idx, g);
    if (!t.inRange) *badIndex = 1; // (the build throws; the triangle counts as inert until then)
    const Box6 b = triBox(t);
    for (int k = 0; k < 3; k++) cent[3 * static_cast<size_t>(g) + k] = (b.mn[k] + b.mx[k]) * 0.5f;
    box[g] = b;
}

// leaf position i <- input triangle keys[i] & 0xFFFFFFFF: the 48-byte triangle record, the shading record and (when any
// mesh has them) the uv record, written straight from the mesh arrays
__global__ __launch_bounds__(256) void gatherKernel(const unsigned long long* __restrict__ keys, uint32_t n, const MeshEntry* __restrict__ table,
                                                    uint32_t n_meshes, const float* __restrict__ xyz, const uint32_t* __restrict__ idx,
                                                    const float* __restrict__ normals, const float* __restrict__ uvsIn, crt_bvh_tri* __restrict__ tris,
                                                    crt_bvh_shade* __restrict__ shade, crt_bvh_uv* __restrict__ uvs)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = static_cast<uint32_t>(keys[i] & 0xFFFFFFFFull);
    const TriFetch t = fetchTri(table, n_meshes, xyz, idx, g);
    crt_bvh_tri T;
    triRecord(t, T.v0, T.e1, T.e2);
    T.inst = t.mesh;
    T.prim = g - t.M.triStart;
    T.gid = g;
    tris[i] = T;
    crt_bvh_shade S;
    for (int k = 0; k < 3; k++) { S.n0[k] = 0.0f; S.n1[k] = 0.0f; S.n2[k] = 0.0f; }
    S.material = t.M.material;
    S.pad[0] = 0; S.pad[1] = 0;
    triNormals(t, normals, S.n0, S.n1, S.n2);
    shade[i] = S;
    if (uvs) {
        crt_bvh_uv U;
        U.uv0[0] = U.uv0[1] = U.uv1[0] = U.uv1[1] = U.uv2[0] = U.uv2[1] = 0.0f;
        if (t.M.hasUvs) {
            U.uv0[0] = uvsIn[3 * static_cast<size_t>(t.v[0])]; U.uv0[1] = uvsIn[3 * static_cast<size_t>(t.v[0]) + 1];
            U.uv1[0] = uvsIn[3 * static_cast<size_t>(t.v[1])]; U.uv1[1] = uvsIn[3 * static_cast<size_t>(t.v[1]) + 1];
            U.uv2[0] = uvsIn[3 * static_cast<size_t>(t.v[2])]; U.uv2[1] = uvsIn[3 * static_cast<size_t>(t.v[2]) + 1];
        }
        uvs[i] = U;
    }
}

// ---- binary -> 4-wide collapse + quantisation on the device (the rules: bvh_wide.h; the host routine collapseBvh4 gives the
// same bytes).  Level by level from the root: every wide node of the level absorbs its binary nodes (wideSlots) and reserves
// places for its inner children in the next level (one atomic per wavefront: a wave prefix sum inside).  The result must be
// numbered in DFS pre-order like the host's: subtree sizes bottom-up, then ids top-down (id of child k = id of the parent
// + 1 + sizes of the children before it), then every node is written -- full precision and quantised -- at its id.
struct WideTmp {
    crt_bvh_node4 W;     // inner refs = binary indices
    uint32_t child[4];   // temporary index (level order) of the inner children, ~0u for leaf / empty slots
};

__device__ __forceinline__ uint32_t waveExclusiveSum(uint32_t v, uint32_t& total)
{
    uint32_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if ((threadIdx.x & 63u) >= static_cast<uint32_t>(off)) incl += up;
    }
    total = __shfl(incl, 63, 64);
    return incl - v;
}

__global__ __launch_bounds__(256) void wideExpandKernel(const crt_bvh_node* __restrict__ nodes, const uint32_t* __restrict__ frontier /* {binary, depth} pairs */,
                                                        uint32_t count, uint32_t base, uint32_t nextBase, WideTmp* __restrict__ tmp,
                                                        uint32_t* __restrict__ nextFrontier, uint32_t* __restrict__ nextCount, uint32_t* __restrict__ maxDepth)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t inner = 0;
    WideSlot sl[4];
    int n = 0;
    if (i < count) {
        uint32_t deep = 0;
        n = wideSlots(nodes, static_cast<int32_t>(frontier[2u * i]), frontier[2u * i + 1u], sl, &deep);
        atomicMax(maxDepth, deep);
        for (int k = 0; k < n; k++) inner += sl[k].ref >= 0 ? 1u : 0u;
    }
    uint32_t total = 0;
    const uint32_t before = waveExclusiveSum(inner, total);
    uint32_t waveBase = 0;
    if ((threadIdx.x & 63u) == 0u && total) waveBase = atomicAdd(nextCount, total);
    waveBase = __shfl(waveBase, 0, 64);
    if (i >= count) return;
    WideTmp& T = tmp[base + i];
    fillWide(sl, n, T.W);
    uint32_t at = waveBase + before;
    for (int k = 0; k < 4; k++) {
        T.child[k] = ~0u;
        if (k < n && sl[k].ref >= 0) {
            nextFrontier[2u * at] = static_cast<uint32_t>(sl[k].ref);
            nextFrontier[2u * at + 1u] = sl[k].depth;
            T.child[k] = nextBase + at;
            at++;
        }
    }
}

__global__ __launch_bounds__(256) void wideSizeKernel(const WideTmp* __restrict__ tmp, uint32_t base, uint32_t count, uint32_t* __restrict__ size)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const WideTmp& T = tmp[base + i];
    uint32_t s = 1;
    for (int k = 0; k < 4; k++)
        if (T.child[k] != ~0u) s += size[T.child[k]];
    size[base + i] = s;
}

__global__ __launch_bounds__(256) void wideIdKernel(const WideTmp* __restrict__ tmp, uint32_t base, uint32_t count, const uint32_t* __restrict__ size,
                                                    uint32_t* __restrict__ id)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const WideTmp& T = tmp[base + i];
    uint32_t run = id[base + i] + 1u; // (the root's id is set to 0 by the host)
    for (int k = 0; k < 4; k++)
        if (T.child[k] != ~0u) {
            id[T.child[k]] = run;
            run += size[T.child[k]];
        }
}

__global__ __launch_bounds__(256) void wideEmitKernel(const WideTmp* __restrict__ tmp, uint32_t total, const uint32_t* __restrict__ id,
                                                      crt_bvh_node4* __restrict__ nodes4, crt_bvh_node4q* __restrict__ nodes4q)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total) return;
    crt_bvh_node4 W = tmp[t].W;
    for (int k = 0; k < 4; k++)
        if (tmp[t].child[k] != ~0u) W.ref[k] = static_cast<int32_t>(id[tmp[t].child[k]]);
    nodes4[id[t]] = W;
    crt_bvh_node4q Q;
    quantizeNode4(W, Q);
    nodes4q[id[t]] = Q;
}

// the decoded plane table (render_kernels.h, kPlaneStride): one thread per float of it.  Plane byte k of a record (qlo_x ..
// qhi_z, child j = byte j of each little-endian word) is float k of its row; the row's last 8 floats are zero.
__global__ __launch_bounds__(256) void decodePlanesKernel(const unsigned char* __restrict__ nodes, uint32_t n, float* __restrict__ planes)
{
    const size_t t = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= static_cast<size_t>(n) * kPlaneStride) return;
    const size_t node = t / kPlaneStride;
    const uint32_t k = static_cast<uint32_t>(t % kPlaneStride);
    planes[t] = k < 24u ? static_cast<float>(nodes[node * sizeof(crt_bvh_node4q) + offsetof(crt_bvh_node4q, qlo_x) + k]) : 0.0f;
}

} // namespace

size_t collapseScratchBytes(uint32_t nBinary)
{
    const size_t n = nBinary ? nBinary : 1u;
    return sizeof(WideTmp) * n + sizeof(uint32_t) * (2 * n + 4 * n + 4); // tmp, size + id, two frontiers, scalars
}

// Binary -> 4-wide collapse + quantisation of the nBinary nodes at `nodes` (the rules: bvh_wide.h).  Scratch: collapseScratchBytes.
// nodes4 / nodes4q: buffers of at least nBinary records (a wide node absorbs one binary node at least); or, with `fresh` set, they
// are ignored and fresh->nodes4 / nodes4q are allocated here for exactly the wide node count and written instead.
// Synchronises the stream once per wide level (the next level's count decides the next launch).
void collapseWideGpu(const crt_bvh_node* nodes, uint32_t nBinary, void* scratch, void* nodes4, void* nodes4q, DeviceTree* fresh,
                     ihipStream_t* stream, uint32_t* nWideOut, uint32_t* depth4Out, uint32_t* maxDepthOut)
{
    const size_t n = nBinary ? nBinary : 1u;
    WideTmp* dTmp = static_cast<WideTmp*>(scratch);
    uint32_t* dSize = reinterpret_cast<uint32_t*>(dTmp + n);
    uint32_t* dId = dSize + n;
    uint32_t* dFrontA = dId + n;
    uint32_t* dFrontB = dFrontA + 2 * n;
    uint32_t* dScalars = dFrontB + 2 * n; // [0] next count, [1] max depth
    const dim3 blk(256);
    std::vector<std::pair<uint32_t, uint32_t>> levels; // {first temporary index, count}
    {
        const uint32_t rootEntry[2] = { 0u, 0u };
        HIP_THROW(hipMemcpyAsync(dFrontA, rootEntry, sizeof(rootEntry), hipMemcpyHostToDevice, stream));
        HIP_THROW(hipMemsetAsync(dScalars, 0, sizeof(uint32_t) * 2, stream));
        uint32_t base = 0, count = 1;
        uint32_t* cur = dFrontA;
        uint32_t* nxt = dFrontB;
        while (count) {
            if (static_cast<uint64_t>(base) + count > nBinary) throw std::runtime_error("wide collapse: more wide nodes than binary nodes");
            levels.emplace_back(base, count);
            HIP_THROW(hipMemsetAsync(dScalars, 0, sizeof(uint32_t), stream));
            hipLaunchKernelGGL(wideExpandKernel, dim3((count + 255) / 256), blk, 0, stream, nodes, cur, count, base, base + count, dTmp, nxt,
                               dScalars, dScalars + 1);
            HIP_THROW(hipGetLastError());
            uint32_t nextCount = 0;
            HIP_THROW(hipMemcpyAsync(&nextCount, dScalars, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            HIP_THROW(hipStreamSynchronize(stream));
            base += count;
            count = nextCount;
            std::swap(cur, nxt);
        }
    }
    const uint32_t nWide = levels.back().first + levels.back().second;
    for (size_t L = levels.size(); L-- > 0;)
        hipLaunchKernelGGL(wideSizeKernel, dim3((levels[L].second + 255) / 256), blk, 0, stream, dTmp, levels[L].first, levels[L].second, dSize);
    HIP_THROW(hipMemsetAsync(dId, 0, sizeof(uint32_t), stream)); // the root's id
    for (size_t L = 0; L < levels.size(); L++)
        hipLaunchKernelGGL(wideIdKernel, dim3((levels[L].second + 255) / 256), blk, 0, stream, dTmp, levels[L].first, levels[L].second, dSize, dId);
    HIP_THROW(hipGetLastError());
    if (fresh) {
        fresh->nodes4 = DeviceBuffer(sizeof(crt_bvh_node4) * nWide);
        fresh->nodes4q = DeviceBuffer(quantisedBytes(nWide));
        nodes4 = fresh->nodes4.as<>();
        nodes4q = fresh->nodes4q.as<>();
    }
    hipLaunchKernelGGL(wideEmitKernel, dim3((nWide + 255) / 256), blk, 0, stream, dTmp, nWide, dId, static_cast<crt_bvh_node4*>(nodes4),
                       static_cast<crt_bvh_node4q*>(nodes4q));
    HIP_THROW(hipGetLastError());
    uint32_t maxDepth = 0;
    HIP_THROW(hipMemcpyAsync(&maxDepth, dScalars + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_THROW(hipStreamSynchronize(stream));
    *nWideOut = nWide;
    *depth4Out = static_cast<uint32_t>(levels.size());
    if (maxDepthOut) *maxDepthOut = maxDepth;
}

namespace {

// Morton order, the builder's binary tree, the leaf-ordered records and the wide tree, from meshes already in HBM (n > kLeafMax)
DeviceTree buildFromDevice(const GpuMeshes& in, int builder, ihipStream_t* stream, double* device_ms, const std::function<void(const char*)>& lap)
{
    const bool timing = std::getenv("CRT_BUILD_TIMING") != nullptr;
    const uint32_t n = in.n, n_meshes = in.nMeshes, nInternal = n - 1;
    const MeshEntry* table = static_cast<const MeshEntry*>(in.table);
    DeviceTree out;
    DeviceBuffer dBad(sizeof(int));
    DeviceBuffer dBox(sizeof(Box6) * n), dCent(sizeof(float) * 3 * n), dBounds(sizeof(int) * 6);
    DeviceBuffer dKeysIn(sizeof(unsigned long long) * n), dKeys(sizeof(unsigned long long) * n);
    // the leaf-ordered records stay in HBM: whoever takes the tree copies them out only if someone asks
    out.tris = DeviceBuffer(recordBytes(sizeof(crt_bvh_tri), n));
    out.shade = DeviceBuffer(recordBytes(sizeof(crt_bvh_shade), n));
    if (in.uvsIn) out.uvs = DeviceBuffer(recordBytes(sizeof(crt_bvh_uv), n));
    // scratch of the sort (digit counts per tile) and of the scan (tile sums); both written by this file's own kernels (gpu_sort.hip.h)
    DeviceBuffer dSortCounts(sizeof(uint32_t) * gpusort::sortScratchWords(n)), dScanSums(gpusort::scanScratchBytes(nInternal));
    HIP_THROW(hipMemsetAsync(dBad.as<>(), 0, sizeof(int), stream));

    EventPair timer;
    timer.start(stream);
    const dim3 blk(256), grdN((n + 255) / 256), grdI((nInternal + 255) / 256);
    hipLaunchKernelGGL(triBoxKernel, grdN, blk, 0, stream, table, n_meshes, in.xyz, in.idx, n, dBox.as<Box6>(), dCent.as<float>(), dBad.as<int>());
    hipLaunchKernelGGL(initBoundsKernel, dim3(1), dim3(64), 0, stream, dBounds.as<int>());
    hipLaunchKernelGGL(boundsKernel, dim3(kBoundsBlocks), blk, 0, stream, dCent.as<float>(), n, dBounds.as<int>());
    // keys = Morton code << 32 | ordinal, written in ordinal order: a stable sort on the four bytes of the high dword orders the full keys;
    // four passes ping-pong dKeys -> dKeysIn -> ... and end in dKeys
    hipLaunchKernelGGL(mortonKernel, grdN, blk, 0, stream, dCent.as<float>(), n, dBounds.as<int>(), dKeys.as<unsigned long long>());
    HIP_THROW(hipGetLastError()); // triBox / bounds / Morton launches
    hipError_t sortStatus = hipSuccess;
    unsigned long long* sorted = gpusort::sortKeysHigh(dKeys.as<unsigned long long>(), dKeysIn.as<unsigned long long>(), n, 4, dSortCounts.as<uint32_t>(), stream, &sortStatus);
    HIP_THROW(sortStatus);
    if (sorted != dKeys.as<unsigned long long>()) throw std::logic_error("sorted keys expected in the first buffer");
    uint32_t nKept = 0; // binary nodes, in DFS pre-order in out.nodes
    const unsigned long long* leafKeys = dKeys.as<unsigned long long>(); // leaf position -> key (gid in the low dword)
    if (builder == kGpuBuilderPloc) {
        int bad = 0;
        HIP_THROW(hipMemcpyAsync(&bad, dBad.as<>(), sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_THROW(hipStreamSynchronize(stream));
        if (bad) throw std::runtime_error("triangle index out of range");
        nKept = plocBuildGpu(dKeys.as<unsigned long long>(), dBox.as<float>(), n, dKeysIn.as<unsigned long long>(), out.nodes, stream);
        leafKeys = dKeysIn.as<unsigned long long>();
    } else {
        DeviceBuffer dK(sizeof(KNode) * nInternal), dParI(sizeof(int) * nInternal), dParL(sizeof(int) * n);
        DeviceBuffer dNodeBox(sizeof(Box6) * nInternal), dFlags(sizeof(unsigned int) * nInternal);
        DeviceBuffer dKept(sizeof(uint32_t) * nInternal), dRank(sizeof(uint32_t) * nInternal);
        hipLaunchKernelGGL(hierarchyKernel, grdI, blk, 0, stream, dKeys.as<unsigned long long>(), n, dK.as<KNode>(), dParI.as<int>(), dParL.as<int>());
        HIP_THROW(hipMemsetAsync(dFlags.as<>(), 0, sizeof(unsigned int) * nInternal, stream));
        hipLaunchKernelGGL(fitKernel, grdN, blk, 0, stream, dK.as<KNode>(), dBox.as<Box6>(), dKeys.as<unsigned long long>(), n, dParI.as<int>(),
                           dParL.as<int>(), dNodeBox.as<Box6>(), dFlags.as<unsigned int>());
        hipLaunchKernelGGL(keptKernel, grdI, blk, 0, stream, dK.as<KNode>(), nInternal, dKept.as<uint32_t>());
        HIP_THROW(hipGetLastError()); // hierarchy / fit / kept launches
        HIP_THROW(gpusort::exclusiveSum(dKept.as<uint32_t>(), dRank.as<uint32_t>(), nInternal, dScanSums.as<uint32_t>(), stream));
        uint32_t lastKept = 0, lastRank = 0;
        int bad = 0;
        HIP_THROW(hipMemcpyAsync(&lastKept, dKept.as<uint32_t>() + (nInternal - 1), 4, hipMemcpyDeviceToHost, stream));
        HIP_THROW(hipMemcpyAsync(&lastRank, dRank.as<uint32_t>() + (nInternal - 1), 4, hipMemcpyDeviceToHost, stream));
        HIP_THROW(hipMemcpyAsync(&bad, dBad.as<>(), sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_THROW(hipStreamSynchronize(stream));
        if (bad) throw std::runtime_error("triangle index out of range");
        nKept = lastKept + lastRank;
        out.nodes = DeviceBuffer(sizeof(crt_bvh_node) * nKept);
        hipLaunchKernelGGL(emitKernel, grdI, blk, 0, stream, dK.as<KNode>(), dKept.as<uint32_t>(), dRank.as<uint32_t>(), dNodeBox.as<Box6>(), dBox.as<Box6>(),
                           dKeys.as<unsigned long long>(), nInternal, out.nodes.as<crt_bvh_node>());
        HIP_THROW(hipGetLastError());
        HIP_THROW(hipStreamSynchronize(stream)); // the Karras scratch dies with this scope
    }
    hipLaunchKernelGGL(gatherKernel, grdN, blk, 0, stream, leafKeys, n, table, n_meshes, in.xyz, in.idx, in.normals, in.uvsIn, out.tris.as<crt_bvh_tri>(),
                       out.shade.as<crt_bvh_shade>(), out.uvs.as<crt_bvh_uv>());
    HIP_THROW(hipGetLastError());
    if (timing) { HIP_THROW(hipStreamSynchronize(stream)); }
    lap("device build");
    // ---- collapse to the 4-wide tree and quantise, still on the device
    DeviceBuffer dScratch(collapseScratchBytes(nKept));
    out.nNodes = nKept;
    out.nTris = n;
    collapseWideGpu(out.nodes.as<crt_bvh_node>(), nKept, dScratch.as<>(), nullptr, nullptr, &out, stream, &out.nNodes4, &out.depth4, &out.maxDepth);
    const double ms = timer.stopAndWait(stream);
    if (device_ms) *device_ms = ms;
    lap("device collapse + quantise");
    return out;
}

// A handful of triangles (n <= kLeafMax): one leaf, wrapped in a node whose right child is an empty leaf with the same box (as the
// SAH path does); nothing worth a kernel launch -- the host does it with the same rules, in the leaf order the device path would
// give: by Morton key.  The tree stays on the host (out.dev empty); whoever needs it in HBM uploads it (uploadTree).
void buildOneLeaf(const crt_mesh_view* meshes, uint32_t n_meshes, uint32_t n, Bvh& out)
{
    std::vector<crt_bvh_tri> inTri;
    std::vector<crt_bvh_shade> inShade;
    std::vector<float> pboxCent; // per triangle: 6 floats box + 3 floats centroid
    flattenMeshes(meshes, n_meshes, inTri, inShade, pboxCent);
    std::vector<crt_bvh_uv> inUv;
    flattenUvs(meshes, n_meshes, inUv);
    auto boxOf = [&](uint32_t i) {
        Box6 b;
        std::memcpy(&b, &pboxCent[9 * static_cast<size_t>(i)], sizeof(Box6));
        return b;
    };
    auto centOf = [&](uint32_t i, int a) { return pboxCent[9 * static_cast<size_t>(i) + 6 + a]; };
    Box6 root = boxOf(0), cb; // cb: the centroids' bounds
    for (int a = 0; a < 3; a++) cb.mn[a] = cb.mx[a] = centOf(0, a);
    for (uint32_t i = 1; i < n; i++) {
        root = unionBox(root, boxOf(i));
        for (int a = 0; a < 3; a++) {
            cb.mn[a] = minSel(cb.mn[a], centOf(i, a));
            cb.mx[a] = maxSel(cb.mx[a], centOf(i, a));
        }
    }
    crt_bvh_node N;
    N.lx0 = N.rx0 = root.mn[0]; N.lx1 = N.rx1 = root.mx[0]; N.ly0 = N.ry0 = root.mn[1]; N.ly1 = N.ry1 = root.mx[1];
    N.lz0 = N.rz0 = root.mn[2]; N.lz1 = N.rz1 = root.mx[2];
    N.left = leafRef(0u, n);
    N.right = leafRef(0u, 0u);
    N.pad0 = N.pad1 = 0;
    out.nodes.push_back(N);
    float extm = 0.0f;
    for (int a = 0; a < 3; a++) {
        const float ext = cb.mx[a] - cb.mn[a];
        if (ext > extm) extm = ext;
    }
    const float scale = mortonScale(extm);
    std::vector<unsigned long long> keys(n);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t q[3];
        for (int a = 0; a < 3; a++) q[a] = quant10((centOf(i, a) - cb.mn[a]) * scale);
        const uint32_t code = (expandBits10(q[0]) << 2) | (expandBits10(q[1]) << 1) | expandBits10(q[2]); // as mortonKernel
        keys[i] = (static_cast<unsigned long long>(code) << 32) | i;
    }
    std::sort(keys.begin(), keys.end());
    out.tris.resize(n);
    out.shade.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        out.tris[i] = inTri[keys[i] & 0xFFFFFFFFull];
        out.shade[i] = inShade[keys[i] & 0xFFFFFFFFull];
    }
    out.nTris = n;
    out.maxDepth = 1;
    collapseBvh4(out);
    reorderUvs(inUv, out);
}

} // namespace

void buildBvhGpu(const crt_mesh_view* meshes, uint32_t n_meshes, Bvh& out, ihipStream_t* stream, double* device_ms, int builder)
{
    if (builder != kGpuBuilderLbvh && builder != kGpuBuilderPloc) throw std::runtime_error("unknown GPU builder");
    const bool timing = std::getenv("CRT_BUILD_TIMING") != nullptr;
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    auto tlast = tnow();
    auto lap = [&](const char* what) {
        if (!timing) return;
        const auto t = tnow();
        std::fprintf(stderr, "[build] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - tlast).count());
        tlast = t;
    };
    out = Bvh();
    if (device_ms) *device_ms = 0.0;
    uint64_t total = 0, totalVerts = 0;
    bool anyNormals = false, anyUvs = false;
    for (uint32_t m = 0; m < n_meshes; m++) {
        if (meshes[m].n_triangles && (!meshes[m].xyz || !meshes[m].idx)) throw std::runtime_error("mesh with triangles but null vertex/index pointer");
        total += meshes[m].n_triangles;
        totalVerts += meshes[m].n_vertices;
        anyNormals |= meshes[m].normals != nullptr && meshes[m].n_triangles > 0;
        anyUvs |= meshes[m].uvs != nullptr && meshes[m].n_triangles > 0;
    }
    if (total >= (1ull << 28)) throw std::runtime_error("too many triangles (limit 2^28 - 1)");
    if (totalVerts >= (1ull << 32)) throw std::runtime_error("too many vertices");
    const uint32_t n = static_cast<uint32_t>(total);
    if (n == 0) return;

    if (n <= static_cast<uint32_t>(kLeafMax)) return buildOneLeaf(meshes, n_meshes, n, out);

    // ---- the meshes as they are, back to back
    const std::vector<MeshEntry> table = makeMeshTable(meshes, n_meshes);
    std::vector<float> hXyz(3 * static_cast<size_t>(totalVerts)), hNormals, hUvs;
    std::vector<uint32_t> hIdx(3 * static_cast<size_t>(n));
    if (anyNormals) hNormals.assign(3 * static_cast<size_t>(totalVerts), 0.0f);
    if (anyUvs) hUvs.assign(3 * static_cast<size_t>(totalVerts), 0.0f);
    for (uint32_t m = 0; m < n_meshes; m++) {
        const crt_mesh_view& M = meshes[m];
        const size_t t0 = table[m].triStart, v0 = table[m].vertStart;
        if (M.n_vertices && M.xyz) std::memcpy(&hXyz[3 * v0], M.xyz, sizeof(float) * 3 * M.n_vertices); // (a mesh without triangles may come without arrays)
        if (M.n_triangles && M.idx) std::memcpy(&hIdx[3 * t0], M.idx, sizeof(uint32_t) * 3 * static_cast<size_t>(M.n_triangles));
        if (M.normals && M.n_vertices) std::memcpy(&hNormals[3 * v0], M.normals, sizeof(float) * 3 * M.n_vertices);
        if (M.uvs && M.n_vertices) std::memcpy(&hUvs[3 * v0], M.uvs, sizeof(float) * 3 * M.n_vertices);
    }
    lap("host concatenate");

    DeviceBuffer dTable(sizeof(MeshEntry) * table.size()), dXyz(sizeof(float) * hXyz.size()), dIdx(sizeof(uint32_t) * hIdx.size());
    DeviceBuffer dNormals(sizeof(float) * hNormals.size()), dUvsIn(sizeof(float) * hUvs.size());
    HIP_THROW(hipMemcpyAsync(dTable.as<>(), table.data(), sizeof(MeshEntry) * table.size(), hipMemcpyHostToDevice, stream));
    HIP_THROW(hipMemcpyAsync(dXyz.as<>(), hXyz.data(), sizeof(float) * hXyz.size(), hipMemcpyHostToDevice, stream));
    HIP_THROW(hipMemcpyAsync(dIdx.as<>(), hIdx.data(), sizeof(uint32_t) * hIdx.size(), hipMemcpyHostToDevice, stream));
    if (anyNormals) HIP_THROW(hipMemcpyAsync(dNormals.as<>(), hNormals.data(), sizeof(float) * hNormals.size(), hipMemcpyHostToDevice, stream));
    if (anyUvs) HIP_THROW(hipMemcpyAsync(dUvsIn.as<>(), hUvs.data(), sizeof(float) * hUvs.size(), hipMemcpyHostToDevice, stream));
    if (timing) { HIP_THROW(hipStreamSynchronize(stream)); }
    lap("alloc + H2D meshes");
    GpuMeshes in;
    in.table = dTable.as<>();
    in.nMeshes = n_meshes;
    in.n = n;
    in.xyz = dXyz.as<float>();
    in.idx = dIdx.as<uint32_t>();
    in.normals = dNormals.as<float>();
    in.uvsIn = anyUvs ? dUvsIn.as<float>() : nullptr;
    out.dev = buildFromDevice(in, builder, stream, device_ms, lap);
    out.nTris = out.dev.nTris;
    out.depth4 = out.dev.depth4;
    out.maxDepth = out.dev.maxDepth;
}

DeviceTree rebuildBvhGpu(const GpuMeshes& in, int builder, ihipStream_t* stream, double* device_ms)
{
    if (builder != kGpuBuilderLbvh && builder != kGpuBuilderPloc) throw std::runtime_error("unknown GPU builder");
    if (in.n <= static_cast<uint32_t>(kLeafMax)) throw std::logic_error("rebuildBvhGpu: more than kLeafMax triangles expected");
    if (device_ms) *device_ms = 0.0;
    return buildFromDevice(in, builder, stream, device_ms, [](const char*) {});
}

DeviceTree uploadTree(const Bvh& host, bool withBinaryAndWide)
{
    DeviceTree t;
    auto put = [](DeviceBuffer& b, const auto& v, size_t room) { // (synchronous copies: the host arrays may die after this call)
        b = DeviceBuffer(room);
        if (!v.empty()) HIP_THROW(hipMemcpy(b.as<>(), v.data(), sizeof(v[0]) * v.size(), hipMemcpyHostToDevice));
    };
    if (withBinaryAndWide) {
        put(t.nodes, host.nodes, sizeof(crt_bvh_node) * host.nodes.size());
        put(t.nodes4, host.nodes4, sizeof(crt_bvh_node4) * host.nodes4.size());
    }
    put(t.nodes4q, host.nodes4q, quantisedBytes(host.nodes4q.size()));
    put(t.tris, host.tris, recordBytes(sizeof(crt_bvh_tri), host.tris.size()));
    put(t.shade, host.shade, recordBytes(sizeof(crt_bvh_shade), host.shade.size()));
    if (!host.uvs.empty()) put(t.uvs, host.uvs, recordBytes(sizeof(crt_bvh_uv), host.uvs.size()));
    t.nNodes = static_cast<uint32_t>(host.nodes.size());
    t.nNodes4 = static_cast<uint32_t>(host.nodes4.size());
    t.nTris = host.nTris;
    t.depth4 = host.depth4;
    t.maxDepth = host.maxDepth;
    return t;
}

int deviceExclusiveSum(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* tileSums, ihipStream_t* stream)
{
    return static_cast<int>(gpusort::exclusiveSum(in, out, n, tileSums, stream));
}

size_t deviceScanScratchBytes(uint32_t n) { return gpusort::scanScratchBytes(n); }

int launchDecodePlanes(const void* nodes4q, uint32_t n, float* planes, ihipStream_t* stream)
{
    static_assert(sizeof(crt_bvh_node4q) == 64 && offsetof(crt_bvh_node4q, qlo_x) == 24 && offsetof(crt_bvh_node4q, ref) == 48, "record layout");
    if (n == 0) return 0;
    const size_t total = static_cast<size_t>(n) * kPlaneStride;
    hipLaunchKernelGGL(decodePlanesKernel, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const unsigned char*>(nodes4q), n, planes);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
