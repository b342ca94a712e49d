// PLOC on the GPU (Meister & Bittner 2018, "Parallel Locally-Ordered Clustering"): the second GPU builder (option "gpu_builder"
// = 1), close to the host SAH tree in quality.  It starts from what the LBVH path has already made in bvh_gpu.hip -- the triangle
// boxes and the stable Morton sort -- and leaves a binary tree in DFS pre-order plus the leaf order of the triangles; the caller
// gathers the records and collapses as for the LBVH.  Every rule below fixes the bytes; tests/ploc_reference.py restates them.
//
//   clusters   one per triangle, in sorted order; a cluster's box is its triangle's box (triBoxKernel)
//   distance   d(a, b) = half area of the union box in float32, (dx*dy + dy*dz) + dz*dx (no fused multiply-add: the file is
//              built with -ffp-contract=off), union with the builders' "a < b ? a : b" selects, a = the searching cluster
//   neighbour  NN(i) = the smallest d over j in [i-16, i+16] \ {i}, candidates in ascending j, first candidate kept on ties
//              (so the lower index wins)
//   merge      NN(i) = j, NN(j) = i, i < j: a new node at position i, left = cluster i, right = cluster j; position j is
//              dropped; order kept.  New nodes of one iteration are numbered by position.  Repeat until one cluster is left.
//   bottom-up  at creation: box, triangle count, SAH cost, kept-subtree size and height.  A node of <= kLeafMax triangles is a
//              leaf (all its triangles, in its subtree's DFS order) unless kTravCost*A + C(l) + C(r) < count*A (the host
//              builder's rule); C = count*A for a leaf, the left-hand side for an inner node
//   top-down   one launch per PLOC iteration, newest first (the kernel boundary is the only hand-off, as in refitLevelKernel):
//              pre-order id (root 0, left first), leaf-order position of the first triangle, depth
//   depth      a kept node at depth 6 whose subtree reaches deeper than kMaxDepth (height > 26) is replaced by a balanced tree
//              over its leaf-ordered triangles: split at ceil(count / 2), leaves of <= kLeafMax.  Fewer than 2^28 triangles
//              give at most 26 levels, so every leaf sits at depth <= 32.  Only a tree whose root is taller than kMaxDepth
//              takes this path (two more passes over the iterations and one launch for the balanced subtrees).
#include "bvh_build.h"
#include "hip_own.h"
#include "tri_geometry.hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace crt {
namespace {

constexpr int kRadius = 16;            // neighbour search window: [i - kRadius, i + kRadius]
constexpr uint32_t kBlock = 256;
constexpr uint32_t kRuleDepth = 6;     // where the depth rule cuts
constexpr uint32_t kRuleHeight = static_cast<uint32_t>(kMaxDepth) - kRuleDepth;

struct PNode {           // a cluster: ids < n are the triangles (by sorted position), n.. the merged nodes in creation order
    Box6 box;
    uint32_t left, right; // cluster ids (merged nodes only)
    uint32_t count;       // triangles below
    uint32_t size;        // binary inner nodes its subtree emits when it is kept (0 for a leaf)
    float cost;           // SAH cost
    uint32_t height;      // deepest leaf below, relative (0 for a leaf)
    uint32_t leaf;        // 1: a leaf (triangles and nodes that the leaf rule closes)
    uint32_t pad;
};

struct TopDown { uint32_t first, depth, id, state; }; // state 0: inside a leaf or a balanced subtree, 1: an emitted inner node

struct Balanced { uint32_t id, first, count, pad; };

__device__ __forceinline__ float halfArea(const Box6& b)
{
    const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
    return (dx * dy + dy * dz) + dz * dx;
}

// inner nodes of the balanced tree over c triangles: level k holds 2^k ranges of floor(c / 2^k) or ceil(c / 2^k) triangles,
// c mod 2^k of them the larger; a range of more than kLeafMax is an inner node (and so are all its ancestors)
__device__ uint32_t balancedInner(uint32_t c)
{
    uint32_t s = 0;
    for (uint32_t k = 0; k < 32u; k++) {
        const uint32_t f = c >> k, r = c - (f << k);
        if (f > static_cast<uint32_t>(kLeafMax)) s += 1u << k;
        else if (f == static_cast<uint32_t>(kLeafMax) && r) s += r;
        else break;
    }
    return s;
}

__global__ __launch_bounds__(kBlock) void plocInitKernel(const unsigned long long* __restrict__ keys, const Box6* __restrict__ triBox, uint32_t n,
                                                         PNode* __restrict__ nodes, uint32_t* __restrict__ ids, Box6* __restrict__ cbox)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const Box6 b = triBox[static_cast<uint32_t>(keys[p] & 0xFFFFFFFFull)];
    PNode N;
    N.box = b;
    N.left = N.right = ~0u;
    N.count = 1u;
    N.size = 0u;
    N.cost = halfArea(b); // a one-triangle leaf: 1 * A
    N.height = 0u;
    N.leaf = 1u;
    N.pad = 0u;
    nodes[p] = N;
    ids[p] = p;
    cbox[p] = b;
}

// one thread per cluster; the workgroup's clusters and the kRadius on either side are staged in LDS (288 boxes, 6.9 KB)
__global__ __launch_bounds__(kBlock) void plocNeighbourKernel(const Box6* __restrict__ cbox, uint32_t m, uint32_t* __restrict__ nn)
{
    __shared__ Box6 s[kBlock + 2 * kRadius];
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock - kRadius;
    for (uint32_t k = threadIdx.x; k < kBlock + 2 * kRadius; k += kBlock) {
        const int64_t g = base + k;
        if (g >= 0 && g < static_cast<int64_t>(m)) s[k] = cbox[g];
    }
    __syncthreads();
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= static_cast<int64_t>(m)) return;
    const Box6 a = s[i - base];
    const int64_t lo = i - kRadius > 0 ? i - kRadius : 0, hi = i + kRadius < static_cast<int64_t>(m) - 1 ? i + kRadius : static_cast<int64_t>(m) - 1;
    float best = 0.0f;
    int64_t bestJ = -1;
    for (int64_t j = lo; j <= hi; j++) {
        if (j == i) continue;
        const float d = halfArea(unionBox(a, s[j - base]));
        if (bestJ < 0 || d < best) {
            best = d;
            bestJ = j;
        }
    }
    nn[i] = static_cast<uint32_t>(bestJ);
}

__global__ __launch_bounds__(kBlock) void plocFlagsKernel(const uint32_t* __restrict__ nn, uint32_t m, uint32_t* __restrict__ keep,
                                                          uint32_t* __restrict__ merge)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const uint32_t j = nn[i];
    const bool mutual = nn[j] == i;
    keep[i] = mutual && i > j ? 0u : 1u;
    merge[i] = mutual && i < j ? 1u : 0u;
}

__global__ void plocTotalsKernel(const uint32_t* __restrict__ keep, const uint32_t* __restrict__ keepRank, const uint32_t* __restrict__ merge,
                                 const uint32_t* __restrict__ mergeRank, uint32_t m, uint32_t* __restrict__ totals)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        totals[0] = keepRank[m - 1] + keep[m - 1];
        totals[1] = mergeRank[m - 1] + merge[m - 1];
    }
}

// the next cluster array; a merging position creates its node (the children are final: made by earlier launches)
__global__ __launch_bounds__(kBlock) void plocMergeKernel(const uint32_t* __restrict__ ids, const Box6* __restrict__ cbox, const uint32_t* __restrict__ nn,
                                                          const uint32_t* __restrict__ keep, const uint32_t* __restrict__ keepRank,
                                                          const uint32_t* __restrict__ merge, const uint32_t* __restrict__ mergeRank, uint32_t m,
                                                          uint32_t nodeBase, PNode* __restrict__ nodes, uint32_t* __restrict__ idsOut,
                                                          Box6* __restrict__ cboxOut)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m || !keep[i]) return;
    const uint32_t pos = keepRank[i];
    if (!merge[i]) {
        idsOut[pos] = ids[i];
        cboxOut[pos] = cbox[i];
        return;
    }
    const uint32_t j = nn[i];
    const uint32_t L = ids[i], R = ids[j];
    const PNode& Ln = nodes[L];
    const PNode& Rn = nodes[R];
    PNode N;
    N.box = unionBox(cbox[i], cbox[j]);
    N.left = L;
    N.right = R;
    N.count = Ln.count + Rn.count;
    const float A = halfArea(N.box);
    const float inner = (kTravCost * A + Ln.cost) + Rn.cost;
    const float asLeaf = static_cast<float>(N.count) * A;
    N.leaf = N.count <= static_cast<uint32_t>(kLeafMax) && !(inner < asLeaf) ? 1u : 0u;
    N.cost = N.leaf ? asLeaf : inner;
    N.size = N.leaf ? 0u : 1u + Ln.size + Rn.size;
    N.height = N.leaf ? 0u : 1u + (Ln.height > Rn.height ? Ln.height : Rn.height);
    N.pad = 0u;
    const uint32_t id = nodeBase + mergeRank[i];
    nodes[id] = N;
    idsOut[pos] = id;
    cboxOut[pos] = N.box;
}

// rare path (root taller than kMaxDepth): the kept-subtree sizes again, oldest first, with the balanced trees' sizes in place
__global__ __launch_bounds__(kBlock) void plocSizeKernel(PNode* __restrict__ nodes, uint32_t lo, uint32_t count, const uint32_t* __restrict__ bal)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= count) return;
    const uint32_t x = lo + t;
    const PNode N = nodes[x];
    nodes[x].size = bal[x] ? balancedInner(N.count) : (N.leaf ? 0u : 1u + nodes[N.left].size + nodes[N.right].size);
}

// One PLOC iteration's nodes, newest iteration first: each node reads what its parent wrote for it and writes its children's.
// emit = 0 (rare path only): mark the nodes the depth rule replaces.  emit = 1: write the emitted binary nodes at their ids,
// list the balanced ones, and give every triangle its leaf-order position.
__global__ __launch_bounds__(kBlock) void plocTopDownKernel(const PNode* __restrict__ nodes, uint32_t n, uint32_t lo, uint32_t count, TopDown* __restrict__ td,
                                                            uint32_t* __restrict__ bal, int emit, crt_bvh_node* __restrict__ out,
                                                            uint32_t* __restrict__ triPos, Balanced* __restrict__ balList, uint32_t* __restrict__ balCount)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= count) return;
    const uint32_t x = lo + t;
    const PNode N = nodes[x];
    const TopDown T = td[x];
    uint32_t state = T.state;
    if (state == 1u) {
        if (!emit) {
            if (T.depth == kRuleDepth && N.height > kRuleHeight) {
                bal[x] = 1u;
                state = 0u;
            }
        } else if (bal[x]) {
            Balanced B;
            B.id = T.id; B.first = T.first; B.count = N.count; B.pad = 0u;
            balList[atomicAdd(balCount, 1u)] = B;
            state = 0u;
        }
    }
    const uint32_t ch[2] = { N.left, N.right };
    int32_t ref[2];
    uint32_t first = T.first, id = T.id + 1u;
    for (int c = 0; c < 2; c++) {
        const uint32_t y = ch[c];
        const PNode& C = nodes[y];
        const bool inner = state == 1u && !C.leaf;
        ref[c] = inner ? static_cast<int32_t>(id) : leafRef(first, C.count);
        if (y < n) triPos[y] = first;
        else {
            TopDown U;
            U.first = first; U.depth = T.depth + 1u; U.id = inner ? id : 0u; U.state = inner ? 1u : 0u;
            td[y] = U;
        }
        first += C.count;
        if (inner) id += C.size;
    }
    if (emit && state == 1u) {
        const Box6& lb = nodes[ch[0]].box;
        const Box6& rb = nodes[ch[1]].box;
        crt_bvh_node B;
        B.lx0 = lb.mn[0]; B.lx1 = lb.mx[0]; B.ly0 = lb.mn[1]; B.ly1 = lb.mx[1]; B.lz0 = lb.mn[2]; B.lz1 = lb.mx[2];
        B.rx0 = rb.mn[0]; B.rx1 = rb.mx[0]; B.ry0 = rb.mn[1]; B.ry1 = rb.mx[1]; B.rz0 = rb.mn[2]; B.rz1 = rb.mx[2];
        B.left = ref[0]; B.right = ref[1]; B.pad0 = 0; B.pad1 = 0;
        out[T.id] = B;
    }
}

// leaf position of every triangle -> its sorted key there (what gatherKernel reads) and, on the rare path, its box
__global__ __launch_bounds__(kBlock) void plocPermuteKernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ triPos, uint32_t n,
                                                            unsigned long long* __restrict__ leafKeys, const Box6* __restrict__ triBox, Box6* __restrict__ leafBox)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const unsigned long long k = keys[p];
    leafKeys[triPos[p]] = k;
    if (leafBox) leafBox[triPos[p]] = triBox[static_cast<uint32_t>(k & 0xFFFFFFFFull)];
}

__device__ Box6 rangeBox(const Box6* __restrict__ leafBox, uint32_t first, uint32_t count)
{
    Box6 b = leafBox[first];
    for (uint32_t k = 1; k < count; k++) b = unionBox(b, leafBox[first + k]);
    return b;
}

// rare path: one workgroup per balanced subtree writes its inner nodes level by level; node j of level k finds its range and
// pre-order id by walking its path from the subtree's root (left: id + 1, right: id + 1 + inner nodes of the left range)
__global__ __launch_bounds__(kBlock) void plocBalancedKernel(const Balanced* __restrict__ list, const Box6* __restrict__ leafBox, crt_bvh_node* __restrict__ out)
{
    const Balanced B = list[blockIdx.x];
    for (uint32_t k = 0; k < 32u; k++) {
        const uint32_t f = B.count >> k;
        if (f < static_cast<uint32_t>(kLeafMax) || (f == static_cast<uint32_t>(kLeafMax) && B.count == (f << k))) break; // no range > kLeafMax left
        for (uint64_t j = threadIdx.x; j < (1ull << k); j += kBlock) {
            uint32_t first = B.first, cnt = B.count, id = B.id;
            for (uint32_t bit = k; bit-- > 0;) {
                const uint32_t half = (cnt + 1u) >> 1;
                if ((j >> bit) & 1u) {
                    id += 1u + balancedInner(half);
                    first += half;
                    cnt -= half;
                } else {
                    id += 1u;
                    cnt = half;
                }
            }
            if (cnt <= static_cast<uint32_t>(kLeafMax)) continue;
            const uint32_t half = (cnt + 1u) >> 1;
            const Box6 lb = rangeBox(leafBox, first, half), rb = rangeBox(leafBox, first + half, cnt - half);
            crt_bvh_node N;
            N.lx0 = lb.mn[0]; N.lx1 = lb.mx[0]; N.ly0 = lb.mn[1]; N.ly1 = lb.mx[1]; N.lz0 = lb.mn[2]; N.lz1 = lb.mx[2];
            N.rx0 = rb.mn[0]; N.rx1 = rb.mx[0]; N.ry0 = rb.mn[1]; N.ry1 = rb.mx[1]; N.rz0 = rb.mn[2]; N.rz1 = rb.mx[2];
            N.left = half <= static_cast<uint32_t>(kLeafMax) ? leafRef(first, half) : static_cast<int32_t>(id + 1u);
            N.right = cnt - half <= static_cast<uint32_t>(kLeafMax) ? leafRef(first + half, cnt - half)
                                                                    : static_cast<int32_t>(id + 1u + balancedInner(half));
            N.pad0 = 0; N.pad1 = 0;
            out[id] = N;
        }
    }
}

inline dim3 grid(uint32_t count) { return dim3((count + kBlock - 1u) / kBlock); }

} // namespace

uint32_t plocBuildGpu(const unsigned long long* sortedKeys, const float* triBoxes, uint32_t n, unsigned long long* leafKeys, DeviceBuffer& nodesOut,
                      ihipStream_t* stream)
{
    static_assert(sizeof(Box6) == 24 && sizeof(PNode) == 56 && sizeof(TopDown) == 16, "record layout");
    if (n < 2u) throw std::logic_error("plocBuildGpu: at least two triangles");
    const Box6* triBox = reinterpret_cast<const Box6*>(triBoxes);
    const uint32_t nAll = 2u * n - 1u;
    DeviceBuffer dNodes(sizeof(PNode) * nAll), dTd(sizeof(TopDown) * nAll), dBal(sizeof(uint32_t) * nAll);
    DeviceBuffer dIdsA(sizeof(uint32_t) * n), dIdsB(sizeof(uint32_t) * n), dBoxA(sizeof(Box6) * n), dBoxB(sizeof(Box6) * n);
    DeviceBuffer dNn(sizeof(uint32_t) * n), dKeep(sizeof(uint32_t) * n), dKeepRank(sizeof(uint32_t) * n), dMerge(sizeof(uint32_t) * n),
                 dMergeRank(sizeof(uint32_t) * n);
    DeviceBuffer dScan(deviceScanScratchBytes(n)), dTotals(sizeof(uint32_t) * 4), dTriPos(sizeof(uint32_t) * n);
    PNode* nodes = dNodes.as<PNode>();
    uint32_t* ids = dIdsA.as<uint32_t>();
    uint32_t* idsNext = dIdsB.as<uint32_t>();
    Box6* cbox = dBoxA.as<Box6>();
    Box6* cboxNext = dBoxB.as<Box6>();
    uint32_t* totals = dTotals.as<uint32_t>();

    hipLaunchKernelGGL(plocInitKernel, grid(n), dim3(kBlock), 0, stream, sortedKeys, triBox, n, nodes, ids, cbox);
    HIP_THROW(hipGetLastError());
    // clustering: one pass per iteration; the next iteration's size comes back to the host
    std::vector<std::pair<uint32_t, uint32_t>> iters; // {first node id, nodes created}
    uint32_t m = n, created = 0;
    while (m > 1u) {
        hipLaunchKernelGGL(plocNeighbourKernel, grid(m), dim3(kBlock), 0, stream, cbox, m, dNn.as<uint32_t>());
        hipLaunchKernelGGL(plocFlagsKernel, grid(m), dim3(kBlock), 0, stream, dNn.as<uint32_t>(), m, dKeep.as<uint32_t>(), dMerge.as<uint32_t>());
        HIP_THROW(hipGetLastError());
        HIP_THROW(static_cast<hipError_t>(deviceExclusiveSum(dKeep.as<uint32_t>(), dKeepRank.as<uint32_t>(), m, dScan.as<uint32_t>(), stream)));
        HIP_THROW(static_cast<hipError_t>(deviceExclusiveSum(dMerge.as<uint32_t>(), dMergeRank.as<uint32_t>(), m, dScan.as<uint32_t>(), stream)));
        const uint32_t nodeBase = n + created;
        hipLaunchKernelGGL(plocMergeKernel, grid(m), dim3(kBlock), 0, stream, ids, cbox, dNn.as<uint32_t>(), dKeep.as<uint32_t>(),
                           dKeepRank.as<uint32_t>(), dMerge.as<uint32_t>(), dMergeRank.as<uint32_t>(), m, nodeBase, nodes, idsNext, cboxNext);
        hipLaunchKernelGGL(plocTotalsKernel, dim3(1), dim3(64), 0, stream, dKeep.as<uint32_t>(), dKeepRank.as<uint32_t>(), dMerge.as<uint32_t>(),
                           dMergeRank.as<uint32_t>(), m, totals);
        HIP_THROW(hipGetLastError());
        uint32_t h[2] = { 0, 0 };
        HIP_THROW(hipMemcpyAsync(h, totals, sizeof(h), hipMemcpyDeviceToHost, stream));
        HIP_THROW(hipStreamSynchronize(stream));
        if (h[1] == 0u || h[0] + h[1] != m || created + h[1] > n - 1u) throw std::runtime_error("PLOC: no mutual neighbours (non-finite triangle boxes?)");
        iters.emplace_back(nodeBase, h[1]);
        created += h[1];
        m = h[0];
        std::swap(ids, idsNext);
        std::swap(cbox, cboxNext);
    }
    const uint32_t root = n + created - 1u; // = 2n - 2
    PNode rootNode;
    HIP_THROW(hipMemcpyAsync(&rootNode, nodes + root, sizeof(PNode), hipMemcpyDeviceToHost, stream));
    HIP_THROW(hipMemsetAsync(dBal.as<>(), 0, sizeof(uint32_t) * nAll, stream));
    const TopDown rootTd = { 0u, 0u, 0u, 1u };
    HIP_THROW(hipMemcpyAsync(dTd.as<TopDown>() + root, &rootTd, sizeof(rootTd), hipMemcpyHostToDevice, stream));
    HIP_THROW(hipStreamSynchronize(stream)); // (rootTd, rootNode)
    const bool tooDeep = rootNode.height > static_cast<uint32_t>(kMaxDepth);
    DeviceBuffer dBalList(tooDeep ? sizeof(Balanced) * (1u << kRuleDepth) : 0), dBalCount(sizeof(uint32_t));
    HIP_THROW(hipMemsetAsync(dBalCount.as<>(), 0, sizeof(uint32_t), stream));
    if (tooDeep) {
        for (size_t k = iters.size(); k-- > 0;)
            hipLaunchKernelGGL(plocTopDownKernel, grid(iters[k].second), dim3(kBlock), 0, stream, nodes, n, iters[k].first, iters[k].second,
                               dTd.as<TopDown>(), dBal.as<uint32_t>(), 0, nullptr, dTriPos.as<uint32_t>(), nullptr, nullptr);
        for (size_t k = 0; k < iters.size(); k++)
            hipLaunchKernelGGL(plocSizeKernel, grid(iters[k].second), dim3(kBlock), 0, stream, nodes, iters[k].first, iters[k].second, dBal.as<uint32_t>());
        HIP_THROW(hipGetLastError());
        HIP_THROW(hipMemcpyAsync(&rootNode, nodes + root, sizeof(PNode), hipMemcpyDeviceToHost, stream));
        HIP_THROW(hipStreamSynchronize(stream));
    }
    const uint32_t nBinary = rootNode.size;
    DeviceBuffer dOut(sizeof(crt_bvh_node) * nBinary); // handed over at the end
    crt_bvh_node* out = dOut.as<crt_bvh_node>();
    for (size_t k = iters.size(); k-- > 0;)
        hipLaunchKernelGGL(plocTopDownKernel, grid(iters[k].second), dim3(kBlock), 0, stream, nodes, n, iters[k].first, iters[k].second,
                           dTd.as<TopDown>(), dBal.as<uint32_t>(), 1, out, dTriPos.as<uint32_t>(),
                           dBalList.as<Balanced>(), dBalCount.as<uint32_t>());
    HIP_THROW(hipGetLastError());
    DeviceBuffer dLeafBox(tooDeep ? sizeof(Box6) * n : 0);
    hipLaunchKernelGGL(plocPermuteKernel, grid(n), dim3(kBlock), 0, stream, sortedKeys, dTriPos.as<uint32_t>(), n, leafKeys, triBox,
                       tooDeep ? dLeafBox.as<Box6>() : nullptr);
    HIP_THROW(hipGetLastError());
    if (tooDeep) {
        uint32_t nBal = 0;
        HIP_THROW(hipMemcpyAsync(&nBal, dBalCount.as<>(), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_THROW(hipStreamSynchronize(stream));
        if (nBal > (1u << kRuleDepth)) throw std::logic_error("PLOC: more balanced subtrees than nodes at the rule's depth");
        if (nBal) {
            hipLaunchKernelGGL(plocBalancedKernel, dim3(nBal), dim3(kBlock), 0, stream, dBalList.as<Balanced>(), dLeafBox.as<Box6>(), out);
            HIP_THROW(hipGetLastError());
        }
    }
    HIP_THROW(hipStreamSynchronize(stream)); // the scratch above dies with this call
    nodesOut = std::move(dOut);
    return nBinary;
}

} // namespace crt
