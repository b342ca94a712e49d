// HIP kernels for gfx950 (MI355X): all-hits ray queries (crt_list_hits*, include/crt_hip.h) -- every triangle a ray crosses
// in (tmin, tmax), as a CSR list sorted by distance.
//
// A call is the hit count of point_kernels.hip (hitCountKernel, unchanged) followed by the kernels of this file, all on one
// stream without a host round trip:
//   scan   exclusive sum of the n uint32 counts into n + 1 uint64 offsets (tile sums, one-workgroup scan of the sums, rescan
//          of each tile: the 64-bit sibling of gpu_sort.hip.h's prefix sum)
//   fill   the count's traversal once more (the same everyHitIteration of query.hip.h on the same records, so it accepts the
//          same triangles), whose leaf step writes a hit's prescaled t' and its leaf-order triangle record at offsets[ray] + k++
//   sort   every segment by (t', global id), then resolve: t' 2^-e, (u, v) by re-running triTest as the ray query's record
//          re-read at retirement, inst and prim from the triangle record.  Segments of up to short_max records: one lane per
//          ray, insertion sort.  Longer ones: one wavefront per ray, an all-ascending bitonic network, through LDS in tiles
//          of kSortTile records and over global memory for the strides a tile cannot hold (any length, no scratch).
// fill and sort read offsets[n] first and leave when it exceeds the capacity: the decision "does it fit" is the device's.
//
// The sort compares t' as floats and, only on equal t', the global ids, which it reads from the triangle records (the work
// arrays hold the record index the resolve needs, not the id).  The order is total: a triangle sits in one leaf.
#include "query.hip.h"
#include "../../include/crt_hip.h"

namespace crt {
namespace {

// ---- scan: n uint32 counts -> n + 1 uint64 offsets.  Tiles of 2048 counts; tile n / 2048 holds offsets[n], so there are
// n / 2048 + 1 tiles (up to 2^21 + 1 for n = 2^32 - 1: indices are 64-bit).
constexpr uint32_t kScanThreads = 256, kScanItems = 8, kScanTile = kScanThreads * kScanItems, kScanWaves = kScanThreads / 64;
constexpr uint32_t kSumThreads = 1024;

inline uint32_t listTiles(uint32_t n) { return n / kScanTile + 1u; }

__global__ __launch_bounds__(kScanThreads) void listTileSumKernel(const uint32_t* __restrict__ v, uint32_t n, unsigned long long* __restrict__ sums)
{
    __shared__ unsigned long long part[kScanWaves];
    const unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * kScanTile + threadIdx.x * kScanItems;
    unsigned long long s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanItems; j++) s += base + j < n ? v[base + j] : 0u;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = 0;
        for (uint32_t w = 0; w < kScanWaves; w++) tot += part[w];
        sums[blockIdx.x] = tot;
    }
}

// exclusive sum of v[0..m) in place, one workgroup
__global__ __launch_bounds__(kSumThreads) void listScanSumsKernel(unsigned long long* __restrict__ v, uint32_t m)
{
    __shared__ unsigned long long part[kSumThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (m + kSumThreads - 1u) / kSumThreads;
    const uint32_t lo = t * per < m ? t * per : m, hi = lo + per < m ? lo + per : m;
    unsigned long long sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += v[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < kSumThreads; d <<= 1) {
        const unsigned long long add = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    unsigned long long run = part[t] - sum;
    for (uint32_t i = lo; i < hi; i++) {
        const unsigned long long c = v[i];
        v[i] = run;
        run += c;
    }
}

__global__ __launch_bounds__(kScanThreads) void listTileScanKernel(const uint32_t* __restrict__ v, uint32_t n, const unsigned long long* __restrict__ tileStarts,
                                                                  unsigned long long* __restrict__ out /* n + 1 */)
{
    __shared__ unsigned long long part[kScanWaves];
    const unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * kScanTile + threadIdx.x * kScanItems;
    uint32_t x[kScanItems];
    unsigned long long s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanItems; j++) {
        x[j] = base + j < n ? v[base + j] : 0u;
        s += x[j];
    }
    unsigned long long incl = s;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long up = __shfl_up(incl, off, 64);
        if ((threadIdx.x & 63u) >= static_cast<uint32_t>(off)) incl += up;
    }
    if ((threadIdx.x & 63u) == 63u) part[threadIdx.x >> 6] = incl;
    __syncthreads();
    unsigned long long run = tileStarts[blockIdx.x] + incl - s;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) run += part[w];
#pragma unroll
    for (uint32_t j = 0; j < kScanItems; j++) {
        if (base + j <= n) out[base + j] = run; // entry n is the total
        run += x[j];
    }
}

// ---- fill

// The fill's job for runQuery (query.hip.h): the every-hit traversal whose accepted hits go into the ray's segment.  k counts
// every accepted hit; only the first `room` are stored, so that the fill could never write outside the segment even if it
// disagreed with the count.  A finished ray has nothing to retire: its records are in place.
struct ListFillJob {
    const ListParams& q;
    Stack stack;
    int cur;
    Ray r;
    float tmin = 0.0f, tmax = 0.0f, tcull = 0.0f;
    unsigned long long base = 0;
    uint32_t room = 0, k = 0;

    __device__ __forceinline__ explicit ListFillJob(const ListParams& params) : q(params) { r = makeRay(f3(0.0f, 0.0f, 0.0f), f3(0.0f, 0.0f, 1.0f)); }
    __device__ __forceinline__ void retire(uint32_t) {}
    __device__ __forceinline__ void start(uint32_t idx)
    {
        const float4* recs = reinterpret_cast<const float4*>(q.c.records);
        base = q.offsets[idx];
        room = static_cast<uint32_t>(q.offsets[static_cast<size_t>(idx) + 1u] - base);
        k = 0;
        const float4 a = recs[2u * static_cast<size_t>(idx)], b = recs[2u * static_cast<size_t>(idx) + 1u];
        queryRay(a, b, r, tmin, tmax); // prescaled, as the ray queries
        tcull = cullBound(tmax);
        // a record with a NaN (or an empty interval) is not traced: no crossings
        cur = (queryRayOk(a, b, tmin, tmax) & (q.c.n_nodes != 0u)) ? LayLegacy::kRoot : LayLegacy::kDone;
    }
    template <bool COUNT>
    __device__ __forceinline__ void step(uint32_t& cntNodes, uint32_t& cntTris)
    {
        everyHitIteration<COUNT>(reinterpret_cast<const float4*>(q.c.nodes), reinterpret_cast<const float4*>(q.c.tris), r, tmin, tmax, tcull, stack,
                                 static_cast<int>(q.c.inner_min), cur, cntNodes, cntTris, [&](float t, uint32_t id) {
                                     if (k < room) {
                                         q.tkey[base + k] = t;
                                         q.idkey[base + k] = id;
                                     }
                                     k++;
                                 });
    }
};

template <bool COUNT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LayLegacy::kWavesPerEu, 8))) void listFillKernel(const ListParams q)
{
    if (q.offsets[q.c.n] > q.capacity) return;
    runQuery<COUNT, ListFillJob>(q);
}

// ---- sort and resolve

__device__ __forceinline__ uint32_t gidOf(const float4* tris, uint32_t id) { return __float_as_uint(LayLegacy::triPtr(tris, id)[2].w); }

// (ta, ia) sorts before (tb, ib): t' as floats (-0 == +0), equal t' by global triangle id
__device__ __forceinline__ bool listBefore(float ta, uint32_t ia, float tb, uint32_t ib, const float4* tris)
{
    return (ta < tb) || ((ta == tb) && (gidOf(tris, ia) < gidOf(tris, ib)));
}

// ascending compare-exchange of records lo < hi of a key array pair (LDS or global)
__device__ __forceinline__ void listCmpSwap(float* tk, uint32_t* ik, size_t lo, size_t hi, const float4* tris)
{
    const float ta = tk[lo], tb = tk[hi];
    const uint32_t ia = ik[lo], ib = ik[hi];
    if (listBefore(tb, ib, ta, ia, tris)) {
        tk[lo] = tb; tk[hi] = ta;
        ik[lo] = ib; ik[hi] = ia;
    }
}

struct ListRay {
    Ray r;
    float tmin;
    int e;
};

__device__ __forceinline__ ListRay listRay(const ListParams& q, uint32_t ray)
{
    const float4* recs = reinterpret_cast<const float4*>(q.c.records);
    const float4 a = recs[2u * static_cast<size_t>(ray)], b = recs[2u * static_cast<size_t>(ray) + 1u];
    ListRay lr;
    float tmax;
    lr.e = queryRay(a, b, lr.r, lr.tmin, tmax);
    return lr;
}

// record j of the outputs from the sorted work arrays.  tkey / idkey may be the t / prim outputs themselves: a record is read
// before it is written, by the one thread that resolves it.
__device__ __forceinline__ void listResolve(const ListParams& q, const float4* tris, const ListRay& lr, unsigned long long j)
{
    const float tp = q.tkey[j];
    const uint32_t id = q.idkey[j];
    const float4* T = LayLegacy::triPtr(tris, id);
    const float4 a = T[0], b = T[1], c = T[2];
    if (q.t) q.t[j] = __builtin_amdgcn_ldexpf(tp, -lr.e);
    if (q.uv) {
        float t, u, v;
        (void)triTest<false>(lr.r, a, b, c, lr.tmin, t, u, v);
        reinterpret_cast<float2*>(q.uv)[j] = make_float2(u, v);
    }
    if (q.inst) q.inst[j] = __float_as_uint(a.w); // v0.w = mesh ordinal
    if (q.prim) q.prim[j] = __float_as_uint(b.w); // e1.w = triangle of the mesh
}

// one lane per ray: segments of 1 .. short_max records; longer ones are queued for listSortLongKernel
__global__ __launch_bounds__(256) void listSortShortKernel(const ListParams q)
{
    if (q.offsets[q.c.n] > q.capacity) return;
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= q.c.n) return;
    const unsigned long long lo = q.offsets[i];
    const unsigned long long len = q.offsets[i + 1u] - lo;
    if (len == 0ull) return;
    if (len > q.short_max) {
        q.longRays[atomicAdd(q.longCount, 1u)] = static_cast<uint32_t>(i);
        return;
    }
    const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
    float* tk = q.tkey + lo;
    uint32_t* ik = q.idkey + lo;
    const uint32_t cnt = static_cast<uint32_t>(len);
    for (uint32_t j = 1; j < cnt; j++) {
        const float tj = tk[j];
        const uint32_t ij = ik[j];
        uint32_t m = j;
        while (m > 0u && listBefore(tj, ij, tk[m - 1u], ik[m - 1u], tris)) {
            tk[m] = tk[m - 1u];
            ik[m] = ik[m - 1u];
            m--;
        }
        tk[m] = tj;
        ik[m] = ij;
    }
    const ListRay lr = listRay(q, static_cast<uint32_t>(i));
    for (uint32_t j = 0; j < cnt; j++) listResolve(q, tris, lr, lo + j);
}

// One wavefront per queued ray.  The network: for block sizes k = 2, 4, ... the "flip" step (record i of a block's lower half
// against its mirror i ^ (k - 1)) and then the strides k / 4 .. 1 (i against i + j), every comparator ascending.  Such a
// network sorts any length: a comparator whose upper record lies beyond the segment is skipped, which is what padding with
// +inf records would do.  Blocks up to kSortTile sort inside LDS tile by tile; for larger blocks the flip and the strides
// >= kSortTile run over global memory and the remaining strides again in LDS.
constexpr uint32_t kSortTile = 1024;

__device__ __forceinline__ void listTileSteps(float* tk, uint32_t* ik, uint32_t live, uint32_t jFirst, uint32_t lane, const float4* tris)
{
    for (uint32_t j = jFirst; j > 0u; j >>= 1) {
        for (uint32_t p = lane; p < kSortTile / 2u; p += 64u) {
            const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u));
            if (i + j < live) listCmpSwap(tk, ik, i, i + j, tris);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void listSortLongKernel(const ListParams q)
{
    __shared__ float s_t[kSortTile];
    __shared__ uint32_t s_id[kSortTile];
    if (q.offsets[q.c.n] > q.capacity) return;
    const uint32_t lane = threadIdx.x;
    const float4* tris = reinterpret_cast<const float4*>(q.c.tris);
    const uint32_t nLong = *q.longCount;
    for (uint32_t w = blockIdx.x; w < nLong; w += gridDim.x) {
        const uint32_t ray = q.longRays[w];
        const unsigned long long lo = q.offsets[ray];
        const unsigned long long len = q.offsets[static_cast<size_t>(ray) + 1u] - lo; // a ray's count is a uint32
        float* tk = q.tkey + lo;
        uint32_t* ik = q.idkey + lo;
        // blocks up to a tile: everything in LDS
        for (unsigned long long tb = 0; tb < len; tb += kSortTile) {
            const uint32_t live = static_cast<uint32_t>(len - tb < kSortTile ? len - tb : kSortTile);
            for (uint32_t x = lane; x < live; x += 64u) { s_t[x] = tk[tb + x]; s_id[x] = ik[tb + x]; }
            __syncthreads();
            for (uint32_t k = 2; k <= kSortTile && (k >> 1) < live; k <<= 1) {
                for (uint32_t p = lane; p < kSortTile / 2u; p += 64u) {
                    const uint32_t h = k >> 1, i = ((p & ~(h - 1u)) << 1) | (p & (h - 1u)), m = i ^ (k - 1u);
                    if (m < live) listCmpSwap(s_t, s_id, i, m, tris);
                }
                __syncthreads();
                listTileSteps(s_t, s_id, live, k >> 2, lane, tris);
            }
            for (uint32_t x = lane; x < live; x += 64u) { tk[tb + x] = s_t[x]; ik[tb + x] = s_id[x]; }
            __syncthreads();
        }
        // larger blocks
        for (unsigned long long k = 2ull * kSortTile; (k >> 1) < len; k <<= 1) {
            const unsigned long long h = k >> 1;
            for (unsigned long long p = lane;; p += 64u) {
                const unsigned long long i = ((p & ~(h - 1ull)) << 1) | (p & (h - 1ull)), m = i ^ (k - 1ull); // i grows with p
                if (i >= len) break;
                if (m < len) listCmpSwap(tk, ik, i, m, tris);
            }
            __syncthreads();
            for (unsigned long long j = k >> 2; j >= kSortTile; j >>= 1) {
                for (unsigned long long p = lane;; p += 64u) {
                    const unsigned long long i = ((p & ~(j - 1ull)) << 1) | (p & (j - 1ull));
                    if (i >= len) break;
                    if (i + j < len) listCmpSwap(tk, ik, i, i + j, tris);
                }
                __syncthreads();
            }
            for (unsigned long long tb = 0; tb < len; tb += kSortTile) {
                const uint32_t live = static_cast<uint32_t>(len - tb < kSortTile ? len - tb : kSortTile);
                for (uint32_t x = lane; x < live; x += 64u) { s_t[x] = tk[tb + x]; s_id[x] = ik[tb + x]; }
                __syncthreads();
                listTileSteps(s_t, s_id, live, kSortTile >> 1, lane, tris);
                for (uint32_t x = lane; x < live; x += 64u) { tk[tb + x] = s_t[x]; ik[tb + x] = s_id[x]; }
                __syncthreads();
            }
        }
        const ListRay lr = listRay(q, ray);
        for (unsigned long long j = lane; j < len; j += 64u) listResolve(q, tris, lr, lo + j);
        __syncthreads();
    }
}

} // namespace

// the kind of this file for launchQuery (render_kernels.h)
QueryKernel kKernelListFill = { reinterpret_cast<const void*>(&listFillKernel<false>), reinterpret_cast<const void*>(&listFillKernel<true>), 1u };

size_t listScanScratchBytes(uint32_t n) { return sizeof(unsigned long long) * listTiles(n); }

int launchListScan(const uint32_t* counts, uint32_t n, unsigned long long* offsets, unsigned long long* tileSums, ihipStream_t* stream)
{
    const uint32_t nTiles = listTiles(n);
    hipError_t e;
    hipLaunchKernelGGL(listTileSumKernel, dim3(nTiles), dim3(kScanThreads), 0, stream, counts, n, tileSums);
    if ((e = hipGetLastError()) != hipSuccess) return static_cast<int>(e);
    hipLaunchKernelGGL(listScanSumsKernel, dim3(1), dim3(kSumThreads), 0, stream, tileSums, nTiles);
    if ((e = hipGetLastError()) != hipSuccess) return static_cast<int>(e);
    hipLaunchKernelGGL(listTileScanKernel, dim3(nTiles), dim3(kScanThreads), 0, stream, counts, n, tileSums, offsets);
    return static_cast<int>(hipGetLastError());
}

int launchListSort(const ListParams& q, ihipStream_t* stream)
{
    if (q.c.n == 0u) return static_cast<int>(hipSuccess);
    const uint32_t blocks = static_cast<uint32_t>((static_cast<unsigned long long>(q.c.n) + 255u) / 256u);
    hipLaunchKernelGGL(listSortShortKernel, dim3(blocks), dim3(256), 0, stream, q);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return static_cast<int>(e);
    hipLaunchKernelGGL(listSortLongKernel, dim3(2048), dim3(64), 0, stream, q);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
