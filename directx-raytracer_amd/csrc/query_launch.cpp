// Host side of the persistent query kernels (query.hip.h runQuery): the table of the kinds' kernels, the sizing of the
// persistent grid and the one launch.  Every kernel file states the QueryKernel rows of its kinds (render_kernels.h).
#include "render_kernels.h"

#include <hip/hip_runtime_api.h>

namespace crt {
namespace {

// Resident wavefronts per SIMD the persistent grids are sized for: at most 7, whatever the kernel's registers allow.  The
// occlusion form of the ray query fits 8 (60 VGPRs), but with 8 its random leg took 0.56 ms against 0.46 with 7 (incoherent
// rays: more concurrent traversals, more cache misses).
constexpr int kQueryMaxWavesPerSimd = 7;

// the LDS part of a workgroup's stacks: 64 lanes x stack_entries entries
size_t queryLdsBytes(const QueryKernel& k, uint32_t stack_entries)
{
    return static_cast<size_t>(stack_entries) * k.entryWords * 64u * sizeof(int);
}

// Resident workgroups of a persistent query kernel (one wavefront each, four SIMDs per CU): what the occupancy calculator
// allows per CU for `ldsBytes` of stack, at most kQueryMaxWavesPerSimd per SIMD, x the CUs of the current device.  0: unknown.
// The caller caches it.
uint32_t queryResidentWorkgroups(const void* kernel, size_t ldsBytes)
{
    int dev = 0, cus = 0, perCu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kernel, 64, ldsBytes) != hipSuccess || perCu <= 0 || cus <= 0)
        return 0u;
    const int most = 4 * kQueryMaxWavesPerSimd;
    return static_cast<uint32_t>(perCu > most ? most : perCu) * static_cast<uint32_t>(cus);
}

} // namespace

const QueryKernel& queryKernel(QueryKind kind)
{
    static const QueryKernel* const kernels[kQueryKinds] = { &kKernelClosestHit, &kKernelOcclusion, &kKernelClosestPoint,
                                                             &kKernelCount,      &kKernelOccupancy, &kKernelListFill,
                                                             &kKernelShade,      &kKernelPath,      &kKernelWinding,
                                                             &kKernelWhitted,    &kKernelAmbient };
    return *kernels[kind];
}

uint32_t queryResident(QueryKind kind, uint32_t stack_entries)
{
    const QueryKernel& k = queryKernel(kind);
    return queryResidentWorkgroups(k.plain, queryLdsBytes(k, stack_entries));
}

void queryLayout(uint32_t n, uint32_t resident, uint32_t& chunk, uint32_t& grid)
{
    // about four reservations per wavefront, of 64 to 1024 records: one atomic on one address costs the whole device a few ns
    uint64_t c = (static_cast<uint64_t>(n) / (4u * static_cast<uint64_t>(resident)) + 63u) & ~static_cast<uint64_t>(63u);
    chunk = static_cast<uint32_t>(c < 64u ? 64u : (c > 1024u ? 1024u : c));
    const uint64_t chunks = (static_cast<uint64_t>(n) + chunk - 1u) / chunk;
    grid = static_cast<uint32_t>(chunks < resident ? chunks : resident);
}

int launchQuery(QueryKind kind, const void* params, bool counting, uint32_t grid, ihipStream_t* stream)
{
    const QueryCommon& c = *static_cast<const QueryCommon*>(params); // (every kind's parameter struct begins with it)
    if (c.n == 0u || grid == 0u) return static_cast<int>(hipSuccess);
    const QueryKernel& k = queryKernel(kind);
    void* args[] = { const_cast<void*>(params) }; // the struct is the kernel's one argument
    (void)hipLaunchKernel(counting ? k.counted : k.plain, dim3(grid), dim3(64), args, queryLdsBytes(k, c.stack_entries), stream);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
