// C ABI of libcrt_hip.so (include/crt_hip.h): renderer context over the HIP runtime + scene-layer accessors.
// Each entry point cites the reference member it replaces in the header.  No CPU fallback exists here: every
// render path ends in launchRender() (render_kernels.hip; mode 200: path_kernels.hip).
#include "mem_util.h"
#include "../../include/crt_hip.h"

#include "bvh_build.h"
#include "bvh_wide.h"
#include "refit.h"
#include "render_kernels.h"
#include "scene.h"

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h> // types and prototypes only: the library is dlopen'ed by crt_comm_init (no link-time dependency)

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

using crt::RenderParams;

// Diagnostics that change what a frame does or costs ("timeline", "debug_skip_units", "debug_force_measure") exist only in
// the diagnostic builds (tools/diag_build.sh, tools/prof_build.sh: -DCRT_DIAG=1); the product rejects the option names.
#ifndef CRT_DIAG
#ifdef CRT_PROF
#define CRT_DIAG 1
#else
#define CRT_DIAG 0
#endif
#endif

struct crt_scene {
    crt::Scene scene;
    // uint32 copies of the int index vectors are not needed: std::vector<int> is reinterpreted like the
    // reference does for its index buffers (R/DXRTRenderer.cpp:314-315)
};

// "The work enqueued on a stream up to here": an event, the stream it was last recorded on, and whether it was recorded at all.
// Everything on the context that one call leaves behind for a later call, possibly on another stream, is guarded by one.
namespace {
struct Fence {
    hipEvent_t event = nullptr; // created at the first record (the frame slots': by crt_create)
    hipStream_t stream = nullptr;
    bool pending = false;

    hipError_t record(hipStream_t s)
    {
        if (!event)
            if (const hipError_t e = hipEventCreateWithFlags(&event, hipEventDisableTiming)) return e;
        stream = s;
        pending = true;
        return hipEventRecord(event, s);
    }
    // `s` runs behind the recorded work.  A wait is only enqueued when it can matter: not for an event that has already completed
    // (a host-side poll), and -- unless sameStreamToo -- not for work recorded on `s` itself, which runs in order anyway: every
    // barrier packet costs the stream a few microseconds
    hipError_t wait(hipStream_t s, bool sameStreamToo) const
    {
        if (!pending || (!sameStreamToo && stream == s) || hipEventQuery(event) == hipSuccess) return hipSuccess;
        return hipStreamWaitEvent(s, event, 0);
    }
    void destroy()
    {
        if (event) (void)hipEventDestroy(event);
        event = nullptr;
        pending = false;
    }
};
} // namespace

struct crt_ctx {
    int device = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t evStart = nullptr, evStop = nullptr;
    std::string error;

    crt::Bvh bvh; // host copy of what sits in HBM
    void* dNodes = nullptr;     // quantised wide nodes: what the kernels traverse
    void* dPlanes = nullptr;    // their decoded plane table (render_kernels.h kPlaneStride), rebuilt at every upload
    // crt_winding_numbers*: the moment table beside the nodes (render_kernels.h kMomentStride), made by the first call that wants
    // it and again once the tree or the records have changed: valid while momentsSerial == sceneSerial, which every upload, refit
    // and rebuild bumps.  Freed with the tree (freeScene, adoptTree)
    void* dMoments = nullptr;
    uint32_t momentsNodes = 0;  // nodes the buffer has room for
    uint32_t momentsSerial = 0;
    void* dBinNodes = nullptr;  // gpu_build only: the binary tree and the full-precision wide tree as the builder left them in
    void* dWideNodes = nullptr; // HBM (no host copy exists; crt_bvh_export* read them back)
    void* dTris = nullptr;
    void* dShade = nullptr;
    void* dLights = nullptr;
    void* dMats = nullptr;
    void* dUvs = nullptr;
    void* dTextures = nullptr;
    void* dTexels = nullptr;
    uint32_t nTextures = 0;
    uint32_t nLights = 0, nMats = 0;
    bool haveScene = false;
    bool gpuBuild = false;      // option "gpu_build": a build on the device instead of the host SAH builder
    int gpuBuilder = crt::kGpuBuilderLbvh; // option "gpu_builder": which one, for "gpu_build" uploads and crt_rebuild
    double buildMs = 0.0;       // wall time of the last crt_upload_scene (build + upload)
    double buildDeviceMs = 0.0; // of which GPU kernels (gpu_build only)
    uint32_t sceneSerial = 0;
    // option "dynamic": the next upload keeps what a refit needs (refit.h); dyn = that state for the current scene, else NULL.
    // A dynamic scene's tree and records exist in HBM only: the host copies in bvh are dropped and the exports read the device.
    bool dynamicOpt = false;
    crt::DynamicScene* dyn = nullptr;
    float sceneLo[3] = { 0.f, 0.f, 0.f }, sceneHi[3] = { 0.f, 0.f, 0.f }; // box of the tree's root: where split rays are cut into segments

    float pos[3] = { 0.f, 0.f, 0.f };
    float rot[9] = { 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f };
    float miss[3] = { 0.f, 1.f, 1.f }; // hlsl:75
    uint32_t mode = 0;                 // R/DXRTRenderer.h:246 default shading mode
    bool counting = false;
    uint32_t pathSpp = 4, pathBounces = 3, pathSeed = 1234; // mode 200 (BASELINE.json configs[4]: 4 spp, 3 bounces)
    uint32_t phongKsPermille = 0, phongExp = 32;            // mode 100: specular term, off by default
    uint32_t tunePathTile = 0;     // mode 200 work split: 0 = default (8), 8 / 16 = pixel tile edge per workgroup
    uint32_t tunePathPipeline = 0; // mode 200: 0 = one persistent kernel with wavefront-private queues (default: 21.2 vs 23.4 ms on C5), 1 = the stages as separate launches over global queues
    uint32_t tunePathPassPaths = 1u << 24; // wavefront pipeline: paths one pass may carry (112 bytes of queue / radiance memory each)
    uint32_t tunePathRanges = 8;   // mode 200: 8 = every XCD works through its own contiguous part of the frame first, 1 = one shared work counter
    // wave scheduling threshold of the closest-hit traversal loop (traversal.hip.h closestIteration; an int: > 0 = node steps while
    // that many lanes stand on inner nodes, -k = while k eighths of the wavefront's LIVE lanes do) and of the any-hit loop.
    // -6 against round 2's fixed 32: primary rays only 0.193 -> 0.172 ms, icosphere soup 0.256 -> 0.231, 5M triangles 0.367 -> 0.352,
    // C3 with shadow rays 0.2866 -> 0.2847, path tracing C5 22.6 -> 22.0 ms, lone launch of an 8-rank share 181 -> 174 us
    uint32_t tuneInnerMin = static_cast<uint32_t>(-6);
    uint32_t tuneInnerMinAny = static_cast<uint32_t>(-6);
    uint32_t tuneStackEntries = 0; // 0 = from the BVH depth
    uint32_t tuneWideOffsets = 0;  // 0 = by the scene's sizes (crt::wideOffsets), 1 = always the 64-bit form
    uint32_t tuneXcdGroup = 16;
    uint32_t tuneBoostUnits = 512;
    // Split packets (split_packet.hip.h): the n most expensive 8x8 packets are rendered by 64 / split_rays wavefronts each whose
    // lanes share the segments of the block's rays.  kSplitAuto (option value -1, the default): none for a whole frame on one GPU
    // -- the launch order keeps the chip full there and splitting only adds work (C3: 0.299 -> 0.336 ms with 64 split) -- and 64 /
    // 128 packets for a tile share of 2 / >= 4 ranks, whose lone launch lasts as long as its slowest wavefront: 221 -> 188, 199 -> 132,
    // 178 -> 118 us at 2 / 4 / 8 ranks on the C3 frame (tools/split_probe.py).
    static constexpr uint32_t kSplitAuto = 0xFFFFFFFFu;
    uint32_t tuneSplitUnits = kSplitAuto;
    uint32_t tuneSplitRaysLog2 = 2; // option "split_rays": 4 rays per wavefront of a split packet (16 wavefronts per packet)
    uint32_t tuneSplitSegsLog2 = 4; // option "split_segments": 16 pieces per split ray
    bool tuneXcdAffine = false;
    uint32_t debugSkipUnits = 0;
    hipStream_t lastRenderStream = nullptr;
    bool haveLastRenderStream = false;
    // launch order from measured costs of an earlier frame: 0 never, 1 always, 2 (default) only for frames issued on the
    // same stream as the frame before.  Such frames run one after another, and starting the packets on the longest
    // critical paths first shortens each of them (0.52 -> 0.43 ms on the 1M-triangle frame); frames issued on
    // alternating streams overlap, the tail of one fills with the head of the next, so the order has nothing left to
    // gain and its bookkeeping only adds cross-stream dependencies (0.43 vs 0.40 ms per frame with 4 in flight).
    int adaptiveOrder = 2;
    // Per-frame scratch lives in a ring of kRing slots: frame f uses slot f % kRing and first waits (on the GPU, never on
    // the host) for the frame that used the slot before it, so up to kRing frames issued on different streams run
    // concurrently without sharing a spill arena or a cost/order buffer.
    static constexpr int kRing = 4;
    struct FrameSlot {
        int* spill = nullptr;          // traversal-stack spill arena (traversal.hip.h Stack)
        size_t spillBytes = 0;
        uint32_t* unitCost = nullptr;  // unitCapacity entries each: what the frame's wavefronts report, ...
        uint32_t* unitOrder = nullptr; // ... and the launch order sorted from it
        uint64_t orderKey = 0;         // frame geometry the stored order belongs to; 0 = none
        uint32_t orderView = 0;        // viewSerial the stored order was measured under
        uint32_t orderGen = 0;         // consecutive measurements of this frame geometry
        uint32_t orderFrame = 0;       // frameSerial of the last measurement
        Fence rendered;                // the slot's last frame, on the stream it ran on
        Fence sorted;                  // the sort of that frame's costs, on the side stream
    };
    FrameSlot slot[kRing];
    uint32_t unitCapacity = 0;       // of every slot's cost and order buffer: the four grow together
    bool debugForceMeasure = false;  // diagnostics: measure and sort at every frame even for an unchanged view
    uint32_t tuneRemeasureEvery = 1; // a changing view re-measures at every use of a slot: stale orders cost more than the measuring (tools/moving_camera.py)
    uint32_t viewSerial = 1;         // bumped when camera, mode or path settings change: costs must be measured again
    uint32_t frameSerial = 0;
    hipStream_t sideStream = nullptr; // sorts the costs of frame f while later frames render
    unsigned long long* dCounters = nullptr;
    // Scratch that belongs to the stream that last used it: calls issued on one stream run one after the other and share ONE
    // arena; only calls on different streams (up to kRing in flight) get arenas of their own (takeArena).
    struct Arena {
        unsigned char* mem = nullptr;
        size_t bytes = 0;
        bool used = false;       // lastUse.stream is meaningful
        Fence lastUse;           // of the last call that used the arena; its stream is the arena's OWNER, set when a stream takes
                                 // the arena (before anything is recorded) and the only stream that ever records it
        uint32_t serial = 0;     // of the last use (the least recently used arena is taken over by a new stream)
    };
    // mode 200: scratch of the persistent path kernel (one region per RESIDENT workgroup + the launch's work counter); serial =
    // frameSerial.  A pool of the frames' own: frames and queries never share an arena
    Arena pathArena[kRing];
    unsigned long long* dTimeline = nullptr; // diagnostic: 3 words per workgroup, counting variant only
    size_t timelineWords = 0;
    bool wantTimeline = false;

    // native multi-GPU frame assembly (crt_comm_init): RCCL communicator + per-ring-slot staging / gathered / frame buffers
    ncclComm_t comm = nullptr;
    struct HostExchange* hostComm = nullptr; // crt_comm_init_host: the tiles travel through shared host memory instead of RCCL
    uint32_t commRank = 0, commRanks = 0;
    struct DistSlot {
        void* stage = nullptr;    // this rank's tiles
        void* gathered = nullptr; // every rank's
        void* frame = nullptr;    // the assembled frame of a call that gave no device buffer
        size_t stageBytes = 0, gatheredBytes = 0, frameBytes = 0;
        Fence done;               // end of the frame that last used the three, on the stream it ran on
    };
    DistSlot dist[kRing];
    uint32_t distSerial = 0;

    // scratch frame buffers for the host-output path, grown on demand
    void* dFrame[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    size_t dFrameBytes[5] = { 0, 0, 0, 0, 0 };

    // progressive accumulation (crt_set_accumulation): mode-200 frames add their samples to per-pixel sums while the key holds.
    // Everything a frame's samples depend on is in the key; spp, counting and the tuning options are not (results never depend
    // on them).  Floats are compared bitwise: a viewer that sets the same pose every tick keeps accumulating.
    struct AccKey {
        float pos[3], rot[9], miss[3];
        uint32_t mode, bounces, seed, sceneSerial, textureSerial, width, height, kind, rank, nRanks;
    };
    uint32_t textureSerial = 0;     // bumped by crt_set_textures
    uint32_t accMax = 0;            // samples per pixel the sums may reach; 0 = off
    uint32_t accSamples = 0;        // samples per pixel in the sums
    AccKey accKey{};                // what the sums belong to (meaningful while accSamples > 0)
    void* dAccum = nullptr;         // 4 doubles per output index of the RGBA8 store (pixel, or staging index of a tile share)
    size_t accumBytes = 0;
    // consecutive accumulating frames depend on each other through the sums: the next one waits (on the GPU) for the last one
    Fence accumUsed;

    // batched ray and point queries (crt_trace_rays* / crt_occluded_rays*, crt_closest_points* / crt_count_hits* /
    // crt_occupancy*): per arena the launch's cursor, counters and the stack spill arena of the persistent query kernel.  Arenas
    // of this pool belong to queries alone (never to a frame); serial = ++raySerial.
    Arena rayArena[kRing];
    uint32_t raySerial = 0;
    uint32_t queryResident[crt::kQueryKinds] = {};        // resident workgroups of each query kernel on this device ...
    uint32_t queryResidentEntries[crt::kQueryKinds] = {}; // ... for this many LDS stack entries
    void* dRayStage = nullptr; // the host entry points' records and outputs, grown on demand
    size_t rayStageBytes = 0;
    // crt_list_hits*: the host form's record arrays (grown on demand, apart from dRayStage, which holds its rays and offsets
    // while the total is read back) and the sort's crossover ("list_short_max")
    void* dListStage = nullptr;
    size_t listStageBytes = 0;
    // lists of up to this many hits are sorted by one lane, longer ones by a wavefront.  Measured (DESIGN.md section 5d,
    // tools/list_hits_bench.py, lists of 0 .. 1024 hits): 2.89 ms from 4 to 24, 2.92 at 32, 2.93 at 64 (all within the 1 %
    // spread of the rounds), 3.02 at 256, 3.93 with every list on one lane.  Any value up to ~64 would do.
    uint32_t tuneListShortMax = 24;
    // crt_trace_rays_backward* / crt_closest_points_backward*: the float64 vertex sums of a dynamic scene, 3 doubles per vertex.
    // Allocated by the first call that wants vertex gradients, freed with the scene (freeScene); calls share it in stream order
    double* dGradSum = nullptr;
    Fence gradUsed; // the last call that used the sums, on the stream it ran on
    hipEvent_t evList[5] = {};    // a listing with stats: before the count, after count / scan / fill / sort
    double listPhaseMs[4] = {};   // count, scan, fill, sort + resolve of the last listing that was given stats (crt_debug_list_phases)
};

namespace {

thread_local std::string g_createError;

int fail(crt_ctx* ctx, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->error = buf;
    else g_createError = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return fail((ctx), CRT_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

void freeScene(crt_ctx* c)
{
    void** ptrs[] = { &c->dNodes, &c->dPlanes, &c->dMoments, &c->dBinNodes, &c->dWideNodes, &c->dTris, &c->dShade, &c->dLights, &c->dMats, &c->dUvs };
    for (void** p : ptrs) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    c->momentsNodes = 0;
    if (c->dGradSum) (void)hipFree(c->dGradSum);
    c->dGradSum = nullptr;
    delete c->dyn;
    c->dyn = nullptr;
    c->haveScene = false;
}

// forget the stored launch orders: the scene changed, or how orders are made or used did
void dropOrders(crt_ctx* c)
{
    for (crt_ctx::FrameSlot& s : c->slot) s.orderKey = 0;
}

// the root record as it sits in HBM: where split rays are cut into segments
int readSceneBox(crt_ctx* c)
{
    for (int a = 0; a < 3; a++) c->sceneLo[a] = c->sceneHi[a] = 0.0f;
    if (c->bvh.dev.nNodes4 > 0) {
        crt_bvh_node4q root;
        HIP_TRY(c, hipMemcpy(&root, c->dNodes, sizeof(root), hipMemcpyDeviceToHost));
        for (int a = 0; a < 3; a++) {
            c->sceneLo[a] = root.lo[a];
            c->sceneHi[a] = crt::decodePlane(255u, root.s[a], root.lo[a]);
        }
    }
    return CRT_OK;
}

// a device buffer of `used` valid bytes moved into one of `bytes` (>= used)
int regrow(crt_ctx* c, void*& p, size_t used, size_t bytes)
{
    void* q = nullptr;
    HIP_TRY(c, hipMalloc(&q, bytes));
    if (p && used) {
        const hipError_t e = hipMemcpy(q, p, used, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            (void)hipFree(q);
            return fail(c, CRT_EHIP, "hipMemcpy failed: %s", hipGetErrorString(e));
        }
    }
    if (p) (void)hipFree(p);
    p = q;
    return CRT_OK;
}

// (ensureBuffer, reserveRayStage and takeArena keep C names: a helper defined below the header's extern "C" has one even in this
// unnamed namespace and so stands in the library's dynamic symbol table, these three since they were written; new helpers down
// there are static instead)
extern "C" {

// A device buffer of at least `need` bytes; one that grows keeps nothing of its contents.  Work in flight on any stream may still
// use the old buffer, hence the device-wide wait.  ownScratch: the buffer is scratch the call keeps for itself; an allocation
// failure is then CRT_ENOMEM (no HIP error left behind), and the caller words the message
int ensureBuffer(crt_ctx* c, void** ptr, size_t* have, size_t need, bool ownScratch = false)
{
    if (*have >= need) return CRT_OK;
    HIP_TRY(c, hipDeviceSynchronize());
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr;
    *have = 0;
    if (!ownScratch) HIP_TRY(c, hipMalloc(ptr, need));
    else if (hipMalloc(ptr, need) != hipSuccess) {
        (void)hipGetLastError();
        *ptr = nullptr;
        return CRT_ENOMEM;
    }
    *have = need;
    return CRT_OK;
}

// The arena of `pool` for a call on the context's stream, grown to `need` bytes and stamped with `serial`: the arena this stream
// used last; else an unused one; else the least recently used one of another stream, once the call that used it last is done.
// ownScratch: as ensureBuffer
int takeArena(crt_ctx* c, crt_ctx::Arena (&pool)[crt_ctx::kRing], size_t need, uint32_t serial, bool ownScratch, crt_ctx::Arena*& out)
{
    crt_ctx::Arena* arena = nullptr;
    for (auto& a : pool)
        if (a.used && a.lastUse.stream == c->stream) arena = &a;
    if (!arena) {
        for (auto& a : pool)
            if (!arena || (!a.used && arena->used) || (a.used == arena->used && a.serial < arena->serial)) arena = &a;
        HIP_TRY(c, arena->lastUse.wait(c->stream, true)); // (whichever stream it was: the arena changes hands)
        arena->lastUse.stream = c->stream;
        arena->used = true;
    }
    const int rc = ensureBuffer(c, reinterpret_cast<void**>(&arena->mem), &arena->bytes, need, ownScratch);
    if (rc == CRT_ENOMEM) return fail(c, CRT_ENOMEM, "query scratch: %zu bytes of device memory not available", need);
    if (rc) return rc;
    arena->serial = serial;
    out = arena;
    return CRT_OK;
}

// the staging buffer of the host forms, grown to `total` bytes
int reserveRayStage(crt_ctx* c, size_t total)
{
    HIP_TRY(c, hipSetDevice(c->device));
    return ensureBuffer(c, &c->dRayStage, &c->rayStageBytes, total);
}

} // extern "C"

inline size_t up256(size_t b) { return (b + 255u) & ~static_cast<size_t>(255u); }

void stampTotal(crt_frame_stats* stats, std::chrono::steady_clock::time_point t0)
{
    if (stats) stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---- Host staging.  A host form is its device form run over the context's staging buffer (dRayStage): the caller lists the
// call's buffers as planes, stageBegin lays them out in list order, each on a 256-byte boundary, grows the buffer, hands back
// the device pointers and enqueues the uploads; after the run stageEnd enqueues the downloads, in list order, and waits for
// the stream.  The pointers hold until the next host form on the context plans its own layout, so a host form is synchronous
// and none of them outlives the call.
struct StagePlane {
    const void* src; // host data the run reads, uploaded before it; NULL = none
    void* dst;       // host buffer the plane is downloaded into after the run; NULL = none
    size_t bytes;
    int over = -1;   // >= 0: the room of that earlier plane, none of its own: a result written in place, downloaded at this place
};

// dev[i] = NULL for a plane that takes no room: one with neither src nor dst (an optional buffer the caller left out)
int stageBegin(crt_ctx* c, const StagePlane* planes, int n, void** dev)
{
    size_t total = 0;
    for (int i = 0; i < n; i++)
        if (planes[i].over < 0 && (planes[i].src || planes[i].dst)) total += up256(planes[i].bytes);
    if (const int rc = reserveRayStage(c, total)) return rc;
    unsigned char* at = static_cast<unsigned char*>(c->dRayStage);
    for (int i = 0; i < n; i++) {
        const StagePlane& pl = planes[i];
        dev[i] = nullptr;
        if (pl.over >= 0) dev[i] = pl.dst ? dev[pl.over] : nullptr;
        else if (pl.src || pl.dst) {
            dev[i] = at;
            at += up256(pl.bytes);
        }
    }
    for (int i = 0; i < n; i++)
        if (planes[i].src) HIP_TRY(c, hipMemcpyAsync(dev[i], planes[i].src, planes[i].bytes, hipMemcpyHostToDevice, c->stream));
    return CRT_OK;
}

int stageDownload(crt_ctx* c, const StagePlane* planes, int n, void* const* dev)
{
    for (int i = 0; i < n; i++)
        if (planes[i].dst) HIP_TRY(c, hipMemcpyAsync(planes[i].dst, dev[i], planes[i].bytes, hipMemcpyDeviceToHost, c->stream));
    return CRT_OK;
}

int stageEnd(crt_ctx* c, const StagePlane* planes, int n, void* const* dev)
{
    if (const int rc = stageDownload(c, planes, n, dev)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

// The context takes a tree in HBM over: its buffers replace the context's (c->bvh.dev keeps the counts and no buffer), the plane
// table of the old tree goes.
static void adoptTree(crt_ctx* c, crt::DeviceTree&& t)
{
    void** olds[] = { &c->dBinNodes, &c->dWideNodes, &c->dNodes, &c->dPlanes, &c->dMoments, &c->dTris, &c->dShade, &c->dUvs };
    for (void** q : olds) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    c->momentsNodes = 0;
    c->dBinNodes = t.nodes.release();
    c->dWideNodes = t.nodes4.release();
    c->dNodes = t.nodes4q.release();
    c->dTris = t.tris.release();
    c->dShade = t.shade.release();
    c->dUvs = t.uvs.release();
    c->bvh.depth4 = t.depth4;
    c->bvh.maxDepth = t.maxDepth;
    c->bvh.nTris = t.nTris;
    c->bvh.dev = std::move(t);
}

// The wide tree, its quantised form and the plane table get room for one node per binary inner node: a refit may collapse to more
// wide nodes than the build did.  What they hold stays (a plane table that does not exist yet is only allocated).
static int reserveRefitCapacity(crt_ctx* c)
{
    const uint32_t cap = c->bvh.dev.nNodes ? c->bvh.dev.nNodes : 1u, n4 = c->bvh.dev.nNodes4;
    if (int rc = regrow(c, c->dWideNodes, sizeof(crt_bvh_node4) * n4, sizeof(crt_bvh_node4) * cap)) return rc;
    if (int rc = regrow(c, c->dNodes, sizeof(crt_bvh_node4q) * n4, crt::quantisedBytes(cap))) return rc;
    return regrow(c, c->dPlanes, c->dPlanes ? sizeof(float) * crt::kPlaneStride * n4 : 0, sizeof(float) * crt::kPlaneStride * cap);
}

// Upload with option "dynamic": the binary and the wide tree are in HBM by now (built there, or uploaded with the rest); they get
// their refit capacity and the meshes are kept.
int setupDynamic(crt_ctx* c, const crt_mesh_view* meshes, uint32_t n_meshes)
{
    if (int rc = reserveRefitCapacity(c)) return rc;
    c->dyn = new (std::nothrow) crt::DynamicScene();
    if (!c->dyn) return fail(c, CRT_ENOMEM, "out of host memory");
    try {
        crt::dynamicInit(*c->dyn, meshes, n_meshes, c->bvh.nodes.empty() ? nullptr : c->bvh.nodes.data(),
                         static_cast<const crt_bvh_node*>(c->dBinNodes), c->bvh.dev.nNodes, c->stream);
    } catch (const std::bad_alloc&) {
        return fail(c, CRT_ENOMEM, "out of host memory while keeping the dynamic scene");
    } catch (const std::exception& ex) {
        return fail(c, CRT_EHIP, "dynamic scene: %s", ex.what());
    }
    std::vector<crt_bvh_node>().swap(c->bvh.nodes);
    std::vector<crt_bvh_node4>().swap(c->bvh.nodes4);
    std::vector<crt_bvh_node4q>().swap(c->bvh.nodes4q);
    std::vector<crt_bvh_tri>().swap(c->bvh.tris);
    std::vector<crt_bvh_shade>().swap(c->bvh.shade);
    return CRT_OK;
}

// Apply the pending updates of a dynamic scene (crt_update_vertices*, crt_set_mesh_transform) before anything reads the tree or the
// records.  A refit changes the scene as a re-upload does: new sceneSerial (accumulated sums and launch orders are stale), new root
// box, and the wide tree's node count and depth may differ.
int applyRefit(crt_ctx* c, double* device_ms)
{
    if (device_ms) *device_ms = 0.0;
    if (!c->dyn || !c->dyn->pending) return CRT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize()); // frames in flight on any stream the caller used still read the records and the tree
    crt::RefitTargets t;
    t.binNodes = static_cast<crt_bvh_node*>(c->dBinNodes);
    t.tris = static_cast<crt_bvh_tri*>(c->dTris);
    t.shade = static_cast<crt_bvh_shade*>(c->dShade);
    t.nodes4 = c->dWideNodes;
    t.nodes4q = c->dNodes;
    t.planes = static_cast<float*>(c->dPlanes);
    uint32_t nWide = 0, depth4 = 0;
    try {
        crt::dynamicRefit(*c->dyn, t, c->stream, &nWide, &depth4, device_ms);
    } catch (const std::exception& ex) {
        return fail(c, CRT_EHIP, "refit failed: %s", ex.what());
    }
    c->bvh.dev.nNodes4 = nWide;
    c->bvh.depth4 = depth4;
    if (int rc = readSceneBox(c)) return rc;
    c->sceneSerial++;
    dropOrders(c);
    return CRT_OK;
}

int ensureFrame(crt_ctx* c, int slot, size_t bytes)
{
    if (c->dFrameBytes[slot] >= bytes) return CRT_OK;
    if (c->dFrame[slot]) (void)hipFree(c->dFrame[slot]);
    c->dFrame[slot] = nullptr;
    c->dFrameBytes[slot] = 0;
    HIP_TRY(c, hipMalloc(&c->dFrame[slot], bytes));
    c->dFrameBytes[slot] = bytes;
    return CRT_OK;
}

uint32_t tilesFor(uint32_t w, uint32_t h) { return ((w + crt::kTile - 1) / crt::kTile) * ((h + crt::kTile - 1) / crt::kTile); }

void fillParams(const crt_ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t nRanks, RenderParams& p)
{
    std::memset(&p, 0, sizeof(p));
    p.nodes = c->dNodes;
    p.planes = static_cast<const float*>(c->dPlanes);
    p.tris = c->dTris;
    p.shade = c->dShade;
    p.lights = c->dLights;
    p.mats = c->dMats;
    p.uvs = c->dUvs;
    p.textures = c->dTextures;
    p.texels = static_cast<const unsigned char*>(c->dTexels);
    p.n_textures = c->nTextures;
    p.n_nodes = c->bvh.dev.nNodes4;
    p.n_tris = c->bvh.nTris;
    p.n_lights = c->nLights;
    p.n_mats = c->nMats;
    crt::copyBytes(p.pos, c->pos, sizeof(p.pos));
    crt::copyBytes(p.rot, c->rot, sizeof(p.rot));
    crt::copyBytes(p.miss, c->miss, sizeof(p.miss));
    crt::copyBytes(p.scene_lo, c->sceneLo, sizeof(p.scene_lo));
    crt::copyBytes(p.scene_hi, c->sceneHi, sizeof(p.scene_hi));
    p.mode = c->mode;
    p.spp = c->pathSpp;
    p.max_bounces = c->pathBounces;
    p.seed = c->pathSeed;
    p.phong_ks = static_cast<float>(c->phongKsPermille) / 1000.0f;
    p.phong_exp = c->phongExp;
    p.width = w;
    p.height = h;
    p.tiles_x = (w + crt::kTile - 1) / crt::kTile;
    p.tiles_y = (h + crt::kTile - 1) / crt::kTile;
    p.rank = rank;
    p.n_ranks = nRanks;
    const uint32_t nTiles = p.tiles_x * p.tiles_y;
    p.n_local_tiles = rank < nTiles ? (nTiles - rank + nRanks - 1) / nRanks : 0;
    p.counters = c->dCounters;
    p.timeline = nullptr;
    p.unit_order = nullptr;
    p.spill = nullptr;
    p.unit_cost = nullptr;
    p.tune_inner_min = c->tuneInnerMin;
    p.tune_inner_min_any = c->tuneInnerMinAny;
    p.xcd_group = c->tuneXcdGroup;
    p.boost_units = c->tuneBoostUnits;
    p.split_units = 0; // set in frameLaunchOrder once a launch order is in use
    p.split_rays_log2 = c->tuneSplitRaysLog2;
    p.split_segs_log2 = c->tuneSplitSegsLog2;
    p.debug_skip_units = c->debugSkipUnits;
    // LDS part of the per-lane stack: 16 entries x 64 lanes x 4 B = 4 KB per wavefront, so that LDS never limits the 7
    // wavefronts per SIMD the kernel's register budget allows (12 .. 20 entries measured alike, 24 costs 4 %); no ray of the
    // bench scenes holds more than 15 entries, deeper ones (up to 3 * depth4 + 1: tests/test_deep_stacks.py) spill to the arena
    p.stack_entries = c->tuneStackEntries ? c->tuneStackEntries : 16u;
    p.wide_offsets = crt::wideOffsets(p.n_nodes, p.n_tris, c->tuneWideOffsets) ? 1u : 0u;
    p.n_batch = 1;
    p.units_per_frame = crt::renderUnitCount(p);
}

// the scene's shading tables as the shaded and the path-traced query take them (crt::ShadeQueryParams, crt::PathQueryParams)
template <class Q> void sceneTables(const crt_ctx* c, Q& q)
{
    q.shade = c->dShade; // as fillParams
    q.lights = c->dLights;
    q.mats = c->dMats;
    q.uvs = c->dUvs;
    q.textures = c->dTextures;
    q.texels = static_cast<const unsigned char*>(c->dTexels);
    q.n_textures = c->nTextures;
    q.n_lights = c->nLights;
    q.n_mats = c->nMats;
    crt::copyBytes(q.miss, c->miss, sizeof(q.miss));
    q.inner_min_any = c->tuneInnerMinAny;
}

// a frame that uses the sums runs after the last one that did, even when issued on another stream (crt_set_stream)
int orderAccum(crt_ctx* c)
{
    HIP_TRY(c, c->accumUsed.wait(c->stream, false));
    return CRT_OK;
}

// after the launch: the sums now hold acc_total samples
int commitAccum(crt_ctx* c, const RenderParams& p)
{
    HIP_TRY(c, c->accumUsed.record(c->stream));
    c->accSamples = p.acc_total;
    return CRT_OK;
}

// What a call with stats reports after its launch: waits for the stream, then kernel_ms = evStart .. evStop and every count zero.
// A launch that counts gives dCounters and four words: with counting on its four counter words are read into them (else zeros),
// of which the fetches mean the same for every kind of call; the ray counts are the caller's to fill in
int readStats(crt_ctx* c, crt_frame_stats* stats, const unsigned long long* dCounters = nullptr, unsigned long long* words = nullptr)
{
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->evStart, c->evStop));
    std::memset(stats, 0, sizeof(*stats));
    stats->kernel_ms = ms;
    if (!dCounters) return CRT_OK;
    std::memset(words, 0, 4 * sizeof(*words));
    if (c->counting) {
        HIP_TRY(c, hipMemcpy(words, dCounters, 4 * sizeof(*words), hipMemcpyDeviceToHost));
        stats->nodes_visited = words[0];
        stats->tris_tested = words[1];
    }
    return CRT_OK;
}

// ---- One frame (runRender), step by step.  Each step enqueues on the context's stream only what its comment says.

// diagnostic builds, option "timeline": 3 words per workgroup, zeroed before the frame
int frameTimeline(crt_ctx* c, RenderParams& p)
{
    if (!c->wantTimeline || p.n_batch != 1) return CRT_OK;
    const size_t words = 3 * (static_cast<size_t>(p.tiles_x + 4) * (p.tiles_y + 4) * 4 + 1024);
    if (c->timelineWords < words) {
        if (c->dTimeline) (void)hipFree(c->dTimeline);
        c->dTimeline = nullptr;
        HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&c->dTimeline), words * sizeof(unsigned long long)));
        c->timelineWords = words;
    }
    HIP_TRY(c, hipMemsetAsync(c->dTimeline, 0, c->timelineWords * sizeof(unsigned long long), c->stream));
    p.timeline = c->dTimeline;
    return CRT_OK;
}

// Mode 200: how the frame is cut into work items, and the scratch of the persistent path kernel from the stream's arena
// (enqueues: a wait when the arena changes hands, and the zeroing of the work counters)
int framePathScratch(crt_ctx* c, RenderParams& p, crt_ctx::Arena*& arena)
{
    // path tracing: resident wavefronts stream the paths of one pixel tile after the other through private queues in HBM.  One
    // 8x8 packet x up to 16 samples per work item (256 paths at 4 spp) measured best at every frame size -- 6.6 vs 10.1 ms on C3
    // at 1080p, 27.3 vs 29.2 ms on C5 at 4K against one 16x16 macro tile x 4 samples
    p.path_tile = c->tunePathTile ? c->tunePathTile : 8u;
    // the stages as separate launches over global queues (8x8 work items, 64-byte nodes), or one persistent kernel
    p.path_wavefront = (c->tunePathPipeline == 1u && p.path_tile == 8u) ? 1u : 0u;
    p.path_samples = std::min<uint32_t>(p.path_tile == 16u ? 4u : 16u, std::max<uint32_t>(1u, p.spp));
    p.path_region_bytes = crt::pathRegionBytes(p.path_tile, p.path_samples);
    p.path_work_items = crt::pathWorkgroupCount(p);
    const size_t kHead = 512; // the work counters (one 64-byte line per range) live in front of the regions
    p.path_ranges = c->tunePathRanges;
    uint32_t wfItems = 0;
    if (p.path_wavefront) {
        wfItems = crt::pathWavefrontPassItems(p, c->tunePathPassPaths);
        p.wf_paths = wfItems * 64u * p.path_samples;
        crt::pathWavefrontLayout(p, wfItems, p.wf_chunk, p.wf_stride);
    }
    const size_t need = p.path_wavefront ? crt::pathWavefrontBytes(p, wfItems) : kHead + static_cast<size_t>(crt::pathGridSize(p)) * p.path_region_bytes;
    if (const int rc = takeArena(c, c->pathArena, need, c->frameSerial, false, arena)) return rc;
    if (p.path_wavefront) {
        const size_t plane = static_cast<size_t>(p.wf_paths) * 16u, qplane = static_cast<size_t>(p.wf_stride) * 16u; // one float4 per path / queue entry
        unsigned char* at = arena->mem;
        p.wf_counts = reinterpret_cast<uint32_t*>(at); at += crt::kWfHeadBytes;
        p.wf_shade_q = at; at += 3u * qplane;
        p.wf_trace_q = at; at += 2u * qplane;
        p.wf_done = at; at += plane;
        p.wf_thr = at; at += plane;
        p.wf_accum = p.spp > p.path_samples ? at : nullptr;
    } else {
        p.path_counter = reinterpret_cast<uint32_t*>(arena->mem);
        p.path_scratch = arena->mem + kHead;
        HIP_TRY(c, hipMemsetAsync(p.path_counter, 0, kHead, c->stream));
    }
    return CRT_OK;
}

// How many packets are split, at most a quarter of them.  Option "split_units", whose default kSplitAuto stands for two numbers:
// 128 when the spill arena is sized (sizing: the most the rule below can ask for), and for the launch none / 64 / 128 by the
// number of ranks (the measurements stand at kSplitAuto)
uint32_t splitUnits(const crt_ctx* c, const RenderParams& p, bool sizing)
{
    uint32_t want = c->tuneSplitUnits;
    if (want == crt_ctx::kSplitAuto) want = sizing || p.n_ranks >= 4u ? 128u : (p.n_ranks >= 2u ? 64u : 0u);
    return std::min(want, crt::renderUnitCount(p) / 4u);
}

// the slot's stack spill arena (enqueues nothing; after framePathScratch, whose work split sizes it in mode 200)
int frameSpill(crt_ctx* c, crt_ctx::FrameSlot& slot, RenderParams& p)
{
    // deepest stack a ray can build: three pending siblings per wide level; what does not fit the LDS part spills
    const uint32_t deepest = 3u * c->bvh.depth4 + 1u;
    p.spill_stride = deepest > p.stack_entries ? deepest - p.stack_entries : 1u;
    // (mode 200: one slice per resident workgroup of the persistent kernel)
    // (+ 64 slices for each of the four wavefronts of a split packet)
    const size_t groups = p.mode >= 200u ? static_cast<size_t>(crt::pathGridSize(p))
                                         : (static_cast<size_t>(crt::renderUnitCount(p)) + 16u * splitUnits(c, p, true)) * p.n_batch;
    const size_t need = groups * 64u * p.spill_stride * sizeof(int);
    if (const int rc = ensureBuffer(c, reinterpret_cast<void**>(&slot.spill), &slot.spillBytes, need)) return rc;
    p.spill = slot.spill;
    return CRT_OK;
}

// every slot's cost and order buffer made to hold nUnits entries, after one device-wide wait; the stored orders are lost
int growUnitBuffers(crt_ctx* c, uint32_t nUnits)
{
    HIP_TRY(c, hipDeviceSynchronize()); // (frames of other streams may still use the buffers about to be replaced)
    for (crt_ctx::FrameSlot& s : c->slot) {
        if (s.unitCost) (void)hipFree(s.unitCost);
        if (s.unitOrder) (void)hipFree(s.unitOrder);
        s.unitCost = s.unitOrder = nullptr;
        s.sorted.pending = false;
    }
    dropOrders(c);
    c->unitCapacity = 0;
    for (crt_ctx::FrameSlot& s : c->slot) {
        HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&s.unitCost), sizeof(uint32_t) * nUnits));
        HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&s.unitOrder), sizeof(uint32_t) * nUnits));
    }
    c->unitCapacity = nUnits;
    return CRT_OK;
}

// Cost feedback: the lifetimes frame f's wavefronts report are sorted on a side stream while the next frames render and
// order the launch of frame f + kRing (same ring slot), so neither the sort nor the dependency on an earlier frame
// sits on a frame's critical path and kRing frames can be in flight.  Hint only: a stale or missing order changes
// speed, never results.
struct LaunchOrder {
    uint32_t nUnits = 0;
    uint64_t key = 0;     // the frame geometry an order measured by this frame belongs to
    bool measure = false; // this frame reports its costs, and they are sorted behind it
};

// Whether the frame is launched in the slot's stored order (p.unit_order), how many packets it splits (p.split_units) and whether
// it measures (p.unit_cost, lo.measure).  Enqueues nothing
int frameLaunchOrder(crt_ctx* c, crt_ctx::FrameSlot& slot, RenderParams& p, LaunchOrder& lo)
{
    lo.nUnits = crt::renderUnitCount(p);
    lo.key = (static_cast<uint64_t>(p.width) << 40) ^ (static_cast<uint64_t>(p.height) << 20) ^ (static_cast<uint64_t>(p.n_ranks) << 8) ^ p.rank ^
             (static_cast<uint64_t>(c->sceneSerial) << 52) ^ 1ull;
    const bool sameStream = c->haveLastRenderStream && c->lastRenderStream == c->stream;
    c->lastRenderStream = c->stream;
    c->haveLastRenderStream = true;
    if (!(c->adaptiveOrder == 1 || (c->adaptiveOrder == 2 && sameStream)) || !lo.nUnits || p.mode >= 200u) return CRT_OK; // (the path pipeline has its own work split)
    if (c->unitCapacity < lo.nUnits)
        if (const int rc = growUnitBuffers(c, lo.nUnits)) return rc;
    const bool usable = slot.orderKey == lo.key;
    p.unit_order = usable ? slot.unitOrder : nullptr;
    p.split_units = usable ? splitUnits(c, p, false) : 0u; // (at most a quarter of the packets: the spill arena is sized for that)
    // Costs are measured (and sorted) twice in a row -- the first measurement ran under an unordered launch -- and then:
    // an unchanged view keeps its order for good; a view that keeps changing (a moving camera) measures again every
    // remeasure_every-th use of the slot.  Default 1: the order ages fast -- with a camera turning 0.01 degrees per frame
    // an order 32 frames old cost 0.367 ms per frame, 128 frames old 0.423, against 0.347 when measured every frame.
    // (The feedback itself -- cost stores, the sort beside the next frame -- is 1.4 % of a frame: tools/moving_camera.py --wobble;
    //  the rest of that run's difference to a static view was the frame's own cost changing along the orbit.)
    const bool twice = usable && slot.orderGen >= 2;
    const bool sameView = slot.orderView == c->viewSerial;
    const bool recent = (c->frameSerial - slot.orderFrame) < static_cast<uint32_t>(crt_ctx::kRing) * c->tuneRemeasureEvery;
    if (c->debugForceMeasure || !(twice && (sameView || recent))) {
        p.unit_cost = slot.unitCost;
        lo.measure = true;
        slot.orderGen = usable ? slot.orderGen + 1 : 1;
        slot.orderView = c->viewSerial;
        slot.orderFrame = c->frameSerial;
    }
    return CRT_OK;
}

// The previous user of this slot (frame f - kRing, possibly on another stream) and the sort of its costs must be done before this
// frame touches the slot's spill arena, cost or order buffer; a frame that uses the sums runs after the last one that did.
// Enqueues up to three waits (Fence::wait: only where one can matter); the sort ran on the side stream, so it always can
int frameWaits(crt_ctx* c, crt_ctx::FrameSlot& slot, const RenderParams& p)
{
    HIP_TRY(c, slot.sorted.wait(c->stream, true));
    if (p.acc_sum)
        if (const int rc = orderAccum(c)) return rc;
    HIP_TRY(c, slot.rendered.wait(c->stream, false));
    slot.sorted.pending = false;
    return CRT_OK;
}

// the launch, between the timer's events when stats are wanted, and the records of everything it used
int frameLaunch(crt_ctx* c, crt_ctx::FrameSlot& slot, crt_ctx::Arena* arena, const RenderParams& p, const LaunchOrder& lo, bool timed)
{
    // split packets add their quarters' lifetimes into their cost slot: start from zero
    if (p.unit_cost && p.split_units) HIP_TRY(c, hipMemsetAsync(p.unit_cost, 0, sizeof(uint32_t) * lo.nUnits, c->stream));
    if (timed) HIP_TRY(c, hipEventRecord(c->evStart, c->stream));
    const int rc = crt::launchRender(p, c->counting, c->stream);
    if (rc != 0) return fail(c, CRT_EHIP, "render kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
    if (timed) HIP_TRY(c, hipEventRecord(c->evStop, c->stream)); // kernel_ms = the render kernel alone
    HIP_TRY(c, slot.rendered.record(c->stream));
    if (arena) HIP_TRY(c, arena->lastUse.record(c->stream));
    if (p.acc_sum) return commitAccum(c, p);
    return CRT_OK;
}

// the frame's costs sorted into the slot's launch order, on the side stream behind the frame
int frameSortCosts(crt_ctx* c, crt_ctx::FrameSlot& slot, const LaunchOrder& lo)
{
    hipStream_t ss = c->sideStream;
    HIP_TRY(c, hipStreamWaitEvent(ss, slot.rendered.event, 0));
    const int rs = crt::launchSortUnits(slot.unitCost, slot.unitOrder, lo.nUnits, c->tuneXcdAffine, ss);
    if (rs != 0) return fail(c, CRT_EHIP, "sort kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rs)));
    HIP_TRY(c, slot.sorted.record(ss));
    slot.orderKey = lo.key;
    return CRT_OK;
}

// synchronises; rays_primary = the pixels this launch rendered, or with counting what the kernel counted
int frameStats(crt_ctx* c, const RenderParams& p, crt_frame_stats* stats)
{
    unsigned long long words[4];
    if (const int rc = readStats(c, stats, c->dCounters, words)) return rc;
    const uint32_t nTiles = p.tiles_x * p.tiles_y;
    for (uint32_t k = p.rank; k < nTiles; k += p.n_ranks) {
        const uint32_t tx = k % p.tiles_x, ty = k / p.tiles_x;
        const uint32_t w = std::min<uint32_t>(crt::kTile, p.width - tx * crt::kTile);
        const uint32_t h = std::min<uint32_t>(crt::kTile, p.height - ty * crt::kTile);
        stats->rays_primary += static_cast<uint64_t>(w) * h;
    }
    if (c->counting) {
        stats->rays_shadow = words[2];
        stats->rays_primary = words[3]; // closest-hit rays: camera rays, plus bounce rays in mode 200
    }
    return CRT_OK;
}

// enqueue one frame; when stats != nullptr, bracket with events, synchronise and fill the timers/counters
int runRender(crt_ctx* c, RenderParams& p, crt_frame_stats* stats)
{
    HIP_TRY(c, hipSetDevice(c->device)); // the calling thread's current device may be another one (scratch hipMallocs below)
    if (c->counting) HIP_TRY(c, hipMemsetAsync(c->dCounters, 0, 32 * sizeof(unsigned long long), c->stream));
    int rc = frameTimeline(c, p);
    if (rc) return rc;
    // Per-frame scratch lives in a ring: see crt_ctx::kRing
    crt_ctx::FrameSlot& slot = c->slot[c->frameSerial++ % crt_ctx::kRing];
    crt_ctx::Arena* arena = nullptr; // mode 200 only
    if (p.mode >= 200u && (rc = framePathScratch(c, p, arena)) != CRT_OK) return rc;
    if ((rc = frameSpill(c, slot, p)) != CRT_OK) return rc;
    LaunchOrder lo;
    if ((rc = frameLaunchOrder(c, slot, p, lo)) != CRT_OK) return rc;
    if ((rc = frameWaits(c, slot, p)) != CRT_OK) return rc;
    if ((rc = frameLaunch(c, slot, arena, p, lo, stats != nullptr)) != CRT_OK) return rc;
    if (lo.measure && (rc = frameSortCosts(c, slot, lo)) != CRT_OK) return rc;
    return stats ? frameStats(c, p, stats) : CRT_OK;
}

enum { kAccFrame = 1u, kAccTiles = 2u }; // the entry-point kinds whose frames accumulate (part of the key)

// Mode 200 with accumulation on: start the sums over when the key changed, make room for them, and choose the samples this call
// traces: acc_base .. acc_base + spp - 1, at most up to the limit.  p.spp = 0 afterwards: the sums are at the limit and the call
// only resolves them (runAccumResolve).  Other modes leave p and the sums alone.
int beginAccum(crt_ctx* c, RenderParams& p, uint32_t kind)
{
    if (c->accMax == 0u || p.mode < 200u) return CRT_OK;
    crt_ctx::AccKey k;
    std::memset(&k, 0, sizeof(k));
    crt::copyBytes(k.pos, p.pos, sizeof(k.pos));
    crt::copyBytes(k.rot, p.rot, sizeof(k.rot));
    crt::copyBytes(k.miss, p.miss, sizeof(k.miss));
    k.mode = p.mode;
    k.bounces = p.max_bounces;
    k.seed = p.seed;
    k.sceneSerial = c->sceneSerial;
    k.textureSerial = c->textureSerial;
    k.width = p.width;
    k.height = p.height;
    k.kind = kind;
    k.rank = p.rank;
    k.nRanks = p.n_ranks;
    if (c->accSamples == 0u || std::memcmp(&k, &c->accKey, sizeof(k)) != 0) {
        c->accSamples = 0u;
        c->accKey = k;
    }
    const size_t outputs = kind == kAccTiles ? static_cast<size_t>(crt_tile_slots(p.width, p.height, p.n_ranks)) * crt::kTile * crt::kTile
                                             : static_cast<size_t>(p.width) * p.height;
    const size_t need = outputs * 4u * sizeof(double); // float64 sums {x, y}, {z, 0} (path_kernels.hip loadSum)
    if (c->accumBytes < need) { // (a larger frame: the key has changed, nothing in the old sums is kept)
        HIP_TRY(c, hipSetDevice(c->device));
        if (const int rc = ensureBuffer(c, &c->dAccum, &c->accumBytes, need)) return rc;
    }
    const uint32_t traced = std::min(p.spp, c->accMax - c->accSamples);
    p.acc_sum = c->dAccum;
    p.acc_base = c->accSamples;
    p.acc_total = c->accSamples + traced;
    p.spp = traced;
    return CRT_OK;
}

// accumulation at its limit: the stored sums resolved once more, no ray traced (stats: zero rays)
int runAccumResolve(crt_ctx* c, const RenderParams& p, crt_frame_stats* stats)
{
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = orderAccum(c);
    if (rc) return rc;
    if (c->counting) HIP_TRY(c, hipMemsetAsync(c->dCounters, 0, 32 * sizeof(unsigned long long), c->stream));
    if (stats) HIP_TRY(c, hipEventRecord(c->evStart, c->stream));
    rc = crt::launchPathAccumResolve(p, c->stream);
    if (rc != 0) return fail(c, CRT_EHIP, "resolve kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
    if (stats) HIP_TRY(c, hipEventRecord(c->evStop, c->stream));
    if ((rc = commitAccum(c, p)) != CRT_OK) return rc;
    return stats ? readStats(c, stats) : CRT_OK;
}

// one frame of an entry point that accumulates (kind: kAccFrame / kAccTiles)
int runFrame(crt_ctx* c, RenderParams& p, crt_frame_stats* stats, uint32_t kind)
{
    const int rc = beginAccum(c, p, kind);
    if (rc) return rc;
    return p.acc_sum && p.spp == 0u ? runAccumResolve(c, p, stats) : runRender(c, p, stats);
}

int checkRenderable(crt_ctx* c, uint32_t w, uint32_t h)
{
    if (!c) return CRT_EINVAL;
    if (!c->haveScene) return fail(c, CRT_ESTATE, "no scene uploaded: call crt_upload_scene first");
    if (w == 0 || h == 0 || w > 65536 || h > 65536) return fail(c, CRT_EINVAL, "bad frame size %ux%u", w, h);
    return applyRefit(c, nullptr);
}

// ---- crt_set_option: one row per option.  What an option means and why it has its default stands at the field it is stored in.
template <int lo, int hi> bool within(int v) { return v >= lo && v <= hi; }
template <int... values> bool oneOf(int v) { return ((v == values) || ...); }
bool any(int) { return true; }
bool innerMin(int v) { return v >= -8 && v <= 65 && v != 0; } // negative: adaptive, eighths of the live lanes
uint32_t log2Of(int v) { return v == 4 ? 2u : (v == 8 ? 3u : 4u); }

enum OptionEffect { kNoEffect, kNewView /* viewSerial++, even for the value it had: costs are measured again */, kDropOrders };
struct Option {
    const char* name;
    bool (*accepts)(int);
    void (*store)(crt_ctx& c, int v);
    OptionEffect effect = kNoEffect;
    const char* refusal = nullptr; // the option's own message for a value it does not accept; NULL = the common one
};
#define U32(field) [](crt_ctx& c, int v) { c.field = static_cast<uint32_t>(v); }
#define FLAG(field) [](crt_ctx& c, int v) { c.field = v != 0; }
const Option kOptions[] = {
    { "gpu_build", any, FLAG(gpuBuild) },
    { "dynamic", any, FLAG(dynamicOpt) },
    { "gpu_builder", oneOf<crt::kGpuBuilderLbvh, crt::kGpuBuilderPloc>, [](crt_ctx& c, int v) { c.gpuBuilder = v; } },
    // the 64-byte 4-wide tree is the only layout: 0 names it, any other width is rejected
    { "bvh_width", oneOf<0>, [](crt_ctx&, int) {} },
    { "spp", within<1, 65536>, U32(pathSpp), kNewView },
    { "max_bounces", within<0, 64>, U32(pathBounces), kNewView },
    { "phong_ks", within<0, 100000>, U32(phongKsPermille), kNewView },
    { "phong_exponent", within<1, 65536>, U32(phongExp), kNewView },
    { "seed", any, U32(pathSeed) },
    { "path_pipeline", oneOf<0, 1>, U32(tunePathPipeline) },
    { "path_pass_paths", within<(1 << 16), (1 << 25)>, U32(tunePathPassPaths) },
    { "path_ranges", oneOf<1, 8>, U32(tunePathRanges) },
    { "path_tile", oneOf<0, 8, 16>, U32(tunePathTile) },
    { "inner_min", innerMin, U32(tuneInnerMin) },
    { "inner_min_any", innerMin, U32(tuneInnerMinAny) },
    { "list_short_max", within<1, 1024>, U32(tuneListShortMax) },
    { "xcd_group", oneOf<1, 2, 4, 8, 16>, U32(tuneXcdGroup) },
    { "xcd_affine_order", oneOf<0, 1>, FLAG(tuneXcdAffine), kDropOrders }, // orders sorted the other way are stale
    { "split_units", within<-1, 65536>, [](crt_ctx& c, int v) { c.tuneSplitUnits = v < 0 ? crt_ctx::kSplitAuto : static_cast<uint32_t>(v); } },
    { "split_rays", oneOf<4, 8, 16>, [](crt_ctx& c, int v) { c.tuneSplitRaysLog2 = log2Of(v); } },
    { "split_segments", oneOf<4, 8, 16>, [](crt_ctx& c, int v) { c.tuneSplitSegsLog2 = log2Of(v); } },
    { "boost_units", within<0, INT_MAX>, U32(tuneBoostUnits) },
#if CRT_DIAG
    { "debug_skip_units", within<0, INT_MAX>, U32(debugSkipUnits) },
    { "timeline", any, FLAG(wantTimeline) },
    { "debug_force_measure", any, FLAG(debugForceMeasure) },
#endif
    { "remeasure_every", within<1, 1024>, U32(tuneRemeasureEvery) },
    { "adaptive_order", within<0, 2>, [](crt_ctx& c, int v) { c.adaptiveOrder = v; }, kDropOrders, "adaptive_order takes 0 (off), 1 (on) or 2 (auto)" },
    { "stack_entries", within<0, crt::kStackEntries>, U32(tuneStackEntries) },
    { "wide_offsets", oneOf<0, 1>, U32(tuneWideOffsets) },
};
#undef U32
#undef FLAG

} // namespace

extern "C" {

uint32_t crt_abi_version(void) { return CRT_ABI_VERSION; }

namespace {
// the 1-workgroup sort that orders a later frame runs beside the next frame's render kernel: highest priority, so it is
// dispatched at once instead of queueing behind 32 640 render workgroups
hipError_t createSideStream(crt_ctx* c)
{
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess) return e;
    return hipStreamCreateWithPriority(&c->sideStream, hipStreamNonBlocking, greatest);
}
// the frame slots' events up front: without them crt_create fails, not the first frame
hipError_t createRingEvents(crt_ctx* c)
{
    for (crt_ctx::FrameSlot& s : c->slot)
        for (Fence* f : { &s.rendered, &s.sorted })
            if (const hipError_t e = hipEventCreateWithFlags(&f->event, hipEventDisableTiming)) return e;
    return hipSuccess;
}
} // namespace

int crt_create(crt_ctx** out, int device_id)
{
    if (!out) return fail(nullptr, CRT_EINVAL, "crt_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, CRT_ENODEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device_id < 0 || device_id >= n) return fail(nullptr, CRT_EINVAL, "device_id %d out of range [0,%d)", device_id, n);
    crt_ctx* c = new (std::nothrow) crt_ctx();
    if (!c) return fail(nullptr, CRT_ENOMEM, "out of host memory");
    c->device = device_id;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->ownStream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&c->evStart)) != hipSuccess || (e = hipEventCreate(&c->evStop)) != hipSuccess ||
        (e = createSideStream(c)) != hipSuccess ||
        (e = createRingEvents(c)) != hipSuccess ||
        (e = hipMalloc(reinterpret_cast<void**>(&c->dCounters), 32 * sizeof(unsigned long long))) != hipSuccess) {
        const int rc = fail(nullptr, CRT_ENODEVICE, "HIP initialisation failed on device %d: %s", device_id, hipGetErrorString(e));
        crt_destroy(c);
        return rc;
    }
    c->stream = c->ownStream;
    *out = c;
    return CRT_OK;
}

void crt_destroy(crt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize(); // frames may still be in flight on streams the caller set earlier, not only on the current one
    freeScene(c);
    for (int i = 0; i < 5; i++)
        if (c->dFrame[i]) (void)hipFree(c->dFrame[i]);
    (void)crt_comm_destroy(c);
    if (c->sideStream) (void)hipStreamSynchronize(c->sideStream);
    for (int i = 0; i < crt_ctx::kRing; i++) {
        crt_ctx::FrameSlot& s = c->slot[i];
        crt_ctx::DistSlot& d = c->dist[i];
        for (void* p : std::initializer_list<void*>{ s.spill, s.unitCost, s.unitOrder, d.stage, d.gathered, d.frame, c->pathArena[i].mem, c->rayArena[i].mem })
            if (p) (void)hipFree(p);
        for (Fence* f : { &s.rendered, &s.sorted, &d.done, &c->pathArena[i].lastUse, &c->rayArena[i].lastUse }) f->destroy();
    }
    if (c->dCounters) (void)hipFree(c->dCounters);
    if (c->dTextures) (void)hipFree(c->dTextures);
    if (c->dTexels) (void)hipFree(c->dTexels);
    if (c->sideStream) (void)hipStreamDestroy(c->sideStream);
    if (c->dTimeline) (void)hipFree(c->dTimeline);
    if (c->dAccum) (void)hipFree(c->dAccum);
    c->accumUsed.destroy();
    c->gradUsed.destroy();
    if (c->dRayStage) (void)hipFree(c->dRayStage);
    if (c->dListStage) (void)hipFree(c->dListStage);
    for (hipEvent_t e : c->evList)
        if (e) (void)hipEventDestroy(e);
    if (c->evStart) (void)hipEventDestroy(c->evStart);
    if (c->evStop) (void)hipEventDestroy(c->evStop);
    if (c->ownStream) (void)hipStreamDestroy(c->ownStream);
    delete c;
}

const char* crt_last_error(const crt_ctx* c) { return c ? c->error.c_str() : g_createError.c_str(); }

int crt_bvh_build_host(const crt_mesh_view* meshes, uint32_t n_meshes, crt_bvh_node** nodes, uint32_t* n_nodes,
                       crt_bvh_tri** tris, crt_bvh_shade** shade, uint32_t* n_tris, uint32_t* max_depth)
{
    if ((!meshes && n_meshes) || !nodes || !n_nodes || !tris || !n_tris) return fail(nullptr, CRT_EINVAL, "crt_bvh_build_host: NULL argument");
    try {
        crt::Bvh b;
        crt::buildBvh(meshes, n_meshes, b);
        *n_nodes = static_cast<uint32_t>(b.nodes.size());
        *n_tris = static_cast<uint32_t>(b.tris.size());
        if (max_depth) *max_depth = b.maxDepth;
        *nodes = static_cast<crt_bvh_node*>(std::malloc(sizeof(crt_bvh_node) * (b.nodes.size() + 1)));
        *tris = static_cast<crt_bvh_tri*>(std::malloc(sizeof(crt_bvh_tri) * (b.tris.size() + 1)));
        if (shade) *shade = static_cast<crt_bvh_shade*>(std::malloc(sizeof(crt_bvh_shade) * (b.tris.size() + 1)));
        if (!*nodes || !*tris || (shade && !*shade)) return fail(nullptr, CRT_ENOMEM, "out of host memory");
        crt::copyBytes(*nodes, b.nodes.data(), sizeof(crt_bvh_node) * b.nodes.size());
        crt::copyBytes(*tris, b.tris.data(), sizeof(crt_bvh_tri) * b.tris.size());
        if (shade) crt::copyBytes(*shade, b.shade.data(), sizeof(crt_bvh_shade) * b.shade.size());
    } catch (const std::exception& ex) {
        return fail(nullptr, CRT_EINVAL, "BVH build failed: %s", ex.what());
    }
    return CRT_OK;
}

void crt_free(void* p) { std::free(p); }

void* crt_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void crt_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

int crt_upload_scene(crt_ctx* c, const crt_mesh_view* meshes, uint32_t n_meshes, const crt_light* lights, uint32_t n_lights,
                     const crt_material* materials, uint32_t n_materials)
{
    if (!c) return CRT_EINVAL;
    if ((!meshes && n_meshes) || (!lights && n_lights) || (!materials && n_materials)) return fail(c, CRT_EINVAL, "NULL array with non-zero count");
    const auto tb0 = std::chrono::steady_clock::now();
    double deviceMs = 0.0;
    crt::Bvh built; // swapped into the context only once the build has succeeded: a failed build leaves the old scene intact
    try {
        if (c->gpuBuild) {
            HIP_TRY(c, hipSetDevice(c->device));
            crt::buildBvhGpu(meshes, n_meshes, built, c->stream, &deviceMs, c->gpuBuilder);
        } else {
            crt::buildBvh(meshes, n_meshes, built);
        }
    } catch (const std::bad_alloc&) {
        return fail(c, CRT_ENOMEM, "out of host memory while building the BVH");
    } catch (const std::exception& ex) {
        return fail(c, CRT_EINVAL, "BVH build failed: %s", ex.what());
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize()); // frames in flight on any stream the caller used still read the old scene's buffers
    freeScene(c); // from here on a failure leaves NO scene (haveScene = false): never the new host tree over old device buffers
    crt::DeviceTree tree = std::move(built.dev); // (a failure before the context adopts it frees it with this call)
    const bool builtOnDevice = static_cast<bool>(tree.tris);
    std::swap(c->bvh, built);
    c->buildDeviceMs = deviceMs;
    if (!builtOnDevice) { // a host tree: what the kernels traverse goes to HBM, for a dynamic scene also what a refit starts from
        try {
            tree = crt::uploadTree(c->bvh, c->dynamicOpt);
        } catch (const std::exception& ex) {
            return fail(c, CRT_EHIP, "%s", ex.what());
        }
    }
    adoptTree(c, std::move(tree));
    if (c->bvh.dev.nNodes4 > 0) { // from the records in HBM, so a tree built on the device gets its table the same way
        HIP_TRY(c, hipMalloc(&c->dPlanes, sizeof(float) * crt::kPlaneStride * c->bvh.dev.nNodes4));
        HIP_TRY(c, static_cast<hipError_t>(crt::launchDecodePlanes(c->dNodes, c->bvh.dev.nNodes4, static_cast<float*>(c->dPlanes), nullptr)));
        HIP_TRY(c, hipDeviceSynchronize());
    }
    HIP_TRY(c, hipMalloc(&c->dLights, sizeof(crt_light) * (n_lights + 1)));
    HIP_TRY(c, hipMalloc(&c->dMats, sizeof(crt_material) * (n_materials + 1)));
    if (n_lights) HIP_TRY(c, hipMemcpy(c->dLights, lights, sizeof(crt_light) * n_lights, hipMemcpyHostToDevice));
    if (n_materials) HIP_TRY(c, hipMemcpy(c->dMats, materials, sizeof(crt_material) * n_materials, hipMemcpyHostToDevice));
    c->nLights = n_lights;
    c->nMats = n_materials;
    if (int rc = readSceneBox(c)) return rc; // (built here or on the device alike)
    if (c->dynamicOpt) {
        if (int rc = setupDynamic(c, meshes, n_meshes)) {
            freeScene(c);
            return rc;
        }
    }
    c->buildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count();
    c->haveScene = true;
    c->sceneSerial++;
    dropOrders(c);
    return CRT_OK;
}

int crt_set_textures(crt_ctx* c, const crt_texture* textures, uint32_t n)
{
    if (!c) return CRT_EINVAL;
    if (!textures && n) return fail(c, CRT_EINVAL, "crt_set_textures: NULL array with non-zero count");
    std::vector<crt::TextureRec> recs(n);
    std::vector<unsigned char> pool;
    for (uint32_t i = 0; i < n; i++) {
        const crt_texture& t = textures[i];
        if (t.type > 3u) return fail(c, CRT_EINVAL, "texture %u: unknown type %u", i, t.type);
        crt::TextureRec& r = recs[i];
        r.type = t.type;
        crt::copyBytes(r.a, t.color_a, 12);
        crt::copyBytes(r.b, t.color_b, 12);
        r.scalar = t.scalar;
        r.texel_offset = r.width = r.height = r.channels = 0;
        if (t.type == 3u) {
            if (!t.pixels || t.width == 0 || t.height == 0 || t.channels < 3)
                return fail(c, CRT_EINVAL, "texture %u: bitmap needs pixels, width, height and >= 3 channels", i);
            const size_t bytes = static_cast<size_t>(t.width) * t.height * t.channels;
            if (pool.size() + bytes > 0xFFFFFFFFull) return fail(c, CRT_EINVAL, "texture %u: more than 4 GiB of texels in one table", i);
            r.texel_offset = static_cast<uint32_t>(pool.size());
            r.width = t.width; r.height = t.height; r.channels = t.channels;
            pool.insert(pool.end(), t.pixels, t.pixels + bytes);
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    if (c->dTextures) (void)hipFree(c->dTextures);
    if (c->dTexels) (void)hipFree(c->dTexels);
    c->dTextures = c->dTexels = nullptr;
    c->nTextures = 0;
    c->textureSerial++; // accumulated sums of the old textures are stale
    HIP_TRY(c, hipMalloc(&c->dTextures, sizeof(crt::TextureRec) * (n + 1)));
    HIP_TRY(c, hipMalloc(&c->dTexels, pool.size() + 16));
    if (n) HIP_TRY(c, hipMemcpy(c->dTextures, recs.data(), sizeof(crt::TextureRec) * n, hipMemcpyHostToDevice));
    if (!pool.empty()) HIP_TRY(c, hipMemcpy(c->dTexels, pool.data(), pool.size(), hipMemcpyHostToDevice));
    c->nTextures = n;
    return CRT_OK;
}

int crt_bvh_export_uv(const crt_ctx* c, crt_bvh_uv* uvs, int* has_uvs)
{
    if (!c || !c->haveScene) return CRT_ESTATE;
    if (has_uvs) *has_uvs = c->dUvs ? 1 : 0;
    if (uvs && c->dUvs) { // (the host copy exists only for trees built on the host)
        if (!c->bvh.uvs.empty()) crt::copyBytes(uvs, c->bvh.uvs.data(), sizeof(crt_bvh_uv) * c->bvh.uvs.size());
        else if (hipMemcpy(uvs, c->dUvs, sizeof(crt_bvh_uv) * c->bvh.nTris, hipMemcpyDeviceToHost) != hipSuccess) return CRT_EHIP;
    }
    return CRT_OK;
}

int crt_set_camera(crt_ctx* c, const float pos[3], const float rot[9])
{
    if (!c) return CRT_EINVAL;
    if (!pos || !rot) return fail(c, CRT_EINVAL, "crt_set_camera: NULL argument");
    if (std::memcmp(c->pos, pos, sizeof(c->pos)) != 0 || std::memcmp(c->rot, rot, sizeof(c->rot)) != 0) c->viewSerial++;
    crt::copyBytes(c->pos, pos, sizeof(c->pos));
    crt::copyBytes(c->rot, rot, sizeof(c->rot));
    return CRT_OK;
}

int crt_set_shading_mode(crt_ctx* c, uint32_t mode)
{
    if (!c) return CRT_EINVAL;
    if (c->mode != mode) c->viewSerial++;
    c->mode = mode;
    return CRT_OK;
}

int crt_set_miss_color(crt_ctx* c, const float rgb[3])
{
    if (!c) return CRT_EINVAL;
    if (!rgb) return fail(c, CRT_EINVAL, "crt_set_miss_color: NULL argument");
    crt::copyBytes(c->miss, rgb, sizeof(c->miss));
    return CRT_OK;
}

int crt_set_counting(crt_ctx* c, int enabled)
{
    if (!c) return CRT_EINVAL;
    c->counting = enabled != 0;
    return CRT_OK;
}

int crt_set_option(crt_ctx* c, const char* name, int value)
{
    if (!c || !name) return CRT_EINVAL;
    for (const Option& o : kOptions) {
        if (std::strcmp(name, o.name) != 0) continue;
        if (!o.accepts(value)) {
            if (o.refusal) return fail(c, CRT_EINVAL, "%s", o.refusal);
            break;
        }
        o.store(*c, value);
        if (o.effect == kNewView) c->viewSerial++;
        if (o.effect == kDropOrders) dropOrders(c);
        return CRT_OK;
    }
#if !CRT_DIAG
    for (const char* diagnostic : { "debug_skip_units", "timeline", "debug_force_measure" })
        if (std::strcmp(name, diagnostic) == 0) return fail(c, CRT_EINVAL, "option '%s' exists only in the diagnostic build (tools/diag_build.sh)", name);
#endif
    return fail(c, CRT_EINVAL, "unknown option '%s' or value %d out of range", name, value);
}

int crt_debug_read_timeline(crt_ctx* c, unsigned long long* out, size_t max_words, size_t* n_words)
{
    if (!c || !out || !n_words) return CRT_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = c->timelineWords < max_words ? c->timelineWords : max_words;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n) HIP_TRY(c, hipMemcpy(out, c->dTimeline, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    *n_words = n;
    return CRT_OK;
}

int crt_debug_read_counters(crt_ctx* c, unsigned long long out[32])
{
    if (!c || !out) return CRT_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, c->dCounters, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_debug_list_phases(crt_ctx* c, double out_ms[4])
{
    if (!c || !out_ms) return CRT_EINVAL;
    std::memcpy(out_ms, c->listPhaseMs, sizeof(c->listPhaseMs));
    return CRT_OK;
}

int crt_debug_check_rcp(int device_id, unsigned long long out[8])
{
    if (!out) return fail(nullptr, CRT_EINVAL, "crt_debug_check_rcp: out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(nullptr, CRT_ENODEVICE, "no HIP device available");
    if (device_id < 0 || device_id >= n) return fail(nullptr, CRT_EINVAL, "device_id %d out of range [0,%d)", device_id, n);
    HIP_TRY(nullptr, hipSetDevice(device_id));
    unsigned long long init[8] = { 0, 0, 0, 0, 0, 0, ~0ull, 0 };
    unsigned long long* d = nullptr;
    HIP_TRY(nullptr, hipMalloc(reinterpret_cast<void**>(&d), sizeof(init)));
    hipError_t e = hipMemcpy(d, init, sizeof(init), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = static_cast<hipError_t>(crt::launchRcpCheck(d, nullptr));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d, sizeof(init), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(nullptr, CRT_EHIP, "crt_debug_check_rcp: %s", hipGetErrorString(e));
    return CRT_OK;
}

int crt_debug_wide_offsets(unsigned long long n_nodes, unsigned long long n_tris, int option)
{
    return crt::wideOffsets(n_nodes, n_tris, static_cast<uint32_t>(option)) ? 1 : 0;
}

int crt_set_stream(crt_ctx* c, void* hip_stream)
{
    if (!c) return CRT_EINVAL;
    c->stream = static_cast<hipStream_t>(hip_stream);
    return CRT_OK;
}

int crt_reset_stream(crt_ctx* c)
{
    if (!c) return CRT_EINVAL;
    c->stream = c->ownStream;
    return CRT_OK;
}

int crt_synchronize(crt_ctx* c)
{
    if (!c) return CRT_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

int crt_set_accumulation(crt_ctx* c, uint32_t max_samples)
{
    if (!c) return CRT_EINVAL;
    if (max_samples > (1u << 24)) return fail(c, CRT_EINVAL, "crt_set_accumulation: max_samples %u above 2^24", max_samples);
    c->accMax = max_samples;
    c->accSamples = 0u;
    if (max_samples == 0u && c->dAccum) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipDeviceSynchronize()); // frames in flight may still use the sums
        (void)hipFree(c->dAccum);
        c->dAccum = nullptr;
        c->accumBytes = 0;
    }
    return CRT_OK;
}

int crt_reset_accumulation(crt_ctx* c)
{
    if (!c) return CRT_EINVAL;
    c->accSamples = 0u;
    return CRT_OK;
}

int crt_accumulated_samples(const crt_ctx* c, uint32_t* samples)
{
    if (!c || !samples) return CRT_EINVAL;
    *samples = c->accMax ? c->accSamples : 0u;
    return CRT_OK;
}

namespace {

// Batched ray and point queries.  A query is n records of one kind (32-byte rays or 16-byte points) and up to seven outputs
// of a fixed size per record; every kind (crt::QueryKind) runs one persistent kernel over an arena of the context.
using crt::QueryKind;
constexpr int kQueryOutputs = 7; // the most any kind has (crt_shade_rays*)
// what an entry point asks for
struct QuerySpec {
    const char* what;
    QueryKind kind;
    void* out[kQueryOutputs]; // the kind's outputs in the order of its QueryShape; NULL = not wanted
    float beta = 0.0f;        // crt_winding_numbers*: travels with the call
};

// The parameter struct of a kind with an entry point of its own, each beginning with its QueryCommon (c), and what fills it
// from the call: d = the outputs as device pointers; innerMin = the scheduling knob the kind's traversal reads
union QueryParams {
    crt::QueryCommon c;
    crt::RayQueryParams ray;
    crt::PointQueryParams point;
    crt::WindingQueryParams winding;
    crt::ShadeQueryParams shade;
};
using QueryFill = int (*)(crt_ctx* c, const QuerySpec& s, void* const d[kQueryOutputs], QueryParams& p, uint32_t& innerMin);

// the closest-point search's absolute pruning margin: 2^-18 x the diagonal of the root box, rounded up
float pointPad(const crt_ctx* c)
{
    double dd = 0.0;
    for (int a = 0; a < 3; a++) {
        const double e = static_cast<double>(c->sceneHi[a]) - static_cast<double>(c->sceneLo[a]);
        dd += e * e;
    }
    return static_cast<float>(std::sqrt(dd) * 0x1p-18 * (1.0 + 0x1p-20));
}

// The moment table of the tree as it stands (crt_winding_numbers*, crt_winding_moments_export), built on the context's stream
// when there is none or the scene has changed since.  The scratch dies with the call, hence the wait.
int ensureMoments(crt_ctx* c)
{
    const uint32_t n4 = c->bvh.dev.nNodes4;
    if (c->dMoments && c->momentsNodes >= n4 && c->momentsSerial == c->sceneSerial) return CRT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->dMoments || c->momentsNodes < n4) {
        HIP_TRY(c, hipDeviceSynchronize()); // a query in flight on another stream may still read the old table
        if (c->dMoments) (void)hipFree(c->dMoments);
        c->dMoments = nullptr;
        c->momentsNodes = 0;
        HIP_TRY(c, hipMalloc(&c->dMoments, sizeof(float) * crt::kMomentStride * (n4 ? n4 : 1u)));
        c->momentsNodes = n4;
    }
    void* scratch = nullptr;
    HIP_TRY(c, hipMalloc(&scratch, crt::windingScratchBytes(n4)));
    hipError_t e = hipMemsetAsync(c->dMoments, 0, sizeof(float) * crt::kMomentStride * (n4 ? n4 : 1u), c->stream); // (nodes the root does not reach)
    if (e == hipSuccess) e = static_cast<hipError_t>(crt::launchWindingMoments(c->dNodes, c->dTris, n4, c->bvh.depth4, static_cast<float*>(c->dMoments), scratch, c->stream));
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(scratch);
    if (e != hipSuccess) return fail(c, CRT_EHIP, "winding moments: %s", hipGetErrorString(e));
    c->momentsSerial = c->sceneSerial;
    return CRT_OK;
}

// the scene's shading tables (sceneTables) and the context's shading state of a shaded query
void shadeTables(const crt_ctx* c, crt::ShadeQueryParams& q)
{
    sceneTables(c, q);
    q.mode = c->mode;
    q.phong_ks = static_cast<float>(c->phongKsPermille) / 1000.0f;
    q.phong_exp = c->phongExp;
}

int fillClosestHit(crt_ctx* c, const QuerySpec&, void* const d[kQueryOutputs], QueryParams& p, uint32_t& innerMin)
{
    p.ray.t = static_cast<float*>(d[0]);
    p.ray.uv = static_cast<float*>(d[1]);
    p.ray.inst = static_cast<uint32_t*>(d[2]);
    p.ray.prim = static_cast<uint32_t*>(d[3]);
    innerMin = c->tuneInnerMin;
    return CRT_OK;
}
int fillOcclusion(crt_ctx* c, const QuerySpec&, void* const d[kQueryOutputs], QueryParams& p, uint32_t& innerMin)
{
    p.ray.occluded = static_cast<unsigned char*>(d[0]);
    innerMin = c->tuneInnerMinAny;
    return CRT_OK;
}
int fillClosestPoint(crt_ctx* c, const QuerySpec&, void* const d[kQueryOutputs], QueryParams& p, uint32_t& innerMin)
{
    p.point.dist = static_cast<float*>(d[0]);
    p.point.point = static_cast<float*>(d[1]);
    p.point.uv = static_cast<float*>(d[2]);
    p.point.inst = static_cast<uint32_t*>(d[3]);
    p.point.prim = static_cast<uint32_t*>(d[4]);
    p.point.pad = pointPad(c);
    innerMin = c->tuneInnerMin;
    return CRT_OK;
}
int fillCount(crt_ctx* c, const QuerySpec&, void* const d[kQueryOutputs], QueryParams& p, uint32_t& innerMin)
{
    p.point.count = static_cast<uint32_t*>(d[0]);
    innerMin = c->tuneInnerMinAny;
    return CRT_OK;
}
int fillOccupancy(crt_ctx* c, const QuerySpec&, void* const d[kQueryOutputs], QueryParams& p, uint32_t& innerMin)
{
    p.point.inside = static_cast<unsigned char*>(d[0]);
    innerMin = c->tuneInnerMinAny;
    return CRT_OK;
}
// crt_shade_rays*: the closest hit and the context's shading mode at it (shade_kernels.hip)
int fillShade(crt_ctx* c, const QuerySpec&, void* const d[kQueryOutputs], QueryParams& p, uint32_t& innerMin)
{
    p.shade.rgb = static_cast<float*>(d[0]);
    p.shade.normal = static_cast<float*>(d[1]);
    p.shade.albedo = static_cast<float*>(d[2]);
    p.shade.t = static_cast<float*>(d[3]);
    p.shade.uv = static_cast<float*>(d[4]);
    p.shade.inst = static_cast<uint32_t*>(d[5]);
    p.shade.prim = static_cast<uint32_t*>(d[6]);
    shadeTables(c, p.shade);
    innerMin = c->tuneInnerMin;
    return CRT_OK;
}
// crt_winding_numbers*: the walk over the tree and its moment table (winding_kernels.hip)
int fillWinding(crt_ctx* c, const QuerySpec& s, void* const d[kQueryOutputs], QueryParams& p, uint32_t& innerMin)
{
    if (const int rc = ensureMoments(c)) return rc;
    p.winding.moments = static_cast<const float*>(c->dMoments);
    p.winding.beta = s.beta > 0.0f ? s.beta : 0.0f; // (a NaN too)
    p.winding.w = static_cast<float*>(d[0]);
    innerMin = c->tuneInnerMinAny;
    return CRT_OK;
}

// The static shape of a kind, by QueryKind: its records, its outputs in a fixed order and its fill.  (The listing's fill and
// the path-traced queries have no entry point that comes through a QuerySpec.)
struct QueryShape {
    uint32_t recordBytes;
    const char* outputNames; // for the alignment message
    struct {
        uint32_t bytes; // per record
        uint32_t align; // of a device pointer
    } out[kQueryOutputs];
    QueryFill fill;
};
const QueryShape kQueryShapes[crt::kQueryKinds] = {
    /* kQueryClosestHit */ { 32u, "t / uv / inst / prim", { { 4u, 4u }, { 8u, 8u }, { 4u, 4u }, { 4u, 4u } }, fillClosestHit },
    /* kQueryOcclusion */ { 32u, "occlusion", { { 1u, 1u } }, fillOcclusion },
    /* kQueryClosestPoint */
    { 16u, "dist / point / uv / inst / prim", { { 4u, 4u }, { 12u, 4u }, { 8u, 8u }, { 4u, 4u }, { 4u, 4u } }, fillClosestPoint },
    /* kQueryCount */ { 32u, "count", { { 4u, 4u } }, fillCount },
    /* kQueryOccupancy */ { 16u, "inside", { { 1u, 1u } }, fillOccupancy },
    /* kQueryListFill */ {},
    /* kQueryShade */
    { 32u, "rgb / normal / albedo / t / uv / inst / prim", { { 12u, 4u }, { 12u, 4u }, { 12u, 4u }, { 4u, 4u }, { 8u, 8u }, { 4u, 4u }, { 4u, 4u } }, fillShade },
    /* kQueryPath */ {},
    /* kQueryWinding */ { 16u, "w", { { 4u, 4u } }, fillWinding },
};

// what every query entry point checks before anything is launched.  A shaded query (crt_shade_rays*) promises that a failed
// call launches nothing: its refit follows its argument checks (queryDevice / queryHost) instead of coming here
int checkQuery(crt_ctx* c, const QuerySpec& s)
{
    const char* what = s.what;
    if (!c) return fail(nullptr, CRT_EINVAL, "%s: NULL context", what);
    if (!c->haveScene) return fail(c, CRT_ESTATE, "%s: no scene uploaded: call crt_upload_scene first", what);
    if (s.kind == crt::kQueryShade) {
        if (c->mode >= 200u)
            return fail(c, CRT_EINVAL, "%s: shading mode %u (path tracing) is not available for caller-supplied rays: set a mode below 200", what, c->mode);
        return CRT_OK;
    }
    return applyRefit(c, nullptr);
}

int checkOutputs(crt_ctx* c, const QuerySpec& s)
{
    for (const void* p : s.out)
        if (p) return CRT_OK;
    return fail(c, CRT_EINVAL, "%s: every output is NULL", s.what);
}

int checkDeviceOutputs(crt_ctx* c, const QuerySpec& s, const void* records)
{
    if (!records) return fail(c, CRT_EINVAL, "%s: record buffer is NULL", s.what);
    if (reinterpret_cast<uintptr_t>(records) & 15u) return fail(c, CRT_EINVAL, "%s: record buffer %p is not 16-byte aligned", s.what, records);
    if (const int rc = checkOutputs(c, s)) return rc;
    const QueryShape& shape = kQueryShapes[s.kind];
    for (int i = 0; i < kQueryOutputs; i++)
        if (s.out[i] && (reinterpret_cast<uintptr_t>(s.out[i]) & (shape.out[i].align - 1u)))
            return fail(c, CRT_EINVAL, "%s: output %p (%s) is not %u-byte aligned", s.what, s.out[i], shape.outputNames, shape.out[i].align);
    return CRT_OK;
}

// resident workgroups of the kind's kernel with the LDS stack the options ask for, from the context's cache; the persistent
// grid and the chunking of n records follow from it
int queryGrid(crt_ctx* c, QueryKind kind, uint32_t n, uint32_t& stack_entries, uint32_t& chunk, uint32_t& grid)
{
    stack_entries = c->tuneStackEntries ? c->tuneStackEntries : 16u; // as fillParams
    if (c->queryResident[kind] == 0u || c->queryResidentEntries[kind] != stack_entries) {
        c->queryResident[kind] = crt::queryResident(kind, stack_entries);
        c->queryResidentEntries[kind] = stack_entries;
        if (c->queryResident[kind] == 0u) return fail(c, CRT_EHIP, "query kernel: occupancy query failed");
    }
    crt::queryLayout(n, c->queryResident[kind], chunk, grid);
    return CRT_OK;
}

// What a query kernel gets from its arena: grid, chunking, cursor, counters and the stack spill arena
struct QueryLaunch {
    uint32_t stack_entries, spill_stride, chunk, grid;
    uint32_t* cursor;
    unsigned long long* counters;
    int* spill;
    unsigned char* extra; // extraBytes of the arena behind the spill area (256-byte aligned), or null
    crt_ctx::Arena* arena;
};

// One query of n > 0 records on the context's stream, in two halves around the kernel launch.  beginQuery sizes the persistent
// grid, takes an arena and (with stats) starts the timer.  endQuery takes the launch's HIP error code and, with stats,
// synchronises and fills them.
// extraBytes: scratch of the query's own with the arena's lifetime (an allocation failure is then CRT_ENOMEM); minGrid: the
// spill area is sized for at least that many workgroups (a query that runs a second persistent kernel over the same arena).
int beginQuery(crt_ctx* c, QueryKind kind, uint32_t n, crt_frame_stats* stats, QueryLaunch& ql, size_t extraBytes = 0, uint32_t minGrid = 0)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = queryGrid(c, kind, n, ql.stack_entries, ql.chunk, ql.grid)) return rc;
    const uint32_t deepest = 3u * c->bvh.depth4 + 1u; // as frameSpill
    ql.spill_stride = (deepest > ql.stack_entries ? deepest - ql.stack_entries : 1u) * crt::queryKernel(kind).entryWords;

    constexpr size_t kHead = 256; // cursor at 0, counters at 64
    const size_t spillBytes = up256(static_cast<size_t>(std::max(ql.grid, minGrid)) * 64u * ql.spill_stride * sizeof(int));
    crt_ctx::Arena* arena = nullptr;
    if (const int rc = takeArena(c, c->rayArena, kHead + spillBytes + extraBytes, ++c->raySerial, extraBytes != 0u, arena)) return rc;
    ql.extra = extraBytes ? arena->mem + kHead + spillBytes : nullptr;
    ql.cursor = reinterpret_cast<uint32_t*>(arena->mem);
    ql.counters = reinterpret_cast<unsigned long long*>(arena->mem + 64);
    ql.spill = reinterpret_cast<int*>(arena->mem + kHead);
    HIP_TRY(c, hipMemsetAsync(arena->mem, 0, kHead, c->stream));
    ql.arena = arena;
    if (stats) HIP_TRY(c, hipEventRecord(c->evStart, c->stream));
    return CRT_OK;
}

int endQuery(crt_ctx* c, QueryKind kind, uint32_t n, const QueryLaunch& ql, int rc, crt_frame_stats* stats)
{
    if (rc != 0) return fail(c, CRT_EHIP, "query kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
    if (stats) HIP_TRY(c, hipEventRecord(c->evStop, c->stream));
    HIP_TRY(c, ql.arena->lastUse.record(c->stream));
    if (!stats) return CRT_OK;
    unsigned long long words[4]; // (zeros unless counting is on)
    if (const int rs = readStats(c, stats, ql.counters, words)) return rs;
    if (kind == crt::kQueryOcclusion) stats->rays_shadow = n;
    else stats->rays_primary = kind == crt::kQueryOccupancy ? 3ull * n : n;
    if (c->counting && (kind == crt::kQueryShade || kind == crt::kQueryPath)) stats->rays_shadow = words[2]; // the shadow rays traced (mode 100; paths)
    if (kind == crt::kQueryPath) stats->rays_primary += words[3];                                      // the bounce rays of the paths
    return CRT_OK;
}

// the part of a query kernel's parameters every kind shares, from the context and the launch
crt::QueryCommon queryCommon(const crt_ctx* c, const QueryLaunch& ql, const void* d_records, uint32_t n, uint32_t inner_min)
{
    crt::QueryCommon q;
    q.nodes = c->dNodes;
    q.tris = c->dTris;
    q.n_nodes = c->bvh.dev.nNodes4;
    q.records = d_records;
    q.n = n;
    q.cursor = ql.cursor;
    q.counters = ql.counters;
    q.spill = ql.spill;
    q.spill_stride = ql.spill_stride;
    q.stack_entries = ql.stack_entries;
    q.inner_min = inner_min;
    q.chunk = ql.chunk;
    return q;
}

// a query of any kind with an entry point: its fill, then one launch between beginQuery and endQuery
int runKind(crt_ctx* c, const QuerySpec& s, uint32_t n, const void* d_records, void* const d[kQueryOutputs], crt_frame_stats* stats)
{
    QueryParams p;
    std::memset(&p, 0, sizeof(p));
    uint32_t innerMin = 0;
    if (const int rc = kQueryShapes[s.kind].fill(c, s, d, p, innerMin)) return rc;
    QueryLaunch ql;
    if (const int rc = beginQuery(c, s.kind, n, stats, ql)) return rc;
    p.c = queryCommon(c, ql, d_records, n, innerMin);
    return endQuery(c, s.kind, n, ql, crt::launchQuery(s.kind, &p, c->counting, ql.grid, c->stream), stats);
}

void zeroStats(crt_frame_stats* stats, std::chrono::steady_clock::time_point t0)
{
    if (!stats) return;
    std::memset(stats, 0, sizeof(*stats));
    stampTotal(stats, t0);
}

int queryDevice(crt_ctx* c, const QuerySpec& s, uint32_t n, const void* d_records, crt_frame_stats* stats)
{
    int rc = checkQuery(c, s);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (n == 0u) { // nothing to look at, nothing launched
        zeroStats(stats, t0);
        return CRT_OK;
    }
    if ((rc = checkDeviceOutputs(c, s, d_records)) != CRT_OK) return rc;
    if (s.kind == crt::kQueryShade && (rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    if ((rc = runKind(c, s, n, d_records, s.out, stats)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// host buffers: staged through the context's device buffer {records | outputs in order}; synchronous
int queryHost(crt_ctx* c, const QuerySpec& s, uint32_t n, const float* records, crt_frame_stats* stats)
{
    int rc = checkQuery(c, s);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (n == 0u) {
        zeroStats(stats, t0);
        return CRT_OK;
    }
    if (!records) return fail(c, CRT_EINVAL, "%s: record buffer is NULL", s.what);
    if ((rc = checkOutputs(c, s)) != CRT_OK) return rc;
    if (s.kind == crt::kQueryShade && (rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    constexpr int kPlanes = 1 + kQueryOutputs;
    const QueryShape& shape = kQueryShapes[s.kind];
    StagePlane planes[kPlanes] = { { records, nullptr, static_cast<size_t>(n) * shape.recordBytes } };
    for (int i = 0; i < kQueryOutputs; i++) planes[1 + i] = { nullptr, s.out[i], static_cast<size_t>(n) * shape.out[i].bytes };
    void* dev[kPlanes];
    if ((rc = stageBegin(c, planes, kPlanes, dev)) != CRT_OK) return rc;
    crt_frame_stats local;
    if ((rc = runKind(c, s, n, dev[0], dev + 1, stats ? stats : &local)) != CRT_OK) return rc;
    if ((rc = stageEnd(c, planes, kPlanes, dev)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// ---- crt_path_rays*: the frames' mode-200 paths for caller records (path_query_kernels.hip).  Work items are (record, sample)
// pairs; a launch covers at most "path_pass_paths" of them (all records x a range of samples; a buffer of more records than
// that is also cut into blocks of records), each followed by the resolve that adds the pass's samples to the running sums.
// Everything runs over one arena between one beginQuery and one endQuery: the radiance and throughput slots and, when the
// caller gave no sums and there is more than one pass, the n x 3 float64 sums between the passes.
struct PathCall {
    const void* rays;
    const uint32_t* ids;
    uint32_t first, samples;
    float* rgb;
    double* sums;
    float* t;
    float* uv;
    uint32_t* inst;
    uint32_t* prim;
    bool anyOutput() const { return rgb || sums || t || uv || inst || prim; }
};

// the checks that need no buffer; n = 0 ends the call after them
int checkPathCall(crt_ctx* c, const char* what, uint32_t first, uint32_t samples)
{
    if (!c) return fail(nullptr, CRT_EINVAL, "%s: NULL context", what);
    if (!c->haveScene) return fail(c, CRT_ESTATE, "%s: no scene uploaded: call crt_upload_scene first", what);
    if (samples == 0u) return fail(c, CRT_EINVAL, "%s: n_samples is 0", what);
    if (static_cast<uint64_t>(first) + samples > (1ull << 24))
        return fail(c, CRT_EINVAL, "%s: first_sample + n_samples = %llu exceeds 2^24", what, static_cast<unsigned long long>(first) + samples);
    return CRT_OK;
}

int runPathQuery(crt_ctx* c, uint32_t n, const PathCall& a, crt_frame_stats* stats)
{
    const uint32_t cap = c->tunePathPassPaths;
    const uint32_t blockRecords = std::min(n, cap);
    const uint32_t passSamples = std::max(1u, std::min(a.samples, cap / blockRecords));
    const size_t slots = static_cast<size_t>(blockRecords) * passSamples; // <= cap <= 2^25
    const bool keepSums = passSamples < a.samples && !a.sums && a.rgb;
    const size_t slotBytes = up256(slots * 16u), sumBytes = keepSums ? up256(static_cast<size_t>(blockRecords) * 24u) : 0u;

    crt::PathQueryParams q;
    std::memset(&q, 0, sizeof(q));
    sceneTables(c, q);
    q.max_bounces = c->pathBounces;
    q.seed = c->pathSeed;
    QueryLaunch ql;
    if (const int rc = beginQuery(c, crt::kQueryPath, static_cast<uint32_t>(slots), stats, ql, 2u * slotBytes + sumBytes)) return rc;
    q.rad = ql.extra;
    q.thr = ql.extra + slotBytes;
    double* kept = keepSums ? reinterpret_cast<double*>(ql.extra + 2u * slotBytes) : nullptr;

    int hrc = 0;
    bool launched = false;
    for (uint64_t r0 = 0; r0 < n && hrc == 0; r0 += blockRecords) {
        const uint32_t nr = static_cast<uint32_t>(std::min<uint64_t>(blockRecords, n - r0));
        double* sums = a.sums ? a.sums + 3u * r0 : nullptr;
        double* running = sums ? sums : kept;
        for (uint32_t s0 = 0; s0 < a.samples && hrc == 0; s0 += passSamples) {
            const uint32_t ns = std::min(passSamples, a.samples - s0);
            const uint32_t items = nr * ns;
            if (launched) HIP_TRY(c, hipMemsetAsync(ql.cursor, 0, sizeof(uint32_t), c->stream)); // (the counters go on counting)
            launched = true;
            uint32_t chunk = 0, grid = 0;
            crt::queryLayout(items, c->queryResident[crt::kQueryPath], chunk, grid);
            grid = std::min(grid, ql.grid); // (the spill area is sized for ql.grid workgroups, the largest pass's)
            q.c = queryCommon(c, ql, static_cast<const unsigned char*>(a.rays) + 32u * r0, items, c->tuneInnerMin);
            q.c.chunk = chunk;
            q.ids = a.ids ? a.ids + r0 : nullptr;
            q.id_base = static_cast<uint32_t>(r0);
            q.n_records = nr;
            q.sample0 = a.first + s0;
            const bool firstPass = s0 == 0u, lastPass = s0 + ns == a.samples;
            q.t = firstPass && a.t ? a.t + r0 : nullptr;
            q.uv = firstPass && a.uv ? a.uv + 2u * r0 : nullptr;
            q.inst = firstPass && a.inst ? a.inst + r0 : nullptr;
            q.prim = firstPass && a.prim ? a.prim + r0 : nullptr;
            hrc = crt::launchQuery(crt::kQueryPath, &q, c->counting, grid, c->stream);
            if (hrc == 0 && (a.rgb || a.sums)) {
                const double* in = firstPass ? (sums && a.first > 0u ? sums : nullptr) : running;
                double* out = lastPass ? sums : running;
                float* rgb = lastPass && a.rgb ? a.rgb + 3u * r0 : nullptr;
                hrc = crt::launchPathResolve(q.rad, nr, ns, in, out, rgb, a.sums ? a.first + a.samples : a.samples, c->stream);
            }
        }
    }
    if (const int rc = endQuery(c, crt::kQueryPath, 0u, ql, hrc, stats)) return rc;
    if (stats) stats->rays_primary += static_cast<uint64_t>(n) * a.samples; // (endQuery: the bounce rays, with counting)
    return CRT_OK;
}

// ---- all-hits listing (crt_list_hits*): count -> scan -> fill -> sort + resolve over one arena, between one beginQuery and
// one endQuery.  The counts (reused as the sort's queue of long rays), the scan's tile sums and the key scratch live in the
// arena, so that a second listing on another stream gets its own.

struct ListRun {
    QueryLaunch ql;
    crt::ListParams q;
    uint32_t fillGrid = 0, fillChunk = 0;
    unsigned char* keyScratch = nullptr;
    bool timed = false; // stats were asked for: the phases are bracketed by the context's evList
};

int listMark(crt_ctx* c, const ListRun& lr, int i)
{
    return lr.timed ? static_cast<int>(hipEventRecord(c->evList[i], c->stream)) : 0;
}

// count + scan.  keyBytes: scratch wanted behind the counts and the tile sums (device form: work arrays the caller did not supply)
int listBegin(crt_ctx* c, uint32_t n, const void* d_rays, void* d_offsets, size_t keyBytes, crt_frame_stats* stats, ListRun& lr)
{
    HIP_TRY(c, hipSetDevice(c->device));
    uint32_t entries = 0;
    if (const int rc = queryGrid(c, crt::kQueryListFill, n, entries, lr.fillChunk, lr.fillGrid)) return rc;
    lr.timed = stats != nullptr;
    if (lr.timed)
        for (hipEvent_t& e : c->evList)
            if (!e) HIP_TRY(c, hipEventCreate(&e));
    const size_t countBytes = up256(static_cast<size_t>(n) * sizeof(uint32_t)), scanBytes = up256(crt::listScanScratchBytes(n));
    if (const int rc = beginQuery(c, crt::kQueryCount, n, stats, lr.ql, countBytes + scanBytes + keyBytes, lr.fillGrid)) return rc;
    const QueryLaunch& ql = lr.ql;
    uint32_t* counts = reinterpret_cast<uint32_t*>(ql.extra);
    unsigned long long* tileSums = reinterpret_cast<unsigned long long*>(ql.extra + countBytes);
    lr.keyScratch = ql.extra + countBytes + scanBytes;

    crt::PointQueryParams pq;
    std::memset(&pq, 0, sizeof(pq));
    pq.c = queryCommon(c, ql, d_rays, n, c->tuneInnerMinAny);
    pq.count = counts;

    crt::ListParams& q = lr.q;
    std::memset(&q, 0, sizeof(q));
    q.c = pq.c;
    q.c.chunk = lr.fillChunk; // (the fill's own grid and chunking; everything else as the count)
    q.offsets = static_cast<const unsigned long long*>(d_offsets);
    q.longRays = counts;
    q.longCount = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(ql.cursor) + 128); // in the arena's zeroed head
    q.short_max = c->tuneListShortMax;

    int rc = listMark(c, lr, 0);
    if (rc == 0) rc = crt::launchQuery(crt::kQueryCount, &pq, c->counting, ql.grid, c->stream);
    if (rc == 0) rc = listMark(c, lr, 1);
    if (rc == 0) rc = crt::launchListScan(counts, n, static_cast<unsigned long long*>(d_offsets), tileSums, c->stream);
    if (rc == 0) rc = listMark(c, lr, 2);
    return rc == 0 ? CRT_OK : endQuery(c, crt::kQueryCount, n, ql, rc, nullptr);
}

// fill + sort + resolve into the record arrays: the cursor (not the counters) starts again for the second traversal
int listFill(crt_ctx* c, ListRun& lr, unsigned long long capacity, float* tkey, uint32_t* idkey, void* const out[4])
{
    crt::ListParams& q = lr.q;
    q.capacity = capacity;
    q.tkey = tkey;
    q.idkey = idkey;
    q.t = static_cast<float*>(out[0]);
    q.uv = static_cast<float*>(out[1]);
    q.inst = static_cast<uint32_t*>(out[2]);
    q.prim = static_cast<uint32_t*>(out[3]);
    const hipError_t e = hipMemsetAsync(q.c.cursor, 0, sizeof(uint32_t), c->stream);
    if (e != hipSuccess) return static_cast<int>(e);
    int rc = crt::launchQuery(crt::kQueryListFill, &q, c->counting, lr.fillGrid, c->stream);
    if (rc == 0) rc = listMark(c, lr, 3);
    if (rc == 0) rc = crt::launchListSort(q, c->stream);
    if (rc == 0) rc = listMark(c, lr, 4);
    return rc;
}

// after endQuery has synchronised a timed listing: the phases' HIP-event times (fill and sort 0 when they did not run)
int listPhases(crt_ctx* c, const ListRun& lr, bool filled)
{
    if (!lr.timed) return CRT_OK;
    for (int i = 0; i < 4; i++) {
        float ms = 0.f;
        if (i < 2 || filled) HIP_TRY(c, hipEventElapsedTime(&ms, c->evList[i], c->evList[i + 1]));
        c->listPhaseMs[i] = ms;
    }
    return CRT_OK;
}

int listCheck(crt_ctx* c, const char* what, uint32_t n, const void* rays, const void* offsets, std::chrono::steady_clock::time_point t0,
              uint64_t* total, crt_frame_stats* stats, bool& done)
{
    done = false;
    if (!c) return fail(nullptr, CRT_EINVAL, "%s: NULL context", what);
    if (!c->haveScene) return fail(c, CRT_ESTATE, "%s: no scene uploaded: call crt_upload_scene first", what);
    if (n == 0u) {
        zeroStats(stats, t0);
        if (total) *total = 0u;
        done = true;
        return CRT_OK;
    }
    if (!rays) return fail(c, CRT_EINVAL, "%s: ray buffer is NULL", what);
    if (!offsets) return fail(c, CRT_EINVAL, "%s: offsets is NULL", what);
    return CRT_OK; // (the caller applies pending refits once its own argument checks are through: a failed call launches nothing)
}

} // namespace

int crt_trace_rays_device(crt_ctx* c, uint32_t n, const void* d_rays, void* d_t, void* d_uv, void* d_inst, void* d_prim, crt_frame_stats* stats)
{
    return queryDevice(c, { "crt_trace_rays_device", crt::kQueryClosestHit, { d_t, d_uv, d_inst, d_prim } }, n, d_rays, stats);
}

int crt_occluded_rays_device(crt_ctx* c, uint32_t n, const void* d_rays, void* d_occluded, crt_frame_stats* stats)
{
    return queryDevice(c, { "crt_occluded_rays_device", crt::kQueryOcclusion, { d_occluded } }, n, d_rays, stats);
}

int crt_trace_rays(crt_ctx* c, uint32_t n, const float* rays, float* t, float* uv, uint32_t* inst, uint32_t* prim, crt_frame_stats* stats)
{
    return queryHost(c, { "crt_trace_rays", crt::kQueryClosestHit, { t, uv, inst, prim } }, n, rays, stats);
}

int crt_occluded_rays(crt_ctx* c, uint32_t n, const float* rays, uint8_t* occluded, crt_frame_stats* stats)
{
    return queryHost(c, { "crt_occluded_rays", crt::kQueryOcclusion, { occluded } }, n, rays, stats);
}

int crt_shade_rays_device(crt_ctx* c, uint32_t n, const void* d_rays, void* d_rgb, void* d_normal, void* d_albedo, void* d_t, void* d_uv,
                          void* d_inst, void* d_prim, crt_frame_stats* stats)
{
    return queryDevice(c, { "crt_shade_rays_device", crt::kQueryShade, { d_rgb, d_normal, d_albedo, d_t, d_uv, d_inst, d_prim } }, n, d_rays, stats);
}

int crt_shade_rays(crt_ctx* c, uint32_t n, const float* rays, float* rgb, float* normal, float* albedo, float* t, float* uv, uint32_t* inst,
                   uint32_t* prim, crt_frame_stats* stats)
{
    return queryHost(c, { "crt_shade_rays", crt::kQueryShade, { rgb, normal, albedo, t, uv, inst, prim } }, n, rays, stats);
}

int crt_path_rays_device(crt_ctx* c, uint32_t n, const void* d_rays, const void* d_ids, uint32_t first_sample, uint32_t n_samples, void* d_rgb,
                         void* d_sums, void* d_t, void* d_uv, void* d_inst, void* d_prim, crt_frame_stats* stats)
{
    const char* what = "crt_path_rays_device";
    int rc = checkPathCall(c, what, first_sample, n_samples);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (n == 0u) { // nothing to look at, nothing launched
        zeroStats(stats, t0);
        return CRT_OK;
    }
    const PathCall a{ d_rays, static_cast<const uint32_t*>(d_ids), first_sample, n_samples, static_cast<float*>(d_rgb), static_cast<double*>(d_sums),
                      static_cast<float*>(d_t), static_cast<float*>(d_uv), static_cast<uint32_t*>(d_inst), static_cast<uint32_t*>(d_prim) };
    if (!d_rays) return fail(c, CRT_EINVAL, "%s: record buffer is NULL", what);
    if (!a.anyOutput()) return fail(c, CRT_EINVAL, "%s: every output is NULL", what);
    const struct { const void* p; uintptr_t align; const char* name; } ptrs[] = { { d_rays, 16u, "rays" }, { d_ids, 4u, "ids" }, { d_rgb, 4u, "rgb" },
        { d_sums, 8u, "sums" }, { d_t, 4u, "t" }, { d_uv, 8u, "uv" }, { d_inst, 4u, "inst" }, { d_prim, 4u, "prim" } };
    for (const auto& p : ptrs)
        if (reinterpret_cast<uintptr_t>(p.p) & (p.align - 1u))
            return fail(c, CRT_EINVAL, "%s: %s buffer %p is not %u-byte aligned", what, p.name, p.p, static_cast<unsigned>(p.align));
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    if ((rc = runPathQuery(c, n, a, stats)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// host buffers: staged through the context's query staging buffer {rays | ids | sums | rgb | t | uv | inst | prim}; synchronous
int crt_path_rays(crt_ctx* c, uint32_t n, const float* rays, const uint32_t* ids, uint32_t first_sample, uint32_t n_samples, float* rgb,
                  double* sums, float* t, float* uv, uint32_t* inst, uint32_t* prim, crt_frame_stats* stats)
{
    const char* what = "crt_path_rays";
    int rc = checkPathCall(c, what, first_sample, n_samples);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (n == 0u) {
        zeroStats(stats, t0);
        return CRT_OK;
    }
    if (!rays) return fail(c, CRT_EINVAL, "%s: record buffer is NULL", what);
    if (!(rgb || sums || t || uv || inst || prim)) return fail(c, CRT_EINVAL, "%s: every output is NULL", what);
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    const size_t nn = n;
    // (the sums a first call starts are not read)
    const StagePlane planes[8] = { { rays, nullptr, nn * 32u }, { ids, nullptr, nn * 4u }, { first_sample > 0u ? sums : nullptr, sums, nn * 24u },
                                   { nullptr, rgb, nn * 12u }, { nullptr, t, nn * 4u }, { nullptr, uv, nn * 8u }, { nullptr, inst, nn * 4u },
                                   { nullptr, prim, nn * 4u } };
    void* dev[8];
    if ((rc = stageBegin(c, planes, 8, dev)) != CRT_OK) return rc;
    const PathCall a{ dev[0], static_cast<const uint32_t*>(dev[1]), first_sample, n_samples, static_cast<float*>(dev[3]), static_cast<double*>(dev[2]),
                      static_cast<float*>(dev[4]), static_cast<float*>(dev[5]), static_cast<uint32_t*>(dev[6]), static_cast<uint32_t*>(dev[7]) };
    crt_frame_stats local;
    if ((rc = runPathQuery(c, n, a, stats ? stats : &local)) != CRT_OK) return rc;
    if ((rc = stageEnd(c, planes, 8, dev)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

namespace {

// ---- camera rays, frame guides and the denoiser (camera_kernels.hip, denoise_kernels.hip)
constexpr uint64_t kMaxFramePixels = 1ull << 28;

int checkFrameSize(crt_ctx* c, const char* what, uint32_t w, uint32_t h)
{
    if (w == 0u || h == 0u) return fail(c, CRT_EINVAL, "%s: frame size %u x %u", what, w, h);
    if (static_cast<uint64_t>(w) * h > kMaxFramePixels) return fail(c, CRT_EINVAL, "%s: %u x %u exceeds 2^28 pixels", what, w, h);
    return CRT_OK;
}

int checkDevicePointers(crt_ctx* c, const char* what, std::initializer_list<const void*> ptrs, uintptr_t align)
{
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & (align - 1u))
            return fail(c, CRT_EINVAL, "%s: buffer %p is not %u-byte aligned", what, p, static_cast<unsigned>(align));
    return CRT_OK;
}

crt::CameraRayParams cameraRayParams(const crt_ctx* c, uint32_t w, uint32_t h, uint32_t sample, void* d_rays)
{
    crt::CameraRayParams p;
    std::memset(&p, 0, sizeof(p));
    crt::copyBytes(p.pos, c->pos, sizeof(p.pos));
    crt::copyBytes(p.rot, c->rot, sizeof(p.rot));
    p.width = w;
    p.height = h;
    p.sample = sample;
    p.seed = c->pathSeed;
    p.rays = d_rays;
    return p;
}

int checkCameraRays(crt_ctx* c, const char* what, uint32_t w, uint32_t h, uint32_t sample, const void* rays)
{
    if (!c) return fail(nullptr, CRT_EINVAL, "%s: NULL context", what);
    if (const int rc = checkFrameSize(c, what, w, h)) return rc;
    if (sample != CRT_SAMPLE_CENTRE && sample >= (1u << 24)) return fail(c, CRT_EINVAL, "%s: sample %u is neither below 2^24 nor CRT_SAMPLE_CENTRE", what, sample);
    if (!rays) return fail(c, CRT_EINVAL, "%s: record buffer is NULL", what);
    return CRT_OK;
}

// kernels that need no arena, timed when stats are wanted: `launch` returns a HIP error code.  With stats the call synchronises
// and every count is zero
int runTimed(crt_ctx* c, const char* what, crt_frame_stats* stats, const std::function<int()>& launch)
{
    if (stats) HIP_TRY(c, hipEventRecord(c->evStart, c->stream));
    const int hrc = launch();
    if (hrc != 0) return fail(c, CRT_EHIP, "%s: kernel launch failed: %s", what, hipGetErrorString(static_cast<hipError_t>(hrc)));
    if (!stats) return CRT_OK;
    HIP_TRY(c, hipEventRecord(c->evStop, c->stream));
    return readStats(c, stats);
}

int runCameraRays(crt_ctx* c, const char* what, uint32_t w, uint32_t h, uint32_t sample, void* d_rays, crt_frame_stats* stats)
{
    const crt::CameraRayParams p = cameraRayParams(c, w, h, sample, d_rays);
    if (const int rc = runTimed(c, what, stats, [&] { return crt::launchCameraRays(p, c->stream); })) return rc;
    if (stats) stats->rays_primary = static_cast<uint64_t>(w) * h;
    return CRT_OK;
}

// crt_frame_guides*: the camera-ray kernel into the query arena, then the shaded query over those records in a debug mode
// (the surface is evaluated for normal / albedo in every mode; no colour is asked for)
int runFrameGuides(crt_ctx* c, uint32_t w, uint32_t h, void* d_normal, void* d_albedo, void* d_t, crt_frame_stats* stats)
{
    const uint32_t n = w * h;
    crt::ShadeQueryParams q;
    std::memset(&q, 0, sizeof(q));
    shadeTables(c, q);
    q.mode = 3u;
    q.normal = static_cast<float*>(d_normal);
    q.albedo = static_cast<float*>(d_albedo);
    q.t = static_cast<float*>(d_t);
    QueryLaunch ql;
    if (const int rc = beginQuery(c, crt::kQueryShade, n, stats, ql, up256(static_cast<size_t>(n) * 32u))) return rc;
    int hrc = crt::launchCameraRays(cameraRayParams(c, w, h, CRT_SAMPLE_CENTRE, ql.extra), c->stream);
    if (hrc == 0) {
        q.c = queryCommon(c, ql, ql.extra, n, c->tuneInnerMin);
        hrc = crt::launchQuery(crt::kQueryShade, &q, c->counting, ql.grid, c->stream);
    }
    return endQuery(c, crt::kQueryShade, n, ql, hrc, stats);
}

int checkFrameGuides(crt_ctx* c, const char* what, uint32_t w, uint32_t h, const void* normal, const void* albedo, const void* t)
{
    if (!c) return fail(nullptr, CRT_EINVAL, "%s: NULL context", what);
    if (!c->haveScene) return fail(c, CRT_ESTATE, "%s: no scene uploaded: call crt_upload_scene first", what);
    if (const int rc = checkFrameSize(c, what, w, h)) return rc;
    if (!normal && !albedo && !t) return fail(c, CRT_EINVAL, "%s: every output is NULL", what);
    return CRT_OK;
}

// ---- the a-trous filters (denoise_kernels.hip).  crt_denoise* and crt_denoise_variance* are one call: `guided` says which, and
// the plain filter is the one without variance planes, its sigma_color where the guided one has sigma_luminance
const crt_denoise_params kDenoiseDefaults = { 5u, 4.0f, 0.3f, 0.05f, 1u };
const crt_denoise_variance_params kDenoiseVarianceDefaults = { 5u, 0.0625f, 0.3f, 0.05f, 1u };

int checkDenoise(crt_ctx* c, const char* what, bool guided, uint32_t w, uint32_t h, const void* rgb, const void* normal, const void* albedo,
                 const void* t, const void* variance, const void* out, const crt_denoise_params& prm)
{
    if (!c) return fail(nullptr, CRT_EINVAL, "%s: NULL context", what);
    if (guided && !(prm.sigma_color > 0.0f))
        return fail(c, CRT_EINVAL, "%s: sigma_luminance = %g must be > 0 (+inf switches the term off)", what, static_cast<double>(prm.sigma_color));
    if (const int rc = checkFrameSize(c, what, w, h)) return rc;
    if (prm.iterations < 1u || prm.iterations > 8u) return fail(c, CRT_EINVAL, "%s: iterations = %u is outside 1..8", what, prm.iterations);
    const struct { const char* name; float v; } sig[] = { { "sigma_color", prm.sigma_color }, { "sigma_normal", prm.sigma_normal }, { "sigma_depth", prm.sigma_depth } };
    for (const auto& s : sig)
        if (!(s.v > 0.0f)) return fail(c, CRT_EINVAL, "%s: %s = %g must be > 0 (+inf switches the term off)", what, s.name, static_cast<double>(s.v));
    if (prm.demodulate > 1u) return fail(c, CRT_EINVAL, "%s: demodulate = %u is neither 0 nor 1", what, prm.demodulate);
    if (!rgb || !normal || !albedo || !t || !out || (guided && !variance)) return fail(c, CRT_EINVAL, "%s: NULL buffer", what);
    return CRT_OK;
}

// 1 / sigma^2 as the kernels take it: 0 for +inf, never infinite (0 x inf would poison a tap of equal value)
float invSquare(float sigma)
{
    const double s = static_cast<double>(sigma);
    return static_cast<float>(std::min(1.0 / (s * s), static_cast<double>(FLT_MAX)));
}

// the stream's query arena as three float4 planes {guide, colour[0], colour[1]}, the launch, and the arena's last use, recorded
// before a timed call synchronises
int runDenoise(crt_ctx* c, const char* what, uint32_t w, uint32_t h, const void* d_rgb, const void* d_normal, const void* d_albedo, const void* d_t,
               const void* d_variance, void* d_out, void* d_varianceOut, const crt_denoise_params& prm, crt_frame_stats* stats)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t plane = up256(static_cast<size_t>(w) * h * 16u);
    static_assert(crt::kDenoiseScratchPerPixel == 48u, "three float4 planes");
    crt_ctx::Arena* arena = nullptr;
    if (const int rc = takeArena(c, c->rayArena, 3u * plane, ++c->raySerial, true, arena)) return rc;
    crt::DenoiseParams p;
    std::memset(&p, 0, sizeof(p));
    p.width = w;
    p.height = h;
    p.iterations = prm.iterations;
    p.demodulate = prm.demodulate;
    p.sigma_first = d_variance ? prm.sigma_color : invSquare(prm.sigma_color);
    p.inv_sigma_normal2 = invSquare(prm.sigma_normal);
    p.sigma_depth = prm.sigma_depth;
    p.rgb = static_cast<const float*>(d_rgb);
    p.normal = static_cast<const float*>(d_normal);
    p.albedo = static_cast<const float*>(d_albedo);
    p.t = static_cast<const float*>(d_t);
    p.variance = static_cast<const float*>(d_variance);
    p.out = static_cast<float*>(d_out);
    p.varianceOut = static_cast<float*>(d_varianceOut);
    p.guide = arena->mem;
    p.colour[0] = arena->mem + plane;
    p.colour[1] = arena->mem + 2u * plane;
    return runTimed(c, what, stats, [&] {
        const int hrc = crt::launchDenoise(p, c->stream);
        if (hrc != 0) return hrc;
        return static_cast<int>(arena->lastUse.record(c->stream));
    });
}

// The device forms ...
static int denoiseDevice(crt_ctx* c, const char* what, bool guided, uint32_t w, uint32_t h, const void* d_rgb, const void* d_normal,
                         const void* d_albedo, const void* d_t, const void* d_variance, void* d_out, void* d_varianceOut,
                         const crt_denoise_params& prm, crt_frame_stats* stats)
{
    int rc = checkDenoise(c, what, guided, w, h, d_rgb, d_normal, d_albedo, d_t, d_variance, d_out, prm);
    if (rc) return rc;
    if ((rc = checkDevicePointers(c, what, { d_rgb, d_normal, d_albedo, d_t, d_variance, d_out, d_varianceOut }, 4u)) != CRT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = runDenoise(c, what, w, h, d_rgb, d_normal, d_albedo, d_t, d_variance, d_out, d_varianceOut, prm, stats)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// ... and the host forms: staged through the context's query staging buffer {rgb | normal | albedo | t | variance}, filtered in
// place; synchronous
static int denoiseHost(crt_ctx* c, const char* what, bool guided, uint32_t w, uint32_t h, const float* rgb, const float* normal,
                       const float* albedo, const float* t, const float* variance, float* out, float* varianceOut,
                       const crt_denoise_params& prm, crt_frame_stats* stats)
{
    int rc = checkDenoise(c, what, guided, w, h, rgb, normal, albedo, t, variance, out, prm);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t nn = static_cast<size_t>(w) * h;
    const StagePlane planes[7] = { { rgb, nullptr, nn * 12u }, { normal, nullptr, nn * 12u }, { albedo, nullptr, nn * 12u }, { t, nullptr, nn * 4u },
                                   { variance, nullptr, nn * 4u }, { nullptr, out, nn * 12u, 0 }, { nullptr, varianceOut, nn * 4u, 4 } };
    void* dev[7];
    if ((rc = stageBegin(c, planes, 7, dev)) != CRT_OK) return rc;
    if ((rc = runDenoise(c, what, w, h, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], prm, stats)) != CRT_OK) return rc;
    if ((rc = stageEnd(c, planes, 7, dev)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// the guided filter's parameters in the plain filter's struct
static crt_denoise_params guidedParams(const crt_denoise_variance_params* params)
{
    const crt_denoise_variance_params prm = params ? *params : kDenoiseVarianceDefaults;
    return { prm.iterations, prm.sigma_luminance, prm.sigma_normal, prm.sigma_depth, prm.demodulate };
}

} // namespace

int crt_camera_rays_device(crt_ctx* c, uint32_t w, uint32_t h, uint32_t sample, void* d_rays, crt_frame_stats* stats)
{
    const char* what = "crt_camera_rays_device";
    int rc = checkCameraRays(c, what, w, h, sample, d_rays);
    if (rc) return rc;
    if ((rc = checkDevicePointers(c, what, { d_rays }, 16u)) != CRT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = runCameraRays(c, what, w, h, sample, d_rays, stats)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

int crt_camera_rays(crt_ctx* c, uint32_t w, uint32_t h, uint32_t sample, float* rays, crt_frame_stats* stats)
{
    const char* what = "crt_camera_rays";
    int rc = checkCameraRays(c, what, w, h, sample, rays);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t bytes = static_cast<size_t>(w) * h * 32u;
    if ((rc = reserveRayStage(c, bytes)) != CRT_OK) return rc;
    if ((rc = runCameraRays(c, what, w, h, sample, c->dRayStage, stats)) != CRT_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(rays, c->dRayStage, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stampTotal(stats, t0);
    return CRT_OK;
}

int crt_frame_guides_device(crt_ctx* c, uint32_t w, uint32_t h, void* d_normal, void* d_albedo, void* d_t, crt_frame_stats* stats)
{
    const char* what = "crt_frame_guides_device";
    int rc = checkFrameGuides(c, what, w, h, d_normal, d_albedo, d_t);
    if (rc) return rc;
    if ((rc = checkDevicePointers(c, what, { d_normal, d_albedo, d_t }, 4u)) != CRT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    if ((rc = runFrameGuides(c, w, h, d_normal, d_albedo, d_t, stats)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// host buffers: staged through the context's query staging buffer {normal | albedo | t}; synchronous
int crt_frame_guides(crt_ctx* c, uint32_t w, uint32_t h, float* normal, float* albedo, float* t, crt_frame_stats* stats)
{
    const char* what = "crt_frame_guides";
    int rc = checkFrameGuides(c, what, w, h, normal, albedo, t);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    const size_t nn = static_cast<size_t>(w) * h;
    const StagePlane planes[3] = { { nullptr, normal, nn * 12u }, { nullptr, albedo, nn * 12u }, { nullptr, t, nn * 4u } };
    void* dev[3];
    if ((rc = stageBegin(c, planes, 3, dev)) != CRT_OK) return rc;
    if ((rc = runFrameGuides(c, w, h, dev[0], dev[1], dev[2], stats)) != CRT_OK) return rc;
    if ((rc = stageEnd(c, planes, 3, dev)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

int crt_denoise_device(crt_ctx* c, uint32_t w, uint32_t h, const void* d_rgb, const void* d_normal, const void* d_albedo, const void* d_t,
                       void* d_out, const crt_denoise_params* params, crt_frame_stats* stats)
{
    return denoiseDevice(c, "crt_denoise_device", false, w, h, d_rgb, d_normal, d_albedo, d_t, nullptr, d_out, nullptr,
                         params ? *params : kDenoiseDefaults, stats);
}

int crt_denoise(crt_ctx* c, uint32_t w, uint32_t h, const float* rgb, const float* normal, const float* albedo, const float* t, float* out,
                const crt_denoise_params* params, crt_frame_stats* stats)
{
    return denoiseHost(c, "crt_denoise", false, w, h, rgb, normal, albedo, t, nullptr, out, nullptr, params ? *params : kDenoiseDefaults, stats);
}

namespace {

// ---- temporal reprojection (temporal_kernels.hip)
const crt_temporal_params kTemporalDefaults = { 0.1f, 0.01f, 0.9f, 64u, 1u };

int checkTemporal(crt_ctx* c, const char* what, uint32_t w, uint32_t h, const float* camCur, const float* camPrev, const void* rgb,
                  const void* normal, const void* albedo, const void* t, const void* histNext, const crt_temporal_params& prm)
{
    if (!c) return fail(nullptr, CRT_EINVAL, "%s: NULL context", what);
    if (const int rc = checkFrameSize(c, what, w, h)) return rc;
    if (!camCur || !camPrev) return fail(c, CRT_EINVAL, "%s: NULL camera", what);
    if (!(prm.alpha >= 0.0f && prm.alpha <= 1.0f)) return fail(c, CRT_EINVAL, "%s: alpha = %g is outside [0, 1]", what, static_cast<double>(prm.alpha));
    if (!(prm.depth_tolerance > 0.0f))
        return fail(c, CRT_EINVAL, "%s: depth_tolerance = %g must be > 0", what, static_cast<double>(prm.depth_tolerance));
    if (prm.normal_threshold != prm.normal_threshold) return fail(c, CRT_EINVAL, "%s: normal_threshold is NaN", what);
    if (prm.max_history < 1u || prm.max_history > (1u << 24))
        return fail(c, CRT_EINVAL, "%s: max_history = %u is outside 1..2^24", what, prm.max_history);
    if (prm.demodulate > 1u) return fail(c, CRT_EINVAL, "%s: demodulate = %u is neither 0 nor 1", what, prm.demodulate);
    if (!rgb || !normal || !t || !histNext) return fail(c, CRT_EINVAL, "%s: NULL buffer", what);
    if (prm.demodulate && !albedo) return fail(c, CRT_EINVAL, "%s: NULL albedo while demodulating", what);
    return CRT_OK;
}

// crt_temporal_variance*: the moment buffers and parameters beside the history's
struct TemporalMoments {
    const void* prev;
    void* next;
    void* variance;
    float alphaMoments;
    uint32_t minHistory;
};

int runTemporal(crt_ctx* c, const char* what, uint32_t w, uint32_t h, const float* camCur, const float* camPrev, const void* d_rgb,
                const void* d_normal, const void* d_albedo, const void* d_t, const void* d_histPrev, void* d_histNext, void* d_out,
                const void* d_prevPoint, const crt_temporal_params& prm, crt_frame_stats* stats, const TemporalMoments* moments = nullptr)
{
    HIP_TRY(c, hipSetDevice(c->device));
    crt::TemporalParams p;
    std::memset(&p, 0, sizeof(p));
    crt::copyBytes(p.posCur, camCur, sizeof(p.posCur));
    crt::copyBytes(p.rotCur, camCur + 3, sizeof(p.rotCur));
    crt::copyBytes(p.posPrev, camPrev, sizeof(p.posPrev));
    crt::copyBytes(p.rotPrev, camPrev + 3, sizeof(p.rotPrev));
    p.width = w;
    p.height = h;
    p.demodulate = prm.demodulate;
    p.staticCamera = std::memcmp(camCur, camPrev, 12u * sizeof(float)) == 0 ? 1u : 0u;
    p.alpha = prm.alpha;
    p.depthTolerance = prm.depth_tolerance;
    p.normalThreshold = prm.normal_threshold;
    p.maxHistory = static_cast<float>(prm.max_history);
    p.rgb = static_cast<const float*>(d_rgb);
    p.normal = static_cast<const float*>(d_normal);
    p.albedo = static_cast<const float*>(d_albedo);
    p.t = static_cast<const float*>(d_t);
    p.histPrev = d_histPrev;
    p.histNext = d_histNext;
    p.out = static_cast<float*>(d_out);
    p.prevPoint = static_cast<const float*>(d_prevPoint);
    if (moments) {
        p.momPrev = moments->prev;
        p.momNext = moments->next;
        p.variance = static_cast<float*>(moments->variance);
        p.alphaMoments = moments->alphaMoments;
        p.minHistory = static_cast<float>(moments->minHistory);
    }
    return runTimed(c, what, stats, [&] { return crt::launchTemporal(p, c->stream); });
}

// what crt_temporal_variance* checks beyond checkTemporal
int checkTemporalVariance(crt_ctx* c, const char* what, const void* histPrev, const TemporalMoments& m)
{
    if (!(m.alphaMoments >= 0.0f && m.alphaMoments <= 1.0f))
        return fail(c, CRT_EINVAL, "%s: alpha_moments = %g is outside [0, 1]", what, static_cast<double>(m.alphaMoments));
    if (m.minHistory < 1u || m.minHistory > (1u << 24)) return fail(c, CRT_EINVAL, "%s: min_history = %u is outside 1..2^24", what, m.minHistory);
    if (!m.next || !m.variance) return fail(c, CRT_EINVAL, "%s: NULL buffer", what);
    if ((histPrev == nullptr) != (m.prev == nullptr))
        return fail(c, CRT_EINVAL, "%s: hist_prev and mom_prev must be given together or not at all", what);
    return CRT_OK;
}

// The three temporal entry points are one call: plain (prevPoint == NULL), with motion, and with moments (moments != NULL).
// The device forms ...
int temporalDevice(crt_ctx* c, const char* what, uint32_t w, uint32_t h, const float* camCur, const float* camPrev, const void* d_rgb,
                   const void* d_normal, const void* d_albedo, const void* d_t, const void* d_histPrev, void* d_histNext, void* d_out,
                   const void* d_prevPoint, const crt_temporal_params* params, const TemporalMoments* moments, crt_frame_stats* stats)
{
    const crt_temporal_params prm = params ? *params : kTemporalDefaults;
    int rc = checkTemporal(c, what, w, h, camCur, camPrev, d_rgb, d_normal, d_albedo, d_t, d_histNext, prm);
    if (rc == CRT_OK && moments) rc = checkTemporalVariance(c, what, d_histPrev, *moments);
    if (rc) return rc;
    const TemporalMoments m = moments ? *moments : TemporalMoments{};
    if ((rc = checkDevicePointers(c, what, { d_rgb, d_normal, d_albedo, d_t, d_out, d_prevPoint, m.variance }, 4u)) != CRT_OK) return rc;
    if ((rc = checkDevicePointers(c, what, { m.prev, m.next }, 8u)) != CRT_OK) return rc;
    if ((rc = checkDevicePointers(c, what, { d_histPrev, d_histNext }, 16u)) != CRT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = runTemporal(c, what, w, h, camCur, camPrev, d_rgb, d_normal, d_albedo, d_t, d_histPrev, d_histNext, d_out, d_prevPoint, prm, stats,
                          moments)) != CRT_OK)
        return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// ... and the host forms: staged as {rgb | normal | albedo | t | hist_prev | hist_next | prev_point | mom_prev | mom_next | variance},
// the colour accumulated in place and read back last; synchronous
int temporalHost(crt_ctx* c, const char* what, uint32_t w, uint32_t h, const float* camCur, const float* camPrev, const float* rgb,
                 const float* normal, const float* albedo, const float* t, const float* histPrev, float* histNext, float* out,
                 const float* prevPoint, const crt_temporal_params* params, const TemporalMoments* moments, crt_frame_stats* stats)
{
    const crt_temporal_params prm = params ? *params : kTemporalDefaults;
    int rc = checkTemporal(c, what, w, h, camCur, camPrev, rgb, normal, albedo, t, histNext, prm);
    if (rc == CRT_OK && moments) rc = checkTemporalVariance(c, what, histPrev, *moments);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const TemporalMoments m = moments ? *moments : TemporalMoments{};
    const size_t nn = static_cast<size_t>(w) * h;
    const StagePlane planes[11] = { { rgb, nullptr, nn * 12u }, { normal, nullptr, nn * 12u }, { albedo, nullptr, nn * 12u }, { t, nullptr, nn * 4u },
                                    { histPrev, nullptr, nn * 32u }, { nullptr, histNext, nn * 32u }, { prevPoint, nullptr, nn * 12u },
                                    { m.prev, nullptr, nn * 8u }, { nullptr, m.next, nn * 8u }, { nullptr, m.variance, nn * 4u },
                                    { nullptr, out, nn * 12u, 0 } };
    void* dev[11];
    if ((rc = stageBegin(c, planes, 11, dev)) != CRT_OK) return rc;
    const TemporalMoments staged = { dev[7], dev[8], dev[9], m.alphaMoments, m.minHistory };
    if ((rc = runTemporal(c, what, w, h, camCur, camPrev, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[10], dev[6], prm, stats,
                          moments ? &staged : nullptr)) != CRT_OK)
        return rc;
    if ((rc = stageEnd(c, planes, 11, dev)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

} // namespace

int crt_temporal_accumulate_device(crt_ctx* c, uint32_t w, uint32_t h, const float* camCur, const float* camPrev, const void* d_rgb,
                                   const void* d_normal, const void* d_albedo, const void* d_t, const void* d_histPrev, void* d_histNext,
                                   void* d_out, const crt_temporal_params* params, crt_frame_stats* stats)
{
    return temporalDevice(c, "crt_temporal_accumulate_device", w, h, camCur, camPrev, d_rgb, d_normal, d_albedo, d_t, d_histPrev, d_histNext, d_out,
                          nullptr, params, nullptr, stats);
}

int crt_temporal_accumulate(crt_ctx* c, uint32_t w, uint32_t h, const float* camCur, const float* camPrev, const float* rgb,
                            const float* normal, const float* albedo, const float* t, const float* histPrev, float* histNext, float* out,
                            const crt_temporal_params* params, crt_frame_stats* stats)
{
    return temporalHost(c, "crt_temporal_accumulate", w, h, camCur, camPrev, rgb, normal, albedo, t, histPrev, histNext, out, nullptr,
                        params, nullptr, stats);
}

int crt_temporal_accumulate_motion_device(crt_ctx* c, uint32_t w, uint32_t h, const float* camCur, const float* camPrev, const void* d_rgb,
                                          const void* d_normal, const void* d_albedo, const void* d_t, const void* d_prevPoint,
                                          const void* d_histPrev, void* d_histNext, void* d_out, const crt_temporal_params* params,
                                          crt_frame_stats* stats)
{
    return temporalDevice(c, "crt_temporal_accumulate_motion_device", w, h, camCur, camPrev, d_rgb, d_normal, d_albedo, d_t, d_histPrev, d_histNext,
                          d_out, d_prevPoint, params, nullptr, stats);
}

int crt_temporal_accumulate_motion(crt_ctx* c, uint32_t w, uint32_t h, const float* camCur, const float* camPrev, const float* rgb,
                                   const float* normal, const float* albedo, const float* t, const float* prevPoint, const float* histPrev,
                                   float* histNext, float* out, const crt_temporal_params* params, crt_frame_stats* stats)
{
    return temporalHost(c, "crt_temporal_accumulate_motion", w, h, camCur, camPrev, rgb, normal, albedo, t, histPrev, histNext, out, prevPoint,
                        params, nullptr, stats);
}

namespace {

// ---- variance: luminance moments in the temporal pass (temporal_kernels.hip); the variance-guided filter is denoiseDevice / denoiseHost
const crt_temporal_variance_params kTemporalVarianceDefaults = { { 0.1f, 0.01f, 0.9f, 64u, 1u }, 0.2f, 4u };

} // namespace

int crt_temporal_variance_device(crt_ctx* c, uint32_t w, uint32_t h, const float* camCur, const float* camPrev, const void* d_rgb,
                                 const void* d_normal, const void* d_albedo, const void* d_t, const void* d_prevPoint, const void* d_histPrev,
                                 void* d_histNext, const void* d_momPrev, void* d_momNext, void* d_variance, void* d_out,
                                 const crt_temporal_variance_params* params, crt_frame_stats* stats)
{
    const crt_temporal_variance_params prm = params ? *params : kTemporalVarianceDefaults;
    const TemporalMoments moments = { d_momPrev, d_momNext, d_variance, prm.alpha_moments, prm.min_history };
    return temporalDevice(c, "crt_temporal_variance_device", w, h, camCur, camPrev, d_rgb, d_normal, d_albedo, d_t, d_histPrev, d_histNext, d_out,
                          d_prevPoint, &prm.base, &moments, stats);
}

int crt_temporal_variance(crt_ctx* c, uint32_t w, uint32_t h, const float* camCur, const float* camPrev, const float* rgb, const float* normal,
                          const float* albedo, const float* t, const float* prevPoint, const float* histPrev, float* histNext,
                          const float* momPrev, float* momNext, float* variance, float* out, const crt_temporal_variance_params* params,
                          crt_frame_stats* stats)
{
    const crt_temporal_variance_params prm = params ? *params : kTemporalVarianceDefaults;
    const TemporalMoments moments = { momPrev, momNext, variance, prm.alpha_moments, prm.min_history };
    return temporalHost(c, "crt_temporal_variance", w, h, camCur, camPrev, rgb, normal, albedo, t, histPrev, histNext, out, prevPoint, &prm.base,
                        &moments, stats);
}

int crt_denoise_variance_device(crt_ctx* c, uint32_t w, uint32_t h, const void* d_rgb, const void* d_normal, const void* d_albedo, const void* d_t,
                                const void* d_variance, void* d_out, void* d_varianceOut, const crt_denoise_variance_params* params,
                                crt_frame_stats* stats)
{
    return denoiseDevice(c, "crt_denoise_variance_device", true, w, h, d_rgb, d_normal, d_albedo, d_t, d_variance, d_out, d_varianceOut,
                         guidedParams(params), stats);
}

int crt_denoise_variance(crt_ctx* c, uint32_t w, uint32_t h, const float* rgb, const float* normal, const float* albedo, const float* t,
                         const float* variance, float* out, float* varianceOut, const crt_denoise_variance_params* params, crt_frame_stats* stats)
{
    return denoiseHost(c, "crt_denoise_variance", true, w, h, rgb, normal, albedo, t, variance, out, varianceOut, guidedParams(params), stats);
}

int crt_closest_points_device(crt_ctx* c, uint32_t n, const void* d_points, void* d_dist, void* d_point, void* d_uv, void* d_inst,
                              void* d_prim, crt_frame_stats* stats)
{
    return queryDevice(c, { "crt_closest_points_device", crt::kQueryClosestPoint, { d_dist, d_point, d_uv, d_inst, d_prim } }, n, d_points, stats);
}

int crt_closest_points(crt_ctx* c, uint32_t n, const float* points, float* dist, float* point, float* uv, uint32_t* inst, uint32_t* prim,
                       crt_frame_stats* stats)
{
    return queryHost(c, { "crt_closest_points", crt::kQueryClosestPoint, { dist, point, uv, inst, prim } }, n, points, stats);
}

int crt_count_hits_device(crt_ctx* c, uint32_t n, const void* d_rays, void* d_count, crt_frame_stats* stats)
{
    return queryDevice(c, { "crt_count_hits_device", crt::kQueryCount, { d_count } }, n, d_rays, stats);
}

int crt_count_hits(crt_ctx* c, uint32_t n, const float* rays, uint32_t* count, crt_frame_stats* stats)
{
    return queryHost(c, { "crt_count_hits", crt::kQueryCount, { count } }, n, rays, stats);
}

int crt_occupancy_device(crt_ctx* c, uint32_t n, const void* d_points, void* d_inside, crt_frame_stats* stats)
{
    return queryDevice(c, { "crt_occupancy_device", crt::kQueryOccupancy, { d_inside } }, n, d_points, stats);
}

int crt_occupancy(crt_ctx* c, uint32_t n, const float* points, uint8_t* inside, crt_frame_stats* stats)
{
    return queryHost(c, { "crt_occupancy", crt::kQueryOccupancy, { inside } }, n, points, stats);
}

int crt_winding_numbers_device(crt_ctx* c, uint32_t n, const void* d_points, float beta, void* d_w, crt_frame_stats* stats)
{
    return queryDevice(c, { "crt_winding_numbers_device", crt::kQueryWinding, { d_w }, beta }, n, d_points, stats);
}

int crt_winding_numbers(crt_ctx* c, uint32_t n, const float* points, float beta, float* w, crt_frame_stats* stats)
{
    return queryHost(c, { "crt_winding_numbers", crt::kQueryWinding, { w }, beta }, n, points, stats);
}

int crt_winding_moments_export(const crt_ctx* cc, float* moments)
{
    if (!cc) return CRT_EINVAL;
    crt_ctx* c = const_cast<crt_ctx*>(cc); // a pending refit runs first, as for the tree's exports
    if (!c->haveScene) return fail(c, CRT_ESTATE, "crt_winding_moments_export: no scene uploaded: call crt_upload_scene first");
    if (!moments) return fail(c, CRT_EINVAL, "crt_winding_moments_export: moments is NULL");
    if (const int rc = applyRefit(c, nullptr)) return rc;
    if (const int rc = ensureMoments(c)) return rc;
    if (c->bvh.dev.nNodes4 > 0)
        HIP_TRY(c, hipMemcpy(moments, c->dMoments, sizeof(float) * crt::kMomentStride * c->bvh.dev.nNodes4, hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_list_hits_device(crt_ctx* c, uint32_t n, const void* d_rays, void* d_offsets, uint64_t capacity, void* d_t, void* d_uv, void* d_inst,
                         void* d_prim, uint64_t* total, crt_frame_stats* stats)
{
    const char* what = "crt_list_hits_device";
    const auto t0 = std::chrono::steady_clock::now();
    bool done;
    int rc = listCheck(c, what, n, d_rays, d_offsets, t0, total, stats, done);
    if (rc || done) return rc;
    if (reinterpret_cast<uintptr_t>(d_rays) & 15u) return fail(c, CRT_EINVAL, "%s: ray buffer %p is not 16-byte aligned", what, d_rays);
    if (reinterpret_cast<uintptr_t>(d_offsets) & 7u) return fail(c, CRT_EINVAL, "%s: offsets %p is not 8-byte aligned", what, d_offsets);
    if ((reinterpret_cast<uintptr_t>(d_uv) & 7u) || ((reinterpret_cast<uintptr_t>(d_t) | reinterpret_cast<uintptr_t>(d_inst) | reinterpret_cast<uintptr_t>(d_prim)) & 3u))
        return fail(c, CRT_EINVAL, "%s: a record array is misaligned (uv 8-byte, t / inst / prim 4-byte)", what);
    const bool fill = d_t || d_uv || d_inst || d_prim;
    // work arrays the caller's own t / prim arrays cannot stand in for, sized from the capacity
    size_t keyBytes = 0;
    if (fill && (!d_t || !d_prim)) {
        if (capacity > (static_cast<uint64_t>(1) << 40)) return fail(c, CRT_ENOMEM, "%s: key scratch for a capacity of %llu records", what, static_cast<unsigned long long>(capacity));
        keyBytes = (d_t ? 0u : up256(static_cast<size_t>(capacity) * 4u)) + (d_prim ? 0u : up256(static_cast<size_t>(capacity) * 4u));
    }
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    ListRun lr;
    if ((rc = listBegin(c, n, d_rays, d_offsets, keyBytes, stats, lr)) != CRT_OK) return rc;
    int hrc = 0;
    if (fill) {
        unsigned char* scratch = lr.keyScratch;
        float* tkey = static_cast<float*>(d_t);
        if (!tkey) { tkey = reinterpret_cast<float*>(scratch); scratch += up256(static_cast<size_t>(capacity) * 4u); }
        uint32_t* idkey = d_prim ? static_cast<uint32_t*>(d_prim) : reinterpret_cast<uint32_t*>(scratch);
        void* const out[4] = { d_t, d_uv, d_inst, d_prim };
        hrc = listFill(c, lr, capacity, tkey, idkey, out);
    }
    if ((rc = endQuery(c, crt::kQueryCount, n, lr.ql, hrc, stats)) != CRT_OK) return rc;
    if ((rc = listPhases(c, lr, fill)) != CRT_OK) return rc;
    if (total) {
        unsigned long long tot = 0;
        HIP_TRY(c, hipMemcpyAsync(&tot, static_cast<const unsigned long long*>(d_offsets) + n, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        *total = tot;
    }
    stampTotal(stats, t0);
    return CRT_OK;
}

int crt_list_hits(crt_ctx* c, uint32_t n, const float* rays, uint64_t* offsets, uint64_t capacity, float* t, float* uv, uint32_t* inst,
                  uint32_t* prim, uint64_t* total, crt_frame_stats* stats)
{
    const char* what = "crt_list_hits";
    const auto t0 = std::chrono::steady_clock::now();
    bool done;
    int rc = listCheck(c, what, n, rays, offsets, t0, total, stats, done);
    if (done && offsets) offsets[0] = 0u;
    if (rc || done) return rc;
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    const StagePlane planes[2] = { { rays, nullptr, static_cast<size_t>(n) * 32u }, { nullptr, offsets, (static_cast<size_t>(n) + 1u) * sizeof(uint64_t) } };
    void* dev[2];
    if ((rc = stageBegin(c, planes, 2, dev)) != CRT_OK) return rc;
    unsigned long long* dOff = static_cast<unsigned long long*>(dev[1]);
    ListRun lr;
    if ((rc = listBegin(c, n, dev[0], dOff, 0u, stats, lr)) != CRT_OK) return rc;
    // the one read-back: does the total fit the caller's arrays?
    unsigned long long tot = 0;
    hipError_t he = hipMemcpyAsync(&tot, dOff + n, sizeof(tot), hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    const bool fill = (t || uv || inst || prim) && he == hipSuccess && tot <= capacity && tot > 0u;
    unsigned char* rec = nullptr;
    const size_t cap4 = up256(static_cast<size_t>(tot) * 4u), cap8 = up256(static_cast<size_t>(tot) * 8u);
    bool noMem = false;
    if (fill) { // t, prim (the work arrays), inst, uv.  Without the memory the call still goes through endQuery: the count has used the arena
        const int grown = ensureBuffer(c, &c->dListStage, &c->listStageBytes, 3u * cap4 + cap8, true);
        if (grown == CRT_EHIP) return grown; // (the device-wide wait failed: endQuery would only return the same)
        noMem = grown == CRT_ENOMEM;
        rec = static_cast<unsigned char*>(c->dListStage);
    }
    int hrc = static_cast<int>(he);
    void* const out[4] = { rec, uv ? rec + 3u * cap4 : nullptr, inst ? rec + 2u * cap4 : nullptr, rec ? rec + cap4 : nullptr };
    if (fill && !noMem && hrc == 0) hrc = listFill(c, lr, tot, static_cast<float*>(out[0]), static_cast<uint32_t*>(out[3]), out);
    if ((rc = endQuery(c, crt::kQueryCount, n, lr.ql, hrc, stats)) != CRT_OK) return rc;
    if ((rc = listPhases(c, lr, fill && !noMem)) != CRT_OK) return rc;
    if (noMem) return fail(c, CRT_ENOMEM, "%s: staging for %llu records not available", what, tot);
    if ((rc = stageDownload(c, planes, 2, dev)) != CRT_OK) return rc;
    if (fill) {
        if (t) HIP_TRY(c, hipMemcpyAsync(t, out[0], static_cast<size_t>(tot) * 4u, hipMemcpyDeviceToHost, c->stream));
        if (uv) HIP_TRY(c, hipMemcpyAsync(uv, out[1], static_cast<size_t>(tot) * 8u, hipMemcpyDeviceToHost, c->stream));
        if (inst) HIP_TRY(c, hipMemcpyAsync(inst, out[2], static_cast<size_t>(tot) * 4u, hipMemcpyDeviceToHost, c->stream));
        if (prim) HIP_TRY(c, hipMemcpyAsync(prim, out[3], static_cast<size_t>(tot) * 4u, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (total) *total = tot;
    stampTotal(stats, t0);
    return CRT_OK;
}

int crt_render_frame_device(crt_ctx* c, uint32_t w, uint32_t h, void* d_rgba8, void* d_hit_inst, void* d_hit_prim,
                            void* d_hit_t, void* d_rgb_f32, crt_frame_stats* stats)
{
    int rc = checkRenderable(c, w, h);
    if (rc) return rc;
    if (!d_rgba8) return fail(c, CRT_EINVAL, "d_rgba8 is NULL");
    const auto t0 = std::chrono::steady_clock::now();
    RenderParams p;
    fillParams(c, w, h, 0, 1, p);
    p.rgba8 = static_cast<uint32_t*>(d_rgba8);
    p.hit_inst = static_cast<uint32_t*>(d_hit_inst);
    p.hit_prim = static_cast<uint32_t*>(d_hit_prim);
    p.hit_t = static_cast<float*>(d_hit_t);
    p.rgb_f32 = static_cast<float*>(d_rgb_f32);
    rc = runFrame(c, p, stats, kAccFrame);
    if (rc) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

int crt_render_frame(crt_ctx* c, uint32_t w, uint32_t h, uint8_t* rgba8, uint32_t* hit_inst, uint32_t* hit_prim, float* hit_t,
                     float* rgb_f32, crt_frame_stats* stats)
{
    int rc = checkRenderable(c, w, h);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = static_cast<size_t>(w) * h;
    void* host[5] = { rgba8, hit_inst, hit_prim, hit_t, rgb_f32 };
    const size_t bytes[5] = { n * 4, n * 4, n * 4, n * 4, n * 12 };
    for (int i = 0; i < 5; i++)
        if (host[i] || i == 0)
            if ((rc = ensureFrame(c, i, bytes[i])) != CRT_OK) return rc;
    RenderParams p;
    fillParams(c, w, h, 0, 1, p);
    p.rgba8 = static_cast<uint32_t*>(c->dFrame[0]);
    p.hit_inst = host[1] ? static_cast<uint32_t*>(c->dFrame[1]) : nullptr;
    p.hit_prim = host[2] ? static_cast<uint32_t*>(c->dFrame[2]) : nullptr;
    p.hit_t = host[3] ? static_cast<float*>(c->dFrame[3]) : nullptr;
    p.rgb_f32 = host[4] ? static_cast<float*>(c->dFrame[4]) : nullptr;
    crt_frame_stats local;
    rc = runFrame(c, p, stats ? stats : &local, kAccFrame); // synchronous like the reference's renderFrame
    if (rc) return rc;
    const bool traced = !(p.acc_sum && p.spp == 0u); // a frame at the accumulation limit writes no hit outputs
    for (int i = 0; i < 5; i++)
        if (host[i] && (traced || i == 0 || i == 4)) HIP_TRY(c, hipMemcpyAsync(host[i], c->dFrame[i], bytes[i], hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stampTotal(stats, t0);
    return CRT_OK;
}

uint32_t crt_tile_count(uint32_t w, uint32_t h) { return tilesFor(w, h); }

uint32_t crt_tile_slots(uint32_t w, uint32_t h, uint32_t n_ranks)
{
    if (n_ranks == 0) return 0;
    return (tilesFor(w, h) + n_ranks - 1) / n_ranks;
}

int crt_render_tiles_device(crt_ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t n_ranks, void* d_staging, crt_frame_stats* stats)
{
    int rc = checkRenderable(c, w, h);
    if (rc) return rc;
    if (!d_staging || n_ranks == 0 || rank >= n_ranks) return fail(c, CRT_EINVAL, "bad tile arguments (rank %u of %u)", rank, n_ranks);
    const auto t0 = std::chrono::steady_clock::now();
    RenderParams p;
    fillParams(c, w, h, rank, n_ranks, p);
    p.staging = 1;
    p.rgba8 = static_cast<uint32_t*>(d_staging);
    rc = runFrame(c, p, stats, kAccTiles);
    if (rc) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

namespace {
// shared by the two batch entry points: frame 0 takes the place of the single frame, the others go to the batch arrays
int runBatch(crt_ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t n_ranks, bool staging, uint32_t n_frames, const float* cameras,
             void* const* d_out, crt_frame_stats* stats)
{
    int rc = checkRenderable(c, w, h);
    if (rc) return rc;
    if (n_frames == 0 || n_frames > static_cast<uint32_t>(crt::kMaxBatch)) return fail(c, CRT_EINVAL, "n_frames %u outside [1,%d]", n_frames, crt::kMaxBatch);
    if (!d_out || n_ranks == 0 || rank >= n_ranks) return fail(c, CRT_EINVAL, "bad batch arguments (rank %u of %u)", rank, n_ranks);
    for (uint32_t f = 0; f < n_frames; f++)
        if (!d_out[f]) return fail(c, CRT_EINVAL, "output pointer of frame %u is NULL", f);
    if (c->accMax != 0u && c->mode >= 200u)
        return fail(c, CRT_EINVAL, "batch entry points do not accumulate (their frames have different cameras): turn accumulation off for mode %u", c->mode);
    const auto t0 = std::chrono::steady_clock::now();
    RenderParams p;
    fillParams(c, w, h, rank, n_ranks, p);
    p.staging = staging ? 1u : 0u;
    p.n_batch = n_frames;
    p.rgba8 = static_cast<uint32_t*>(d_out[0]);
    if (cameras) {
        crt::copyBytes(p.pos, cameras, sizeof(p.pos));
        crt::copyBytes(p.rot, cameras + 3, sizeof(p.rot));
    }
    for (uint32_t f = 1; f < n_frames; f++) {
        const float* cam = cameras ? cameras + 12 * f : nullptr;
        crt::copyBytes(p.batch_pos[f - 1], cam ? cam : c->pos, sizeof(p.pos));
        crt::copyBytes(p.batch_rot[f - 1], cam ? cam + 3 : c->rot, sizeof(p.rot));
        p.batch_rgba8[f - 1] = static_cast<uint32_t*>(d_out[f]);
    }
    rc = runRender(c, p, stats);
    if (rc) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}
} // namespace

int crt_render_frames_batch_device(crt_ctx* c, uint32_t w, uint32_t h, uint32_t n_frames, const float* cameras, void* const* d_rgba8,
                                   crt_frame_stats* stats)
{
    return runBatch(c, w, h, 0, 1, false, n_frames, cameras, d_rgba8, stats);
}

int crt_render_tiles_batch_device(crt_ctx* c, uint32_t w, uint32_t h, uint32_t rank, uint32_t n_ranks, uint32_t n_frames,
                                  const float* cameras, void* const* d_staging, crt_frame_stats* stats)
{
    return runBatch(c, w, h, rank, n_ranks, true, n_frames, cameras, d_staging, stats);
}

int crt_untile_batch_device(crt_ctx* c, uint32_t w, uint32_t h, uint32_t n_ranks, uint32_t n_frames, uint32_t frame, const void* d_gathered,
                            void* d_rgba8)
{
    if (!c) return CRT_EINVAL;
    if (!d_gathered || !d_rgba8 || n_ranks == 0 || w == 0 || h == 0 || n_frames == 0 || frame >= n_frames)
        return fail(c, CRT_EINVAL, "crt_untile_batch_device: bad argument");
    const uint32_t slots = crt_tile_slots(w, h, n_ranks);
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = crt::launchUntile(static_cast<const uint32_t*>(d_gathered), static_cast<uint32_t*>(d_rgba8), w, h, n_ranks,
                                     n_frames * slots, frame * slots, c->stream);
    if (rc != 0) return fail(c, CRT_EHIP, "untile kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
    return CRT_OK;
}

int crt_untile_device(crt_ctx* c, uint32_t w, uint32_t h, uint32_t n_ranks, const void* d_gathered, void* d_rgba8)
{
    return crt_untile_batch_device(c, w, h, n_ranks, 1, 0, d_gathered, d_rgba8);
}

int crt_bvh_info(const crt_ctx* c, uint32_t* n_nodes, uint32_t* n_tris, uint32_t* max_depth)
{
    if (!c || !c->haveScene) return CRT_ESTATE;
    if (int rc = applyRefit(const_cast<crt_ctx*>(c), nullptr)) return rc; // (pending updates of a dynamic scene)
    if (n_nodes) *n_nodes = c->bvh.dev.nNodes;
    if (n_tris) *n_tris = c->bvh.nTris;
    if (max_depth) *max_depth = c->bvh.maxDepth;
    return CRT_OK;
}

int crt_build_stats(const crt_ctx* c, double* upload_ms, double* device_build_ms)
{
    if (!c || !c->haveScene) return CRT_ESTATE;
    if (upload_ms) *upload_ms = c->buildMs;
    if (device_build_ms) *device_build_ms = c->buildDeviceMs;
    return CRT_OK;
}

int crt_bvh_info4(const crt_ctx* c, uint32_t* n_nodes4, uint32_t* depth4)
{
    if (!c || !c->haveScene) return CRT_ESTATE;
    if (int rc = applyRefit(const_cast<crt_ctx*>(c), nullptr)) return rc; // (pending updates of a dynamic scene)
    if (n_nodes4) *n_nodes4 = c->bvh.dev.nNodes4;
    if (depth4) *depth4 = c->bvh.depth4;
    return CRT_OK;
}

int crt_bvh_export4(const crt_ctx* c, crt_bvh_node4* nodes4)
{
    if (!c || !c->haveScene) return CRT_ESTATE;
    if (int rc = applyRefit(const_cast<crt_ctx*>(c), nullptr)) return rc; // (pending updates of a dynamic scene)
    if (nodes4) {
        if (!c->dWideNodes) crt::copyBytes(nodes4, c->bvh.nodes4.data(), sizeof(crt_bvh_node4) * c->bvh.nodes4.size());
        else if (hipMemcpy(nodes4, c->dWideNodes, sizeof(crt_bvh_node4) * c->bvh.dev.nNodes4, hipMemcpyDeviceToHost) != hipSuccess) return CRT_EHIP;
    }
    return CRT_OK;
}

int crt_bvh_export4q(const crt_ctx* c, crt_bvh_node4q* nodes4q)
{
    if (!c || !c->haveScene) return CRT_ESTATE;
    if (int rc = applyRefit(const_cast<crt_ctx*>(c), nullptr)) return rc; // (pending updates of a dynamic scene)
    if (nodes4q) {
        if (!c->dWideNodes) crt::copyBytes(nodes4q, c->bvh.nodes4q.data(), sizeof(crt_bvh_node4q) * c->bvh.nodes4q.size());
        else if (hipMemcpy(nodes4q, c->dNodes, sizeof(crt_bvh_node4q) * c->bvh.dev.nNodes4, hipMemcpyDeviceToHost) != hipSuccess) return CRT_EHIP;
    }
    return CRT_OK;
}

int crt_bvh_export_planes4q(const crt_ctx* c, float* planes)
{
    if (!c || !c->haveScene) return CRT_ESTATE;
    if (int rc = applyRefit(const_cast<crt_ctx*>(c), nullptr)) return rc; // (pending updates of a dynamic scene)
    if (planes && c->bvh.dev.nNodes4 > 0 &&
        hipMemcpy(planes, c->dPlanes, sizeof(float) * crt::kPlaneStride * c->bvh.dev.nNodes4, hipMemcpyDeviceToHost) != hipSuccess)
        return CRT_EHIP;
    return CRT_OK;
}

int crt_bvh_quantize4(const crt_bvh_node4* nodes4, uint32_t n, crt_bvh_node4q* out)
{
    if ((!nodes4 || !out) && n) return fail(nullptr, CRT_EINVAL, "crt_bvh_quantize4: NULL argument");
    for (uint32_t i = 0; i < n; i++) crt::quantizeNode4(nodes4[i], out[i]);
    return CRT_OK;
}

int crt_bvh_build_host4(const crt_mesh_view* meshes, uint32_t n_meshes, crt_bvh_node4** nodes4, uint32_t* n_nodes4, uint32_t* depth4)
{
    if ((!meshes && n_meshes) || !nodes4 || !n_nodes4) return fail(nullptr, CRT_EINVAL, "crt_bvh_build_host4: NULL argument");
    try {
        crt::Bvh b;
        crt::buildBvh(meshes, n_meshes, b);
        *n_nodes4 = static_cast<uint32_t>(b.nodes4.size());
        if (depth4) *depth4 = b.depth4;
        *nodes4 = static_cast<crt_bvh_node4*>(std::malloc(sizeof(crt_bvh_node4) * (b.nodes4.size() + 1)));
        if (!*nodes4) return fail(nullptr, CRT_ENOMEM, "out of host memory");
        crt::copyBytes(*nodes4, b.nodes4.data(), sizeof(crt_bvh_node4) * b.nodes4.size());
    } catch (const std::exception& ex) {
        return fail(nullptr, CRT_EINVAL, "BVH build failed: %s", ex.what());
    }
    return CRT_OK;
}

int crt_bvh_export(const crt_ctx* c, crt_bvh_node* nodes, crt_bvh_tri* tris, crt_bvh_shade* shade)
{
    if (!c || !c->haveScene) return CRT_ESTATE;
    if (int rc = applyRefit(const_cast<crt_ctx*>(c), nullptr)) return rc; // (pending updates of a dynamic scene)
    if (nodes) {
        if (!c->dBinNodes) crt::copyBytes(nodes, c->bvh.nodes.data(), sizeof(crt_bvh_node) * c->bvh.nodes.size());
        else if (hipMemcpy(nodes, c->dBinNodes, sizeof(crt_bvh_node) * c->bvh.dev.nNodes, hipMemcpyDeviceToHost) != hipSuccess) return CRT_EHIP;
    }
    // a tree built on the GPU keeps its leaf-ordered records in HBM only: copy them out of there
    const bool onDevice = c->bvh.tris.empty() && c->bvh.nTris != 0;
    if (tris) {
        if (!onDevice) crt::copyBytes(tris, c->bvh.tris.data(), sizeof(crt_bvh_tri) * c->bvh.tris.size());
        else if (hipMemcpy(tris, c->dTris, sizeof(crt_bvh_tri) * c->bvh.nTris, hipMemcpyDeviceToHost) != hipSuccess) return CRT_EHIP;
    }
    if (shade) {
        if (!onDevice) crt::copyBytes(shade, c->bvh.shade.data(), sizeof(crt_bvh_shade) * c->bvh.shade.size());
        else if (hipMemcpy(shade, c->dShade, sizeof(crt_bvh_shade) * c->bvh.nTris, hipMemcpyDeviceToHost) != hipSuccess) return CRT_EHIP;
    }
    return CRT_OK;
}


// ------------------------------------------------------------------------------------------- dynamic geometry (refit.h)
namespace {

int checkDynamic(const crt_ctx* c, uint32_t mesh, const char* what)
{
    if (!c->haveScene || !c->dyn) return fail(const_cast<crt_ctx*>(c), CRT_ESTATE, "%s: no scene uploaded with option \"dynamic\" = 1", what);
    if (mesh >= c->dyn->meshes.size()) return fail(const_cast<crt_ctx*>(c), CRT_EINVAL, "%s: mesh %u out of range (%zu meshes)", what, mesh, c->dyn->meshes.size());
    return CRT_OK;
}

int updateVertices(crt_ctx* c, uint32_t mesh, uint32_t n_vertices, const void* xyz, const void* normals, hipMemcpyKind kind, const char* what)
{
    if (!c) return CRT_EINVAL;
    if (int rc = checkDynamic(c, mesh, what)) return rc;
    crt::DynamicMesh& D = c->dyn->meshes[mesh];
    if (n_vertices != D.nVerts) return fail(c, CRT_EINVAL, "%s: mesh %u has %u vertices, not %u (the topology is fixed)", what, mesh, D.nVerts, n_vertices);
    if (!xyz) return fail(c, CRT_EINVAL, "%s: xyz is NULL", what);
    if (normals && !D.hasNormals) return fail(c, CRT_EINVAL, "%s: mesh %u was uploaded without normals", what, mesh);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t off = 3 * static_cast<size_t>(D.vertStart), bytes = sizeof(float) * 3 * D.nVerts;
    if (bytes) {
        HIP_TRY(c, hipMemcpyAsync(c->dyn->dRestXyz + off, xyz, bytes, kind, c->stream));
        if (normals) HIP_TRY(c, hipMemcpyAsync(c->dyn->dRestNormals + off, normals, bytes, kind, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // the caller's buffers are read during the call
    }
    D.dirty = true;
    c->dyn->pending = true;
    c->accSamples = 0u; // the sums belong to the old geometry (the refit also gives the scene a new serial)
    return CRT_OK;
}

} // namespace

int crt_update_vertices(crt_ctx* c, uint32_t mesh, uint32_t n_vertices, const float* xyz, const float* normals)
{
    return updateVertices(c, mesh, n_vertices, xyz, normals, hipMemcpyHostToDevice, "crt_update_vertices");
}

int crt_update_vertices_device(crt_ctx* c, uint32_t mesh, uint32_t n_vertices, const void* d_xyz, const void* d_normals)
{
    return updateVertices(c, mesh, n_vertices, d_xyz, d_normals, hipMemcpyDeviceToDevice, "crt_update_vertices_device");
}

int crt_set_mesh_transform(crt_ctx* c, uint32_t mesh, const float m[12])
{
    if (!c) return CRT_EINVAL;
    if (int rc = checkDynamic(c, mesh, "crt_set_mesh_transform")) return rc;
    static const float kIdentity[12] = { 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f };
    const float* M = m ? m : kIdentity;
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(M[i])) return fail(c, CRT_EINVAL, "crt_set_mesh_transform: entry %d is not finite", i);
    crt::DynamicMesh& D = c->dyn->meshes[mesh];
    float nm[9] = { 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f };
    if (D.hasNormals) { // inverse transpose of the 3x3, in double, rounded to float once
        const double a = M[0], b = M[1], cc = M[2], d = M[4], e = M[5], f = M[6], g = M[8], h = M[9], k = M[10];
        const double A = e * k - f * h, B = -(d * k - f * g), C = d * h - e * g;
        const double det = a * A + b * B + cc * C;
        if (det == 0.0 || !std::isfinite(det)) return fail(c, CRT_EINVAL, "crt_set_mesh_transform: singular 3x3 on mesh %u, which has normals", mesh);
        // inverse = adjugate / det; its transpose = cofactor matrix / det
        const double cof[9] = { A, B, C, -(b * k - cc * h), a * k - cc * g, -(a * h - b * g), b * f - cc * e, -(a * f - cc * d), a * e - b * d };
        for (int i = 0; i < 9; i++) {
            nm[i] = static_cast<float>(cof[i] / det);
            if (!std::isfinite(nm[i])) return fail(c, CRT_EINVAL, "crt_set_mesh_transform: the 3x3 of mesh %u is too close to singular", mesh);
        }
    }
    std::memcpy(D.m, M, sizeof(D.m));
    std::memcpy(D.nm, nm, sizeof(D.nm));
    D.identity = std::memcmp(M, kIdentity, sizeof(kIdentity)) == 0; // bitwise: a -0.0 entry is not the identity
    D.dirty = true;
    c->dyn->pending = true;
    c->accSamples = 0u; // the sums belong to the old geometry (the refit also gives the scene a new serial)
    return CRT_OK;
}

int crt_refit(crt_ctx* c, double* device_ms)
{
    if (device_ms) *device_ms = 0.0;
    if (!c) return CRT_EINVAL;
    if (!c->haveScene || !c->dyn) return fail(c, CRT_ESTATE, "crt_refit: no scene uploaded with option \"dynamic\" = 1");
    return applyRefit(c, device_ms);
}

int crt_rebuild(crt_ctx* c, double* device_ms)
{
    if (device_ms) *device_ms = 0.0;
    if (!c) return CRT_EINVAL;
    if (!c->haveScene || !c->dyn) return fail(c, CRT_ESTATE, "crt_rebuild: no scene uploaded with option \"dynamic\" = 1");
    if (c->dyn->nTris == 0) return applyRefit(c, device_ms); // no tree to build: the pending updates are all there is
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize()); // frames in flight on any stream the caller used still read the records and the tree
    crt::DeviceTree built;
    try {
        built = crt::dynamicRebuild(*c->dyn, c->gpuBuilder, static_cast<const crt_bvh_tri*>(c->dTris), c->dUvs, c->stream, device_ms);
    } catch (const std::bad_alloc&) {
        freeScene(c); // the world vertices may already be moved and the level lists half rewritten: as a failed upload, no scene
        return fail(c, CRT_ENOMEM, "crt_rebuild: out of host memory");
    } catch (const std::exception& ex) {
        freeScene(c);
        return fail(c, CRT_EHIP, "crt_rebuild failed: %s", ex.what());
    }
    // adopt the new tree and records, with the refit capacity of a dynamic upload
    adoptTree(c, std::move(built));
    int rc = reserveRefitCapacity(c);
    if (!rc) {
        hipError_t e = static_cast<hipError_t>(crt::launchDecodePlanes(c->dNodes, c->bvh.dev.nNodes4, static_cast<float*>(c->dPlanes), c->stream));
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, CRT_EHIP, "plane table: %s", hipGetErrorString(e));
    }
    if (!rc) rc = readSceneBox(c);
    if (rc) {
        freeScene(c);
        return rc;
    }
    c->sceneSerial++;
    c->accSamples = 0u;
    dropOrders(c);
    return CRT_OK;
}

int crt_mesh_vertices(const crt_ctx* cc, uint32_t mesh, float* xyz, float* normals)
{
    if (!cc) return CRT_EINVAL;
    crt_ctx* c = const_cast<crt_ctx*>(cc); // a pending refit runs first
    if (int rc = checkDynamic(c, mesh, "crt_mesh_vertices")) return rc;
    const crt::DynamicMesh& D = c->dyn->meshes[mesh];
    if (!xyz) return fail(c, CRT_EINVAL, "crt_mesh_vertices: xyz is NULL");
    if (normals && !D.hasNormals) return fail(c, CRT_EINVAL, "crt_mesh_vertices: mesh %u was uploaded without normals", mesh);
    if (int rc = applyRefit(c, nullptr)) return rc;
    const size_t off = 3 * static_cast<size_t>(D.vertStart), bytes = sizeof(float) * 3 * D.nVerts;
    if (bytes) {
        HIP_TRY(c, hipMemcpyAsync(xyz, c->dyn->dWorldXyz + off, bytes, hipMemcpyDeviceToHost, c->stream));
        if (normals) HIP_TRY(c, hipMemcpyAsync(normals, c->dyn->dWorldNormals + off, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return CRT_OK;
}

// ------------------------------------------------------------------------------------------- motion (motion_kernels.hip)
namespace {

int checkMotionScene(crt_ctx* c, const char* what)
{
    if (!c) return fail(nullptr, CRT_EINVAL, "%s: NULL context", what);
    if (!c->haveScene || !c->dyn) return fail(c, CRT_ESTATE, "%s: no scene uploaded with option \"dynamic\" = 1", what);
    return CRT_OK;
}

crt::PreviousPointsParams previousPointsParams(const crt_ctx* c, uint32_t n, const void* d_inst, const void* d_prim, const void* d_uv, void* d_point)
{
    crt::PreviousPointsParams p;
    std::memset(&p, 0, sizeof(p));
    p.table = c->dyn->dTable;
    p.nMeshes = static_cast<uint32_t>(c->dyn->meshes.size());
    p.n = n;
    p.world = c->dyn->dWorldXyz;
    p.prev = c->dyn->dPrevXyz;
    p.idx = c->dyn->dIdx;
    p.inst = static_cast<const uint32_t*>(d_inst);
    p.prim = static_cast<const uint32_t*>(d_prim);
    p.uv = static_cast<const float*>(d_uv);
    p.point = static_cast<float*>(d_point);
    return p;
}

int runPreviousPoints(crt_ctx* c, const char* what, uint32_t n, const void* d_inst, const void* d_prim, const void* d_uv, void* d_point,
                      crt_frame_stats* stats)
{
    const crt::PreviousPointsParams p = previousPointsParams(c, n, d_inst, d_prim, d_uv, d_point);
    if (const int rc = runTimed(c, what, stats, [&] { return crt::launchPreviousPoints(p, c->stream); })) return rc;
    if (stats) stats->rays_primary = n;
    return CRT_OK;
}

// crt_frame_motion*: as runFrameGuides, the camera-ray kernel into the query arena, the closest-hit query over those records with
// its uv / inst / prim beside them in the arena, then the previous points of those hits
int runFrameMotion(crt_ctx* c, uint32_t w, uint32_t h, void* d_point, crt_frame_stats* stats)
{
    const uint32_t n = w * h;
    const size_t nn = n;
    crt::RayQueryParams q;
    std::memset(&q, 0, sizeof(q));
    QueryLaunch ql;
    if (const int rc = beginQuery(c, crt::kQueryClosestHit, n, stats, ql, up256(nn * 32u) + up256(nn * 8u) + 2u * up256(nn * 4u))) return rc;
    unsigned char* rays = ql.extra;
    q.uv = reinterpret_cast<float*>(rays + up256(nn * 32u));
    q.inst = reinterpret_cast<uint32_t*>(rays + up256(nn * 32u) + up256(nn * 8u));
    q.prim = q.inst + up256(nn * 4u) / 4u;
    int hrc = crt::launchCameraRays(cameraRayParams(c, w, h, CRT_SAMPLE_CENTRE, rays), c->stream);
    if (hrc == 0) {
        q.c = queryCommon(c, ql, rays, n, c->tuneInnerMin);
        hrc = crt::launchQuery(crt::kQueryClosestHit, &q, c->counting, ql.grid, c->stream);
    }
    if (hrc == 0) hrc = crt::launchPreviousPoints(previousPointsParams(c, n, q.inst, q.prim, q.uv, d_point), c->stream);
    return endQuery(c, crt::kQueryClosestHit, n, ql, hrc, stats);
}

int checkFrameMotion(crt_ctx* c, const char* what, uint32_t w, uint32_t h, const void* point)
{
    if (const int rc = checkMotionScene(c, what)) return rc;
    if (const int rc = checkFrameSize(c, what, w, h)) return rc;
    if (!point) return fail(c, CRT_EINVAL, "%s: NULL buffer", what);
    return CRT_OK;
}

} // namespace

int crt_motion_snapshot(crt_ctx* c)
{
    const char* what = "crt_motion_snapshot";
    int rc = checkMotionScene(c, what);
    if (rc) return rc;
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    crt::DynamicScene& d = *c->dyn;
    const size_t bytes = sizeof(float) * 3 * static_cast<size_t>(d.nVerts);
    if (!d.dPrevXyz) HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&d.dPrevXyz), bytes ? bytes : sizeof(float) * 3));
    if (bytes) HIP_TRY(c, hipMemcpyAsync(d.dPrevXyz, d.dWorldXyz, bytes, hipMemcpyDeviceToDevice, c->stream));
    return CRT_OK;
}

int crt_previous_points_device(crt_ctx* c, uint32_t n, const void* d_inst, const void* d_prim, const void* d_uv, void* d_point, crt_frame_stats* stats)
{
    const char* what = "crt_previous_points_device";
    int rc = checkMotionScene(c, what);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (n == 0u) { // nothing to look at, nothing launched
        zeroStats(stats, t0);
        return CRT_OK;
    }
    if (!d_inst || !d_prim || !d_uv || !d_point) return fail(c, CRT_EINVAL, "%s: NULL buffer", what);
    if ((rc = checkDevicePointers(c, what, { d_inst, d_prim, d_point }, 4u)) != CRT_OK) return rc;
    if ((rc = checkDevicePointers(c, what, { d_uv }, 8u)) != CRT_OK) return rc;
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = runPreviousPoints(c, what, n, d_inst, d_prim, d_uv, d_point, stats)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// host buffers: staged through the context's query staging buffer {inst | prim | uv | point}; synchronous
int crt_previous_points(crt_ctx* c, uint32_t n, const uint32_t* inst, const uint32_t* prim, const float* uv, float* point, crt_frame_stats* stats)
{
    const char* what = "crt_previous_points";
    int rc = checkMotionScene(c, what);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (n == 0u) {
        zeroStats(stats, t0);
        return CRT_OK;
    }
    if (!inst || !prim || !uv || !point) return fail(c, CRT_EINVAL, "%s: NULL buffer", what);
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    const size_t nn = n;
    const StagePlane planes[4] = { { inst, nullptr, nn * 4u }, { prim, nullptr, nn * 4u }, { uv, nullptr, nn * 8u }, { nullptr, point, nn * 12u } };
    void* dev[4];
    if ((rc = stageBegin(c, planes, 4, dev)) != CRT_OK) return rc;
    if ((rc = runPreviousPoints(c, what, n, dev[0], dev[1], dev[2], dev[3], stats)) != CRT_OK) return rc;
    if ((rc = stageEnd(c, planes, 4, dev)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

int crt_frame_motion_device(crt_ctx* c, uint32_t w, uint32_t h, void* d_prevPoint, crt_frame_stats* stats)
{
    const char* what = "crt_frame_motion_device";
    int rc = checkFrameMotion(c, what, w, h, d_prevPoint);
    if (rc) return rc;
    if ((rc = checkDevicePointers(c, what, { d_prevPoint }, 4u)) != CRT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    if ((rc = runFrameMotion(c, w, h, d_prevPoint, stats)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// host buffer: staged through the context's query staging buffer; synchronous
int crt_frame_motion(crt_ctx* c, uint32_t w, uint32_t h, float* prevPoint, crt_frame_stats* stats)
{
    const char* what = "crt_frame_motion";
    int rc = checkFrameMotion(c, what, w, h, prevPoint);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    const size_t bytes = static_cast<size_t>(w) * h * 12u;
    if ((rc = reserveRayStage(c, bytes)) != CRT_OK) return rc;
    if ((rc = runFrameMotion(c, w, h, c->dRayStage, stats)) != CRT_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(prevPoint, c->dRayStage, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stampTotal(stats, t0);
    return CRT_OK;
}

// ------------------------------------------------------------------------------------------- gradients (grad_kernels.hip)
namespace {

// The vertex gradient of a backward call: the float64 sums (allocated on first use), zeroed in front of the record kernel and
// rounded into d_grad_xyz behind it.  A call on another stream than the last one's waits for it on the GPU: the sums are the
// context's, not the stream's.  gradSumsZero and gradSumsEnd return HIP error codes, as the launches between them
int gradSumsReserve(crt_ctx* c, void* d_grad_xyz, double*& sums)
{
    sums = nullptr;
    const size_t bytes = sizeof(double) * 3 * static_cast<size_t>(c->dyn->nVerts);
    if (!d_grad_xyz || bytes == 0u) return CRT_OK;
    if (!c->dGradSum) HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&c->dGradSum), bytes));
    sums = c->dGradSum;
    return CRT_OK;
}

int gradSumsZero(crt_ctx* c, double* sums)
{
    if (!sums) return static_cast<int>(hipSuccess);
    if (const hipError_t e = c->gradUsed.wait(c->stream, false)) return static_cast<int>(e);
    return static_cast<int>(hipMemsetAsync(sums, 0, sizeof(double) * 3 * static_cast<size_t>(c->dyn->nVerts), c->stream));
}

int gradSumsEnd(crt_ctx* c, const double* sums, void* d_grad_xyz)
{
    if (!sums) return static_cast<int>(hipSuccess);
    const int hrc = crt::launchGradFinalize(sums, static_cast<float*>(d_grad_xyz), 3 * static_cast<size_t>(c->dyn->nVerts), c->stream);
    return hrc != 0 ? hrc : static_cast<int>(c->gradUsed.record(c->stream));
}

struct RayGradCall {
    const void *rays, *inst, *prim, *t, *uv, *gradT, *gradUv;
    void *gradRays, *gradXyz;
};
struct PointGradCall {
    const void *points, *inst, *prim, *uv, *gradDist;
    void *gradPoints, *gradXyz;
};

int runRayGrad(crt_ctx* c, const char* what, uint32_t n, const RayGradCall& a, crt_frame_stats* stats)
{
    crt::RayGradParams p;
    std::memset(&p, 0, sizeof(p));
    p.table = c->dyn->dTable;
    p.nMeshes = static_cast<uint32_t>(c->dyn->meshes.size());
    p.n = n;
    p.world = c->dyn->dWorldXyz;
    p.idx = c->dyn->dIdx;
    p.rays = static_cast<const float*>(a.rays);
    p.inst = static_cast<const uint32_t*>(a.inst);
    p.prim = static_cast<const uint32_t*>(a.prim);
    p.t = static_cast<const float*>(a.t);
    p.uv = static_cast<const float*>(a.uv);
    p.gradT = static_cast<const float*>(a.gradT);
    p.gradUv = static_cast<const float*>(a.gradUv);
    p.gradRays = static_cast<float*>(a.gradRays);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = gradSumsReserve(c, a.gradXyz, p.sums)) return rc;
    const auto launch = [&] {
        int hrc = gradSumsZero(c, p.sums);
        if (hrc == 0) hrc = crt::launchRayGrad(p, c->stream);
        return hrc != 0 ? hrc : gradSumsEnd(c, p.sums, a.gradXyz);
    };
    if (const int rc = runTimed(c, what, stats, launch)) return rc;
    if (stats) stats->rays_primary = n;
    return CRT_OK;
}

int runPointGrad(crt_ctx* c, const char* what, uint32_t n, const PointGradCall& a, crt_frame_stats* stats)
{
    crt::PointGradParams p;
    std::memset(&p, 0, sizeof(p));
    p.table = c->dyn->dTable;
    p.nMeshes = static_cast<uint32_t>(c->dyn->meshes.size());
    p.n = n;
    p.world = c->dyn->dWorldXyz;
    p.idx = c->dyn->dIdx;
    p.points = static_cast<const float*>(a.points);
    p.inst = static_cast<const uint32_t*>(a.inst);
    p.prim = static_cast<const uint32_t*>(a.prim);
    p.uv = static_cast<const float*>(a.uv);
    p.gradDist = static_cast<const float*>(a.gradDist);
    p.gradPoints = static_cast<float*>(a.gradPoints);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = gradSumsReserve(c, a.gradXyz, p.sums)) return rc;
    const auto launch = [&] {
        int hrc = gradSumsZero(c, p.sums);
        if (hrc == 0) hrc = crt::launchPointGrad(p, c->stream);
        return hrc != 0 ? hrc : gradSumsEnd(c, p.sums, a.gradXyz);
    };
    if (const int rc = runTimed(c, what, stats, launch)) return rc;
    if (stats) stats->rays_primary = n;
    return CRT_OK;
}

int checkRayGrad(crt_ctx* c, const char* what, const RayGradCall& a)
{
    if (!a.rays || !a.inst || !a.prim || !a.t || !a.uv) return fail(c, CRT_EINVAL, "%s: NULL buffer", what);
    if (!a.gradT && !a.gradUv) return fail(c, CRT_EINVAL, "%s: grad_t and grad_uv are both NULL", what);
    if (!a.gradRays && !a.gradXyz) return fail(c, CRT_EINVAL, "%s: every output is NULL", what);
    return CRT_OK;
}

int checkPointGrad(crt_ctx* c, const char* what, const PointGradCall& a)
{
    if (!a.points || !a.inst || !a.prim || !a.uv || !a.gradDist) return fail(c, CRT_EINVAL, "%s: NULL buffer", what);
    if (!a.gradPoints && !a.gradXyz) return fail(c, CRT_EINVAL, "%s: every output is NULL", what);
    return CRT_OK;
}

size_t gradXyzBytes(const crt_ctx* c) { return sizeof(float) * 3 * static_cast<size_t>(c->dyn->nVerts); }

} // namespace

int crt_trace_rays_backward_device(crt_ctx* c, uint32_t n, const void* d_rays, const void* d_inst, const void* d_prim, const void* d_t,
                                   const void* d_uv, const void* d_grad_t, const void* d_grad_uv, void* d_grad_rays, void* d_grad_xyz,
                                   crt_frame_stats* stats)
{
    const char* what = "crt_trace_rays_backward_device";
    int rc = checkMotionScene(c, what);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (n == 0u) { // nothing to look at, nothing launched
        zeroStats(stats, t0);
        return CRT_OK;
    }
    const RayGradCall a{ d_rays, d_inst, d_prim, d_t, d_uv, d_grad_t, d_grad_uv, d_grad_rays, d_grad_xyz };
    if ((rc = checkRayGrad(c, what, a)) != CRT_OK) return rc;
    if ((rc = checkDevicePointers(c, what, { d_rays, d_grad_rays }, 16u)) != CRT_OK) return rc;
    if ((rc = checkDevicePointers(c, what, { d_uv, d_grad_uv }, 8u)) != CRT_OK) return rc;
    if ((rc = checkDevicePointers(c, what, { d_inst, d_prim, d_t, d_grad_t, d_grad_xyz }, 4u)) != CRT_OK) return rc;
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    if ((rc = runRayGrad(c, what, n, a, stats)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// host buffers: staged through the context's query staging buffer {rays | inst | prim | t | uv | grad_t | grad_uv | grad_rays |
// grad_xyz}; synchronous
int crt_trace_rays_backward(crt_ctx* c, uint32_t n, const float* rays, const uint32_t* inst, const uint32_t* prim, const float* t, const float* uv,
                            const float* grad_t, const float* grad_uv, float* grad_rays, float* grad_xyz, crt_frame_stats* stats)
{
    const char* what = "crt_trace_rays_backward";
    int rc = checkMotionScene(c, what);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (n == 0u) {
        zeroStats(stats, t0);
        return CRT_OK;
    }
    if ((rc = checkRayGrad(c, what, { rays, inst, prim, t, uv, grad_t, grad_uv, grad_rays, grad_xyz })) != CRT_OK) return rc;
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    const size_t nn = n;
    const StagePlane planes[9] = { { rays, nullptr, nn * 32u }, { inst, nullptr, nn * 4u }, { prim, nullptr, nn * 4u }, { t, nullptr, nn * 4u },
                                   { uv, nullptr, nn * 8u }, { grad_t, nullptr, nn * 4u }, { grad_uv, nullptr, nn * 8u },
                                   { nullptr, grad_rays, nn * 32u }, { nullptr, grad_xyz, gradXyzBytes(c) } };
    void* dev[9];
    if ((rc = stageBegin(c, planes, 9, dev)) != CRT_OK) return rc;
    if ((rc = runRayGrad(c, what, n, { dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], dev[8] }, stats)) != CRT_OK) return rc;
    if ((rc = stageEnd(c, planes, 9, dev)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

int crt_closest_points_backward_device(crt_ctx* c, uint32_t n, const void* d_points, const void* d_inst, const void* d_prim, const void* d_uv,
                                       const void* d_grad_dist, void* d_grad_points, void* d_grad_xyz, crt_frame_stats* stats)
{
    const char* what = "crt_closest_points_backward_device";
    int rc = checkMotionScene(c, what);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (n == 0u) {
        zeroStats(stats, t0);
        return CRT_OK;
    }
    const PointGradCall a{ d_points, d_inst, d_prim, d_uv, d_grad_dist, d_grad_points, d_grad_xyz };
    if ((rc = checkPointGrad(c, what, a)) != CRT_OK) return rc;
    if ((rc = checkDevicePointers(c, what, { d_points, d_grad_points }, 16u)) != CRT_OK) return rc;
    if ((rc = checkDevicePointers(c, what, { d_uv }, 8u)) != CRT_OK) return rc;
    if ((rc = checkDevicePointers(c, what, { d_inst, d_prim, d_grad_dist, d_grad_xyz }, 4u)) != CRT_OK) return rc;
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    if ((rc = runPointGrad(c, what, n, a, stats)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// host buffers: staged {points | inst | prim | uv | grad_dist | grad_points | grad_xyz}; synchronous
int crt_closest_points_backward(crt_ctx* c, uint32_t n, const float* points, const uint32_t* inst, const uint32_t* prim, const float* uv,
                                const float* grad_dist, float* grad_points, float* grad_xyz, crt_frame_stats* stats)
{
    const char* what = "crt_closest_points_backward";
    int rc = checkMotionScene(c, what);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if (n == 0u) {
        zeroStats(stats, t0);
        return CRT_OK;
    }
    if ((rc = checkPointGrad(c, what, { points, inst, prim, uv, grad_dist, grad_points, grad_xyz })) != CRT_OK) return rc;
    if ((rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
    const size_t nn = n;
    const StagePlane planes[7] = { { points, nullptr, nn * 16u }, { inst, nullptr, nn * 4u }, { prim, nullptr, nn * 4u }, { uv, nullptr, nn * 8u },
                                   { grad_dist, nullptr, nn * 4u }, { nullptr, grad_points, nn * 16u }, { nullptr, grad_xyz, gradXyzBytes(c) } };
    void* dev[7];
    if ((rc = stageBegin(c, planes, 7, dev)) != CRT_OK) return rc;
    if ((rc = runPointGrad(c, what, n, { dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6] }, stats)) != CRT_OK) return rc;
    if ((rc = stageEnd(c, planes, 7, dev)) != CRT_OK) return rc;
    stampTotal(stats, t0);
    return CRT_OK;
}

// ------------------------------------------------------------------------------------------- native RCCL gather
// One process per GPU; every rank renders its macro tiles into a tile-major staging buffer, ONE ncclAllGather per frame moves
// them over xGMI (1 044 480 bytes per rank at 1080p / 8 GPUs, each rank's 7 inbound messages on 7 different links), the
// untile kernel rebuilds the row-major frame: all on the context's stream, no host synchronisation in between.
// RCCL is resolved at run time (dlopen): a process that already carries an RCCL (torch's librccl.so.1) shares that copy, a
// C++-only process takes /opt/rocm/lib's; a process that never calls crt_comm_* needs none.
namespace {
struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*getUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*commInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*commDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*allGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*getErrorString)(ncclResult_t) = nullptr;
    std::string error;
};

// loaded once, whichever thread asks first (the initialiser of a function-local static runs exactly once; later callers wait for it)
RcclApi loadRccl()
{
    RcclApi api;
    for (const char* name : { "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so" }) {
        api.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (api.handle) break;
    }
    if (!api.handle) {
        const char* why = dlerror(); // may be NULL
        api.error = std::string("cannot load RCCL (librccl.so.1): ") + (why ? why : "unknown dlopen error");
        return api;
    }
    api.getUniqueId = reinterpret_cast<decltype(api.getUniqueId)>(dlsym(api.handle, "ncclGetUniqueId"));
    api.commInitRank = reinterpret_cast<decltype(api.commInitRank)>(dlsym(api.handle, "ncclCommInitRank"));
    api.commDestroy = reinterpret_cast<decltype(api.commDestroy)>(dlsym(api.handle, "ncclCommDestroy"));
    api.allGather = reinterpret_cast<decltype(api.allGather)>(dlsym(api.handle, "ncclAllGather"));
    api.getErrorString = reinterpret_cast<decltype(api.getErrorString)>(dlsym(api.handle, "ncclGetErrorString"));
    if (!api.getUniqueId || !api.commInitRank || !api.commDestroy || !api.allGather || !api.getErrorString) {
        api.error = "RCCL library lacks an expected entry point";
        api.handle = nullptr;
    }
    return api;
}

RcclApi& rccl()
{
    static RcclApi api = loadRccl();
    return api;
}

} // namespace

int crt_comm_unique_id(void* id_out)
{
    if (!id_out) return fail(nullptr, CRT_EINVAL, "crt_comm_unique_id: NULL argument");
    RcclApi& api = rccl();
    if (!api.handle) return fail(nullptr, CRT_ENODEVICE, "%s", api.error.c_str());
    ncclUniqueId id;
    const ncclResult_t r = api.getUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, CRT_EHIP, "ncclGetUniqueId failed: %s", api.getErrorString(r));
    static_assert(sizeof(id) == CRT_COMM_ID_BYTES, "crt_hip.h states the size of an RCCL unique id");
    std::memcpy(id_out, &id, sizeof(id));
    return CRT_OK;
}

int crt_comm_init(crt_ctx* c, uint32_t rank, uint32_t n_ranks, const void* unique_id)
{
    if (!c) return CRT_EINVAL;
    if (!unique_id || n_ranks == 0 || rank >= n_ranks) return fail(c, CRT_EINVAL, "crt_comm_init: bad arguments (rank %u of %u)", rank, n_ranks);
    if (c->comm) return fail(c, CRT_ESTATE, "crt_comm_init: the context already has a communicator (crt_comm_destroy first)");
    RcclApi& api = rccl();
    if (!api.handle) return fail(c, CRT_ENODEVICE, "%s", api.error.c_str());
    HIP_TRY(c, hipSetDevice(c->device));
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    const ncclResult_t r = api.commInitRank(&c->comm, static_cast<int>(n_ranks), id, static_cast<int>(rank));
    if (r != ncclSuccess) {
        c->comm = nullptr;
        return fail(c, CRT_EHIP, "ncclCommInitRank(rank %u of %u) failed: %s", rank, n_ranks, api.getErrorString(r));
    }
    c->commRank = rank;
    c->commRanks = n_ranks;
    return CRT_OK;
}

// ---- the same frame assembly with shared host memory as the transport: for ranks that share ONE GPU (RCCL refuses that), i.e. for
// rehearsing the multi-rank path on a one-GPU machine, and as a fallback where RCCL cannot be loaded.  A POSIX shared-memory object
// holds a header (arrival counter + generation of a sense-reversing barrier) and the ranks' tile slices; per frame: copy the own
// slice in, barrier, copy all slices out, barrier.  Never a measurement of anything.
struct HostExchange {
    struct Header {
        std::atomic<uint32_t> magic, arrive, generation;
        uint32_t nRanks;
        uint64_t capacity;
    };
    static constexpr uint32_t kMagic = 0x43525431u;
    static constexpr size_t kDataAt = 4096;
    int fd = -1;
    void* map = nullptr;
    size_t bytes = 0;
    std::string name;
    bool owner = false;
    Header* header() const { return static_cast<Header*>(map); }
    unsigned char* data() const { return static_cast<unsigned char*>(map) + kDataAt; }
    bool barrier(uint32_t n) const // false: a peer did not arrive within a minute
    {
        Header* h = header();
        const uint32_t gen = h->generation.load(std::memory_order_acquire);
        if (h->arrive.fetch_add(1, std::memory_order_acq_rel) + 1 == n) {
            h->arrive.store(0, std::memory_order_relaxed);
            h->generation.fetch_add(1, std::memory_order_acq_rel);
            return true;
        }
        const auto t0 = std::chrono::steady_clock::now();
        while (h->generation.load(std::memory_order_acquire) == gen) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) return false;
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        return true;
    }
    void close()
    {
        if (map) munmap(map, bytes);
        if (fd >= 0) ::close(fd);
        if (owner && !name.empty()) shm_unlink(name.c_str());
        map = nullptr;
        fd = -1;
    }
};

int crt_comm_init_host(crt_ctx* c, uint32_t rank, uint32_t n_ranks, const char* name)
{
    if (!c) return CRT_EINVAL;
    if (!name || name[0] != '/' || n_ranks == 0 || rank >= n_ranks) return fail(c, CRT_EINVAL, "crt_comm_init_host: bad arguments (rank %u of %u, name must start with '/')", rank, n_ranks);
    if (c->comm || c->hostComm) return fail(c, CRT_ESTATE, "crt_comm_init_host: the context already has a communicator (crt_comm_destroy first)");
    std::unique_ptr<HostExchange> x(new HostExchange);
    x->name = name;
    x->bytes = HostExchange::kDataAt + (size_t(1) << 28); // room for a 8K RGBA8 frame; pages are only taken when touched
    if (rank == 0) {
        x->fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
        if (x->fd < 0) return fail(c, CRT_EIO, "crt_comm_init_host: cannot create shared memory '%s': %s", name, std::strerror(errno));
        x->owner = true;
        if (ftruncate(x->fd, static_cast<off_t>(x->bytes)) != 0) {
            const int e = errno;
            x->close();
            return fail(c, CRT_EIO, "crt_comm_init_host: cannot size '%s': %s", name, std::strerror(e));
        }
    } else {
        for (int tries = 0; tries < 6000 && x->fd < 0; tries++) { // up to 60 s for rank 0 to come up
            x->fd = shm_open(name, O_RDWR, 0600);
            if (x->fd < 0) std::this_thread::sleep_for(std::chrono::milliseconds(10));
        }
        if (x->fd < 0) return fail(c, CRT_EIO, "crt_comm_init_host: rank %u found no shared memory '%s'", rank, name);
        struct stat st;
        for (int tries = 0; tries < 6000; tries++) { // ... and to size it
            if (fstat(x->fd, &st) == 0 && static_cast<size_t>(st.st_size) >= x->bytes) break;
            std::this_thread::sleep_for(std::chrono::milliseconds(10));
        }
    }
    x->map = mmap(nullptr, x->bytes, PROT_READ | PROT_WRITE, MAP_SHARED, x->fd, 0);
    if (x->map == MAP_FAILED) {
        const int e = errno;
        x->map = nullptr;
        x->close();
        return fail(c, CRT_EIO, "crt_comm_init_host: cannot map '%s': %s", name, std::strerror(e));
    }
    HostExchange::Header* h = x->header();
    if (rank == 0) {
        h->arrive.store(0);
        h->generation.store(0);
        h->nRanks = n_ranks;
        h->capacity = x->bytes - HostExchange::kDataAt;
        h->magic.store(HostExchange::kMagic, std::memory_order_release);
    } else {
        int tries = 0;
        while (h->magic.load(std::memory_order_acquire) != HostExchange::kMagic && tries++ < 6000) std::this_thread::sleep_for(std::chrono::milliseconds(10));
        if (h->magic.load(std::memory_order_acquire) != HostExchange::kMagic || h->nRanks != n_ranks) {
            x->close();
            return fail(c, CRT_EIO, "crt_comm_init_host: '%s' is not this launch's exchange (%u ranks expected)", name, n_ranks);
        }
    }
    if (!x->barrier(n_ranks)) { // collective, like crt_comm_init: everybody is attached before anybody goes on (and before rank 0 may unlink)
        x->close();
        return fail(c, CRT_EIO, "crt_comm_init_host: not all %u ranks arrived within a minute", n_ranks);
    }
    c->hostComm = x.release();
    c->commRank = rank;
    c->commRanks = n_ranks;
    return CRT_OK;
}

int crt_comm_destroy(crt_ctx* c)
{
    if (!c) return CRT_EINVAL;
    if (c->hostComm) {
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        c->hostComm->close();
        delete c->hostComm;
        c->hostComm = nullptr;
        c->commRanks = 0;
        return CRT_OK;
    }
    if (!c->comm) return CRT_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    const ncclResult_t r = rccl().commDestroy(c->comm);
    c->comm = nullptr;
    c->commRanks = 0;
    return r == ncclSuccess ? CRT_OK : fail(c, CRT_EHIP, "ncclCommDestroy failed: %s", rccl().getErrorString(r));
}

int crt_comm_info(const crt_ctx* c, uint32_t* rank, uint32_t* n_ranks)
{
    if (!c) return CRT_EINVAL;
    if (rank) *rank = c->commRank;
    if (n_ranks) *n_ranks = c->commRanks; // 0: no communicator
    return CRT_OK;
}

int crt_render_frame_distributed(crt_ctx* c, uint32_t w, uint32_t h, void* d_rgba8, uint8_t* host_rgba8, crt_frame_stats* stats)
{
    int rc = checkRenderable(c, w, h);
    if (rc) return rc;
    if (!c->comm && !c->hostComm) return fail(c, CRT_ESTATE, "crt_render_frame_distributed: no communicator (crt_comm_init first)");
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t n = c->commRanks, slots = crt_tile_slots(w, h, n);
    const size_t per = static_cast<size_t>(slots) * crt::kTile * crt::kTile * 4; // bytes each rank contributes
    crt_ctx::DistSlot& d = c->dist[c->distSerial++ % crt_ctx::kRing];
    if ((rc = ensureBuffer(c, &d.stage, &d.stageBytes, per)) != CRT_OK) return rc;
    if ((rc = ensureBuffer(c, &d.gathered, &d.gatheredBytes, per * n)) != CRT_OK) return rc;
    void* frame = d_rgba8;
    if (!frame) {
        if ((rc = ensureBuffer(c, &d.frame, &d.frameBytes, static_cast<size_t>(w) * h * 4)) != CRT_OK) return rc;
        frame = d.frame;
    }
    // the slot's previous frame (4 frames ago) may have been issued on another stream: order behind it on the GPU
    HIP_TRY(c, d.done.wait(c->stream, false));
    crt_frame_stats local;
    rc = crt_render_tiles_device(c, w, h, c->commRank, n, d.stage, stats ? &local : nullptr);
    if (rc) return rc;
    if (c->comm) {
        const ncclResult_t r = rccl().allGather(d.stage, d.gathered, per, ncclUint8, c->comm, c->stream);
        if (r != ncclSuccess) return fail(c, CRT_EHIP, "ncclAllGather failed: %s", rccl().getErrorString(r));
    } else { // through shared host memory: own slice in, everybody waits, all slices out, everybody waits again before the next frame's writes
        HostExchange* x = c->hostComm;
        if (per * n > x->header()->capacity) return fail(c, CRT_EINVAL, "crt_render_frame_distributed: frame too large for the host exchange");
        HIP_TRY(c, hipMemcpyAsync(x->data() + per * c->commRank, d.stage, per, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!x->barrier(n)) return fail(c, CRT_EIO, "crt_render_frame_distributed: a rank did not deliver its tiles within a minute");
        HIP_TRY(c, hipMemcpyAsync(d.gathered, x->data(), per * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!x->barrier(n)) return fail(c, CRT_EIO, "crt_render_frame_distributed: a rank did not collect the tiles within a minute");
    }
    rc = crt_untile_device(c, w, h, n, d.gathered, frame);
    if (rc) return rc;
    if (host_rgba8) HIP_TRY(c, hipMemcpyAsync(host_rgba8, frame, static_cast<size_t>(w) * h * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, d.done.record(c->stream));
    if (stats || host_rgba8) HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (stats) {
        *stats = local; // kernel_ms and the counters describe this rank's tile launch
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return CRT_OK;
}

// ------------------------------------------------------------------------------------------- scene layer
int crt_scene_load(const char* path, crt_scene** out, char* err, size_t err_len)
{
    if (!path || !out) return CRT_EINVAL;
    *out = nullptr;
    crt_scene* s = new (std::nothrow) crt_scene();
    if (!s) return CRT_ENOMEM;
    try {
        s->scene.parseSceneFile(path);
    } catch (const std::exception& ex) {
        if (err && err_len) snprintf(err, err_len, "%s", ex.what());
        delete s;
        return std::strstr(ex.what(), "cannot open") ? CRT_EIO : CRT_EPARSE;
    }
    *out = s;
    return CRT_OK;
}

int crt_scene_save(const crt_scene* s, const char* path, char* err, size_t err_len)
{
    if (!s || !path) return CRT_EINVAL;
    try {
        crt::SceneParser::saveBinary(path, s->scene);
    } catch (const std::exception& ex) {
        if (err && err_len) snprintf(err, err_len, "%s", ex.what());
        return CRT_EIO;
    }
    return CRT_OK;
}

int crt_scene_new(crt_scene** out)
{
    if (!out) return CRT_EINVAL;
    *out = new (std::nothrow) crt_scene();
    return *out ? CRT_OK : CRT_ENOMEM;
}

void crt_scene_free(crt_scene* s) { delete s; }

int crt_scene_add_mesh(crt_scene* s, const float* xyz, uint32_t nv, const uint32_t* idx, uint32_t nt, int32_t material_index)
{
    if (!s || (!xyz && nv) || (!idx && nt)) return CRT_EINVAL;
    for (uint32_t i = 0; i < 3 * nt; i++)
        if (idx[i] >= nv) return CRT_EINVAL;
    crt::Mesh& m = s->scene.addObject();
    m.reserve(nv, 3 * static_cast<size_t>(nt));
    for (uint32_t i = 0; i < nv; i++) m.addVertex(crt::Vector(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
    for (uint32_t i = 0; i < 3 * nt; i++) m.addIndex(static_cast<int>(idx[i]));
    m.setMaterialIndex(material_index);
    m.calculateVertexNormals();
    return CRT_OK;
}

int crt_scene_add_light(crt_scene* s, const float pos[3], float intensity)
{
    if (!s || !pos) return CRT_EINVAL;
    s->scene.addLight(crt::Light(crt::Vector(pos[0], pos[1], pos[2]), intensity));
    return CRT_OK;
}

int crt_scene_add_material(crt_scene* s, const crt_material* m)
{
    if (!s || !m) return CRT_EINVAL;
    crt::Material mat;
    mat.setType(static_cast<crt::MaterialType>(m->type <= 4 ? m->type : 0));
    mat.setAlbedo(crt::Vector(m->albedo[0], m->albedo[1], m->albedo[2]));
    mat.setSmoothShading(m->smooth != 0);
    mat.setIor(m->ior);
    s->scene.addMaterial(mat);
    return CRT_OK;
}

uint32_t crt_scene_mesh_count(const crt_scene* s) { return s ? static_cast<uint32_t>(s->scene.getObjects().size()) : 0; }

int crt_scene_mesh(const crt_scene* s, uint32_t i, crt_mesh_view* out)
{
    if (!s || !out || i >= s->scene.getObjects().size()) return CRT_EINVAL;
    const crt::Mesh& m = s->scene.getObjects()[i];
    out->xyz = m.getVertices().empty() ? nullptr : m.getVertices().data()->data();
    out->idx = reinterpret_cast<const uint32_t*>(m.getIndices().data());
    out->normals = m.getVertexNormals().size() == m.getVertices().size() && !m.getVertexNormals().empty()
                       ? m.getVertexNormals().data()->data() : nullptr;
    out->uvs = (m.getUV().size() == m.getVertices().size() && !m.getUV().empty()) ? m.getUV().data()->data() : nullptr;
    out->n_vertices = static_cast<uint32_t>(m.getVertices().size());
    out->n_triangles = static_cast<uint32_t>(m.getIndices().size() / 3);
    out->material_index = m.getMaterialIndex();
    return CRT_OK;
}

uint32_t crt_scene_light_count(const crt_scene* s) { return s ? static_cast<uint32_t>(s->scene.getLights().size()) : 0; }

int crt_scene_light(const crt_scene* s, uint32_t i, crt_light* out)
{
    if (!s || !out || i >= s->scene.getLights().size()) return CRT_EINVAL;
    const crt::Light& l = s->scene.getLights()[i];
    crt::copyBytes(out->pos, l.getPosition().data(), 12);
    out->intensity = l.getIntensity();
    return CRT_OK;
}

uint32_t crt_scene_material_count(const crt_scene* s) { return s ? static_cast<uint32_t>(s->scene.getMaterials().size()) : 0; }

int crt_scene_material(const crt_scene* s, uint32_t i, crt_material* out)
{
    if (!s || !out || i >= s->scene.getMaterials().size()) return CRT_EINVAL;
    const crt::Material& m = s->scene.getMaterials()[i];
    crt::copyBytes(out->albedo, m.getAlbedo().data(), 12);
    out->type = static_cast<uint32_t>(m.getType());
    out->smooth = m.isSmoothShading() ? 1u : 0u;
    out->ior = m.getIor();
    out->texture = m.isTexture() ? s->scene.textureIndexByName(m.getTextureName()) : -1; // getTextureByName, R/CRTScene.cpp:52-63
    return CRT_OK;
}

uint32_t crt_scene_texture_count(const crt_scene* s) { return s ? static_cast<uint32_t>(s->scene.getTextures().size()) : 0; }

int crt_scene_texture_color(const crt_scene* s, uint32_t i, float u, float v, float out_rgb[3])
{
    if (!s || !out_rgb || i >= s->scene.getTextures().size()) return CRT_EINVAL;
    const crt::Vector c = s->scene.getTextures()[i].getColor(u, v);
    crt::copyBytes(out_rgb, c.data(), 12);
    return CRT_OK;
}

int crt_scene_add_texture(crt_scene* s, const char* name, const char* type, const float color_a[3], const float color_b[3], float scalar,
                          const char* file_path)
{
    if (!s || !name || !type) return CRT_EINVAL;
    crt::TextureDesc t;
    t.name = name;
    t.type = type;
    if (t.type != "albedo" && t.type != "edges" && t.type != "checker" && t.type != "bitmap") return CRT_EINVAL;
    if (color_a) t.colorA = crt::Vector(color_a[0], color_a[1], color_a[2]);
    if (color_b) t.colorB = crt::Vector(color_b[0], color_b[1], color_b[2]);
    t.scalar = scalar;
    if (file_path) t.filePath = file_path;
    if (t.typeCode() == 3u) {
        try {
            t.loadBitmap(std::string());
        } catch (const std::exception&) {
            return CRT_EIO;
        }
    }
    s->scene.addTexture(t);
    return CRT_OK;
}

int crt_scene_set_material_texture(crt_scene* s, uint32_t material, const char* texture_name)
{
    if (!s || !texture_name || material >= s->scene.getMaterials().size()) return CRT_EINVAL;
    s->scene.materialsRef()[material].setTextureName(texture_name);
    return CRT_OK;
}

int crt_scene_set_mesh_uvs(crt_scene* s, uint32_t mesh, const float* uvs)
{
    if (!s || !uvs || mesh >= s->scene.getObjects().size()) return CRT_EINVAL;
    crt::Mesh& m = s->scene.objectsRef()[mesh];
    std::vector<crt::Vector> uv(m.getVertices().size());
    for (size_t i = 0; i < uv.size(); i++) uv[i] = crt::Vector(uvs[3 * i], uvs[3 * i + 1], uvs[3 * i + 2]);
    m.setUVs(std::move(uv));
    return CRT_OK;
}

int crt_scene_settings(const crt_scene* s, uint32_t* width, uint32_t* height, float background_rgb[3])
{
    if (!s) return CRT_EINVAL;
    const crt::Settings& st = s->scene.getSettings();
    if (width) *width = static_cast<uint32_t>(st.imageWidth);
    if (height) *height = static_cast<uint32_t>(st.imageHeight);
    if (background_rgb) crt::copyBytes(background_rgb, st.backgroundColor.data(), 12);
    return CRT_OK;
}

int crt_scene_camera_get(const crt_scene* s, float pos[3], float rot[9])
{
    if (!s) return CRT_EINVAL;
    if (pos) crt::copyBytes(pos, s->scene.getCamera().getPosition().data(), 12);
    if (rot) crt::copyBytes(rot, s->scene.getCamera().getRotationMatrix().data(), 36);
    return CRT_OK;
}

int crt_scene_camera_set(crt_scene* s, const float pos[3], const float rot[9])
{
    if (!s) return CRT_EINVAL;
    if (pos) s->scene.getCamera().setPosition(crt::Vector(pos[0], pos[1], pos[2]));
    if (rot) s->scene.getCamera().setRotationMatrix(crt::Matrix(rot[0], rot[1], rot[2], rot[3], rot[4], rot[5], rot[6], rot[7], rot[8]));
    return CRT_OK;
}

#define CAMERA_OP(name, call)                        \
    int name                                         \
    {                                                \
        if (!s) return CRT_EINVAL;                   \
        s->scene.getCamera().call;                   \
        return CRT_OK;                               \
    }
CAMERA_OP(crt_scene_camera_rotate(crt_scene* s, float dyaw, float dpitch), rotate(dyaw, dpitch))
CAMERA_OP(crt_scene_camera_zoom(crt_scene* s, float amount), zoom(amount))
CAMERA_OP(crt_scene_camera_move_forward(crt_scene* s, float d), moveForward(d))
CAMERA_OP(crt_scene_camera_move_right(crt_scene* s, float d), moveRight(d))
CAMERA_OP(crt_scene_camera_pan(crt_scene* s, float deg), pan(deg))
CAMERA_OP(crt_scene_camera_tilt(crt_scene* s, float deg), tilt(deg))
CAMERA_OP(crt_scene_camera_roll(crt_scene* s, float deg), roll(deg))
#undef CAMERA_OP

int crt_scene_camera_pan_around_target(crt_scene* s, float degrees, const float target[3])
{
    if (!s || !target) return CRT_EINVAL;
    s->scene.getCamera().panAroundTarget(degrees, crt::Vector(target[0], target[1], target[2]));
    return CRT_OK;
}

int crt_upload_scene_from(crt_ctx* c, const crt_scene* s)
{
    if (!c) return CRT_EINVAL;
    if (!s) return fail(c, CRT_EINVAL, "scene is NULL");
    const uint32_t nm = crt_scene_mesh_count(s), nl = crt_scene_light_count(s), nmat = crt_scene_material_count(s);
    std::vector<crt_mesh_view> meshes(nm);
    std::vector<crt_light> lights(nl);
    std::vector<crt_material> mats(nmat);
    for (uint32_t i = 0; i < nm; i++) crt_scene_mesh(s, i, &meshes[i]);
    for (uint32_t i = 0; i < nl; i++) crt_scene_light(s, i, &lights[i]);
    for (uint32_t i = 0; i < nmat; i++) crt_scene_material(s, i, &mats[i]);
    int rc = crt_upload_scene(c, meshes.data(), nm, lights.data(), nl, mats.data(), nmat);
    if (rc) return rc;
    std::vector<crt_texture> tex;
    for (const crt::TextureDesc& t : s->scene.getTextures()) {
        crt_texture x{};
        x.type = t.typeCode();
        crt::copyBytes(x.color_a, t.colorA.data(), 12);
        crt::copyBytes(x.color_b, t.colorB.data(), 12);
        x.scalar = t.scalar;
        x.pixels = t.pixels.empty() ? nullptr : t.pixels.data();
        x.width = static_cast<uint32_t>(t.width);
        x.height = static_cast<uint32_t>(t.height);
        x.channels = static_cast<uint32_t>(t.channels);
        tex.push_back(x);
    }
    rc = crt_set_textures(c, tex.data(), static_cast<uint32_t>(tex.size()));
    if (rc) return rc;
    return crt_set_camera_from(c, s);
}

int crt_set_camera_from(crt_ctx* c, const crt_scene* s)
{
    if (!c) return CRT_EINVAL;
    if (!s) return fail(c, CRT_EINVAL, "scene is NULL");
    return crt_set_camera(c, s->scene.getCamera().getPosition().data(), s->scene.getCamera().getRotationMatrix().data());
}

} // extern "C"
