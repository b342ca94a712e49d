// Internal to the C-ABI layer (host C++ only): the renderer context and what more than one of the layer's units uses.
//   crt_api.cpp      context, streams, options, scene upload, tree exports; defines the shared helpers declared here
//   api_frames.cpp   the per-frame path: runRender, launch-order feedback, accumulation, frame / tile / batch entry points
//   api_queries.cpp  ray, point, shaded, Whitted, ambient-occlusion, path and listing queries
//   api_image.cpp    camera rays, frame guides, the a-trous filters, temporal reprojection and variance
//   api_dynamic.cpp  vertex updates, transforms, refit / rebuild, motion, gradients
//   api_comm.cpp     RCCL gather and the host-memory exchange
//   api_scene.cpp    the crt_scene_* layer (no context, no HIP: it does not include this header)
// Helpers the units share live in namespace crtapi; what a unit keeps to itself stands in its unnamed namespace.  Only the crt_*
// functions carry C names (from their declarations in the public header), and exports.map keeps all the rest out of the library's
// dynamic symbol table.
#pragma once

#include "../../include/crt_hip.h"

#include "bvh_build.h"
#include "refit.h"
#include "render_kernels.h"

#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <initializer_list>
#include <string>

struct ncclComm; // <rccl/rccl.h> is api_comm.cpp's alone
typedef struct ncclComm* ncclComm_t;
struct HostExchange; // api_comm.cpp

// "The work enqueued on a stream up to here": an event, the stream it was last recorded on, and whether it was recorded at all.
// Everything on the context that one call leaves behind for a later call, possibly on another stream, is guarded by one.
namespace crtapi {
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
} // namespace crtapi

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
    float binLo[3] = { 0.f, 0.f, 0.f }, binHi[3] = { 0.f, 0.f, 0.f };     // the same box in full precision, from node 0 of the binary tree
                                                                          // (crt_bvh_export): what "ao_radius" is a fraction of

    float pos[3] = { 0.f, 0.f, 0.f };
    float rot[9] = { 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f };
    float miss[3] = { 0.f, 1.f, 1.f }; // hlsl:75
    uint32_t mode = 0;                 // R/DXRTRenderer.h:246 default shading mode
    bool counting = false;
    uint32_t pathSpp = 4, pathBounces = 3, pathSeed = 1234; // mode 200 (BASELINE.json configs[4]: 4 spp, 3 bounces)
    uint32_t phongKsPermille = 0, phongExp = 32;            // mode 100: specular term, off by default
    uint32_t aoSamples = 16, aoRadiusPermille = 0, aoSky = 0; // mode 120: occlusion rays per hit, their reach (0: unbounded), sky colour
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
    // launch order from measured costs of an earlier frame: 0 never, 1 always, 2 (default) only for frames issued on the
    // same stream as the frame before.  Such frames run one after another, and starting the packets on the longest
    // critical paths first shortens each of them (0.52 -> 0.43 ms on the 1M-triangle frame); frames issued on
    // alternating streams overlap, the tail of one fills with the head of the next, so the order has nothing left to
    // gain and its bookkeeping only adds cross-stream dependencies (0.43 vs 0.40 ms per frame with 4 in flight).
    int adaptiveOrder = 2;
    bool debugForceMeasure = false;  // diagnostics: measure and sort at every frame even for an unchanged view
    uint32_t tuneRemeasureEvery = 1; // a changing view re-measures at every use of a slot: stale orders cost more than the measuring (tools/moving_camera.py)
    bool wantTimeline = false;       // diagnostics, option "timeline": frames.dTimeline
    // lists of up to this many hits are sorted by one lane, longer ones by a wavefront.  Measured (DESIGN.md section 5d,
    // tools/list_hits_bench.py, lists of 0 .. 1024 hits): 2.89 ms from 4 to 24, 2.92 at 32, 2.93 at 64 (all within the 1 %
    // spread of the rounds), 3.02 at 256, 3.93 with every list on one lane.  Any value up to ~64 would do.
    uint32_t tuneListShortMax = 24;
    uint32_t viewSerial = 1;         // bumped when camera, mode or path settings change (crt_api.cpp): costs must be measured again (api_frames.cpp)
    uint32_t textureSerial = 0;      // bumped by crt_set_textures
    unsigned long long* dCounters = nullptr;

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
        uint32_t orderFrame = 0;       // frames.serial of the last measurement
        crtapi::Fence rendered;        // the slot's last frame, on the stream it ran on
        crtapi::Fence sorted;          // the sort of that frame's costs, on the side stream
    };
    // Scratch that belongs to the stream that last used it: calls issued on one stream run one after the other and share ONE
    // arena; only calls on different streams (up to kRing in flight) get arenas of their own (takeArena).
    struct Arena {
        unsigned char* mem = nullptr;
        size_t bytes = 0;
        bool used = false;       // lastUse.stream is meaningful
        crtapi::Fence lastUse;   // of the last call that used the arena; its stream is the arena's OWNER, set when a stream takes
                                 // the arena (before anything is recorded) and the only stream that ever records it
        uint32_t serial = 0;     // of the last use (the least recently used arena is taken over by a new stream)
    };

    // ---- What follows belongs to one unit each: a group's members are named in that unit alone, and in crt_create / crt_destroy /
    // freeScene (their lifetime).  What more than one unit reads or writes stands flat, above and between the groups.

    // api_frames.cpp: the per-frame path
    struct Frames {
        FrameSlot slot[kRing];
        uint32_t unitCapacity = 0;       // of every slot's cost and order buffer: the four grow together
        uint32_t serial = 0;             // frames issued
        hipStream_t sideStream = nullptr; // sorts the costs of frame f while later frames render
        hipStream_t lastRenderStream = nullptr;
        bool haveLastRenderStream = false;
        // mode 200: scratch of the persistent path kernel (one region per RESIDENT workgroup + the launch's work counter); serial =
        // frames.serial.  A pool of the frames' own: frames and queries never share an arena
        Arena pathArena[kRing];
        unsigned long long* dTimeline = nullptr; // diagnostic: 3 words per workgroup, counting variant only
        size_t timelineWords = 0;
        // scratch frame buffers for the host-output path, grown on demand
        void* dFrame[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
        size_t dFrameBytes[5] = { 0, 0, 0, 0, 0 };
    } frames;

    // api_frames.cpp: progressive accumulation (crt_set_accumulation): mode-200 frames add their samples to per-pixel sums while the
    // key holds.  Everything a frame's samples depend on is in the key; spp, counting and the tuning options are not (results never
    // depend on them).  Floats are compared bitwise: a viewer that sets the same pose every tick keeps accumulating.
    struct AccKey {
        float pos[3], rot[9], miss[3];
        uint32_t mode, bounces, seed, sceneSerial, textureSerial, width, height, kind, rank, nRanks;
    };
    struct Acc {
        uint32_t max = 0;               // samples per pixel the sums may reach; 0 = off
        AccKey key{};                   // what the sums belong to (meaningful while accSamples > 0)
        void* dSums = nullptr;          // 4 doubles per output index of the RGBA8 store (pixel, or staging index of a tile share)
        size_t bytes = 0;
        // consecutive accumulating frames depend on each other through the sums: the next one waits (on the GPU) for the last one
        crtapi::Fence used;
    } acc;
    uint32_t accSamples = 0;            // samples per pixel in the sums (flat: the dynamic-geometry calls reset it, api_dynamic.cpp)

    // batched ray and point queries (crt_trace_rays* / crt_occluded_rays*, crt_closest_points* / crt_count_hits* /
    // crt_occupancy*): per arena the launch's cursor, counters and the stack spill arena of the persistent query kernel.  Arenas
    // of this pool belong to queries alone (never to a frame of runRender; a mode-150 or mode-120 frame is a query); serial = ++raySerial.
    // (Flat: the a-trous filter of api_image.cpp takes its planes from this pool too)
    Arena rayArena[kRing];
    uint32_t raySerial = 0;
    void* dRayStage = nullptr; // the host entry points' records and outputs, grown on demand
    size_t rayStageBytes = 0;

    // api_queries.cpp
    struct Queries {
        uint32_t resident[crt::kQueryKinds] = {};        // resident workgroups of each query kernel on this device ...
        uint32_t residentEntries[crt::kQueryKinds] = {}; // ... for this many LDS stack entries
        // crt_list_hits*: the host form's record arrays (grown on demand, apart from dRayStage, which holds its rays and offsets
        // while the total is read back)
        void* dListStage = nullptr;
        size_t listStageBytes = 0;
        hipEvent_t evList[5] = {};    // a listing with stats: before the count, after count / scan / fill / sort
        double listPhaseMs[4] = {};   // count, scan, fill, sort + resolve of the last listing that was given stats (crt_debug_list_phases)
    } queries;

    // api_dynamic.cpp, crt_trace_rays_backward* / crt_closest_points_backward*: the float64 vertex sums of a dynamic scene, 3 doubles
    // per vertex.  Allocated by the first call that wants vertex gradients, freed with the scene (freeScene); calls share it in
    // stream order
    struct Grad {
        double* dSum = nullptr;
        crtapi::Fence used; // the last call that used the sums, on the stream it ran on
    } grad;

    // api_comm.cpp: native multi-GPU frame assembly (crt_comm_init): RCCL communicator + per-ring-slot staging / gathered / frame buffers
    struct DistSlot {
        void* stage = nullptr;    // this rank's tiles
        void* gathered = nullptr; // every rank's
        void* frame = nullptr;    // the assembled frame of a call that gave no device buffer
        size_t stageBytes = 0, gatheredBytes = 0, frameBytes = 0;
        crtapi::Fence done;       // end of the frame that last used the three, on the stream it ran on
    };
    struct Dist {
        ncclComm_t comm = nullptr;
        struct HostExchange* hostComm = nullptr; // crt_comm_init_host: the tiles travel through shared host memory instead of RCCL
        uint32_t rank = 0, ranks = 0;
        DistSlot slot[kRing];
        uint32_t serial = 0;
    } dist;
};

namespace crtapi {

// What a query kernel gets from its arena: grid, chunking, cursor, counters and the stack spill arena
struct QueryLaunch {
    uint32_t stack_entries, spill_stride, chunk, grid;
    uint32_t* cursor;
    unsigned long long* counters;
    int* spill;
    unsigned char* extra; // extraBytes of the arena behind the spill area (256-byte aligned), or null
    crt_ctx::Arena* arena;
};

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

// sets the context's error string (ctx == NULL: the thread's create error, crt_last_error(NULL)) and returns `code`
int fail(crt_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return crtapi::fail((ctx), CRT_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

inline size_t up256(size_t b) { return (b + 255u) & ~static_cast<size_t>(255u); }

void stampTotal(crt_frame_stats* stats, std::chrono::steady_clock::time_point t0);
int readStats(crt_ctx* c, crt_frame_stats* stats, const unsigned long long* dCounters = nullptr, unsigned long long* words = nullptr);

int stageBegin(crt_ctx* c, const StagePlane* planes, int n, void** dev);
int stageDownload(crt_ctx* c, const StagePlane* planes, int n, void* const* dev);
int stageEnd(crt_ctx* c, const StagePlane* planes, int n, void* const* dev);

// the scene and its tree (crt_api.cpp; dropOrders and refuseWhitted: api_frames.cpp)
void freeScene(crt_ctx* c);
void dropOrders(crt_ctx* c);
int refuseWhitted(crt_ctx* c, const char* what);
int readSceneBox(crt_ctx* c);
void adoptTree(crt_ctx* c, crt::DeviceTree&& t);
int reserveRefitCapacity(crt_ctx* c);
int applyRefit(crt_ctx* c, double* device_ms);
int checkRenderable(crt_ctx* c, uint32_t w, uint32_t h);

// buffers, arenas, stats and argument checks (crt_api.cpp)
int ensureBuffer(crt_ctx* c, void** ptr, size_t* have, size_t need, bool ownScratch = false);
int takeArena(crt_ctx* c, crt_ctx::Arena (&pool)[crt_ctx::kRing], size_t need, uint32_t serial, bool ownScratch, crt_ctx::Arena*& out);
int reserveRayStage(crt_ctx* c, size_t total);
void zeroStats(crt_frame_stats* stats, std::chrono::steady_clock::time_point t0);
int runTimed(crt_ctx* c, const char* what, crt_frame_stats* stats, const std::function<int()>& launch);
int checkFrameSize(crt_ctx* c, const char* what, uint32_t w, uint32_t h);
int checkDevicePointers(crt_ctx* c, const char* what, std::initializer_list<const void*> ptrs, uintptr_t align);
// api_queries.cpp
void shadeTables(const crt_ctx* c, crt::ShadeQueryParams& q);
bool whittedMode(const crt_ctx* c);
bool ambientMode(const crt_ctx* c);
struct ShadedFrame { // a frame in mode 150 or 120: a query over its camera rays
    uint32_t width, height;
    uint32_t* rgba8;
};
int runShaded(crt_ctx* c, crt::QueryKind kind, uint32_t n, const void* d_records, void* const d[7], const ShadedFrame* frame,
              crt_frame_stats* stats);
int beginQuery(crt_ctx* c, crt::QueryKind kind, uint32_t n, crt_frame_stats* stats, QueryLaunch& ql, size_t extraBytes = 0,
               uint32_t minGrid = 0);
int endQuery(crt_ctx* c, crt::QueryKind kind, uint32_t n, const QueryLaunch& ql, int rc, crt_frame_stats* stats);
crt::QueryCommon queryCommon(const crt_ctx* c, const QueryLaunch& ql, const void* d_records, uint32_t n, uint32_t inner_min);
// api_image.cpp
crt::CameraRayParams cameraRayParams(const crt_ctx* c, uint32_t w, uint32_t h, uint32_t sample, void* d_rays);

} // namespace crtapi
