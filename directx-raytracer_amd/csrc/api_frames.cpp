// C ABI, the per-frame host path (crt_ctx.h maps the units): from crt_render_frame* / crt_render_tiles* / the batch calls
// through runRender's named steps to launchRender() / launchPath(), with the launch-order feedback and progressive accumulation.
// Nothing on this path leaves the unit except the shared buffer and arena helpers.
#include "crt_ctx.h"

#include "mem_util.h"

#include <algorithm>
#include <chrono>
#include <cstring>

using crt::RenderParams;
using namespace crtapi;

namespace crtapi {

// forget the stored launch orders: the scene changed, or how orders are made or used did
void dropOrders(crt_ctx* c)
{
    for (crt_ctx::FrameSlot& s : c->frames.slot) s.orderKey = 0;
}

// the tile, batch and distributed entry points render shares of the render kernel's work: the Whitted and the ambient-occlusion
// query kinds (modes 150 and 120) have none.  Checked before anything else of the call (a NULL context is the caller's next check)
int refuseWhitted(crt_ctx* c, const char* what)
{
    if (!c || !(whittedMode(c) || ambientMode(c))) return CRT_OK;
    return fail(c, CRT_EINVAL, "%s: shading mode %u (%s) renders whole frames only (crt_render_frame*): set another mode", what, c->mode,
                whittedMode(c) ? "Whitted" : "ambient occlusion");
}

} // namespace crtapi

namespace {

int ensureFrame(crt_ctx* c, int slot, size_t bytes)
{
    if (c->frames.dFrameBytes[slot] >= bytes) return CRT_OK;
    if (c->frames.dFrame[slot]) (void)hipFree(c->frames.dFrame[slot]);
    c->frames.dFrame[slot] = nullptr;
    c->frames.dFrameBytes[slot] = 0;
    HIP_TRY(c, hipMalloc(&c->frames.dFrame[slot], bytes));
    c->frames.dFrameBytes[slot] = bytes;
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

// a frame that uses the sums runs after the last one that did, even when issued on another stream (crt_set_stream)
int orderAccum(crt_ctx* c)
{
    HIP_TRY(c, c->acc.used.wait(c->stream, false));
    return CRT_OK;
}

// after the launch: the sums now hold acc_total samples
int commitAccum(crt_ctx* c, const RenderParams& p)
{
    HIP_TRY(c, c->acc.used.record(c->stream));
    c->accSamples = p.acc_total;
    return CRT_OK;
}

// ---- One frame (runRender), step by step.  Each step enqueues on the context's stream only what its comment says.

// diagnostic builds, option "timeline": 3 words per workgroup, zeroed before the frame
int frameTimeline(crt_ctx* c, RenderParams& p)
{
    if (!c->wantTimeline || p.n_batch != 1) return CRT_OK;
    const size_t words = 3 * (static_cast<size_t>(p.tiles_x + 4) * (p.tiles_y + 4) * 4 + 1024);
    if (c->frames.timelineWords < words) {
        if (c->frames.dTimeline) (void)hipFree(c->frames.dTimeline);
        c->frames.dTimeline = nullptr;
        HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&c->frames.dTimeline), words * sizeof(unsigned long long)));
        c->frames.timelineWords = words;
    }
    HIP_TRY(c, hipMemsetAsync(c->frames.dTimeline, 0, c->frames.timelineWords * sizeof(unsigned long long), c->stream));
    p.timeline = c->frames.dTimeline;
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
    if (const int rc = takeArena(c, c->frames.pathArena, need, c->frames.serial, false, arena)) return rc;
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
    for (crt_ctx::FrameSlot& s : c->frames.slot) {
        if (s.unitCost) (void)hipFree(s.unitCost);
        if (s.unitOrder) (void)hipFree(s.unitOrder);
        s.unitCost = s.unitOrder = nullptr;
        s.sorted.pending = false;
    }
    dropOrders(c);
    c->frames.unitCapacity = 0;
    for (crt_ctx::FrameSlot& s : c->frames.slot) {
        HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&s.unitCost), sizeof(uint32_t) * nUnits));
        HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&s.unitOrder), sizeof(uint32_t) * nUnits));
    }
    c->frames.unitCapacity = nUnits;
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
    const bool sameStream = c->frames.haveLastRenderStream && c->frames.lastRenderStream == c->stream;
    c->frames.lastRenderStream = c->stream;
    c->frames.haveLastRenderStream = true;
    if (!(c->adaptiveOrder == 1 || (c->adaptiveOrder == 2 && sameStream)) || !lo.nUnits || p.mode >= 200u) return CRT_OK; // (the path pipeline has its own work split)
    if (c->frames.unitCapacity < lo.nUnits)
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
    const bool recent = (c->frames.serial - slot.orderFrame) < static_cast<uint32_t>(crt_ctx::kRing) * c->tuneRemeasureEvery;
    if (c->debugForceMeasure || !(twice && (sameView || recent))) {
        p.unit_cost = slot.unitCost;
        lo.measure = true;
        slot.orderGen = usable ? slot.orderGen + 1 : 1;
        slot.orderView = c->viewSerial;
        slot.orderFrame = c->frames.serial;
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
    hipStream_t ss = c->frames.sideStream;
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
    crt_ctx::FrameSlot& slot = c->frames.slot[c->frames.serial++ % crt_ctx::kRing];
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
    if (c->acc.max == 0u || p.mode < 200u) return CRT_OK;
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
    if (c->accSamples == 0u || std::memcmp(&k, &c->acc.key, sizeof(k)) != 0) {
        c->accSamples = 0u;
        c->acc.key = k;
    }
    const size_t outputs = kind == kAccTiles ? static_cast<size_t>(crt_tile_slots(p.width, p.height, p.n_ranks)) * crt::kTile * crt::kTile
                                             : static_cast<size_t>(p.width) * p.height;
    const size_t need = outputs * 4u * sizeof(double); // float64 sums {x, y}, {z, 0} (path_kernels.hip loadSum)
    if (c->acc.bytes < need) { // (a larger frame: the key has changed, nothing in the old sums is kept)
        HIP_TRY(c, hipSetDevice(c->device));
        if (const int rc = ensureBuffer(c, &c->acc.dSums, &c->acc.bytes, need)) return rc;
    }
    const uint32_t traced = std::min(p.spp, c->acc.max - c->accSamples);
    p.acc_sum = c->acc.dSums;
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

// A frame in mode 150 (CRT_MODE_WHITTED) or 120 (CRT_MODE_AMBIENT) is a query, not a launch of the render kernel: the
// pixel-centre camera rays, the mode's query kind over them and the quantisation of its float colour (runShaded,
// api_queries.cpp), on the stream's query arena.  Nothing of runRender runs: the frame ring, the launch orders and their cost
// state stay as they are.
int runQueryFrame(crt_ctx* c, const RenderParams& p, crt_frame_stats* stats)
{
    const bool whitted = p.mode == CRT_MODE_WHITTED;
    const char* what = whitted ? "a frame in shading mode 150" : "a frame in shading mode 120";
    if (const int rc = checkFrameSize(c, what, p.width, p.height)) return rc; // (the camera-ray kernel's limit)
    void* const out[7] = { p.rgb_f32, nullptr, nullptr, p.hit_t, nullptr, p.hit_inst, p.hit_prim };
    const ShadedFrame frame = { p.width, p.height, p.rgba8 };
    return runShaded(c, whitted ? crt::kQueryWhitted : crt::kQueryAmbient, p.width * p.height, nullptr, out, &frame, stats);
}

// one frame of an entry point that accumulates (kind: kAccFrame / kAccTiles)
int runFrame(crt_ctx* c, RenderParams& p, crt_frame_stats* stats, uint32_t kind)
{
    if (p.mode == CRT_MODE_WHITTED || p.mode == CRT_MODE_AMBIENT) return runQueryFrame(c, p, stats);
    const int rc = beginAccum(c, p, kind);
    if (rc) return rc;
    return p.acc_sum && p.spp == 0u ? runAccumResolve(c, p, stats) : runRender(c, p, stats);
}

} // namespace

int crt_set_accumulation(crt_ctx* c, uint32_t max_samples)
{
    if (!c) return CRT_EINVAL;
    if (max_samples > (1u << 24)) return fail(c, CRT_EINVAL, "crt_set_accumulation: max_samples %u above 2^24", max_samples);
    c->acc.max = max_samples;
    c->accSamples = 0u;
    if (max_samples == 0u && c->acc.dSums) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipDeviceSynchronize()); // frames in flight may still use the sums
        (void)hipFree(c->acc.dSums);
        c->acc.dSums = nullptr;
        c->acc.bytes = 0;
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
    *samples = c->acc.max ? c->accSamples : 0u;
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
    p.rgba8 = static_cast<uint32_t*>(c->frames.dFrame[0]);
    p.hit_inst = host[1] ? static_cast<uint32_t*>(c->frames.dFrame[1]) : nullptr;
    p.hit_prim = host[2] ? static_cast<uint32_t*>(c->frames.dFrame[2]) : nullptr;
    p.hit_t = host[3] ? static_cast<float*>(c->frames.dFrame[3]) : nullptr;
    p.rgb_f32 = host[4] ? static_cast<float*>(c->frames.dFrame[4]) : nullptr;
    crt_frame_stats local;
    rc = runFrame(c, p, stats ? stats : &local, kAccFrame); // synchronous like the reference's renderFrame
    if (rc) return rc;
    const bool traced = !(p.acc_sum && p.spp == 0u); // a frame at the accumulation limit writes no hit outputs
    for (int i = 0; i < 5; i++)
        if (host[i] && (traced || i == 0 || i == 4)) HIP_TRY(c, hipMemcpyAsync(host[i], c->frames.dFrame[i], bytes[i], hipMemcpyDeviceToHost, c->stream));
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
    int rc = refuseWhitted(c, "crt_render_tiles_device");
    if (rc == CRT_OK) rc = checkRenderable(c, w, h);
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
    int rc = refuseWhitted(c, staging ? "crt_render_tiles_batch_device" : "crt_render_frames_batch_device");
    if (rc == CRT_OK) rc = checkRenderable(c, w, h);
    if (rc) return rc;
    if (n_frames == 0 || n_frames > static_cast<uint32_t>(crt::kMaxBatch)) return fail(c, CRT_EINVAL, "n_frames %u outside [1,%d]", n_frames, crt::kMaxBatch);
    if (!d_out || n_ranks == 0 || rank >= n_ranks) return fail(c, CRT_EINVAL, "bad batch arguments (rank %u of %u)", rank, n_ranks);
    for (uint32_t f = 0; f < n_frames; f++)
        if (!d_out[f]) return fail(c, CRT_EINVAL, "output pointer of frame %u is NULL", f);
    if (c->acc.max != 0u && c->mode >= 200u)
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

int crt_debug_read_timeline(crt_ctx* c, unsigned long long* out, size_t max_words, size_t* n_words)
{
    if (!c || !out || !n_words) return CRT_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = c->frames.timelineWords < max_words ? c->frames.timelineWords : max_words;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n) HIP_TRY(c, hipMemcpy(out, c->frames.dTimeline, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    *n_words = n;
    return CRT_OK;
}
