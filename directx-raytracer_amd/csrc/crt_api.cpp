// C ABI of libcrt_hip.so (include/crt_hip.h), core unit: the renderer context, its streams and options, scene upload and
// adoption of a tree, the tree's exports, and the definitions of the helpers every unit of the layer shares (crt_ctx.h, which
// also maps the other units).  Each entry point cites the reference member it replaces in the header.  No CPU fallback exists
// here: every render path ends in launchRender() (render_kernels.hip; mode 200: path_kernels.hip).
#include "crt_ctx.h"

#include "bvh_wide.h"
#include "mem_util.h"

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <utility>
#include <vector>

using namespace crtapi;

// Diagnostics that change what a frame does or costs ("timeline", "debug_skip_units", "debug_force_measure") exist only in
// the diagnostic builds (tools/diag_build.sh, tools/prof_build.sh: -DCRT_DIAG=1); the product rejects the option names.
#ifndef CRT_DIAG
#ifdef CRT_PROF
#define CRT_DIAG 1
#else
#define CRT_DIAG 0
#endif
#endif

namespace {

thread_local std::string g_createError;

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

} // namespace

namespace crtapi {

// A device buffer of at least `need` bytes; one that grows keeps nothing of its contents.  Work in flight on any stream may still
// use the old buffer, hence the device-wide wait.  ownScratch: the buffer is scratch the call keeps for itself; an allocation
// failure is then CRT_ENOMEM (no HIP error left behind), and the caller words the message
int ensureBuffer(crt_ctx* c, void** ptr, size_t* have, size_t need, bool ownScratch)
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

void freeScene(crt_ctx* c)
{
    void** ptrs[] = { &c->dNodes, &c->dPlanes, &c->dMoments, &c->dBinNodes, &c->dWideNodes, &c->dTris, &c->dShade, &c->dLights, &c->dMats, &c->dUvs };
    for (void** p : ptrs) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    c->momentsNodes = 0;
    if (c->grad.dSum) (void)hipFree(c->grad.dSum);
    c->grad.dSum = nullptr;
    delete c->dyn;
    c->dyn = nullptr;
    c->haveScene = false;
}

// the root record as it sits in HBM: where split rays are cut into segments; and the union of the two child boxes of the
// binary tree's node 0, from where crt_bvh_export reads it (the quantised root's far planes are rounded outwards)
int readSceneBox(crt_ctx* c)
{
    for (int a = 0; a < 3; a++) c->sceneLo[a] = c->sceneHi[a] = c->binLo[a] = c->binHi[a] = 0.0f;
    if (c->bvh.dev.nNodes > 0 && (c->dBinNodes || !c->bvh.nodes.empty())) {
        crt_bvh_node root;
        if (c->dBinNodes) HIP_TRY(c, hipMemcpy(&root, c->dBinNodes, sizeof(root), hipMemcpyDeviceToHost));
        else root = c->bvh.nodes[0];
        const float lo[3][2] = { { root.lx0, root.rx0 }, { root.ly0, root.ry0 }, { root.lz0, root.rz0 } };
        const float hi[3][2] = { { root.lx1, root.rx1 }, { root.ly1, root.ry1 }, { root.lz1, root.rz1 } };
        for (int a = 0; a < 3; a++) {
            c->binLo[a] = std::fmin(lo[a][0], lo[a][1]);
            c->binHi[a] = std::fmax(hi[a][0], hi[a][1]);
        }
    }
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

void stampTotal(crt_frame_stats* stats, std::chrono::steady_clock::time_point t0)
{
    if (stats) stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

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
void adoptTree(crt_ctx* c, crt::DeviceTree&& t)
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
int reserveRefitCapacity(crt_ctx* c)
{
    const uint32_t cap = c->bvh.dev.nNodes ? c->bvh.dev.nNodes : 1u, n4 = c->bvh.dev.nNodes4;
    if (int rc = regrow(c, c->dWideNodes, sizeof(crt_bvh_node4) * n4, sizeof(crt_bvh_node4) * cap)) return rc;
    if (int rc = regrow(c, c->dNodes, sizeof(crt_bvh_node4q) * n4, crt::quantisedBytes(cap))) return rc;
    return regrow(c, c->dPlanes, c->dPlanes ? sizeof(float) * crt::kPlaneStride * n4 : 0, sizeof(float) * crt::kPlaneStride * cap);
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

// What a call with stats reports after its launch: waits for the stream, then kernel_ms = evStart .. evStop and every count zero.
// A launch that counts gives dCounters and four words: with counting on its four counter words are read into them (else zeros),
// of which the fetches mean the same for every kind of call; the ray counts are the caller's to fill in
int readStats(crt_ctx* c, crt_frame_stats* stats, const unsigned long long* dCounters, unsigned long long* words)
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

int checkRenderable(crt_ctx* c, uint32_t w, uint32_t h)
{
    if (!c) return CRT_EINVAL;
    if (!c->haveScene) return fail(c, CRT_ESTATE, "no scene uploaded: call crt_upload_scene first");
    if (w == 0 || h == 0 || w > 65536 || h > 65536) return fail(c, CRT_EINVAL, "bad frame size %ux%u", w, h);
    return applyRefit(c, nullptr);
}

} // namespace crtapi

namespace {

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
    // mode 120 runs outside the frame ring and the accumulation: nothing of theirs follows these
    { "ao_samples", within<1, 4096>, U32(aoSamples) },
    { "ao_radius", within<0, 1000000>, U32(aoRadiusPermille) },
    { "ao_sky", oneOf<0, 1>, U32(aoSky) },
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

uint32_t crt_abi_version(void) { return CRT_ABI_VERSION; }

namespace {
// the 1-workgroup sort that orders a later frame runs beside the next frame's render kernel: highest priority, so it is
// dispatched at once instead of queueing behind 32 640 render workgroups
hipError_t createSideStream(crt_ctx* c)
{
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess) return e;
    return hipStreamCreateWithPriority(&c->frames.sideStream, hipStreamNonBlocking, greatest);
}
// the frame slots' events up front: without them crt_create fails, not the first frame
hipError_t createRingEvents(crt_ctx* c)
{
    for (crt_ctx::FrameSlot& s : c->frames.slot)
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
        if (c->frames.dFrame[i]) (void)hipFree(c->frames.dFrame[i]);
    (void)crt_comm_destroy(c);
    if (c->frames.sideStream) (void)hipStreamSynchronize(c->frames.sideStream);
    for (int i = 0; i < crt_ctx::kRing; i++) {
        crt_ctx::FrameSlot& s = c->frames.slot[i];
        crt_ctx::DistSlot& d = c->dist.slot[i];
        for (void* p : std::initializer_list<void*>{ s.spill, s.unitCost, s.unitOrder, d.stage, d.gathered, d.frame, c->frames.pathArena[i].mem, c->rayArena[i].mem })
            if (p) (void)hipFree(p);
        for (Fence* f : { &s.rendered, &s.sorted, &d.done, &c->frames.pathArena[i].lastUse, &c->rayArena[i].lastUse }) f->destroy();
    }
    if (c->dCounters) (void)hipFree(c->dCounters);
    if (c->dTextures) (void)hipFree(c->dTextures);
    if (c->dTexels) (void)hipFree(c->dTexels);
    if (c->frames.sideStream) (void)hipStreamDestroy(c->frames.sideStream);
    if (c->frames.dTimeline) (void)hipFree(c->frames.dTimeline);
    if (c->acc.dSums) (void)hipFree(c->acc.dSums);
    c->acc.used.destroy();
    c->grad.used.destroy();
    if (c->dRayStage) (void)hipFree(c->dRayStage);
    if (c->queries.dListStage) (void)hipFree(c->queries.dListStage);
    for (hipEvent_t e : c->queries.evList)
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

int crt_debug_read_counters(crt_ctx* c, unsigned long long out[32])
{
    if (!c || !out) return CRT_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, c->dCounters, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
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

// ---- shared with the other units (crt_ctx.h)
namespace crtapi {

void zeroStats(crt_frame_stats* stats, std::chrono::steady_clock::time_point t0)
{
    if (!stats) return;
    std::memset(stats, 0, sizeof(*stats));
    stampTotal(stats, t0);
}

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

} // namespace crtapi
