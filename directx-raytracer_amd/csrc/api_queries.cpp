// C ABI, batched queries (crt_ctx.h maps the units): ray, point, shaded (modes 120 and 150 among them), winding, path-traced and all-hits listing queries,
// each entry point next to the run path it calls.
#include "crt_ctx.h"

#include "mem_util.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

using namespace crtapi;

namespace {

// the scene's shading tables as the shaded, the path-traced, the Whitted and the ambient-occlusion query take them
// (crt::ShadeQueryParams, crt::PathQueryParams, crt::WhittedQueryParams, crt::AmbientQueryParams)
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
    crt::WhittedQueryParams whitted;
    crt::AmbientQueryParams ambient;
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

// the specular term of mode 100's light sum, from the options
template <class Q> void phongState(const crt_ctx* c, Q& q)
{
    q.phong_ks = static_cast<float>(c->phongKsPermille) / 1000.0f;
    q.phong_exp = c->phongExp;
}
// the outputs of crt_shade_rays* from the device pointers d[0..6]
crt::ShadedOutputs shadedOutputs(void* const d[kQueryOutputs])
{
    static_assert(kQueryOutputs == 7, "the outputs of crt_shade_rays*");
    return { static_cast<float*>(d[0]), static_cast<float*>(d[1]), static_cast<float*>(d[2]), static_cast<float*>(d[3]),
             static_cast<float*>(d[4]), static_cast<uint32_t*>(d[5]), static_cast<uint32_t*>(d[6]) };
}
// the same outputs from record r0 on (a NULL stays NULL)
crt::ShadedOutputs offsetOutputs(const crt::ShadedOutputs& o, uint64_t r0)
{
    const auto at = [r0](auto* p, uint32_t per) { return p ? p + per * r0 : nullptr; };
    return { at(o.rgb, 3u), at(o.normal, 3u), at(o.albedo, 3u), at(o.t, 1u), at(o.uv, 2u), at(o.inst, 1u), at(o.prim, 1u) };
}

} // namespace

// the scene's shading tables (sceneTables) and the context's shading state of a shaded query
void crtapi::shadeTables(const crt_ctx* c, crt::ShadeQueryParams& q)
{
    sceneTables(c, q);
    q.mode = c->mode;
    phongState(c, q);
}

// crt_shade_rays* and the frames in mode 150: whether the context's mode asks for the Whitted kind (101..149 and 151..199 are mode 100)
bool crtapi::whittedMode(const crt_ctx* c) { return c->mode == CRT_MODE_WHITTED; }
// the same for mode 120 and the ambient-occlusion kind
bool crtapi::ambientMode(const crt_ctx* c) { return c->mode == CRT_MODE_AMBIENT; }

namespace {

// the kinds of crt_shade_rays*: the context's mode is checked, and the refit follows the argument checks
bool shadedKind(QueryKind kind) { return kind == crt::kQueryShade || kind == crt::kQueryWhitted || kind == crt::kQueryAmbient; }
// the kind crt_shade_rays* runs in the context's mode
QueryKind shadedKindOf(const crt_ctx* c)
{
    if (c && whittedMode(c)) return crt::kQueryWhitted;
    return c && ambientMode(c) ? crt::kQueryAmbient : crt::kQueryShade;
}

// The reach of mode 120's occlusion rays (include/crt_hip.h "ambient occlusion"): option "ao_radius" in thousandths of the
// diagonal of the root box as crt_bvh_export reports it (readSceneBox), every operation rounded to float32 on its own
// (-ffp-contract=off); 0 = the interval of a mode-200 bounce ray
float ambientRadius(const crt_ctx* c)
{
    if (c->aoRadiusPermille == 0u) return 10000.0f; // traversal.hip.h kTMax
    const float dx = c->binHi[0] - c->binLo[0], dy = c->binHi[1] - c->binLo[1], dz = c->binHi[2] - c->binLo[2];
    const float D = std::sqrt((dx * dx + dy * dy) + dz * dz);
    return (static_cast<float>(c->aoRadiusPermille) / 1000.0f) * D;
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
    p.shade.out = shadedOutputs(d);
    shadeTables(c, p.shade);
    innerMin = c->tuneInnerMin;
    return CRT_OK;
}
// crt_shade_rays* in mode 150 (whitted_kernels.hip): the outputs of fillShade; the record state comes from the launch's arena (runShaded)
int fillWhitted(crt_ctx* c, const QuerySpec&, void* const d[kQueryOutputs], QueryParams& p, uint32_t& innerMin)
{
    crt::WhittedQueryParams& q = p.whitted;
    q.out = shadedOutputs(d);
    sceneTables(c, q);
    q.max_bounces = c->pathBounces;
    phongState(c, q);
    innerMin = c->tuneInnerMin;
    return CRT_OK;
}
// crt_shade_rays* and the frames in mode 120 (ao_kernels.hip): the outputs of fillShade
int fillAmbient(crt_ctx* c, const QuerySpec&, void* const d[kQueryOutputs], QueryParams& p, uint32_t& innerMin)
{
    crt::AmbientQueryParams& q = p.ambient;
    q.out = shadedOutputs(d);
    sceneTables(c, q);
    phongState(c, q);
    q.samples = c->aoSamples;
    q.radius = ambientRadius(c);
    q.sky = c->aoSky;
    q.seed = c->pathSeed;
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
    /* kQueryWhitted */
    { 32u, "rgb / normal / albedo / t / uv / inst / prim", { { 12u, 4u }, { 12u, 4u }, { 12u, 4u }, { 4u, 4u }, { 8u, 8u }, { 4u, 4u }, { 4u, 4u } }, fillWhitted },
    /* kQueryAmbient */
    { 32u, "rgb / normal / albedo / t / uv / inst / prim", { { 12u, 4u }, { 12u, 4u }, { 12u, 4u }, { 4u, 4u }, { 8u, 8u }, { 4u, 4u }, { 4u, 4u } }, fillAmbient },
};

// what every query entry point checks before anything is launched.  A shaded query (crt_shade_rays*) promises that a failed
// call launches nothing: its refit follows its argument checks (queryDevice / queryHost) instead of coming here
int checkQuery(crt_ctx* c, const QuerySpec& s)
{
    const char* what = s.what;
    if (!c) return fail(nullptr, CRT_EINVAL, "%s: NULL context", what);
    if (!c->haveScene) return fail(c, CRT_ESTATE, "%s: no scene uploaded: call crt_upload_scene first", what);
    if (shadedKind(s.kind)) {
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
    if (c->queries.resident[kind] == 0u || c->queries.residentEntries[kind] != stack_entries) {
        c->queries.resident[kind] = crt::queryResident(kind, stack_entries);
        c->queries.residentEntries[kind] = stack_entries;
        if (c->queries.resident[kind] == 0u) return fail(c, CRT_EHIP, "query kernel: occupancy query failed");
    }
    crt::queryLayout(n, c->queries.resident[kind], chunk, grid);
    return CRT_OK;
}

} // namespace

// One query of n > 0 records on the context's stream, in two halves around the kernel launch.  beginQuery sizes the persistent
// grid, takes an arena and (with stats) starts the timer.  endQuery takes the launch's HIP error code and, with stats,
// synchronises and fills them.
// extraBytes: scratch of the query's own with the arena's lifetime (an allocation failure is then CRT_ENOMEM); minGrid: the
// spill area is sized for at least that many workgroups (a query that runs a second persistent kernel over the same arena).
int crtapi::beginQuery(crt_ctx* c, QueryKind kind, uint32_t n, crt_frame_stats* stats, QueryLaunch& ql, size_t extraBytes, uint32_t minGrid)
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

int crtapi::endQuery(crt_ctx* c, QueryKind kind, uint32_t n, const QueryLaunch& ql, int rc, crt_frame_stats* stats)
{
    if (rc != 0) return fail(c, CRT_EHIP, "query kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
    if (stats) HIP_TRY(c, hipEventRecord(c->evStop, c->stream));
    HIP_TRY(c, ql.arena->lastUse.record(c->stream));
    if (!stats) return CRT_OK;
    unsigned long long words[4]; // (zeros unless counting is on)
    if (const int rs = readStats(c, stats, ql.counters, words)) return rs;
    if (kind == crt::kQueryOcclusion) stats->rays_shadow = n;
    else stats->rays_primary = kind == crt::kQueryOccupancy ? 3ull * n : n;
    if (c->counting && (shadedKind(kind) || kind == crt::kQueryPath)) stats->rays_shadow = words[2];   // the shadow rays traced (modes 100, 120 with its occlusion rays, 150; paths)
    if (kind == crt::kQueryPath || kind == crt::kQueryWhitted) stats->rays_primary += words[3];        // the bounce rays of the paths, the turns of mode 150
    return CRT_OK;
}

// the part of a query kernel's parameters every kind shares, from the context and the launch
crt::QueryCommon crtapi::queryCommon(const crt_ctx* c, const QueryLaunch& ql, const void* d_records, uint32_t n, uint32_t inner_min)
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

// A query of the Whitted or the ambient-occlusion kind of n records into the outputs d (shadedOutputs' order), over one arena
// between one beginQuery and one endQuery.
// The Whitted kind keeps the records' state (kWhittedStateBytes each) in the arena, so a launch covers at most "path_pass_paths"
// records, as a pass of crt_path_rays* does; a larger buffer runs as several launches over blocks of records.  (The ambient
// kind keeps none: crt_shade_rays* in mode 120 goes through runKind as any other kind, and only its frames come here.)
// frame (crt_render_frame* in modes 150 and 120): d_records is NULL and the records are the frame's pixel-centre camera rays,
// made in the arena by the camera-ray kernel, all in one launch; behind the query the float colour (d[0], or scratch of the
// arena when the caller wants none) is quantised into frame->rgba8.  The other frame outputs are the query's own, bit for bit:
// hit_t is t (on a miss the record's tmax, which is the frames' 10000), hit_inst / hit_prim are inst / prim.
int crtapi::runShaded(crt_ctx* c, QueryKind kind, uint32_t n, const void* d_records, void* const d[7], const ShadedFrame* frame,
                      crt_frame_stats* stats)
{
    const bool whitted = kind == crt::kQueryWhitted;
    QueryParams p;
    std::memset(&p, 0, sizeof(p));
    uint32_t innerMin = 0;
    if (const int rc = kQueryShapes[kind].fill(c, QuerySpec{}, d, p, innerMin)) return rc;
    crt::ShadedOutputs& out = whitted ? p.whitted.out : p.ambient.out;
    const uint32_t block = frame ? n : std::min(n, c->tunePathPassPaths);
    const size_t stateBytes = whitted ? up256(static_cast<size_t>(block) * crt::kWhittedStateBytes) : 0u;
    const size_t rayBytes = frame ? up256(static_cast<size_t>(n) * 32u) : 0u, rgbBytes = frame && !out.rgb ? up256(static_cast<size_t>(n) * 12u) : 0u;
    QueryLaunch ql;
    if (const int rc = beginQuery(c, kind, block, stats, ql, stateBytes + rayBytes + rgbBytes)) return rc;
    if (whitted) p.whitted.state = ql.extra;
    int hrc = 0;
    if (frame) {
        d_records = ql.extra + stateBytes;
        if (!out.rgb) out.rgb = reinterpret_cast<float*>(ql.extra + stateBytes + rayBytes);
        hrc = crt::launchCameraRays(cameraRayParams(c, frame->width, frame->height, CRT_SAMPLE_CENTRE, ql.extra + stateBytes), c->stream);
    }
    const crt::ShadedOutputs all = out; // the outputs of record 0
    for (uint64_t r0 = 0; r0 < n && hrc == 0; r0 += block) {
        const uint32_t nr = static_cast<uint32_t>(std::min<uint64_t>(block, n - r0));
        if (r0 != 0u) HIP_TRY(c, hipMemsetAsync(ql.cursor, 0, sizeof(uint32_t), c->stream)); // (the counters go on counting)
        uint32_t chunk = 0, grid = 0;
        crt::queryLayout(nr, c->queries.resident[kind], chunk, grid);
        grid = std::min(grid, ql.grid); // (the spill area is sized for ql.grid workgroups, the largest block's)
        p.c = queryCommon(c, ql, static_cast<const unsigned char*>(d_records) + 32u * r0, nr, innerMin);
        p.c.chunk = chunk;
        out = offsetOutputs(all, r0);
        hrc = crt::launchQuery(kind, &p, c->counting, grid, c->stream);
    }
    if (frame && hrc == 0) hrc = crt::launchRgbToRgba8(all.rgb, frame->rgba8, n, c->stream);
    return endQuery(c, kind, n, ql, hrc, stats);
}

namespace {

// a query of any kind with an entry point: its fill, then one launch between beginQuery and endQuery
int runKind(crt_ctx* c, const QuerySpec& s, uint32_t n, const void* d_records, void* const d[kQueryOutputs], crt_frame_stats* stats)
{
    if (s.kind == crt::kQueryWhitted) return runShaded(c, s.kind, n, d_records, d, nullptr, stats);
    QueryParams p;
    std::memset(&p, 0, sizeof(p));
    uint32_t innerMin = 0;
    if (const int rc = kQueryShapes[s.kind].fill(c, s, d, p, innerMin)) return rc;
    QueryLaunch ql;
    if (const int rc = beginQuery(c, s.kind, n, stats, ql)) return rc;
    p.c = queryCommon(c, ql, d_records, n, innerMin);
    return endQuery(c, s.kind, n, ql, crt::launchQuery(s.kind, &p, c->counting, ql.grid, c->stream), stats);
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
    if (shadedKind(s.kind) && (rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
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
    if (shadedKind(s.kind) && (rc = applyRefit(c, nullptr)) != CRT_OK) return rc;
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
            crt::queryLayout(items, c->queries.resident[crt::kQueryPath], chunk, grid);
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
    return lr.timed ? static_cast<int>(hipEventRecord(c->queries.evList[i], c->stream)) : 0;
}

// count + scan.  keyBytes: scratch wanted behind the counts and the tile sums (device form: work arrays the caller did not supply)
int listBegin(crt_ctx* c, uint32_t n, const void* d_rays, void* d_offsets, size_t keyBytes, crt_frame_stats* stats, ListRun& lr)
{
    HIP_TRY(c, hipSetDevice(c->device));
    uint32_t entries = 0;
    if (const int rc = queryGrid(c, crt::kQueryListFill, n, entries, lr.fillChunk, lr.fillGrid)) return rc;
    lr.timed = stats != nullptr;
    if (lr.timed)
        for (hipEvent_t& e : c->queries.evList)
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
        if (i < 2 || filled) HIP_TRY(c, hipEventElapsedTime(&ms, c->queries.evList[i], c->queries.evList[i + 1]));
        c->queries.listPhaseMs[i] = ms;
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
    return queryDevice(c, { "crt_shade_rays_device", shadedKindOf(c), { d_rgb, d_normal, d_albedo, d_t, d_uv, d_inst, d_prim } }, n, d_rays, stats);
}

int crt_shade_rays(crt_ctx* c, uint32_t n, const float* rays, float* rgb, float* normal, float* albedo, float* t, float* uv, uint32_t* inst,
                   uint32_t* prim, crt_frame_stats* stats)
{
    return queryHost(c, { "crt_shade_rays", shadedKindOf(c), { rgb, normal, albedo, t, uv, inst, prim } }, n, rays, stats);
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
        const int grown = ensureBuffer(c, &c->queries.dListStage, &c->queries.listStageBytes, 3u * cap4 + cap8, true);
        if (grown == CRT_EHIP) return grown; // (the device-wide wait failed: endQuery would only return the same)
        noMem = grown == CRT_ENOMEM;
        rec = static_cast<unsigned char*>(c->queries.dListStage);
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

int crt_debug_list_phases(crt_ctx* c, double out_ms[4])
{
    if (!c || !out_ms) return CRT_EINVAL;
    std::memcpy(out_ms, c->queries.listPhaseMs, sizeof(c->queries.listPhaseMs));
    return CRT_OK;
}
