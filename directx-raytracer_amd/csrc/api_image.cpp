// C ABI, image space (crt_ctx.h maps the units): camera rays, frame guides, the a-trous filters, temporal reprojection and
// variance.
#include "crt_ctx.h"

#include "mem_util.h"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cstring>

using namespace crtapi;

// ---- camera rays, frame guides and the denoiser (camera_kernels.hip, denoise_kernels.hip)
crt::CameraRayParams crtapi::cameraRayParams(const crt_ctx* c, uint32_t w, uint32_t h, uint32_t sample, void* d_rays)
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

namespace {

int checkCameraRays(crt_ctx* c, const char* what, uint32_t w, uint32_t h, uint32_t sample, const void* rays)
{
    if (!c) return fail(nullptr, CRT_EINVAL, "%s: NULL context", what);
    if (const int rc = checkFrameSize(c, what, w, h)) return rc;
    if (sample != CRT_SAMPLE_CENTRE && sample >= (1u << 24)) return fail(c, CRT_EINVAL, "%s: sample %u is neither below 2^24 nor CRT_SAMPLE_CENTRE", what, sample);
    if (!rays) return fail(c, CRT_EINVAL, "%s: record buffer is NULL", what);
    return CRT_OK;
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
    q.out.normal = static_cast<float*>(d_normal);
    q.out.albedo = static_cast<float*>(d_albedo);
    q.out.t = static_cast<float*>(d_t);
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
