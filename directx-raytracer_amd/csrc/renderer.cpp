#include "renderer.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <thread>

namespace crt {

Renderer::Renderer() = default;

Renderer::~Renderer()
{
    if (ctx) crt_destroy(ctx);
}

void Renderer::check(int rc, const char* what) const
{
    if (rc != CRT_OK) throw std::runtime_error(std::string(what) + ": " + crt_last_error(ctx));
}

void Renderer::prepareForRendering(const std::string& sceneFile, int deviceId)
{
    prepareForRendering(std::make_unique<Scene>(sceneFile), deviceId);
}

void Renderer::prepareForRendering(std::unique_ptr<Scene> ownedScene, int deviceId)
{
    scene = std::move(ownedScene);
    if (!ctx) {
        const int rc = crt_create(&ctx, deviceId);
        if (rc != CRT_OK) throw std::runtime_error(std::string("crt_create: ") + crt_last_error(nullptr));
    }
    uploadScene();
    prepareForRayTracing();
}

void Renderer::prepareForRayTracing() {}

void Renderer::uploadScene()
{
    std::vector<crt_mesh_view> meshes;
    for (const Mesh& m : scene->getObjects()) {
        crt_mesh_view v{};
        v.xyz = m.getVertices().empty() ? nullptr : m.getVertices().data()->data();
        v.idx = reinterpret_cast<const uint32_t*>(m.getIndices().data());
        v.normals = (m.getVertexNormals().size() == m.getVertices().size() && !m.getVertices().empty())
                        ? m.getVertexNormals().data()->data() : nullptr;
        v.uvs = (m.getUV().size() == m.getVertices().size() && !m.getUV().empty()) ? m.getUV().data()->data() : nullptr;
        v.n_vertices = static_cast<uint32_t>(m.getVertices().size());
        v.n_triangles = static_cast<uint32_t>(m.getIndices().size() / 3);
        v.material_index = m.getMaterialIndex();
        meshes.push_back(v);
    }
    std::vector<crt_light> lights;
    for (const Light& l : scene->getLights())
        lights.push_back(crt_light{ { l.getPosition().getX(), l.getPosition().getY(), l.getPosition().getZ() }, l.getIntensity() });
    std::vector<crt_material> mats;
    for (const Material& m : scene->getMaterials())
        mats.push_back(crt_material{ { m.getAlbedo().getX(), m.getAlbedo().getY(), m.getAlbedo().getZ() },
                                     static_cast<uint32_t>(m.getType()), m.isSmoothShading() ? 1u : 0u, m.getIor(),
                                     m.isTexture() ? scene->textureIndexByName(m.getTextureName()) : -1 });
    check(crt_set_option(ctx, "dynamic", dynamicGeometry ? 1 : 0), "crt_set_option");
    check(crt_set_option(ctx, "gpu_build", gpuBuilder >= 0 ? 1 : 0), "crt_set_option");
    check(crt_set_option(ctx, "gpu_builder", gpuBuilder >= 0 ? gpuBuilder : 0), "crt_set_option");
    check(crt_upload_scene(ctx, meshes.data(), static_cast<uint32_t>(meshes.size()), lights.data(),
                           static_cast<uint32_t>(lights.size()), mats.data(), static_cast<uint32_t>(mats.size())),
          "crt_upload_scene");
    std::vector<crt_texture> tex;
    for (const TextureDesc& t : scene->getTextures()) {
        crt_texture x{};
        x.type = t.typeCode();
        x.color_a[0] = t.colorA.getX(); x.color_a[1] = t.colorA.getY(); x.color_a[2] = t.colorA.getZ();
        x.color_b[0] = t.colorB.getX(); x.color_b[1] = t.colorB.getY(); x.color_b[2] = t.colorB.getZ();
        x.scalar = t.scalar;
        x.pixels = t.pixels.empty() ? nullptr : t.pixels.data();
        x.width = static_cast<uint32_t>(t.width);
        x.height = static_cast<uint32_t>(t.height);
        x.channels = static_cast<uint32_t>(t.channels);
        tex.push_back(x);
    }
    check(crt_set_textures(ctx, tex.data(), static_cast<uint32_t>(tex.size())), "crt_set_textures");
}

void Renderer::render() { renderFrame(); }

void Renderer::renderFrame()
{
    if (!ctx || !scene) throw std::runtime_error("renderFrame before prepareForRendering");
    if (isChangedShadingMode) { // frameBegin: updateDebugCB only when dirty (R/DXRTRenderer.cpp:457-463)
        check(crt_set_shading_mode(ctx, currentShadingMode), "crt_set_shading_mode");
        isChangedShadingMode = false;
    }
    // updateCameraCB every frame (R/DXRTRenderer.cpp:464)
    check(crt_set_camera(ctx, scene->getCamera().getPosition().data(), scene->getCamera().getRotationMatrix().data()), "crt_set_camera");
    frame.resize(static_cast<size_t>(width) * height * 4);
    float* rgbF32 = nullptr;
    if (keepFloatColour && !nRanks) {
        floatColour.resize(static_cast<size_t>(width) * height * 3);
        rgbF32 = floatColour.data();
    }
    if (nRanks) check(crt_render_frame_distributed(ctx, width, height, nullptr, frame.data(), &stats), "crt_render_frame_distributed");
    else check(crt_render_frame(ctx, width, height, frame.data(), nullptr, nullptr, nullptr, rgbF32, &stats), "crt_render_frame");
}

double Renderer::rebuild()
{
    if (!ctx) throw std::runtime_error("rebuild before prepareForRendering");
    double ms = 0.0;
    check(crt_rebuild(ctx, &ms), "crt_rebuild");
    return ms;
}

void Renderer::setMeshTransform(uint32_t mesh, const float m[12])
{
    if (!ctx) throw std::runtime_error("setMeshTransform before prepareForRendering");
    check(crt_set_mesh_transform(ctx, mesh, m), "crt_set_mesh_transform");
}

void Renderer::updateMeshVertices(uint32_t mesh, const float* xyz, size_t nVertices, const float* normals)
{
    if (!ctx) throw std::runtime_error("updateMeshVertices before prepareForRendering");
    if (nVertices > UINT32_MAX) throw std::runtime_error("updateMeshVertices: more than 2^32 - 1 vertices");
    check(crt_update_vertices(ctx, mesh, static_cast<uint32_t>(nVertices), xyz, normals), "crt_update_vertices");
}

void Renderer::setOption(const char* name, int value)
{
    if (!ctx) throw std::runtime_error("setOption before prepareForRendering");
    check(crt_set_option(ctx, name, value), name);
}

void Renderer::setAmbientOcclusion(uint32_t samples, uint32_t radiusThousandths, bool sky)
{
    if (samples > INT32_MAX || radiusThousandths > INT32_MAX) throw std::runtime_error("setAmbientOcclusion: value out of range");
    setOption("ao_samples", static_cast<int>(samples));
    setOption("ao_radius", static_cast<int>(radiusThousandths));
    setOption("ao_sky", sky ? 1 : 0);
}

void Renderer::setAccumulation(uint32_t maxSamples)
{
    if (!ctx) throw std::runtime_error("setAccumulation before prepareForRendering");
    check(crt_set_accumulation(ctx, maxSamples), "crt_set_accumulation");
}

uint32_t Renderer::getAccumulatedSamples() const
{
    uint32_t n = 0;
    if (ctx) check(crt_accumulated_samples(ctx, &n), "crt_accumulated_samples");
    return n;
}

void Renderer::traceRays(const float* rays, size_t n, RayHit* out)
{
    if (!ctx) throw std::runtime_error("traceRays before prepareForRendering");
    if (n > UINT32_MAX) throw std::runtime_error("traceRays: more than 2^32 - 1 rays");
    if (n == 0) return;
    const uint32_t m = static_cast<uint32_t>(n);
    std::vector<float> t(n), uv(2 * n);
    std::vector<uint32_t> inst(n), prim(n);
    check(crt_trace_rays(ctx, m, rays, t.data(), uv.data(), inst.data(), prim.data(), nullptr), "crt_trace_rays");
    for (size_t i = 0; i < n; i++) out[i] = RayHit{ t[i], uv[2 * i], uv[2 * i + 1], inst[i], prim[i] };
}

void Renderer::shadeRays(const float* rays, size_t n, ShadedHit* out)
{
    if (!ctx) throw std::runtime_error("shadeRays before prepareForRendering");
    if (n > UINT32_MAX) throw std::runtime_error("shadeRays: more than 2^32 - 1 rays");
    if (isChangedShadingMode) { // a mode set since the last frame applies here as it would to the next frame
        check(crt_set_shading_mode(ctx, currentShadingMode), "crt_set_shading_mode");
        isChangedShadingMode = false;
    }
    if (n == 0) return;
    const uint32_t m = static_cast<uint32_t>(n);
    std::vector<float> rgb(3 * n), normal(3 * n), albedo(3 * n), t(n), uv(2 * n);
    std::vector<uint32_t> inst(n), prim(n);
    check(crt_shade_rays(ctx, m, rays, rgb.data(), normal.data(), albedo.data(), t.data(), uv.data(), inst.data(), prim.data(), nullptr), "crt_shade_rays");
    for (size_t i = 0; i < n; i++) {
        ShadedHit& o = out[i];
        for (int k = 0; k < 3; k++) {
            o.rgb[k] = rgb[3 * i + k];
            o.normal[k] = normal[3 * i + k];
            o.albedo[k] = albedo[3 * i + k];
        }
        o.hit = RayHit{ t[i], uv[2 * i], uv[2 * i + 1], inst[i], prim[i] };
    }
}

void Renderer::pathRays(const float* rays, size_t n, PathHit* out, const uint32_t* ids, uint32_t firstSample, uint32_t nSamples, double* sums)
{
    if (!ctx) throw std::runtime_error("pathRays before prepareForRendering");
    if (n > UINT32_MAX) throw std::runtime_error("pathRays: more than 2^32 - 1 rays");
    const uint32_t m = static_cast<uint32_t>(n);
    std::vector<float> rgb(3 * n), t(n), uv(2 * n);
    std::vector<uint32_t> inst(n), prim(n);
    check(crt_path_rays(ctx, m, rays, ids, firstSample, nSamples, rgb.data(), sums, t.data(), uv.data(), inst.data(), prim.data(), nullptr), "crt_path_rays");
    for (size_t i = 0; i < n; i++) {
        PathHit& o = out[i];
        for (int k = 0; k < 3; k++) o.rgb[k] = rgb[3 * i + k];
        o.hit = RayHit{ t[i], uv[2 * i], uv[2 * i + 1], inst[i], prim[i] };
    }
}

void Renderer::syncView()
{
    if (!ctx || !scene) throw std::runtime_error("no scene: call prepareForRendering first");
    if (isChangedShadingMode) {
        check(crt_set_shading_mode(ctx, currentShadingMode), "crt_set_shading_mode");
        isChangedShadingMode = false;
    }
    check(crt_set_camera(ctx, scene->getCamera().getPosition().data(), scene->getCamera().getRotationMatrix().data()), "crt_set_camera");
}

void Renderer::cameraRays(std::vector<float>& rays, uint32_t sample)
{
    syncView();
    rays.resize(static_cast<size_t>(width) * height * 8);
    check(crt_camera_rays(ctx, width, height, sample, rays.data(), nullptr), "crt_camera_rays");
}

void Renderer::frameGuides(Guides& out)
{
    syncView();
    const size_t n = static_cast<size_t>(width) * height;
    out.normal.resize(3 * n);
    out.albedo.resize(3 * n);
    out.t.resize(n);
    check(crt_frame_guides(ctx, width, height, out.normal.data(), out.albedo.data(), out.t.data(), nullptr), "crt_frame_guides");
}

void Renderer::denoise(const float* rgb, const Guides& guides, float* out, const crt_denoise_params* params)
{
    if (!ctx) throw std::runtime_error("denoise before prepareForRendering");
    const size_t n = static_cast<size_t>(width) * height;
    if (guides.normal.size() != 3 * n || guides.albedo.size() != 3 * n || guides.t.size() != n)
        throw std::runtime_error("denoise: the guides are not of the current frame size");
    check(crt_denoise(ctx, width, height, rgb, guides.normal.data(), guides.albedo.data(), guides.t.data(), out, params, nullptr), "crt_denoise");
}

void Renderer::denoiseFrame(const crt_denoise_params* params)
{
    const size_t n = static_cast<size_t>(width) * height;
    if (floatColour.size() != 3 * n || frame.size() != 4 * n) throw std::runtime_error("denoiseFrame: no frame with float colour (setKeepFloatColour, renderFrame)");
    Guides g;
    frameGuides(g);
    denoise(floatColour.data(), g, floatColour.data(), params);
    quantiseFloatColour();
}

void Renderer::quantiseFloatColour()
{
    const size_t n = static_cast<size_t>(width) * height;
    // the kernels' unorm8 (traversal.hip.h): saturate (NaN -> 0), x 255, + 0.5, truncate
    auto unorm8 = [](float c) { return static_cast<uint8_t>(std::fmin(std::fmax(c, 0.0f), 1.0f) * 255.0f + 0.5f); };
    for (size_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) frame[4 * i + k] = unorm8(floatColour[3 * i + k]);
        frame[4 * i + 3] = 255;
    }
}

void Renderer::temporalAccumulate(const float camCur[12], const float camPrev[12], const float* rgb, const Guides& guides, const float* histPrev,
                                  float* histNext, float* out, const crt_temporal_params* params)
{
    if (!ctx) throw std::runtime_error("temporalAccumulate before prepareForRendering");
    const size_t n = static_cast<size_t>(width) * height;
    if (guides.normal.size() != 3 * n || guides.albedo.size() != 3 * n || guides.t.size() != n)
        throw std::runtime_error("temporalAccumulate: the guides are not of the current frame size");
    check(crt_temporal_accumulate(ctx, width, height, camCur, camPrev, rgb, guides.normal.data(), guides.albedo.data(), guides.t.data(), histPrev,
                                  histNext, out, params, nullptr),
          "crt_temporal_accumulate");
}

void Renderer::motionSnapshot()
{
    if (!ctx) throw std::runtime_error("motionSnapshot before prepareForRendering");
    check(crt_motion_snapshot(ctx), "crt_motion_snapshot");
}

void Renderer::previousPoints(const uint32_t* inst, const uint32_t* prim, const float* uv, size_t n, std::vector<float>& points)
{
    if (!ctx) throw std::runtime_error("previousPoints before prepareForRendering");
    if (n > UINT32_MAX) throw std::runtime_error("previousPoints: more than 2^32 - 1 records");
    points.resize(3 * n);
    check(crt_previous_points(ctx, static_cast<uint32_t>(n), inst, prim, uv, points.data(), nullptr), "crt_previous_points");
}

void Renderer::frameMotion(std::vector<float>& prevPoint)
{
    syncView();
    prevPoint.resize(static_cast<size_t>(width) * height * 3);
    check(crt_frame_motion(ctx, width, height, prevPoint.data(), nullptr), "crt_frame_motion");
}

static size_t sceneVertexFloats(const Scene& scene)
{
    size_t n = 0;
    for (const Mesh& m : scene.getObjects()) n += m.getVertices().size();
    return 3 * n;
}

void Renderer::traceRaysBackward(const float* rays, const RayHit* hits, const float* gradT, const float* gradUv, size_t n, std::vector<float>* gradRays,
                                 std::vector<float>* gradXyz)
{
    if (!ctx || !scene) throw std::runtime_error("traceRaysBackward before prepareForRendering");
    if (n > UINT32_MAX) throw std::runtime_error("traceRaysBackward: more than 2^32 - 1 records");
    std::vector<uint32_t> inst(n), prim(n);
    std::vector<float> t(n), uv(2 * n);
    for (size_t i = 0; i < n; i++) {
        inst[i] = hits[i].inst;
        prim[i] = hits[i].prim;
        t[i] = hits[i].t;
        uv[2 * i] = hits[i].u;
        uv[2 * i + 1] = hits[i].v;
    }
    if (gradRays) gradRays->assign(8 * n, 0.0f);
    if (gradXyz) gradXyz->assign(sceneVertexFloats(*scene), 0.0f);
    check(crt_trace_rays_backward(ctx, static_cast<uint32_t>(n), rays, inst.data(), prim.data(), t.data(), uv.data(), gradT, gradUv,
                                  gradRays ? gradRays->data() : nullptr, gradXyz ? gradXyz->data() : nullptr, nullptr),
          "crt_trace_rays_backward");
}

void Renderer::closestPointsBackward(const float* points, const uint32_t* inst, const uint32_t* prim, const float* uv, const float* gradDist, size_t n,
                                     std::vector<float>* gradPoints, std::vector<float>* gradXyz)
{
    if (!ctx || !scene) throw std::runtime_error("closestPointsBackward before prepareForRendering");
    if (n > UINT32_MAX) throw std::runtime_error("closestPointsBackward: more than 2^32 - 1 records");
    if (gradPoints) gradPoints->assign(4 * n, 0.0f);
    if (gradXyz) gradXyz->assign(sceneVertexFloats(*scene), 0.0f);
    check(crt_closest_points_backward(ctx, static_cast<uint32_t>(n), points, inst, prim, uv, gradDist, gradPoints ? gradPoints->data() : nullptr,
                                      gradXyz ? gradXyz->data() : nullptr, nullptr),
          "crt_closest_points_backward");
}

void Renderer::windingNumbers(const float* points, size_t n, std::vector<float>& w, float beta)
{
    if (!ctx || !scene) throw std::runtime_error("windingNumbers before prepareForRendering");
    if (n > UINT32_MAX) throw std::runtime_error("windingNumbers: more than 2^32 - 1 records");
    w.assign(n, 0.0f);
    check(crt_winding_numbers(ctx, static_cast<uint32_t>(n), points, beta, w.data(), nullptr), "crt_winding_numbers");
}

void Renderer::windingMoments(std::vector<float>& moments)
{
    if (!ctx || !scene) throw std::runtime_error("windingMoments before prepareForRendering");
    uint32_t n4 = 0, depth4 = 0;
    check(crt_bvh_info4(ctx, &n4, &depth4), "crt_bvh_info4");
    moments.assign(32 * static_cast<size_t>(n4), 0.0f);
    if (n4) check(crt_winding_moments_export(ctx, moments.data()), "crt_winding_moments_export");
}

void Renderer::temporalFrame(const crt_temporal_params* params, bool motion)
{
    const size_t n = static_cast<size_t>(width) * height;
    if (floatColour.size() != 3 * n || frame.size() != 4 * n) throw std::runtime_error("temporalFrame: no frame with float colour (setKeepFloatColour, renderFrame)");
    Guides g;
    frameGuides(g);
    float cam[12];
    const auto pos = scene->getCamera().getPosition();
    const auto rot = scene->getCamera().getRotationMatrix();
    for (int k = 0; k < 3; k++) cam[k] = pos.data()[k];
    for (int k = 0; k < 9; k++) cam[3 + k] = rot.data()[k];
    const bool have = haveHistory && history[historyAt].size() == 8 * n;
    history[historyAt ^ 1].resize(8 * n);
    if (motion) {
        std::vector<float> prevPoint;
        frameMotion(prevPoint);
        check(crt_temporal_accumulate_motion(ctx, width, height, cam, have ? historyCamera : cam, floatColour.data(), g.normal.data(), g.albedo.data(),
                                             g.t.data(), prevPoint.data(), have ? history[historyAt].data() : nullptr, history[historyAt ^ 1].data(),
                                             floatColour.data(), params, nullptr),
              "crt_temporal_accumulate_motion");
    } else {
        temporalAccumulate(cam, have ? historyCamera : cam, floatColour.data(), g, have ? history[historyAt].data() : nullptr,
                           history[historyAt ^ 1].data(), floatColour.data(), params);
    }
    historyAt ^= 1;
    haveHistory = true;
    haveMoments = false;
    for (int k = 0; k < 12; k++) historyCamera[k] = cam[k];
    quantiseFloatColour();
}

void Renderer::temporalVariance(const float camCur[12], const float camPrev[12], const float* rgb, const Guides& guides, const float* prevPoint,
                                const float* histPrev, float* histNext, const float* momPrev, float* momNext, float* varianceOut, float* out,
                                const crt_temporal_variance_params* params)
{
    if (!ctx) throw std::runtime_error("temporalVariance before prepareForRendering");
    const size_t n = static_cast<size_t>(width) * height;
    if (guides.normal.size() != 3 * n || guides.albedo.size() != 3 * n || guides.t.size() != n)
        throw std::runtime_error("temporalVariance: the guides are not of the current frame size");
    check(crt_temporal_variance(ctx, width, height, camCur, camPrev, rgb, guides.normal.data(), guides.albedo.data(), guides.t.data(), prevPoint,
                                histPrev, histNext, momPrev, momNext, varianceOut, out, params, nullptr),
          "crt_temporal_variance");
}

void Renderer::denoiseVariance(const float* rgb, const Guides& guides, const float* varianceIn, float* out, float* varianceOut,
                               const crt_denoise_variance_params* params)
{
    if (!ctx) throw std::runtime_error("denoiseVariance before prepareForRendering");
    const size_t n = static_cast<size_t>(width) * height;
    if (guides.normal.size() != 3 * n || guides.albedo.size() != 3 * n || guides.t.size() != n)
        throw std::runtime_error("denoiseVariance: the guides are not of the current frame size");
    check(crt_denoise_variance(ctx, width, height, rgb, guides.normal.data(), guides.albedo.data(), guides.t.data(), varianceIn, out, varianceOut,
                               params, nullptr),
          "crt_denoise_variance");
}

void Renderer::temporalVarianceFrame(const crt_temporal_variance_params* params, bool motion)
{
    const size_t n = static_cast<size_t>(width) * height;
    if (floatColour.size() != 3 * n || frame.size() != 4 * n)
        throw std::runtime_error("temporalVarianceFrame: no frame with float colour (setKeepFloatColour, renderFrame)");
    Guides g;
    frameGuides(g);
    float cam[12];
    const auto pos = scene->getCamera().getPosition();
    const auto rot = scene->getCamera().getRotationMatrix();
    for (int k = 0; k < 3; k++) cam[k] = pos.data()[k];
    for (int k = 0; k < 9; k++) cam[3 + k] = rot.data()[k];
    const bool have = haveHistory && haveMoments && history[historyAt].size() == 8 * n && moments[historyAt].size() == 2 * n;
    history[historyAt ^ 1].resize(8 * n);
    moments[historyAt ^ 1].resize(2 * n);
    variance.resize(n);
    std::vector<float> prevPoint;
    if (motion) frameMotion(prevPoint);
    temporalVariance(cam, have ? historyCamera : cam, floatColour.data(), g, motion ? prevPoint.data() : nullptr,
                     have ? history[historyAt].data() : nullptr, history[historyAt ^ 1].data(), have ? moments[historyAt].data() : nullptr,
                     moments[historyAt ^ 1].data(), variance.data(), floatColour.data(), params);
    historyAt ^= 1;
    haveHistory = true;
    haveMoments = true;
    for (int k = 0; k < 12; k++) historyCamera[k] = cam[k];
    quantiseFloatColour();
}

void Renderer::denoiseVarianceFrame(const crt_denoise_variance_params* params)
{
    const size_t n = static_cast<size_t>(width) * height;
    if (floatColour.size() != 3 * n || frame.size() != 4 * n || variance.size() != n)
        throw std::runtime_error("denoiseVarianceFrame: no frame with a variance (temporalVarianceFrame)");
    Guides g;
    frameGuides(g);
    denoiseVariance(floatColour.data(), g, variance.data(), floatColour.data(), nullptr, params);
    quantiseFloatColour();
}

void Renderer::varianceFrame(const crt_temporal_variance_params* temporalParams, const crt_denoise_variance_params* denoiseParams, bool motion)
{
    temporalVarianceFrame(temporalParams, motion);
    denoiseVarianceFrame(denoiseParams);
}

void Renderer::listHits(const float* rays, size_t n, std::vector<uint64_t>& offsets, std::vector<RayHit>& hits)
{
    if (!ctx) throw std::runtime_error("listHits before prepareForRendering");
    if (n > UINT32_MAX) throw std::runtime_error("listHits: more than 2^32 - 1 rays");
    const uint32_t m = static_cast<uint32_t>(n);
    offsets.assign(n + 1, 0);
    uint64_t total = 0;
    check(crt_list_hits(ctx, m, rays, offsets.data(), 0, nullptr, nullptr, nullptr, nullptr, &total, nullptr), "crt_list_hits");
    hits.resize(total);
    if (total == 0) return;
    std::vector<float> t(total), uv(2 * total);
    std::vector<uint32_t> inst(total), prim(total);
    check(crt_list_hits(ctx, m, rays, offsets.data(), total, t.data(), uv.data(), inst.data(), prim.data(), &total, nullptr), "crt_list_hits");
    for (size_t i = 0; i < hits.size(); i++) hits[i] = RayHit{ t[i], uv[2 * i], uv[2 * i + 1], inst[i], prim[i] };
}

void Renderer::occluded(const float* rays, size_t n, uint8_t* out)
{
    if (!ctx) throw std::runtime_error("occluded before prepareForRendering");
    if (n > UINT32_MAX) throw std::runtime_error("occluded: more than 2^32 - 1 rays");
    check(crt_occluded_rays(ctx, static_cast<uint32_t>(n), rays, out, nullptr), "crt_occluded_rays");
}

// The id file holds {nonce, communicator id}.  The nonce names the launch (crt_render --ranks draws a fresh one per run): a file
// left behind by an earlier run, or by another launch that was given the same path, carries a different nonce and is waited out
// like a file that is not there yet instead of being taken for this run's id (ranks joining a dead communicator block for good).
void Renderer::joinRanks(uint32_t rankIn, uint32_t nRanksIn, const std::string& idFile, unsigned long long nonce)
{
    if (!ctx) throw std::runtime_error("joinRanks before prepareForRendering");
    unsigned char id[CRT_COMM_ID_BYTES];
    if (rankIn == 0) {
        if (crt_comm_unique_id(id) != CRT_OK) throw std::runtime_error(std::string("crt_comm_unique_id: ") + crt_last_error(nullptr));
        const std::string tmp = idFile + ".tmp";
        FILE* f = std::fopen(tmp.c_str(), "wb");
        const bool ok = f && std::fwrite(&nonce, 1, sizeof(nonce), f) == sizeof(nonce) && std::fwrite(id, 1, sizeof(id), f) == sizeof(id);
        if (f) std::fclose(f);
        if (!ok) throw std::runtime_error("cannot write '" + tmp + "'");
        if (std::rename(tmp.c_str(), idFile.c_str()) != 0) throw std::runtime_error("cannot publish '" + idFile + "'");
    } else {
        bool have = false;
        for (int tries = 0; tries < 6000 && !have; tries++) { // up to 60 s for rank 0 to come up
            FILE* f = std::fopen(idFile.c_str(), "rb");
            if (f) {
                unsigned long long seen = 0;
                have = std::fread(&seen, 1, sizeof(seen), f) == sizeof(seen) && seen == nonce && std::fread(id, 1, sizeof(id), f) == sizeof(id);
                std::fclose(f);
            }
            if (!have) std::this_thread::sleep_for(std::chrono::milliseconds(10));
        }
        if (!have) throw std::runtime_error("rank " + std::to_string(rankIn) + ": no communicator id of this launch in '" + idFile + "'");
    }
    check(crt_comm_init(ctx, rankIn, nRanksIn, id), "crt_comm_init");
    rank = rankIn;
    nRanks = nRanksIn;
}

void Renderer::joinRanksThroughHostMemory(uint32_t rankIn, uint32_t nRanksIn, unsigned long long nonce)
{
    if (!ctx) throw std::runtime_error("joinRanksThroughHostMemory before prepareForRendering");
    char name[64];
    std::snprintf(name, sizeof(name), "/crt_render_%016llx", nonce); // the launch's nonce names the shared-memory object
    check(crt_comm_init_host(ctx, rankIn, nRanksIn, name), "crt_comm_init_host");
    rank = rankIn;
    nRanks = nRanksIn;
}

void Renderer::stopRendering()
{
    if (ctx) check(crt_synchronize(ctx), "crt_synchronize");
}

void Renderer::changeShadingMode(uint32_t value)
{
    currentShadingMode = value;
    isChangedShadingMode = true;
}

Scene& Renderer::getScene()
{
    if (!scene) throw std::runtime_error("getScene before prepareForRendering");
    return *scene;
}

void Renderer::setFrameSize(uint32_t w, uint32_t h)
{
    width = w;
    height = h;
}

void Renderer::setCounting(bool on)
{
    if (ctx) check(crt_set_counting(ctx, on ? 1 : 0), "crt_set_counting");
}

void Renderer::writePPM(const std::string& path) const
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write '" + path + "'");
    std::fprintf(f, "P6\n%u %u\n255\n", width, height);
    std::vector<uint8_t> row(static_cast<size_t>(width) * 3);
    for (uint32_t y = 0; y < height; y++) {
        const uint8_t* src = frame.data() + static_cast<size_t>(y) * width * 4;
        for (uint32_t x = 0; x < width; x++) {
            row[3 * x] = src[4 * x];
            row[3 * x + 1] = src[4 * x + 1];
            row[3 * x + 2] = src[4 * x + 2];
        }
        std::fwrite(row.data(), 1, row.size(), f);
    }
    std::fclose(f);
}

// PNG, 8-bit RGB, scanlines unfiltered, the zlib stream made of stored blocks: every PNG reader accepts it and the writer needs
// no compressor (an 8 MB frame becomes an 8 MB file; the viewer's frames are for looking at and for regression checks).
void Renderer::writePNG(const std::string& path) const
{
    static uint32_t crcTable[256];
    static bool haveTable = false;
    if (!haveTable) {
        for (uint32_t n = 0; n < 256; n++) {
            uint32_t c = n;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            crcTable[n] = c;
        }
        haveTable = true;
    }
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write '" + path + "'");
    auto be32 = [](uint8_t* p, uint32_t v) { p[0] = uint8_t(v >> 24); p[1] = uint8_t(v >> 16); p[2] = uint8_t(v >> 8); p[3] = uint8_t(v); };
    auto chunk = [&](const char* type, const std::vector<uint8_t>& body) {
        uint8_t head[8];
        be32(head, static_cast<uint32_t>(body.size()));
        std::memcpy(head + 4, type, 4);
        uint32_t c = 0xFFFFFFFFu;
        for (int i = 4; i < 8; i++) c = crcTable[(c ^ head[i]) & 255u] ^ (c >> 8);
        for (uint8_t b : body) c = crcTable[(c ^ b) & 255u] ^ (c >> 8);
        uint8_t tail[4];
        be32(tail, c ^ 0xFFFFFFFFu);
        std::fwrite(head, 1, 8, f);
        if (!body.empty()) std::fwrite(body.data(), 1, body.size(), f);
        std::fwrite(tail, 1, 4, f);
    };
    static const uint8_t magic[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
    std::fwrite(magic, 1, 8, f);
    std::vector<uint8_t> ihdr(13);
    be32(ihdr.data(), width);
    be32(ihdr.data() + 4, height);
    ihdr[8] = 8; ihdr[9] = 2; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0; // 8 bits, RGB, deflate, filter method 0, not interlaced
    chunk("IHDR", ihdr);
    // raw image data: a filter byte (0) and 3 bytes per pixel for every scanline
    std::vector<uint8_t> raw;
    raw.reserve(static_cast<size_t>(height) * (1 + 3 * static_cast<size_t>(width)));
    for (uint32_t y = 0; y < height; y++) {
        raw.push_back(0);
        const uint8_t* src = frame.data() + static_cast<size_t>(y) * width * 4;
        for (uint32_t x = 0; x < width; x++) raw.insert(raw.end(), src + 4 * x, src + 4 * x + 3);
    }
    std::vector<uint8_t> z;
    z.reserve(raw.size() + raw.size() / 65535 * 5 + 16);
    z.push_back(0x78); z.push_back(0x01);
    uint32_t a = 1, b = 0; // Adler-32 of the raw data
    for (size_t at = 0; at < raw.size() || at == 0; at += 65535) {
        const size_t n = std::min<size_t>(65535, raw.size() - at);
        z.push_back(at + n >= raw.size() ? 1 : 0); // last block?
        z.push_back(uint8_t(n)); z.push_back(uint8_t(n >> 8)); z.push_back(uint8_t(~n)); z.push_back(uint8_t((~n) >> 8));
        z.insert(z.end(), raw.begin() + static_cast<std::ptrdiff_t>(at), raw.begin() + static_cast<std::ptrdiff_t>(at + n));
        for (size_t i = at; i < at + n; i++) {
            a = (a + raw[i]) % 65521u;
            b = (b + a) % 65521u;
        }
        if (raw.empty()) break;
    }
    uint8_t adler[4];
    be32(adler, (b << 16) | a);
    z.insert(z.end(), adler, adler + 4);
    chunk("IDAT", z);
    chunk("IEND", {});
    std::fclose(f);
}

} // namespace crt
