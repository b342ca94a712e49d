// crt::Renderer -- C++ host class with the public interface of DXRTRenderer (R/DXRTRenderer.h:74-94):
//   prepareForRendering / prepareForRayTracing / render / renderFrame / stopRendering / changeShadingMode / getScene
// so that the reference's app loop (R/DXRTApp.cpp:29-120) can drive the MI355X renderer unchanged.  It owns the
// scene like the reference (std::unique_ptr<CRTScene>, R/DXRTRenderer.h:242) and talks to the GPU only through
// the C ABI of include/crt_hip.h.  The window handle of the reference is replaced by a scene path + device id;
// the swap chain by a host frame buffer (R8G8B8A8) that can be written as PPM.
#pragma once

#include "../../include/crt_hip.h"
#include "scene.h"

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace crt {

class Renderer {
public:
    Renderer();
    ~Renderer();
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    // R/DXRTRenderer.cpp:44-62: device + scene + geometry upload + acceleration structure.
    // sceneFile defaults to the path the reference hard-codes (R/DXRTRenderer.cpp:245). Throws std::runtime_error.
    void prepareForRendering(const std::string& sceneFile = "Scenes/Dragon.crtscene", int deviceId = 0);
    void prepareForRendering(std::unique_ptr<Scene> ownedScene, int deviceId = 0);
    void prepareForRayTracing(); // root signature / PSO / SBT have no HIP counterpart: kept as a no-op
    void render();               // R/DXRTRenderer.cpp:35-42: one frame
    void renderFrame();          // R/DXRTRenderer.cpp:1370-1408: camera CB update + dispatch + sync
    void stopRendering();        // drains the stream (the reference's body is empty, R/DXRTRenderer.cpp:1354-1357)
    void changeShadingMode(uint32_t value);
    Scene& getScene();

    // headless replacements for the swap chain
    void setFrameSize(uint32_t width, uint32_t height); // reference: fixed 1920x1080 (R/DXRTRenderer.cpp:1348-1349)
    uint32_t getFrameWidth() const { return width; }
    uint32_t getFrameHeight() const { return height; }
    const std::vector<uint8_t>& getFrame() const { return frame; } // RGBA8, row-major, top-left origin
    void writePPM(const std::string& path) const;
    void writePNG(const std::string& path) const; // 8-bit RGB, stored (uncompressed) deflate blocks
    const crt_frame_stats& getLastFrameStats() const { return stats; }
    void setCounting(bool on);
    void setOption(const char* name, int value); // crt_set_option: "spp", "max_bounces", "seed", "phong_ks", "phong_exponent", ...
    // mode 120 (CRT_MODE_AMBIENT): the options "ao_samples" (1..4096), "ao_radius" (thousandths of the scene box's diagonal,
    // 0 = unbounded) and "ao_sky" (point lights plus a sky of the miss colour instead of the grey visibility)
    void setAmbientOcclusion(uint32_t samples, uint32_t radiusThousandths, bool sky);
    // crt_set_accumulation: mode-200 frames add their samples to running sums while the camera holds still (0 = off)
    void setAccumulation(uint32_t maxSamples);
    uint32_t getAccumulatedSamples() const; // crt_accumulated_samples

    // batched ray queries on the uploaded scene (crt_trace_rays / crt_occluded_rays, synchronous): n records of 8 floats
    // {ox, oy, oz, tmin, dx, dy, dz, tmax}.  A miss reports inst = prim = CRT_MISS, t = the ray's tmax, u = v = 0.
    struct RayHit {
        float t, u, v;
        uint32_t inst, prim;
    };
    void traceRays(const float* rays, size_t n, RayHit* out);
    void occluded(const float* rays, size_t n, uint8_t* out); // 1 = some triangle lies in (tmin, tmax)
    // the closest hit shaded in the current mode (crt_shade_rays, synchronous; modes 0..100, 120: the share of the sky the hit
    // point sees, CRT_MODE_AMBIENT, and 150: the colour seen through mirrors and glass, CRT_MODE_WHITTED): colour, shading normal
    // and albedo beside the hit.  A miss reports the miss colour, a zero normal and a zero albedo.
    struct ShadedHit {
        float rgb[3], normal[3], albedo[3];
        RayHit hit;
    };
    void shadeRays(const float* rays, size_t n, ShadedHit* out);
    // mode-200 radiance of every ray (crt_path_rays, synchronous; any shading mode): n_samples paths per record, samples
    // firstSample .. firstSample + nSamples - 1 of path id ids[i] (nullptr: i); sums (nullptr, or 3 doubles per ray, in / out)
    // carries the sample sums from call to call.  The hit is the record's own closest hit.
    struct PathHit {
        float rgb[3];
        RayHit hit;
    };
    void pathRays(const float* rays, size_t n, PathHit* out, const uint32_t* ids = nullptr, uint32_t firstSample = 0, uint32_t nSamples = 1,
                  double* sums = nullptr);
    // the frames' own camera rays for the current frame size and the scene's camera (crt_camera_rays, synchronous): width x
    // height records of 8 floats, record py * width + px.  sample = CRT_SAMPLE_CENTRE: the rays of modes 0..100; a value
    // below 2^24: the jittered rays of that mode-200 frame sample
    void cameraRays(std::vector<float>& rays, uint32_t sample = CRT_SAMPLE_CENTRE);
    // the guide buffers of the current frame size and camera (crt_frame_guides, synchronous; any shading mode): per pixel
    // the shading normal and the albedo (3 floats) and t of the pixel-centre ray
    struct Guides {
        std::vector<float> normal, albedo, t;
    };
    void frameGuides(Guides& out);
    // the edge-avoiding a-trous filter (crt_denoise, synchronous) on width x height buffers: rgb (3 floats per pixel) with its
    // guides into out (may be rgb); params = nullptr: the defaults
    void denoise(const float* rgb, const Guides& guides, float* out, const crt_denoise_params* params = nullptr);
    // renderFrame() also keeps the frame's float colour (single-GPU path), for denoiseFrame()
    void setKeepFloatColour(bool on) { keepFloatColour = on; }
    const std::vector<float>& getFloatColour() const { return floatColour; }
    // the last frame's float colour denoised with its guides and quantised into getFrame() with the frames' own UNORM rule
    void denoiseFrame(const crt_denoise_params* params = nullptr);
    // temporal reprojection (crt_temporal_accumulate, synchronous) on width x height buffers: rgb with its guides, blended with
    // the history records histPrev (8 floats per pixel; nullptr = no history) that were taken with camera camPrev, into
    // histNext and out (may be rgb or nullptr).  Cameras: {pos[3], rot3x3 row-major[9]}; params = nullptr: the defaults
    void temporalAccumulate(const float camCur[12], const float camPrev[12], const float* rgb, const Guides& guides, const float* histPrev,
                            float* histNext, float* out, const crt_temporal_params* params = nullptr);
    // the last frame's float colour accumulated with the history of the frames before it and quantised into getFrame().  The
    // renderer owns the two history buffers and the previous camera; a change of the frame size drops the history, and so
    // does resetTemporal() (after a cut, or after geometry moved when temporalFrame runs without motion)
    // motion: with the previous points of the frame (frameMotion) a moved mesh keeps its history; needs a dynamic scene and a
    // motionSnapshot() after each frame, before the meshes are moved
    void temporalFrame(const crt_temporal_params* params = nullptr, bool motion = false);
    // crt_motion_snapshot: remember the current world vertices of a dynamic scene as "previous"
    void motionSnapshot();
    // crt_previous_points (synchronous): where the hits (inst, prim, {u, v}) were at the last snapshot, 3 floats per record, NaN for a
    // miss and for a triangle that did not move
    void previousPoints(const uint32_t* inst, const uint32_t* prim, const float* uv, size_t n, std::vector<float>& points);
    // crt_frame_motion (synchronous): the previous points of the pixel-centre camera rays, width * height * 3 floats
    void frameMotion(std::vector<float>& prevPoint);
    // crt_trace_rays_backward (synchronous; needs a dynamic scene): the gradients of a loss on the hits traceRays reported for
    // `rays` -- gradT: dL/dt per record, gradUv: dL/du, dL/dv per record, either may be nullptr (zeros), not both -- with respect
    // to the rays (gradRays: 8 floats per record {dL/do, 0, dL/dd, 0}) and to the world vertices (gradXyz: 3 floats per vertex,
    // the scene's meshes back to back).  Either output may be nullptr, not both
    void traceRaysBackward(const float* rays, const RayHit* hits, const float* gradT, const float* gradUv, size_t n, std::vector<float>* gradRays,
                           std::vector<float>* gradXyz);
    // crt_closest_points_backward (synchronous; needs a dynamic scene): the gradients of a loss on the distances crt_closest_points
    // reported for `points` (4 floats per record) at the surface points (inst, prim, {u, v}) -- gradDist: dL/ddist per record --
    // with respect to the points (gradPoints: 4 floats per record {dL/dp, 0}) and to the world vertices (gradXyz, as above)
    void closestPointsBackward(const float* points, const uint32_t* inst, const uint32_t* prim, const float* uv, const float* gradDist, size_t n,
                               std::vector<float>* gradPoints, std::vector<float>* gradXyz);
    // crt_winding_numbers (synchronous): the generalised winding number of n points (4 floats per record {x, y, z, unused}), one
    // float each; beta > 0: clusters farther than beta x their radius are taken by their dipole, beta <= 0: every triangle
    void windingNumbers(const float* points, size_t n, std::vector<float>& w, float beta = 2.0f);
    // crt_winding_moments_export: 32 floats per wide node of the tree as it stands
    void windingMoments(std::vector<float>& moments);
    void resetTemporal() { haveHistory = false; }
    // temporalAccumulate with luminance moments (crt_temporal_variance, synchronous): momPrev / momNext hold 2 floats per pixel
    // beside the history records (momPrev is nullptr exactly when histPrev is), variance receives 1 float per pixel; prevPoint:
    // nullptr, or the previous points of the frame (frameMotion)
    void temporalVariance(const float camCur[12], const float camPrev[12], const float* rgb, const Guides& guides, const float* prevPoint,
                          const float* histPrev, float* histNext, const float* momPrev, float* momNext, float* variance, float* out,
                          const crt_temporal_variance_params* params = nullptr);
    // denoise with a variance-driven luminance weight (crt_denoise_variance, synchronous): variance as temporalVariance wrote it,
    // varianceOut (may be variance, may be nullptr) the filtered variance
    void denoiseVariance(const float* rgb, const Guides& guides, const float* variance, float* out, float* varianceOut = nullptr,
                         const crt_denoise_variance_params* params = nullptr);
    // temporalFrame() through crt_temporal_variance: the renderer owns two moment buffers beside the history buffers and keeps
    // the frame's variance (getVariance()) for denoiseVarianceFrame().  A temporalFrame() in between drops the moments, and the
    // history with them
    void temporalVarianceFrame(const crt_temporal_variance_params* params = nullptr, bool motion = false);
    const std::vector<float>& getVariance() const { return variance; }
    // the accumulated colour of the last temporalVarianceFrame() filtered with its variance and quantised into getFrame(); the
    // history keeps the unfiltered colour
    void denoiseVarianceFrame(const crt_denoise_variance_params* params = nullptr);
    // both: the last frame accumulated with moments, then filtered with the variance into getFrame()
    void varianceFrame(const crt_temporal_variance_params* temporalParams = nullptr, const crt_denoise_variance_params* denoiseParams = nullptr,
                       bool motion = false);
    // every crossing of every ray, ascending in t (crt_list_hits, synchronous): the hits of ray i are hits[offsets[i]] ..
    // hits[offsets[i + 1] - 1].  One offsets-only call learns the total, a second one fills the records.
    void listHits(const float* rays, size_t n, std::vector<uint64_t>& offsets, std::vector<RayHit>& hits);

    // dynamic geometry (crt_update_vertices / crt_set_mesh_transform, include/crt_hip.h): enable before prepareForRendering, whose
    // upload then keeps what a refit needs.  Updates are applied before the next frame or ray query.
    void setDynamicGeometry(bool on) { dynamicGeometry = on; }
    void setMeshTransform(uint32_t mesh, const float m[12]);                                          // row-major 3x4; nullptr = identity
    void updateMeshVertices(uint32_t mesh, const float* xyz, size_t nVertices, const float* normals = nullptr); // normals: nullptr = keep
    // crt_rebuild: pending updates applied and a new tree built on the GPU from the world vertices (builder: setGpuBuilder);
    // returns the device ms
    double rebuild();
    // the acceleration structure of the next upload and of rebuild(): -1 = host SAH (the default; rebuild() then uses the LBVH),
    // 0 = LBVH on the GPU, 1 = PLOC on the GPU (options "gpu_build" / "gpu_builder").  Set before prepareForRendering.
    void setGpuBuilder(int builder) { gpuBuilder = builder; }

    // N GPUs, one process each (no reference counterpart): join the RCCL communicator of an N-rank run.  Rank 0 creates the
    // 128-byte id and publishes it as `idFile` (written under a temporary name, then renamed); the other ranks wait for the
    // file.  Afterwards renderFrame() renders this rank's tiles, gathers and de-interleaves: every rank holds the frame.
    void joinRanks(uint32_t rank, uint32_t nRanks, const std::string& idFile, unsigned long long nonce = 0);
    // the same with shared host memory as the transport (crt_comm_init_host): ranks that share one GPU -- a rehearsal, not a measurement
    void joinRanksThroughHostMemory(uint32_t rank, uint32_t nRanks, unsigned long long nonce);
    uint32_t getRank() const { return rank; }
    uint32_t getRankCount() const { return nRanks; }

private:
    crt_ctx* ctx = nullptr;
    std::unique_ptr<Scene> scene;
    uint32_t width = 1920, height = 1080;
    uint32_t currentShadingMode = 0; // R/DXRTRenderer.h:246
    bool isChangedShadingMode = true;
    std::vector<uint8_t> frame;
    std::vector<float> floatColour; // rgb_f32 of the last frame when keepFloatColour
    bool keepFloatColour = false;
    std::vector<float> history[2]; // temporalFrame(): history[historyAt] is the previous frame's
    int historyAt = 0;
    bool haveHistory = false;
    float historyCamera[12] = {};
    std::vector<float> moments[2]; // temporalVarianceFrame(): moments[historyAt] belongs to history[historyAt]
    bool haveMoments = false;
    std::vector<float> variance;   // of the last temporalVarianceFrame()
    void quantiseFloatColour(); // floatColour into frame with the frames' own UNORM rule
    void syncView(); // a pending mode change and the scene's camera, as renderFrame() applies them
    crt_frame_stats stats{};
    uint32_t rank = 0, nRanks = 0; // nRanks = 0: single-GPU path (crt_render_frame)
    bool dynamicGeometry = false;
    int gpuBuilder = -1;
    void uploadScene();
    void check(int rc, const char* what) const;
};

} // namespace crt
