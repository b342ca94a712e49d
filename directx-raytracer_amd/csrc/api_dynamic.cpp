// C ABI, dynamic geometry (crt_ctx.h maps the units): vertex updates and transforms, refit and rebuild, motion, and the
// gradients of ray and closest-point queries.
#include "crt_ctx.h"

#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <new>
#include <utility>

using namespace crtapi;

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
    if (!c->grad.dSum) HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&c->grad.dSum), bytes));
    sums = c->grad.dSum;
    return CRT_OK;
}

int gradSumsZero(crt_ctx* c, double* sums)
{
    if (!sums) return static_cast<int>(hipSuccess);
    if (const hipError_t e = c->grad.used.wait(c->stream, false)) return static_cast<int>(e);
    return static_cast<int>(hipMemsetAsync(sums, 0, sizeof(double) * 3 * static_cast<size_t>(c->dyn->nVerts), c->stream));
}

int gradSumsEnd(crt_ctx* c, const double* sums, void* d_grad_xyz)
{
    if (!sums) return static_cast<int>(hipSuccess);
    const int hrc = crt::launchGradFinalize(sums, static_cast<float*>(d_grad_xyz), 3 * static_cast<size_t>(c->dyn->nVerts), c->stream);
    return hrc != 0 ? hrc : static_cast<int>(c->grad.used.record(c->stream));
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
