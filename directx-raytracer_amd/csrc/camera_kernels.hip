// HIP kernel for gfx950 (MI355X): the frames' camera rays as ray records (crt_camera_rays*, and the first step of
// crt_frame_guides*).  One thread per pixel.  Nothing of the ray generation is restated here: the direction is rayDirJ and the
// jitter of a mode-200 sample is the pcgHash / rngNext chain of shading.hip.h, called with the arguments pathKernel and the
// render kernel call them with (path_kernels.hip stage A; render_kernels.hip rayDir), so that a record is bit for bit the ray
// the frame kernels trace for that pixel.
//
// Arithmetic contract: identical, operation for operation, to oracle/crt_oracle.c (compiled with -ffp-contract=off).
#include "shading.hip.h"

namespace crt {
namespace {

__global__ __launch_bounds__(256) void cameraRayKernel(const CameraRayParams p)
{
    const uint32_t n = p.width * p.height; // <= 2^28 (crt_api.cpp checkFrameSize)
    const uint32_t pixId = blockIdx.x * 256u + threadIdx.x;
    if (pixId >= n) return;
    const uint32_t px = pixId % p.width, py = pixId / p.width;
    float jx = 0.5f, jy = 0.5f;
    if (p.sample != kSampleCentre) {
        uint32_t rng = pcgHash(pixId ^ pcgHash(p.sample + pcgHash(p.seed)));
        jx = rngNext(rng);
        jy = rngNext(rng);
    }
    const F3 d = rayDirJ(p.rot, px, py, jx, jy, static_cast<float>(p.width), static_cast<float>(p.height));
    float4* rec = reinterpret_cast<float4*>(p.rays) + 2u * static_cast<size_t>(pixId);
    rec[0] = make_float4(p.pos[0], p.pos[1], p.pos[2], kTMin);
    rec[1] = make_float4(d.x, d.y, d.z, kTMax);
}

} // namespace

int launchCameraRays(const CameraRayParams& p, ihipStream_t* stream)
{
    const uint32_t n = p.width * p.height;
    if (n == 0u) return static_cast<int>(hipSuccess);
    const dim3 g((n + 255u) / 256u), block(256);
    hipLaunchKernelGGL(cameraRayKernel, g, block, 0, stream, p);
    return static_cast<int>(hipGetLastError());
}

} // namespace crt
