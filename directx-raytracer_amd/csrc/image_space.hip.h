// What the image-space passes share (temporal_kernels.hip, denoise_kernels.hip): one thread per pixel, a
// wavefront = 64 consecutive x of one row, a workgroup = 4 rows, the kernel strides over tiles -- so every tap of a pass is a
// contiguous row segment per wavefront.  Nothing here does arithmetic of its own: the helpers are the expressions the kernels
// wrote out before, -ffp-contract=off, fmaf exactly where it stands.  They are values without control flow on purpose: that is
// the form in which the kernels compile to the instruction streams they had (section 5l).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstddef>
#include <cstdint>

namespace crt {
namespace {

constexpr uint32_t kTileX = 64, kTileY = 4; // pixels of a workgroup: one wavefront per row
constexpr uint32_t kMaxGrid = 1u << 20;     // workgroups of a launch; the kernels stride over what is left

// host side: the grid of a launch over `groups` workgroups' worth of work, and of one over the tiles of an image (0: no pixel)
inline uint32_t cappedGrid(size_t groups) { return static_cast<uint32_t>(std::min<size_t>(groups, kMaxGrid)); }
inline uint32_t tileGrid(uint32_t width, uint32_t height)
{
    return cappedGrid(static_cast<size_t>((width + kTileX - 1u) / kTileX) * ((height + kTileY - 1u) / kTileY));
}

// The tile walk:   const TileWalk walk(width, height);
//                  for (uint32_t tile = blockIdx.x; tile < walk.nTiles; tile += gridDim.x) { const uint2 o = walk.origin(tile); ...
// (o.x + walk.lx, o.y + walk.ly) is this lane's pixel; it may lie outside the image.  The loop is uniform over the workgroup, so
// a kernel that keeps every lane in it may hold barriers.
struct TileWalk {
    uint32_t tilesX, nTiles; // nTiles < 2^28 for width * height <= 2^28
    uint32_t lx, ly;         // the lane's place in its tile
    __device__ __forceinline__ TileWalk(uint32_t width, uint32_t height)
        : tilesX((width + kTileX - 1u) / kTileX), nTiles(tilesX * ((height + kTileY - 1u) / kTileY)), lx(threadIdx.x & 63u), ly(threadIdx.x >> 6)
    {
    }
    __device__ __forceinline__ uint2 origin(uint32_t tile) const // the tile's first pixel
    {
        const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
        return make_uint2(tx * kTileX, ty * kTileY);
    }
};

__device__ __forceinline__ size_t pixelIndex(uint32_t width, int x, int y) { return static_cast<size_t>(y) * width + static_cast<size_t>(x); }
// a predicated tap: is it wanted and inside the image?  One that is not loads the centre's own record and gets weight 0
__device__ __forceinline__ bool tapInside(uint32_t width, uint32_t height, int qx, int qy, bool wanted = true)
{
    return wanted & (static_cast<uint32_t>(qx) < width) & (static_cast<uint32_t>(qy) < height);
}

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= FLT_MAX; } // false for NaN
// what the guides say of a pixel whose values are finite: a normal that is not zero, a hit in front of the camera
__device__ __forceinline__ bool guideLive(float nx, float ny, float nz, float t) { return (nx != 0.0f || ny != 0.0f || nz != 0.0f) && t > 0.0f; }

__device__ __forceinline__ float luminance(float r, float g, float b) { return fmaf(0.0722f, b, fmaf(0.7152f, g, 0.2126f * r)); }
__device__ __forceinline__ float albedoFloor(float a) { return fmaxf(a, 1e-3f); } // what a colour is divided by and multiplied back with

} // namespace
} // namespace crt
