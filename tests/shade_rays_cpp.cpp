// crt::Renderer::shadeRays from C++ (tests/test_shade_rays.py::test_cpp_layer):
//   shade_rays_cpp SCENE RAYS MODE OUT
// SCENE: a scene file crt_scene_load accepts; RAYS: n x 8 float32 records; MODE: the shading mode; OUT: n ShadedHit records
// (56 bytes: rgb, normal, albedo, then the RayHit).
#include "renderer.h"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s SCENE RAYS MODE OUT\n", argv[0]);
        return 2;
    }
    try {
        std::ifstream in(argv[2], std::ios::binary | std::ios::ate);
        const std::streamsize bytes = in.tellg();
        in.seekg(0);
        std::vector<float> rays(static_cast<size_t>(bytes) / sizeof(float));
        in.read(reinterpret_cast<char*>(rays.data()), bytes);
        const size_t n = rays.size() / 8;

        crt::Renderer r;
        r.prepareForRendering(argv[1], 0);
        r.changeShadingMode(static_cast<uint32_t>(std::atoi(argv[3])));
        std::vector<crt::Renderer::ShadedHit> hits(n);
        r.shadeRays(rays.data(), n, hits.data());
        static_assert(sizeof(crt::Renderer::ShadedHit) == 56, "nine floats and a RayHit");
        std::ofstream out(argv[4], std::ios::binary);
        out.write(reinterpret_cast<const char*>(hits.data()), static_cast<std::streamsize>(n * sizeof(crt::Renderer::ShadedHit)));
        std::printf("%zu rays\n", n);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "shade_rays_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
