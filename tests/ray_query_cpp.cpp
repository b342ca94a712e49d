// crt::Renderer::traceRays / occluded from C++ (tests/test_ray_queries.py::test_cpp_layer):
//   ray_query_cpp SCENE RAYS OUT
// SCENE: a scene file crt_scene_load accepts; RAYS: n x 8 float32 records; OUT: n RayHit records (20 bytes) followed by
// n occlusion bytes.
#include "renderer.h"

#include <cstdio>
#include <exception>
#include <fstream>
#include <memory>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s SCENE RAYS OUT\n", argv[0]);
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
        std::vector<crt::Renderer::RayHit> hits(n);
        std::vector<uint8_t> occ(n);
        r.traceRays(rays.data(), n, hits.data());
        r.occluded(rays.data(), n, occ.data());
        static_assert(sizeof(crt::Renderer::RayHit) == 20, "five 4-byte fields");
        std::ofstream out(argv[3], std::ios::binary);
        out.write(reinterpret_cast<const char*>(hits.data()), static_cast<std::streamsize>(n * sizeof(crt::Renderer::RayHit)));
        out.write(reinterpret_cast<const char*>(occ.data()), static_cast<std::streamsize>(n));
        std::printf("%zu rays\n", n);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ray_query_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
