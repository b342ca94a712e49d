// crt::Renderer::pathRays from C++ (tests/test_path_rays.py::test_cpp_layer):
//   path_rays_cpp SCENE RAYS FIRST SAMPLES BOUNCES SEED OUT
// SCENE: a scene file crt_scene_load accepts; RAYS: n x 8 float32 records (ids = record numbers); FIRST, SAMPLES: the sample
// range, traced as two calls chained through one sums buffer when SAMPLES > 1; OUT: n PathHit records (32 bytes: rgb, RayHit).
#include "renderer.h"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s SCENE RAYS FIRST SAMPLES BOUNCES SEED OUT\n", argv[0]);
        return 2;
    }
    try {
        std::ifstream in(argv[2], std::ios::binary | std::ios::ate);
        const std::streamsize bytes = in.tellg();
        in.seekg(0);
        std::vector<float> rays(static_cast<size_t>(bytes) / sizeof(float));
        in.read(reinterpret_cast<char*>(rays.data()), bytes);
        const size_t n = rays.size() / 8;
        const uint32_t first = static_cast<uint32_t>(std::atoi(argv[3])), samples = static_cast<uint32_t>(std::atoi(argv[4]));

        crt::Renderer r;
        r.prepareForRendering(argv[1], 0);
        r.setOption("max_bounces", std::atoi(argv[5]));
        r.setOption("seed", std::atoi(argv[6]));
        std::vector<crt::Renderer::PathHit> hits(n);
        static_assert(sizeof(crt::Renderer::PathHit) == 32, "three floats and a RayHit");
        if (samples > 1 && first == 0) { // the first sample alone, then the rest on top of its sums
            std::vector<double> sums(3 * n);
            r.pathRays(rays.data(), n, hits.data(), nullptr, 0, 1, sums.data());
            r.pathRays(rays.data(), n, hits.data(), nullptr, 1, samples - 1, sums.data());
        } else {
            r.pathRays(rays.data(), n, hits.data(), nullptr, first, samples);
        }
        std::ofstream out(argv[7], std::ios::binary);
        out.write(reinterpret_cast<const char*>(hits.data()), static_cast<std::streamsize>(n * sizeof(crt::Renderer::PathHit)));
        std::printf("%zu rays\n", n);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "path_rays_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
