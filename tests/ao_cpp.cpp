// crt::Renderer::setAmbientOcclusion and shadeRays in shading mode 120 from C++ (tests/test_occlusion_mode.py::test_cpp_layer_and_driver):
//   ao_cpp SCENE WIDTH HEIGHT SAMPLES RADIUS SKY OUT
// SCENE: a scene file crt_scene_load accepts.  OUT receives one ShadedHit record (56 bytes: rgb, normal, albedo, then the
// RayHit) per pixel-centre camera ray of a WIDTH x HEIGHT frame.
#include "renderer.h"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s SCENE WIDTH HEIGHT SAMPLES RADIUS SKY OUT\n", argv[0]);
        return 2;
    }
    try {
        crt::Renderer r;
        r.prepareForRendering(argv[1], 0);
        r.setFrameSize(static_cast<uint32_t>(std::atoi(argv[2])), static_cast<uint32_t>(std::atoi(argv[3])));
        r.changeShadingMode(CRT_MODE_AMBIENT);
        r.setAmbientOcclusion(static_cast<uint32_t>(std::atoi(argv[4])), static_cast<uint32_t>(std::atoi(argv[5])), std::atoi(argv[6]) != 0);
        std::vector<float> rays;
        r.cameraRays(rays);
        const size_t n = rays.size() / 8;
        std::vector<crt::Renderer::ShadedHit> hits(n);
        r.shadeRays(rays.data(), n, hits.data());
        static_assert(sizeof(crt::Renderer::ShadedHit) == 56, "nine floats and a RayHit");
        std::ofstream out(argv[7], std::ios::binary);
        out.write(reinterpret_cast<const char*>(hits.data()), static_cast<std::streamsize>(n * sizeof(crt::Renderer::ShadedHit)));
        std::printf("%zu rays\n", n);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ao_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
