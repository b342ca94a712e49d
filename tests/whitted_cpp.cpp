// crt::Renderer::renderFrame and shadeRays in shading mode 150 from C++ (tests/test_whitted.py::test_cpp_layer_and_driver):
//   whitted_cpp SCENE WIDTH HEIGHT BOUNCES OUT
// SCENE: a scene file crt_scene_load accepts.  OUT receives, back to back: the frame's RGBA8 (4 bytes per pixel), its float
// colour (3 floats per pixel) and one ShadedHit record (56 bytes: rgb, normal, albedo, then the RayHit) per pixel-centre
// camera ray of that frame.
#include "renderer.h"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s SCENE WIDTH HEIGHT BOUNCES OUT\n", argv[0]);
        return 2;
    }
    try {
        crt::Renderer r;
        r.prepareForRendering(argv[1], 0);
        r.setFrameSize(static_cast<uint32_t>(std::atoi(argv[2])), static_cast<uint32_t>(std::atoi(argv[3])));
        r.changeShadingMode(CRT_MODE_WHITTED);
        r.setOption("max_bounces", std::atoi(argv[4]));
        r.setKeepFloatColour(true);
        r.renderFrame();
        std::vector<float> rays;
        r.cameraRays(rays);
        const size_t n = rays.size() / 8;
        std::vector<crt::Renderer::ShadedHit> hits(n);
        r.shadeRays(rays.data(), n, hits.data());
        static_assert(sizeof(crt::Renderer::ShadedHit) == 56, "nine floats and a RayHit");
        std::ofstream out(argv[5], std::ios::binary);
        out.write(reinterpret_cast<const char*>(r.getFrame().data()), static_cast<std::streamsize>(r.getFrame().size()));
        out.write(reinterpret_cast<const char*>(r.getFloatColour().data()), static_cast<std::streamsize>(r.getFloatColour().size() * sizeof(float)));
        out.write(reinterpret_cast<const char*>(hits.data()), static_cast<std::streamsize>(n * sizeof(crt::Renderer::ShadedHit)));
        std::printf("%zu pixels\n", n);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "whitted_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
