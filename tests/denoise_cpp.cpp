// crt::Renderer::cameraRays / frameGuides / denoise from C++ (tests/test_denoise.py::test_cpp_layer):
//   denoise_cpp SCENE WIDTH HEIGHT MODE SAMPLE OUT
// SCENE: a scene file crt_scene_load accepts; MODE: the shading mode of the frame.  OUT receives float32 arrays one after the
// other, n = WIDTH * HEIGHT: the pixel-centre camera rays (8n), the camera rays of frame sample SAMPLE (8n), the guides normal
// (3n), albedo (3n), t (n), the frame's float colour (3n) and that colour denoised with the default parameters (3n).
#include "renderer.h"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s SCENE WIDTH HEIGHT MODE SAMPLE OUT\n", argv[0]);
        return 2;
    }
    try {
        crt::Renderer r;
        r.prepareForRendering(argv[1], 0);
        r.setFrameSize(static_cast<uint32_t>(std::atoi(argv[2])), static_cast<uint32_t>(std::atoi(argv[3])));
        r.changeShadingMode(static_cast<uint32_t>(std::atoi(argv[4])));
        const size_t n = static_cast<size_t>(r.getFrameWidth()) * r.getFrameHeight();
        std::vector<float> centre, jittered;
        r.cameraRays(centre);
        r.cameraRays(jittered, static_cast<uint32_t>(std::atoi(argv[5])));
        crt::Renderer::Guides g;
        r.frameGuides(g);
        r.setKeepFloatColour(true);
        r.renderFrame();
        const std::vector<float> rgb = r.getFloatColour();
        std::vector<float> out(3 * n);
        r.denoise(rgb.data(), g, out.data());
        std::ofstream f(argv[6], std::ios::binary);
        const std::vector<float>* const parts[] = { &centre, &jittered, &g.normal, &g.albedo, &g.t, &rgb, &out };
        for (const std::vector<float>* a : parts)
            f.write(reinterpret_cast<const char*>(a->data()), static_cast<std::streamsize>(a->size() * sizeof(float)));
        std::printf("%zu pixels\n", n);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "denoise_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
