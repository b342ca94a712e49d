// crt::Renderer::temporalAccumulate from C++ (tests/test_temporal.py::test_cpp_layer):
//   temporal_cpp SCENE WIDTH HEIGHT IN OUT
// SCENE: a scene file crt_scene_load accepts (the renderer wants one; the call itself reads none of it).  IN holds float32
// arrays one after the other, n = WIDTH * HEIGHT: the current camera (12), the previous camera (12), rgb (3n), normal (3n),
// albedo (3n), t (n) and the history records (8n).  OUT receives the new history records (8n) and the accumulated colour (3n),
// with the default parameters.
#include "renderer.h"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <stdexcept>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s SCENE WIDTH HEIGHT IN OUT\n", argv[0]);
        return 2;
    }
    try {
        crt::Renderer r;
        r.prepareForRendering(argv[1], 0);
        r.setFrameSize(static_cast<uint32_t>(std::atoi(argv[2])), static_cast<uint32_t>(std::atoi(argv[3])));
        const size_t n = static_cast<size_t>(r.getFrameWidth()) * r.getFrameHeight();
        std::vector<float> in(24 + 18 * n);
        std::ifstream f(argv[4], std::ios::binary);
        if (!f.read(reinterpret_cast<char*>(in.data()), static_cast<std::streamsize>(in.size() * sizeof(float)))) throw std::runtime_error("short input");
        const float* rgb = in.data() + 24;
        crt::Renderer::Guides g;
        g.normal.assign(rgb + 3 * n, rgb + 6 * n);
        g.albedo.assign(rgb + 6 * n, rgb + 9 * n);
        g.t.assign(rgb + 9 * n, rgb + 10 * n);
        std::vector<float> hist(8 * n), out(3 * n);
        r.temporalAccumulate(in.data(), in.data() + 12, rgb, g, rgb + 10 * n, hist.data(), out.data());
        std::ofstream o(argv[5], std::ios::binary);
        o.write(reinterpret_cast<const char*>(hist.data()), static_cast<std::streamsize>(hist.size() * sizeof(float)));
        o.write(reinterpret_cast<const char*>(out.data()), static_cast<std::streamsize>(out.size() * sizeof(float)));
        std::printf("%zu pixels\n", n);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "temporal_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
