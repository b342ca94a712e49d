// crt::Renderer::temporalVariance and denoiseVariance from C++ (tests/test_variance.py::test_cpp_layer):
//   variance_cpp SCENE WIDTH HEIGHT IN OUT
// SCENE: a scene file crt_scene_load accepts (the renderer wants one; the calls themselves read none of it).  IN holds float32
// arrays one after the other, n = WIDTH * HEIGHT: the current camera (12), the previous camera (12), rgb (3n), normal (3n),
// albedo (3n), t (n), the history records (8n) and their moments (2n).  OUT receives the new history records (8n), the new
// moments (2n), the variance (n) and the accumulated colour (3n), then that colour filtered with the variance (3n) and the
// filtered variance (n), all with the default parameters.
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
        std::vector<float> in(24 + 20 * n);
        std::ifstream f(argv[4], std::ios::binary);
        if (!f.read(reinterpret_cast<char*>(in.data()), static_cast<std::streamsize>(in.size() * sizeof(float)))) throw std::runtime_error("short input");
        const float* rgb = in.data() + 24;
        crt::Renderer::Guides g;
        g.normal.assign(rgb + 3 * n, rgb + 6 * n);
        g.albedo.assign(rgb + 6 * n, rgb + 9 * n);
        g.t.assign(rgb + 9 * n, rgb + 10 * n);
        std::vector<float> hist(8 * n), mom(2 * n), var(n), out(3 * n), filtered(3 * n), varOut(n);
        r.temporalVariance(in.data(), in.data() + 12, rgb, g, nullptr, rgb + 10 * n, hist.data(), rgb + 18 * n, mom.data(), var.data(), out.data());
        r.denoiseVariance(out.data(), g, var.data(), filtered.data(), varOut.data());
        std::ofstream o(argv[5], std::ios::binary);
        for (const std::vector<float>* v : { &hist, &mom, &var, &out, &filtered, &varOut })
            o.write(reinterpret_cast<const char*>(v->data()), static_cast<std::streamsize>(v->size() * sizeof(float)));
        std::printf("%zu pixels\n", n);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "variance_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
