// crt::Renderer::windingNumbers / windingMoments from C++ (tests/test_winding.py::test_cpp_layer):
//   winding_cpp SCENE POINTS BETA OUT
// SCENE: a scene file crt_scene_load accepts; POINTS: n x 4 float32 records; OUT: n winding numbers (float32) followed by
// the moment table (32 floats per wide node).
#include "renderer.h"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s SCENE POINTS BETA OUT\n", argv[0]);
        return 2;
    }
    try {
        std::ifstream in(argv[2], std::ios::binary | std::ios::ate);
        const std::streamsize bytes = in.tellg();
        in.seekg(0);
        std::vector<float> points(static_cast<size_t>(bytes) / sizeof(float));
        in.read(reinterpret_cast<char*>(points.data()), bytes);
        const size_t n = points.size() / 4;

        crt::Renderer r;
        r.prepareForRendering(argv[1], 0);
        std::vector<float> w, moments;
        r.windingNumbers(points.data(), n, w, static_cast<float>(std::atof(argv[3])));
        r.windingMoments(moments);
        std::ofstream out(argv[4], std::ios::binary);
        out.write(reinterpret_cast<const char*>(w.data()), static_cast<std::streamsize>(w.size() * sizeof(float)));
        out.write(reinterpret_cast<const char*>(moments.data()), static_cast<std::streamsize>(moments.size() * sizeof(float)));
        std::printf("%zu points, %zu nodes\n", n, moments.size() / 32);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "winding_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
