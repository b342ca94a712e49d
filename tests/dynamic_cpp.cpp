// crt::Renderer with dynamic geometry from C++ (tests/test_dynamic_geometry.py::test_cpp_layer):
//   dynamic_cpp SCENE RAYS OUT MESH TX TY TZ
// Uploads SCENE with dynamic geometry on, translates mesh MESH by (TX, TY, TZ) through setMeshTransform, gives its rest vertices
// again unchanged through updateMeshVertices, traces RAYS (n x 8 float32) and writes n RayHit records (20 bytes).
#include "renderer.h"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s SCENE RAYS OUT MESH TX TY TZ\n", argv[0]);
        return 2;
    }
    try {
        std::ifstream in(argv[2], std::ios::binary | std::ios::ate);
        const std::streamsize bytes = in.tellg();
        in.seekg(0);
        std::vector<float> rays(static_cast<size_t>(bytes) / sizeof(float));
        in.read(reinterpret_cast<char*>(rays.data()), bytes);
        const size_t n = rays.size() / 8;
        const uint32_t mesh = static_cast<uint32_t>(std::atoi(argv[4]));
        const float m[12] = { 1.f, 0.f, 0.f, std::strtof(argv[5], nullptr), 0.f, 1.f, 0.f, std::strtof(argv[6], nullptr),
                              0.f, 0.f, 1.f, std::strtof(argv[7], nullptr) };

        crt::Renderer r;
        r.setDynamicGeometry(true);
        r.prepareForRendering(argv[1], 0);
        r.setMeshTransform(mesh, m);
        // re-giving the rest vertices as they were uploaded changes nothing but goes through the update path
        const crt::Mesh& M = r.getScene().getObjects().at(mesh);
        r.updateMeshVertices(mesh, M.getVertices().data()->data(), M.getVertices().size());
        std::vector<crt::Renderer::RayHit> hits(n);
        r.traceRays(rays.data(), n, hits.data());
        std::ofstream out(argv[3], std::ios::binary);
        out.write(reinterpret_cast<const char*>(hits.data()), static_cast<std::streamsize>(n * sizeof(crt::Renderer::RayHit)));
        std::printf("%zu rays\n", n);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "dynamic_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
