// crt::Renderer's gradient calls from C++ (tests/test_gradients.py::test_cpp_layer):
//   grad_cpp SCENE WIDTH HEIGHT OUT
// Uploads SCENE with dynamic geometry on, traces the WIDTH x HEIGHT pixel-centre camera rays (n records) and writes to OUT:
// traceRaysBackward's grad_rays (8n float32) and grad_xyz (3 per vertex) for the incoming gradients g_t = (i % 7 + 1) / 4 on a hit
// and 0 on a miss, g_uv = ((i % 5 - 2) / 2, (i % 3 - 1) / 4); then closestPointsBackward's grad_points (4n) and grad_xyz for the ray
// origins as points against the hits' surface points (inst, prim, uv) with grad_dist = g_t.
#include "renderer.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s SCENE WIDTH HEIGHT OUT\n", argv[0]);
        return 2;
    }
    try {
        crt::Renderer r;
        r.setDynamicGeometry(true);
        r.prepareForRendering(argv[1], 0);
        r.setFrameSize(static_cast<uint32_t>(std::atoi(argv[2])), static_cast<uint32_t>(std::atoi(argv[3])));
        std::vector<float> rays;
        r.cameraRays(rays);
        const size_t n = rays.size() / 8;
        std::vector<crt::Renderer::RayHit> hits(n);
        r.traceRays(rays.data(), n, hits.data());
        std::vector<float> gT(n), gUv(2 * n), points(4 * n), uv(2 * n);
        std::vector<uint32_t> inst(n), prim(n);
        for (size_t i = 0; i < n; i++) {
            gT[i] = hits[i].inst != CRT_MISS ? static_cast<float>(i % 7 + 1) * 0.25f : 0.0f;
            gUv[2 * i] = (static_cast<float>(i % 5) - 2.0f) * 0.5f;
            gUv[2 * i + 1] = (static_cast<float>(i % 3) - 1.0f) * 0.25f;
            for (int k = 0; k < 3; k++) points[4 * i + k] = rays[8 * i + k];
            points[4 * i + 3] = INFINITY;
            inst[i] = hits[i].inst;
            prim[i] = hits[i].prim;
            uv[2 * i] = hits[i].u;
            uv[2 * i + 1] = hits[i].v;
        }
        std::vector<float> gradRays, gradXyz, gradPoints, gradXyzP;
        r.traceRaysBackward(rays.data(), hits.data(), gT.data(), gUv.data(), n, &gradRays, &gradXyz);
        r.closestPointsBackward(points.data(), inst.data(), prim.data(), uv.data(), gT.data(), n, &gradPoints, &gradXyzP);
        std::ofstream o(argv[4], std::ios::binary);
        for (const std::vector<float>* v : { &gradRays, &gradXyz, &gradPoints, &gradXyzP })
            o.write(reinterpret_cast<const char*>(v->data()), static_cast<std::streamsize>(v->size() * sizeof(float)));
        std::printf("%zu records, %zu vertices\n", n, gradXyz.size() / 3);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "grad_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
