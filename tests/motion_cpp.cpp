// crt::Renderer's motion loop from C++ (tests/test_motion.py::test_cpp_layer):
//   motion_cpp SCENE WIDTH HEIGHT MESH TX TY TZ OUT
// Uploads SCENE with dynamic geometry on, renders a mode-3 frame and accumulates it (temporalFrame with motion: no history yet),
// takes the snapshot, translates mesh MESH by (TX, TY, TZ), renders again and writes to OUT, n = WIDTH * HEIGHT: the previous
// points of frameMotion (3n float32) and the float colour temporalFrame(nullptr, true) accumulated (3n).
#include "renderer.h"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 9) {
        std::fprintf(stderr, "usage: %s SCENE WIDTH HEIGHT MESH TX TY TZ OUT\n", argv[0]);
        return 2;
    }
    try {
        const uint32_t mesh = static_cast<uint32_t>(std::atoi(argv[4]));
        const float m[12] = { 1.f, 0.f, 0.f, std::strtof(argv[5], nullptr), 0.f, 1.f, 0.f, std::strtof(argv[6], nullptr),
                              0.f, 0.f, 1.f, std::strtof(argv[7], nullptr) };
        crt::Renderer r;
        r.setDynamicGeometry(true);
        r.prepareForRendering(argv[1], 0);
        r.setFrameSize(static_cast<uint32_t>(std::atoi(argv[2])), static_cast<uint32_t>(std::atoi(argv[3])));
        r.changeShadingMode(3);
        r.setKeepFloatColour(true);
        r.renderFrame();
        r.temporalFrame(nullptr, true);
        r.motionSnapshot();
        r.setMeshTransform(mesh, m);
        r.renderFrame();
        std::vector<float> prevPoint;
        r.frameMotion(prevPoint);
        r.temporalFrame(nullptr, true);
        std::ofstream o(argv[8], std::ios::binary);
        o.write(reinterpret_cast<const char*>(prevPoint.data()), static_cast<std::streamsize>(prevPoint.size() * sizeof(float)));
        o.write(reinterpret_cast<const char*>(r.getFloatColour().data()), static_cast<std::streamsize>(r.getFloatColour().size() * sizeof(float)));
        std::printf("%zu pixels\n", prevPoint.size() / 3);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "motion_cpp: %s\n", e.what());
        return 1;
    }
    return 0;
}
