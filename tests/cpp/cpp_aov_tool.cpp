// cpp_aov_tool — drives the C++ mirror's frame AOVs for tests/test_gpu_aov.py.
//   cpp_aov_tool aov <scene> <w> <h> <planes> <x0> <y0> <rw> <rh> <out.bin>
//       Raytracer::render_aov of the rectangle (all zero: the whole frame) of the w x h frame; the
//       requested planes, in bit order and each tightly packed, to out.bin (GPU)
//   cpp_aov_tool layout                                  sizes of the AOV records (no GPU)
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "../../rrte_amd/cpp/examples.hpp"

using namespace rrte_renderer;

template <class T>
static void put(std::ofstream& out, const std::vector<T>& v) {
    out.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    try {
        if (cmd == "layout") {
            std::printf("rrte_aov_desc %zu rrte_aov_buffers %zu\n", sizeof(rrte_aov_desc), sizeof(rrte_aov_buffers));
            return 0;
        }
        if (cmd == "aov" && argc >= 11) {
            const uint32_t w = (uint32_t)std::atoi(argv[3]), h = (uint32_t)std::atoi(argv[4]);
            const uint32_t planes = (uint32_t)std::strtoul(argv[5], nullptr, 0);
            AovRect rect;
            rect.x0 = (uint32_t)std::atoi(argv[6]);
            rect.y0 = (uint32_t)std::atoi(argv[7]);
            rect.width = (uint32_t)std::atoi(argv[8]);
            rect.height = (uint32_t)std::atoi(argv[9]);
            const auto sc = rrte_examples::by_name(argv[2], w, h, Mode::LambertShadow);
            Raytracer rt(sc.config, 0);
            const AovPlanes a = rt.render_aov(sc.objects, sc.camera, planes, rect, sc.lights);
            std::ofstream out(argv[10], std::ios::binary);
            put(out, a.depth);
            put(out, a.prim);
            put(out, a.material);
            put(out, a.tri);
            put(out, a.normal);
            put(out, a.position);
            put(out, a.albedo);
            std::printf("aov %ux%u planes 0x%x frames %llu\n", a.width, a.height, planes,
                        (unsigned long long)rt.stats().frames);
            return 0;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 2;
}
