// cpp_query_tool — drives the C++ mirror's ray queries for tests/test_gpu_query.py.
//   cpp_query_tool raycast <scene> <rays.bin> <hits.bin> [any]   Raytracer::raycast of the rrte_ray records in
//                                                                rays.bin; the rrte_ray_hit records to hits.bin (GPU)
//   cpp_query_tool pick <scene> <w> <h> <hits.bin>               Raytracer::pick of every pixel, row-major (GPU)
//   cpp_query_tool layout                                        sizes and offsets of the query records (no GPU)
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

#include "../../rrte_amd/cpp/examples.hpp"

using namespace rrte_renderer;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    try {
        if (cmd == "layout") {
            std::printf("rrte_ray %zu rrte_ray_hit %zu hit.material %zu\n", sizeof(rrte_ray), sizeof(rrte_ray_hit),
                        offsetof(rrte_ray_hit, material));
            return 0;
        }
        if (cmd == "raycast" && argc >= 5) {
            const auto sc = rrte_examples::by_name(argv[2], 64, 36, Mode::LambertShadow);
            std::ifstream in(argv[3], std::ios::binary);
            const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            if (raw.empty() || raw.size() % sizeof(rrte_ray)) return 2;
            std::vector<rrte_ray> rays(raw.size() / sizeof(rrte_ray));
            std::memcpy(rays.data(), raw.data(), raw.size());
            Raytracer rt(sc.config, 0);
            const bool any = argc > 5 && std::strcmp(argv[5], "any") == 0;
            const auto hits = rt.raycast(sc.objects, rays, any, sc.lights);
            std::ofstream out(argv[4], std::ios::binary);
            out.write(reinterpret_cast<const char*>(hits.data()), (std::streamsize)(hits.size() * sizeof(rrte_ray_hit)));
            std::printf("raycast %zu rays frames %llu\n", hits.size(), (unsigned long long)rt.stats().frames);
            return 0;
        }
        if (cmd == "pick" && argc >= 6) {
            const uint32_t w = (uint32_t)std::atoi(argv[3]), h = (uint32_t)std::atoi(argv[4]);
            const auto sc = rrte_examples::by_name(argv[2], w, h, Mode::LambertShadow);
            std::vector<std::pair<uint32_t, uint32_t>> px;
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x) px.emplace_back(x, y);
            Raytracer rt(sc.config, 0);
            const auto hits = rt.pick(sc.objects, sc.camera, px, sc.lights);
            std::ofstream out(argv[5], std::ios::binary);
            out.write(reinterpret_cast<const char*>(hits.data()), (std::streamsize)(hits.size() * sizeof(rrte_ray_hit)));
            return 0;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 2;
}
