// cpp_instance_tool — the C++ mirror's mesh instances for tests/test_cpp_instances.py (no GPU).
//   cpp_instance_tool ir <meshes.bin> <w> <h> <mode> <out.bin>
// meshes.bin holds the two base meshes of instance_demo, ball then ring, each as
//   u32 vertices, u32 triangles, f32 positions[3 * vertices], f32 normals[3 * vertices], u32 indices[3 * triangles]
// (the normals as given to the Mesh constructor, which normalises them).  Writes the lowered IR bytes
// of rrte_examples::instance_demo and its render parameters, as cpp_mirror_tool ir does.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>

#include "../../rrte_amd/cpp/examples.hpp"

using namespace rrte_renderer;

static std::shared_ptr<Mesh> read_mesh(std::ifstream& in) {
    uint32_t n[2] = {0, 0};
    in.read(reinterpret_cast<char*>(n), sizeof n);
    if (!in || n[0] > (1u << 24) || n[1] > (1u << 24)) throw std::runtime_error("bad mesh header");
    std::vector<float> pos(3 * (size_t)n[0]), nrm(3 * (size_t)n[0]);
    std::vector<uint32_t> idx(3 * (size_t)n[1]);
    in.read(reinterpret_cast<char*>(pos.data()), (std::streamsize)(pos.size() * sizeof(float)));
    in.read(reinterpret_cast<char*>(nrm.data()), (std::streamsize)(nrm.size() * sizeof(float)));
    in.read(reinterpret_cast<char*>(idx.data()), (std::streamsize)(idx.size() * sizeof(uint32_t)));
    if (!in) throw std::runtime_error("truncated mesh");
    return std::make_shared<Mesh>(std::move(pos), std::move(idx), std::move(nrm));
}

int main(int argc, char** argv) {
    if (argc < 7 || std::strcmp(argv[1], "ir") != 0) return 2;
    try {
        std::ifstream in(argv[2], std::ios::binary);
        if (!in) throw std::runtime_error("cannot open the mesh file");
        const auto ball = read_mesh(in);
        const auto ring = read_mesh(in);
        const Mode mode = std::strcmp(argv[5], "refcompat") == 0 ? Mode::RefCompat : Mode::LambertShadow;
        const auto sc = rrte_examples::instance_demo((uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]), mode,
                                                     ball, ring);
        const LoweredScene ls(sc.objects, sc.lights, sc.camera);
        // one Mesh object, one range: the two bases only, however many instances name them
        if (ls.ir().num_mesh_vertices != ball->positions.size() / 3 + ring->positions.size() / 3) return 3;
        const auto b = ls.bytes();
        const rrte_render_params p = sc.config.lower();
        std::ofstream out(argv[6], std::ios::binary);
        out.write(reinterpret_cast<const char*>(b.data()), (std::streamsize)b.size());
        out.write(reinterpret_cast<const char*>(&p), sizeof p);
        return out ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
