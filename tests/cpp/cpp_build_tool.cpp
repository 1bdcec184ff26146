// cpp_build_tool — the C++ mirror's mesh build policy for tests/test_gpu_build.py (GPU).
//   cpp_build_tool render <mesh.bin> <w> <h> <out.bin>
// mesh.bin holds one mesh as cpp_instance_tool reads it (u32 vertices, u32 triangles, positions,
// normals, indices).  Raytracer::set_mesh_build with a bad value must throw and change nothing; then
// the scene {ground sphere, the mesh} is rendered under RRTE_MESH_BUILD_DEVICE.  Writes the
// rrte_build_info before the render, the one after it, then the W*H*4 frame.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>

#include "../../include/rrte/rrte_renderer.hpp"

using namespace rrte_renderer;

static std::shared_ptr<Mesh> read_mesh(std::ifstream& in, std::shared_ptr<Material> m) {
    uint32_t n[2] = {0, 0};
    in.read(reinterpret_cast<char*>(n), sizeof n);
    if (!in || n[0] > (1u << 24) || n[1] > (1u << 24)) throw std::runtime_error("bad mesh header");
    std::vector<float> pos(3 * (size_t)n[0]), nrm(3 * (size_t)n[0]);
    std::vector<uint32_t> idx(3 * (size_t)n[1]);
    in.read(reinterpret_cast<char*>(pos.data()), (std::streamsize)(pos.size() * sizeof(float)));
    in.read(reinterpret_cast<char*>(nrm.data()), (std::streamsize)(nrm.size() * sizeof(float)));
    in.read(reinterpret_cast<char*>(idx.data()), (std::streamsize)(idx.size() * sizeof(uint32_t)));
    if (!in) throw std::runtime_error("truncated mesh");
    return std::make_shared<Mesh>(std::move(pos), std::move(idx), std::move(nrm), std::move(m));
}

int main(int argc, char** argv) {
    if (argc < 6 || std::strcmp(argv[1], "render") != 0) return 2;
    try {
        std::ifstream in(argv[2], std::ios::binary);
        if (!in) throw std::runtime_error("cannot open the mesh file");
        const auto mesh = read_mesh(in, std::make_shared<LambertianMaterial>(Color{0.8f, 0.3f, 0.3f, 1.0f}));
        const uint32_t w = (uint32_t)std::atoi(argv[3]), h = (uint32_t)std::atoi(argv[4]);
        RaytracerConfig cfg;
        cfg.max_depth = 1;
        cfg.samples_per_pixel = 1;
        cfg.width = w;
        cfg.height = h;
        cfg.mode = Mode::LambertShadow;
        cfg.jitter = Jitter::Center;
        Camera cam = Camera::new_perspective(rrte_math::to_radians(45.0f), (float)w / (float)h, 0.1f, 100.0f);
        cam.transform.position = Vec3(1.0f, 7.0f, 16.0f);
        cam.look_at(Vec3(1.0f, 1.5f, 0.0f), Vec3(0.0f, 1.0f, 0.0f));
        Objects objs = {std::make_shared<Sphere>(Vec3(0.0f, -1000.0f, 0.0f), 1000.0f,
                                                 std::make_shared<LambertianMaterial>(Color{0.5f, 0.5f, 0.5f, 1.0f})),
                        mesh};
        Lights lights = {std::make_shared<PointLight>(Vec3(-10.0f, 15.0f, 10.0f), Color{1.0f, 1.0f, 1.0f, 1.0f}, 25.0f)};
        std::ofstream out(argv[5], std::ios::binary);
        Raytracer rt(cfg, 0);
        rt.set_jit(RRTE_JIT_OFF);
        try {  // a value that names no policy is refused and changes nothing
            rt.set_mesh_build(2u);
            return 3;
        } catch (const Error&) {
        }
        rt.set_mesh_build(RRTE_MESH_BUILD_DEVICE);
        const rrte_build_info before = rt.build_info();
        const auto frame = rt.render(objs, lights, {}, cam);
        const rrte_build_info after = rt.build_info();
        out.write(reinterpret_cast<const char*>(&before), sizeof before);
        out.write(reinterpret_cast<const char*>(&after), sizeof after);
        out.write(reinterpret_cast<const char*>(frame.data()), (std::streamsize)frame.size());
        return out ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
