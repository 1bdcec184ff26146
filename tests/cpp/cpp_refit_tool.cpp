// cpp_refit_tool — the C++ mirror's deforming meshes for tests/test_cpp_refit.py.
//   cpp_refit_tool ir <mesh.bin> <pose.bin> <w> <h> <out.bin>        (no GPU)
//   cpp_refit_tool render <mesh.bin> <pose.bin> <w> <h> <out.bin>    (GPU)
// mesh.bin holds one mesh as cpp_instance_tool reads it (u32 vertices, u32 triangles, positions,
// normals, indices); pose.bin holds 3 * vertices f32: the deformed positions.
//   ir:     Mesh::set_vertices(pose) (normals recomputed), then the lowered IR bytes of {ground sphere,
//           the mesh} and the render parameters, as cpp_mirror_tool ir writes them.
//   render: Raytracer::render of the base pose, set_vertices(pose), Raytracer::render_deformed; writes
//           u64 refits, u64 device_refits, u32 levels, u32 deformed, then the W*H*4 frame.
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
    if (argc < 7) return 2;
    const bool render = std::strcmp(argv[1], "render") == 0;
    if (!render && std::strcmp(argv[1], "ir") != 0) return 2;
    try {
        std::ifstream in(argv[2], std::ios::binary);
        if (!in) throw std::runtime_error("cannot open the mesh file");
        const auto mesh = read_mesh(in, std::make_shared<LambertianMaterial>(Color{0.8f, 0.3f, 0.3f, 1.0f}));
        std::vector<float> pose(mesh->positions.size());
        std::ifstream pin(argv[3], std::ios::binary);
        pin.read(reinterpret_cast<char*>(pose.data()), (std::streamsize)(pose.size() * sizeof(float)));
        if (!pin) throw std::runtime_error("truncated pose");
        const uint32_t w = (uint32_t)std::atoi(argv[4]), h = (uint32_t)std::atoi(argv[5]);
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
        std::ofstream out(argv[6], std::ios::binary);
        try {  // a pose of another vertex count is refused and changes nothing
            mesh->set_vertices(std::vector<float>(pose.size() + 3));
            return 3;
        } catch (const Error&) {
        }
        if (!render) {
            mesh->set_vertices(pose);
            const LoweredScene ls(objs, lights, cam);
            const auto b = ls.bytes();
            const rrte_render_params p = cfg.lower();
            out.write(reinterpret_cast<const char*>(b.data()), (std::streamsize)b.size());
            out.write(reinterpret_cast<const char*>(&p), sizeof p);
            return out ? 0 : 1;
        }
        Raytracer rt(cfg, 0);
        rt.set_jit(RRTE_JIT_OFF);
        rt.render(objs, lights, {}, cam);
        mesh->set_vertices(pose);
        const auto frame = rt.render_deformed(objs, lights, {}, cam);
        const rrte_refit_info ri = rt.refit_info();
        out.write(reinterpret_cast<const char*>(&ri), sizeof ri);
        out.write(reinterpret_cast<const char*>(frame.data()), (std::streamsize)frame.size());
        return out ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
