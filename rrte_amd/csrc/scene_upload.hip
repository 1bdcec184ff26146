// scene_upload.hip — from the caller's rrte_scene_ir to the scene version on the device: validation,
// lowering to device records (precomputing the per-object Transform matrices the reference rebuilds
// per ray, primitives.rs:303,421,522,628), the scene key and the mesh cache, and upload_scene with the
// refit and scene-accelerator parts of a version.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.hpp"
#include "sdf_guard.hpp"

using namespace rrte;

namespace {  // (the kernel's symbol stays the one it had inside rrte_hip.hip)

// RRTE_DEBUG bit 2 (diagnostics): the indices of the uploaded scene, checked on the DEVICE copy the
// kernels read (one thread per object, on the upload stream right after the copy): check-
// word bit 16 an object kind out of range, 32 an SDF node range outside the uploaded nodes, 64 a
// CSG-guard link outside its program (it must name a later node of the same program).  The host
// validated the caller's IR (validate); this catches a device copy that differs from it.
__global__ __launch_bounds__(64) void scene_records_check(const DPrim* prims, uint32_t np, const rrte_sdf_node* nodes,
                                                          uint32_t nn, unsigned long long* counters) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= np) return;
    const DPrim& pr = prims[i];
    uint32_t bad = 0u;
    if (pr.kind > RRTE_PRIM_MESH_INSTANCE) {
        bad |= 16u;
    } else if (pr.kind == RRTE_PRIM_SDF) {
        if ((uint64_t)pr.sdf_first + pr.sdf_count > nn) {
            bad |= 32u;
        } else {
            for (uint32_t k = 0; k < pr.sdf_count; ++k) {
                const uint32_t link = nodes[pr.sdf_first + k].i[2];
                if (link != 0u && (link - 1u <= k || link - 1u >= pr.sdf_count)) {
                    bad |= 64u;
                    break;
                }
            }
        }
    }
    if (bad) atomicOr(counters + 1, (unsigned long long)bad);
}

}  // namespace

namespace rrte {

// ---- glam restatement on the host (same algorithms as oracle/, see there) ----
void mat4_srt(const float trs[10], float m[16]) {
    float x = trs[3], y = trs[4], z = trs[5], w = trs[6];
    float x2 = x + x, y2 = y + y, z2 = z + z;
    float xx = x * x2, xy = x * y2, xz = x * z2;
    float yy = y * y2, yz = y * z2, zz = z * z2;
    float wx = w * x2, wy = w * y2, wz = w * z2;
    float sx = trs[7], sy = trs[8], sz = trs[9];
    const float cols[3][3] = {{1.0f - (yy + zz), xy + wz, xz - wy},
                              {xy - wz, 1.0f - (xx + zz), yz + wx},
                              {xz + wy, yz - wx, 1.0f - (xx + yy)}};
    const float sc[3] = {sx, sy, sz};
    for (int c = 0; c < 3; ++c) {
        for (int r = 0; r < 3; ++r) m[c * 4 + r] = cols[c][r] * sc[c];
        m[c * 4 + 3] = 0.0f * sc[c];
    }
    m[12] = trs[0]; m[13] = trs[1]; m[14] = trs[2]; m[15] = 1.0f;
}

// glam Mat4::inverse (glm cofactor form), transform.rs:55-57
static void mat4_inverse(const float* a, float* out) {
    auto M = [a](int c, int r) { return a[c * 4 + r]; };
    const float coef[18] = {
        M(2, 2) * M(3, 3) - M(3, 2) * M(2, 3), M(1, 2) * M(3, 3) - M(3, 2) * M(1, 3),
        M(1, 2) * M(2, 3) - M(2, 2) * M(1, 3), M(2, 1) * M(3, 3) - M(3, 1) * M(2, 3),
        M(1, 1) * M(3, 3) - M(3, 1) * M(1, 3), M(1, 1) * M(2, 3) - M(2, 1) * M(1, 3),
        M(2, 1) * M(3, 2) - M(3, 1) * M(2, 2), M(1, 1) * M(3, 2) - M(3, 1) * M(1, 2),
        M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2), M(2, 0) * M(3, 3) - M(3, 0) * M(2, 3),
        M(1, 0) * M(3, 3) - M(3, 0) * M(1, 3), M(1, 0) * M(2, 3) - M(2, 0) * M(1, 3),
        M(2, 0) * M(3, 2) - M(3, 0) * M(2, 2), M(1, 0) * M(3, 2) - M(3, 0) * M(1, 2),
        M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2), M(2, 0) * M(3, 1) - M(3, 0) * M(2, 1),
        M(1, 0) * M(3, 1) - M(3, 0) * M(1, 1), M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1)};
    // Fac_k = (c_a, c_a, c_b, c_c) in glm's numbering
    const float fac[6][4] = {{coef[0], coef[0], coef[1], coef[2]},     {coef[3], coef[3], coef[4], coef[5]},
                             {coef[6], coef[6], coef[7], coef[8]},     {coef[9], coef[9], coef[10], coef[11]},
                             {coef[12], coef[12], coef[13], coef[14]}, {coef[15], coef[15], coef[16], coef[17]}};
    const float vec[4][4] = {{M(1, 0), M(0, 0), M(0, 0), M(0, 0)},
                             {M(1, 1), M(0, 1), M(0, 1), M(0, 1)},
                             {M(1, 2), M(0, 2), M(0, 2), M(0, 2)},
                             {M(1, 3), M(0, 3), M(0, 3), M(0, 3)}};
    float inv[16];
    for (int i = 0; i < 4; ++i) {
        float sa = (i & 1) ? -1.0f : 1.0f, sb = -sa;
        inv[0 * 4 + i] = ((vec[1][i] * fac[0][i] - vec[2][i] * fac[1][i]) + vec[3][i] * fac[2][i]) * sa;
        inv[1 * 4 + i] = ((vec[0][i] * fac[0][i] - vec[2][i] * fac[3][i]) + vec[3][i] * fac[4][i]) * sb;
        inv[2 * 4 + i] = ((vec[0][i] * fac[1][i] - vec[1][i] * fac[3][i]) + vec[3][i] * fac[5][i]) * sa;
        inv[3 * 4 + i] = ((vec[0][i] * fac[2][i] - vec[1][i] * fac[4][i]) + vec[2][i] * fac[5][i]) * sb;
    }
    float d0 = M(0, 0) * inv[0], d1 = M(0, 1) * inv[4], d2 = M(0, 2) * inv[8], d3 = M(0, 3) * inv[12];
    float det = (d0 + d1) + (d2 + d3);
    float rdet = 1.0f / det;
    for (int i = 0; i < 16; ++i) out[i] = inv[i] * rdet;
}

void to_affine12(const float* m16, float* m12) {
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r) m12[c * 3 + r] = m16[c * 4 + r];
}

static bool sdf_program_ok(const rrte_sdf_node* nodes, uint32_t count) {
    int sp = 0, pp = 0;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t op = nodes[i].op;
        if (op >= RRTE_SDF_SPHERE && op <= RRTE_SDF_ELLIPSOID) {
            if (++sp > RRTE_SDF_MAX_STACK) return false;
        } else if (op >= RRTE_SDF_UNION && op <= RRTE_SDF_SMOOTH_INTERSECTION) {
            if (sp < 2) return false;
            --sp;
        } else if (op >= RRTE_SDF_BEND && op <= RRTE_SDF_WAVE) {
            if (++pp > RRTE_SDF_MAX_POINT_STACK) return false;
            if ((op == RRTE_SDF_BEND || op == RRTE_SDF_TWIST || op == RRTE_SDF_TAPER || op == RRTE_SDF_WAVE) &&
                (nodes[i].i[0] > 2 || nodes[i].i[1] > 2))
                return false;
            if (op == RRTE_SDF_NOISE && nodes[i].i[0] > RRTE_SDF_MAX_OCTAVES) return false;
        } else if (op == RRTE_SDF_POP_POINT) {
            if (pp < 1) return false;
            --pp;
        } else {
            return false;
        }
    }
    return sp == 1 && pp == 0;
}

// The part of validate() that concerns the scene alone (the ray queries validate only this).
rrte_status validate_scene(rrte_ctx* c, const rrte_scene_ir* s) {
    if ((s->num_prims && !s->prims) || (s->num_lights && !s->lights) || (s->num_materials && !s->materials) ||
        (s->num_sdf_nodes && !s->sdf_nodes))
        return fail(c, RRTE_INVALID_ARG, "null array with nonzero count");
    if (s->camera.projection > RRTE_ORTHOGRAPHIC) return fail(c, RRTE_INVALID_ARG, "unknown projection");
    if ((s->num_mesh_vertices && !s->mesh_vertices) || (s->num_mesh_indices && !s->mesh_indices))
        return fail(c, RRTE_INVALID_ARG, "null mesh array with nonzero count");
    if (s->num_mesh_indices % 3) return fail(c, RRTE_INVALID_ARG, "mesh index count not a multiple of 3");
    if (s->num_mesh_indices / 3 >= (1u << 24)) return fail(c, RRTE_INVALID_ARG, "more than 2^24 mesh triangles");
    for (uint32_t i = 0; i < s->num_prims; ++i) {
        const rrte_prim& pr = s->prims[i];
        if (pr.kind > RRTE_PRIM_MESH_INSTANCE)
            return fail(c, RRTE_UNSUPPORTED_PRIM, "prim %u: unknown kind %u", i, pr.kind);
        if (pr.kind == RRTE_PRIM_MESH || pr.kind == RRTE_PRIM_MESH_INSTANCE) {
            if ((uint64_t)pr.sdf_first + pr.sdf_count > s->num_mesh_indices / 3)
                return fail(c, RRTE_INVALID_ARG, "prim %u: mesh triangle range out of bounds", i);
        }
        if (pr.kind == RRTE_PRIM_MESH_INSTANCE) {
            for (int k = 0; k < 10; ++k)
                if (!std::isfinite(pr.trs[k]))
                    return fail(c, RRTE_INVALID_ARG, "prim %u: mesh instance transform is not finite", i);
            if (pr.trs[7] == 0.0f || pr.trs[8] == 0.0f || pr.trs[9] == 0.0f)
                return fail(c, RRTE_INVALID_ARG, "prim %u: mesh instance scale has a zero component", i);
        }
        if (pr.kind == RRTE_PRIM_SDF) {
            if ((uint64_t)pr.sdf_first + pr.sdf_count > s->num_sdf_nodes)
                return fail(c, RRTE_INVALID_ARG, "prim %u: SDF node range out of bounds", i);
            if (!sdf_program_ok(s->sdf_nodes + pr.sdf_first, pr.sdf_count))
                return fail(c, RRTE_INVALID_ARG, "prim %u: malformed SDF program", i);
        }
    }
    for (uint32_t i = 0; i < s->num_lights; ++i)
        if (s->lights[i].kind > RRTE_LIGHT_AMBIENT)
            return fail(c, RRTE_UNSUPPORTED_PRIM, "light %u: unknown kind %u", i, s->lights[i].kind);
    for (uint32_t i = 0; i < s->num_materials; ++i)
        if (s->materials[i].kind > RRTE_MAT_EMISSIVE)
            return fail(c, RRTE_UNSUPPORTED_PRIM, "material %u: unknown kind %u", i, s->materials[i].kind);
    return RRTE_OK;
}

rrte_status validate(rrte_ctx* c, const rrte_scene_ir* s, const rrte_render_params* p) {
    if (!s || !p) return fail(c, RRTE_INVALID_ARG, "null scene or params");
    if (p->width == 0 || p->height == 0) return fail(c, RRTE_INVALID_ARG, "zero-sized frame %ux%u", p->width, p->height);
    if ((uint64_t)p->width * p->height > (1ull << 30)) return fail(c, RRTE_INVALID_ARG, "frame too large");
    if (p->samples_per_pixel == 0) return fail(c, RRTE_INVALID_ARG, "samples_per_pixel must be >= 1");
    if (p->mode > RRTE_MODE_LAMBERT_SHADOW) return fail(c, RRTE_INVALID_ARG, "unknown mode %u", p->mode);
    if (p->jitter > RRTE_JITTER_RANDOM) return fail(c, RRTE_INVALID_ARG, "unknown jitter %u", p->jitter);
    // (the high bits are the library's own per-launch flags, kFlagSlabRgb24 / kFlagHostStore)
    if (p->flags & ~(uint32_t)(RRTE_FLAG_F32_LINEAR | RRTE_FLAG_GATHER_OVERLAP))
        return fail(c, RRTE_INVALID_ARG, "unknown flags 0x%x", p->flags);
    return validate_scene(c, s);
}

// Conservative world-space bounding sphere of one object for wave culling
// (cull.hpp, shadow_cull): every point the object's
// intersector can report lies inside it.  Radius +inf = never culled (planes,
// non-finite data).  Computed in double and inflated, so f32 rounding in the
// intersectors stays inside.
static float4 prim_bound(const rrte_prim& in, const DPrim& d) {
    const double inf = __builtin_huge_val();
    double c[3] = {in.p[0], in.p[1], in.p[2]}, r = inf;
    bool local = true;  // bound given in object space (transformed below)
    switch (in.kind) {
    case RRTE_PRIM_SPHERE: r = fabs((double)in.p[3]); local = false; break;
    case RRTE_PRIM_TRIANGLE: {
        for (int k = 0; k < 3; ++k) c[k] = ((double)in.p[k] + in.p[3 + k] + in.p[6 + k]) / 3.0;
        r = 0.0;
        for (int v = 0; v < 3; ++v) {
            double dx = in.p[3 * v] - c[0], dy = in.p[3 * v + 1] - c[1], dz = in.p[3 * v + 2] - c[2];
            r = fmax(r, sqrt(dx * dx + dy * dy + dz * dz));
        }
        local = false;
        break;
    }
    case RRTE_PRIM_CUBE: {
        double sx = in.p[4], sy = in.p[5], sz = in.p[6];
        r = 0.5 * sqrt(sx * sx + sy * sy + sz * sz);
        break;
    }
    case RRTE_PRIM_CYLINDER:
    case RRTE_PRIM_CONE: {
        double rad = in.p[3], hh = 0.5 * in.p[4];
        r = sqrt(rad * rad + hh * hh);
        break;
    }
    case RRTE_PRIM_CAPSULE: r = 0.5 * fabs((double)in.p[4]) + fabs((double)in.p[3]); break;
    case RRTE_PRIM_SDF: r = fabs((double)in.p[3]); local = false; break;  // the sphere tracer's own bound
    default: break;                                                       // plane: unbounded
    }
    return sphere_bound(c, r, local ? d.xf : nullptr);  // (bvh.hip; mesh objects get theirs from assign_mesh_prims)
}

// Lower the ABI records to device records (matrices precomputed once per
// object instead of per ray as in primitives.rs:303,421,522,628).
void lower_scene(const rrte_scene_ir* s, std::vector<DPrim>& prims, std::vector<DMaterial>& mats,
                 std::vector<DLight>& lights, std::vector<float4>* bounds) {
    prims.assign(s->num_prims, DPrim{});
    if (bounds) bounds->assign(s->num_prims, float4{});
    for (uint32_t i = 0; i < s->num_prims; ++i) {
        const rrte_prim& in = s->prims[i];
        DPrim& o = prims[i];
        memset(&o, 0, sizeof o);
        o.kind = in.kind;
        o.material = in.material;
        o.sdf_first = in.sdf_first;
        o.sdf_count = in.sdf_count;
        o.sdf_max_steps = in.sdf_max_steps;
        o.sdf_step_scale = in.sdf_step_scale;
        o.sdf_hit_eps = in.sdf_hit_eps;
        memcpy(o.p, in.p, sizeof o.p);
        float m[16], inv[16];
        mat4_srt(in.trs, m);
        mat4_inverse(m, inv);
        to_affine12(m, o.xf);
        to_affine12(inv, o.inv);
        if (bounds) (*bounds)[i] = prim_bound(in, o);
    }
    mats.assign(s->num_materials, DMaterial{});
    for (uint32_t i = 0; i < s->num_materials; ++i) {
        static_assert(sizeof(rrte_material) == sizeof(DMaterial), "material layout");
        memcpy(&mats[i], &s->materials[i], sizeof(DMaterial));
    }
    lights.assign(s->num_lights, DLight{});
    for (uint32_t i = 0; i < s->num_lights; ++i) {
        const rrte_light& in = s->lights[i];
        DLight& o = lights[i];
        memset(&o, 0, sizeof o);
        o.kind = in.kind;
        o.intensity = in.intensity;
        o.range = in.range;
        o.linear = in.linear;
        o.quadratic = in.quadratic;
        o.inner_angle = in.inner_angle;
        o.outer_angle = in.outer_angle;
        memcpy(o.position, in.position, sizeof o.position);
        memcpy(o.direction, in.direction, sizeof o.direction);
        memcpy(o.color, in.color, sizeof o.color);
        for (int k = 0; k < 4; ++k) o.cI[k] = in.color[k] * in.intensity;  // Color * f32 (light.rs:189)
    }
}

// Upload the scene if it differs from the cached copy (the analogue of
// caching on Scene::is_dirty, crates/rrte-scene/src/lib.rs:310-312).  The key
// is the IR's bytes; mesh arrays enter it through (addresses, counts,
// mesh_version), or by content when mesh_version is 0.
struct MeshKey {
    const void* v;
    const void* i;
    uint64_t nv, ni, version;
};

// The key parts of a scene IR (compared byte for byte against the cached scene's key).  The parts from
// kKeyMesh on are the mesh identity: the mesh cache's key (mesh_cache_hit).
enum KeyPart { kKeyPrims, kKeyMaterials, kKeyLights, kKeyNodes, kKeyMesh, kKeyMeshVertices, kKeyMeshIndices, kKeyCount };
struct SceneKeyParts {
    const void* parts[kKeyCount];
    size_t lens[kKeyCount];
    size_t total;
    MeshKey mk;
};
static void scene_key_parts(const rrte_scene_ir* s, SceneKeyParts& kp) {
    kp.mk = MeshKey{s->mesh_vertices, s->mesh_indices, s->num_mesh_vertices, s->num_mesh_indices, s->mesh_version};
    const size_t bmv = s->mesh_version ? 0 : sizeof(rrte_mesh_vertex) * s->num_mesh_vertices;
    const size_t bmi = s->mesh_version ? 0 : sizeof(uint32_t) * s->num_mesh_indices;
    const void* parts[kKeyCount] = {s->prims, s->materials, s->lights, s->sdf_nodes, &kp.mk, s->mesh_vertices, s->mesh_indices};
    const size_t lens[kKeyCount] = {sizeof(rrte_prim) * s->num_prims, sizeof(rrte_material) * s->num_materials,
                            sizeof(rrte_light) * s->num_lights, sizeof(rrte_sdf_node) * s->num_sdf_nodes,
                            sizeof(MeshKey), bmv, bmi};
    kp.total = 0;
    for (int i = 0; i < kKeyCount; ++i) {
        kp.parts[i] = parts[i];
        kp.lens[i] = lens[i];
        kp.total += lens[i];
    }
}

// True if `s` is the scene cached on the device (no upload needed).
static bool scene_same(const rrte_ctx* c, const rrte_scene_ir* s) {
    SceneKeyParts kp;
    scene_key_parts(s, kp);
    if (c->scene_key.size() != kp.total) return false;
    const unsigned char* k = c->scene_key.data();
    for (int i = 0; i < kKeyCount; ++i) {
        if (kp.lens[i] && memcmp(k, kp.parts[i], kp.lens[i])) return false;
        k += kp.lens[i];
    }
    return true;
}

// The scene's topology -- what a topology kernel compiles in (jit.hip, scene_view.hpp TopoPrim /
// TopoNode / TopoLight) -- as a key, with its structural decisions in `topo`: object kinds and SDF
// node ranges, node ops and integer arguments (CSG-guard links included), light kinds, per-object
// SDF convexity (value-dependent for cones) and per-light cullability.  Also stores each SDF
// program's leaf scale (sdf_leaf_scale, the secant exit's error bound) in its first node's spare
// slot f[11], where a topology kernel reads it; no other code reads f[11].
std::string topology_of(const std::vector<DPrim>& prims, const std::vector<DLight>& lights,
                        std::vector<rrte_sdf_node>& nodes, JitTopo& topo) {
    std::string key;
    auto put = [&](uint32_t v) { key.append(reinterpret_cast<const char*>(&v), sizeof v); };
    put((uint32_t)prims.size());
    put((uint32_t)lights.size());
    put((uint32_t)nodes.size());
    topo.convex.assign(prims.size(), 0);
    topo.cullable.assign(lights.size(), 0);
    for (size_t i = 0; i < prims.size(); ++i) {
        const DPrim& p = prims[i];
        put(p.kind);
        put(p.sdf_first);
        put(p.sdf_count);
        if (p.kind == RRTE_PRIM_SDF && p.sdf_count && (size_t)p.sdf_first + p.sdf_count <= nodes.size()) {
            topo.convex[i] = sdf_convex(&nodes[p.sdf_first], p.sdf_count) ? 1 : 0;
            nodes[p.sdf_first].f[11] = sdf_leaf_scale(&nodes[p.sdf_first], p.sdf_count);
        }
        put(topo.convex[i]);
    }
    for (const rrte_sdf_node& n : nodes) {
        put(n.op);
        put(n.i[0]);
        put(n.i[1]);
        put(n.i[2]);
    }
    for (size_t i = 0; i < lights.size(); ++i) {
        topo.cullable[i] = light_record_cullable(lights[i]) ? 1 : 0;
        put(lights[i].kind);
        put(topo.cullable[i]);
    }
    return key;
}

// The features of a scene (kFeat*) that pick its generic kernel variant.
static uint32_t scene_features(const std::vector<DPrim>& prims, const std::vector<rrte_sdf_node>& nodes) {
    uint32_t f = 0u;
    for (const DPrim& p : prims) {
        if (p.kind == RRTE_PRIM_MESH) f |= kFeatMesh;
        else if (p.kind == RRTE_PRIM_MESH_INSTANCE) f |= kFeatMesh | kFeatInstance;
        else if (p.kind == RRTE_PRIM_SDF) f |= kFeatSdf;
        else if (p.kind != RRTE_PRIM_SPHERE) f |= kFeatAnalytic;
    }
    for (const rrte_sdf_node& n : nodes)
        if (n.op >= 64u) f |= kFeatDeform;  // deformers and their point pops
    return f;
}

// True if the context's mesh data (rrte_ctx::mesh_cache) was built from the mesh arrays of `s` (kp: its
// key parts; the mesh identity is the parts from kKeyMesh on) for exactly the ranges the objects of `s` name.
static bool mesh_cache_hit(const rrte_ctx* c, const SceneKeyParts& kp, const rrte_scene_ir* s) {
    if (!c->mesh_cache_valid) return false;
    if (c->mesh_cache_key.size() != kp.lens[kKeyMesh] + kp.lens[kKeyMeshVertices] + kp.lens[kKeyMeshIndices]) return false;
    const unsigned char* k = c->mesh_cache_key.data();
    for (int i = kKeyMesh; i < kKeyCount; ++i) {
        if (kp.lens[i] && memcmp(k, kp.parts[i], kp.lens[i])) return false;
        k += kp.lens[i];
    }
    std::vector<std::pair<uint32_t, uint32_t>> want = mesh_ranges_of(s), have;
    for (const MeshRange& m : c->mesh_cache.ranges) have.emplace_back(m.first, m.count);
    std::sort(want.begin(), want.end());
    std::sort(have.begin(), have.end());
    return want == have;
}

static void set_mesh_cache_key(rrte_ctx* c, const SceneKeyParts& kp) {
    c->mesh_cache_key.clear();
    for (int i = kKeyMesh; i < kKeyCount; ++i)
        c->mesh_cache_key.insert(c->mesh_cache_key.end(), static_cast<const unsigned char*>(kp.parts[i]),
                                 static_cast<const unsigned char*>(kp.parts[i]) + kp.lens[i]);
}

// Policy DEVICE on a mesh-cache miss: the LBVH build (mesh_build.hip) on the upload stream into
// `built`.  *done = false when the host builder must take this miss (counted by the caller).
static rrte_status build_meshes_device(rrte_ctx* c, const rrte_scene_ir* s, MeshData& built, bool* done) {
    *done = false;
    const auto t0 = std::chrono::steady_clock::now();
    const bool planned = c->builder.plan(s);
    if (c->env.host_prof)  // (a refused plan has paid for its scan too)
        c->build_times.host_scan += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (!planned) return RRTE_OK;
    rrte_status r;
    if ((r = ensure(c, c->d_build, c->builder.scratch_bytes())) != RRTE_OK) return r;
    uint32_t depth = 0;
    hipError_t err = hipSuccess;
    const BuildResult br = c->builder.run(s, c->d_build, c->upload_stream, (c->env.debug & 4u) ? c->d_counters + 1 : nullptr,
                                          built, &depth, &err, c->env.host_prof ? &c->build_times : nullptr);
    if (br == BuildResult::HipError) HIPCHK(c, err);
    if (br != BuildResult::Built) {
        built = MeshData{};
        return RRTE_OK;
    }
    c->build_depth = depth;
    *done = true;
    return RRTE_OK;
}

rrte_status upload_scene(rrte_ctx* c, const rrte_scene_ir* s, hipStream_t st, double* upload_ms) {
    const size_t bn = sizeof(rrte_sdf_node) * s->num_sdf_nodes;
    SceneKeyParts kparts;
    scene_key_parts(s, kparts);
    const size_t key_len = kparts.total;
    const bool same = scene_same(c, s) && !c->accel_dirty;
    if (!same && c->batch.rendered < c->batch.n) {
        // the open batch's frames render the cached scene: launch them before the scene changes.  Local
        // only (no gather): a rank's own preview render with another scene must not close a batch the
        // other ranks keep open
        rrte_status r = render_batch(c, false);
        if (r != RRTE_OK) return r;
    }
    *upload_ms = 0.0;
    if (same) {
        ++c->same_scene_renders;
        return RRTE_OK;
    }
    (void)st;  // the copy runs on the context's upload stream; launches wait for its event (issue_launch)
    const auto t_up0 = std::chrono::steady_clock::now();
    auto t_sec = t_up0;
    auto lap_up = [&](int i) {  // (RRTE_HOST_PROFILE)
        if (!c->env.host_prof) return;
        const auto n = std::chrono::steady_clock::now();
        c->hpu[i] += std::chrono::duration<double, std::micro>(n - t_sec).count();
        t_sec = n;
    };

    for (uint32_t k = 0; k < s->num_mesh_indices; ++k)
        if (s->mesh_indices[k] >= s->num_mesh_vertices)
            return fail(c, RRTE_INVALID_ARG, "mesh index %u out of range (%u vertices)", k, s->num_mesh_vertices);
    std::vector<DPrim> prims;
    std::vector<DMaterial> mats;
    std::vector<DLight> lights;
    std::vector<float4> bounds;
    lower_scene(s, prims, mats, lights, &bounds);
    lap_up(0);
    // Mesh cache: the mesh data is rebuilt only when the mesh arrays (scene_key_parts' identity) or the
    // set of ranges the objects name changed; otherwise the last built data is copied into this
    // scene version as it is (moving an instance, or anything else in the scene, builds no BVH)
    if (!mesh_cache_hit(c, kparts, s)) {
        MeshData built;
        bool on_device = false;
        if (c->mesh_build == RRTE_MESH_BUILD_DEVICE) {
            rrte_status br = build_meshes_device(c, s, built, &on_device);
            if (br != RRTE_OK) return br;
            if (on_device) c->device_builds += built.ranges.size();
            else ++c->host_fallbacks;
        }
        if (!on_device) build_mesh_ranges(s, built);
        if (built.too_deep) return fail(c, RRTE_UNSUPPORTED_PRIM, "mesh BVH deeper than the traversal stack");
        c->bvh_builds += built.ranges.size();
        c->mesh_cache = std::move(built);
        set_mesh_cache_key(c, kparts);
        c->mesh_cache_indices.assign(s->mesh_indices, s->mesh_indices + s->num_mesh_indices);
        c->mesh_cache_valid = true;
        c->mesh_deformed = false;  // (a real build: the records are these vertices')
        c->refit_static_valid = false;
    }
    const MeshData& md = c->mesh_cache;
    // A deformed cache (rrte_hip_mesh_refit): md's records are stale; this version is refitted on the
    // device from the scene's vertices, behind the copy (below)
    const bool refit = c->mesh_deformed && c->refit_static_valid && !md.tris.empty();
    const RefitStatic& rs = c->refit_static;
    assign_mesh_prims(s, md, prims.data(), bounds.data());
    // The scene accelerator: one tree per scene version over the culling spheres (the mesh objects have
    // theirs by now); a scene that meets the policy and min_prims but cannot be accelerated takes the
    // default path (counted)
    AccelTree atree;
    const bool accel_wanted = c->accel_policy == RRTE_SCENE_ACCEL_ON && s->num_prims >= c->accel_min;
    const bool accel_built = accel_wanted && accel_build(reinterpret_cast<const float*>(bounds.data()), s->num_prims,
                                                         kAccelStack, atree) == AccelBuild::Built;
    lap_up(1);
    // SDF programs with their exact CSG early-outs (sdf_guard.hpp); the key above stays the caller's IR
    std::vector<rrte_sdf_node> nodes = decorate_scene_sdf(s, c->env.guard_leaves);
    lap_up(2);
    JitTopo topo;
    std::string tkey = topology_of(prims, lights, nodes, topo);
    lap_up(3);

    // Frames in flight keep reading the current version: retire it and upload into the next version
    // of the ring once the frames that read THAT one have completed (normally long ago: a wait here
    // means more scene changes than versions within the frames in flight; bounded, like every wait
    // that may sit behind a gather)
    rrte_status r;
    if (c->sb_cur >= 0 && (r = c->sb[c->sb_cur].ver.retire(c)) != RRTE_OK) return r;
    const int nx = (c->sb_cur + 1) % rrte_ctx::kSceneVersions;
    rrte_ctx::SceneBuf& B = c->sb[nx];
    if ((r = B.ver.wait_retired(c)) != RRTE_OK) return r;
    c->same_scene_renders = 0;
    ++c->scene_gen;
    c->sb_cur = -1;  // (until the upload has completed: a failure below leaves no current version)
    c->scene_key.clear();
    // one allocation, one staging buffer, one copy (256-B aligned sub-arrays)
    // The parts of a scene version, in the order they lie in its one allocation.  kPartRefit*: the
    // refit's inputs (empty unless this version is refitted); kPartAccel*: the scene accelerator's
    // records, leaf entries and always-mask (empty unless this version is accelerated)
    enum {
        kPartPrims, kPartMaterials, kPartLights, kPartNodes, kPartBounds,
        kPartMeshNodes, kPartMeshTris, kPartMeshNorms, kPartMeshPerm,
        kPartRefitVerts, kPartRefitSlotVtx, kPartRefitLeaves, kPartRefitOrder,
        kPartAccelNodes, kPartAccelLeafPrims, kPartAccelAlways,
        kPartCount
    };
    struct Part { const void* src; size_t bytes; size_t off; };
    Part parts[kPartCount] = {};
    parts[kPartPrims] = {prims.data(), prims.size() * sizeof(DPrim), 0};
    parts[kPartMaterials] = {mats.data(), mats.size() * sizeof(DMaterial), 0};
    parts[kPartLights] = {lights.data(), lights.size() * sizeof(DLight), 0};
    parts[kPartNodes] = {nodes.data(), bn, 0};
    parts[kPartBounds] = {bounds.data(), bounds.size() * sizeof(float4), 0};
    parts[kPartMeshNodes] = {md.nodes.data(), md.nodes.size() * sizeof(float4), 0};
    parts[kPartMeshTris] = {md.tris.data(), md.tris.size() * sizeof(float4), 0};
    parts[kPartMeshNorms] = {md.norms.data(), md.norms.size() * sizeof(float4), 0};
    parts[kPartMeshPerm] = {md.perm.data(), md.perm.size() * sizeof(uint32_t), 0};
    parts[kPartRefitVerts] = {s->mesh_vertices, refit ? s->num_mesh_vertices * sizeof(rrte_mesh_vertex) : 0, 0};
    parts[kPartRefitSlotVtx] = {rs.slot_vtx.data(), refit ? rs.slot_vtx.size() * sizeof(uint32_t) : 0, 0};
    parts[kPartRefitLeaves] = {rs.leaves.data(), refit ? rs.leaves.size() * sizeof(uint2) : 0, 0};
    parts[kPartRefitOrder] = {rs.order.data(), refit ? rs.order.size() * sizeof(uint2) : 0, 0};
    parts[kPartAccelNodes] = {atree.nodes.data(), atree.nodes.size() * sizeof(float), 0};
    parts[kPartAccelLeafPrims] = {atree.leaf_prims.data(), atree.leaf_prims.size() * sizeof(uint32_t), 0};
    parts[kPartAccelAlways] = {atree.always.data(), atree.always.size() * sizeof(uint32_t), 0};
    lap_up(4);
    size_t total = 0;
    for (Part& pt : parts) {
        pt.off = total;
        total += (pt.bytes + 255u) & ~(size_t)255u;
    }
    total = std::max<size_t>(total, 256u);
    // the staging buffer may still feed this version's previous upload if no launch ever read it
    if (B.ver.ev_up) HIPCHK(c, hipEventSynchronize(B.ver.ev_up));  // (upload stream: copies only, bounded)
    if ((r = ensure(c, B.d_buf, total)) != RRTE_OK) return r;
    HIPCHK(c, B.h_stage.grow(total));  // (its copies have completed: ev_up above)
    HIPCHK(c, B.ver.ev_up.create());
    for (const Part& pt : parts)
        if (pt.bytes) memcpy(B.h_stage + pt.off, pt.src, pt.bytes);
    lap_up(5);
    hipStream_t us = c->upload_stream;  // (created with the context)
    // fault injection for the check below (RRTE_FAULT_BAD_SLOT=2 with RRTE_DEBUG bit 2): object 0's
    // kind out of range in the device copy only (kernels skip an unknown kind; the host copy stays valid)
    if (c->env.fault_bad_slot == 2 && (c->env.debug & 4u) && !prims.empty())
        reinterpret_cast<DPrim*>(B.h_stage + parts[kPartPrims].off)->kind = 0xbadu;
    HIPCHK(c, hipMemcpyAsync(B.d_buf, B.h_stage, total, hipMemcpyHostToDevice, us));
    lap_up(6);
    if ((c->env.debug & 4u) && !prims.empty()) {
        hipLaunchKernelGGL(scene_records_check, dim3(((uint32_t)prims.size() + 63u) / 64u), dim3(64), 0, us,
                           reinterpret_cast<const DPrim*>(B.d_buf + parts[kPartPrims].off), (uint32_t)prims.size(),
                           reinterpret_cast<const rrte_sdf_node*>(B.d_buf + parts[kPartNodes].off), (uint32_t)nodes.size(),
                           c->d_counters);
        HIPCHK(c, hipGetLastError());
    }
    if (refit) {  // on the upload stream: launches wait for ev_up, frames in flight read other versions
        RefitDevice rd{};
        rd.nodes = reinterpret_cast<float4*>(B.d_buf + parts[kPartMeshNodes].off);
        rd.tris = reinterpret_cast<float4*>(B.d_buf + parts[kPartMeshTris].off);
        rd.norms = reinterpret_cast<float4*>(B.d_buf + parts[kPartMeshNorms].off);
        rd.verts = reinterpret_cast<const float2*>(B.d_buf + parts[kPartRefitVerts].off);
        rd.slot_vtx = reinterpret_cast<const uint32_t*>(B.d_buf + parts[kPartRefitSlotVtx].off);
        rd.leaves = reinterpret_cast<const uint2*>(B.d_buf + parts[kPartRefitLeaves].off);
        rd.order = reinterpret_cast<const uint2*>(B.d_buf + parts[kPartRefitOrder].off);
        rd.n_verts = s->num_mesh_vertices;
        rd.n_slots = (uint32_t)(md.tris.size() / 3);
        rd.n_recs = (uint32_t)(md.nodes.size() / 4);
        rd.check = (c->env.debug & 4u) ? c->d_counters + 1 : nullptr;
        HIPCHK(c, launch_refit(rs, rd, us));
        ++c->device_refits;
    }
    HIPCHK(c, B.ver.published(us));
    lap_up(7);
    // host time to lower the scene and enqueue its upload (the copy itself is asynchronous)
    *upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up0).count();
    uint8_t* d = B.d_buf;
    c->d_prims = reinterpret_cast<DPrim*>(d + parts[kPartPrims].off);
    c->d_mats = reinterpret_cast<DMaterial*>(d + parts[kPartMaterials].off);
    c->d_lights = reinterpret_cast<DLight*>(d + parts[kPartLights].off);
    c->d_nodes = reinterpret_cast<rrte_sdf_node*>(d + parts[kPartNodes].off);
    c->d_bounds = reinterpret_cast<float4*>(d + parts[kPartBounds].off);
    c->mesh_view = MeshView{reinterpret_cast<float4*>(d + parts[kPartMeshNodes].off), reinterpret_cast<float4*>(d + parts[kPartMeshTris].off),
                            reinterpret_cast<float4*>(d + parts[kPartMeshNorms].off), reinterpret_cast<uint32_t*>(d + parts[kPartMeshPerm].off)};
    c->accel_dirty = false;
    if (accel_built) ++c->accel_builds;  // (counted once the version is current: a failed upload built nothing)
    else if (accel_wanted) ++c->accel_fallbacks;
    c->accel_on = accel_built;
    c->accel = AccelView{};
    c->accel_nodes = c->accel_depth = c->accel_bounded = c->accel_unbounded = 0u;
    if (accel_built) {
        c->accel = AccelView{reinterpret_cast<const float4*>(d + parts[kPartAccelNodes].off),
                             reinterpret_cast<const uint32_t*>(d + parts[kPartAccelLeafPrims].off),
                             reinterpret_cast<const uint32_t*>(d + parts[kPartAccelAlways].off), nullptr, atree.always_groups,
                             atree.root, (uint32_t)atree.always.size(), atree.group_shift, s->num_prims};
        c->accel_nodes = (uint32_t)(atree.nodes.size() / 16u);
        c->accel_depth = atree.depth;
        c->accel_bounded = atree.bounded;
        c->accel_unbounded = atree.unbounded;
    }
    c->sb_cur = nx;
    c->h_prims = prims;
    c->h_bounds = bounds;
    c->h_mats = mats;
    c->h_lights = lights;
    c->h_nodes = std::move(nodes);
    c->scene_feat = scene_features(c->h_prims, c->h_nodes);
    c->value_edits = (!c->topo_key.empty() && tkey == c->topo_key) ? c->value_edits + 1 : 0;
    c->topo_key = std::move(tkey);
    c->topo = std::move(topo);
    c->n_prims = s->num_prims;
    c->n_mats = s->num_materials;
    c->n_lights = s->num_lights;
    c->n_nodes = s->num_sdf_nodes;
    c->scene_key.resize(key_len);
    unsigned char* k = c->scene_key.data();
    for (int i = 0; i < kKeyCount; ++i) {
        if (kparts.lens[i]) memcpy(k, kparts.parts[i], kparts.lens[i]);
        k += kparts.lens[i];
    }
    lap_up(8);
    c->hpu_n += c->env.host_prof;
    return RRTE_OK;
}

}  // namespace rrte

extern "C" {

// include/rrte_hip_refit.h
rrte_status rrte_hip_mesh_refit(rrte_ctx* c, const rrte_scene_ir* s) {
    if (!c || !s) return RRTE_INVALID_ARG;
    if ((s->num_mesh_vertices && !s->mesh_vertices) || (s->num_mesh_indices && !s->mesh_indices))
        return fail(c, RRTE_INVALID_ARG, "mesh refit: null mesh array");
    if (!c->mesh_cache_valid || c->mesh_cache_key.size() < sizeof(MeshKey))
        return fail(c, RRTE_INVALID_ARG, "mesh refit: no mesh data to refit (nothing built yet)");
    MeshKey have;
    memcpy(&have, c->mesh_cache_key.data(), sizeof have);
    if (have.nv != s->num_mesh_vertices)
        return fail(c, RRTE_INVALID_ARG, "mesh refit: vertex count %u differs from the built %u", s->num_mesh_vertices, (uint32_t)have.nv);
    if (have.ni != s->num_mesh_indices || c->mesh_cache_indices.size() != s->num_mesh_indices)
        return fail(c, RRTE_INVALID_ARG, "mesh refit: index count %u differs from the built %u", s->num_mesh_indices, (uint32_t)have.ni);
    if (s->num_mesh_indices && memcmp(c->mesh_cache_indices.data(), s->mesh_indices, sizeof(uint32_t) * s->num_mesh_indices))
        return fail(c, RRTE_INVALID_ARG, "mesh refit: an index value differs from the built indices (topology change)");
    {
        std::vector<std::pair<uint32_t, uint32_t>> want = mesh_ranges_of(s), got;
        for (const MeshRange& m : c->mesh_cache.ranges) got.emplace_back(m.first, m.count);
        std::sort(want.begin(), want.end());
        std::sort(got.begin(), got.end());
        if (want != got) return fail(c, RRTE_INVALID_ARG, "mesh refit: the scene's triangle ranges differ from the built ones");
    }
    for (uint32_t v = 0; v < s->num_mesh_vertices; ++v) {
        const float* p = s->mesh_vertices[v].position;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
            return fail(c, RRTE_INVALID_ARG, "mesh refit: vertex %u has a non-finite position", v);
    }
    if (!c->refit_static_valid) {  // first refit of this topology
        RefitStatic rs;
        if (!build_refit_static(c->mesh_cache, c->mesh_cache_indices.data(), (uint32_t)c->mesh_cache_indices.size(), rs))
            return fail(c, RRTE_INVALID_ARG, "mesh refit: the stored mesh data does not describe trees over its triangles");
        c->refit_static = std::move(rs);
        c->refit_static_valid = true;
    }
    refit_range_bounds(s, c->mesh_cache);
    SceneKeyParts kp;
    scene_key_parts(s, kp);
    set_mesh_cache_key(c, kp);
    c->mesh_deformed = true;
    ++c->refits;
    return RRTE_OK;
}

rrte_status rrte_hip_mesh_nodes(rrte_ctx* c, void* out, size_t bytes, uint32_t* records) {
    if (!c || !records || (bytes && !out)) return RRTE_INVALID_ARG;
    *records = 0;
    if (c->sb_cur < 0 || !c->mesh_cache_valid) return RRTE_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const rrte_ctx::SceneBuf& B = c->sb[c->sb_cur];
    const size_t all = c->mesh_cache.nodes.size() * sizeof(float4);
    *records = (uint32_t)(c->mesh_cache.nodes.size() / 4);
    const size_t n = std::min(bytes, all);
    if (!n) return RRTE_OK;
    if (B.ver.ev_up) HIPCHK(c, hipEventSynchronize(B.ver.ev_up));
    HIPCHK(c, hipMemcpy(out, c->mesh_view.nodes, n, hipMemcpyDeviceToHost));
    return RRTE_OK;
}

rrte_status rrte_hip_mesh_slots(rrte_ctx* c, uint32_t* out, size_t count, uint32_t* slots) {
    if (!c || !slots || (count && !out)) return RRTE_INVALID_ARG;
    *slots = 0;
    if (c->sb_cur < 0 || !c->mesh_cache_valid) return RRTE_OK;
    const size_t all = c->mesh_cache.tris.size() / 3;
    *slots = (uint32_t)all;
    for (size_t k = 0; k < std::min(count, all); ++k) memcpy(out + k, &c->mesh_cache.tris[3 * k].w, sizeof(uint32_t));
    return RRTE_OK;
}

rrte_status rrte_hip_sdf_guards(const rrte_sdf_node* in, uint32_t count, uint32_t min_leaves, rrte_sdf_node* out,
                                uint32_t* guards) {
    if ((count && (!in || !out)) || !guards) return RRTE_INVALID_ARG;
    if (count && !sdf_program_ok(in, count)) return RRTE_UNSUPPORTED_PRIM;
    if (count) memmove(out, in, sizeof(rrte_sdf_node) * count);
    for (uint32_t i = 0; i < count; ++i) out[i].i[kGuardSlot] = 0u;
    *guards = min_leaves && count ? decorate_sdf_guards(out, count, min_leaves) : 0u;
    return RRTE_OK;
}

}  // extern "C"
