// C entry points of the host library (include/portrayer_host.h).
#include <algorithm>
#include <cstring>
#include <map>
#include <string>

#include "../../examples/examples.hpp"
#include "../../include/portrayer_host.h"
#include "host_internal.hpp"

using namespace portrayer;
using namespace portrayer::math;

struct ph_scene {
    scene::HierScene hier;
};
struct ph_renderer {
    std::unique_ptr<detail::Renderer> r;
    // ph_renderer_ao_camera: position and normal of its primary-visibility pass and the device copies of its three outputs, for ao_points pixels; allocated on
    // first use, grown with the image, freed with the renderer (before its context goes). ph_renderer_gather_camera uses the same five (its sums in the fifth)
    void* d_ao[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    uint64_t ao_points = 0;
    // ph_renderer_ao_chart / ph_renderer_gather_chart: the same five for the map's texels, and the device copy of the caller's UV set (chart_uv_bytes long)
    void* d_chart_uv = nullptr;
    uint64_t chart_uv_bytes = 0;
    void ao_release() {
        for (void*& p : d_ao) { if (p) pt_device_free(r->context(), p); p = nullptr; }
        ao_points = 0;
        if (d_chart_uv) pt_device_free(r->context(), d_chart_uv);
        d_chart_uv = nullptr; chart_uv_bytes = 0;
    }
    ~ph_renderer() { if (r) ao_release(); }
};

static thread_local std::string g_error;

template <class F>
static int guarded(F&& f) {
    try {
        return f();
    } catch (const Panic& e) {
        g_error = std::string("panic: ") + e.what();
        return PH_ERR_PANIC;
    } catch (const std::exception& e) {
        g_error = e.what();
        return PH_ERR_RUNTIME;
    }
}
static int bad(const char* msg) { g_error = msg; return PH_ERR_ARGUMENT; }

extern "C" const char* ph_last_error(void) { return g_error.c_str(); }

extern "C" int ph_scene_create(const ph_scene_desc* d, ph_scene** out) {
    if (!d || !out) return bad("null argument");
    return guarded([&]() -> int {
        *out = nullptr;
        const uint32_t n = d->n_nodes;
        if (n == 0 || d->root >= n) return bad("scene needs a root node");
        std::vector<Arc<texture::Texture>> textures;     // one of each per image: a material picks the view it needs
        std::vector<Arc<texture::NormalMap>> normal_maps;
        for (uint32_t t = 0; t < d->n_textures; t++) {
            auto buf = texture::RgbImageBuffer::from_pixels(d->texture_size[2 * t], d->texture_size[2 * t + 1], d->texture_rgb + d->texture_offset[t]);
            textures.push_back(std::make_shared<texture::Texture>(texture::Texture{texture::ImageTexture{buf}}));
            normal_maps.push_back(std::make_shared<texture::NormalMap>(texture::NormalMap{std::move(buf)}));
        }
        std::vector<Arc<material::Material>> mats;
        for (uint32_t i = 0; i < d->n_materials; i++) {
            const double* m = d->materials + 10 * (size_t)i;
            auto mat = std::make_shared<material::Material>(material::Material{Rgb{m[0], m[1], m[2]}, Rgb{m[3], m[4], m[5]}, m[6], m[7], m[8], m[9]});
            if (d->material_texture && d->material_texture[i] >= 0) {
                if ((uint32_t)d->material_texture[i] >= d->n_textures) throw std::runtime_error("texture index out of range");
                mat->texture = textures[d->material_texture[i]];
            }
            if (d->material_normal_map && d->material_normal_map[i] >= 0) {
                if ((uint32_t)d->material_normal_map[i] >= d->n_textures) throw std::runtime_error("texture index out of range");
                mat->normals = normal_maps[d->material_normal_map[i]];
            }
            if (d->material_uv_trans) for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) mat->uv_trans.m[r][k] = d->material_uv_trans[9 * (size_t)i + 3 * r + k];
            mats.push_back(std::move(mat));
        }
        std::vector<Arc<primitive::MeshData>> meshes;
        for (uint32_t i = 0; i < d->n_meshes; i++) {
            uint64_t v0 = d->mesh_vert_off[i], v1 = d->mesh_vert_off[i + 1], t0 = d->mesh_tri_off[i], t1 = d->mesh_tri_off[i + 1];
            std::vector<Vec3> pos, nrm;
            for (uint64_t v = v0; v < v1; v++) pos.emplace_back(d->mesh_positions[3 * v], d->mesh_positions[3 * v + 1], d->mesh_positions[3 * v + 2]);
            if (d->mesh_has_normals && d->mesh_has_normals[i] && d->mesh_normals)
                for (uint64_t v = v0; v < v1; v++) nrm.emplace_back(d->mesh_normals[3 * v], d->mesh_normals[3 * v + 1], d->mesh_normals[3 * v + 2]);
            std::vector<std::array<uint32_t, 3>> tris;
            for (uint64_t t = t0; t < t1; t++) tris.push_back({d->mesh_indices[3 * t], d->mesh_indices[3 * t + 1], d->mesh_indices[3 * t + 2]});
            std::vector<Uv> uvs;
            if (d->mesh_has_texcoords && d->mesh_has_texcoords[i] && d->mesh_texcoords)
                for (uint64_t v = v0; v < v1; v++) uvs.push_back(Uv{d->mesh_texcoords[2 * v], d->mesh_texcoords[2 * v + 1]});
            meshes.push_back(primitive::MeshData::create(std::move(pos), std::move(tris), std::move(nrm), std::move(uvs)));
        }
        // Children must exist before their parents are finished: build in reverse topological order by
        // memoised recursion (the description is a DAG; shared nodes become shared Arcs).
        std::vector<Arc<scene::SceneNode>> built(n);
        std::vector<int> state(n, 0);
        std::function<Arc<scene::SceneNode>(uint32_t)> build = [&](uint32_t i) -> Arc<scene::SceneNode> {
            if (state[i] == 2) return built[i];
            if (state[i] == 1) throw Panic("scene graph has a cycle");
            state[i] = 1;
            scene::SceneNode node;
            int t = d->prim_type[i];
            if (t >= 0) {
                if (d->material[i] < 0 || (uint32_t)d->material[i] >= d->n_materials) throw std::runtime_error("material index out of range");
                Arc<material::Material> mat = mats[d->material[i]];
                primitive::Shading sh = (d->prim_flags[i] & 1) ? primitive::Shading::Smooth : primitive::Shading::Flat;
                auto mesh_at = [&](int32_t k) -> Arc<primitive::MeshData> {
                    if (k < 0 || (uint32_t)k >= d->n_meshes) throw std::runtime_error("mesh index out of range");
                    return meshes[k];
                };
                switch (t) {
                case PT_PRIM_SPHERE: node = scene::SceneNode::from(scene::Geometry::create(primitive::Sphere{}, mat)); break;
                case PT_PRIM_CUBE: node = scene::SceneNode::from(scene::Geometry::create(primitive::Cube{}, mat)); break;
                case PT_PRIM_PLANE: node = scene::SceneNode::from(scene::Geometry::create(primitive::Plane{}, mat)); break;
                case PT_PRIM_CYLINDER: node = scene::SceneNode::from(scene::Geometry::create(primitive::Cylinder{}, mat)); break;
                case PT_PRIM_CONE: node = scene::SceneNode::from(scene::Geometry::create(primitive::Cone{}, mat)); break;
                case PT_PRIM_MESH: node = scene::SceneNode::from(scene::Geometry::create(primitive::Mesh::create(mesh_at(d->prim_data[i]), sh), mat)); break;
                case PT_PRIM_KDMESH: node = scene::SceneNode::from(scene::Geometry::create(primitive::KDMesh::create(mesh_at(d->prim_data[i]), sh), mat)); break;
                case PT_PRIM_TRIANGLE: {
                    int32_t k = d->prim_data[i];
                    if (k < 0 || (uint32_t)k >= d->n_triangles) throw std::runtime_error("triangle index out of range");
                    const double* v = d->tri_vertices + 9 * (size_t)k;
                    primitive::Triangle tri = primitive::Triangle::flat(Vec3(v[0], v[1], v[2]), Vec3(v[3], v[4], v[5]), Vec3(v[6], v[7], v[8]));
                    if (d->tri_has_normals && d->tri_has_normals[k] && d->tri_normals) {
                        const double* q = d->tri_normals + 9 * (size_t)k;
                        tri.normals = std::array<Vec3, 3>{Vec3(q[0], q[1], q[2]), Vec3(q[3], q[4], q[5]), Vec3(q[6], q[7], q[8])};
                    }
                    if (d->tri_has_texcoords && d->tri_has_texcoords[k] && d->tri_texcoords) {
                        const double* q = d->tri_texcoords + 6 * (size_t)k;
                        tri.tex_coords = std::array<Uv, 3>{Uv{q[0], q[1]}, Uv{q[2], q[3]}, Uv{q[4], q[5]}};
                    }
                    node = scene::SceneNode::from(scene::Geometry::create(tri, mat));
                    break;
                }
                default: throw std::runtime_error("unknown primitive type");
                }
            }
            const double* a = d->args + d->args_off[i];
            for (uint32_t k = d->ops_off[i]; k < d->ops_off[i + 1]; k++) {
                switch (d->ops[k]) {
                case 's': node.scaled(Vec3(a[0], a[1], a[2])); a += 3; break;
                case 't': node.translated(Vec3(a[0], a[1], a[2])); a += 3; break;
                case 'x': node.rotated_x(Radians::from_radians(a[0])); a += 1; break;
                case 'y': node.rotated_y(Radians::from_radians(a[0])); a += 1; break;
                case 'z': node.rotated_z(Radians::from_radians(a[0])); a += 1; break;
                default: throw std::runtime_error("unknown builder op");
                }
            }
            for (uint32_t k = d->child_off[i]; k < d->child_off[i + 1]; k++) {
                if (d->children[k] >= n) throw std::runtime_error("child index out of range");
                node.with_child(build(d->children[k]));
            }
            built[i] = node.into();
            state[i] = 2;
            return built[i];
        };
        auto s = std::make_unique<ph_scene>();
        s->hier.root = build(d->root);
        for (uint32_t i = 0; i < d->n_lights; i++) {
            const double* l = d->lights + 15 * (size_t)i;
            s->hier.lights.push_back(light::Light{Vec3(l[0], l[1], l[2]), Rgb{l[3], l[4], l[5]}, light::Falloff{l[6], l[7], l[8]},
                                                  light::Parallelogram{Vec3(l[9], l[10], l[11]), Vec3(l[12], l[13], l[14])}});
        }
        s->hier.ambient = Rgb{d->ambient[0], d->ambient[1], d->ambient[2]};
        *out = s.release();
        return PH_OK;
    });
}

static examples::Example make_example(const std::string& name, const std::string& assets, int n) {
    if (name == "single-triangle") return examples::single_triangle();
    if (name == "primitives-simple") return examples::primitives_simple();
    if (name == "macho-cows") return examples::macho_cows(assets);
    if (name == "entering-the-mirror-dimension") return examples::entering_the_mirror_dimension(assets);
    if (name == "big-scene") return examples::big_scene(n > 1 ? n : 10);
    if (name == "synthetic:big-mesh") return examples::synthetic_big_mesh(assets, n > 1 ? n : 6);
    if (name == "synthetic:big-soup") return examples::synthetic_big_soup(assets, n > 1 ? n : 6);
    if (name == "smooth-shading") return examples::smooth_shading(assets);
    if (name == "glossy-reflection") return examples::glossy_reflection();
    if (name == "soft-shadows") return examples::soft_shadows(assets);
    if (name == "hier") return examples::hier(assets);
    if (name == "instance") return examples::instance(assets);
    if (name == "antialiasing") return examples::antialiasing(assets);
    if (name == "fish") return examples::fish(assets);
    if (name == "normal-mapping") return examples::normal_mapping(assets);
    if (name == "transmission-refraction") return examples::transmission_refraction(assets);
    if (name == "water-glass") return examples::water_glass(assets);
    if (name == "simple") return examples::simple();
    if (name == "nonhier") return examples::nonhier(assets);
    if (name == "nonhier2") return examples::nonhier2(assets);
    if (name == "four-shapes") return examples::four_shapes();
    if (name == "graphics-poster") return examples::graphics_poster(assets);
    if (name == "simple-cows") return examples::simple_cows(assets);
    if (name == "primitives") return examples::primitives(assets);
    if (name == "texture-mapping") return examples::texture_mapping(assets);
    if (name == "cube-mapping") return examples::cube_mapping(assets);
    if (name == "graphics-castle") return examples::graphics_castle(assets);
    if (name == "graphics-temple") return examples::graphics_temple(assets);
    if (name == "monkeys-making-monkeys") return examples::monkeys_making_monkeys(assets);
    if (name == "robot-alarm-clock") return examples::robot_alarm_clock(assets);
    throw std::runtime_error("unknown example scene: " + name);
}

extern "C" int ph_example_scene(const char* name, const char* assets_dir, int n, ph_scene** out, double camera[10], uint32_t size[2]) {
    if (!name || !out) return bad("null argument");
    return guarded([&]() -> int {
        examples::Example ex = make_example(name, assets_dir ? assets_dir : "assets", n);
        auto s = std::make_unique<ph_scene>();
        s->hier = std::move(ex.scene);
        if (camera) {
            const Vec3 v[3] = {ex.cam.eye, ex.cam.center, ex.cam.up};
            for (int k = 0; k < 3; k++) { camera[3 * k] = v[k].x; camera[3 * k + 1] = v[k].y; camera[3 * k + 2] = v[k].z; }
            camera[9] = ex.cam.fovy.get();
        }
        if (size) { size[0] = (uint32_t)ex.width; size[1] = (uint32_t)ex.height; }
        *out = s.release();
        return PH_OK;
    });
}

extern "C" void ph_scene_destroy(ph_scene* s) { delete s; }

namespace {
struct Linear {  // unique nodes in DFS pre-order, materials / meshes in order of first use
    std::vector<const scene::SceneNode*> nodes;
    std::map<const scene::SceneNode*, uint32_t> node_id;
    std::vector<const material::Material*> mats;
    std::map<const material::Material*, int32_t> mat_id;
    std::vector<const primitive::MeshData*> meshes;
    std::map<const primitive::MeshData*, int32_t> mesh_id;
    std::vector<const primitive::Triangle*> tris;
    size_t n_children = 0;
    void visit(const scene::SceneNode* n) {
        if (node_id.count(n)) return;
        node_id[n] = (uint32_t)nodes.size();
        nodes.push_back(n);
        for (const auto& c : n->children()) visit(c.get());
    }
    explicit Linear(const scene::HierScene& h) {
        visit(h.root.get());
        for (const scene::SceneNode* n : nodes) {
            n_children += n->children().size();
            if (!n->geometry()) continue;
            const auto& g = *n->geometry();
            if (!mat_id.count(g.material.get())) { mat_id[g.material.get()] = (int32_t)mats.size(); mats.push_back(g.material.get()); }
            if (g.primitive.mesh && !mesh_id.count(g.primitive.mesh.get())) { mesh_id[g.primitive.mesh.get()] = (int32_t)meshes.size(); meshes.push_back(g.primitive.mesh.get()); }
            if (g.primitive.kind == primitive::Primitive::TriangleK) tris.push_back(&g.primitive.triangle);
        }
    }
};
}  // namespace

// Textures, normal maps and texture coordinates of the scene, in the numbering of ph_scene_export (materials / meshes /
// triangles in order of first use). Two calls: with texture_rgb == NULL it only fills counts = {n_textures, texel bytes}.
extern "C" int ph_scene_export_textures(const ph_scene* s, uint64_t counts[2], int32_t* material_texture, int32_t* material_normal_map,
                                        double* material_uv_trans, uint32_t* texture_size, uint64_t* texture_offset, uint8_t* texture_rgb,
                                        double* mesh_texcoords, uint8_t* mesh_has_texcoords, double* tri_texcoords, uint8_t* tri_has_texcoords) {
    if (!s || !counts) return bad("null argument");
    return guarded([&]() -> int {
        Linear lin(s->hier);
        std::vector<const texture::RgbImageBuffer*> textures;
        std::map<const texture::RgbImageBuffer*, int32_t> tex_id;
        auto index = [&](const texture::RgbImageBuffer* b) {
            auto it = tex_id.find(b);
            if (it == tex_id.end()) { it = tex_id.emplace(b, (int32_t)textures.size()).first; textures.push_back(b); }
            return it->second;
        };
        for (size_t i = 0; i < lin.mats.size(); i++) {
            const material::Material* m = lin.mats[i];
            int32_t a = m->texture ? index(&m->texture->image.buffer) : -1, b = m->normals ? index(&m->normals->buffer) : -1;
            if (material_texture) material_texture[i] = a;
            if (material_normal_map) material_normal_map[i] = b;
            if (material_uv_trans) for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) material_uv_trans[9 * i + 3 * r + k] = m->uv_trans.m[r][k];
        }
        uint64_t off = 0;
        for (size_t t = 0; t < textures.size(); t++) {
            if (texture_size) { texture_size[2 * t] = (uint32_t)textures[t]->width; texture_size[2 * t + 1] = (uint32_t)textures[t]->height; }
            if (texture_offset) texture_offset[t] = off;
            if (texture_rgb) std::memcpy(texture_rgb + off, textures[t]->rgb.data(), textures[t]->rgb.size());
            off += textures[t]->rgb.size();
        }
        counts[0] = textures.size(); counts[1] = off;
        uint64_t vo = 0;
        for (size_t m = 0; m < lin.meshes.size(); m++) {
            const primitive::MeshData* md = lin.meshes[m];
            const bool ht = md->tex_coords().size() == md->positions().size();
            if (mesh_has_texcoords) mesh_has_texcoords[m] = ht ? 1 : 0;
            if (mesh_texcoords)
                for (size_t v = 0; v < md->positions().size(); v++) {
                    mesh_texcoords[2 * (vo + v)] = ht ? md->tex_coords()[v].u : 0.0;
                    mesh_texcoords[2 * (vo + v) + 1] = ht ? md->tex_coords()[v].v : 0.0;
                }
            vo += md->positions().size();
        }
        for (size_t t = 0; t < lin.tris.size(); t++) {
            const primitive::Triangle* tr = lin.tris[t];
            if (tri_has_texcoords) tri_has_texcoords[t] = tr->tex_coords ? 1 : 0;
            if (tri_texcoords)
                for (int k = 0; k < 3; k++) {
                    tri_texcoords[6 * t + 2 * k] = tr->tex_coords ? (*tr->tex_coords)[k].u : 0.0;
                    tri_texcoords[6 * t + 2 * k + 1] = tr->tex_coords ? (*tr->tex_coords)[k].v : 0.0;
                }
        }
        return PH_OK;
    });
}

extern "C" int ph_scene_counts(const ph_scene* s, uint64_t c[8]) {
    if (!s || !c) return bad("null argument");
    return guarded([&]() -> int {
        Linear lin(s->hier);
        uint64_t verts = 0, mtris = 0;
        for (auto* m : lin.meshes) { verts += m->positions().size(); mtris += m->triangles().size(); }
        c[0] = lin.nodes.size(); c[1] = lin.n_children; c[2] = lin.meshes.size(); c[3] = verts; c[4] = mtris;
        c[5] = lin.tris.size(); c[6] = lin.mats.size(); c[7] = s->hier.lights.size();
        return PH_OK;
    });
}

extern "C" int ph_scene_export(const ph_scene* s, double* node_trans, int32_t* prim_type, int32_t* prim_data, int32_t* prim_flags,
                               int32_t* material, uint32_t* child_off, uint32_t* children, uint32_t* root,
                               uint64_t* mesh_vert_off, uint64_t* mesh_tri_off, double* mesh_positions, double* mesh_normals,
                               uint8_t* mesh_has_normals, uint32_t* mesh_indices, double* tri_vertices, double* tri_normals,
                               uint8_t* tri_has_normals, double* materials, double* lights, double ambient[3]) {
    if (!s) return bad("null argument");
    return guarded([&]() -> int {
        Linear lin(s->hier);
        uint32_t ck = 0, tk = 0;
        for (size_t i = 0; i < lin.nodes.size(); i++) {
            const scene::SceneNode* n = lin.nodes[i];
            if (node_trans) std::memcpy(node_trans + 16 * i, n->trans().m, 128);
            int32_t t = -1, data = 0, flags = 0, mat = 0;
            if (n->geometry()) {
                const auto& g = *n->geometry();
                t = (int32_t)g.primitive.kind;
                mat = lin.mat_id[g.material.get()];
                if (g.primitive.mesh) { data = lin.mesh_id[g.primitive.mesh.get()]; flags = g.primitive.shading == primitive::Shading::Smooth ? 1 : 0; }
                if (g.primitive.kind == primitive::Primitive::TriangleK) data = (int32_t)tk++;
            }
            if (prim_type) prim_type[i] = t;
            if (prim_data) prim_data[i] = data;
            if (prim_flags) prim_flags[i] = flags;
            if (material) material[i] = mat;
            if (child_off) child_off[i] = ck;
            for (const auto& c : n->children()) { if (children) children[ck] = lin.node_id[c.get()]; ck++; }
        }
        if (child_off) child_off[lin.nodes.size()] = ck;
        if (root) *root = 0;
        uint64_t vo = 0, to = 0;
        for (size_t m = 0; m < lin.meshes.size(); m++) {
            const primitive::MeshData* md = lin.meshes[m];
            if (mesh_vert_off) mesh_vert_off[m] = vo;
            if (mesh_tri_off) mesh_tri_off[m] = to;
            bool hn = md->normals().size() == md->positions().size();
            if (mesh_has_normals) mesh_has_normals[m] = hn ? 1 : 0;
            for (size_t v = 0; v < md->positions().size(); v++) {
                const Vec3& p = md->positions()[v];
                if (mesh_positions) { mesh_positions[3 * (vo + v)] = p.x; mesh_positions[3 * (vo + v) + 1] = p.y; mesh_positions[3 * (vo + v) + 2] = p.z; }
                if (mesh_normals) {
                    Vec3 q = hn ? md->normals()[v] : Vec3::zero();
                    mesh_normals[3 * (vo + v)] = q.x; mesh_normals[3 * (vo + v) + 1] = q.y; mesh_normals[3 * (vo + v) + 2] = q.z;
                }
            }
            for (size_t t = 0; t < md->triangles().size(); t++)
                if (mesh_indices) for (int k = 0; k < 3; k++) mesh_indices[3 * (to + t) + k] = md->triangles()[t][k];
            vo += md->positions().size(); to += md->triangles().size();
        }
        if (mesh_vert_off) mesh_vert_off[lin.meshes.size()] = vo;
        if (mesh_tri_off) mesh_tri_off[lin.meshes.size()] = to;
        for (size_t t = 0; t < lin.tris.size(); t++) {
            const primitive::Triangle* tr = lin.tris[t];
            const Vec3 v[3] = {tr->a, tr->b, tr->c};
            for (int k = 0; k < 3; k++) {
                if (tri_vertices) { tri_vertices[9 * t + 3 * k] = v[k].x; tri_vertices[9 * t + 3 * k + 1] = v[k].y; tri_vertices[9 * t + 3 * k + 2] = v[k].z; }
                if (tri_normals) {
                    Vec3 q = tr->normals ? (*tr->normals)[k] : Vec3::zero();
                    tri_normals[9 * t + 3 * k] = q.x; tri_normals[9 * t + 3 * k + 1] = q.y; tri_normals[9 * t + 3 * k + 2] = q.z;
                }
            }
            if (tri_has_normals) tri_has_normals[t] = tr->normals ? 1 : 0;
        }
        for (size_t i = 0; i < lin.mats.size() && materials; i++) {
            const material::Material* m = lin.mats[i];
            const double row[10] = {m->diffuse.r, m->diffuse.g, m->diffuse.b, m->specular.r, m->specular.g, m->specular.b,
                                    m->shininess, m->reflectivity, m->glossy_side_length, m->refraction_index};
            std::memcpy(materials + 10 * i, row, sizeof row);
        }
        for (size_t i = 0; i < s->hier.lights.size() && lights; i++) {
            const light::Light& l = s->hier.lights[i];
            const double row[15] = {l.position.x, l.position.y, l.position.z, l.color.r, l.color.g, l.color.b, l.falloff.c0, l.falloff.c1, l.falloff.c2,
                                    l.area.a.x, l.area.a.y, l.area.a.z, l.area.b.x, l.area.b.y, l.area.b.z};
            std::memcpy(lights + 15 * i, row, sizeof row);
        }
        if (ambient) { ambient[0] = s->hier.ambient.r; ambient[1] = s->hier.ambient.g; ambient[2] = s->hier.ambient.b; }
        return PH_OK;
    });
}

extern "C" int ph_scene_flatten(const ph_scene* s, uint32_t cap, double* trans, double* invtrans, double* normal_trans,
                                int32_t* prim_type, int32_t* material, double* bounds) {
    if (!s) return bad("null argument");
    return guarded([&]() -> int {
        detail::FlatScene flat = detail::FlatScene::from(s->hier);
        std::map<const material::Material*, int32_t> mat_id;
        for (size_t i = 0; i < flat.root.size(); i++) {
            const auto& fn = flat.root[i];
            const material::Material* m = fn.geometry.material.get();
            if (!mat_id.count(m)) { int32_t id = (int32_t)mat_id.size(); mat_id[m] = id; }
            if (i >= cap) continue;
            if (trans) std::memcpy(trans + 16 * i, fn.trans.m, 128);
            if (invtrans) std::memcpy(invtrans + 16 * i, fn.invtrans.m, 128);
            if (normal_trans) std::memcpy(normal_trans + 16 * i, fn.normal_trans.m, 128);
            if (prim_type) prim_type[i] = (int32_t)fn.geometry.primitive.kind;
            if (material) material[i] = mat_id[m];
            if (bounds) {
                detail::BoundingBox b = fn.bounds();
                double* o = bounds + 6 * i;
                o[0] = b.min.x; o[1] = b.min.y; o[2] = b.min.z; o[3] = b.max.x; o[4] = b.max.y; o[5] = b.max.z;
            }
        }
        return (int)flat.root.size();
    });
}

extern "C" int ph_scene_graph(const ph_scene* s, uint32_t node_cap, uint32_t chain_cap, uint32_t graph_cap, uint32_t* chain_off, uint32_t* chain,
                              uint32_t* dfs_rank, double* graph_trans, double* graph_invtrans, double* graph_normal_trans, uint32_t counts[2]) {
    if (!s || !counts) return bad("null argument");
    return guarded([&]() -> int {
        detail::FlatScene flat = detail::FlatScene::from(s->hier);
        detail::GraphPacking g = detail::pack_graph(flat);
        const size_t n = flat.root.size();
        counts[0] = (uint32_t)g.chain.size(); counts[1] = g.n_graph_nodes;
        if (chain_off && node_cap >= n) std::memcpy(chain_off, g.chain_off.data(), (n + 1) * 4);
        if (dfs_rank && node_cap >= n) std::memcpy(dfs_rank, g.dfs_rank.data(), n * 4);
        if (chain && chain_cap >= g.chain.size()) std::memcpy(chain, g.chain.data(), g.chain.size() * 4);
        if (graph_cap >= g.n_graph_nodes) {
            if (graph_trans) std::memcpy(graph_trans, g.trans.data(), g.trans.size() * 8);
            if (graph_invtrans) std::memcpy(graph_invtrans, g.invtrans.data(), g.invtrans.size() * 8);
            if (graph_normal_trans) std::memcpy(graph_normal_trans, g.normal_trans.data(), g.normal_trans.size() * 8);
        }
        return (int)n;
    });
}

// a linearised tree into the caller's arrays; returns the node count
static int emit_kdtree(const detail::KdTree& t, uint32_t node_cap, uint32_t item_cap, int32_t* axis, double* plane, int32_t* front, int32_t* back,
                       int32_t* first, int32_t* count, int32_t* leaf_items, uint32_t* n_items, double root_bounds[6], int32_t* max_depth) {
    if (t.axis.size() > node_cap || t.items.size() > item_cap) { g_error = "output capacity too small"; return PH_ERR_SMALL; }
    for (size_t i = 0; i < t.axis.size(); i++) {
        if (axis) axis[i] = t.axis[i];
        if (plane) plane[i] = t.plane[i];
        if (front) front[i] = t.front[i];
        if (back) back[i] = t.back[i];
        if (first) first[i] = t.first[i];
        if (count) count[i] = t.count[i];
    }
    for (size_t i = 0; i < t.items.size(); i++) if (leaf_items) leaf_items[i] = t.items[i];
    if (n_items) *n_items = (uint32_t)t.items.size();
    if (root_bounds) {
        root_bounds[0] = t.root_min.x; root_bounds[1] = t.root_min.y; root_bounds[2] = t.root_min.z;
        root_bounds[3] = t.root_max.x; root_bounds[4] = t.root_max.y; root_bounds[5] = t.root_max.z;
    }
    if (max_depth) *max_depth = t.max_depth;
    return (int)t.axis.size();
}

extern "C" int ph_scene_kdtree(const ph_scene* s, int kd_depth, uint32_t node_cap, uint32_t item_cap, int32_t* axis, double* plane,
                               int32_t* front, int32_t* back, int32_t* first, int32_t* count, int32_t* leaf_items, uint32_t* n_items,
                               double root_bounds[6], int32_t* max_depth) {
    if (!s) return bad("null argument");
    return guarded([&]() -> int {
        detail::FlatScene flat = detail::FlatScene::from(s->hier);
        detail::KdTree t = detail::kd_scene_tree(flat, kd_depth < 0 ? 10 : (size_t)kd_depth);
        return emit_kdtree(t, node_cap, item_cap, axis, plane, front, back, first, count, leaf_items, n_items, root_bounds, max_depth);
    });
}

extern "C" int ph_scene_kdmesh_tree(const ph_scene* s, uint32_t mesh, int kd_mesh_depth, uint32_t node_cap, uint32_t item_cap, int32_t* axis, double* plane,
                                    int32_t* front, int32_t* back, int32_t* first, int32_t* count, int32_t* leaf_items, uint32_t* n_items,
                                    double root_bounds[6], int32_t* max_depth) {
    if (!s) return bad("null argument");
    return guarded([&]() -> int {
        detail::FlatScene flat = detail::FlatScene::from(s->hier);
        std::vector<const primitive::MeshData*> meshes;  // numbered by first use, as the upload numbers them
        for (const auto& fn : flat.root) {
            const auto& p = fn.geometry.primitive;
            if (p.kind != primitive::Primitive::MeshK && p.kind != primitive::Primitive::KDMeshK) continue;
            if (std::find(meshes.begin(), meshes.end(), p.mesh.get()) == meshes.end()) meshes.push_back(p.mesh.get());
        }
        if (mesh >= meshes.size()) return bad("no such mesh");
        detail::KdTree t = detail::kd_mesh_tree(*meshes[mesh], kd_mesh_depth < 0 ? (size_t)detail::kd_mesh_depth_setting() : (size_t)kd_mesh_depth);
        return emit_kdtree(t, node_cap, item_cap, axis, plane, front, back, first, count, leaf_items, n_items, root_bounds, max_depth);
    });
}

static camera::CameraSettings camera_from(const double c[10]) {
    return camera::CameraSettings{Vec3(c[0], c[1], c[2]), Vec3(c[3], c[4], c[5]), Vec3(c[6], c[7], c[8]), Radians::from_radians(c[9])};
}

extern "C" int ph_camera(const double c[10], double width, double height, pt_camera* out) {
    if (!c || !out) return bad("null argument");
    return guarded([&]() -> int {
        *out = detail::Camera(camera_from(c), width, height).to_abi();
        return PH_OK;
    });
}

extern "C" int ph_obj_load(const char* path, uint64_t counts[3], double* positions, double* normals, uint32_t* indices, uint64_t vert_cap, uint64_t tri_cap) {
    if (!path || !counts) return bad("null argument");
    return guarded([&]() -> int {
        auto md = primitive::MeshData::load_obj(path);
        bool hn = md->normals().size() == md->positions().size();
        counts[0] = md->positions().size(); counts[1] = md->triangles().size(); counts[2] = hn ? 1 : 0;
        for (size_t v = 0; v < md->positions().size() && v < vert_cap; v++) {
            if (positions) { positions[3 * v] = md->positions()[v].x; positions[3 * v + 1] = md->positions()[v].y; positions[3 * v + 2] = md->positions()[v].z; }
            if (normals && hn) { normals[3 * v] = md->normals()[v].x; normals[3 * v + 1] = md->normals()[v].y; normals[3 * v + 2] = md->normals()[v].z; }
        }
        for (size_t t = 0; t < md->triangles().size() && t < tri_cap; t++)
            if (indices) for (int k = 0; k < 3; k++) indices[3 * t + k] = md->triangles()[t][k];
        return PH_OK;
    });
}

extern "C" int ph_renderer_create(const ph_scene* s, int traverse, int kd_depth, int device, ph_renderer** out) {
    if (!s || !out) return bad("null argument");
    if (traverse != PT_TRAVERSE_FLAT && traverse != PT_TRAVERSE_KD && traverse != PT_TRAVERSE_HIER) return bad("traverse must be PT_TRAVERSE_FLAT, PT_TRAVERSE_KD or PT_TRAVERSE_HIER");
    return guarded([&]() -> int {
        auto r = std::make_unique<ph_renderer>();
        r->r = std::make_unique<detail::Renderer>(s->hier, traverse == PT_TRAVERSE_KD ? render::Traversal::KdTree : (traverse == PT_TRAVERSE_HIER ? render::Traversal::Hier : render::Traversal::Flat), kd_depth, device);
        *out = r.release();
        return PH_OK;
    });
}
extern "C" void ph_renderer_destroy(ph_renderer* r) { delete r; }
extern "C" pt_context* ph_renderer_context(ph_renderer* r) { return r ? r->r->context() : nullptr; }
extern "C" pt_node* ph_renderer_node(ph_renderer* r) { return r ? r->r->node() : nullptr; }
extern "C" int ph_renderer_ranks(ph_renderer* r) { return !r ? 0 : (r->r->node() ? pt_node_ranks(r->r->node()) : 1); }
extern "C" int ph_renderer_prepare_ms(ph_renderer* r, double out[5]) {
    if (!r || !out) return bad("null argument");
    const auto& p = r->r->prepare_ms();
    out[0] = p.flatten; out[1] = p.pack; out[2] = p.context; out[3] = p.kd_build; out[4] = p.upload;
    return PH_OK;
}

extern "C" int ph_renderer_render(ph_renderer* r, const double camera[10], const pt_render_params* p, const double* background,
                                  uint8_t* rgb, double* linear, pt_stats* stats) {
    if (!r || !camera || !p || !background || !rgb) return bad("null argument");
    return guarded([&]() -> int {
        if (p->tile_ranks != 1 || p->tile_rank != 0) {  // multi-GPU callers drive pt_render_device themselves
            pt_camera pc = detail::Camera(camera_from(camera), (double)p->width, (double)p->height).to_abi();
            int rc = pt_render(r->r->context(), &pc, background, p, rgb, linear, stats);
            if (rc != PT_OK) { g_error = pt_last_error(r->r->context()); return rc == PT_ERR_SLICE ? PH_ERR_PANIC : PH_ERR_RUNTIME; }
            return PH_OK;
        }
        r->r->render(camera_from(camera), p->width, p->height, background, p->background_rows != 0, p->slice, p->samples, p->seed,
                     p->sample_mode, p->collect_stats != 0, rgb, linear, stats);
        return PH_OK;
    });
}

extern "C" int ph_scene_same_structure(const ph_scene* a, const ph_scene* b, char* why, size_t n) {
    if (why && n) why[0] = 0;
    if (!a || !b) return bad("null argument");
    return guarded([&]() -> int {
        const std::string diff = detail::structure_difference(detail::FlatScene::from(a->hier), detail::FlatScene::from(b->hier));
        if (why && n) { std::strncpy(why, diff.c_str(), n - 1); why[n - 1] = 0; }
        return diff.empty() ? 1 : 0;
    });
}

extern "C" int ph_scene_same_topology(const ph_scene* a, const ph_scene* b, char* why, size_t n) {
    if (why && n) why[0] = 0;
    if (!a || !b) return bad("null argument");
    return guarded([&]() -> int {
        const std::string diff = detail::structure_difference(detail::FlatScene::from(a->hier), detail::FlatScene::from(b->hier), true);
        if (why && n) { std::strncpy(why, diff.c_str(), n - 1); why[n - 1] = 0; }
        return diff.empty() ? 1 : 0;
    });
}

extern "C" int ph_renderer_deform(ph_renderer* r, const ph_scene* s, int rebuild) {
    if (!r || !s) return bad("null argument");
    return guarded([&]() -> int {
        try {
            r->r->deform(s->hier, rebuild != 0);
        } catch (const std::invalid_argument& e) {
            g_error = e.what();
            return PH_ERR_ARGUMENT;
        }
        return PH_OK;
    });
}

extern "C" int ph_renderer_deform_device(ph_renderer* r, uint32_t n_meshes, const ph_device_mesh* meshes, int rebuild, const ph_scene* moved) {
    if (!r || (n_meshes && !meshes)) return bad("null argument");
    return guarded([&]() -> int {
        try {
            std::vector<detail::Renderer::DeviceMesh> dm(n_meshes);
            for (uint32_t k = 0; k < n_meshes; k++) dm[k] = detail::Renderer::DeviceMesh{meshes[k].mesh, meshes[k].d_positions, meshes[k].d_normals};
            r->r->deform_device(dm, rebuild != 0, moved ? &moved->hier : nullptr);
        } catch (const std::invalid_argument& e) {
            g_error = e.what();
            return PH_ERR_ARGUMENT;
        }
        return PH_OK;
    });
}

extern "C" int64_t ph_renderer_mesh_count(ph_renderer* r) { return r ? (int64_t)r->r->mesh_count() : (int64_t)bad("null argument"); }
extern "C" int64_t ph_renderer_mesh_vertices(ph_renderer* r, uint32_t mesh) {
    if (!r) return bad("null argument");
    const int64_t n = r->r->mesh_vertices(mesh);
    return n < 0 ? (int64_t)bad("mesh index out of range") : n;
}

extern "C" int ph_renderer_update(ph_renderer* r, const ph_scene* s) {
    if (!r || !s) return bad("null argument");
    return guarded([&]() -> int {
        try {
            r->r->update(s->hier);
        } catch (const std::invalid_argument& e) {
            g_error = e.what();
            return PH_ERR_ARGUMENT;
        }
        return PH_OK;
    });
}

extern "C" int ph_renderer_aov(ph_renderer* r, const double camera[10], const pt_aov_params* p, const pt_aov_buffers* out, double* kernel_ms) {
    if (!r || !camera || !p || !out) return bad("null argument");
    return guarded([&]() -> int {
        pt_camera pc = detail::Camera(camera_from(camera), (double)p->width, (double)p->height).to_abi();  // the camera a render of this size gets
        int rc = pt_aov(r->r->context(), &pc, p, out, kernel_ms);  // (a renderer spread over a node: rank 0's context, the whole slice)
        if (rc != PT_OK) { g_error = pt_last_error(r->r->context()); return rc == PT_ERR_SLICE ? PH_ERR_PANIC : PH_ERR_RUNTIME; }
        return PH_OK;
    });
}

extern "C" int ph_renderer_guides(ph_renderer* r, const double camera[10], const pt_aov_params* p, const pt_guides_buffers* out, double* kernel_ms) {
    if (!r || !camera || !p || !out) return bad("null argument");
    return guarded([&]() -> int {
        pt_camera pc = detail::Camera(camera_from(camera), (double)p->width, (double)p->height).to_abi();  // the camera a render of this size gets
        int rc = pt_guides(r->r->context(), &pc, p, out, kernel_ms);  // (a renderer spread over a node: rank 0's context, the whole slice)
        if (rc != PT_OK) { g_error = pt_last_error(r->r->context()); return rc == PT_ERR_SLICE ? PH_ERR_PANIC : PH_ERR_RUNTIME; }
        return PH_OK;
    });
}

extern "C" int ph_renderer_rays(ph_renderer* r, const pt_rays_params* p, const double* origins, const double* directions, const pt_rays_buffers* out, double* kernel_ms) {
    if (!r || !p || !out) return bad("null argument");
    if (p->n && (!origins || !directions)) return bad("null argument");
    return guarded([&]() -> int {
        r->r->rays(*p, origins, directions, *out, kernel_ms);  // (a renderer spread over a node: rank 0's context, every ray)
        return PH_OK;
    });
}

extern "C" int ph_renderer_segments(ph_renderer* r, const pt_rays_params* p, const double* origins, const double* directions, const double* t_max, const pt_rays_buffers* out,
                                    double* kernel_ms) {
    if (!r || !p || !out) return bad("null argument");
    if (p->n && (!origins || !directions || !t_max)) return bad("null argument");
    return guarded([&]() -> int {
        r->r->segments(*p, origins, directions, t_max, *out, kernel_ms);  // (a renderer spread over a node: rank 0's context, every ray)
        return PH_OK;
    });
}

// A pt_ return code of the renderer's context as this API shows it: the library's words in g_error, an argument error as one, anything else a runtime error.
static int shown(pt_context* c, int rc) {
    if (rc == PT_OK) return PH_OK;
    g_error = pt_last_error(c);
    return rc == PT_ERR_ARGUMENT ? PH_ERR_ARGUMENT : PH_ERR_RUNTIME;
}

// Ambient occlusion at points of the caller's own (pt_ao): host buffers in and out.
extern "C" int ph_renderer_ao(ph_renderer* r, const pt_ao_params* p, const double* positions, const double* normals, const pt_ao_buffers* out, double* kernel_ms) {
    if (!r || !p || !out) return bad("null argument");
    if (p->n && (!positions || !normals)) return bad("null argument");
    if (p->n == 0) { if (kernel_ms) *kernel_ms = 0.0; return PH_OK; }
    return guarded([&]() -> int {
        pt_context* c = r->r->context();  // (a renderer spread over a node: rank 0's context, every point)
        return shown(c, pt_ao(c, p, positions, normals, out, kernel_ms));
    });
}

// Gathered radiance at points of the caller's own (pt_gather): host buffers in and out.
extern "C" int ph_renderer_gather(ph_renderer* r, const pt_gather_params* p, const double* positions, const double* normals, const double* background,
                                  const pt_gather_buffers* out, double* kernel_ms) {
    if (!r || !p || !background || !out) return bad("null argument");
    if (p->n && (!positions || !normals)) return bad("null argument");
    if (p->n == 0) { if (kernel_ms) *kernel_ms = 0.0; return PH_OK; }
    return guarded([&]() -> int {
        pt_context* c = r->r->context();  // (a renderer spread over a node: rank 0's context, every point)
        return shown(c, pt_gather(c, p, positions, normals, background, out, kernel_ms));
    });
}

// Direct light at points of the caller's own (pt_direct): host buffers in and out.
extern "C" int ph_renderer_direct(ph_renderer* r, const pt_direct_params* p, const double* positions, const double* normals, const pt_direct_buffers* out, double* kernel_ms) {
    if (!r || !p || !out) return bad("null argument");
    if (p->n && (!positions || !normals)) return bad("null argument");
    if (p->n == 0) { if (kernel_ms) *kernel_ms = 0.0; return PH_OK; }
    return guarded([&]() -> int {
        pt_context* c = r->r->context();  // (a renderer spread over a node: rank 0's context, every point)
        return shown(c, pt_direct(c, p, positions, normals, out, kernel_ms));
    });
}

// Light probes at points in free space (pt_probe): host buffers in and out.
extern "C" int ph_renderer_probe(ph_renderer* r, const pt_probe_params* p, const double* positions, const double* background, const pt_probe_buffers* out, double* kernel_ms) {
    if (!r || !p || !background || !out) return bad("null argument");
    if (p->n && !positions) return bad("null argument");
    if (p->n == 0) { if (kernel_ms) *kernel_ms = 0.0; return PH_OK; }
    return guarded([&]() -> int {
        pt_context* c = r->r->context();  // (a renderer spread over a node: rank 0's context, every probe)
        return shown(c, pt_probe(c, p, positions, background, out, kernel_ms));
    });
}

// A mesh's light-map texels as surface points (pt_chart): host buffers in and out.
extern "C" int ph_renderer_chart_triangles(ph_renderer* r, uint32_t node, uint64_t* n_tris) {
    if (!r || !n_tris) return bad("null argument");
    return guarded([&]() -> int { return shown(r->r->context(), pt_chart_triangles(r->r->context(), node, n_tris)); });
}

// The mesh under flattened node `node`, for a caller that expands a per-vertex UV set to corners: counts = {vertices, triangles}; `indices` (optional) gets
// cap_tris x 3 vertex indices, and cap_tris must then be the triangle count.
extern "C" int ph_renderer_chart_mesh(ph_renderer* r, uint32_t node, uint64_t counts[2], uint32_t cap_tris, uint32_t* indices) {
    if (!r || !counts) return bad("null argument");
    return guarded([&]() -> int {
        const auto& nodes = r->r->flat().root;
        if (node >= nodes.size()) return bad("node index out of range");
        const auto& prim = nodes[node].geometry.primitive;
        if (prim.kind != primitive::Primitive::MeshK && prim.kind != primitive::Primitive::KDMeshK) return bad("the node is no mesh");
        counts[0] = prim.mesh->positions().size(); counts[1] = prim.mesh->triangles().size();
        if (!indices) return PH_OK;
        if (cap_tris != counts[1]) return bad("cap_tris is not the mesh's triangle count");
        size_t k = 0;
        for (const auto& t : prim.mesh->triangles()) { indices[k++] = t[0]; indices[k++] = t[1]; indices[k++] = t[2]; }
        return PH_OK;
    });
}

extern "C" int ph_renderer_chart(ph_renderer* r, const pt_chart_params* p, const double* uv, const pt_chart_buffers* out, double* kernel_ms) {
    if (!r || !p || !out) return bad("null argument");
    return guarded([&]() -> int {
        pt_context* c = r->r->context();  // (a renderer spread over a node: rank 0's context, the whole map)
        return shown(c, pt_chart(c, p, uv, out, kernel_ms));
    });
}

// ---- A pass over points that never leave the device: where the points come from (camera_points: a camera's pixels; chart_points: a light map's texels) and what
// is evaluated there (behind_points: ambient occlusion, gather or direct light). The renderer's point scratch d_ao holds n points: position (0) and normal (1) as
// the points' pass writes them, and the second pass's results - 4 bytes a point (2: occluded, lit), 1 byte (3: valid) and 24 bytes (4: bent, sum). A new pass over
// points is a queue step and a list of results for behind_points; a new source of points is a function like the two here.

// The scratch grown to n points. Returns a ph_ code, as everything below does.
static int points_scratch(ph_renderer* r, uint64_t n) {
    if (r->ao_points >= n) return PH_OK;
    pt_context* c = r->r->context();
    const size_t bytes[5] = {n * 24, n * 24, n * 4, n * 1, n * 24};
    int rc = PT_OK;
    r->ao_release();
    for (int k = 0; k < 5 && rc == PT_OK; k++) rc = pt_device_alloc(c, bytes[k], &r->d_ao[k]);
    if (rc != PT_OK) { const int code = shown(c, rc); r->ao_release(); return code; }
    r->ao_points = n;
    return PH_OK;
}

// The points under the pixel centres of a width x height image: the scratch, and pt_aov_device queued on the default stream with position and normal in its first
// two buffers. The pass is left OPEN: behind_points queues its own pass behind it and closes both. *pc: the camera a render of this size gets, for its eye.
static int camera_points(ph_renderer* r, const double camera[10], uint32_t width, uint32_t height, pt_camera* pc) {
    pt_context* c = r->r->context();
    if (int code = points_scratch(r, (uint64_t)width * height)) return code;
    *pc = detail::Camera(camera_from(camera), (double)width, (double)height).to_abi();
    pt_aov_params ap;
    ap.width = width; ap.height = height;
    ap.slice.x0 = 0; ap.slice.y0 = 0; ap.slice.x1 = width - 1; ap.slice.y1 = height - 1;
    ap.offset[0] = 0.5; ap.offset[1] = 0.5;
    pt_aov_buffers ab = {nullptr, (double*)r->d_ao[0], (double*)r->d_ao[1], nullptr, nullptr, nullptr};
    return shown(c, pt_aov_device(c, pc, &ap, &ab, nullptr));
}

// The texels of a mesh's light map: the scratch, the caller's UV set copied beside it (uv NULL: the mesh's own), and pt_chart_device queued on the default
// stream with position and normal in the scratch's first two buffers. The pass is left OPEN, as camera_points leaves its own.
static int chart_points(ph_renderer* r, const pt_chart_params* cp, const double* uv) {
    pt_context* c = r->r->context();
    int rc = PT_OK;
    uint64_t n_tris = 0;
    if ((rc = pt_chart_triangles(c, cp->node, &n_tris))) return shown(c, rc);
    if (int code = points_scratch(r, (uint64_t)cp->width * cp->height)) return code;
    if (uv && n_tris) {
        if (r->chart_uv_bytes < n_tris * 48) {
            if (r->d_chart_uv) pt_device_free(c, r->d_chart_uv);
            r->d_chart_uv = nullptr; r->chart_uv_bytes = 0;
            if ((rc = pt_device_alloc(c, n_tris * 48, &r->d_chart_uv))) return shown(c, rc);
            r->chart_uv_bytes = n_tris * 48;
        }
        if ((rc = pt_copy_to_device(c, r->d_chart_uv, uv, n_tris * 48))) return shown(c, rc);
    }
    pt_chart_buffers cb = {(double*)r->d_ao[0], (double*)r->d_ao[1], nullptr, nullptr};
    return shown(c, pt_chart_device(c, cp, uv && n_tris ? (const double*)r->d_chart_uv : nullptr, &cb, nullptr));
}

// One result of the pass behind the points: the caller's array (NULL: not asked for), the scratch buffer it comes back from, its length.
struct PointsOut { void* host; int slot; size_t bytes; };
template <class T>
static T* slot_if(ph_renderer* r, const T* host, int slot) { return host ? (T*)r->d_ao[slot] : nullptr; }

// Once the points' pass (left open) has position and normal on their way into the scratch: queue(context, d_positions, d_normals) puts a pt_*_device pass behind it
// on the same (default) stream, both passes are closed - the points' first, and its error is the one reported - and the results asked for are copied out, in
// `outs`' order.
template <class Queue, size_t N>
static int behind_points(ph_renderer* r, Queue&& queue, int (*finish)(pt_context*, double*), const PointsOut (&outs)[N], double* kernel_ms) {
    pt_context* c = r->r->context();
    int rc = queue(c, (const double*)r->d_ao[0], (const double*)r->d_ao[1]);
    if (rc) { const int code = shown(c, rc); pt_aov_finish(c, nullptr); return code; }
    const int rc_points = pt_aov_finish(c, nullptr);
    if (rc_points) g_error = pt_last_error(c);
    rc = finish(c, kernel_ms);
    if (rc_points) return PH_ERR_RUNTIME;
    if (rc) return shown(c, rc);
    for (const PointsOut& o : outs)
        if (o.host && (rc = pt_copy_from_device(c, o.host, r->d_ao[o.slot], o.bytes))) return shown(c, rc);
    return PH_OK;
}

// The three passes there are behind points; q: the caller's parameters with n, first_index, flags and eye set for the points' source.
static int ao_behind_points(ph_renderer* r, const pt_ao_params& q, const pt_ao_buffers* out, double* kernel_ms) {
    const pt_ao_buffers db = {slot_if(r, out->occluded, 2), slot_if(r, out->valid, 3), slot_if(r, out->bent, 4)};
    const PointsOut outs[3] = {{out->occluded, 2, q.n * 4}, {out->valid, 3, q.n}, {out->bent, 4, q.n * 24}};
    return behind_points(r, [&](pt_context* c, const double* P, const double* N) { return pt_ao_device(c, &q, P, N, &db, nullptr); }, pt_ao_finish, outs, kernel_ms);
}
static int gather_behind_points(ph_renderer* r, const pt_gather_params& q, const double* background, const pt_gather_buffers* out, double* kernel_ms) {
    const pt_gather_buffers db = {slot_if(r, out->sum, 4), slot_if(r, out->valid, 3)};
    const PointsOut outs[2] = {{out->sum, 4, q.n * 24}, {out->valid, 3, q.n}};
    return behind_points(r, [&](pt_context* c, const double* P, const double* N) { return pt_gather_device(c, &q, P, N, background, &db, nullptr); }, pt_gather_finish, outs,
                         kernel_ms);
}
static int direct_behind_points(ph_renderer* r, const pt_direct_params& q, const pt_direct_buffers* out, double* kernel_ms) {
    const pt_direct_buffers db = {slot_if(r, out->sum, 4), slot_if(r, out->lit, 2), slot_if(r, out->valid, 3)};
    const PointsOut outs[3] = {{out->sum, 4, q.n * 24}, {out->lit, 2, q.n * 4}, {out->valid, 3, q.n}};
    return behind_points(r, [&](pt_context* c, const double* P, const double* N) { return pt_direct_device(c, &q, P, N, &db, nullptr); }, pt_direct_finish, outs, kernel_ms);
}

// What the camera forms refuse before anything else, and the chart forms; asked: one of the pass's buffers was asked for. NULL: nothing.
static const char* camera_form_error(uint32_t width, uint32_t height, bool asked) {
    if (width == 0 || height == 0) return "width and height must be positive";
    if ((uint64_t)width * height > PT_AO_MAX) return "more than PT_AO_MAX pixels";
    return asked ? nullptr : "no output buffer asked for";
}
static const char* chart_form_error(const pt_chart_params* chart, bool asked) {
    if (chart->width == 0 || chart->height == 0) return "width and height must be positive";
    if ((uint64_t)chart->width * chart->height > PT_AO_MAX) return "more than PT_AO_MAX texels";
    return asked ? nullptr : "no output buffer asked for";
}

// The point passes under every pixel of a width x height image: point q = y * width + x is what pt_aov finds at the pixel's centre, its normal turned towards the
// camera's eye - so params->n, first_index, eye and flags (PT_AO_FACE_EYE; of a direct pass's own, PT_DIRECT_TO_LIGHT is kept) are set here - and only the
// results asked for cross the bus.
extern "C" int ph_renderer_ao_camera(ph_renderer* r, const double camera[10], uint32_t width, uint32_t height, const pt_ao_params* p, const pt_ao_buffers* out, double* kernel_ms) {
    if (!r || !camera || !p || !out) return bad("null argument");
    if (const char* why = camera_form_error(width, height, out->occluded || out->valid || out->bent)) return bad(why);
    return guarded([&]() -> int {
        pt_camera pc;
        if (int code = camera_points(r, camera, width, height, &pc)) return code;
        pt_ao_params q = *p;
        q.n = (uint64_t)width * height; q.first_index = 0; q.flags = PT_AO_FACE_EYE;
        for (int k = 0; k < 3; k++) q.eye[k] = pc.eye[k];
        return ao_behind_points(r, q, out, kernel_ms);
    });
}

extern "C" int ph_renderer_gather_camera(ph_renderer* r, const double camera[10], uint32_t width, uint32_t height, const pt_gather_params* p, const double* background,
                                         const pt_gather_buffers* out, double* kernel_ms) {
    if (!r || !camera || !p || !background || !out) return bad("null argument");
    if (const char* why = camera_form_error(width, height, out->sum || out->valid)) return bad(why);
    return guarded([&]() -> int {
        pt_camera pc;
        if (int code = camera_points(r, camera, width, height, &pc)) return code;
        pt_gather_params q = *p;
        q.n = (uint64_t)width * height; q.first_index = 0; q.flags = PT_AO_FACE_EYE;
        for (int k = 0; k < 3; k++) q.eye[k] = pc.eye[k];
        return gather_behind_points(r, q, background, out, kernel_ms);
    });
}

extern "C" int ph_renderer_direct_camera(ph_renderer* r, const double camera[10], uint32_t width, uint32_t height, const pt_direct_params* p, const pt_direct_buffers* out,
                                         double* kernel_ms) {
    if (!r || !camera || !p || !out) return bad("null argument");
    if (const char* why = camera_form_error(width, height, out->sum || out->lit || out->valid)) return bad(why);
    return guarded([&]() -> int {
        pt_camera pc;
        if (int code = camera_points(r, camera, width, height, &pc)) return code;
        pt_direct_params q = *p;
        q.n = (uint64_t)width * height; q.first_index = 0; q.flags = PT_AO_FACE_EYE | (p->flags & PT_DIRECT_TO_LIGHT);
        for (int k = 0; k < 3; k++) q.eye[k] = pc.eye[k];
        return direct_behind_points(r, q, out, kernel_ms);
    });
}

// The point passes at every texel of a mesh's light map: point q = y * width + x is pt_chart's, first_index 0, no PT_AO_FACE_EYE (a chart's normals face outwards
// or, with PT_CHART_FLIP_NORMAL, inwards). Of `params` samples, pass, seed, bias - an ambient-occlusion pass's radius, a direct pass's PT_DIRECT_TO_LIGHT - are read.
extern "C" int ph_renderer_ao_chart(ph_renderer* r, const pt_chart_params* chart, const double* uv, const pt_ao_params* p, const pt_ao_buffers* out, double* kernel_ms) {
    if (!r || !chart || !p || !out) return bad("null argument");
    if (const char* why = chart_form_error(chart, out->occluded || out->valid || out->bent)) return bad(why);
    return guarded([&]() -> int {
        if (int code = chart_points(r, chart, uv)) return code;
        pt_ao_params q = *p;
        q.n = (uint64_t)chart->width * chart->height; q.first_index = 0; q.flags = 0;
        return ao_behind_points(r, q, out, kernel_ms);
    });
}

extern "C" int ph_renderer_gather_chart(ph_renderer* r, const pt_chart_params* chart, const double* uv, const pt_gather_params* p, const double* background,
                                        const pt_gather_buffers* out, double* kernel_ms) {
    if (!r || !chart || !p || !background || !out) return bad("null argument");
    if (const char* why = chart_form_error(chart, out->sum || out->valid)) return bad(why);
    return guarded([&]() -> int {
        if (int code = chart_points(r, chart, uv)) return code;
        pt_gather_params q = *p;
        q.n = (uint64_t)chart->width * chart->height; q.first_index = 0; q.flags = 0;
        return gather_behind_points(r, q, background, out, kernel_ms);
    });
}

extern "C" int ph_renderer_direct_chart(ph_renderer* r, const pt_chart_params* chart, const double* uv, const pt_direct_params* p, const pt_direct_buffers* out,
                                        double* kernel_ms) {
    if (!r || !chart || !p || !out) return bad("null argument");
    if (const char* why = chart_form_error(chart, out->sum || out->lit || out->valid)) return bad(why);
    return guarded([&]() -> int {
        if (int code = chart_points(r, chart, uv)) return code;
        pt_direct_params q = *p;
        q.n = (uint64_t)chart->width * chart->height; q.first_index = 0; q.flags = p->flags & PT_DIRECT_TO_LIGHT;
        return direct_behind_points(r, q, out, kernel_ms);
    });
}

extern "C" int ph_renderer_radiance(ph_renderer* r, const pt_radiance_params* p, const double* origins, const double* directions, const double* background, double* rgb,
                                    double* kernel_ms) {
    if (!r || !p || !background) return bad("null argument");
    if (p->n && (!origins || !directions || !rgb)) return bad("null argument");
    if ((p->reorder != 0 && p->reorder != 1) || (p->background_per_ray != 0 && p->background_per_ray != 1)) return bad("reorder and background_per_ray are 0 or 1");
    if (p->n > PT_RAYS_MAX) return bad("more than PT_RAYS_MAX rays in one call");
    if (p->n == 0) { if (kernel_ms) *kernel_ms = 0.0; return PH_OK; }  // nothing to shade, nothing written (the flags are checked all the same, as pt_radiance does)
    return guarded([&]() -> int {
        r->r->radiance(*p, origins, directions, background, rgb, kernel_ms);  // (a renderer spread over a node: rank 0's context, every ray)
        return PH_OK;
    });
}

// A film of the renderer's context (pt_film_*). The handle remembers the film's size: the camera of an add is the one a render of that size gets.
struct ph_film {
    pt_film* f = nullptr;
    uint32_t width = 0, height = 0;
    // ph_renderer_film_denoise: the guides its aov pass writes (position, normal, node) and the device copies of its three outputs, allocated on first use
    void* d_guide[3] = {nullptr, nullptr, nullptr};
    void* d_out[3] = {nullptr, nullptr, nullptr};
    void* d_albedo = nullptr;  // ph_renderer_film_denoise_albedo: the albedo its guides pass writes
};
static int film_rc(ph_renderer* r, int rc) {
    if (rc == PT_OK) return PH_OK;
    g_error = pt_last_error(r->r->context());
    return rc == PT_ERR_SLICE ? PH_ERR_PANIC : PH_ERR_RUNTIME;
}

extern "C" int ph_renderer_film_create(ph_renderer* r, uint32_t width, uint32_t height, ph_film** out) {
    if (!r || !out) return bad("null argument");
    *out = nullptr;
    if (width == 0 || height == 0) return bad("a film's width and height must be positive");
    if (r->r->node()) return bad("a film lives on one device: this renderer is spread over several ranks (PORTRAYER_GPUS); create it with one");
    return guarded([&]() -> int {
        auto f = std::make_unique<ph_film>();
        f->width = width; f->height = height;
        int rc = film_rc(r, pt_film_create(r->r->context(), width, height, &f->f));
        if (rc != PH_OK) return rc;
        *out = f.release();
        return PH_OK;
    });
}

extern "C" int ph_renderer_film_destroy(ph_renderer* r, ph_film* film) {
    if (!r || !film) return bad("null argument");
    return guarded([&]() -> int {
        int rc = film_rc(r, pt_film_destroy(r->r->context(), film->f));
        if (rc != PH_OK) return rc;
        for (void* d : {film->d_guide[0], film->d_guide[1], film->d_guide[2], film->d_out[0], film->d_out[1], film->d_out[2], film->d_albedo}) if (d) pt_device_free(r->r->context(), d);
        delete film;
        return rc;
    });
}

extern "C" int ph_renderer_film_reset(ph_renderer* r, ph_film* film) {
    if (!r || !film) return bad("null argument");
    return guarded([&]() -> int { return film_rc(r, pt_film_reset(r->r->context(), film->f)); });
}

extern "C" int ph_renderer_film_add(ph_renderer* r, ph_film* film, const double camera[10], const double* background, const pt_film_params* p, double* kernel_ms) {
    if (!r || !film || !camera || !background || !p) return bad("null argument");
    return guarded([&]() -> int {
        pt_camera pc = detail::Camera(camera_from(camera), (double)film->width, (double)film->height).to_abi();  // the camera a render of this size gets
        return film_rc(r, pt_film_add(r->r->context(), film->f, &pc, background, p, kernel_ms));
    });
}

// The same behind a lens (pt_film_add_lens): the camera is the one a render of the film's size gets, the lens is the caller's.
extern "C" int ph_renderer_film_add_lens(ph_renderer* r, ph_film* film, const double camera[10], const pt_lens* lens, const double* background, const pt_film_params* p, double* kernel_ms) {
    if (!r || !film || !camera || !lens || !background || !p) return bad("null argument");
    return guarded([&]() -> int {
        pt_camera pc = detail::Camera(camera_from(camera), (double)film->width, (double)film->height).to_abi();
        return film_rc(r, pt_film_add_lens(r->r->context(), film->f, &pc, lens, background, p, kernel_ms));
    });
}

extern "C" int ph_renderer_film_resolve(ph_renderer* r, ph_film* film, uint8_t* rgb, double* linear) {
    if (!r || !film || (!rgb && !linear)) return bad("null argument");
    return guarded([&]() -> int { return film_rc(r, pt_film_resolve(r->r->context(), film->f, rgb, linear)); });
}

extern "C" int ph_renderer_film_counts(ph_renderer* r, ph_film* film, uint32_t* counts) {
    if (!r || !film || !counts) return bad("null argument");
    return guarded([&]() -> int { return film_rc(r, pt_film_counts(r->r->context(), film->f, counts)); });
}

extern "C" int ph_renderer_film_create_moments(ph_renderer* r, uint32_t width, uint32_t height, ph_film** out) {
    if (!r || !out) return bad("null argument");
    *out = nullptr;
    if (width == 0 || height == 0) return bad("a film's width and height must be positive");
    if (r->r->node()) return bad("a film lives on one device: this renderer is spread over several ranks (PORTRAYER_GPUS); create it with one");
    return guarded([&]() -> int {
        auto f = std::make_unique<ph_film>();
        f->width = width; f->height = height;
        int rc = film_rc(r, pt_film_create_moments(r->r->context(), width, height, &f->f));
        if (rc != PH_OK) return rc;
        *out = f.release();
        return PH_OK;
    });
}

extern "C" int ph_renderer_film_add_map(ph_renderer* r, ph_film* film, const double camera[10], const double* background, const pt_film_map_params* p, const uint32_t* budget, double* kernel_ms) {
    if (!r || !film || !camera || !background || !p || !budget) return bad("null argument");
    return guarded([&]() -> int {
        pt_camera pc = detail::Camera(camera_from(camera), (double)film->width, (double)film->height).to_abi();  // the camera a render of this size gets
        return film_rc(r, pt_film_add_map(r->r->context(), film->f, &pc, background, p, budget, kernel_ms));
    });
}

extern "C" int ph_renderer_film_error(ph_renderer* r, ph_film* film, double* err) {
    if (!r || !film || !err) return bad("null argument");
    return guarded([&]() -> int { return film_rc(r, pt_film_error(r->r->context(), film->f, err)); });
}

// The closed loop: budget on the device, its two-word summary to the host, a device map's add, until no pixel wants more or max_passes have run. The map
// never leaves the device.
extern "C" int ph_renderer_film_refine(ph_renderer* r, ph_film* film, const double camera[10], const double* background, const pt_film_map_params* sampling, const pt_film_refine_params* refine,
                                       uint32_t max_passes, uint64_t out[3], double* kernel_ms) {
    if (!r || !film || !camera || !background || !sampling || !refine || !out) return bad("null argument");
    if (sampling->background_rows != 0 && sampling->background_rows != 1) return bad("background_rows is 0 or 1");
    return guarded([&]() -> int {
        pt_context* c = r->r->context();
        pt_camera pc = detail::Camera(camera_from(camera), (double)film->width, (double)film->height).to_abi();
        const size_t n = (size_t)film->width * film->height;
        const size_t bg_bytes = (sampling->background_rows ? (size_t)film->height : n) * 24;
        void *d_bg = nullptr, *d_budget = nullptr, *d_summary = nullptr;
        auto release = [&]() { for (void* d : {d_bg, d_budget, d_summary}) if (d) pt_device_free(c, d); };
        int rc;
        if ((rc = pt_device_alloc(c, bg_bytes, &d_bg)) || (rc = pt_device_alloc(c, n * 4, &d_budget)) || (rc = pt_device_alloc(c, 16, &d_summary)) ||
            (rc = pt_copy_to_device(c, d_bg, background, bg_bytes))) {
            rc = film_rc(r, rc);
            release();
            return rc;
        }
        pt_film_map_params mp = *sampling;
        mp.slice = refine->slice;
        mp.max_samples = refine->step;
        uint64_t passes = 0, samples = 0, summary[2] = {0, 0};
        double ms_all = 0.0;
        for (;;) {
            if ((rc = pt_film_budget_device(c, film->f, refine, (uint32_t*)d_budget, (uint64_t*)d_summary, nullptr)) || (rc = pt_copy_from_device(c, summary, d_summary, 16))) break;
            if (summary[0] == 0 || passes == max_passes) break;
            double ms = 0.0;
            if ((rc = pt_film_add_map_device(c, film->f, &pc, (const double*)d_bg, &mp, (const uint32_t*)d_budget, nullptr))) break;
            if ((rc = pt_radiance_finish(c, &ms))) break;
            ms_all += ms;
            passes++;
            samples += summary[1];
        }
        if (rc == PT_OK && passes) {  // the library's host copy of the counts was raised by `step` per pass: back to the device's values
            std::vector<uint32_t> counts(n);
            rc = pt_film_counts(c, film->f, counts.data());
        }
        rc = film_rc(r, rc);
        release();
        if (rc != PH_OK) return rc;
        out[0] = passes; out[1] = samples; out[2] = summary[0];
        if (kernel_ms) *kernel_ms = ms_all;
        return PH_OK;
    });
}

// The film, denoised (pt_film_denoise): with the caller's guides the library's host path; without, the guides come from a primary-visibility pass at the pixel
// centres for `camera` and never leave the device - pt_aov_device into buffers kept with the handle, pt_aov_finish, pt_film_denoise_device, the outputs copied out.
// demodulated (ph_renderer_film_denoise_albedo, pt_film_denoise_albedo): the caller's guides come with the caller's albedo; without them ONE guides pass
// (pt_guides_device) writes the albedo beside the guides in the same trace, and pt_film_denoise_albedo_device takes the place of pt_film_denoise_device.
static int film_denoise(ph_renderer* r, ph_film* film, const double camera[10], const pt_denoise_params* p, const pt_denoise_guides* guides, bool demodulated, const double* albedo, uint8_t* rgb,
                        double* linear, double* variance) {
    if (!r || !film || !p || (!guides && !camera) || (!rgb && !linear && !variance)) return bad("null argument");
    if (demodulated && (guides != nullptr) != (albedo != nullptr)) return bad("the caller's guides and the caller's albedo come together");
    return guarded([&]() -> int {
        pt_context* c = r->r->context();
        if (guides) return film_rc(r, demodulated ? pt_film_denoise_albedo(c, film->f, p, guides, albedo, rgb, linear, variance) : pt_film_denoise(c, film->f, p, guides, rgb, linear, variance));
        const size_t n = (size_t)film->width * film->height;
        const bool want_n = p->normal_power_log2 >= 0 || p->sigma_plane > 0.0, want_pos = p->sigma_plane > 0.0;
        const size_t guide_bytes[3] = {n * 24, n * 24, n * 4}, out_bytes[3] = {n * 3, n * 24, n * 8};
        const bool guide_wanted[3] = {want_pos, want_n, true};
        void* host_out[3] = {rgb, linear, variance};
        int rc = PT_OK;
        for (int k = 0; k < 3 && rc == PT_OK; k++) {
            if (guide_wanted[k] && !film->d_guide[k]) rc = pt_device_alloc(c, guide_bytes[k], &film->d_guide[k]);
            if (rc == PT_OK && host_out[k] && !film->d_out[k]) rc = pt_device_alloc(c, out_bytes[k], &film->d_out[k]);
        }
        if (rc == PT_OK && demodulated && !film->d_albedo) rc = pt_device_alloc(c, n * 24, &film->d_albedo);
        if (rc != PT_OK) return film_rc(r, rc);
        // pixels without samples keep the caller's bytes: where there are any, the caller's buffers go to the device first
        std::vector<uint32_t> counts(n);
        if ((rc = pt_film_counts(c, film->f, counts.data()))) return film_rc(r, rc);
        if (std::find(counts.begin(), counts.end(), 0u) != counts.end())
            for (int k = 0; k < 3; k++)
                if (host_out[k] && (rc = pt_copy_to_device(c, film->d_out[k], host_out[k], out_bytes[k]))) return film_rc(r, rc);
        pt_camera pc = detail::Camera(camera_from(camera), (double)film->width, (double)film->height).to_abi();  // the camera a render of this size gets
        pt_aov_params ap;
        ap.width = film->width; ap.height = film->height;
        ap.slice.x0 = 0; ap.slice.y0 = 0; ap.slice.x1 = film->width - 1; ap.slice.y1 = film->height - 1;
        ap.offset[0] = 0.5; ap.offset[1] = 0.5;
        pt_denoise_guides dg = {want_pos ? (double*)film->d_guide[0] : nullptr, want_n ? (double*)film->d_guide[1] : nullptr, (int32_t*)film->d_guide[2]};
        void* d_rgb = rgb ? film->d_out[0] : nullptr;
        double *d_linear = linear ? (double*)film->d_out[1] : nullptr, *d_variance = variance ? (double*)film->d_out[2] : nullptr;
        if (demodulated) {
            pt_guides_buffers gb = {(double*)film->d_albedo, (double*)dg.position, (double*)dg.normal, (int32_t*)dg.node};
            if ((rc = pt_guides_device(c, &pc, &ap, &gb, nullptr))) return film_rc(r, rc);
            if ((rc = pt_guides_finish(c, nullptr))) return film_rc(r, rc);
            if ((rc = pt_film_denoise_albedo_device(c, film->f, p, &dg, gb.albedo, d_rgb, d_linear, d_variance, nullptr))) return film_rc(r, rc);
        } else {
            pt_aov_buffers ab = {nullptr, (double*)dg.position, (double*)dg.normal, (int32_t*)dg.node, nullptr, nullptr};
            if ((rc = pt_aov_device(c, &pc, &ap, &ab, nullptr))) return film_rc(r, rc);
            if ((rc = pt_aov_finish(c, nullptr))) return film_rc(r, rc);
            if ((rc = pt_film_denoise_device(c, film->f, p, &dg, d_rgb, d_linear, d_variance, nullptr))) return film_rc(r, rc);
        }
        for (int k = 0; k < 3; k++)
            if (host_out[k] && (rc = pt_copy_from_device(c, host_out[k], film->d_out[k], out_bytes[k]))) return film_rc(r, rc);
        return PH_OK;
    });
}

extern "C" int ph_renderer_film_denoise(ph_renderer* r, ph_film* film, const double camera[10], const pt_denoise_params* p, const pt_denoise_guides* guides, uint8_t* rgb, double* linear,
                                        double* variance) {
    return film_denoise(r, film, camera, p, guides, false, nullptr, rgb, linear, variance);
}

extern "C" int ph_renderer_film_denoise_albedo(ph_renderer* r, ph_film* film, const double camera[10], const pt_denoise_params* p, const pt_denoise_guides* guides, const double* albedo,
                                               uint8_t* rgb, double* linear, double* variance) {
    return film_denoise(r, film, camera, p, guides, true, albedo, rgb, linear, variance);
}

extern "C" int ph_example_render_to_png(const char* name, const char* assets_dir, int n, uint32_t width, uint32_t height, const char* png_path) {
    if (!name || !png_path) return bad("null argument");
    return guarded([&]() -> int {
        examples::Example ex = make_example(name, assets_dir ? assets_dir : "assets", n);
        render::Image image = render::Image::create(png_path, width ? width : ex.width, height ? height : ex.height);
        image.render<reporter::NullProgress>(ex.scene, ex.cam, ex.background);
        image.save();
        return PH_OK;
    });
}

extern "C" int ph_png_read(const char* path, uint32_t size[2], uint8_t* rgb, uint64_t cap) {
    if (!path || !size) return bad("null argument");
    return guarded([&]() -> int {
        size_t w = 0, h = 0;
        std::vector<uint8_t> buf;
        if (!detail::png_read(path, &w, &h, &buf)) { g_error = "file not found"; return PH_ERR_RUNTIME; }
        size[0] = (uint32_t)w; size[1] = (uint32_t)h;
        if (rgb) { if (cap < buf.size()) { g_error = "output capacity too small"; return PH_ERR_SMALL; } std::memcpy(rgb, buf.data(), buf.size()); }
        return PH_OK;
    });
}
extern "C" int ph_image_read(const char* path, uint32_t size[2], uint8_t* rgb, uint64_t cap) {
    if (!path || !size) return bad("null argument");
    return guarded([&]() -> int {
        size_t w = 0, h = 0;
        std::vector<uint8_t> buf;
        if (!detail::image_read(path, &w, &h, &buf)) { g_error = "file not found"; return PH_ERR_RUNTIME; }
        size[0] = (uint32_t)w; size[1] = (uint32_t)h;
        if (rgb) {
            if (cap < buf.size()) return bad("buffer too small");
            std::memcpy(rgb, buf.data(), buf.size());
        }
        return PH_OK;
    });
}

extern "C" int ph_png_write(const char* path, uint32_t width, uint32_t height, const uint8_t* rgb) {
    if (!path || !rgb) return bad("null argument");
    return guarded([&]() -> int {
        detail::png_write(path, width, height, std::vector<uint8_t>(rgb, rgb + (size_t)width * height * 3));
        return PH_OK;
    });
}

// examples/*.cpp main(): Image::new(..)?; image.render::<RenderProgress, _>(&scene, cam, sky); image.save()
int portrayer::examples::run_main(Example ex) {
    try {
        render::Image image = render::Image::create(ex.output, ex.width, ex.height);
        image.render<reporter::RenderProgress>(ex.scene, ex.cam, ex.background);
        image.save();
        const auto& st = image.last_stats();
        std::fprintf(stderr, "%s: kernel %.2f ms, total %.2f ms\n", ex.output.c_str(), st.kernel_ms, st.total_ms);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
