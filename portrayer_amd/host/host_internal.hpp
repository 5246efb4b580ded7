// Host-side pieces of Image::render that the reference runs once per render before its pixel loop
// (src/render.rs:93-126): flattening (src/flat_scene.rs), bounding boxes (src/bounding_box.rs), the
// scene k-d tree build (src/kdtree/leaf.rs, src/kdtree/kdscene.rs) and the camera (src/camera.rs).
#pragma once

#include <string>
#include <vector>

#include "../../include/portrayer_hip.h"
#include "portrayer.hpp"

namespace portrayer {
namespace detail {

struct BoundingBox {  // bounding_box.rs:39-117
    math::Vec3 min, max;
    math::Mat4 invtrans;
    static BoundingBox create(math::Vec3 min, math::Vec3 max);  // BoundingBox::new, panics unless min <= max
    double extent() const {  // bounding_box.rs:95-99: squared diagonal
        math::Vec3 d = max - min;
        return d.magnitude_squared();
    }
};
BoundingBox operator*(const math::Mat4& m, const BoundingBox& b);  // bounding_box.rs:123-148
BoundingBox primitive_bounds(const primitive::Primitive& p);       // Bounds for Primitive, primitive.rs:46-53

struct FlatSceneNode {  // flat_scene.rs:50-61
    scene::Geometry geometry;
    math::Mat4 trans, invtrans, normal_trans;
    // not in the reference's FlatSceneNode: where the node sits in the hierarchy, for PT_TRAVERSE_HIER
    std::vector<const scene::SceneNode*> chain;  // root .. the SceneNode that owns the geometry
    std::vector<uint32_t> path;                  // child index taken at every step below the root
    FlatSceneNode(scene::Geometry g, const math::Mat4& t);  // flat_scene.rs:103-108
    BoundingBox bounds() const { return trans * primitive_bounds(geometry.primitive); }  // flat_scene.rs:63-69
};

struct FlatScene {  // flat_scene.rs:16
    std::vector<FlatSceneNode> root;
    std::vector<light::Light> lights;
    math::Rgb ambient;
    static FlatScene from(const scene::HierScene& s);  // flat_scene.rs:18-46
};

struct GraphPacking {  // the ABI-4 scene-graph arrays of pt_scene (include/portrayer_hip.h)
    uint32_t n_graph_nodes = 0;
    std::vector<double> trans, invtrans, normal_trans;  // n_graph_nodes x 16
    std::vector<uint32_t> chain_off, chain, dfs_rank;
};
GraphPacking pack_graph(const FlatScene& flat);

// Whether `b` is `a` moved: the same flattened nodes in the same order - per node the primitive kind, the mesh / triangle (numbered by first
// use, equal in content), the shading flag, the material (numbered by first use, equal in its ten values, maps and uv transform) and the
// path through the graph (so graph nodes, chains and dfs_rank agree) - and as many lights. Transforms, light values and the ambient
// light may differ. Returns "" or the first difference.
// deformable = true asks for the same TOPOLOGY instead: a mesh may also differ in the values of its vertex positions and normals (vertex count, triangles,
// texture coordinates and the presence of normals must still be equal) - what Renderer::deform accepts.
std::string structure_difference(const FlatScene& a, const FlatScene& b, bool deformable = false);

struct PartitionConfig {  // leaf.rs:55-67
    size_t target_max_nodes = 3;
    long target_max_merit = 3;
    size_t max_tries = 10;
};

// KDTreeNode (node.rs:13-25) linearised in pre-order; node 0 is the root.
struct KdTree {
    std::vector<int32_t> axis, front, back, first, count, items;
    std::vector<double> plane;
    math::Vec3 root_min, root_max;
    int max_depth = 0;
};
// KDLeaf::partitioned (leaf.rs:89-231) over a list of cached bounds (NodeBounds, leaf.rs:16-34)
KdTree kd_partition(const std::vector<BoundingBox>& bounds, size_t max_depth, PartitionConfig conf);
KdTree kd_scene_tree(const FlatScene& flat, size_t max_depth);  // KDTreeScene::from, kdscene.rs:19-43
KdTree kd_mesh_tree(const primitive::MeshData& mesh, size_t max_depth);  // KDMesh::new, kdmesh.rs:37-58: the tree over a mesh's triangles
long kd_mesh_depth_setting();  // the environment's KD_MESH_DEPTH, else 10 (kdmesh.rs:15, :51-53)

struct Camera {  // camera.rs:17-45
    math::Vec3 eye;
    math::Mat4 view_to_world;
    double fov_factor, aspect_ratio, width, height;
    Camera(const camera::CameraSettings& cam, double width, double height);
    pt_camera to_abi() const;
};

// A scene prepared for the GPU: flattened, packed and uploaded once (pt_scene_upload); render() may
// then be called any number of times. Image::render builds one per call, like render.rs:121-126.
class Renderer {
   public:
    Renderer(const scene::HierScene& scene, render::Traversal traversal, int kd_depth, int device);
    ~Renderer();
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;
    void render(const camera::CameraSettings& cam, uint32_t width, uint32_t height, const double* background, bool background_rows,
                pt_rect slice, uint32_t samples, uint64_t seed, int sample_mode, bool collect_stats, uint8_t* rgb, double* linear,
                pt_stats* stats);
    // Rays of the caller's own (pt_rays): host buffers in and out; throws std::runtime_error with the library's message on any error.
    void rays(const pt_rays_params& params, const double* origins, const double* directions, const pt_rays_buffers& out, double* kernel_ms);
    // The same over bounded segments (pt_segments): t_max holds n bounds; throws likewise.
    void segments(const pt_rays_params& params, const double* origins, const double* directions, const double* t_max, const pt_rays_buffers& out, double* kernel_ms);
    // Radiance along rays of the caller's own (pt_radiance): host buffers in and out; throws likewise.
    void radiance(const pt_radiance_params& params, const double* origins, const double* directions, const double* background, double* rgb, double* kernel_ms);
    // The resident scene moved (pt_scene_update): `scene` must have the structure of the one this renderer was made from (structure_difference; throws
    // std::invalid_argument naming the first difference) and may differ in transforms, lights' values and ambient light. Nothing but the node matrices, the
    // lights and - in k-d mode - the rebuilt reference k-d tree goes to the device. On an error the renderer keeps its scene, unless the library says it is gone.
    void update(const scene::HierScene& scene);
    // Resident meshes deformed (pt_scene_deform): `scene` must have the topology of the one this renderer was made from (structure_difference(.., true); throws
    // std::invalid_argument naming the first difference). The meshes whose positions or normals differ in a bit are sent - vertices and bounds only - and their
    // trees refitted on the device; rebuild = true rebuilds those the device built at upload instead (and refits the others). The motion is performed as by update().
    void deform(const scene::HierScene& scene, bool rebuild = false);
    // Resident meshes deformed from vertices that are already in the memory of the renderer's device (pt_vertex_bounds_device + pt_scene_deform_device): per
    // mesh its index in the renderer's numbering (first use by the flattened nodes, as deform() numbers them), a device pointer to n_vertices x 3 f64 positions
    // and optionally one to as many normals. `moved` (optional) must have the structure of the resident scene; its matrices and lights ride along as in
    // update(). Such a mesh is remembered as posed on the device: the host's MeshData no longer describes it, so a later deform(scene) sends it whatever its
    // comparison says; update() keeps working (the boxes it needs are the library's resident ones). Throws std::invalid_argument for the k-d traversal (its
    // tree is built by the host from the meshes' bounds) and for a renderer with several ranks (each rank's device needs its own copy of the vertices).
    struct DeviceMesh { uint32_t mesh; const double* d_positions; const double* d_normals; };
    void deform_device(const std::vector<DeviceMesh>& meshes, bool rebuild = false, const scene::HierScene* moved = nullptr);
    size_t mesh_count() const;                 // distinct meshes, in the renderer's numbering
    int64_t mesh_vertices(size_t m) const;     // vertices of mesh m, -1: no such mesh
    pt_context* context() const { return ctx_; }  // rank 0's context when the scene is on a node
    pt_node* node() const { return node_; }
    const FlatScene& flat() const { return flat_; }
    struct PrepareMs { double flatten = 0, pack = 0, context = 0, kd_build = 0, upload = 0; };  // where the time before the first pixel goes
    const PrepareMs& prepare_ms() const { return prep_; }

   private:
    FlatScene flat_;
    pt_context* ctx_ = nullptr;
    pt_node* node_ = nullptr;  // PORTRAYER_GPUS > 1: the render is tile-partitioned over the node's GPUs (one RCCL gather)
    PrepareMs prep_;
    render::Traversal traversal_ = render::Traversal::Flat;
    int kd_depth_ = -1;
    std::vector<uint8_t> posed_on_device_;  // per mesh: deformed by deform_device since flat_ last described it
    void move(FlatScene&& moved, const std::vector<pt_mesh_deform>* deforms, const std::vector<pt_mesh_deform_device>* device_deforms = nullptr);
};

// PNG codec for Image::new / Image::save (render.rs:165-208; the reference uses the `image` crate)
bool png_read(const std::string& path, size_t* width, size_t* height, std::vector<uint8_t>* rgb);
bool jpeg_read(const std::string& path, size_t* width, size_t* height, std::vector<uint8_t>* rgb);   // jpeg.cpp
bool image_read(const std::string& path, size_t* width, size_t* height, std::vector<uint8_t>* rgb);  // PNG or JPEG, by signature
void png_write(const std::string& path, size_t width, size_t height, const std::vector<uint8_t>& rgb);

}  // namespace detail
}  // namespace portrayer
