/* portrayer_hip.h — C ABI of the MI355X (gfx950) ray-cast / shade path.
 *
 * This library replaces the body of the reference's pixel loop and everything it calls:
 *   ImageSliceMut::render           src/render.rs:127-150   (the rayon loop over pixels)
 *   render_single_pixel             src/render.rs:22-51
 *   Camera::ray_at                  src/camera.rs:48-84
 *   Ray::color, RayCast / RayHit    src/ray.rs:39-148
 *   FlatSceneNode::ray_cast         src/flat_scene.rs:71-99
 *   KDTreeNode::ray_cast_impl       src/kdtree/node.rs:66-203
 *   Primitive::ray_hit dispatch     src/primitive.rs:55-62 and src/primitive/{sphere,triangle,mesh,cube,plane,cylinder,cone}.rs
 *   BoundingBox::test_hit           src/bounding_box.rs:104-116
 *   Material::hit_color             src/material.rs:91-320
 * The reference has no FFI of its own (it is one Rust crate); these entry points are what a
 * binding placed where render.rs:127-150 is today would call — INTEGRATION.md shows that binding.
 * Host-side work that the reference does once per render stays with the caller and crosses this
 * boundary as plain arrays: flattening (src/flat_scene.rs:18-46), matrix inverses, bounding boxes
 * (src/bounding_box.rs:55-82, :123-148), the scene k-d tree build (src/kdtree/leaf.rs:89-231,
 * src/kdtree/kdscene.rs:19-43), the camera matrix (src/camera.rs:34-45) and the background closure
 * evaluated per integer pixel (src/render.rs:31-34).
 *
 * Conventions: every array is caller-owned, read-only for the duration of the call and may be
 * freed afterwards; matrices are row-major 4x4 (16 doubles); no callbacks, no unwinding: every
 * function returns 0 or a negative PT_ERR_* code and pt_last_error() describes the failure.
 * One context per GPU; calls on one context must be serialised by the caller.
 */
#ifndef PORTRAYER_HIP_H
#define PORTRAYER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 8

/* enum Primitive, src/primitive.rs:67-81 */
enum { PT_PRIM_SPHERE = 0, PT_PRIM_TRIANGLE = 1, PT_PRIM_MESH = 2, PT_PRIM_KDMESH = 3, PT_PRIM_PLANE = 4, PT_PRIM_CUBE = 5, PT_PRIM_CYLINDER = 6, PT_PRIM_CONE = 7 };
/* cargo features flat_scene / kdtree, src/render.rs:121-126 */
enum { PT_TRAVERSE_FLAT = 1, PT_TRAVERSE_KD = 2, PT_TRAVERSE_HIER = 3 };
/* sample position inside the pixel (the reference draws it from thread_rng, src/render.rs:38-39) */
enum { PT_SAMPLE_CENTRE = 0, PT_SAMPLE_RNG = 1 };

enum {
    PT_OK = 0,
    PT_ERR_ARGUMENT = -1,   /* null pointer, bad index, bad enum                                     */
    PT_ERR_DEVICE = -2,     /* HIP runtime error (text in pt_last_error)                             */
    PT_ERR_NO_SCENE = -3,   /* pt_render before pt_scene_upload                                      */
    PT_ERR_SLICE = -4,      /* slice corner outside the image: ImageSliceMut::new panics, render.rs:79-90 */
    PT_ERR_SCENE = -5,      /* inconsistent scene (mesh without vertices, mesh.rs:71; smooth shading without normals, mesh.rs:135-138;
                               a textured material on a primitive without texture coordinates, material.rs:133,141) */
    PT_ERR_TRAVERSAL = -6   /* a lane ran out of traversal stack (never expected; results invalid)    */
};

typedef struct pt_context pt_context;

/* The flattened scene: Scene<Vec<FlatSceneNode>> (src/flat_scene.rs:16, :50-61), nodes in the
 * breadth-first order FlatScene::from emits them (src/flat_scene.rs:18-46). */
typedef struct {
    uint32_t n_nodes;
    const double *trans;          /* n_nodes x 16  FlatSceneNode::trans                                  */
    const double *invtrans;       /* n_nodes x 16  trans.inverted()                (flat_scene.rs:104)    */
    const double *normal_trans;   /* n_nodes x 16  invtrans.transposed()           (flat_scene.rs:105)    */
    const int32_t *prim_type;     /* PT_PRIM_*                                                           */
    const int32_t *prim_data;     /* MESH/KDMESH: mesh index; TRIANGLE: triangle index; else ignored     */
    const int32_t *prim_flags;    /* bit 0: Shading::Smooth (mesh.rs:11-18) / triangle has vertex normals */
    const int32_t *material;      /* index into materials                                                */
    /* MeshData, src/primitive/mesh.rs:21-34 */
    uint32_t n_meshes;
    const uint64_t *mesh_vert_off;   /* n_meshes + 1, in vertices                                         */
    const uint64_t *mesh_tri_off;    /* n_meshes + 1, in triangles                                        */
    const double *mesh_positions;    /* total vertices x 3                                                */
    const double *mesh_normals;      /* total vertices x 3, or NULL when no mesh has normals              */
    const uint8_t *mesh_has_normals; /* n_meshes, or NULL                                                 */
    const uint32_t *mesh_indices;    /* total triangles x 3, indices local to the mesh                    */
    const double *mesh_bounds_invtrans; /* n_meshes x 16: BoundingBox::invtrans of the mesh AABB (bounding_box.rs:55-82) */
    /* stand-alone Triangle primitives, src/primitive/triangle.rs:8-19 */
    uint32_t n_triangles;
    const double *tri_vertices;      /* n_triangles x 9: a, b, c                                          */
    const double *tri_normals;       /* n_triangles x 9, or NULL                                          */
    /* Material hot fields, src/material.rs:50-86: diffuse rgb, specular rgb, shininess, reflectivity,
     * glossy_side_length, refraction_index */
    uint32_t n_materials;
    const double *materials;         /* n_materials x 10                                                  */
    /* Light, src/light.rs:74-91: position, color, falloff c0 c1 c2, area.a, area.b */
    uint32_t n_lights;
    const double *lights;            /* n_lights x 15                                                     */
    double ambient[3];               /* Scene::ambient, src/scene.rs:17                                   */
    /* Image textures and normal maps, src/texture.rs (ABI 2). All optional: leave NULL / 0 for scenes
     * without textured materials. Texels are the RGB8 pixels as the image decoder returns them
     * (RgbImageBuffer, texture.rs:74-76); sRGB -> linear (texture.rs:162-168) happens at sampling. */
    const double *mesh_texcoords;       /* total vertices x 2 (MeshData::tex_coords, mesh.rs:30), or NULL  */
    const uint8_t *mesh_has_texcoords;  /* n_meshes, or NULL                                               */
    const double *tri_texcoords;        /* n_triangles x 6 (Triangle::tex_coords, triangle.rs:18), or NULL */
    const uint8_t *tri_has_texcoords;   /* n_triangles, or NULL                                            */
    const int32_t *material_texture;    /* n_materials: texture index or -1 (Material::texture, material.rs:75) */
    const int32_t *material_normal_map; /* n_materials: texture index or -1 (Material::normals, material.rs:85) */
    const double *material_uv_trans;    /* n_materials x 9 row-major Mat3 (material.rs:83); NULL = identity  */
    uint32_t n_textures;
    const uint32_t *texture_size;       /* n_textures x 2: width, height                                   */
    const uint64_t *texture_offset;     /* n_textures: byte offset of texel (0,0) in texture_rgb           */
    const uint8_t *texture_rgb;         /* all texels, row-major RGB8                                      */
    /* KDMesh triangle trees (ABI 3): KDMesh::new builds a k-d tree over the mesh's triangles
     * (src/kdtree/kdmesh.rs:37-58, KD_MESH_DEPTH) whose traversal can miss hits a Mesh finds (squared
     * extent, bounding_box.rs:95-99); to reproduce that the host passes the trees, linearised like
     * pt_kdtree with node indices into the shared kdm_* arrays. Optional: a KDMesh whose mesh has
     * mesh_kd_root < 0 (or NULL arrays) is traversed like a Mesh. */
    const int32_t *mesh_kd_root;        /* n_meshes: root node index in kdm_*, or -1                       */
    const int32_t *mesh_kd_depth;       /* n_meshes: Split levels above the deepest leaf                   */
    const double *mesh_kd_bounds;       /* n_meshes x 6: root bounds min, max                              */
    const double *mesh_kd_bounds_invtrans; /* n_meshes x 16: BoundingBox::invtrans of the root bounds      */
    uint32_t n_kdm_nodes;
    const int32_t *kdm_axis; const double *kdm_plane; const int32_t *kdm_front, *kdm_back, *kdm_first, *kdm_count;
    uint32_t n_kdm_items;
    const int32_t *kdm_items;           /* triangle indices local to the mesh, in leaf Vec order            */
    /* The scene GRAPH (ABI 4), for PT_TRAVERSE_HIER: the reference's default traversal (no `flat_scene` /
     * `kdtree` feature) transforms the ray level by level down the hierarchy with each SceneNode's OWN inverse
     * and carries hit point and normal back up level by level (src/scene.rs:80-120). That rounds differently
     * from one composed matrix per flattened node, and where a ray starts on a refractive surface the
     * difference decides hits. NULL / 0 for the other traversals. */
    uint32_t n_graph_nodes;             /* distinct SceneNodes on the paths to the flattened nodes            */
    const double *graph_trans;          /* n_graph_nodes x 16  SceneNode::trans        (scene.rs:150-160)     */
    const double *graph_invtrans;       /* n_graph_nodes x 16  SceneNode::invtrans                            */
    const double *graph_normal_trans;   /* n_graph_nodes x 16  SceneNode::normal_trans                        */
    const uint32_t *node_chain_off;     /* n_nodes + 1: flattened node i's path is node_chain[off[i] .. off[i+1]) */
    const uint32_t *node_chain;         /* graph node indices from the root down to the node itself           */
    const uint32_t *node_dfs_rank;      /* n_nodes: place in depth-first order, a node before its children:   */
                                        /*   the order in which equal hits are resolved (ray.rs:87-99 under scene.rs:95-117) */
} pt_scene;

/* The scene k-d tree the host built (KDTreeScene::from, src/kdtree/kdscene.rs:19-43), linearised;
 * node 0 is the root. Needed for PT_TRAVERSE_KD only.
 * Limits (pt_scene_upload fails with PT_ERR_SCENE beyond them): at most 32 split levels on any path
 * from the root (the reference's KD_DEPTH defaults to 10, kdscene.rs:36; a tree deeper than 32 has more
 * than 2^32 leaves unless it is a degenerate chain), fewer than 2^26 nodes, fewer than 2^27 leaf items. */
typedef struct {
    uint32_t n_nodes;
    const int32_t *axis;      /* 0,1,2: KDTreeNode::Split on that axis; -1: KDTreeNode::Leaf (node.rs:13-25) */
    const double *plane;      /* Split: sep_plane.point on `axis`                                         */
    const int32_t *front;     /* Split: front_nodes                                                       */
    const int32_t *back;      /* Split: back_nodes                                                        */
    const int32_t *first;     /* Leaf: its nodes are leaf_items[first .. first + count), in Vec order      */
    const int32_t *count;
    uint32_t n_items;
    const int32_t *leaf_items; /* flat node indices                                                       */
    double root_min[3], root_max[3]; /* root bounds; extent() = squared diagonal (bounding_box.rs:95-99)   */
    int32_t max_depth;        /* Split levels above the deepest leaf (sizes the traversal stack)          */
} pt_kdtree;

/* Camera, src/camera.rs:17-31, as Camera::new (camera.rs:34-45) computes it */
typedef struct {
    double eye[3];
    double view_to_world[16];
    double fov_factor;    /* tan(fovy / 2)  */
    double aspect_ratio;  /* width / height */
    double width, height;
} pt_camera;

typedef struct { uint32_t x0, y0, x1, y1; } pt_rect; /* inclusive corners like ImageSliceMut, render.rs:56-66 */

typedef struct {
    uint32_t width, height;     /* Image::width / height                                                 */
    pt_rect slice;              /* pixels to render; others are left untouched (render.rs:135-138)        */
    uint32_t samples;           /* env SAMPLES (render.rs:107-113), > 0                                   */
    uint64_t seed;              /* key of the counter-based sample generator                             */
    int32_t sample_mode;        /* PT_SAMPLE_*                                                            */
    int32_t background_rows;    /* 1: background is height x 3 (one colour per row); 0: height x width x 3 */
    uint32_t tile_rank;         /* multi-GPU: render only the 8x8 tiles t of the slice with              */
    uint32_t tile_ranks;        /*   t % tile_ranks == tile_rank (1 GPU: 0 of 1)                          */
    int32_t collect_stats;      /* 1: run the counting build of the kernel and fill ray/test counters     */
} pt_render_params;

typedef struct {
    uint64_t primary, shadow, reflect, refract; /* rays traced                                           */
    uint64_t depth11_skipped;   /* depth-11 rays the reference would trace and discard (material.rs:102-104) */
    uint64_t hits;              /* shaded hits                                                           */
    uint64_t n_inner, n_leaf;   /* tree nodes visited (bounding-volume nodes in FLAT, k-d nodes in KD)    */
    uint64_t n_analytic;        /* flat-node candidate tests (ray transform + primitive dispatch)         */
    uint64_t n_tri;             /* triangle tests                                                         */
    uint64_t n_bbox;            /* mesh bounding-box tests                                                */
    uint64_t kd_plane_miss;     /* places where the reference would panic (node.rs:146-147, :177-178)      */
    uint64_t stack_overflow;    /* must be 0                                                              */
    double kernel_ms;           /* device time of the render kernel (HIP events)                          */
    double total_ms;            /* upload of per-call inputs + kernel + read-back                         */
    uint64_t diag[8];           /* (ABI 5) lane-occupancy diagnostics of -DPT_DIAG builds (profiles/diag.sh); 0 otherwise */
    uint32_t kernel_mode;       /* (ABI 6) which instantiation of the render kernel ran: PT_KERNEL_MODE_* ...                */
    uint32_t kernel_variant;    /* ... and PT_KERNEL_* (tests assert that a timed configuration is the one they checked)    */
} pt_stats;

/* pt_stats.kernel_mode: the walk the kernel was compiled with */
enum { PT_KERNEL_MODE_FLAT = 1, PT_KERNEL_MODE_KD = 2, PT_KERNEL_MODE_FLAT_NOMESH = 3, PT_KERNEL_MODE_FLAT_KDMESH = 4, PT_KERNEL_MODE_HIER = 5,
       PT_KERNEL_MODE_HIER_NOMESH = 6, PT_KERNEL_MODE_KD_NOMESH = 7,
       PT_KERNEL_MODE_HIER_MESH = 8 /* hierarchical, Mesh instances but no KDMesh trees (5 has both compiled in) */,
       PT_KERNEL_MODE_KD_MESH = 9 /* kdtree semantics, Mesh instances but no KDMesh trees (2 has both compiled in) */ };
/* pt_stats.kernel_variant: bit 0-3 waves per SIMD the kernel was compiled for (3 or 4); PT_KERNEL_INTERPRETER: the per-lane
 * interpreter that scenes with reflective materials need (material.rs:216-303), else the straight-line kernel; PT_KERNEL_PARK:
 * a parked recursion frame per lane in LDS; PT_KERNEL_COUNTING: the counting build (collect_stats); PT_KERNEL_TEXTURED */
enum { PT_KERNEL_WAVES_MASK = 15, PT_KERNEL_INTERPRETER = 16, PT_KERNEL_PARK = 32, PT_KERNEL_COUNTING = 64, PT_KERNEL_TEXTURED = 128,
       PT_KERNEL_FORK = 256 /* idle lanes take the refracted subtrees busy lanes offer (LDS queue, ballot / popcount ranks) */,
       PT_KERNEL_CHAIN = 512 /* the straight-line kernel with a loop over the depth: every reflective material of the scene is opaque */ };

int pt_abi_version(void);
int pt_device_count(void);

int pt_context_create(int device, pt_context **out);
void pt_context_destroy(pt_context *ctx);
const char *pt_last_error(const pt_context *ctx);

/* Uploads the scene into HBM and builds the traversal structures. `traverse` = PT_TRAVERSE_*;
 * `kd` must be non-NULL for PT_TRAVERSE_KD. Replaces any scene uploaded before. */
int pt_scene_upload(pt_context *ctx, const pt_scene *scene, int traverse, const pt_kdtree *kd);

/* Moves the resident scene: the scene stays as uploaded except for the node matrices (and, in PT_TRAVERSE_HIER, the graph nodes'), the lights and
 * the ambient light, which are replaced by the ones given here. After PT_OK every entry point answers as if pt_scene_upload had been called with the
 * original pt_scene carrying these arrays - the same bits in pixels, linear means, aov / rays / radiance results and the ray counters primary, shadow,
 * reflect, refract, hits, depth11_skipped (tree-visit counters may differ) - in the traversal the scene was uploaded with; in PT_TRAVERSE_KD the new
 * k-d tree is part of the call (`kd`, NULL otherwise). Primitive types and data, materials, meshes and their trees, KDMesh trees, textures, node paths
 * and dfs_rank stay resident and untouched: no triangle, tree-item or texture data is copied; only the scene-level tree is rebuilt (on the host or on
 * the device: PORTRAYER_BUILD, as for mesh trees). The call is synchronous.
 * Errors, all before the first write (the resident scene stays usable): PT_ERR_ARGUMENT (NULL context / motion / matrix arrays; n_nodes, n_graph_nodes
 * or - with lights - n_lights other than the uploaded scene's; PT_TRAVERSE_HIER without graph_*; PT_TRAVERSE_KD without `kd`, `kd` in another traversal,
 * an inconsistent k-d tree; "a render is in flight": a pt_render_device, pt_aov_device, pt_rays_device or pt_radiance_device not yet closed by its
 * _finish), PT_ERR_NO_SCENE. PT_ERR_SCENE as for an upload (tree too deep for the traversal stack, the k-d limits): after it the context has NO scene,
 * as after a refused pt_scene_upload. */
typedef struct {
    uint32_t n_nodes;                 /* must equal the uploaded scene's */
    const double *trans, *invtrans, *normal_trans;          /* n_nodes x 16 each, as in pt_scene */
    uint32_t n_graph_nodes;           /* PT_TRAVERSE_HIER: must equal the uploaded scene's; else 0 */
    const double *graph_trans, *graph_invtrans, *graph_normal_trans;
    uint32_t n_lights;                /* with lights != NULL: must equal the uploaded scene's */
    const double *lights;             /* n_lights x 15, or NULL: lights stay as they are */
    const double *ambient;            /* 3 doubles, or NULL */
} pt_scene_motion;
int pt_scene_update(pt_context *ctx, const pt_scene_motion *motion, const pt_kdtree *kd);

/* Deforms resident meshes: new vertex positions (and normals) under the topology the mesh was uploaded with, then the pt_scene_update above (every instance's
 * world box, the root box, the scene-level tree and - in PT_TRAVERSE_KD - `kd` depend on the mesh's new box; `motion` is required and may carry the matrices
 * already resident). After PT_OK every entry point answers as if pt_scene_upload had been called with the original pt_scene carrying these positions, normals,
 * mesh bounds and the motion's arrays: the same bits in pixels, linear means, aov / rays / radiance results (`sub` included), the ray counters primary, shadow,
 * reflect, refract, hits, depth11_skipped and kernel_mode / kernel_variant (tree-visit counters may differ). Only the vertices cross to the device
 * (n_vertices x 24 bytes, 48 with normals): triangle records are expanded there through the resident indices, and the mesh's tree - which keeps its place in the
 * tree arrays - is REFITTED (rebuild = 0: same topology, every box recomputed bottom-up; a large deformation costs walk speed, never a result) or REBUILT by
 * the device builder in place (rebuild = 1: only for a tree the device built at upload, PORTRAYER_BUILD). Indices, texture coordinates, textures, materials,
 * node paths and the trees of meshes not named stay resident and untouched. The first deform of a context allocates what it needs (the indices on the device,
 * a parent index and an arrival counter per tree node, a staging buffer for vertices); later deforms of the same meshes allocate nothing. Synchronous.
 * n_deforms = 0 is a plain pt_scene_update.
 * Errors, all before the first write (the resident scene stays usable): PT_ERR_ARGUMENT (NULL context / deforms / positions / bounds_invtrans / motion; a mesh
 * index out of range or named twice; normals for a mesh uploaded without; a mesh with a KDMesh tree (mesh_kd_root >= 0: the reference's own structure, built
 * by the host from the positions); rebuild = 1 for a tree the upload built on the host; a non-finite coordinate or a mesh box beyond +-1e18; everything
 * pt_scene_update refuses about motion or kd, a pass in flight included), PT_ERR_NO_SCENE. PT_ERR_SCENE as for pt_scene_update: the context then has NO scene. */
typedef struct {
    uint32_t mesh;                  /* index into the uploaded scene's meshes                                   */
    const double *positions;        /* n_vertices x 3, the vertex count the mesh was uploaded with               */
    const double *normals;          /* n_vertices x 3, or NULL: the resident normals stay                        */
    const double *bounds_invtrans;  /* 16 doubles: BoundingBox::invtrans of the NEW mesh AABB (as pt_scene.mesh_bounds_invtrans) */
    int32_t rebuild;                /* 0: refit the resident tree; 1: rebuild it with the device builder, in place */
} pt_mesh_deform;
int pt_scene_deform(pt_context *ctx, uint32_t n_deforms, const pt_mesh_deform *deforms,
                    const pt_scene_motion *motion, const pt_kdtree *kd);
/* Whether pt_scene_deform accepts rebuild = 1 for this mesh of the resident scene: 1 (the device built its tree at upload, so its place has the worst-case
 * size), 0 (the host built it: refit only), PT_ERR_ARGUMENT (NULL context, mesh index out of range), PT_ERR_NO_SCENE. Needs no device work. */
int pt_scene_mesh_rebuildable(const pt_context *ctx, uint32_t mesh);

/* ---- The same deform with vertices that are already in DEVICE memory (a simulation, skinning or a torch tensor on the context's GPU): nothing per vertex
 * crosses the bus or is touched by the host. Two calls, because bounds_invtrans and - in PT_TRAVERSE_KD - `kd` are host structures that depend on the mesh's
 * new box: pt_vertex_bounds_device gives the caller the box, from which it makes BoundingBox::invtrans (and the k-d tree), then pt_scene_deform_device deforms.
 *
 * pt_vertex_bounds_device: the box of n_vertices x 3 f64 positions in device memory, by one reduction pass on the device. out[0..2] = min, out[3..5] = max per
 * axis, with the bits the host loop of pt_scene_upload / pt_scene_deform leaves: where an extreme is a zero that occurs with both signs, the sign of the
 * lowest-index vertex attaining it. *non_finite = how many of the 3 n coordinates are NaN or +-inf; they take no part in min / max. n_vertices = 0 or nothing
 * finite: the empty box (min = +inf, max = -inf). Needs no scene. Synchronous, see "Ordering" below.
 *
 * pt_scene_deform_device: pt_scene_deform with d_positions / d_normals in device memory. After PT_OK the resident scene equals, in everything pt_scene_deform
 * promises, the scene after pt_scene_deform with the same values read from host arrays. The library computes each mesh's box again itself (it never takes a
 * caller's word for a conservative box) and the expand kernel reads the caller's buffers in place: no staging buffer is reserved.
 * Ordering: both calls are synchronous and work on the default stream. They open with a hipDeviceSynchronize of the context's device, which is also what orders
 *   them behind whatever stream produced the vertices: work queued on any stream of that device before the call is complete before the buffers are read. The
 *   caller's buffers are free again when the call returns.
 * Pointers: d_positions (and d_normals, if given) must be 8-byte aligned device memory of the context's device, as hipPointerGetAttributes reports it, and the
 *   allocation (hipMemGetAddressRange) must reach n_vertices x 24 bytes beyond the pointer; a pointer into the middle of a larger allocation is fine. Pageable or
 *   pinned host memory, managed memory and another device's memory are refused: no kernel is launched on a pointer that fails the check.
 * Errors, all before the first write (the resident scene stays usable): PT_ERR_ARGUMENT (everything pt_scene_deform refuses, a pass in flight included; NULL
 *   d_positions / bounds_invtrans / out / non_finite; a pointer that fails the check above; non_finite != 0 or a mesh box beyond +-1e18, in pt_scene_deform's
 *   words; n_vertices >= 2^32), PT_ERR_NO_SCENE, PT_ERR_DEVICE. PT_ERR_SCENE as for pt_scene_update: the context then has NO scene. */
int pt_vertex_bounds_device(pt_context *ctx, uint64_t n_vertices, const double *d_positions, double out[6], uint64_t *non_finite);
typedef struct {
    uint32_t mesh;                  /* index into the uploaded scene's meshes                                   */
    const double *d_positions;      /* DEVICE, n_vertices x 3, the vertex count the mesh was uploaded with       */
    const double *d_normals;        /* DEVICE, n_vertices x 3, or NULL: the resident normals stay                */
    const double *bounds_invtrans;  /* HOST, 16 doubles, as in pt_mesh_deform                                    */
    int32_t rebuild;                /* as in pt_mesh_deform                                                      */
} pt_mesh_deform_device;
int pt_scene_deform_device(pt_context *ctx, uint32_t n_deforms, const pt_mesh_deform_device *deforms,
                           const pt_scene_motion *motion, const pt_kdtree *kd);

/* Renders with host buffers. background: per pt_render_params.background_rows. rgb: height x width
 * x 3 bytes, only pixels of the slice that belong to this tile rank are written. linear (optional):
 * height x width x 3 doubles, the sample mean before gamma (render.rs:45). */
int pt_render(pt_context *ctx, const pt_camera *camera, const double *background, const pt_render_params *params,
              uint8_t *rgb, double *linear, pt_stats *stats);

/* Same, writing into DEVICE memory on `hip_stream` (a hipStream_t, or NULL for the default stream)
 * without synchronising the host: d_rgb is either the full image (compact = 0) or this rank's tiles
 * only, tile-major, 8 x 8 x 3 bytes per tile (compact = 1; size = pt_compact_bytes()). The
 * background must already be resident: d_background is a DEVICE pointer. stats (optional) are
 * filled only if the call is followed by pt_render_finish(). */
int pt_render_device(pt_context *ctx, const pt_camera *camera, const double *d_background, const pt_render_params *params,
                     int compact, void *d_rgb, void *hip_stream);
int pt_render_finish(pt_context *ctx, pt_stats *stats);
/* (ABI 8) Two renders of a context may be in flight at once - pt_render_device, pt_render_device, pt_render_finish (the OLDER one), ... - and since
 * ABI 8 each of the two owns its work buffers, so that they may also run on two streams: pt_context_stream(ctx, k) is the context's own
 * non-blocking stream (a hipStream_t) for the render that takes slot k & 1; pt_context_next_slot() says which slot the next pt_render_device
 * takes (they are taken in turn). The render kernels are persistent: a frame's wavefronts retire one by one over the duration of its longest work
 * items, and a next frame queued on the OTHER stream starts in the places they free instead of waiting for the last of them (the reference
 * renders one image per call, src/render.rs:93-151; consecutive calls are independent, which is what lets two be in flight). For scenes whose
 * kernels park recursion frames in HBM both slots get the SAME stream (two launches at once cost such scenes more than the tail is worth). */
void *pt_context_stream(pt_context *ctx, int slot);
int pt_context_next_slot(const pt_context *ctx);

/* ---- Primary visibility: what is under each pixel. ONE primary ray per pixel of the slice - Camera::ray_at(x + offset[0], y + offset[1]),
 * camera.rs:48-84; (0.5, 0.5) is the pixel centre PT_SAMPLE_CENTRE uses -, its nearest hit over [EPSILON, inf) in the traversal the scene was
 * uploaded with, no shading, no lights, no secondary rays, no random numbers. Every buffer is OPTIONAL (NULL = not wanted, and nothing is computed
 * for it), a full image, row-major; pixels outside the slice are left untouched. Every value carries the bits the render path computes on its way to
 * the pixel's colour:
 *   depth     width x height      f64  ray parameter t of the nearest hit (ray.rs:87-99)                          miss: +inf
 *   position  width x height x 3  f64  world-space hit point (flat_scene.rs:85-95 / scene.rs:100-112)             miss: 0, 0, 0
 *   normal    width x height x 3  f64  world-space normal, normalised (material.rs:123-125), BEFORE a normal map   miss: 0, 0, 0
 *   node      width x height      i32  flattened node index (breadth-first, as in pt_scene)                       miss: -1
 *   sub       width x height      i32  MESH / KDMESH: index of the triangle inside its mesh; else 0               miss: -1
 *   material  width x height      i32  the node's material index: pt_scene.material[node], as uploaded             miss: -1
 * Errors: PT_ERR_ARGUMENT (NULL context / camera / params, all six buffers NULL, a non-finite offset), PT_ERR_NO_SCENE, PT_ERR_SLICE - all before
 * the first HIP call - and PT_ERR_TRAVERSAL as for a render. The pass has work buffers of its own: renders in flight on the context's two slots
 * are not disturbed, and trees of any depth a render accepts are walked (the stack continues in HBM). */
typedef struct {
    uint32_t width, height;     /* Image::width / height                                                 */
    pt_rect slice;              /* pixels to trace; an inverted slice traces nothing (render.rs:60-65)    */
    double offset[2];           /* sample position inside the pixel, x then y                            */
} pt_aov_params;
typedef struct { double *depth; double *position; double *normal; int32_t *node; int32_t *sub; int32_t *material; } pt_aov_buffers;
/* Host buffers, synchronous. kernel_ms (optional): device time of the kernel (HIP events). */
int pt_aov(pt_context *ctx, const pt_camera *camera, const pt_aov_params *params, const pt_aov_buffers *host_out, double *kernel_ms);
/* The same into DEVICE memory, queued on `hip_stream` (a hipStream_t, or NULL for the default stream) without synchronising the host.
 * pt_aov_finish waits for that pass and returns what it found (PT_ERR_TRAVERSAL, else PT_OK) and, optionally, its kernel time; one pass
 * may be in flight per context: a second pt_aov_device / pt_aov before pt_aov_finish is refused with PT_ERR_ARGUMENT. */
int pt_aov_device(pt_context *ctx, const pt_camera *camera, const pt_aov_params *params, const pt_aov_buffers *device_out, void *hip_stream);
int pt_aov_finish(pt_context *ctx, double *kernel_ms);

/* ---- Guides: what a denoiser needs of each pixel, in ONE trace. The pass is pt_aov's - the same pt_aov_params, the same primary ray at
 * (x + offset[0], y + offset[1]), the same nearest hit over [EPSILON, inf), no shading, no lights, no secondary rays, no random numbers - with the diffuse
 * colour under the pixel beside three of pt_aov's buffers. Every buffer is OPTIONAL (NULL = not wanted), a full image, row-major; pixels outside the slice
 * are left untouched.
 *   albedo    width x height x 3  f64  diffuse_color of material.rs:137-143 at the primary hit, in the bits the render path uses: the material's diffuse,
 *                                      or, where the material has a texture, the three srgb_lut entries of the hit's texel (fetched at uv_trans * uv).
 *                                      It is the FIRST hit's colour, whatever the material (a mirror's or a glass's own diffuse).  miss: +0, +0, +0
 *   position, normal, node             as in pt_aov, the same bits and miss values (normal: BEFORE a normal map)
 * Errors: pt_aov's, with "all four buffers NULL" in place of "all six" - all before the first HIP call - and PT_ERR_TRAVERSAL as for a render.
 * The pass runs on pt_aov's pass object and shares its work buffers: a guides pass and an aov pass exclude each other, ONE of the two in flight per
 * context (the second is refused with PT_ERR_ARGUMENT), and pt_guides_finish and pt_aov_finish are the same function - either closes whichever is open. */
typedef struct { double *albedo; double *position; double *normal; int32_t *node; } pt_guides_buffers;
/* Host buffers, synchronous; only the slice's rectangle is copied back. kernel_ms (optional): device time of the kernel (HIP events). */
int pt_guides(pt_context *ctx, const pt_camera *camera, const pt_aov_params *params, const pt_guides_buffers *host_out, double *kernel_ms);
/* The same into DEVICE memory, queued on `hip_stream` without synchronising the host; pt_guides_finish waits for it, as pt_aov_finish does. */
int pt_guides_device(pt_context *ctx, const pt_camera *camera, const pt_aov_params *params, const pt_guides_buffers *device_out, void *hip_stream);
int pt_guides_finish(pt_context *ctx, double *kernel_ms);

/* ---- Ray queries: rays the CALLER supplies (the crate's public Ray / RayCast::ray_cast, ray.rs, kdmesh.rs:99-166) - picking from a point other than
 * the eye, visibility between points, ambient-occlusion and light-map baking, range sensors, cameras the crate does not have. `origins` and
 * `directions` are n x 3 f64 in world space; a direction is used as given, NOT normalised, and t is the ray parameter along it. Per ray, in the
 * traversal the scene was uploaded with:
 *   any_hit = 0   the nearest hit over [EPSILON, inf). Every buffer is OPTIONAL (NULL = not wanted, and nothing is computed for it), n entries, indexed
 *                 like the input; t / position / normal / node / sub / material mean exactly what depth / position / normal / node / sub / material
 *                 mean in pt_aov, miss values included (+inf; 0, 0, 0; -1), and carry the same bits. occluded (u8) = node >= 0.
 *   any_hit = 1   is anything in the way over [EPSILON, inf) (the shadow rays' question, material.rs:171-179): occluded = 1 or 0. ONLY `occluded` may be
 *                 asked for - which occluder a walk meets first depends on how rays are scheduled, so it is not part of the contract.
 * The range is [EPSILON, inf) as everywhere in this code base; pt_segments (below) is this pass over a bounded segment [EPSILON, t_max) per ray.
 * Rays that are NOT TRACED report a miss (occluded = 0), occupy no lane of the walk and change no other ray's result: a ray with a non-finite component,
 * with an all-zero direction, or with a component of origin or direction beyond 1e18 in magnitude. The last rule keeps the f32 constants of the walks'
 * conservative box test finite and their error margins valid (the reciprocal of a direction component and its product with the origin stay inside the f32
 * range; 1e18 is also the bound pt_scene_upload puts on box coordinates). Direction components BELOW 1e-18 in magnitude need no such rule: the box test
 * then ignores that axis, which stays conservative, and the exact f64 primitive tests decide.
 * reorder: 0 = 64 consecutive rays share a wavefront, whose one tree walk pays for the union of their paths; 1 = the device first sorts the rays by
 *   (direction octant, Morton code of the origin inside the scene tree's root box; radix sort) and wavefronts take 64 consecutive rays of THAT order. Results are
 *   bit-identical either way and are written at the caller's index; kernel_ms covers keying, sort and cast. Coherent batches (camera rays in pixel order,
 *   anything already grouped) gain nothing and pay the sort, about 16 bytes of extra traffic per ray per radix pass; it is meant for large batches in
 *   no useful order (bounce rays). From which batch size and degree of disorder on it wins has not been measured yet: this is
 *   the byte count of profiles/rays/notes.md section 2, whose measure.py is the script to settle it with. Measured since (profiles/ao/notes.md): ambient-occlusion
 *   rays with a point's rays next to each other, points in pixel order, are NOT such a batch - at 33 M rays reorder = 1 is 1.3 to 4.1 x slower there.
 * Errors, before the first HIP call: PT_ERR_ARGUMENT (NULL context / params / origins / directions; no buffer asked for; n > PT_RAYS_MAX; any_hit or
 * reorder other than 0 or 1; any_hit = 1 with a buffer other than `occluded`), PT_ERR_NO_SCENE. n = 0 is PT_OK: nothing is launched or written. During the
 * pass: PT_ERR_TRAVERSAL as for a render; trees of any depth a render accepts are walked (the stack continues in HBM). The pass has work buffers of its own:
 * renders in flight on the context's two slots and a pt_aov_device pass are not disturbed. */
#define PT_RAYS_MAX 0x40000000ull   /* rays per call (2^30) */
typedef struct {
    uint64_t n;        /* rays                                                                        */
    int32_t any_hit;   /* 0: nearest hit; 1: occlusion query                                          */
    int32_t reorder;   /* 0: caller's order; 1: the device groups like rays first (see above)         */
} pt_rays_params;
typedef struct { double *t; double *position; double *normal; int32_t *node; int32_t *sub; int32_t *material; uint8_t *occluded; } pt_rays_buffers;
/* Host buffers, synchronous: uploads the rays, copies back the buffers asked for. kernel_ms (optional): device time of the pass (HIP events). */
int pt_rays(pt_context *ctx, const pt_rays_params *params, const double *origins, const double *directions, const pt_rays_buffers *host_out, double *kernel_ms);
/* The same with rays and results in DEVICE memory, queued on `hip_stream` (a hipStream_t, or NULL for the default stream) without synchronising the
 * host. pt_rays_finish waits for that pass and returns what it found (PT_ERR_TRAVERSAL, else PT_OK) and, optionally, its device time; one pass may be
 * in flight per context: a second pt_rays_device / pt_rays before pt_rays_finish is refused with PT_ERR_ARGUMENT. (n = 0 queues nothing and is not in flight.) */
int pt_rays_device(pt_context *ctx, const pt_rays_params *params, const double *d_origins, const double *d_directions, const pt_rays_buffers *device_out, void *hip_stream);
int pt_rays_finish(pt_context *ctx, double *kernel_ms);

/* ---- Ray queries over bounded SEGMENTS: pt_rays with a t_max per ray (n f64, in units of the ray's direction, like t) - visibility between two points
 * (direction = b - a, t_max = 1), ambient occlusion inside a closed room, range sensors. Per ray the result is that of pt_rays restricted to hits with
 * EPSILON <= t < t_max, in every buffer:
 *   any_hit = 0   the nearest hit if its t < t_max, else the miss values.
 *   any_hit = 1   occluded = 1 iff such a hit exists.
 * t_max = +inf gives pt_rays' bits exactly. A ray whose t_max is NaN or <= PT_EPSILON has an empty range: it is NOT TRACED - reports a miss, occupies no
 * lane of the walk and changes no other ray's result - like the rays pt_rays does not trace, whose rules hold here too.
 * In the flat_scene and hierarchical semantics this is the crate's ray_cast(&ray, &mut Range {start: EPSILON, end: t_max}): a primitive returns its smallest
 * root in range, a mesh is entered whenever a triangle could still be hit inside the range (BoundingBox::test_hit, bounding_box.rs:104-116: also by a ray
 * that starts inside the box whose far face lies beyond t_max), exact ties keep their winner. The walks start with the bound and prune with it: boxes beyond
 * t_max are never entered, and an occlusion query ends at the first hit inside the range. Two exceptions, for the reason of the next paragraph - both are tests
 * whose outcome for a hit just inside the bound depends on more than the exact comparison t < t_max, so that the crate's bounded cast would lose hits pt_rays
 * reports: a KDMesh's own triangle k-d tree (kdmesh.rs; its classification of a split's sides reads the range's END - hits on a split plane within EPSILON of
 * t_max) and a Mesh's box test (bounding_box.rs:104-116; the box's entry parameter is rounded differently from a triangle's t - triangles lying IN a face of the
 * box, t_max an ulp behind them). While nothing is found yet both get the range an unbounded walk would give them, and the hit is kept iff t < t_max.
 * In the k-d semantics the crate's own bounded range would enter the split classification (node.rs:121) and could differ in quirk cases; the contract here
 * is BY DEFINITION the unbounded walk's result, filtered by t < t_max. The walk is therefore not pruned and runs as a nearest-hit walk for any_hit = 1 as
 * well (an occlusion walk may stop at an occluder beyond t_max while a nearer one sits in another leaf): a bound saves no time in these semantics.
 * params, buffers, reorder (pt_rays' sort, unchanged: the bound is not part of the key) and kernel_ms as in pt_rays. The pass IS a ray-query pass: it shares
 * pt_rays' work buffers and its one pass in flight - pt_segments_device is closed by pt_rays_finish, and while a pt_rays_device or pt_segments_device pass
 * is open a second one of either kind (or pt_rays / pt_segments) is PT_ERR_ARGUMENT.
 * Errors, before the first HIP call: PT_ERR_ARGUMENT for a NULL t_max, and pt_rays' errors. n = 0 is PT_OK. */
int pt_segments(pt_context *ctx, const pt_rays_params *params, const double *origins, const double *directions, const double *t_max, const pt_rays_buffers *host_out,
                double *kernel_ms);
int pt_segments_device(pt_context *ctx, const pt_rays_params *params, const double *d_origins, const double *d_directions, const double *d_t_max,
                       const pt_rays_buffers *device_out, void *hip_stream);

/* ---- Ambient occlusion: how much of the hemisphere above a point is blocked within `radius`. The caller gives POINTS - n positions and n normals, n x 3 f64 in
 * world space, what pt_aov writes per pixel or a baker's texel centres - and the device makes each point's `samples` rays in registers, walks them as occlusion
 * queries over [EPSILON, radius) and counts. No ray is ever in memory: 48 bytes per point in, at most 29 out.
 * The rays are a CONTRACT, a fixed sequence of correctly rounded f64 operations (portrayer_amd/csrc/pt_ao.h states it; pt_test_ao_rays_host replays it on the
 * host). Point i has the stream index q = first_index + i, and in this order:
 *   1. valid      all six components finite and at most 1e18 in magnitude (pt_rays' rule) and the normal not (0, 0, 0). An INVALID point traces nothing, occupies
 *                 no lane of a walk and reports occluded = 0, valid = 0, bent = (0, 0, 0) - so pt_aov's miss pixels are invalid points.
 *   2. face eye   with PT_AO_FACE_EYE: v = P - eye per component; if dot(N, v) > 0 then N = -N. (dot: (x x' + y y') + z z', as everywhere.)
 *   3. normalise  n = N / sqrt(dot(N, N)), a component-wise division.
 *   4. rotation   j = (uint32)(rng(seed, q, pass, draw 0) * 256.0), the render's counter-based generator; (c, s) = PT_AO_ROT[j] = (cos, sin) of 2 pi (j + 0.5) / 256.
 *   5. local      for k = 0 .. samples - 1 with (x, y, z) = PT_AO_DIRS[k]: lx = c x - s y, ly = s x + c y, lz = z. PT_AO_DIRS: 64 cosine-weighted directions
 *                 about +z, every power-of-two prefix stratified (pt_ao_tables.h; tools/gen_ao_tables.py).
 *   6. frame      sg = copysign(1, n.z); a = -1 / (sg + n.z); b = (n.x n.y) a; T = (1 + ((sg n.x) n.x) a, sg b, -(sg n.x)); B = (b, sg + (n.y n.y) a, -n.y).
 *   7. direction  d = (T lx + B ly) + n lz per component, not renormalised.
 *   8. origin     o = P + n bias.
 *   9. occlusion  occ_k = what pt_segments with any_hit = 1 answers for (o, d, t_max = radius) in the scene's traversal - that definition taken over whole, with
 *                 its exceptions for the k-d semantics, KDMesh trees and mesh boxes, and its rule for rays that are not traced. radius = +inf is pt_rays.
 * Outputs per point, each OPTIONAL (NULL = not wanted), at least one:
 *   occluded  n      u32  the sum of occ_k
 *   valid     n      u8   step 1
 *   bent      n x 3  f64  starting from (0, 0, 0), the sum of d_k over the k with occ_k = 0 in ascending k, left to right, not normalised
 * The bits do not depend on how a batch is cut - a slice [k, k + m) submitted with first_index + k equals that slice of the whole - nor on the work layout the
 * kernel runs in (PORTRAYER_AO_LAYOUT=point|sample picks it at the launch). Another `pass` draws another rotation: a caller sums passes for more than
 * 64 rays per point.
 * The pass IS a ray-query pass: it shares pt_rays' work buffers and its one pass in flight - pt_ao_device is closed by pt_ao_finish, which is pt_rays_finish, and
 * while a pt_rays_device / pt_segments_device / pt_ao_device pass is open a second one of any kind is PT_ERR_ARGUMENT.
 * Errors, before the first HIP call: PT_ERR_ARGUMENT (a NULL context / params / positions / normals / buffers; no buffer asked for; n > PT_AO_MAX; samples not a
 * power of two <= 64; radius NaN or <= PT_EPSILON; bias negative or not finite; flags other than PT_AO_FACE_EYE; PT_AO_FACE_EYE with a non-finite eye),
 * PT_ERR_NO_SCENE. n = 0 is PT_OK: nothing is launched or written. During the pass: PT_ERR_TRAVERSAL as for a render. */
#define PT_AO_FACE_EYE 1u                 /* pt_ao_params.flags: turn each normal towards `eye` first (step 2) */
#define PT_AO_MAX (PT_RAYS_MAX / 64)      /* points per call (2^24): PT_RAYS_MAX rays at 64 samples            */
typedef struct {
    uint64_t n;             /* points, <= PT_AO_MAX                                          */
    uint32_t samples;       /* rays per point: 1, 2, 4, 8, 16, 32 or 64                      */
    uint32_t pass;          /* which rotation a point draws                                  */
    uint64_t seed;
    uint64_t first_index;   /* stream index of point 0                                       */
    double radius;          /* > EPSILON; +inf allowed                                       */
    double bias;            /* finite, >= 0: the origin is lifted by bias along the normal   */
    uint32_t flags;         /* 0 or PT_AO_FACE_EYE                                           */
    double eye[3];          /* read with PT_AO_FACE_EYE only                                 */
} pt_ao_params;
typedef struct { uint32_t *occluded; uint8_t *valid; double *bent; } pt_ao_buffers;
/* Host buffers, synchronous: uploads the points, copies back the buffers asked for. kernel_ms (optional): device time of the pass (HIP events). */
int pt_ao(pt_context *ctx, const pt_ao_params *params, const double *positions, const double *normals, const pt_ao_buffers *host_out, double *kernel_ms);
/* The same with points and results in DEVICE memory, queued on `hip_stream` (a hipStream_t, or NULL for the default stream) without synchronising the host -
 * behind a pt_aov_device on the same stream it reads that pass's position and normal, and nothing per pixel crosses the bus but the results. */
int pt_ao_device(pt_context *ctx, const pt_ao_params *params, const double *d_positions, const double *d_normals, const pt_ao_buffers *device_out, void *hip_stream);
int pt_ao_finish(pt_context *ctx, double *kernel_ms);
/* Test hooks, no context and no GPU. pt_test_ao_rays_host: steps 1 to 8 on the host, by the functions the kernel compiles: origins and directions n x samples x 3
 * (point-major; zeros for an invalid point), valid n. Checks params as pt_ao does (PT_ERR_ARGUMENT). pt_test_ao_tables: the library's PT_AO_DIRS (192) and PT_AO_ROT (512). */
int pt_test_ao_rays_host(uint64_t n, const pt_ao_params *params, const double *positions, const double *normals, double *origins, double *directions, uint8_t *valid);
int pt_test_ao_tables(double *dirs, double *rot);

/* ---- Radiance: rays the CALLER supplies, SHADED (the crate's public Ray::color(scene, background, 0), ray.rs:139-148) - cameras the crate does not have
 * (fisheye, panoramic, orthographic, thin lens), light probes and environment captures from a point inside the scene, one more gathered bounce for a baker
 * that casts its own rays, samplers that choose which samples to trace. Rays as in pt_rays: n x 3 f64 origins and directions in world space, a direction used
 * as given, NOT normalised. rgb[i] (n x 3 f64) carries the bits of Ray::color for ray i against ITS background colour, in the traversal the scene was uploaded
 * with: everything pt_render shades - Blinn-Phong with shadow rays, area lights, glossy reflection, reflection and refraction to depth 10, textures and normal
 * maps - as one linear sample: no mean, no gamma, no clamp. Accumulation is the caller's.
 *   background: 3 doubles (background_per_ray = 0), or n x 3 indexed like the rays (1).
 *   random draws (area lights, glossy reflection) of ray i come from the counter-based generator's stream (seed, stream_base + i, sample), draws 2, 3, ...: the
 *     numbering a render uses behind its two jitter draws. With stream_base = 0 and the rays a full image's pixel centres in pixel order the result is pt_render's
 *     `linear` at samples = 1, PT_SAMPLE_CENTRE and the same seed (background per pixel passed per ray); sample = s gives sample s of that pixel.
 *   The stream belongs to the ray's INDEX, not to where it runs: results are bit-identical with reorder 0 and 1 (as in pt_rays), and a sub-batch [k, k + m)
 *     submitted with stream_base = k equals that slice of the whole batch.
 *   Rays that are NOT TRACED (pt_rays' rule: a non-finite component, an all-zero direction, a component beyond 1e18) report their background colour and disturb
 *     no other ray.
 * Errors, before the first HIP call: PT_ERR_ARGUMENT (NULL context / params / origins / directions / background / rgb; n > PT_RAYS_MAX; reorder or
 * background_per_ray other than 0 or 1), PT_ERR_NO_SCENE. n = 0 is PT_OK: nothing is launched or written. During the pass: PT_ERR_TRAVERSAL as for a render.
 * The pass has work buffers of its own (stack columns, recursion frames, queues, sort keys): renders in flight on the context's two slots, a pt_aov_device
 * pass and a pt_rays_device pass are not disturbed. kernel_ms covers keying and sort (reorder = 1) and the shading kernel. */
typedef struct {
    uint64_t n;                  /* rays, <= PT_RAYS_MAX                                                        */
    int32_t  reorder;            /* as pt_rays_params.reorder                                                   */
    int32_t  background_per_ray; /* 0: background is 3 doubles; 1: n x 3, indexed like the rays                 */
    uint64_t seed;               /* key of the counter-based generator, as pt_render_params.seed                */
    uint64_t stream_base;        /* ray i draws from stream (seed, stream_base + i, sample), draws 2, 3, ...    */
    uint32_t sample;
} pt_radiance_params;
/* Host buffers, synchronous: uploads rays and background, copies rgb back. kernel_ms (optional): device time of the pass (HIP events). */
int pt_radiance(pt_context *ctx, const pt_radiance_params *params, const double *origins, const double *directions, const double *background, double *rgb, double *kernel_ms);
/* The same with every array in DEVICE memory, queued on `hip_stream` (a hipStream_t, or NULL for the default stream) without synchronising the host.
 * pt_radiance_finish waits for that pass and returns what it found (PT_ERR_TRAVERSAL, else PT_OK) and, optionally, its device time; one pass may be in flight
 * per context: a second pt_radiance_device / pt_radiance before pt_radiance_finish is refused with PT_ERR_ARGUMENT. (n = 0 queues nothing and is not in flight.) */
int pt_radiance_device(pt_context *ctx, const pt_radiance_params *params, const double *d_origins, const double *d_directions, const double *d_background, double *d_rgb, void *hip_stream);
int pt_radiance_finish(pt_context *ctx, double *kernel_ms);

/* ---- Gather: the light that arrives at a point from the hemisphere above it - sky and one bounce of everything pt_render shades - as the SUM of `samples`
 * shaded radiance samples along the ambient-occlusion pass's rays. pt_ao can only count what a point's rays meet, pt_radiance shades rays the caller has to make
 * and ship (48 bytes per ray up, 24 down); this pass joins them on the device: POINTS in - n positions and n normals, n x 3 f64 in world space, what pt_aov
 * writes per pixel or a baker's texel centres - and per point one sum out. No ray and no per-ray colour is ever in memory: 48 bytes per point in, at most 25 out.
 * The result is defined, to the bit, by the two contracts that exist. Point i has the stream index q = first_index + i, S = samples, and in this order:
 *   1. - 8.       pt_ao's steps 1 to 8, unchanged and computed by the same functions (portrayer_amd/csrc/pt_ao.h; pt_test_ao_rays_host replays them): valid, face
 *                 eye, normalise, rotation from rng(seed, q, pass, draw 0), local direction from PT_AO_DIRS[k] and PT_AO_ROT[j], frame, direction d_k, origin
 *                 o_k = P + n bias. There is no radius: a gather ray is unbounded, as a radiance ray is.
 *   9. radiance   rgb_k = what pt_radiance answers for the ray (o_k, d_k) with `background` (3 doubles, the sky: what a ray that leaves the scene brings back), the
 *                 generator's stream (seed, q * S + k, sample = pass), draws 2, 3, ... - that definition taken over whole: textures and normal maps, area lights,
 *                 glossy draws, reflection and refraction to depth 10, and its rule that a ray which is NOT TRACED (a component beyond 1e18 or not finite - a
 *                 huge bias can do that to an origin) reports the background. q * S + k is a 64-bit product, reduced modulo 2^64 only.
 * Outputs per point, each OPTIONAL (NULL = not wanted), at least one:
 *   sum    n x 3  f64  starting from (0, 0, 0), rgb_k added per channel in ascending k, left to right. The mean is sum / S; the directions are cosine-weighted, so
 *                      the irradiance estimate is pi x the mean.
 *   valid  n      u8   step 1
 * An INVALID point traces nothing, occupies no lane of a walk and reports sum = (0, 0, 0), valid = 0 - so pt_aov's miss pixels are invalid points.
 * Consequences: the bits do not depend on how a batch is cut - a slice [k, k + m) submitted with first_index + k equals that slice of the whole - nor on which
 * rays share a wavefront; and the pass equals pt_radiance on pt_test_ao_rays_host's rays (same seed, pass, first_index, bias, flags, eye; any radius), flattened
 * point-major, with stream_base = first_index * S and sample = pass, summed in that order. Another `pass` gives other rays and other draws: a caller sums passes.
 * The pass runs on the RADIANCE pass object and its work buffers, as a film's add does: pt_gather_device is closed by pt_gather_finish, which is
 * pt_radiance_finish, and while a pt_radiance_device / pt_film_add_device / pt_film_add_map_device / pt_gather_device pass is open a second one of any kind
 * is PT_ERR_ARGUMENT. Renders on the context's two slots, a pt_aov_device pass and a pt_rays_device pass are not disturbed.
 * Errors, before the first HIP call: PT_ERR_ARGUMENT (a NULL context / params / positions / normals / background / buffers; no buffer asked for; n > PT_AO_MAX;
 * samples not a power of two <= 64; bias negative or not finite; flags other than PT_AO_FACE_EYE; PT_AO_FACE_EYE with a non-finite eye), PT_ERR_NO_SCENE.
 * n = 0 is PT_OK: nothing is launched or written. During the pass: PT_ERR_TRAVERSAL as for a render. */
typedef struct {
    uint64_t n;             /* points, <= PT_AO_MAX                                          */
    uint32_t samples;       /* rays per point: 1, 2, 4, 8, 16, 32 or 64                      */
    uint32_t pass;          /* which rotation a point draws, and the `sample` of its streams */
    uint64_t seed;
    uint64_t first_index;   /* stream index of point 0                                       */
    double bias;            /* finite, >= 0: the origin is lifted by bias along the normal   */
    uint32_t flags;         /* 0 or PT_AO_FACE_EYE                                           */
    double eye[3];          /* read with PT_AO_FACE_EYE only                                 */
} pt_gather_params;
typedef struct { double *sum; uint8_t *valid; } pt_gather_buffers;
/* Host buffers, synchronous: uploads the points, copies back the buffers asked for. kernel_ms (optional): device time of the pass (HIP events). */
int pt_gather(pt_context *ctx, const pt_gather_params *params, const double *positions, const double *normals, const double *background,
              const pt_gather_buffers *host_out, double *kernel_ms);
/* The same with points and results in DEVICE memory, queued on `hip_stream` (a hipStream_t, or NULL for the default stream) without synchronising the host -
 * behind a pt_aov_device on the same stream it reads that pass's position and normal, and nothing per pixel crosses the bus but the results. `background` stays
 * a HOST pointer to 3 doubles: it is read during the call and travels in the kernel's argument block. */
int pt_gather_device(pt_context *ctx, const pt_gather_params *params, const double *d_positions, const double *d_normals, const double *background,
                     const pt_gather_buffers *device_out, void *hip_stream);
int pt_gather_finish(pt_context *ctx, double *kernel_ms);

/* ---- Direct light: the light that reaches a point straight from the scene's LIGHTS, the term pt_gather cannot give (its rays sample the hemisphere by cosine and
 * never meet a point light or a small area light). POINTS in - n positions and n normals, n x 3 f64 in world space, what pt_aov writes per pixel or pt_chart per
 * texel - and the device makes each point's shadow rays at the resident scene's L lights (15 doubles each: position, colour, falloff c0 c1 c2, area a, area b; kept
 * current by pt_scene_update) in registers, walks them as occlusion queries and sums what arrives. No ray and no term is ever in memory: 48 bytes per point in, at
 * most 29 out.
 * The result is a CONTRACT, a fixed sequence of correctly rounded f64 operations (+, -, *, /, sqrt, fmax; no fused multiply-add; portrayer_amd/csrc/pt_direct.h
 * states it; pt_test_direct_host replays it on the host). Point i has the stream index q = first_index + i, S = samples, and in this order:
 *   1. valid      pt_ao's step 1: all six components finite and at most 1e18 in magnitude and the normal not (0, 0, 0). An INVALID point traces nothing, occupies
 *                 no lane of a walk and reports sum = (0, 0, 0), lit = 0, valid = 0 - so pt_aov's miss pixels and pt_chart's unowned texels are invalid points.
 *   2. face eye   with PT_AO_FACE_EYE, as pt_ao's step 2: v = P - eye per component; if dot(N, v) > 0 then N = -N. (dot: (x x' + y y') + z z', as everywhere.)
 *   3. normalise  nrm = N / sqrt(dot(N, N)), a component-wise division, as pt_ao's step 3.
 *   4. origin     o = P + nrm bias.
 *   5. light      light li is a POINT light iff a == (0, 0, 0) or b == (0, 0, 0) (light.rs:51-53): lpos = position for every k. Else lpos = position + (a ca + b cb)
 *                 with ca = 2 rng(seed, q S + k, pass, draw 2 j) - 1 and cb = 2 rng(seed, q S + k, pass, draw 2 j + 1) - 1, the render's counter-based generator;
 *                 j = the number of area lights with an index below li (the render's rule: an area light consumes two draws, a point light none). q S + k is a
 *                 64-bit product and sum, reduced modulo 2^64 only.
 *   6. shadow ray v = lpos - o; dist = sqrt(dot(v, v)); d = v / dist; t_max = +inf: the render's shadow ray (material.rs:149-179), which anything along the ray
 *                 shadows, also behind the light. With PT_DIRECT_TO_LIGHT t_max = dist: the segment ends at the light - what a baker wants.
 *   7. cosine     c = fmax(dot(nrm, d), 0). A sample with c == 0 or c NaN (a light at the point) contributes nothing and casts no ray.
 *   8. occlusion  otherwise occ = what pt_segments with any_hit = 1 answers for (o, d, t_max) in the scene's traversal - that definition taken over whole, with its
 *                 exceptions for the k-d semantics, KDMesh trees and mesh boxes. A ray that pass would not trace (a component of o beyond 1e18 - a huge bias can do
 *                 that - or t_max <= EPSILON) contributes nothing.
 *   9. term       att = (c0 + c1 dist) + (c2 dist) dist (light.rs:31-33); term = (colour c) / att per channel. No material enters: the result is incident light
 *                 weighted by the cosine, and a caller multiplies by the albedo pt_guides gives.
 *  10. sum        starting from (0, 0, 0) and lit = 0, for li ascending and inside that k = 0 .. S - 1 ascending: where the sample contributes and occ == 0,
 *                 sum += term (per channel, left to right) and lit += 1. A point light's sample is the same for every k: it is traced ONCE and added S times, so
 *                 that sum / S is the estimate whatever mix of lights a scene has. In a scene of point lights only, S = 1 is what to ask for.
 * Outputs per point, each OPTIONAL (NULL = not wanted), at least one:
 *   sum    n x 3  f64  step 10
 *   lit    n      u32  step 10: at most L x S
 *   valid  n      u8   step 1
 * A scene without lights gives zeros and step 1's valid, and walks nothing.
 * Consequences: the bits do not depend on how a batch is cut - a slice [k, k + m) submitted with first_index + k equals that slice of the whole - nor on the work
 * layout, nor on which rays share a wavefront; and the pass equals pt_test_direct_host's terms, added in step 10's order where pt_segments (any_hit = 1) on that
 * hook's rays reports no occluder.
 * The pass IS a ray-query pass, as pt_ao is: it shares pt_rays' work buffers and its one pass in flight - pt_direct_device is closed by pt_direct_finish, which is
 * pt_rays_finish, and while a pt_rays_device / pt_segments_device / pt_ao_device / pt_direct_device pass is open a second one of any kind is PT_ERR_ARGUMENT.
 * Errors, before the first HIP call: PT_ERR_ARGUMENT (a NULL context / params / positions / normals / buffers; no buffer asked for; n > PT_AO_MAX; samples not a
 * power of two <= 64; bias negative or not finite; flags other than PT_AO_FACE_EYE | PT_DIRECT_TO_LIGHT; PT_AO_FACE_EYE with a non-finite eye), PT_ERR_NO_SCENE.
 * n = 0 is PT_OK: nothing is launched or written. During the pass: PT_ERR_TRAVERSAL as for a render. */
#define PT_DIRECT_TO_LIGHT 2u             /* pt_direct_params.flags: the shadow segment ends at the light (step 6) */
typedef struct {
    uint64_t n;             /* points, <= PT_AO_MAX                                          */
    uint32_t samples;       /* samples per area light: 1, 2, 4, 8, 16, 32 or 64              */
    uint32_t pass;          /* the `sample` of the points' streams                           */
    uint64_t seed;
    uint64_t first_index;   /* stream index of point 0                                       */
    double bias;            /* finite, >= 0: the origin is lifted by bias along the normal   */
    uint32_t flags;         /* any of PT_AO_FACE_EYE | PT_DIRECT_TO_LIGHT                    */
    double eye[3];          /* read with PT_AO_FACE_EYE only                                 */
} pt_direct_params;
typedef struct { double *sum; uint32_t *lit; uint8_t *valid; } pt_direct_buffers;
/* Host buffers, synchronous: uploads the points, copies back the buffers asked for. kernel_ms (optional): device time of the pass (HIP events). */
int pt_direct(pt_context *ctx, const pt_direct_params *params, const double *positions, const double *normals, const pt_direct_buffers *host_out, double *kernel_ms);
/* The same with points and results in DEVICE memory, queued on `hip_stream` (a hipStream_t, or NULL for the default stream) without synchronising the host -
 * behind a pt_aov_device or pt_chart_device on the same stream it reads that pass's position and normal, and nothing per point crosses the bus but the results.
 * After the checks above it holds every caller pointer to pt_check_device_pointer's rule - device memory of the context's device, and long enough - before
 * anything is queued (PT_ERR_ARGUMENT). */
int pt_direct_device(pt_context *ctx, const pt_direct_params *params, const double *d_positions, const double *d_normals, const pt_direct_buffers *device_out, void *hip_stream);
int pt_direct_finish(pt_context *ctx, double *kernel_ms);
/* Test hook, no context and no GPU: steps 1 to 7 and 9 (and step 8's rule for which rays are traced) on the host, by the functions the kernel compiles, against
 * `lights` (n_lights x 15). origins n x 3; directions and terms n x n_lights x S x 3; t_max n x n_lights x S; valid n. A sample that casts no ray - an invalid
 * point, c == 0 or NaN, a ray pt_segments would not trace - has direction (0, 0, 0), t_max 0 and term (0, 0, 0): pt_segments does not trace such a ray either, so
 * the arrays can be handed to it as they are. Checks params as pt_direct does (PT_ERR_ARGUMENT). */
int pt_test_direct_host(uint64_t n, const pt_direct_params *params, const double *positions, const double *normals, uint32_t n_lights, const double *lights,
                        double *origins, double *directions, double *t_max, double *terms, uint8_t *valid);

/* ---- Probe: the light field at a point in FREE SPACE - what lights a character, a prop or a particle that moves through a baked scene - as the nine order-2
 * spherical-harmonic (SH) sums of `samples` shaded radiance samples over the whole sphere about the point. pt_gather needs a normal and samples one hemisphere by
 * cosine with at most 64 rays; a caller who wants probes would make the sphere's rays on the host, ship 48 bytes per ray up through pt_radiance, pull 24 back and
 * project there. This pass does it on the device: PROBES in - n positions, n x 3 f64 in world space, no normals - and per probe 27 sums out. No ray and no
 * per-ray colour is ever in memory: 24 bytes per probe in, at most 217 out.
 * The result is a CONTRACT, a fixed sequence of correctly rounded f64 operations (+, -, *, /, sqrt; no fused multiply-add) that portrayer_amd/csrc/pt_probe.h
 * states as the functions the kernel compiles, over the tables of portrayer_amd/csrc/pt_probe_tables.h (tools/gen_probe_tables.py: every entry the exact value
 * rounded once) - PT_PROBE_DIRS[1024][3], uniform on the sphere: u = the base-2 radical inverse of k + 1/2048, v = Sobol dimension 2 of k + 1/2048, z = 1 - 2 u,
 * r = sqrt(1 - z z), the entry (r cos 2 pi v, r sin 2 pi v, z), every power-of-two prefix of 64 .. 1024 entries with equally many points per stratum of u and of
 * v; PT_PROBE_SH[5], the nearest doubles to 1 / (2 sqrt pi), sqrt(3 / (4 pi)), sqrt(15 / (4 pi)), sqrt(5 / (16 pi)), sqrt(15 / (16 pi)) - and pt_ao's PT_AO_ROT.
 * Probe i has the stream index q = first_index + i, S = samples, and in this order:
 *   1. valid      the three components of P finite and at most 1e18 in magnitude. An INVALID probe traces nothing, occupies no lane of a walk and reports zeros
 *                 and valid = 0.
 *   2. rotation   j = (uint32)(rng(seed, q, pass, draw 0) * 256), (c, s) = PT_AO_ROT[j]; m = (uint32)(rng(seed, q, pass, draw 1) * 1024), the axis
 *                 N = PT_PROBE_DIRS[m]: every probe turns the table its own way, so neighbouring probes do not share directions.
 *   3. direction  sample k takes (x, y, z) = PT_PROBE_DIRS[k], then pt_ao's steps 3, 5, 6 and 7 with that N: n = N / sqrt(dot(N, N)); lx = c x - s y,
 *                 ly = s x + c y, lz = z; the branch-free frame sg = copysign(1, n.z), a = -1 / (sg + n.z), b = (n.x n.y) a, T = (1 + ((sg n.x) n.x) a, sg b,
 *                 -(sg n.x)), B = (b, sg + (n.y n.y) a, -n.y); d_k = (T lx + B ly) + n lz per component, NOT renormalised. The origin is P itself: no bias, no
 *                 face-eye step.
 *   4. radiance   rgb_k = what pt_radiance answers for the ray (P, d_k) with `background` (3 doubles: what a ray that leaves the scene brings back), the
 *                 generator's stream (seed, q * S + k, sample = pass), draws 2, 3, ... - that definition taken over whole, as pt_gather takes it. q * S + k is
 *                 a 64-bit product, reduced modulo 2^64 only.
 *   5. basis      with d = d_k and c0 .. c4 = PT_PROBE_SH, every product left to right: Y0 = c0, Y1 = c1 d.y, Y2 = c1 d.z, Y3 = c1 d.x, Y4 = (c2 d.x) d.y,
 *                 Y5 = (c2 d.y) d.z, Y6 = c3 ((3 d.z) d.z - 1), Y7 = (c2 d.x) d.z, Y8 = c4 (d.x d.x - d.y d.y).
 *   6. sum        for coefficient i and channel c, per round r of 64 samples: the partial sum starts from 0 and adds Y_i(d_k) * rgb_k[c] for k = 64 r ..
 *                 64 r + 63 ascending; sh[i][c] is round 0's partial plus the later rounds' partials in ascending r, left to right.
 * Outputs per probe, each OPTIONAL (NULL = not wanted), at least one:
 *   sh     n x 9 x 3  f64  step 6. The estimate of SH coefficient i of channel c is sh[i][c] x 4 pi / S: that scaling is the caller's.
 *   valid  n          u8   step 1
 * Consequences: the bits do not depend on how a batch is cut - a slice [k, k + m) submitted with first_index + k equals that slice of the whole - nor on the
 * schedule; and the pass equals pt_radiance on pt_test_probe_host's rays, flattened probe-major, with stream_base = first_index * S and sample = pass, weighted
 * and added in step 6's order. Another `pass` gives other rotations and other draws: a caller sums passes.
 * The pass runs on the RADIANCE pass object and its work buffers, as pt_gather does: pt_probe_device is closed by pt_probe_finish, which is pt_radiance_finish,
 * and while a pt_radiance_device / pt_film_add_device / pt_film_add_map_device / pt_gather_device / pt_probe_device pass is open a second one of any kind is
 * PT_ERR_ARGUMENT. With S > 64 the partial sums of a probe's rounds wait in a scratch of the pass, at most 32 MiB: a call with more probes than that holds runs
 * as several launches inside the one open pass, which the first consequence makes invisible.
 * Errors, before the first HIP call: PT_ERR_ARGUMENT (a NULL context / params / positions / background / buffers; no buffer asked for; n > PT_PROBE_MAX; samples
 * not 64, 128, 256, 512 or 1024), PT_ERR_NO_SCENE. n = 0 is PT_OK: nothing is launched or written. During the pass: PT_ERR_TRAVERSAL as for a render. */
#define PT_PROBE_MAX (PT_RAYS_MAX / 1024)   /* probes per call (2^20): PT_RAYS_MAX rays at 1024 samples */
typedef struct {
    uint64_t n;             /* probes, <= PT_PROBE_MAX                                               */
    uint32_t samples;       /* rays per probe: 64, 128, 256, 512 or 1024                             */
    uint32_t pass;          /* which rotation a probe draws, and the `sample` of its streams         */
    uint64_t seed;
    uint64_t first_index;   /* stream index of probe 0                                               */
} pt_probe_params;
typedef struct { double *sh; uint8_t *valid; } pt_probe_buffers;
/* Host buffers, synchronous: uploads the positions, copies back the buffers asked for. kernel_ms (optional): device time of the pass (HIP events). */
int pt_probe(pt_context *ctx, const pt_probe_params *params, const double *positions, const double *background, const pt_probe_buffers *host_out, double *kernel_ms);
/* The same with positions and results in DEVICE memory, queued on `hip_stream` (a hipStream_t, or NULL for the default stream) without synchronising the host.
 * `background` stays a HOST pointer to 3 doubles: it is read during the call and travels in the kernel's argument block. */
int pt_probe_device(pt_context *ctx, const pt_probe_params *params, const double *d_positions, const double *background, const pt_probe_buffers *device_out,
                    void *hip_stream);
int pt_probe_finish(pt_context *ctx, double *kernel_ms);
/* Test hooks, no context and no GPU. pt_test_probe_host: steps 1 to 5 on the host, by the functions the kernel compiles: origins and directions n x samples x 3,
 * basis n x samples x 9 (Y0 .. Y8), valid n; an invalid probe's rays and basis values are zeros. PT_ERR_ARGUMENT for a NULL pointer or samples the pass refuses.
 * pt_test_probe_tables: the tables as the library holds them (dirs 1024 x 3, sh 5). */
int pt_test_probe_host(uint64_t n, const pt_probe_params *params, const double *positions, double *origins, double *directions, double *basis, uint8_t *valid);
int pt_test_probe_tables(double *dirs, double *sh);

/* ---- Chart: the texels of a mesh's light map as SURFACE POINTS - what pt_ao and pt_gather take (a position and a normal, 48 bytes), made on the device from
 * what is resident there: the triangle records (kept current by pt_scene_deform and pt_scene_deform_device), the node's composed matrices (kept current by
 * pt_scene_update) and a UV set. It does for surfaces what pt_aov does for cameras: behind pt_chart_device on the same stream pt_ao_device / pt_gather_device
 * read position and normal where they are, and a baker moves nothing per texel but the results.
 * `node` is a flattened node of type PT_PRIM_MESH or PT_PRIM_KDMESH; its mesh has T triangles (pt_chart_triangles). `uv` is T x 6 f64, per triangle the (u, v) of
 * its corners a, b, c - per CORNER, because a light-map unwrap splits vertices at seams. uv = NULL: the mesh's own texture coordinates, where the scene keeps
 * them on the device (a scene with a textured material, a mesh with mesh_has_texcoords); PT_ERR_ARGUMENT otherwise.
 * The points are a CONTRACT, a fixed sequence of correctly rounded f64 operations (portrayer_amd/csrc/pt_chart.h states it in ten steps; pt_test_chart_host
 * replays it on the host): a corner is (u width, (1 - v) height), rows top to bottom, no wrap; texel (x, y), index q = y width + x, is sampled at its centre; a
 * triangle with a non-finite corner, one beyond 2^24 texels, or no area owns nothing; the edge functions are evaluated from canonically ordered endpoints, so
 * two triangles that share an edge leave no texel centre between them, and coverage is inclusive; a texel belongs to the LOWEST triangle index that covers
 * it, whatever the schedule. Position and normal are interpolated by the weights (the normal: the vertex normals' where the node shades smoothly, else the
 * face's), taken to world space by the node's COMPOSED matrices in all three traversals, the normal normalised and, with PT_CHART_FLIP_NORMAL, negated.
 * Outputs, each OPTIONAL (NULL = not wanted), at least one, row-major over the map:
 *   position  width x height x 3  f64   not owned: +0, +0, +0
 *   normal    width x height x 3  f64   not owned: +0, +0, +0 - an invalid point for pt_ao and pt_gather: it traces nothing
 *   tri       width x height      i32   the owner, 0 .. T - 1, or -1
 *   covered   width x height      u8    1 or 0
 * The pass runs on pt_aov's pass object, as pt_guides does: ONE aov, guides or chart pass in flight per context (a second is PT_ERR_ARGUMENT), and
 * pt_chart_device is closed by pt_aov_finish. The owner map (4 bytes per texel) is a buffer of the context's, grown on demand.
 * Errors, before the first HIP call and in this order: PT_ERR_ARGUMENT (a NULL context / params / buffers; no buffer asked for; unknown flags; width or height
 * zero, or width x height > PT_AO_MAX), PT_ERR_NO_SCENE, PT_ERR_ARGUMENT (node >= the scene's nodes; a node that is no mesh; uv NULL for a mesh whose texture
 * coordinates are not on the device; a pass in flight). pt_chart_device then holds every caller pointer to pt_check_device_pointer's rule - device memory of the
 * context's device, 8-byte aligned, long enough - before any kernel is queued. */
#define PT_CHART_FLIP_NORMAL 1u
typedef struct { uint32_t node, width, height, flags; } pt_chart_params;
typedef struct { double *position; double *normal; int32_t *tri; uint8_t *covered; } pt_chart_buffers;
/* T of the node's mesh; the errors of pt_chart that concern the node. */
int pt_chart_triangles(pt_context *ctx, uint32_t node, uint64_t *n_tris);
/* Host buffers, synchronous: uploads `uv`, copies back the buffers asked for. kernel_ms (optional): device time of the three kernels (HIP events). */
int pt_chart(pt_context *ctx, const pt_chart_params *params, const double *uv, const pt_chart_buffers *host_out, double *kernel_ms);
/* The same with the UV set and the results in DEVICE memory, queued on `hip_stream` (a hipStream_t, or NULL for the default stream) without synchronising the
 * host; closed by pt_aov_finish. */
int pt_chart_device(pt_context *ctx, const pt_chart_params *params, const double *d_uv, const pt_chart_buffers *device_out, void *hip_stream);
/* Test hook, no context and no GPU: the contract on the host, by the functions the kernels compile. fwd: the node's 12 doubles, nrm: its 9; tri_v, tri_n: n_tris
 * 72-byte records (tri_n NULL: the node shades flat); uv n_tris x 6; outputs as above, host memory. */
int pt_test_chart_host(const double *fwd, const double *nrm, uint64_t n_tris, const double *tri_v, const double *tri_n, const double *uv, uint32_t width,
                       uint32_t height, uint32_t flags, const pt_chart_buffers *out);

/* ---- Film: a width x height accumulator in DEVICE memory that belongs to a context - a preview that sharpens, a render that can stop when it is good enough,
 * more samples where the image is noisy. Per pixel: `total` (3 f64, the sum of its complete 8-sample chunks), `partial` (3 f64, the sum of the open chunk) and
 * `count` (u32, samples taken so far): 52 bytes, nothing per sample.
 *   pt_film_add gives every pixel p of `slice` the samples count[p] .. count[p] + samples - 1, each taken exactly as pt_render takes that sample of that pixel
 *     (PT_SAMPLE_RNG: jitter from draws 0 and 1, x before y; PT_SAMPLE_CENTRE: (0.5, 0.5); the background at the integer pixel; draws 2, 3, ... along the
 *     recursion), and folds them in ascending order into total / partial the way a render's chunk sums associate.
 *   pt_film_resolve writes, for every pixel with count > 0, what pt_render writes with samples = count[p]: the mean as `linear` (width x height x 3 f64) and
 *     gamma, clamp, u8 as `rgb` (width x height x 3). Pixels with count == 0 are left untouched, as pt_render leaves pixels outside its slice.
 * PROMISE: if every pt_film_add to a film used the same camera, background, seed and sample mode and the resident scene did not change, rgb and linear at p
 * carry the bits of pt_render(samples = count[p]) - however the samples were split over calls and slices, in all three traversals. Mixing cameras or seeds
 * is not an error: the film adds what it is given; pt_film_reset zeroes the counts. A film needs no scene except to add, and survives pt_scene_upload.
 * The film is not a faster pt_render: its kernel is the per-lane interpreter whatever the scene (DESIGN 4.12 has the measurements).
 * Errors, before the first HIP call and with the film unchanged: PT_ERR_ARGUMENT (NULL context, film, camera, background, params or out; a film of another
 * context; width or height 0, or 2^31 pixels or more; a bad sample_mode; background_rows other than 0 or 1; samples == 0; a pixel's count that would pass 2^31;
 * a radiance or film pass in flight; both resolve buffers NULL), PT_ERR_SLICE as for a render, PT_ERR_NO_SCENE (add only). An inverted slice adds nothing and
 * is PT_OK. During the pass: PT_ERR_TRAVERSAL as for a render (the film then holds invalid samples: reset it). */
typedef struct pt_film pt_film;
typedef struct {
    pt_rect slice;              /* pixels that get samples                                                        */
    uint32_t samples;           /* per pixel of the slice, > 0                                                    */
    uint64_t seed;              /* as pt_render_params.seed                                                       */
    int32_t sample_mode;        /* PT_SAMPLE_*                                                                    */
    int32_t background_rows;    /* 1: background is height x 3; 0: height x width x 3 (the FILM's width, height)  */
} pt_film_params;
int pt_film_create(pt_context *ctx, uint32_t width, uint32_t height, pt_film **out);
int pt_film_destroy(pt_context *ctx, pt_film *film);   /* films still alive die with the context */
int pt_film_reset(pt_context *ctx, pt_film *film);
/* Host background, synchronous. kernel_ms (optional): device time of the sampling launches and their folds (HIP events). */
int pt_film_add(pt_context *ctx, pt_film *film, const pt_camera *camera, const double *background, const pt_film_params *params, double *kernel_ms);
/* The same with the background in DEVICE memory, queued on `hip_stream` without synchronising the host. A film pass IS a radiance pass for bookkeeping (as
 * pt_segments is a rays pass): it uses the radiance pass's work buffers and its one pass in flight, is closed by pt_radiance_finish, is refused while a
 * radiance or film pass is open, and counts as a render in flight for pt_scene_update / pt_scene_deform. (An inverted slice queues nothing.) */
int pt_film_add_device(pt_context *ctx, pt_film *film, const pt_camera *camera, const double *d_background, const pt_film_params *params, void *hip_stream);
/* Host buffers, either may be NULL but not both; synchronous. */
int pt_film_resolve(pt_context *ctx, pt_film *film, uint8_t *rgb, double *linear);
/* Device buffers, queued on `hip_stream` (behind a pt_film_add_device on the same stream it sees that pass's samples). */
int pt_film_resolve_device(pt_context *ctx, pt_film *film, void *d_rgb, double *d_linear, void *hip_stream);
int pt_film_counts(pt_context *ctx, pt_film *film, uint32_t *counts);   /* host, width x height: the DEVICE's counts; the host's copy is set to them */

/* ---- Film, behind a lens: depth of field, an orthographic view, a fisheye.
 *   pt_film_add_lens gives every pixel of `slice` its next samples exactly as pt_film_add does - the same counts, fold, launches and bookkeeping, moments films
 *     included - and only the PRIMARY ray of sample s of pixel (x, y) differs: it comes from the lens CONTRACT, a fixed sequence of correctly rounded f64
 *     operations (+ - * / sqrt) that portrayer_amd/csrc/pt_lens.h states in six steps and pt_test_lens_rays_host replays on the host. With
 *     pixel = y * width + x and (sx, sy) the jittered position as pt_film_add takes it (draws 0 and 1 of (seed, pixel, s), or the centre):
 *       PT_LENS_THIN    D = pt_render's unnormalised direction through (sx, sy). aperture == 0: pt_film_add's ray itself. Else the lens point (lx, ly) on the
 *                       unit disc is the xy of pt_ao's direction s & 63 turned by pt_ao's rotation j = (uint32)(draw 0 of (seed, pixel, 0x80000000 | (s >> 6)) *
 *                       256): 64 consecutive samples are stratified over the disc. R, U = columns 0 and 1 of view_to_world; e = (R lx + U ly) * aperture;
 *                       origin eye + e, direction normalised(D - e / focus): points at the distance `focus` along the view axis are sharp.
 *       PT_LENS_ORTHO   vx = (2 sx / W - 1) * aspect * extent, vy = (1 - 2 sy / H) * extent (W, H: the camera's width and height); origin
 *                       view_to_world (vx, vy, 0), direction normalised(view_to_world (vx, vy, -1) - origin). extent = half the height of the view volume.
 *       PT_LENS_STEREO  stereographic fisheye: u, v as vx, vy; q = u u + v v; direction normalised(view_to_world (2 u, 2 v, q - 1) - eye), origin eye.
 *                       extent = tan(fov / 4) for the angle fov across the image height; every pixel has a ray, up to (not including) 360 degrees.
 *     Behind the primary ray everything is pt_film_add's: the stream y * width + x, sample s, draws 2, 3, ..., the background at the integer pixel.
 * PROMISE: sample s of pixel p is, to the bit, what pt_radiance answers for the contract's ray with stream_base + i = p, sample = s and the pixel's background,
 * and the samples are folded as pt_film_add folds them, in all three traversals. The claim covers rays that pt_rays' traced rule accepts; a camera or lens
 * that makes other rays is the caller's error, as for pt_film_add. A film may mix lens and plain adds: it adds what it is given.
 * Errors, before the first HIP call and with the film unchanged: all of pt_film_add's, in its order, then PT_ERR_ARGUMENT for a NULL lens; an unknown model;
 * THIN: aperture not finite or < 0; THIN: focus not finite or <= 0; ORTHO / STEREO: extent not finite or <= 0.
 * Not covered: pt_film_add_map with a lens, and an equirectangular panorama (it needs sin / cos, which the device does not pin in the last bit). */
enum { PT_LENS_THIN = 0, PT_LENS_ORTHO = 1, PT_LENS_STEREO = 2 };
typedef struct {
    int32_t model;              /* PT_LENS_*                                                                      */
    double aperture;            /* THIN: lens radius in world units, >= 0                                         */
    double focus;               /* THIN: distance of the plane of focus along the view axis, > 0                  */
    double extent;              /* ORTHO: half height of the view volume; STEREO: tan(fov / 4); > 0               */
} pt_lens;
/* Host background, synchronous; kernel_ms as for pt_film_add. */
int pt_film_add_lens(pt_context *ctx, pt_film *film, const pt_camera *camera, const pt_lens *lens, const double *background, const pt_film_params *params, double *kernel_ms);
/* The background in DEVICE memory, queued on `hip_stream`; closed by pt_radiance_finish like pt_film_add_device, one pass in flight. */
int pt_film_add_lens_device(pt_context *ctx, pt_film *film, const pt_camera *camera, const pt_lens *lens, const double *d_background, const pt_film_params *params, void *hip_stream);
/* Test hook, no context and no GPU: the contract on the host, by the functions the kernel compiles. Ray i is sample samples[i] of pixel (pixels_xy[2 i],
 * pixels_xy[2 i + 1]) of a film width x height; origins and directions n x 3. PT_ERR_ARGUMENT: a NULL pointer, a bad sample_mode, a lens pt_film_add_lens
 * refuses, a pixel outside the film (nothing is written then). */
int pt_test_lens_rays_host(const pt_camera *camera, const pt_lens *lens, uint32_t width, uint32_t height, uint64_t seed, int32_t sample_mode, uint64_t n,
                           const uint32_t *pixels_xy, const uint32_t *samples, double *origins, double *directions);

/* ---- Film, adaptive: a sample budget per pixel, a noise estimate, and the budget a refine pass gives.
 *   pt_film_add_map gives pixel p of `slice` its next m[p] = min(budget[p], max_samples) samples, each taken and folded exactly as pt_film_add does it: the
 *     PROMISE above is unchanged after any mix of pt_film_add and pt_film_add_map. `budget` is width x height u32, row-major like pt_film_counts; only the
 *     slice is read. The samples of a launch are laid out one per lane, whatever their pixels want: no lane idles beside a pixel that wanted more.
 *     max_samples is 1 .. PT_FILM_MAP_MAX; the number of launches follows from it (a device map is not known to the host). A map of zeros is PT_OK and changes
 *     nothing. Bookkeeping and refusals are pt_film_add(_device)'s: one radiance / film pass in flight, closed by pt_radiance_finish; a pixel's count may not
 *     pass 2^31 - for a host map by its own m[p], for a device map by max_samples, by which the HOST's copy of the counts is then raised over the slice: an
 *     upper bound, which pt_film_counts brings back to the device's values. Also refused (PT_ERR_ARGUMENT): a slice of 2^29 pixel slots (8x8 tiles x 64) or more.
 *   pt_film_create_moments makes a film that keeps one more f64 per pixel (60 bytes instead of 52): q, the running sum of y * y, y = (v.x + v.y) + v.z of
 *     every sample v, in plain ascending order (the first sample is assigned: pt_film_reset clears nothing more). Every add to such a film keeps it.
 *   pt_film_error writes width x height f64, the standard error of the mean of y in linear units, in exactly this order of IEEE operations:
 *     n = count[p]; n < 2: +inf; S = the pixel's sum as resolve divides it; mean = S / n; my = (mean.x + mean.y) + mean.z;
 *     var = (q - (n * my) * my) / (n - 1), a var that is not > 0 becomes 0; err = sqrt(var / n). PT_ERR_ARGUMENT on a film without moments.
 *   pt_film_budget_device writes width x height u32: 0 outside `slice`; inside, with c = count[p] and e = the error above:
 *     c < min_count: min(min_count - c, step); else c < max_count and e > threshold: min(step, max_count - c); else 0.
 *     d_summary (2 x u64, zeroed by the call on the stream): the pixels with a budget, and the sum of the budgets. Needs a film with moments; step is
 *     1 .. PT_FILM_MAP_MAX, min_count <= max_count <= 2^31. Queued on `hip_stream`; refused while a pass of the film is open. */
#define PT_FILM_MAP_MAX 4096u
typedef struct {
    pt_rect slice;              /* pixels that may get samples                                                    */
    uint32_t max_samples;       /* no pixel gets more in this call, 1 .. PT_FILM_MAP_MAX                          */
    uint64_t seed;              /* as pt_render_params.seed                                                       */
    int32_t sample_mode;        /* PT_SAMPLE_*                                                                    */
    int32_t background_rows;    /* as pt_film_params.background_rows                                              */
} pt_film_map_params;
typedef struct {
    pt_rect slice;              /* pixels that may get a budget                                                   */
    double threshold;           /* refine where the error is above it                                             */
    uint32_t min_count;         /* every pixel of the slice is brought to this count first                        */
    uint32_t max_count;         /* ... and none beyond this one                                                   */
    uint32_t step;              /* most samples one pass gives a pixel                                            */
} pt_film_refine_params;
int pt_film_create_moments(pt_context *ctx, uint32_t width, uint32_t height, pt_film **out);
/* Host map and background, synchronous; the host's copy of the counts is updated exactly. kernel_ms as for pt_film_add. */
int pt_film_add_map(pt_context *ctx, pt_film *film, const pt_camera *camera, const double *background, const pt_film_map_params *params, const uint32_t *budget, double *kernel_ms);
/* Map and background in DEVICE memory, queued on `hip_stream`; closed by pt_radiance_finish like pt_film_add_device. The map is read by the kernels of the
 * pass: it must stay unchanged until the pass is finished. */
int pt_film_add_map_device(pt_context *ctx, pt_film *film, const pt_camera *camera, const double *d_background, const pt_film_map_params *params, const uint32_t *d_budget, void *hip_stream);
int pt_film_error(pt_context *ctx, pt_film *film, double *err);   /* host, width x height; synchronous */
int pt_film_error_device(pt_context *ctx, pt_film *film, double *d_err, void *hip_stream);
int pt_film_budget_device(pt_context *ctx, pt_film *film, const pt_film_refine_params *params, uint32_t *d_budget, uint64_t *d_summary, void *hip_stream);

/* ---- Film, denoised: a second, explicitly LOSSY way to read a film (resolve keeps its promise; the film's state is not written). An edge-avoiding a-trous
 * wavelet filter over the resolved mean, steered by primary-visibility buffers (`guides`, laid out as pt_aov writes them) and by the film's own noise
 * estimate. The filter has no counterpart in the reference: it is DEFINED as the following sequence of correctly rounded IEEE f64 operations (+ - * /,
 * comparisons; no exp, no libm - the weights are clamped rationals so that a restatement can match in its bits), and the kernels, pt_test_denoise_host and
 * a numpy restatement agree in every bit. portrayer_amd/csrc/pt_denoise.h holds these steps as functions; DESIGN 4.14 has the text.
 *   level 0, per pixel with count > 0: c = pt_film_sum / count (resolve's linear); v = e * e, e = pt_film_error's value, where count >= 2; at count 1
 *     v = my * my, my = (c.x + c.y) + c.z; on a film without moments v = 0, accepted with sigma_color == 0 only.
 *   level l (0 <= l < iterations), step s = 1 << l, H = {1/16, 1/4, 3/8, 1/4, 1/16}: for every centre p with count > 0, cs = (+0, +0, +0), vs = ws = +0; the
 *     taps q = p + s (i, j), j = -2 .. 2 outer, i = -2 .. 2 inner; a tap outside the film or with count[q] == 0 is skipped; then
 *       1. skip if (node[p] < 0) != (node[q] < 0); with PT_DENOISE_SAME_NODE skip if node[p] != node[q];
 *       2. w = H[j + 2] * H[i + 2];
 *       3. on a hit, normal_power_log2 >= 0: a = (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z; a = a > 0 ? a : 0; normal_power_log2 times a = a * a; w = w * a;
 *       4. on a hit, sigma_plane > 0: e = pos_q - pos_p; d = (n_p.x e.x + n_p.y e.y) + n_p.z e.z; t = 1 - (d * d) * kp; w = w * (t > 0 ? t * t : 0);
 *          kp = 1.0 / (sigma_plane * sigma_plane);
 *       5. sigma_color > 0: y = (c.x + c.y) + c.z; dy = y_p - y_q; t = 1 - (dy * dy) / (kc * (v_p + v_q) + 1e-12); w = w * (t > 0 ? t * t : 0);
 *          kc = sigma_color * sigma_color;
 *       6. skip unless w > 0 (also a NaN weight from non-finite guides);
 *       7. cs = cs + c_q * w per channel; vs = vs + (w * w) * v_q; ws = ws + w.
 *     c' = cs / ws, v' = vs / (ws * ws); with ws == 0 (a degenerate guide at p itself) c' = c_p, v' = v_p.
 *   after the last level, each optional: linear = c (width x height x 3 f64), variance = v (width x height f64), rgb = resolve's finishing of c (gamma, clamp,
 *     u8). Pixels with count == 0 are neither centres nor taps and keep what the output buffers hold.
 * MEMORY: a level reads (c, v) and writes the next level's: two work buffers of 32 bytes per pixel that BELONG TO THE FILM - allocated by its first denoise,
 * kept for later ones, freed with the film.
 * Guides: `node` always; `normal` with normal_power_log2 >= 0 or sigma_plane > 0; `position` with sigma_plane > 0. No scene is needed.
 * Errors, with nothing written: PT_ERR_ARGUMENT (NULL context, film, params or guides; a film of another context; iterations outside 1 .. 8; unknown flags;
 * a negative or non-finite sigma; normal_power_log2 outside -1 .. 7; a required guide NULL; all three outputs NULL; sigma_color > 0 on a film without
 * moments; a pass of this film in flight; in the device form a guide or an output that is not 8-byte aligned device memory of the context's device reaching
 * far enough). All but the last come before the first HIP call.
 * PORTRAYER_DENOISE_TILE=0|1 (read per call) selects the direct or the LDS-tiled form of the level kernel; both compute the same bits. */
#define PT_DENOISE_SAME_NODE 1u
typedef struct {
    int32_t iterations;         /* 1 .. 8: filter levels, level l with step 1 << l                                */
    uint32_t flags;             /* PT_DENOISE_SAME_NODE: taps on another node get weight 0                        */
    double sigma_color;         /* >= 0: colour tolerance in standard errors; 0 = no colour weight               */
    double sigma_plane;         /* >= 0: plane-distance tolerance in world units; 0 = off                        */
    int32_t normal_power_log2;  /* -1 .. 7: the clamped normal dot raised to 2^k; -1 = off                        */
} pt_denoise_params;
typedef struct { const double *position; const double *normal; const int32_t *node; } pt_denoise_guides;
/* Guides and outputs in DEVICE memory, queued on `hip_stream` without synchronising the host (behind a finished add on the same stream it sees its samples). */
int pt_film_denoise_device(pt_context *ctx, pt_film *film, const pt_denoise_params *params, const pt_denoise_guides *d_guides, void *d_rgb, double *d_linear, double *d_variance,
                           void *hip_stream);
/* Host buffers, synchronous. */
int pt_film_denoise(pt_context *ctx, pt_film *film, const pt_denoise_params *params, const pt_denoise_guides *host_guides, uint8_t *rgb, double *linear, double *variance);

/* ---- The same filter on DEMODULATED colour: `albedo` (width x height x 3 f64, as pt_guides writes it) is divided out of level 0's colour and
 * multiplied back after the last level, so that texture detail the guide knows of is not blurred. Parameters, guides, levels, bookkeeping, refusals and
 * outputs are pt_film_denoise's; a NULL albedo is PT_ERR_ARGUMENT, and in the device form the albedo is checked like the guides. The steps, as functions of
 * portrayer_amd/csrc/pt_denoise.h, with EPS = PT_DENOISE_ALBEDO_EPS = 0.0078125 (2^-7):
 *   per pixel with count > 0: on a hit (node >= 0), per channel a of the albedo: m = (a >= 0.0 && a < inf) ? a + EPS : 1.0 (a NaN, negative or infinite
 *     channel is not demodulated); on a miss m = (1, 1, 1); mm = ((m.x + m.y) + m.z) / 3.0;
 *   after the level-0 seed: c.x = c.x / m.x, likewise y and z; v = v / (mm * mm) (the film keeps ONE variance, that of the channel sum: exact for grey
 *     albedos, an approximation otherwise);
 *   the levels of pt_film_denoise, unchanged;
 *   after the last level: c.x = c.x * m.x, likewise y and z; v = v * (mm * mm), with the pixel's own m; then linear, variance and rgb as above. */
int pt_film_denoise_albedo_device(pt_context *ctx, pt_film *film, const pt_denoise_params *params, const pt_denoise_guides *d_guides, const double *d_albedo, void *d_rgb, double *d_linear,
                                  double *d_variance, void *hip_stream);
int pt_film_denoise_albedo(pt_context *ctx, pt_film *film, const pt_denoise_params *params, const pt_denoise_guides *host_guides, const double *albedo, uint8_t *rgb, double *linear,
                           double *variance);

/* Bytes of one rank's compact tile buffer for a slice split over tile_ranks ranks (equal for all ranks). */
uint64_t pt_compact_bytes(const pt_render_params *params);
/* Scatters the gathered compact buffers (rank-major) into a row-major image on the device. */
int pt_untile_device(pt_context *ctx, const pt_render_params *params, const void *d_gathered, void *d_rgb, void *hip_stream);

/* Host-side view of the tile partition (no GPU needed): pixel of work slot `slot` of rank `rank`
 * (slot = local tile * 64 + position in the 8x8 tile). Returns 1 and fills x, y; 0 for a padding slot
 * (outside the slice / beyond the last tile); < 0 on bad arguments. */
int pt_tile_slot_pixel(const pt_render_params *params, uint32_t rank, uint32_t slot, uint32_t *x, uint32_t *y);
/* Host version of pt_untile_device: gathered = tile_ranks x pt_compact_bytes(), rank-major. */
int pt_untile_host(const pt_render_params *params, const uint8_t *gathered, uint8_t *rgb);

/* ---- One render call over the GPUs of a node (ABI 5). One context per GPU, the scene replicated; the slice's 8x8
 * tiles are dealt round-robin to the ranks, each rank renders its tiles into a compact buffer on its own stream, ONE
 * RCCL gather (ncclGather over xGMI, single process) brings them to rank 0, which untiles them. The slice API of the
 * reference (src/render.rs:56-66, :211-213) is the rectangular special case this generalises. `devices` = n_devices
 * device indices (NULL: 0 .. n_devices - 1); ranks may share a device (then the gather is device-to-device copies:
 * RCCL needs distinct GPUs). RCCL is loaded on first use. */
typedef struct pt_node pt_node;
int pt_node_create(int n_devices, const int *devices, pt_node **out);
void pt_node_destroy(pt_node *node);
const char *pt_node_last_error(const pt_node *node);
int pt_node_ranks(const pt_node *node);
int pt_node_uses_rccl(const pt_node *node);          /* 1: the gather is RCCL; 0: ranks share a device, copies */
pt_context *pt_node_context(pt_node *node, int rank);
int pt_node_scene_upload(pt_node *node, const pt_scene *scene, int traverse, const pt_kdtree *kd);
/* pt_scene_update on every rank; refused with PT_ERR_ARGUMENT while frames are open (pt_node_frame_begin without its pt_node_frame_end) */
int pt_node_scene_update(pt_node *node, const pt_scene_motion *motion, const pt_kdtree *kd);
/* pt_scene_deform on every rank, refused alike while frames are open */
int pt_node_scene_deform(pt_node *node, uint32_t n_deforms, const pt_mesh_deform *deforms,
                         const pt_scene_motion *motion, const pt_kdtree *kd);
/* Like pt_render (host buffers; params->tile_rank / tile_ranks must be 0 / 1: the node partitions the tiles itself).
 * stats: counters summed over the ranks, kernel_ms of the slowest rank, total_ms of the whole call. */
int pt_node_render(pt_node *node, const pt_camera *camera, const double *background, const pt_render_params *params,
                   uint8_t *rgb, pt_stats *stats);
/* (ABI 6) The same call in its three parts, for callers that render many frames of one size (and for measuring the frame with its
 * inputs resident in HBM): pt_node_upload_background copies the background to every rank (and, when rgb is not NULL, the
 * caller's image to rank 0, so that pixels outside the slice keep their bytes); pt_node_render_resident renders, gathers and
 * untiles into the image resident on rank 0 and returns when it is complete - no host buffer is touched; pt_node_download_image
 * copies that image out. pt_node_device: the device index of a rank (< 0: no such rank). */
int pt_node_upload_background(pt_node *node, const double *background, const pt_render_params *params, const uint8_t *rgb);
int pt_node_render_resident(pt_node *node, const pt_camera *camera, const pt_render_params *params, pt_stats *stats);
int pt_node_download_image(pt_node *node, const pt_render_params *params, uint8_t *rgb);
int pt_node_device(const pt_node *node, int rank);
/* (ABI 7) Frames in a pipeline. pt_node_frame_begin queues a frame - every rank's render (launched by the rank's own host thread), the ONE
 * gather and the untile - and returns without waiting; pt_node_frame_end closes the OLDEST open frame: it returns when that frame's image is
 * complete on rank 0, with its stats (counters summed over the ranks, kernel_ms of the slowest rank). Up to two frames may be open: their
 * tile buffers are separate and the gather runs on streams of its own, so frame k + 1 renders while frame k is gathered and untiled, and
 * the host's launch work disappears behind the GPUs' (render.rs:93-151 renders one frame per call: pt_node_render_resident = begin + end).
 * The image on rank 0 is a single buffer: pt_node_download_image (and pt_node_upload_background) need every frame closed.
 * pt_node_last_frame_host_ms: host milliseconds of the last frame's calls - [0] begin as a whole, [1] end blocked until the image was
 * complete, [2] end after that, [3] the slowest rank's launch inside begin, [4] the ranks' kernel times added up. */
int pt_node_frame_begin(pt_node *node, const pt_camera *camera, const pt_render_params *params);
int pt_node_frame_end(pt_node *node, pt_stats *stats);
int pt_node_frames_in_flight(const pt_node *node);
int pt_node_last_frame_host_ms(const pt_node *node, double out[5]);
/* (ABI 8) every rank's kernel time of the last frame closed, milliseconds (HIP events around the rank's launches); n_out = pt_node_ranks() */
int pt_node_last_frame_rank_kernel_ms(const pt_node *node, double *out, int n_out);

/* Device-side helpers used by the measurement harness. */
int pt_device_alloc(pt_context *ctx, uint64_t bytes, void **out);
int pt_device_free(pt_context *ctx, void *ptr);
int pt_copy_to_device(pt_context *ctx, void *dst, const void *src, uint64_t bytes);
int pt_copy_from_device(pt_context *ctx, void *dst, const void *src, uint64_t bytes);
int pt_synchronize(pt_context *ctx); /* waits for everything queued on the context's device */
/* Streams `bytes` from src to dst with 16-byte accesses `iters` times and returns the best GB/s
 * (read + write counted), the measured HBM roofline the renderer is compared with. */
int pt_measure_copy_bandwidth(pt_context *ctx, uint64_t bytes, int iters, double *gbps);

/* Self-test entry points for the parity tests: run device arithmetic on explicit inputs. */
int pt_test_cast_rays(pt_context *ctx, uint64_t n, const double *origins, const double *directions, int any_hit,
                      double *out_t, int32_t *out_node, int32_t *out_sub);
/* tests: bytes of device memory the context's scene buffers hold (pt_scene_update must not make it grow) */
uint64_t pt_test_scene_bytes(const pt_context *ctx);
/* tests: out[0] the walks' stack_cap, out[1] who built the scene-level tree last (0 pt_scene_upload, 1 pt_scene_update on the host, 2 on the device),
 * out[2] the device build's clustering rounds, out[3] bytes of the tree buffers (bvh, bvh4, bvh_items) */
int pt_test_scene_info(const pt_context *ctx, uint64_t out[4]);
/* tests: the shape of pt_vertex_bounds_device's reduction on this context's device: out[0] = vertices a block takes per step (its thread count), out[1] = the
 * most blocks it launches. More than out[0] vertices use several blocks, more than out[0] x out[1] several grid strides. */
int pt_test_vertex_box_shape(const pt_context *ctx, uint64_t out[2]);
int pt_test_math(pt_context *ctx, int op, uint64_t n, const double *a, const double *b, double *out);
/* (ABI 6) No GPU, no context: x[i]^y[i] by the HOST build of the kernels' pow (csrc/pt_pow.h) in `port` and by this machine's
 * libm in `libm` - the pin of the restated glibc algorithm against the library the reference calls. */
int pt_test_pow_host(uint64_t n, const double *x, const double *y, double *port, double *libm);
/* (ABI 7) the host's libm on explicit inputs (2 pow, 4 atan2, 5 acos): what device results are compared with */
int pt_test_libm_host(int op, uint64_t n, const double *a, const double *b, double *out);
/* Host-side replay (no GPU, no context) of how a launch with these parameters lays its work items and their 64 lanes over pixels,
 * chunks and samples - the kernel's own indexing code. Arrays of width x height, zeroed by the caller: samples carried per pixel,
 * the sum of their indices, the sum of the chunk lengths reported by the lanes that add a chunk up; optionally the number of work
 * items and {pixels, chunks, samples} per wavefront. */
int pt_test_work_items(const pt_render_params *params, uint32_t *sample_count, uint64_t *sample_index_sum, uint32_t *chunk_length_sum,
                       uint64_t *n_items, uint32_t *lane_pixels_chunks_samples);
/* What an uploaded scene says that the choice of its render kernel depends on (the context keeps one per scene; pt_scene_update refreshes n_lights and
 * area_light): what the scene IS, not what follows from it. */
typedef struct pt_scene_traits {
    int32_t traverse;            /* PT_TRAVERSE_*                                                            */
    uint32_t n_nodes, n_lights;  /* flattened nodes, lights                                                  */
    int32_t has_meshes;          /* the scene has meshes (Mesh or KDMesh) ...                                */
    int32_t has_kdmesh;          /* ... and some of them carry a KDMesh tree                                 */
    int32_t reflective;          /* some material is reflective (material.rs:216: its hits spawn rays)       */
    int32_t reflective_opaque;   /* every reflective material is opaque (no index of refraction)             */
    int32_t glossy;              /* some reflective material is glossy (material.rs:221-239: it draws random numbers) */
    int32_t area_light;          /* some light is an area light (light.rs:51-53: it draws random numbers)    */
    int32_t pad;
    uint64_t instanced_tris;     /* triangles over all Mesh / KDMesh nodes, a mesh counted once per instance */
} pt_scene_traits;
/* Host-side (no GPU, no context): the kernel a render of a scene with these traits launches under the environment's PORTRAYER_* switches, as pt_stats reports
 * it - *kernel_mode (PT_KERNEL_MODE_*) and *kernel_variant (PT_KERNEL_*, without PT_KERNEL_COUNTING). mode: the scene's PT_KERNEL_MODE_*, or a negative
 * number for the one that follows from the traits; textured: some material of the scene has a texture or a normal map. */
int pt_test_kernel_choice(const pt_scene_traits *traits, int mode, int textured, uint32_t *kernel_mode, uint32_t *kernel_variant);
/* What a render launch depends on besides the PORTRAYER_* switches: the scene's traits, its mode (PT_KERNEL_MODE_*; negative: the one that follows from the traits),
 * whether it is textured, whether the launch counts (collect_stats), the scene's flattened nodes, lights and traversal-stack entries per lane, the launch's shape - pixel
 * slots (own tiles x 64), wavefront work items, sample chunks per pixel, log2 of the samples (K) and chunks (C) of a pixel side by side in a wavefront (K C = 64: a
 * wavefront is one pixel), the slice's tiles per row, the ranks that share the frame's tiles - and the blocks of the chosen kernel resident on the device. */
typedef struct pt_launch_query {
    pt_scene_traits traits;
    int32_t mode, textured, stats;
    uint32_t n_nodes, n_lights;
    int32_t stack_cap;
    uint32_t n_slots, n_items, n_chunks, k_log2, c_log2, tiles_x, tile_ranks;
    uint32_t grid;
} pt_launch_query;
/* The words of a launch's plan (pt_test_launch_plan): the kernel as pt_stats reports it (PT_KERNEL_COUNTING included), its PT_RUN_* number, its waves per SIMD above
 * three (0: three), parked frames per lane in LDS, LDS bytes a block may take, whether lanes keep recursion frames in HBM, traversal-stack entries per lane in LDS, the
 * share of the resident blocks; how the work items are dealt; the bytes of the slot's five buffers (EYE_TAB_BYTES 0: the launch has none); in `misc` the dark-light
 * records and the occluder table, in `eye_tab` (which begins with the eye table) the certain-shadow table, the list header, the records and the queue, as byte offsets
 * (a region the launch does not have is empty, its offset the next region's); PT_PLAN_HAS_* bits; the entries a list holds at most, the words of the list kernel's
 * pending list, the occluder table's entries per tile row; PORTRAYER_OCC_SEED's request (0 none, 1 hashed, 2 all:K) and its seed or K; the word the list header is
 * set to in front of the list kernel. */
enum { PT_PLAN_KERNEL_MODE, PT_PLAN_KERNEL_VARIANT, PT_PLAN_RUN_VARIANT, PT_PLAN_MORE_WAVES, PT_PLAN_PARK_SLOTS, PT_PLAN_BLOCK_BUDGET, PT_PLAN_NEEDS_SPILL, PT_PLAN_STACK_LDS_CAP,
       PT_PLAN_GRID_SHARE, PT_PLAN_N_LANES, PT_PLAN_WORK_DIV, PT_PLAN_BATCH_MAX, PT_PLAN_FINE_QUEUES, PT_PLAN_ITEM_STRIDE,
       PT_PLAN_SPILL_BYTES, PT_PLAN_STACK_SPILL_BYTES, PT_PLAN_MISC_BYTES, PT_PLAN_ACCUM_BYTES, PT_PLAN_EYE_TAB_BYTES,
       PT_PLAN_DARK_OFF, PT_PLAN_DARK_BYTES, PT_PLAN_OCC_OFF, PT_PLAN_OCC_BYTES, PT_PLAN_CERTAIN_OFF, PT_PLAN_HEADER_OFF, PT_PLAN_RECORDS_OFF, PT_PLAN_QUEUE_OFF,
       PT_PLAN_HAS, PT_PLAN_LIST_CAP, PT_PLAN_LIST_PENDING, PT_PLAN_OCC_ROW, PT_PLAN_OCC_SEED, PT_PLAN_OCC_SEED_VALUE, PT_PLAN_HEADER_FILL, PT_PLAN_WORDS };
/* PT_PLAN_HAS: the occluder table; the eye table; the certain-shadow table; the dark-light records (zeroed) and the kernel that fills them; the list header; the
 * per-pixel lists; the queue of the pixels that need the render kernel (the background skip) */
enum { PT_PLAN_HAS_OCCLUDERS = 1, PT_PLAN_HAS_EYE_TABLE = 2, PT_PLAN_HAS_CERTAIN_TABLE = 4, PT_PLAN_HAS_DARK_RECORDS = 8, PT_PLAN_HAS_DARK_LIGHTS = 16,
       PT_PLAN_HAS_LIST_HEADER = 32, PT_PLAN_HAS_PIXEL_LISTS = 64, PT_PLAN_HAS_QUEUE = 128 };
/* Host-side (no GPU, no context): the plan of a render launch with these inputs under the environment's PORTRAYER_* switches, as PT_PLAN_WORDS words. A malformed
 * PORTRAYER_OCC_SEED, PORTRAYER_PIXEL_LIST_CAP or PORTRAYER_PIXEL_LIST_PENDING: PT_ERR_ARGUMENT, the words of the refusal in why (optional, why_bytes bytes). */
int pt_test_launch_plan(const pt_launch_query *query, uint64_t *words, char *why, uint64_t why_bytes);
/* Host-side run (no GPU, no context) of the tree walks' single-precision slab test. Pair i: the ray origins[3i..], directions[3i..] over [0, t_max[i]]
 * against the box box_lo[3i..], box_hi[3i..]. body 0: the ray constants as the kernels are built, 1: their form with f64 products, 2: their f32 form.
 * Out per pair: the interval the per-lane form computed (t_near, t_far) and verdict - bit 0 the per-lane form accepts the box, bit 1 the wavefront
 * form for mixed signs does, bit 2 the wavefront form for the ray's own octant does, bit 3 the two children of a wavefront form disagree. */
int pt_test_raypk(uint64_t n, int body, const double *origins, const double *directions, const double *t_max, const float *box_lo, const float *box_hi,
                  int32_t *verdict, float *t_near, float *t_far);
/* Host-side run (no GPU, no context) of the shadow rays' certain-occlusion test. Case i: a node of primitive `type` (the PT_* tags of the scene export: 0 sphere,
 * 5 cube have a ball; every other type is never certain) with rows 0..2 of its forward and inverse matrices in fwd[12i..] and inv[12i..], a shaded point P[3i..] and a light position L[3i..].
 * out_certain[i]: the single-precision test says the shadow ray certainly ends in the node; out_exact_hit[i]: the exact test of that node for that ray says so. */
int pt_test_certain_shadow(uint64_t n, int type, const double *fwd, const double *inv, const double *P, const double *L, int32_t *out_certain, int32_t *out_exact_hit);
/* Host-side run (no GPU, no context) of the dark-light test: a point light enclosed in a sphere or a cube is dark from everywhere, and the launch finds that once per light.
 * Case i: a node as for pt_test_certain_shadow, a shaded point P[3i..], a light at L[3i..] with the area vectors area[6i..] (area_a, area_b; NULL: point lights).
 * out_flagged[i]: the light is found enclosed in the node; out_guard[i]: the single-precision lane guard lets P skip the light (0 where not flagged); out_exact_hit[i]: the
 * exact test of the node for the shadow ray from P toward L reports a hit. */
int pt_test_dark_light(uint64_t n, int type, const double *fwd, const double *inv, const double *P, const double *L, const double *area, int32_t *out_flagged, int32_t *out_guard,
                       int32_t *out_exact_hit);
/* The dark-light records of the context's last launch (tests; that launch must be closed). info has 2 entries: [0] the lights that launch had records for - 0 where it had
 * none -, [1] the 32-bit words of a record (8). A record: words 0..2 the light's position as f32 bits, word 3 the guard's ceiling on |L - P|^2 as f32 bits (0: the light is
 * not dark), word 4 the enclosing node + 1 (0: none), word 5 the guard's floor as f32 bits. Where out is not NULL and words >= info[0] * info[1], the records are copied to out. */
int pt_test_dark_lights(pt_context *ctx, uint32_t *out, uint64_t words, uint64_t *info);
/* Host-side run (no GPU, no context) of the beam test behind the primary rays' per-pixel candidate lists, beside the tree walk's own slab test. Case i: a camera
 * (cameras[19i..]: eye, rows 0..2 of view_to_world, fov_factor, aspect_ratio, width, height), a pixel (pixels[2i..]: x, y), a sample position inside it
 * (jitters[2i..], each in [0, 1)) and a box (box_lo[3i..], box_hi[3i..]). accept[i]: some ray through the pixel may reach the box, as the list kernel decides it;
 * bound[i]: the lower bound on every such ray's entry parameter it stores (0 where it rejects); walk[i]: the walk's slab test of the box for the sample's ray, no bound
 * on t - bit 0 the wavefront form for mixed signs accepts, bit 1 the form for the ray's own octant does; rays (may be NULL): the sample's ray, origin and direction. */
int pt_test_pixel_beam(uint64_t n, const double *cameras, const uint32_t *pixels, const double *jitters, const float *box_lo, const float *box_hi,
                       int32_t *accept, float *bound, int32_t *walk, double *rays);
/* What the last launch of the context left in its per-pixel candidate lists (tests; that launch must be closed). out has 11 entries: [0] the records - 0 where the launch
 * had no lists -, [1] the background ones (empty, nothing left out), [2] those cut at the cap, [3] those marked "take the walk", [4 + n] those with n entries, n = 0 .. 6. */
int pt_test_pixel_list_summary(pt_context *ctx, uint64_t *out);
/* pt_test_pixel_beam with a rectangle per case instead of a pixel (rects[4i..]: x, y, nx, ny - the beam of every sample position in [x, x + nx] x [y, y + ny]; the
 * list kernel opens the tree with the 8 x 8 rectangle of a tile's pixel slots) and the sample's position inside it (offsets[2i..], in [0, nx] x [0, ny]). With
 * nx = ny = 1 every output is pt_test_pixel_beam's, bit for bit. */
int pt_test_rect_beam(uint64_t n, const double *cameras, const uint32_t *rects, const double *offsets, const float *box_lo, const float *box_hi,
                      int32_t *accept, float *bound, int32_t *walk, double *rays);
/* The raw records of the last launch's per-pixel candidate lists (tests; that launch must be closed). info has 4 entries: [0] the records - 0 where the launch had no
 * lists -, [1] the 32-bit words of a record, [2] the entries a record holds at most, [3] the scene's flattened nodes. A record: word 0 the number of entries (bit 31: take
 * the walk), word 1 the tail bound's f32 bits, word 2 + k entry k = the bound's upper 16 bits << 16 | the node. Where out is not NULL and words >= info[0] * info[1], the
 * records are copied to out; otherwise (words = 0: a query of the sizes) nothing is. */
int pt_test_pixel_list_records(pt_context *ctx, uint32_t *out, uint64_t words, uint64_t *info);
/* The last launch's queue of the pixels that need the render kernel (tests; that launch must be closed): the pixel slots (local tile << 6 | y * 8 + x inside the tile)
 * whose record is not {no entry, nothing left out, unmarked} and that lie inside the slice, a tile's together in its Morton order, the tiles in no fixed order. info has
 * 3 entries: [0] 1 where the launch had a queue (0: every pixel was dealt, PORTRAYER_BACKGROUND_SKIP=0 among the reasons), [1] the queue's length as the device counted
 * it, [2] the launch's pixel slots. Where out is not NULL and words >= info[1], the ids are copied to out. */
int pt_test_pixel_list_queue(pt_context *ctx, uint32_t *out, uint64_t words, uint64_t *info);
/* Host-side run (no GPU, no context) of the sum the finish kernel gives a pixel that was never dealt: `samples` samples of the colour rgb[0..2] under the summation
 * contract (chunks of 8: a chunk's first sample assigned, the rest added left to right; the first chunk assigned, the rest added in ascending order) -> out[0..2]. */
int pt_test_background_sum(const double *rgb, uint32_t samples, double *out);
/* Host-side run (no GPU, no context) of the film's running sum: `samples` (n x 3) given to one pixel in n_cuts consecutive adds of cuts[k] samples each
 * (their sum must be n), through the functions the film's fold and resolve kernels call. out_sum: what resolve divides by n. */
int pt_test_film_fold_host(uint32_t n, const double *samples, const uint32_t *cuts, uint32_t n_cuts, double out_sum[3]);
/* The same for a film with moments, through the functions pt_film_fold_map_kernel and pt_film_error_kernel call: out_q the pixel's second moment, out_err what
 * pt_film_error writes for it. n = 0 (then samples, cuts may be NULL): the untouched pixel, out_err = +inf. */
int pt_test_film_moments_host(uint32_t n, const double *samples, const uint32_t *cuts, uint32_t n_cuts, double out_sum[3], double *out_q, double *out_err);
/* Host-side run (no GPU, no context) of the plan of launch round `round` of pt_film_add_map over `slice` of a width x height film: the list the sampling
 * kernel walks, one entry per sample, (pixel slot << 3) | j in ascending (slot, j) order; pixel slots are the slice's 8x8 tiles, row-major, rows of a tile.
 * *n_out: the list's length (also where it exceeds `cap`, the room in `list`). */
int pt_test_film_plan_host(uint32_t width, uint32_t height, const pt_rect *slice, const uint32_t *budget, uint32_t max_samples, uint32_t round, uint32_t *list, uint32_t cap,
                           uint32_t *n_out);
/* The same list by the plan KERNELS of `ctx`'s device (host `budget` in, list copied back; nothing is sampled, no scene or film needed). */
int pt_test_film_plan(pt_context *ctx, uint32_t width, uint32_t height, const pt_rect *slice, const uint32_t *budget, uint32_t max_samples, uint32_t round, uint32_t *list, uint32_t cap,
                      uint32_t *n_out);
/* Host-side run (no GPU, no context) of pt_film_denoise's levels through the functions its kernels call, from a level-0 input the caller supplies: `linear`
 * (width x height x 3), `variance` (width x height; NULL = zeros, with sigma_color == 0 only), `counts` and the guides, all host memory. out_linear and
 * out_variance are each optional (not both NULL); pixels with count == 0 are left untouched. */
int pt_test_denoise_host(uint32_t width, uint32_t height, const pt_denoise_params *params, const double *linear, const double *variance, const uint32_t *counts,
                         const pt_denoise_guides *guides, double *out_linear, double *out_variance);
/* The same for pt_film_denoise_albedo: the division after the level-0 input, pt_test_denoise_host's levels, the products after the last level. */
int pt_test_denoise_albedo_host(uint32_t width, uint32_t height, const pt_denoise_params *params, const double *linear, const double *variance, const uint32_t *counts,
                                const pt_denoise_guides *guides, const double *albedo, double *out_linear, double *out_variance);

#ifdef __cplusplus
}
#endif
#endif
