/* portrayer_host.h — C entry points of the C++ host library (portrayer_amd/host/portrayer.hpp) for
 * callers that cannot include C++ (the Python harness in tests/ and bench.py).
 *
 * The host library is the counterpart of the reference crate's public API above the pixel loop:
 * SceneNode builder calls (src/scene.rs:151-205), flattening (src/flat_scene.rs:18-46), bounding
 * boxes (src/bounding_box.rs), the k-d tree build (src/kdtree/leaf.rs:89-231), the camera
 * (src/camera.rs:34-45) and Image::render (src/render.rs:93-126, :216-223). A scene is handed over
 * as a DESCRIPTION — per node the ordered list of builder calls, exactly what a scene script
 * writes — and replayed on the C++ SceneNode API, so this boundary adds no arithmetic of its own.
 * All functions return 0 or a negative code; ph_last_error() gives the message (thread-local).
 */
#ifndef PORTRAYER_HOST_H
#define PORTRAYER_HOST_H

#include <stdint.h>

#include "portrayer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ph_scene ph_scene;       /* a scene::HierScene                                  */
typedef struct ph_renderer ph_renderer; /* a flattened scene resident on one GPU               */

enum { PH_OK = 0, PH_ERR_ARGUMENT = -1, PH_ERR_PANIC = -2 /* where the reference would panic */, PH_ERR_RUNTIME = -3, PH_ERR_SMALL = -4 /* output capacity */ };

typedef struct {
    uint32_t n_nodes;
    /* builder calls of node i, in call order: ops[ops_off[i] .. ops_off[i+1]) with one char per call —
     * 's' scaled(x,y,z)  't' translated(x,y,z)  'x' 'y' 'z' rotated_x/y/z(radians) — and their
     * arguments consumed left to right from args[args_off[i] ..) (scene.rs:163-199). */
    const char *ops; const uint32_t *ops_off;
    const double *args; const uint32_t *args_off;
    const int32_t *prim_type;     /* -1: no geometry, else PT_PRIM_*                                     */
    const int32_t *prim_data;     /* MESH/KDMESH: mesh index; TRIANGLE: triangle index                   */
    const int32_t *prim_flags;    /* bit 0: Shading::Smooth                                              */
    const int32_t *material;
    const uint32_t *child_off;    /* n_nodes + 1                                                         */
    const uint32_t *children;     /* child node indices in `children` Vec order; shared nodes = Arc clones */
    uint32_t root;
    uint32_t n_meshes; const uint64_t *mesh_vert_off, *mesh_tri_off; const double *mesh_positions, *mesh_normals;
    const uint8_t *mesh_has_normals; const uint32_t *mesh_indices;
    uint32_t n_triangles; const double *tri_vertices, *tri_normals; const uint8_t *tri_has_normals;
    uint32_t n_materials; const double *materials; /* x 10, layout of pt_scene.materials                  */
    uint32_t n_lights; const double *lights;       /* x 15, layout of pt_scene.lights                     */
    double ambient[3];
    /* textures (src/texture.rs), same layout as the pt_scene fields of the same names; optional */
    const double *mesh_texcoords; const uint8_t *mesh_has_texcoords;
    const double *tri_texcoords; const uint8_t *tri_has_texcoords;
    const int32_t *material_texture, *material_normal_map; const double *material_uv_trans;
    uint32_t n_textures; const uint32_t *texture_size; const uint64_t *texture_offset; const uint8_t *texture_rgb;
} ph_scene_desc;

const char *ph_last_error(void);

int ph_scene_create(const ph_scene_desc *desc, ph_scene **out);
/* The C++ transliterations of the reference's scene scripts (the .cpp files under examples/): "single-triangle",
 * "primitives-simple", "macho-cows", "entering-the-mirror-dimension", "big-scene" (n = objects per
 * axis, ignored by the others). camera = eye3, center3, up3, fovy (radians); size = width, height. */
int ph_example_scene(const char *name, const char *assets_dir, int n, ph_scene **out, double camera[10], uint32_t size[2]);
void ph_scene_destroy(ph_scene *scene);

/* The scene DAG as arrays: unique nodes in depth-first pre-order from the root, materials and meshes
 * in order of first use. counts = nodes, children, meshes, vertices, mesh triangles, triangles,
 * materials, lights. Buffers may be NULL to skip a field. */
int ph_scene_counts(const ph_scene *scene, uint64_t counts[8]);
int ph_scene_export(const ph_scene *scene, double *node_trans /* x16 */, int32_t *prim_type, int32_t *prim_data, int32_t *prim_flags,
                    int32_t *material, uint32_t *child_off, uint32_t *children, uint32_t *root,
                    uint64_t *mesh_vert_off, uint64_t *mesh_tri_off, double *mesh_positions, double *mesh_normals, uint8_t *mesh_has_normals,
                    uint32_t *mesh_indices, double *tri_vertices, double *tri_normals, uint8_t *tri_has_normals,
                    double *materials, double *lights, double ambient[3]);
/* Textures, normal maps and texture coordinates in ph_scene_export's numbering (materials / meshes / triangles in order of
 * first use). counts = {n_textures, texel bytes}; call once with NULL arrays for the counts. */
int ph_scene_export_textures(const ph_scene *s, uint64_t counts[2], int32_t *material_texture, int32_t *material_normal_map,
                             double *material_uv_trans, uint32_t *texture_size, uint64_t *texture_offset, uint8_t *texture_rgb,
                             double *mesh_texcoords, uint8_t *mesh_has_texcoords, double *tri_texcoords, uint8_t *tri_has_texcoords);

/* FlatScene::from (flat_scene.rs:18-46): returns the number of flat nodes; fills up to cap entries. */
int ph_scene_flatten(const ph_scene *scene, uint32_t cap, double *trans, double *invtrans, double *normal_trans,
                     int32_t *prim_type, int32_t *material, double *bounds /* x6: min, max (flat_scene.rs:63-69) */);
/* The hierarchy as PT_TRAVERSE_HIER takes it (pt_scene's ABI-4 arrays; scene.rs:80-120): per flattened node its path through
 * the distinct SceneNodes (root first) and its depth-first rank; per SceneNode its OWN trans / invtrans / normal_trans.
 * Returns the number of flattened nodes; counts = {chain entries, graph nodes}. chain_off needs node_cap + 1 entries. */
int ph_scene_graph(const ph_scene *scene, uint32_t node_cap, uint32_t chain_cap, uint32_t graph_cap, uint32_t *chain_off, uint32_t *chain,
                   uint32_t *dfs_rank, double *graph_trans, double *graph_invtrans, double *graph_normal_trans, uint32_t counts[2]);
/* KDTreeScene::from (kdscene.rs:19-43), linearised like pt_kdtree. Returns the node count. */
int ph_scene_kdtree(const ph_scene *scene, int kd_depth, uint32_t node_cap, uint32_t item_cap, int32_t *axis, double *plane,
                    int32_t *front, int32_t *back, int32_t *first, int32_t *count, int32_t *leaf_items, uint32_t *n_items,
                    double root_bounds[6], int32_t *max_depth);
/* KDMesh::new (kdmesh.rs:37-58) for mesh `mesh` of the scene (meshes are numbered by first use among the flattened nodes, as the
 * upload numbers them): the tree the upload builds for a KDMesh of that mesh, in the same arrays; items are the mesh's own triangle
 * indices. kd_mesh_depth < 0: the environment's KD_MESH_DEPTH, else 10. Needs no GPU and uploads nothing. Returns the node count. */
int ph_scene_kdmesh_tree(const ph_scene *scene, uint32_t mesh, int kd_mesh_depth, uint32_t node_cap, uint32_t item_cap, int32_t *axis, double *plane,
                         int32_t *front, int32_t *back, int32_t *first, int32_t *count, int32_t *leaf_items, uint32_t *n_items,
                         double root_bounds[6], int32_t *max_depth);
/* Camera::new (camera.rs:34-45) */
int ph_camera(const double camera[10], double width, double height, pt_camera *out);
/* MeshData::load_obj (mesh.rs:57-61): counts = vertices, triangles, has_normals; then copy out. */
int ph_obj_load(const char *path, uint64_t counts[3], double *positions, double *normals, uint32_t *indices, uint64_t vert_cap, uint64_t tri_cap);

/* Flatten (+ k-d build for PT_TRAVERSE_KD) and upload to GPU `device`: what render.rs:121-126 does. */
int ph_renderer_create(const ph_scene *scene, int traverse, int kd_depth, int device, ph_renderer **out);
void ph_renderer_destroy(ph_renderer *r);
pt_context *ph_renderer_context(ph_renderer *r);
/* 1, or the number of ranks when PORTRAYER_GPUS / PORTRAYER_DEVICES put the scene on a node (pt_node_*) */
int ph_renderer_ranks(ph_renderer *r);
/* the pt_node behind the renderer in that case (NULL on a single GPU): for callers that drive pt_node_render_resident themselves */
pt_node *ph_renderer_node(ph_renderer *r);
/* where the time before the first pixel went, in ms: flatten (flat_scene.rs:18-46), packing the ABI arrays, context / node
 * creation, the reference's k-d tree build (kdtree feature only), pt_scene_upload (device trees included) */
int ph_renderer_prepare_ms(ph_renderer *r, double out[5]);
/* The pixel loop (render.rs:127-150) on the GPU, host buffers in and out (see pt_render). */
int ph_renderer_render(ph_renderer *r, const double camera[10], const pt_render_params *params, const double *background,
                       uint8_t *rgb, double *linear, pt_stats *stats);

/* What is under each pixel (see pt_aov): one primary ray per pixel of params->slice through the camera a render of that size would use,
 * host buffers out, each optional. A renderer spread over a node runs the pass on rank 0's context.
 * `node` indexes the flattened nodes (ph_scene_flatten's order); `material` indexes the renderer's material table, which lists the scene's materials in the
 * order the flattened nodes first use them: the numbering of ph_scene_flatten's `material` array, NOT that of ph_scene_export's `materials`. */
int ph_renderer_aov(ph_renderer *r, const double camera[10], const pt_aov_params *params, const pt_aov_buffers *out, double *kernel_ms);

/* What a denoiser needs of each pixel (see pt_guides): the same pass with the diffuse colour under the pixel (`albedo`) beside position, normal and node,
 * in one trace; host buffers out, each optional. The camera, the slice and `node` are ph_renderer_aov's. */
int ph_renderer_guides(ph_renderer *r, const double camera[10], const pt_aov_params *params, const pt_guides_buffers *out, double *kernel_ms);

/* Rays of the caller's own (see pt_rays): n x 3 f64 origins and directions in world space, host buffers out, each optional; any_hit = 1 answers `occluded`
 * only. A renderer spread over a node runs the pass on rank 0's context. `node` and `material` are numbered as for ph_renderer_aov. */
int ph_renderer_rays(ph_renderer *r, const pt_rays_params *params, const double *origins, const double *directions, const pt_rays_buffers *out, double *kernel_ms);
/* The same over bounded segments (see pt_segments): t_max holds n f64, ray i answers for hits with EPSILON <= t < t_max[i]; a NaN or <= EPSILON bound is an
 * empty range and reports a miss. */
int ph_renderer_segments(ph_renderer *r, const pt_rays_params *params, const double *origins, const double *directions, const double *t_max, const pt_rays_buffers *out,
                         double *kernel_ms);

/* The resident scene moved (pt_scene_update): `scene` must have the structure of the one the renderer was created from - ph_scene_same_structure - and may
 * differ in transforms, lights' values and ambient light; PH_ERR_ARGUMENT names the first difference otherwise and the renderer keeps its scene. Only node
 * matrices, lights and (k-d traversal) the rebuilt reference k-d tree go to the device: meshes, their trees and textures stay where they are. A renderer
 * spread over a node updates every rank. */
int ph_renderer_update(ph_renderer *r, const ph_scene *scene);
/* 1 if `b` is `a` moved (same flattened nodes in the same order: primitive kinds, meshes / triangles, shading, materials, paths through the graph; as many
 * lights), 0 if not, with the first difference in `why` (n bytes, optional), or a negative PH_ERR_* code. Needs no GPU. */
int ph_scene_same_structure(const ph_scene *a, const ph_scene *b, char *why, size_t n);
/* Resident meshes deformed (pt_scene_deform): `scene` must have the topology of the one the renderer was created from - ph_scene_same_topology: the same
 * structure, except that a mesh may differ in the values of its vertex positions and normals; PH_ERR_ARGUMENT names the first difference otherwise and the
 * renderer keeps its scene. The meshes whose positions or normals differ in a bit are sent - vertices and bounds only; indices, texture coordinates and
 * textures stay on the device - and their trees are refitted there; rebuild != 0 rebuilds the trees the device built at upload instead and refits the
 * others. Transforms, lights and ambient light move as in ph_renderer_update. Meshes with KDMesh trees cannot be deformed (PH_ERR_RUNTIME). */
int ph_renderer_deform(ph_renderer *r, const ph_scene *scene, int rebuild);
/* As ph_scene_same_structure, for ph_renderer_deform: vertex count, triangles, texture coordinates and presence of normals of a mesh must be equal, the
 * values of positions and normals may differ. */
int ph_scene_same_topology(const ph_scene *a, const ph_scene *b, char *why, size_t n);
/* Resident meshes deformed from vertices that are already in the memory of the renderer's device (pt_vertex_bounds_device + pt_scene_deform_device): per
 * mesh its index in the renderer's numbering (the order in which the flattened nodes first use the meshes: ph_renderer_deform's), a device pointer to
 * n_vertices x 3 doubles and optionally one to as many normals (NULL: the resident normals stay). `moved` may be NULL; otherwise it must have the structure of
 * the resident scene (ph_scene_same_structure) and its transforms, lights and ambient light move as in ph_renderer_update. rebuild as in ph_renderer_deform.
 * Nothing per vertex crosses the bus. The call is synchronous and ordered behind every stream of the device (see pt_scene_deform_device). A mesh deformed
 * this way is remembered as posed on the device: a later ph_renderer_deform sends it whatever its comparison against the host's copy says.
 * PH_ERR_ARGUMENT: the k-d traversal (its tree is built by the host from the meshes' bounds, which the host no longer has; the C ABI supports it with the
 * caller's tree), a renderer with several ranks (each rank's device needs its own copy of the vertices), a mesh index out of range, another structure.
 * PH_ERR_RUNTIME: what the library refuses (a pointer that is not device memory of that device, non-finite coordinates, ...). */
typedef struct { uint32_t mesh; const double *d_positions; const double *d_normals; } ph_device_mesh;
int ph_renderer_deform_device(ph_renderer *r, uint32_t n_meshes, const ph_device_mesh *meshes, int rebuild, const ph_scene *moved);
/* Distinct meshes of the renderer's scene, and the vertex count of mesh `mesh` in the renderer's numbering (negative: PH_ERR_*). Need no GPU work. */
int64_t ph_renderer_mesh_count(ph_renderer *r);
int64_t ph_renderer_mesh_vertices(ph_renderer *r, uint32_t mesh);

/* Ambient occlusion at points of the caller's own (see pt_ao): n x 3 f64 positions and normals in world space, host buffers out, each optional. A renderer
 * spread over a node runs the pass on rank 0's context. n = 0 is PH_OK. */
int ph_renderer_ao(ph_renderer *r, const pt_ao_params *params, const double *positions, const double *normals, const pt_ao_buffers *out, double *kernel_ms);
/* Ambient occlusion under every pixel of a width x height image, through the camera a render of that size would use: a primary-visibility pass at the pixel
 * centres writes position and normal into device memory kept with the renderer, and pt_ao_device reads them there on the same stream with PT_AO_FACE_EYE and
 * the camera's eye; point q = y * width + x. Of `params` samples, pass, seed, radius and bias are read (n, first_index, flags and eye are set here). Host
 * buffers out, width x height entries each, each optional: nothing per pixel crosses the bus but the results. kernel_ms: the ambient-occlusion pass's. */
int ph_renderer_ao_camera(ph_renderer *r, const double camera[10], uint32_t width, uint32_t height, const pt_ao_params *params, const pt_ao_buffers *out,
                          double *kernel_ms);

/* Gathered radiance at points of the caller's own (see pt_gather): n x 3 f64 positions and normals in world space, `background` 3 doubles, host buffers out,
 * each optional: per point the sum of `samples` shaded samples along the ambient-occlusion pass's rays. A renderer spread over a node runs the pass on rank 0's
 * context. n = 0 is PH_OK. */
int ph_renderer_gather(ph_renderer *r, const pt_gather_params *params, const double *positions, const double *normals, const double *background,
                       const pt_gather_buffers *out, double *kernel_ms);
/* Gathered radiance under every pixel of a width x height image, through the camera a render of that size would use, built like ph_renderer_ao_camera: a
 * primary-visibility pass at the pixel centres writes position and normal into device memory kept with the renderer, and pt_gather_device reads them there on
 * the same stream with PT_AO_FACE_EYE and the camera's eye; point q = y * width + x. Of `params` samples, pass, seed and bias are read (n, first_index, flags
 * and eye are set here). Host buffers out, width x height entries each, each optional: nothing per pixel crosses the bus but the results. kernel_ms: the gather
 * pass's. */
int ph_renderer_gather_camera(ph_renderer *r, const double camera[10], uint32_t width, uint32_t height, const pt_gather_params *params, const double *background,
                              const pt_gather_buffers *out, double *kernel_ms);

/* A mesh's light-map texels as surface points (see pt_chart): `params->node` indexes the flattened nodes, `uv` is T x 6 f64 per corner (ph_renderer_chart_triangles
 * gives T) or NULL for the mesh's own texture coordinates; host buffers out, width x height entries each, each optional. A renderer spread over a node runs the
 * pass on rank 0's context. */
int ph_renderer_chart_triangles(ph_renderer *r, uint32_t node, uint64_t *n_tris);
/* The mesh under flattened node `node`: counts = {vertices, triangles}; `indices` (optional): cap_tris x 3 vertex indices, cap_tris = the triangle count - what
 * expands a per-vertex UV set to corners. PH_ERR_ARGUMENT for a node that is out of range or no mesh. Needs no GPU work. */
int ph_renderer_chart_mesh(ph_renderer *r, uint32_t node, uint64_t counts[2], uint32_t cap_tris, uint32_t *indices);
int ph_renderer_chart(ph_renderer *r, const pt_chart_params *params, const double *uv, const pt_chart_buffers *out, double *kernel_ms);
/* Ambient occlusion and gathered radiance at every texel of a mesh's light map, built like ph_renderer_ao_camera / ph_renderer_gather_camera: pt_chart_device
 * writes position and normal into device memory kept with the renderer, and pt_ao_device / pt_gather_device reads them there on the same stream; point
 * q = y * width + x. Of `params` samples, pass, seed, radius and bias are read (n = width x height, first_index = 0 and flags = 0 are set here: a chart's normals
 * are turned by PT_CHART_FLIP_NORMAL, not towards an eye). Host buffers out, each optional: nothing per texel crosses the bus but the results; texels no
 * triangle owns are invalid points. kernel_ms: the ambient-occlusion / gather pass's. */
int ph_renderer_ao_chart(ph_renderer *r, const pt_chart_params *chart, const double *uv, const pt_ao_params *params, const pt_ao_buffers *out, double *kernel_ms);
int ph_renderer_gather_chart(ph_renderer *r, const pt_chart_params *chart, const double *uv, const pt_gather_params *params, const double *background,
                             const pt_gather_buffers *out, double *kernel_ms);

/* Direct light at points of the caller's own (see pt_direct): n x 3 f64 positions and normals in world space, host buffers out, each optional: per point the
 * sum of the cosine-weighted light that arrives unoccluded from the scene's lights, `samples` samples per area light. A renderer spread over a node runs the
 * pass on rank 0's context. n = 0 is PH_OK. */
int ph_renderer_direct(ph_renderer *r, const pt_direct_params *params, const double *positions, const double *normals, const pt_direct_buffers *out, double *kernel_ms);
/* Direct light under every pixel of a width x height image and at every texel of a mesh's light map, built like ph_renderer_ao_camera / ph_renderer_ao_chart and
 * on their device scratch: pt_aov_device / pt_chart_device writes position and normal into device memory kept with the renderer, and pt_direct_device reads them
 * there on the same stream; point q = y * width + x. Of `params` samples, pass, seed, bias and the flag PT_DIRECT_TO_LIGHT are read (n and first_index = 0 are
 * set here; the camera form runs with PT_AO_FACE_EYE and the camera's eye, the chart form without). Host buffers out, width x height entries each, each
 * optional: nothing per point crosses the bus but the results. kernel_ms: the direct-light pass's. */
int ph_renderer_direct_camera(ph_renderer *r, const double camera[10], uint32_t width, uint32_t height, const pt_direct_params *params, const pt_direct_buffers *out,
                              double *kernel_ms);
int ph_renderer_direct_chart(ph_renderer *r, const pt_chart_params *chart, const double *uv, const pt_direct_params *params, const pt_direct_buffers *out,
                             double *kernel_ms);

/* Light probes at points in free space (see pt_probe): n x 3 f64 positions in world space, no normals, `background` 3 doubles, host buffers out, each optional:
 * per probe the nine order-2 spherical-harmonic sums (9 x 3 f64) of `samples` shaded samples over the whole sphere. A renderer spread over a node runs the pass
 * on rank 0's context. n = 0 is PH_OK. */
int ph_renderer_probe(ph_renderer *r, const pt_probe_params *params, const double *positions, const double *background, const pt_probe_buffers *out,
                      double *kernel_ms);

/* Radiance along rays of the caller's own (see pt_radiance): n x 3 f64 origins and directions in world space, `background` 3 doubles or n x 3
 * (params->background_per_ray), rgb n x 3 f64 out: one linear sample of Ray::color per ray. A renderer spread over a node runs the pass on rank 0's context. */
int ph_renderer_radiance(ph_renderer *r, const pt_radiance_params *params, const double *origins, const double *directions, const double *background, double *rgb,
                         double *kernel_ms);

/* A film of the renderer (see pt_film_create ... pt_film_counts): samples accumulate in device memory, add after add, and ph_renderer_film_resolve gives at
 * every pixel the bits of a render with that pixel's count of samples. `camera` as for ph_renderer_render: the camera a render of the film's size gets. The
 * background is height x width x 3 doubles, or height x 3 with params->background_rows. A renderer spread over several ranks (PORTRAYER_GPUS) refuses to
 * create a film (PH_ERR_ARGUMENT): a film lives on one device. PH_ERR_PANIC: a slice corner outside the film; PH_ERR_RUNTIME: what the library refuses. */
typedef struct ph_film ph_film;
int ph_renderer_film_create(ph_renderer *r, uint32_t width, uint32_t height, ph_film **out);
int ph_renderer_film_destroy(ph_renderer *r, ph_film *film);   /* before the renderer; films still alive die with it */
int ph_renderer_film_reset(ph_renderer *r, ph_film *film);
int ph_renderer_film_add(ph_renderer *r, ph_film *film, const double camera[10], const double *background, const pt_film_params *params, double *kernel_ms);
/* The same samples behind a lens (see pt_film_add_lens): a thin lens, an orthographic or a stereographic camera in place of the pinhole. */
int ph_renderer_film_add_lens(ph_renderer *r, ph_film *film, const double camera[10], const pt_lens *lens, const double *background, const pt_film_params *params,
                              double *kernel_ms);
int ph_renderer_film_resolve(ph_renderer *r, ph_film *film, uint8_t *rgb, double *linear);   /* either may be NULL, not both */
int ph_renderer_film_counts(ph_renderer *r, ph_film *film, uint32_t *counts);
/* The adaptive film (pt_film_create_moments, pt_film_add_map, pt_film_error, pt_film_budget_device): a film that also keeps the second moment of its samples;
 * an add with a budget per pixel (`budget`: width x height u32, only params->slice is read); the standard error of every pixel's mean (width x height f64,
 * +inf below 2 samples); and the closed loop - budget on the device, add what it asks for, until no pixel of refine->slice is below min_count or above the
 * threshold (and below max_count), or max_passes have run. `sampling` gives refine its seed, sample_mode and background_rows (its slice and max_samples are
 * ignored: refine->slice, refine->step). out[3]: passes run, samples added, pixels that still wanted samples at the end. kernel_ms (optional): device time
 * of the adds. */
int ph_renderer_film_create_moments(ph_renderer *r, uint32_t width, uint32_t height, ph_film **out);
int ph_renderer_film_add_map(ph_renderer *r, ph_film *film, const double camera[10], const double *background, const pt_film_map_params *params, const uint32_t *budget, double *kernel_ms);
int ph_renderer_film_error(ph_renderer *r, ph_film *film, double *err);
int ph_renderer_film_refine(ph_renderer *r, ph_film *film, const double camera[10], const double *background, const pt_film_map_params *sampling, const pt_film_refine_params *refine,
                            uint32_t max_passes, uint64_t out[3], double *kernel_ms);
/* The film, denoised (pt_film_denoise: an a-trous filter over the resolved mean; lossy, the film's state is not written). With `guides` (host arrays laid out as
 * pt_aov writes them) this is the library's host path and `camera` may be NULL. With guides == NULL the guides are what is under each pixel centre for `camera`:
 * a primary-visibility pass into device buffers kept with the film handle, then the filter, on the device throughout; only the outputs asked for are copied out.
 * rgb (width x height x 3 u8), linear (x 3 f64) and variance (f64) are each optional, not all NULL; pixels without samples keep what they hold. */
int ph_renderer_film_denoise(ph_renderer *r, ph_film *film, const double camera[10], const pt_denoise_params *params, const pt_denoise_guides *guides, uint8_t *rgb, double *linear,
                             double *variance);
/* The same on demodulated colour (pt_film_denoise_albedo). With `guides` AND `albedo` (host arrays as pt_guides writes them; one without the other is refused)
 * it is the library's host path. With both NULL, ONE guides pass for `camera` writes albedo, guides and node into device buffers kept with the film handle,
 * then pt_film_denoise_albedo_device; only the outputs asked for are copied out. */
int ph_renderer_film_denoise_albedo(ph_renderer *r, ph_film *film, const double camera[10], const pt_denoise_params *params, const pt_denoise_guides *guides, const double *albedo,
                                    uint8_t *rgb, double *linear, double *variance);

/* Image::new + Image::render + Image::save with the crate's defaults (env SAMPLES, KD_DEPTH) on an
 * example scene: exercises the whole C++ API the way the reference's main() does. */
int ph_example_render_to_png(const char *name, const char *assets_dir, int n, uint32_t width, uint32_t height, const char *png_path);
int ph_png_read(const char *path, uint32_t size[2], uint8_t *rgb, uint64_t cap);
int ph_png_write(const char *path, uint32_t width, uint32_t height, const uint8_t *rgb);
/* Texture files as texture::RgbImageBuffer::open reads them (src/texture.rs:104-141 via the `image` crate): PNG or
 * JPEG (baseline and progressive), decoded to RGB8. size = {width, height}; rgb may be NULL to query the size. */
int ph_image_read(const char *path, uint32_t size[2], uint8_t *rgb, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif
