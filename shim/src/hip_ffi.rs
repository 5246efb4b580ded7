//! Declarations of the C ABI in include/portrayer_hip.h (PT_ABI_VERSION 8), field for field.
//! tests/test_integration_doc.py of the MI355X repository checks these structs against the header.
#![allow(dead_code)]

use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] pub struct PtContext { _private: [u8; 0] }
#[repr(C)] pub struct PtNode { _private: [u8; 0] }
#[repr(C)] pub struct PtFilm { _private: [u8; 0] }

pub const PT_ABI_VERSION: c_int = 8;

// enum Primitive, src/primitive.rs:67-81
pub const PT_PRIM_SPHERE: i32 = 0;
pub const PT_PRIM_TRIANGLE: i32 = 1;
pub const PT_PRIM_MESH: i32 = 2;
pub const PT_PRIM_KDMESH: i32 = 3;
pub const PT_PRIM_PLANE: i32 = 4;
pub const PT_PRIM_CUBE: i32 = 5;
pub const PT_PRIM_CYLINDER: i32 = 6;
pub const PT_PRIM_CONE: i32 = 7;

// cargo features flat_scene / kdtree / neither, src/render.rs:121-126
pub const PT_TRAVERSE_FLAT: c_int = 1;
pub const PT_TRAVERSE_KD: c_int = 2;
pub const PT_TRAVERSE_HIER: c_int = 3;

pub const PT_SAMPLE_CENTRE: i32 = 0;
pub const PT_SAMPLE_RNG: i32 = 1;

pub const PT_OK: c_int = 0;
pub const PT_ERR_SLICE: c_int = -4;
pub const PT_ERR_SCENE: c_int = -5;

#[repr(C)]
pub struct PtScene {                       // pt_scene
    pub n_nodes: u32,
    pub trans: *const f64, pub invtrans: *const f64, pub normal_trans: *const f64,   // n x 16, row-major
    pub prim_type: *const i32, pub prim_data: *const i32, pub prim_flags: *const i32, pub material: *const i32,
    pub n_meshes: u32,
    pub mesh_vert_off: *const u64, pub mesh_tri_off: *const u64,
    pub mesh_positions: *const f64, pub mesh_normals: *const f64, pub mesh_has_normals: *const u8,
    pub mesh_indices: *const u32, pub mesh_bounds_invtrans: *const f64,
    pub n_triangles: u32, pub tri_vertices: *const f64, pub tri_normals: *const f64,
    pub n_materials: u32, pub materials: *const f64,      // x 10
    pub n_lights: u32, pub lights: *const f64,            // x 15
    pub ambient: [f64; 3],
    // ABI 2: textures (src/texture.rs); null / 0 when the scene has none
    pub mesh_texcoords: *const f64, pub mesh_has_texcoords: *const u8,
    pub tri_texcoords: *const f64, pub tri_has_texcoords: *const u8,
    pub material_texture: *const i32, pub material_normal_map: *const i32, pub material_uv_trans: *const f64,
    pub n_textures: u32, pub texture_size: *const u32, pub texture_offset: *const u64, pub texture_rgb: *const u8,
    // ABI 3: KDMesh triangle trees (src/kdtree/kdmesh.rs), linearised like PtKdTree; null when unused
    pub mesh_kd_root: *const i32, pub mesh_kd_depth: *const i32, pub mesh_kd_bounds: *const f64, pub mesh_kd_bounds_invtrans: *const f64,
    pub n_kdm_nodes: u32, pub kdm_axis: *const i32, pub kdm_plane: *const f64, pub kdm_front: *const i32, pub kdm_back: *const i32,
    pub kdm_first: *const i32, pub kdm_count: *const i32, pub n_kdm_items: u32, pub kdm_items: *const i32,
    // ABI 4: the scene graph for PT_TRAVERSE_HIER = the crate's DEFAULT traversal (src/scene.rs:80-120); null / 0 otherwise
    pub n_graph_nodes: u32, pub graph_trans: *const f64, pub graph_invtrans: *const f64, pub graph_normal_trans: *const f64,
    pub node_chain_off: *const u32, pub node_chain: *const u32, pub node_dfs_rank: *const u32,
}

#[repr(C)]
pub struct PtKdTree {                      // pt_kdtree
    pub n_nodes: u32,
    pub axis: *const i32, pub plane: *const f64, pub front: *const i32, pub back: *const i32,
    pub first: *const i32, pub count: *const i32,
    pub n_items: u32, pub leaf_items: *const i32,
    pub root_min: [f64; 3], pub root_max: [f64; 3], pub max_depth: i32,
}

#[repr(C)]
pub struct PtSceneMotion {                 // pt_scene_motion: the resident scene's new matrices, lights and ambient light (pt_scene_update)
    pub n_nodes: u32,
    pub trans: *const f64, pub invtrans: *const f64, pub normal_trans: *const f64,
    pub n_graph_nodes: u32,
    pub graph_trans: *const f64, pub graph_invtrans: *const f64, pub graph_normal_trans: *const f64,
    pub n_lights: u32,
    pub lights: *const f64,
    pub ambient: *const f64,
}

#[repr(C)]
pub struct PtMeshDeformDevice {            // pt_mesh_deform_device: a resident mesh's new vertices, already in device memory (pt_scene_deform_device)
    pub mesh: u32,
    pub d_positions: *const f64,           // DEVICE, n_vertices x 3
    pub d_normals: *const f64,             // DEVICE, n_vertices x 3, or null
    pub bounds_invtrans: *const f64,       // HOST, 16 doubles
    pub rebuild: i32,
}

#[repr(C)] pub struct PtCamera { pub eye: [f64; 3], pub view_to_world: [f64; 16], pub fov_factor: f64, pub aspect_ratio: f64, pub width: f64, pub height: f64 }
#[repr(C)] pub struct PtRect { pub x0: u32, pub y0: u32, pub x1: u32, pub y1: u32 }

#[repr(C)]
pub struct PtRenderParams {
    pub width: u32, pub height: u32, pub slice: PtRect, pub samples: u32, pub seed: u64,
    pub sample_mode: i32, pub background_rows: i32, pub tile_rank: u32, pub tile_ranks: u32, pub collect_stats: i32,
}

#[repr(C)] pub struct PtAovParams { pub width: u32, pub height: u32, pub slice: PtRect, pub offset: [f64; 2] }   // pt_aov_params: offset (0.5, 0.5) = the pixel centre
#[repr(C)]
pub struct PtAovBuffers {                  // pt_aov_buffers: each optional (null = not wanted), full image, row-major
    pub depth: *mut f64, pub position: *mut f64, pub normal: *mut f64, pub node: *mut i32, pub sub: *mut i32, pub material: *mut i32,
}
#[repr(C)]
pub struct PtGuidesBuffers {               // pt_guides_buffers: each optional (null = not wanted), full image, row-major; albedo width x height x 3 f64, the rest as in pt_aov_buffers
    pub albedo: *mut f64, pub position: *mut f64, pub normal: *mut f64, pub node: *mut i32,
}
#[repr(C)]
pub struct PtAoParams {                    // pt_ao_params: n points; samples 1, 2, 4 .. 64 rays each; point i draws its rotation from the stream (seed, first_index + i, pass)
    pub n: u64, pub samples: u32, pub pass: u32, pub seed: u64, pub first_index: u64,
    pub radius: f64, pub bias: f64, pub flags: u32, pub eye: [f64; 3],
}
#[repr(C)]
pub struct PtAoBuffers {                   // pt_ao_buffers: each optional (null = not wanted), n entries; occluded = rays that met something, bent n x 3 = sum of the others' directions
    pub occluded: *mut u32, pub valid: *mut u8, pub bent: *mut f64,
}
pub const PT_AO_FACE_EYE: u32 = 1;         // PtAoParams.flags: turn each normal towards `eye` first
#[repr(C)]
pub struct PtGatherParams {                // pt_gather_params: pt_ao_params without the radius; ray k of point i draws from the stream (seed, (first_index + i) * samples + k, pass)
    pub n: u64, pub samples: u32, pub pass: u32, pub seed: u64, pub first_index: u64,
    pub bias: f64, pub flags: u32, pub eye: [f64; 3],
}
#[repr(C)]
pub struct PtGatherBuffers {               // pt_gather_buffers: each optional (null = not wanted), n entries; sum n x 3 = a point's shaded samples added in order
    pub sum: *mut f64, pub valid: *mut u8,
}
#[repr(C)]
pub struct PtDirectParams {                // pt_direct_params: pt_ao_params without the radius; sample k of point i at an area light draws from the stream (seed, (first_index + i) * samples + k, pass)
    pub n: u64, pub samples: u32, pub pass: u32, pub seed: u64, pub first_index: u64,
    pub bias: f64, pub flags: u32, pub eye: [f64; 3],
}
#[repr(C)]
pub struct PtDirectBuffers {               // pt_direct_buffers: each optional (null = not wanted), n entries; sum n x 3 = the unoccluded lights' terms added in order, lit = how many
    pub sum: *mut f64, pub lit: *mut u32, pub valid: *mut u8,
}
pub const PT_DIRECT_TO_LIGHT: u32 = 2;     // PtDirectParams.flags (beside PT_AO_FACE_EYE): the shadow segment ends at the light
#[repr(C)]
pub struct PtChartParams { pub node: u32, pub width: u32, pub height: u32, pub flags: u32 }   // pt_chart_params: a flattened mesh node, its light map's size, 0 or PT_CHART_FLIP_NORMAL
#[repr(C)]
pub struct PtChartBuffers {                // pt_chart_buffers: each optional (null = not wanted), width x height entries, row-major; tri = the owning triangle or -1
    pub position: *mut f64, pub normal: *mut f64, pub tri: *mut i32, pub covered: *mut u8,
}
pub const PT_CHART_FLIP_NORMAL: u32 = 1;   // PtChartParams.flags: negate every normal (the inside of a room)
#[repr(C)]
pub struct PtProbeParams {                 // pt_probe_params: a probe has no normal and no bias; ray k of probe i draws from the stream (seed, (first_index + i) * samples + k, pass)
    pub n: u64, pub samples: u32, pub pass: u32, pub seed: u64, pub first_index: u64,
}
#[repr(C)]
pub struct PtProbeBuffers {                // pt_probe_buffers: each optional (null = not wanted), n entries; sh n x 9 x 3 = a probe's order-2 SH sums, x 4 pi / samples the coefficients
    pub sh: *mut f64, pub valid: *mut u8,
}
pub const PT_PROBE_MAX: u64 = 1 << 20;     // probes per call
#[repr(C)] pub struct PtRaysParams { pub n: u64, pub any_hit: i32, pub reorder: i32 }   // pt_rays_params: any_hit 1 = occlusion query, reorder 1 = the device groups like rays first
#[repr(C)]
pub struct PtRadianceParams {              // pt_radiance_params: ray i draws from the generator's stream (seed, stream_base + i, sample), draws 2, 3, ...
    pub n: u64, pub reorder: i32, pub background_per_ray: i32, pub seed: u64, pub stream_base: u64, pub sample: u32,
}
#[repr(C)]
pub struct PtFilmParams {                  // pt_film_params: one add to a film - `samples` more samples for every pixel of `slice`, taken as pt_render takes them
    pub slice: PtRect, pub samples: u32, pub seed: u64, pub sample_mode: i32, pub background_rows: i32,
}
#[repr(C)]
pub struct PtLens {                        // pt_lens: what stands in for the pinhole in pt_film_add_lens; model 0 thin lens (aperture, focus), 1 orthographic, 2 stereographic (extent)
    pub model: i32, pub aperture: f64, pub focus: f64, pub extent: f64,
}
#[repr(C)]
pub struct PtFilmMapParams {               // pt_film_map_params: one add with a budget per pixel - pixel p of `slice` gets its next min(budget[p], max_samples) samples
    pub slice: PtRect, pub max_samples: u32, pub seed: u64, pub sample_mode: i32, pub background_rows: i32,
}
#[repr(C)]
pub struct PtFilmRefineParams {            // pt_film_refine_params: the budget of a refine pass - up to `step` below min_count, or below max_count with an error above the threshold
    pub slice: PtRect, pub threshold: f64, pub min_count: u32, pub max_count: u32, pub step: u32,
}
#[repr(C)]
pub struct PtDenoiseParams {               // pt_denoise_params: the levels of pt_film_denoise's a-trous filter and its edge-stopping weights (0 / -1 = off); flags: PT_DENOISE_SAME_NODE = 1
    pub iterations: i32, pub flags: u32, pub sigma_color: f64, pub sigma_plane: f64, pub normal_power_log2: i32,
}
#[repr(C)]
pub struct PtDenoiseGuides {               // pt_denoise_guides: full images as pt_aov writes them; node always, normal / position where a weight reads them
    pub position: *const f64, pub normal: *const f64, pub node: *const i32,
}
#[repr(C)]
pub struct PtRaysBuffers {                 // pt_rays_buffers: each optional (null = not wanted), n entries, indexed like the rays
    pub t: *mut f64, pub position: *mut f64, pub normal: *mut f64, pub node: *mut i32, pub sub: *mut i32, pub material: *mut i32, pub occluded: *mut u8,
}
#[repr(C)] #[derive(Default)]
pub struct PtStats {
    pub primary: u64, pub shadow: u64, pub reflect: u64, pub refract: u64, pub depth11_skipped: u64, pub hits: u64,
    pub n_inner: u64, pub n_leaf: u64, pub n_analytic: u64, pub n_tri: u64, pub n_bbox: u64,
    pub kd_plane_miss: u64, pub stack_overflow: u64, pub kernel_ms: f64, pub total_ms: f64,
    pub diag: [u64; 8],
    pub kernel_mode: u32, pub kernel_variant: u32,
}

extern "C" {
    pub fn pt_abi_version() -> c_int;
    pub fn pt_device_count() -> c_int;
    pub fn pt_context_create(device: c_int, out: *mut *mut PtContext) -> c_int;
    pub fn pt_context_destroy(ctx: *mut PtContext);
    pub fn pt_last_error(ctx: *const PtContext) -> *const c_char;
    pub fn pt_scene_upload(ctx: *mut PtContext, scene: *const PtScene, traverse: c_int, kd: *const PtKdTree) -> c_int;
    // move the resident scene: new node matrices, lights, ambient light; only the scene-level tree is rebuilt
    pub fn pt_scene_update(ctx: *mut PtContext, motion: *const PtSceneMotion, kd: *const PtKdTree) -> c_int;
    // deform resident meshes from vertices in device memory: the box of such vertices (min xyz, max xyz; count of NaN / inf coordinates), then the deform
    pub fn pt_vertex_bounds_device(ctx: *mut PtContext, n_vertices: u64, d_positions: *const f64, out: *mut f64, non_finite: *mut u64) -> c_int;
    pub fn pt_scene_deform_device(ctx: *mut PtContext, n_deforms: u32, deforms: *const PtMeshDeformDevice, motion: *const PtSceneMotion,
                                  kd: *const PtKdTree) -> c_int;
    pub fn pt_render(ctx: *mut PtContext, camera: *const PtCamera, background: *const f64, params: *const PtRenderParams,
                     rgb: *mut u8, linear: *mut f64, stats: *mut PtStats) -> c_int;
    pub fn pt_render_device(ctx: *mut PtContext, camera: *const PtCamera, d_background: *const f64, params: *const PtRenderParams,
                            compact: c_int, d_rgb: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn pt_render_finish(ctx: *mut PtContext, stats: *mut PtStats) -> c_int;
    // what is under each pixel: one primary ray per pixel of the slice, no shading (depth, position, normal, node / triangle / material ids)
    pub fn pt_aov(ctx: *mut PtContext, camera: *const PtCamera, params: *const PtAovParams, host_out: *const PtAovBuffers, kernel_ms: *mut f64) -> c_int;
    pub fn pt_aov_device(ctx: *mut PtContext, camera: *const PtCamera, params: *const PtAovParams, device_out: *const PtAovBuffers,
                         hip_stream: *mut c_void) -> c_int;
    pub fn pt_aov_finish(ctx: *mut PtContext, kernel_ms: *mut f64) -> c_int;
    // what a denoiser needs of each pixel, in one trace: pt_aov's pass with the diffuse colour under the pixel (albedo) beside position, normal and node.
    // Shares pt_aov's pass: one pass of either kind in flight per context, and pt_guides_finish is pt_aov_finish
    pub fn pt_guides(ctx: *mut PtContext, camera: *const PtCamera, params: *const PtAovParams, host_out: *const PtGuidesBuffers, kernel_ms: *mut f64) -> c_int;
    pub fn pt_guides_device(ctx: *mut PtContext, camera: *const PtCamera, params: *const PtAovParams, device_out: *const PtGuidesBuffers,
                            hip_stream: *mut c_void) -> c_int;
    pub fn pt_guides_finish(ctx: *mut PtContext, kernel_ms: *mut f64) -> c_int;
    // rays of the caller's own: nearest hit (t, position, normal, ids) or occlusion per ray; n x 3 f64 origins and directions in world space
    pub fn pt_rays(ctx: *mut PtContext, params: *const PtRaysParams, origins: *const f64, directions: *const f64, host_out: *const PtRaysBuffers,
                   kernel_ms: *mut f64) -> c_int;
    pub fn pt_rays_device(ctx: *mut PtContext, params: *const PtRaysParams, d_origins: *const f64, d_directions: *const f64, device_out: *const PtRaysBuffers,
                          hip_stream: *mut c_void) -> c_int;
    pub fn pt_rays_finish(ctx: *mut PtContext, kernel_ms: *mut f64) -> c_int;
    // the same over bounded segments: t_max holds n f64 (units of the direction, like t); ray i answers for hits with EPSILON <= t < t_max[i], a NaN or
    // <= EPSILON bound reports a miss. Shares pt_rays' pass: pt_segments_device is closed by pt_rays_finish, one pass of either kind in flight per context.
    pub fn pt_segments(ctx: *mut PtContext, params: *const PtRaysParams, origins: *const f64, directions: *const f64, t_max: *const f64,
                       host_out: *const PtRaysBuffers, kernel_ms: *mut f64) -> c_int;
    pub fn pt_segments_device(ctx: *mut PtContext, params: *const PtRaysParams, d_origins: *const f64, d_directions: *const f64, d_t_max: *const f64,
                              device_out: *const PtRaysBuffers, hip_stream: *mut c_void) -> c_int;
    // ambient occlusion at points of the caller's own: n x 3 f64 positions and normals in world space; the device makes each point's rays in registers (a fixed
    // sequence of f64 operations, pt_ao.h), walks them over [EPSILON, radius) and counts. Shares pt_rays' pass: pt_ao_device is closed by pt_ao_finish, which is
    // pt_rays_finish; queued behind pt_aov_device on the same stream it reads that pass's position and normal where they are
    pub fn pt_ao(ctx: *mut PtContext, params: *const PtAoParams, positions: *const f64, normals: *const f64, host_out: *const PtAoBuffers,
                 kernel_ms: *mut f64) -> c_int;
    pub fn pt_ao_device(ctx: *mut PtContext, params: *const PtAoParams, d_positions: *const f64, d_normals: *const f64, device_out: *const PtAoBuffers,
                        hip_stream: *mut c_void) -> c_int;
    pub fn pt_ao_finish(ctx: *mut PtContext, kernel_ms: *mut f64) -> c_int;
    // radiance along rays of the caller's own (Ray::color as a batch): background 3 f64 or n x 3 (background_per_ray), rgb n x 3 f64, one linear sample per ray
    pub fn pt_radiance(ctx: *mut PtContext, params: *const PtRadianceParams, origins: *const f64, directions: *const f64, background: *const f64, rgb: *mut f64,
                       kernel_ms: *mut f64) -> c_int;
    pub fn pt_radiance_device(ctx: *mut PtContext, params: *const PtRadianceParams, d_origins: *const f64, d_directions: *const f64, d_background: *const f64,
                              d_rgb: *mut f64, hip_stream: *mut c_void) -> c_int;
    pub fn pt_radiance_finish(ctx: *mut PtContext, kernel_ms: *mut f64) -> c_int;
    // gathered radiance at points of the caller's own: per point the sum of `samples` shaded samples (what pt_radiance answers) along pt_ao's rays, made in
    // registers; background 3 f64 on the HOST in both forms. A radiance pass for bookkeeping: pt_gather_device is closed by pt_gather_finish, which is
    // pt_radiance_finish; queued behind pt_aov_device on the same stream it reads that pass's position and normal where they are
    pub fn pt_gather(ctx: *mut PtContext, params: *const PtGatherParams, positions: *const f64, normals: *const f64, background: *const f64,
                     host_out: *const PtGatherBuffers, kernel_ms: *mut f64) -> c_int;
    pub fn pt_gather_device(ctx: *mut PtContext, params: *const PtGatherParams, d_positions: *const f64, d_normals: *const f64, background: *const f64,
                            device_out: *const PtGatherBuffers, hip_stream: *mut c_void) -> c_int;
    pub fn pt_gather_finish(ctx: *mut PtContext, kernel_ms: *mut f64) -> c_int;
    // light probes at points in free space: per probe the nine order-2 spherical-harmonic sums (9 x 3 f64) of `samples` (64 .. 1024) shaded samples - what
    // pt_radiance answers - over the whole sphere, the rays made in registers; 24 bytes per probe in, background 3 f64 on the HOST in both forms. A radiance
    // pass for bookkeeping: pt_probe_device is closed by pt_probe_finish, which is pt_radiance_finish
    pub fn pt_probe(ctx: *mut PtContext, params: *const PtProbeParams, positions: *const f64, background: *const f64,
                    host_out: *const PtProbeBuffers, kernel_ms: *mut f64) -> c_int;
    pub fn pt_probe_device(ctx: *mut PtContext, params: *const PtProbeParams, d_positions: *const f64, background: *const f64,
                           device_out: *const PtProbeBuffers, hip_stream: *mut c_void) -> c_int;
    pub fn pt_probe_finish(ctx: *mut PtContext, kernel_ms: *mut f64) -> c_int;
    // direct light at points of the caller's own: per point the sum of colour x max(cos, 0) / attenuation over the resident scene's lights whose shadow ray
    // (made in registers, a fixed sequence of f64 operations, pt_direct.h; `samples` per area light) meets nothing. Shares pt_rays' pass as pt_ao does:
    // pt_direct_device is closed by pt_direct_finish, which is pt_rays_finish; queued behind pt_aov_device / pt_chart_device on the same stream it reads that
    // pass's position and normal where they are
    pub fn pt_direct(ctx: *mut PtContext, params: *const PtDirectParams, positions: *const f64, normals: *const f64, host_out: *const PtDirectBuffers,
                     kernel_ms: *mut f64) -> c_int;
    pub fn pt_direct_device(ctx: *mut PtContext, params: *const PtDirectParams, d_positions: *const f64, d_normals: *const f64, device_out: *const PtDirectBuffers,
                            hip_stream: *mut c_void) -> c_int;
    pub fn pt_direct_finish(ctx: *mut PtContext, kernel_ms: *mut f64) -> c_int;
    // a mesh's light-map texels as surface points (position and normal in world space: what pt_ao and pt_gather take), made on the device from the resident
    // triangle records and matrices by a contract that is checked in every bit (pt_chart.h). uv: T x 6 f64 per triangle corner, T = pt_chart_triangles; null =
    // the mesh's own texture coordinates where a textured scene keeps them. Runs on pt_aov's pass: pt_chart_device is closed by pt_aov_finish, and behind it
    // on the same stream pt_ao_device / pt_gather_device read position and normal where they are
    pub fn pt_chart_triangles(ctx: *mut PtContext, node: u32, n_tris: *mut u64) -> c_int;
    pub fn pt_chart(ctx: *mut PtContext, params: *const PtChartParams, uv: *const f64, host_out: *const PtChartBuffers, kernel_ms: *mut f64) -> c_int;
    pub fn pt_chart_device(ctx: *mut PtContext, params: *const PtChartParams, d_uv: *const f64, device_out: *const PtChartBuffers,
                           hip_stream: *mut c_void) -> c_int;
    // a film: samples accumulate in device memory, add after add; pt_film_add_device is closed by pt_radiance_finish
    pub fn pt_film_create(ctx: *mut PtContext, width: u32, height: u32, out: *mut *mut PtFilm) -> c_int;
    pub fn pt_film_destroy(ctx: *mut PtContext, film: *mut PtFilm) -> c_int;
    pub fn pt_film_reset(ctx: *mut PtContext, film: *mut PtFilm) -> c_int;
    pub fn pt_film_add(ctx: *mut PtContext, film: *mut PtFilm, camera: *const PtCamera, background: *const f64, params: *const PtFilmParams,
                       kernel_ms: *mut f64) -> c_int;
    pub fn pt_film_add_device(ctx: *mut PtContext, film: *mut PtFilm, camera: *const PtCamera, d_background: *const f64, params: *const PtFilmParams,
                              hip_stream: *mut c_void) -> c_int;
    // the same adds behind a lens (depth of field, an orthographic view, a fisheye): only the primary ray differs, by a contract of f64 operations (pt_lens.h);
    // counts, fold, bookkeeping and refusals are pt_film_add's, then a NULL lens, an unknown model, a bad aperture / focus / extent
    pub fn pt_film_add_lens(ctx: *mut PtContext, film: *mut PtFilm, camera: *const PtCamera, lens: *const PtLens, background: *const f64,
                            params: *const PtFilmParams, kernel_ms: *mut f64) -> c_int;
    pub fn pt_film_add_lens_device(ctx: *mut PtContext, film: *mut PtFilm, camera: *const PtCamera, lens: *const PtLens, d_background: *const f64,
                                   params: *const PtFilmParams, hip_stream: *mut c_void) -> c_int;
    pub fn pt_film_resolve(ctx: *mut PtContext, film: *mut PtFilm, rgb: *mut u8, linear: *mut f64) -> c_int;
    pub fn pt_film_resolve_device(ctx: *mut PtContext, film: *mut PtFilm, d_rgb: *mut c_void, d_linear: *mut f64, hip_stream: *mut c_void) -> c_int;
    pub fn pt_film_counts(ctx: *mut PtContext, film: *mut PtFilm, counts: *mut u32) -> c_int;
    // the adaptive film: a film that also keeps a second moment (60 bytes per pixel), an add with a budget per pixel (host or device map), the standard
    // error of every pixel's mean, and the budget a refine pass gives with its two-word summary; pt_film_add_map_device is closed by pt_radiance_finish
    pub fn pt_film_create_moments(ctx: *mut PtContext, width: u32, height: u32, out: *mut *mut PtFilm) -> c_int;
    pub fn pt_film_add_map(ctx: *mut PtContext, film: *mut PtFilm, camera: *const PtCamera, background: *const f64, params: *const PtFilmMapParams,
                           budget: *const u32, kernel_ms: *mut f64) -> c_int;
    pub fn pt_film_add_map_device(ctx: *mut PtContext, film: *mut PtFilm, camera: *const PtCamera, d_background: *const f64, params: *const PtFilmMapParams,
                                  d_budget: *const u32, hip_stream: *mut c_void) -> c_int;
    pub fn pt_film_error(ctx: *mut PtContext, film: *mut PtFilm, err: *mut f64) -> c_int;
    pub fn pt_film_error_device(ctx: *mut PtContext, film: *mut PtFilm, d_err: *mut f64, hip_stream: *mut c_void) -> c_int;
    pub fn pt_film_budget_device(ctx: *mut PtContext, film: *mut PtFilm, params: *const PtFilmRefineParams, d_budget: *mut u32, d_summary: *mut u64,
                                 hip_stream: *mut c_void) -> c_int;
    // the film, denoised: an a-trous filter over the resolved mean, guided by aov buffers and the film's noise estimate; lossy, the film is not written
    pub fn pt_film_denoise(ctx: *mut PtContext, film: *mut PtFilm, params: *const PtDenoiseParams, host_guides: *const PtDenoiseGuides, rgb: *mut u8, linear: *mut f64,
                           variance: *mut f64) -> c_int;
    pub fn pt_film_denoise_device(ctx: *mut PtContext, film: *mut PtFilm, params: *const PtDenoiseParams, d_guides: *const PtDenoiseGuides, d_rgb: *mut c_void,
                                  d_linear: *mut f64, d_variance: *mut f64, hip_stream: *mut c_void) -> c_int;
    // the same filter on demodulated colour: albedo (width x height x 3 f64, as pt_guides writes it) is divided out before the levels and multiplied back after
    pub fn pt_film_denoise_albedo(ctx: *mut PtContext, film: *mut PtFilm, params: *const PtDenoiseParams, host_guides: *const PtDenoiseGuides, albedo: *const f64,
                                  rgb: *mut u8, linear: *mut f64, variance: *mut f64) -> c_int;
    pub fn pt_film_denoise_albedo_device(ctx: *mut PtContext, film: *mut PtFilm, params: *const PtDenoiseParams, d_guides: *const PtDenoiseGuides, d_albedo: *const f64,
                                         d_rgb: *mut c_void, d_linear: *mut f64, d_variance: *mut f64, hip_stream: *mut c_void) -> c_int;
    pub fn pt_context_stream(ctx: *mut PtContext, slot: c_int) -> *mut c_void;
    pub fn pt_context_next_slot(ctx: *const PtContext) -> c_int;
    // one render call over the GPUs of a node (one context per GPU, one RCCL gather)
    pub fn pt_node_create(n_devices: c_int, devices: *const c_int, out: *mut *mut PtNode) -> c_int;
    pub fn pt_node_destroy(node: *mut PtNode);
    pub fn pt_node_last_error(node: *const PtNode) -> *const c_char;
    pub fn pt_node_scene_upload(node: *mut PtNode, scene: *const PtScene, traverse: c_int, kd: *const PtKdTree) -> c_int;
    pub fn pt_node_scene_update(node: *mut PtNode, motion: *const PtSceneMotion, kd: *const PtKdTree) -> c_int;
    pub fn pt_node_render(node: *mut PtNode, camera: *const PtCamera, background: *const f64, params: *const PtRenderParams,
                          rgb: *mut u8, stats: *mut PtStats) -> c_int;
}
