// Device-side build of a mesh's triangle tree: parallel locally-ordered clustering
// (Meister & Bittner 2018) over the Morton-sorted triangles, run by HIP kernels straight from the
// triangle records that are already in HBM and written in the format pt_trace.h walks (PtBvhNode).
//
// Like the host build (pt_bvh.h) it has no counterpart in the reference and cannot change a result:
// FLAT mode's answer is "nearest hit over all candidates, lowest index on ties", whichever tree finds
// the candidates. It exists because the host build is the longest step of a render of a large mesh
// (1.25 M triangles: ~700 ms on the host) and the reference converts the scene inside every render
// call (render.rs:115-126).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_scene_view.h"

struct PtDeviceBuildResult {
    uint32_t root;   // packed reference of the tree's root
    int depth;       // inner nodes on the longest root-to-leaf path (+1): bound for the walk's stack
    float ms;        // device time of the build (HIP events)
    int rounds;      // clustering rounds it took
};

// Builds the tree of triangles [tri_first, tri_first + n) of `d_tri_v` (9 f64 each, model space) into
// d_nodes[node_base ...] (PT_DEVICE_TREE_NODES(n) nodes) and d_items[item_base ...]
// (PT_DEVICE_TREE_ITEMS(n, max_leaf) GLOBAL triangle indices: the triangles in Morton order, then one
// slot of max_leaf per node for the leaves that hold more than one); the caller allocates both.
// `lo` / `hi` = the mesh's bounds (any box containing all vertices); every triangle's box is grown by
// `pad` on all sides before it is rounded outward to f32 (pt_api pads the host build's boxes the same
// way). n > max_leaf required. Returns hipSuccess or the first error.
#define PT_DEVICE_TREE_NODES(n) ((n) - 1u)
#define PT_DEVICE_TREE_ITEMS(n, max_leaf) ((n) + (uint32_t)(max_leaf) * ((n) - 1u))
hipError_t pt_device_build_mesh_tree(const double* d_tri_v, uint32_t tri_first, uint32_t n, const double lo[3], const double hi[3], double pad, int max_leaf,
                                     PtBvhNode* d_nodes, uint32_t node_base, uint32_t* d_items, uint32_t item_base, hipStream_t stream,
                                     PtDeviceBuildResult* out);

// The scene-level tree of pt_scene_update, built on the device by the same clustering over the flattened nodes' world boxes: one thread per
// node first writes its conservative f32 box from the resident `d_fwd` (12 f64 per node), `d_info` (4 words per node: type, data, flags,
// material), `d_mesh_box` (6 f64 per mesh: the padded model box) and `d_tri_v` (stand-alone triangles) with pt_scene_upload's formulas, then
// the boxes are sorted by the Morton codes of their centres inside `lo` / `hi` (the root box) and clustered. Leaves are DIRECT
// (PT_REF_LEAF | node << 3, pt_bvh.h): nothing is written to an items array. Writes exactly n - 1 nodes at d_nodes[node_base ...]; n >= 2.
// Like every tree here it only finds candidates: equal hits are resolved by node index (by dfs_rank in the hierarchical traversal) in the
// walks, never by tree order, so a render does not depend on which builder made the tree. Like the mesh build it reads one word back per clustering round (the clusters left) and `out` at the end; it copies nothing else.
hipError_t pt_device_build_scene_tree(uint32_t n, const double* d_fwd, const uint32_t* d_info, const double* d_mesh_box, const double* d_tri_v,
                                      const double lo[3], const double hi[3], PtBvhNode* d_nodes, uint32_t node_base, hipStream_t stream,
                                      PtDeviceBuildResult* out);

// ---- pt_scene_deform: new vertices under an unchanged topology -------------------------------------------------------------------
// Expand: one thread per triangle t of [0, n_tris) gathers its three vertices through d_indices[3 (tri_first + t) ..] (indices local to the mesh, as
// uploaded; one >= n_verts leaves its triangle untouched) from d_pos (n_verts x 3 f64) and writes record tri_first + t of d_tri_v (a, b, c), of d_tri_e
// (a, a - b, a - c: plain f64 subtractions, the upload's bits) and - when d_nrm and d_tri_n are given - of d_tri_n.
hipError_t pt_device_expand_mesh(const uint32_t* d_indices, uint32_t tri_first, uint32_t n_tris, const double* d_pos, const double* d_nrm, uint32_t n_verts,
                                 double* d_tri_v, double* d_tri_e, double* d_tri_n, hipStream_t stream);

// d_parent[i] for the two-child nodes [node_first, node_first + node_count) of one mesh tree: (parent << 1) | the parent's child slot, PT_TREE_NO_PARENT
// for the root and for entries no node refers to. Entries of the range that the tree does not use must hold PT_REF_EMPTY children (pt_scene_upload and a
// rebuild fill the range with 0xFF bytes before the device builder runs). Depends on the topology alone: computed once per tree, again after a rebuild.
#define PT_TREE_NO_PARENT 0xFFFFFFFFu
hipError_t pt_device_tree_parents(const PtBvhNode* d_nodes, uint32_t node_first, uint32_t node_count, uint32_t* d_parent, hipStream_t stream);

// Refit: the tree keeps its topology, every box is recomputed bottom-up. One thread per node writes the boxes of the node's LEAF children from the
// triangles their references name through d_items (padded by `pad`, rounded outward to f32 like pt_ploc_prepare and the host build), and carries the
// union upward into the parent's lo[axis][slot] / hi[axis][slot]: a node is complete when two arrivals have been counted at it (d_arrive, zeroed by this
// call for the range; a leaf child is an arrival of the node's own thread); the first to arrive exits, the second continues: no thread waits or spins.
// A device-scope fence separates a box store from the counter increment. item / triangle / parent indices outside their ranges are skipped, not followed.
hipError_t pt_device_refit_mesh_tree(PtBvhNode* d_nodes, uint32_t node_first, uint32_t node_count, const uint32_t* d_items, uint32_t item_first,
                                     uint32_t item_count, const double* d_tri_v, uint32_t tri_first, uint32_t tri_count, double pad,
                                     const uint32_t* d_parent, uint32_t* d_arrive, hipStream_t stream);

// ---- pt_vertex_bounds_device / pt_scene_deform_device: the box of vertices that are already in device memory -------------------------------
// One pass over d_pos (n_verts x 3 f64, 8-byte aligned) read as a flat array, so that a wavefront's 64 lanes load 64 consecutive doubles: a block of
// PT_VBOX_BLOCK threads takes PT_VBOX_BLOCK whole vertices per step (three loads per thread, one coordinate of each axis), the grid strides over those
// steps. Every minimum / maximum is carried as (value, lowest vertex index attaining it) through the lanes of a wavefront (registers), the block's
// wavefronts (LDS) and the blocks (one PtVboxPartial per block, plain stores, folded by a one-block launch of the same reduction): the six doubles carry
// the bits pt_mesh_vertex_box's loop leaves - it keeps the first extreme it meets, which matters where the extreme is a zero that occurs with both signs.
// NaN and +-inf coordinates take no part and are counted. n_verts = 0 or nothing finite: the empty box (lo = +inf, hi = -inf). No atomics.
// The grid is min(steps, PT_VBOX_BLOCKS_PER_CU * n_cu) blocks; d_partials holds pt_vertex_box_partials(n_cu) records. Queued on `stream`: the result is at
// d_partials[0] when the stream has drained.
#define PT_VBOX_BLOCK 256
#define PT_VBOX_BLOCKS_PER_CU 4
struct PtVboxPartial {
    double v[6];        // lo xyz, hi xyz
    uint32_t at[6];     // the lowest vertex index attaining each (0xFFFFFFFF: none)
    uint64_t non_finite;
};
inline uint32_t pt_vertex_box_partials(int n_cu) { return (uint32_t)PT_VBOX_BLOCKS_PER_CU * (uint32_t)(n_cu > 0 ? n_cu : 1); }
hipError_t pt_device_vertex_box(const double* d_pos, uint64_t n_verts, int n_cu, PtVboxPartial* d_partials, hipStream_t stream);
