// The scene behind the C ABI (include/portrayer_hip.h): pt_scene_upload (prepare, then commit: checks, host computation and tree builds, then the writes),
// pt_scene_update, pt_scene_deform / pt_scene_deform_device, and the two small kernels that derive what the walks read from the trees. The context's life
// cycle, the render and the passes are in pt_api.hip.
#include "pt_context.h"

// Two-child tree -> four-child tree (PtBvh4Node, pt_scene_view.h). Node i starts with its two children and, while it has
// fewer than four, replaces the inner child with the largest surface area by that child's two children (the child a ray is
// most likely to enter is the one worth opening; taking over both children's children regardless leaves a node with a leaf
// child at three entries). Mesh trees only: on scene-level trees the grandchildren form measured better (transmission-refraction
// 3.32 against 3.72 node visits per ray). PORTRAYER_COLLAPSE=plain | mesh | area.
// One thread per two-child node; entries of the array that no tree uses (the device build reserves n - 1 nodes per mesh
// and may need fewer) are never referenced and are only kept from reading out of bounds. In a device-built tree's place they
// hold 0xFF bytes, i.e. PT_REF_EMPTY children: pt_scene_upload and a rebuild by pt_scene_deform fill the place before the
// builder runs, and pt_parent_kernel / pt_refit_kernel (pt_build.hip), which scan the whole place, rely on that - the memset is not redundant.
// tri_leaf: the edge record of every triangle named by a slot of the items array, in slot order (80 bytes a slot: 9 f64 + the triangle's index), so
// that a mesh leaf's triangles lie side by side and the wave-uniform walks fetch them without going through bvh_items first.
__global__ void __launch_bounds__(256) pt_tri_leaf_kernel(const uint32_t* __restrict__ items, uint32_t n_items, const double* __restrict__ tri_e, uint32_t n_tris,
                                                         double* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const uint32_t t = items[i];
    double* o = out + 10 * (size_t)i;
    if (t < n_tris) {
        const double* e = tri_e + 9 * (size_t)t;
        for (int k = 0; k < 9; k++) o[k] = e[k];
    } else {
        for (int k = 0; k < 9; k++) o[k] = 0.0;
    }
    union { double d; uint32_t u[2]; } c; c.u[0] = t; c.u[1] = 0u;
    o[9] = c.d;
}

// [first, end): the nodes this launch converts (pt_scene_upload: all n of them; pt_scene_update: the scene-level tree's alone).
__global__ void __launch_bounds__(256) pt_collapse4_kernel(const PtBvhNode* __restrict__ bvh2, PtBvh4Node* __restrict__ bvh4, uint32_t n, int by_area_mode,
                                                            uint32_t scene_first, uint32_t scene_end, uint32_t first, uint32_t end) {
    const uint32_t i = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= end || i >= n) return;
    // by_area_mode 0: never, 1: mesh trees only (nodes outside [scene_first, scene_end)), 2: every tree
    const bool by_area = by_area_mode == 2 || (by_area_mode == 1 && (i < scene_first || i >= scene_end));
    const PtBvhNode a = bvh2[i];
    float lo[4][3], hi[4][3];
    uint32_t child[4];
    int k = 0;
    auto put = [&](const PtBvhNode& nd, int which) {
        pt_node_get_box(nd, which, lo[k], hi[k]);
        child[k] = which ? nd.child1 : nd.child0;
        k++;
    };
    auto inner = [&](uint32_t c) { return c != PT_REF_EMPTY && !(c & PT_REF_LEAF) && c < n; };
    if (by_area) {
        if (a.child0 != PT_REF_EMPTY) put(a, 0);
        if (a.child1 != PT_REF_EMPTY) put(a, 1);
        while (k < 4) {
            int best = -1;
            float best_area = -1.0f;
            for (int j = 0; j < k; j++) {
                if (!inner(child[j])) continue;
                const float dx = hi[j][0] - lo[j][0], dy = hi[j][1] - lo[j][1], dz = hi[j][2] - lo[j][2];
                const float area = dx * dy + dy * dz + dz * dx;
                if (!(area <= best_area)) { best = j; best_area = area; }  // also takes a NaN / infinite area rather than nothing
            }
            if (best < 0) break;
            const PtBvhNode c = bvh2[child[best]];
            const int n_kids = (c.child0 != PT_REF_EMPTY) + (c.child1 != PT_REF_EMPTY);
            if (n_kids == 0) { child[best] = child[k - 1]; for (int ax = 0; ax < 3; ax++) { lo[best][ax] = lo[k - 1][ax]; hi[best][ax] = hi[k - 1][ax]; } k--; continue; }
            // the first child takes the opened entry's place, the second goes to the end
            const int first = c.child0 != PT_REF_EMPTY ? 0 : 1;
            pt_node_get_box(c, first, lo[best], hi[best]);
            child[best] = first ? c.child1 : c.child0;
            if (n_kids == 2) put(c, 1);
        }
    } else {
        auto expand = [&](const PtBvhNode& nd, int which) {
            const uint32_t c0 = which ? nd.child1 : nd.child0;
            if (c0 == PT_REF_EMPTY) return;
            if (!inner(c0)) { put(nd, which); return; }
            const PtBvhNode c = bvh2[c0];
            if (c.child0 != PT_REF_EMPTY) put(c, 0);
            if (c.child1 != PT_REF_EMPTY) put(c, 1);
        };
        expand(a, 0);
        expand(a, 1);
    }
    PtBvh4Node o;
    for (int j = 0; j < 4; j++) {
        const bool used = j < k;
        for (int ax = 0; ax < 3; ax++) { o.lo[ax][j] = used ? lo[j][ax] : (float)PT_BOX_LIMIT; o.hi[ax][j] = used ? hi[j][ax] : -(float)PT_BOX_LIMIT; }
        o.child[j] = used ? child[j] : PT_REF_EMPTY;
    }
    o.pad[0] = o.pad[1] = o.pad[2] = o.pad[3] = 0u;
    bvh4[i] = o;
}

// ------------------------------------------------------------------------------------------------
// Scene upload
// ------------------------------------------------------------------------------------------------
static void pt_transform_box(const double* m, const double lo[3], const double hi[3], PtBuildBox* out) {
    *out = pt_bvh_detail::empty_box();
    for (int ix = 0; ix < 2; ix++) for (int iy = 0; iy < 2; iy++) for (int iz = 0; iz < 2; iz++) {
        double x = ix ? hi[0] : lo[0], y = iy ? hi[1] : lo[1], z = iz ? hi[2] : lo[2];
        for (int r = 0; r < 3; r++) {
            double v = m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + m[4 * r + 3];
            out->lo[r] = std::min(out->lo[r], v);
            out->hi[r] = std::max(out->hi[r], v);
        }
    }
}
static void pt_pad_box(PtBuildBox* b, double rel) {
    for (int k = 0; k < 3; k++) {
        double mag = std::max(std::fabs(b->lo[k]), std::fabs(b->hi[k]));
        double pad = rel * std::max(b->hi[k] - b->lo[k], mag) + 1e-300;
        b->lo[k] -= pad; b->hi[k] += pad;
    }
}

// ------------------------------------------------------------------------------------------------
// Steps of pt_scene_upload that pt_scene_update repeats for a moved scene: both call these, so a host-computed part of an updated
// scene is what an upload of the same scene computes.
// ------------------------------------------------------------------------------------------------
static void pt_pack_node_matrices(uint32_t n, const double* trans, const double* invtrans, const double* normal_trans, std::vector<double>& inv,
                                  std::vector<double>& fwd, std::vector<double>& nrm) {
    inv.resize(12 * (size_t)n); fwd.resize(12 * (size_t)n); nrm.resize(9 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        for (int r = 0; r < 12; r++) { inv[12 * (size_t)i + r] = invtrans[16 * (size_t)i + r]; fwd[12 * (size_t)i + r] = trans[16 * (size_t)i + r]; }
        for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) nrm[9 * (size_t)i + 3 * r + k] = normal_trans[16 * (size_t)i + 4 * r + k];
    }
}

struct PtGraphArrays {
    std::vector<double> g_inv, g_fwd, g_nrm, own_inv;
    std::vector<uint32_t> hier_rec;
};
// PT_TRAVERSE_HIER: the graph nodes' matrices and, per flattened node, its path record and its own level's inverse. chain_off / chain are checked by the caller.
static void pt_pack_graph(uint32_t n, uint32_t g, const double* graph_trans, const double* graph_invtrans, const double* graph_normal_trans,
                          const std::vector<uint32_t>& chain_off, const std::vector<uint32_t>& chain, PtGraphArrays& out) {
    std::vector<double>&g_inv = out.g_inv, &g_fwd = out.g_fwd, &g_nrm = out.g_nrm, &own_inv = out.own_inv;
    std::vector<uint32_t>& hier_rec = out.hier_rec;
    g_inv.resize(12 * (size_t)g); g_fwd.resize(12 * (size_t)g); g_nrm.resize(9 * (size_t)g);
    for (uint32_t i = 0; i < g; i++) {
        for (int r = 0; r < 12; r++) { g_inv[12 * (size_t)i + r] = graph_invtrans[16 * (size_t)i + r]; g_fwd[12 * (size_t)i + r] = graph_trans[16 * (size_t)i + r]; }
        for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) g_nrm[9 * (size_t)i + 3 * r + k] = graph_normal_trans[16 * (size_t)i + 4 * r + k];
    }
    // One record per flattened node for the walks (pt_node_local_ray_uniform): its path in one scalar fetch instead of three dependent
    // ones, and which of its levels are the identity (a group without a transform, like every reference scene's root): multiplying a
    // ray by such a level changes no bit unless a component is -0 or not finite, which the walk rules out once per ray.
    auto identity = [&](uint32_t gi) {
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 4; k++) {
                const double want = r == k ? 1.0 : 0.0;  // (== : a zero of either sign passes)
                if (g_inv[12 * (size_t)gi + 4 * r + k] != want || g_fwd[12 * (size_t)gi + 4 * r + k] != want) return false;
                if (k < 3 && g_nrm[9 * (size_t)gi + 3 * r + k] != want) return false;
            }
        return true;
    };
    std::vector<uint8_t> g_ident(g);
    for (uint32_t i = 0; i < g; i++) g_ident[i] = identity(i) ? 1 : 0;
    hier_rec.assign(8 * (size_t)n, 0u);
    own_inv.assign(12 * (size_t)n, 0.0);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t len = chain_off[i + 1] - chain_off[i];
        uint32_t* rec = &hier_rec[8 * (size_t)i];
        for (int r = 0; r < 12; r++) own_inv[12 * (size_t)i + r] = g_inv[12 * (size_t)chain[chain_off[i + 1] - 1] + r];  // the node's own level: the last of its path
        if (len > 7) { rec[0] = 255u; continue; }
        rec[0] = len;
        for (uint32_t k = 0; k < len; k++) {
            const uint32_t gi = chain[chain_off[i] + k];
            rec[1 + k] = gi;
            if (g_ident[gi]) rec[0] |= 1u << (8 + k);
        }
    }
}

// The box of a mesh's vertices and its largest extent (floored at 1e-30): triangle boxes are padded by 1e-7 ext, the mesh's own box by 1e-5 ext.
// pt_scene_upload and pt_scene_deform both call this.
static double pt_box_extent(const PtBuildBox& b) { return std::max(std::max(b.hi[0] - b.lo[0], b.hi[1] - b.lo[1]), std::max(b.hi[2] - b.lo[2], 1e-30)); }
static double pt_mesh_vertex_box(const double* pos, uint64_t n_verts, PtBuildBox* mb) {
    *mb = pt_bvh_detail::empty_box();
    for (uint64_t v = 0; v < n_verts; v++)
        for (int k = 0; k < 3; k++) { mb->lo[k] = std::min(mb->lo[k], pos[3 * v + k]); mb->hi[k] = std::max(mb->hi[k], pos[3 * v + k]); }
    return pt_box_extent(*mb);
}
// ... the two paddings, `ext` being the extent of the mesh's vertex box
static double pt_triangle_pad(double ext) { return 1e-7 * ext; }
static void pt_pad_mesh_box(PtBuildBox* mb, double ext) {
    for (int k = 0; k < 3; k++) { mb->lo[k] -= 1e-5 * ext; mb->hi[k] += 1e-5 * ext; }
}

// Where a tree is built: on the host (binned SAH, pt_bvh.h: the better tree) or on the
// device (Morton-order tree, pt_build.h: ~100x faster to build). PORTRAYER_BUILD = host | device | auto;
// auto takes the device for trees over PORTRAYER_BUILD_MIN (default 65536) leaves or more, device from 16 on.
struct PtBuildPolicy {
    int mode = 2;
    size_t device_min = 65536;
    bool on_device(size_t leaves) const { return (mode == 1 && leaves >= 16) || (mode == 2 && leaves >= device_min); }
};
static PtBuildPolicy pt_build_policy() {
    PtBuildPolicy p;
    if (const char* e = getenv("PORTRAYER_BUILD")) p.mode = !strcmp(e, "host") ? 0 : (!strcmp(e, "device") ? 1 : 2);
    if (const char* e = getenv("PORTRAYER_BUILD_MIN")) p.device_min = (size_t)std::max(16, atoi(e));
    return p;
}

// the padded model box of a stand-alone triangle (9 f64)
static void pt_triangle_model_box(const double* v, PtBuildBox* b) {
    double ext = 1e-30;
    for (int k = 0; k < 3; k++) {
        b->lo[k] = std::min(v[k], std::min(v[3 + k], v[6 + k])); b->hi[k] = std::max(v[k], std::max(v[3 + k], v[6 + k]));
        ext = std::max(ext, b->hi[k] - b->lo[k]);
    }
    for (int k = 0; k < 3; k++) { b->lo[k] -= 1e-6 * ext; b->hi[k] += 1e-6 * ext; }
}

// Conservative world-space boxes of the flattened nodes and their union, the scene tree's root box (c->root_lo / root_hi): every hit the
// primitive tests can accept lies inside its box (cube.rs:25 / plane.rs:31 accept points up to 1e-5 outside the unit shape; all shapes are
// padded by 1e-4 model units). Spheres, cylinders and cones get their exact boxes under the affine transform instead of the box of their
// transformed unit cube. `info`: 4 words per node (type, data, ..); pt_node_box_kernel (pt_build.hip) is the device's copy of the formulas.
static void pt_node_world_boxes(uint32_t n, const double* trans, const uint32_t* info, const std::vector<PtBuildBox>& mesh_box,
                                const std::vector<PtBuildBox>& tri_box, size_t mesh_tris, std::vector<PtBuildBox>& node_box, double root_lo[3], double root_hi[3]) {
    node_box.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        const int t = (int)info[4 * (size_t)i];
        const uint32_t data = info[4 * (size_t)i + 1];
        const double* M = &trans[16 * (size_t)i];
        PtBuildBox& nb = node_box[i];
        auto disc = [&](double yc, double radius, PtBuildBox* b) {  // disc of `radius` in the model xz-plane at height yc
            for (int r = 0; r < 3; r++) {
                double c = M[4 * r + 1] * yc + M[4 * r + 3];
                double e = radius * std::sqrt(M[4 * r] * M[4 * r] + M[4 * r + 2] * M[4 * r + 2]);
                b->lo[r] = std::min(b->lo[r], c - e); b->hi[r] = std::max(b->hi[r], c + e);
            }
        };
        double lo[3], hi[3];
        bool boxed = false;
        switch (t) {
        case PT_PRIM_SPHERE:
            for (int r = 0; r < 3; r++) {
                double e = 1.0001 * std::sqrt(M[4 * r] * M[4 * r] + M[4 * r + 1] * M[4 * r + 1] + M[4 * r + 2] * M[4 * r + 2]);
                nb.lo[r] = M[4 * r + 3] - e; nb.hi[r] = M[4 * r + 3] + e;
            }
            boxed = true; break;
        case PT_PRIM_CYLINDER: nb = pt_bvh_detail::empty_box(); disc(0.5001, 0.5001, &nb); disc(-0.5001, 0.5001, &nb); boxed = true; break;
        case PT_PRIM_CONE: nb = pt_bvh_detail::empty_box(); disc(0.5001, 1e-4, &nb); disc(-0.5001, 0.5001, &nb); boxed = true; break;
        case PT_PRIM_PLANE: lo[0] = lo[2] = -0.5001; hi[0] = hi[2] = 0.5001; lo[1] = -1e-4; hi[1] = 1e-4; break;
        case PT_PRIM_MESH: case PT_PRIM_KDMESH: for (int k = 0; k < 3; k++) { lo[k] = mesh_box[data].lo[k]; hi[k] = mesh_box[data].hi[k]; } break;
        case PT_PRIM_TRIANGLE: for (int k = 0; k < 3; k++) { lo[k] = tri_box[data - mesh_tris].lo[k]; hi[k] = tri_box[data - mesh_tris].hi[k]; } break;
        default: lo[0] = lo[1] = lo[2] = -0.5001; hi[0] = hi[1] = hi[2] = 0.5001; break;  // cube
        }
        if (!boxed) pt_transform_box(M, lo, hi, &nb);
        pt_pad_box(&nb, 1e-9);
    }
    for (int k = 0; k < 3; k++) { root_lo[k] = INFINITY; root_hi[k] = -INFINITY; }
    for (uint32_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) { root_lo[k] = std::min(root_lo[k], node_box[i].lo[k]); root_hi[k] = std::max(root_hi[k], node_box[i].hi[k]); }
}

// The scene-level tree on the host: binned SAH over the nodes' world boxes (pt_bvh.h), built from index 0 and then moved to where it lives in the
// context's arrays: its nodes from `node_base` on in bvh, its leaf items (none when the leaves are direct) from `item_base` on in bvh_items.
static PtBvhRef pt_build_scene_tree(const std::vector<PtBuildBox>& node_box, int tlas_leaf, bool direct, size_t node_base, size_t item_base,
                                    std::vector<PtBvhNode>& nodes, std::vector<uint32_t>& items) {
    nodes.clear(); items.clear();
    PtBvhRef root = pt_bvh_build(node_box.data(), nullptr, node_box.size(), tlas_leaf, nodes, items, direct);
    auto moved = [&](uint32_t ref) -> uint32_t {
        if (ref == PT_REF_EMPTY) return ref;
        if (!(ref & PT_REF_LEAF)) return ref + (uint32_t)node_base;
        if (direct) return ref;
        return PT_REF_LEAF | (((((ref & ~PT_REF_LEAF) >> 3) + (uint32_t)item_base) << 3) | (ref & 7u));
    };
    for (PtBvhNode& nd : nodes) { nd.child0 = moved(nd.child0); nd.child1 = moved(nd.child1); }
    root.child = moved(root.child);
    return root;
}

// The reference's k-d tree over the flattened nodes (PT_TRAVERSE_KD) as the walks read it, with the conservative f32 boxes the culls use.
struct PtKdArrays {
    std::vector<PtKdNode> kdn;
    std::vector<uint32_t> kdi, kd_ref32;
    std::vector<float> node_box32, kd_box32;
    double kd_extent = 0.0;
    int kd_depth = 0, kd_levels = 0;
};
static int pt_pack_kd(pt_context* c, const pt_kdtree* kd, uint32_t n, const std::vector<PtBuildBox>& node_box, PtKdArrays& out) {
    std::vector<PtKdNode>& kdn = out.kdn;
    std::vector<uint32_t>&kdi = out.kdi, &kd_ref32 = out.kd_ref32;
    std::vector<float>&node_box32 = out.node_box32, &kd_box32 = out.kd_box32;
    int& kd_levels = out.kd_levels;  // split levels on the deepest path of the tree (root = level 0)
    if (kd->n_nodes == 0 || !kd->axis || !kd->plane || !kd->front || !kd->back || !kd->first || !kd->count || (kd->n_items && !kd->leaf_items))
        return pt_fail(c, PT_ERR_ARGUMENT, "incomplete k-d tree");
    kdn.resize(kd->n_nodes);
    for (uint32_t i = 0; i < kd->n_nodes; i++) {
        PtKdNode& k = kdn[i];
        k.axis = kd->axis[i]; k.plane = kd->plane[i]; k.front = kd->front[i]; k.back = kd->back[i];
        k.first = kd->first[i]; k.count = kd->count[i]; k.pad = 0; k.pad2[0] = k.pad2[1] = 0.0f; for (int r = 0; r < 6; r++) k.box[r] = 0.0f;
        if (k.axis >= 0) {
            if (k.axis > 2 || k.front < 0 || k.back < 0 || (uint32_t)k.front >= kd->n_nodes || (uint32_t)k.back >= kd->n_nodes)
                return pt_fail(c, PT_ERR_ARGUMENT, "k-d child out of range");
        } else if (k.first < 0 || k.count < 0 || (uint32_t)(k.first + k.count) > kd->n_items) {
            return pt_fail(c, PT_ERR_ARGUMENT, "k-d leaf range out of bounds");
        }
    }
    kdi.resize(kd->n_items);
    for (uint32_t i = 0; i < kd->n_items; i++) {
        if (kd->leaf_items[i] < 0 || (uint32_t)kd->leaf_items[i] >= n) return pt_fail(c, PT_ERR_ARGUMENT, "k-d leaf item out of range");
        kdi[i] = (uint32_t)kd->leaf_items[i];
    }
    double dx = kd->root_max[0] - kd->root_min[0], dy = kd->root_max[1] - kd->root_min[1], dz = kd->root_max[2] - kd->root_min[2];
    out.kd_extent = (dx * dx + dy * dy) + dz * dz;  // bounding_box.rs:95-99 magnitude_squared
    out.kd_depth = kd->max_depth < 0 ? 0 : kd->max_depth;
    node_box32.resize(6 * kdi.size());  // in leaf-item order: the walk reads a leaf's boxes one after the other
    for (size_t j = 0; j < kdi.size(); j++)
        for (int k = 0; k < 3; k++) {
            node_box32[6 * j + k] = pt_bvh_detail::round_down(node_box[kdi[j]].lo[k]);
            node_box32[6 * j + 3 + k] = pt_bvh_detail::round_up(node_box[kdi[j]].hi[k]);
        }
    // the wave-uniform k-d walk (pt_trace_packet_kd) reads a leaf reference and its cull box in ONE scalar fetch: 32 bytes {node, 0, box}
    kd_ref32.resize(8 * kdi.size());
    for (size_t j = 0; j < kdi.size(); j++) {
        kd_ref32[8 * j] = kdi[j]; kd_ref32[8 * j + 1] = 0u;
        memcpy(&kd_ref32[8 * j + 2], &node_box32[6 * j], 6 * sizeof(float));
    }
    {
        std::vector<std::pair<uint32_t, int>> todo;
        std::vector<uint8_t> seen(kdn.size(), 0);
        if (!kdn.empty()) todo.push_back({0u, 0});
        while (!todo.empty()) {
            auto [i, lev] = todo.back(); todo.pop_back();
            if (seen[i]) return pt_fail(c, PT_ERR_ARGUMENT, "k-d tree is not a tree");
            seen[i] = 1;
            if (kdn[i].axis < 0) continue;
            kd_levels = std::max(kd_levels, lev + 1);
            todo.push_back({(uint32_t)kdn[i].front, lev + 1}); todo.push_back({(uint32_t)kdn[i].back, lev + 1});
        }
    }
    if (kd_levels > PT_KD_WAVE_LEVELS)  // two bits of per-lane state per level in one 64-bit word (pt_trace_packet_kd); a tree that deep has > 2^32 leaves unless it is a degenerate chain
        return pt_fail(c, PT_ERR_SCENE, "k-d tree deeper than 32 levels (the limit of the k-d walk: include/portrayer_hip.h, pt_kdtree)");
    // what the walk's packed words can address: a stack entry is (node << 5) | level, a node is fetched at byte offset node << 6, a leaf reference at (first + i) << 5
    if (kdn.size() >= ((size_t)1 << 26)) return pt_fail(c, PT_ERR_SCENE, "k-d tree of 2^26 nodes or more");
    if (kd_ref32.size() / 8 >= ((size_t)1 << 27)) return pt_fail(c, PT_ERR_SCENE, "k-d tree with 2^27 leaf references or more");
    // children follow their parents in the linearised tree (pre-order): one backward sweep
    kd_box32.assign(6 * kdn.size(), 0.0f);
    for (size_t i = kdn.size(); i-- > 0;) {
        float* b = &kd_box32[6 * i];
        const PtKdNode& k = kdn[i];
        for (int r = 0; r < 3; r++) { b[r] = (float)PT_BOX_LIMIT; b[3 + r] = -(float)PT_BOX_LIMIT; }  // empty
        if (k.axis < 0) {
            for (int32_t j = 0; j < k.count; j++)
                for (int r = 0; r < 3; r++) {
                    b[r] = std::min(b[r], node_box32[6 * (size_t)(k.first + j) + r]);
                    b[3 + r] = std::max(b[3 + r], node_box32[6 * (size_t)(k.first + j) + 3 + r]);
                }
        } else if ((size_t)k.front > i && (size_t)k.back > i) {
            for (int r = 0; r < 3; r++) {
                b[r] = std::min(kd_box32[6 * (size_t)k.front + r], kd_box32[6 * (size_t)k.back + r]);
                b[3 + r] = std::max(kd_box32[6 * (size_t)k.front + 3 + r], kd_box32[6 * (size_t)k.back + 3 + r]);
            }
        } else {  // not in pre-order: no culling at this node
            for (int r = 0; r < 3; r++) { b[r] = -(float)PT_BOX_LIMIT; b[3 + r] = (float)PT_BOX_LIMIT; }
        }
    }
    for (size_t i = 0; i < kdn.size(); i++) for (int r = 0; r < 6; r++) kdn[i].box[r] = kd_box32[6 * i + r];
    return PT_OK;
}
// ... into the context's buffers and the view (k.kdn empty: another traversal)
static int pt_upload_kd(pt_context* c, const PtKdArrays& k, bool kd_mode) {
    int rc;
    if ((rc = pt_upload(c, c->node_box, k.node_box32)) || (rc = pt_upload(c, c->kd_box, k.kd_box32)) || (rc = pt_upload(c, c->kd, k.kdn)) ||
        (rc = pt_upload(c, c->kd_items, k.kdi)) || (rc = pt_upload(c, c->kd_ref, k.kd_ref32)))
        return rc;
    PtSceneView& v = c->view;
    v.kd = (const PtKdNode*)c->kd.p; v.kd_items = (const uint32_t*)c->kd_items.p;
    v.kd_extent = k.kd_extent;
    v.kd_ref = (const uint32_t*)c->kd_ref.p; v.kd_levels = k.kd_levels;
    v.node_box = kd_mode && !k.kdi.empty() ? (const float*)c->node_box.p : nullptr;
    v.kd_box = kd_mode ? (const float*)c->kd_box.p : nullptr;
    if (getenv("PORTRAYER_KD_NO_CULL")) v.kd_box = v.node_box = nullptr;  // experiment: the reference's walk as it is
    if (const char* e = getenv("PORTRAYER_KD_CULL")) { const int m = atoi(e); if (!(m & 1)) v.kd_box = nullptr; if (!(m & 2)) v.node_box = nullptr; }  // experiment: bit 0 tree nodes, bit 1 leaf references
    return PT_OK;
}

// the fields of the traits that the lights decide (pt_scene_upload; pt_scene_update with new lights)
static void pt_set_light_traits(PtSceneTraits& t, const double* lights, uint32_t n_lights) {
    t.n_lights = n_lights;
    t.area_light = 0;
    for (uint32_t l = 0; l < n_lights; l++) {
        const double* L = &lights[15 * (size_t)l];
        const bool empty = (L[9] == 0.0 && L[10] == 0.0 && L[11] == 0.0) || (L[12] == 0.0 && L[13] == 0.0 && L[14] == 0.0);  // light.rs:51-53
        if (!empty) t.area_light = 1;
    }
}

// The walks' stack: a level of the four-child walk pushes up to three pending children; it covers two levels of the two-child tree in the plain
// collapse and at least one when nodes are opened by area. `tlas_depth`: of the scene-level tree (two-child form); `kd_depth`: of the k-d tree
// the scene is walked with NOW (PT_TRAVERSE_KD; it changes when nodes move).
static int pt_wide_depth(int collapse_mode, int depth2) { return collapse_mode ? 3 * depth2 : 3 * ((depth2 + 1) / 2); }
// deepest walk under a scene leaf: a mesh tree (as deep as the trees are NOW: a rebuild may have changed one) or a KDMesh tree
static int pt_stack_below(const pt_context::Resident& res) {
    int max_blas_depth = 0;
    for (const auto& pl : res.place) max_blas_depth = std::max(max_blas_depth, pl.depth);
    return std::max(pt_wide_depth(res.collapse_mode, max_blas_depth), 3 * (res.max_kdm_depth + 1));
}
static int pt_set_stack_cap(pt_context* c, int tlas_depth, int kd_depth) {
    int cap = c->res.traverse == PT_TRAVERSE_KD ? 3 * (kd_depth + 1) + c->res.below + 2 : pt_wide_depth(c->res.collapse_mode, tlas_depth) + c->res.below + 4;
    c->view.stack_cap = std::max(cap, 8);
    if (const char* e = getenv("PORTRAYER_STACK_CAP")) c->view.stack_cap = std::max(1, atoi(e));  // tests: force PT_ERR_TRAVERSAL
    if (c->view.stack_cap > 4096) return pt_fail(c, PT_ERR_SCENE, "tree too deep for the traversal stack");
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// Device steps the upload, an update and a deform share: what they read of the scene is the context's (c->res, the buffers), the context's device is current,
// and what they launch goes to the null stream.
// ------------------------------------------------------------------------------------------------
// the per-mesh padded boxes again, 6 f64 each, for the device build of the scene-level tree
static int pt_upload_mesh_boxes(pt_context* c, const std::vector<PtBuildBox>& mesh_box) {
    std::vector<double> mb(6 * mesh_box.size());
    for (size_t m = 0; m < mesh_box.size(); m++) for (int k = 0; k < 3; k++) { mb[6 * m + k] = mesh_box[m].lo[k]; mb[6 * m + 3 + k] = mesh_box[m].hi[k]; }
    return pt_upload(c, c->mesh_box_dev, mb);
}
// the four-child form the walks read, for the nodes [first, end) of bvh alone
static int pt_queue_collapse4(pt_context* c, size_t first, size_t end) {
    const pt_context::Resident& res = c->res;
    if (end <= first) return PT_OK;
    hipLaunchKernelGGL(pt_collapse4_kernel, dim3((unsigned)((end - first + 255) / 256)), dim3(256), 0, nullptr, (const PtBvhNode*)c->bvh.p, (PtBvh4Node*)c->bvh4.p,
                       (uint32_t)res.tree_nodes, res.collapse_mode, (uint32_t)res.tlas_first, (uint32_t)(res.tlas_first + res.tlas_cap), (uint32_t)first, (uint32_t)end);
    PT_HIP(c, hipGetLastError());
    return PT_OK;
}
// the triangle records in leaf order, for the slots [item_first, item_first + item_count) of bvh_items alone
static int pt_queue_tri_leaf(pt_context* c, size_t item_first, size_t item_count) {
    if (!item_count) return PT_OK;
    hipLaunchKernelGGL(pt_tri_leaf_kernel, dim3((unsigned)((item_count + 255) / 256)), dim3(256), 0, nullptr, (const uint32_t*)c->bvh_items.p + item_first, (uint32_t)item_count,
                       (const double*)c->tri_e.p, (uint32_t)(c->res.mesh_tris + c->res.tri_box.size()), (double*)c->tri_leaf.p + 10 * item_first);
    PT_HIP(c, hipGetLastError());
    return PT_OK;
}
// A mesh's tree built by the device in its place (worst-case size, `pl`), over the triangle records resident in tri_v; lo / hi: the mesh's vertex box. Entries
// of the place that the tree will not use name no children (pt_device_tree_parents reads the whole range): hence the fill.
static int pt_build_mesh_tree_in_place(pt_context* c, pt_context::Resident::MeshPlace& pl, PtMeshInfo& mi, const double lo[3], const double hi[3], double pad, PtDeviceBuildResult* built) {
    PT_HIP(c, hipMemsetAsync((PtBvhNode*)c->bvh.p + pl.node_first, 0xFF, (size_t)pl.node_count * sizeof(PtBvhNode), nullptr));
    PT_HIP(c, pt_device_build_mesh_tree((const double*)c->tri_v.p, mi.tri_first, mi.tri_count, lo, hi, pad, c->res.blas_leaf, (PtBvhNode*)c->bvh.p, pl.node_first,
                                        (uint32_t*)c->bvh_items.p, pl.item_first, nullptr, built));
    mi.blas_root = built->root; pl.depth = built->depth; pl.parents_valid = false;
    return PT_OK;
}

// ------------------------------------------------------------------------------------------------
// pt_scene_upload = pt_upload_prepare, then pt_upload_commit: what the host checks and computes before the first HIP call, and what is then written.
// ------------------------------------------------------------------------------------------------
struct PtUploadPlan {
    const pt_scene* s = nullptr;
    bool verbose = false;
    std::chrono::steady_clock::time_point t_lap;
    void lap(const char* what) {
        if (!verbose) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[pt_scene_upload] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_lap).count());
        t_lap = now;
    }
    // triangles: every mesh expanded to 72-byte vertex records, stand-alone triangles appended; their edge form (pt_triangle_hit_e): corner a, a - b, a - c
    size_t mesh_tris = 0, total_tris = 0;
    std::vector<double> tri_v, tri_e, tri_n;
    // the host-built trees (mesh trees, then the scene-level tree in its place of n - 1 nodes) and the meshes the device builds after the triangles are in HBM
    std::vector<PtBvhNode> bvh;
    std::vector<uint32_t> items;
    struct DeviceMesh { uint32_t m; double lo[3], hi[3], pad; };
    std::vector<DeviceMesh> device_meshes;
    size_t tree_nodes = 0, tree_items = 0;  // in bvh / bvh_items altogether, the device-built trees' places included
    // KDMesh trees (reference structure) with conservative f32 bounds per tree node / per leaf reference (pt_kdmesh_hit's culls)
    std::vector<PtKdNode> mkd;
    std::vector<uint32_t> mkd_items;
    std::vector<float> mkd_box, mkd_item_box;
    // nodes
    std::vector<double> inv, fwd, nrm;
    PtGraphArrays graph;
    std::vector<uint32_t> dfs_rank;
    std::vector<PtBuildBox> node_box;
    double root_lo[3], root_hi[3];
    PtBvhRef tlas;
    bool tlas_direct = false;
    PtKdArrays kda;
    std::vector<double> mats, lights;
    PtSceneTraits traits = {};
    // textures / normal maps (texture.rs)
    bool textured = false;
    std::vector<int32_t> mat_maps;
    std::vector<double> uv_trans, srgb_lut, tri_uv;
    std::vector<PtTexInfo> texinfo;
    std::vector<uint8_t> tex_rgb;
    pt_context::Resident res;  // what the context keeps of the scene on the host (info, boxes, places, PtMeshInfo records ..)
};

static int pt_upload_check_nodes(pt_context* c, const pt_scene* s, bool* any_normals) {
    for (uint32_t i = 0; i < s->n_nodes; i++) {
        int t = s->prim_type[i];
        if (t < PT_PRIM_SPHERE || t > PT_PRIM_CONE) return pt_fail(c, PT_ERR_ARGUMENT, "unknown primitive type");
        if (s->material[i] < 0 || (uint32_t)s->material[i] >= s->n_materials) return pt_fail(c, PT_ERR_ARGUMENT, "material index out of range");
        if (t == PT_PRIM_MESH || t == PT_PRIM_KDMESH) {
            if (s->prim_data[i] < 0 || (uint32_t)s->prim_data[i] >= s->n_meshes) return pt_fail(c, PT_ERR_ARGUMENT, "mesh index out of range");
            if (s->prim_flags[i] & 1) {
                if (!s->mesh_has_normals || !s->mesh_has_normals[s->prim_data[i]] || !s->mesh_normals)
                    return pt_fail(c, PT_ERR_SCENE, "smooth shading needs a vertex normal per vertex (mesh.rs:135-138)");
                *any_normals = true;
            }
        } else if (t == PT_PRIM_TRIANGLE) {
            if (s->prim_data[i] < 0 || (uint32_t)s->prim_data[i] >= s->n_triangles) return pt_fail(c, PT_ERR_ARGUMENT, "triangle index out of range");
            if (s->prim_flags[i] & 1) { if (!s->tri_normals) return pt_fail(c, PT_ERR_SCENE, "triangle normals missing"); *any_normals = true; }
        }
    }
    return PT_OK;
}

// Mesh m: its triangle records, its padded box, its PtMeshInfo and its place, and its tree where the host builds it (p.bvh / p.items).
static int pt_upload_pack_mesh(pt_context* c, PtUploadPlan& p, uint32_t m, const PtBuildPolicy& policy) {
    const pt_scene* s = p.s;
    pt_context::Resident& r = p.res;
    uint64_t v0 = s->mesh_vert_off[m], v1 = s->mesh_vert_off[m + 1], t0 = s->mesh_tri_off[m], t1 = s->mesh_tri_off[m + 1];
    if (v1 <= v0) return pt_fail(c, PT_ERR_SCENE, "meshes must have at least one vertex (mesh.rs:71)");
    const double* pos = s->mesh_positions + 3 * v0;
    const double* nrm = (s->mesh_normals && s->mesh_has_normals && s->mesh_has_normals[m]) ? s->mesh_normals + 3 * v0 : nullptr;
    PtBuildBox mb;
    const double ext = pt_mesh_vertex_box(pos, v1 - v0, &mb);
    const double pad = pt_triangle_pad(ext);
    const bool on_device = policy.on_device(t1 - t0);
    std::vector<PtBuildBox> boxes(on_device ? 0 : t1 - t0);
    std::vector<uint32_t> ids(on_device ? 0 : t1 - t0);
    for (uint64_t t = t0; t < t1; t++) {
        PtBuildBox b = pt_bvh_detail::empty_box();
        for (int corner = 0; corner < 3; corner++) {
            uint32_t vi = s->mesh_indices[3 * t + corner];
            if (vi >= v1 - v0) return pt_fail(c, PT_ERR_ARGUMENT, "mesh index out of range");
            for (int k = 0; k < 3; k++) {
                double x = pos[3 * (size_t)vi + k];
                p.tri_v[9 * t + 3 * corner + k] = x;
                if (r.any_normals) p.tri_n[9 * t + 3 * corner + k] = nrm ? nrm[3 * (size_t)vi + k] : 0.0;
                b.lo[k] = std::min(b.lo[k], x); b.hi[k] = std::max(b.hi[k], x);
            }
        }
        if (on_device) continue;
        for (int k = 0; k < 3; k++) { b.lo[k] -= pad; b.hi[k] += pad; }
        boxes[t - t0] = b;
        ids[t - t0] = (uint32_t)t;
    }
    PtBvhRef ref;
    ref.child = PT_REF_EMPTY; ref.depth = 0;
    pt_context::Resident::MeshPlace& pl = r.place[m];
    pl.n_verts = (uint32_t)(v1 - v0); pl.has_normals = nrm != nullptr; pl.device_built = on_device;
    pl.node_first = (uint32_t)p.bvh.size(); pl.item_first = (uint32_t)p.items.size();
    if (on_device) {  // built after the triangles are in HBM (pt_upload_commit); the place and the root are filled in then
        PtUploadPlan::DeviceMesh dm;
        dm.m = m; dm.pad = pad;
        for (int k = 0; k < 3; k++) { dm.lo[k] = mb.lo[k]; dm.hi[k] = mb.hi[k]; }
        p.device_meshes.push_back(dm);
    } else {
        ref = pt_bvh_build(boxes.data(), ids.data(), boxes.size(), r.blas_leaf, p.bvh, p.items);
        pl.node_count = (uint32_t)p.bvh.size() - pl.node_first; pl.item_count = (uint32_t)p.items.size() - pl.item_first; pl.depth = ref.depth;
    }
    PtMeshInfo& mi = r.meshes[m];
    for (int k = 0; k < 12; k++) mi.bbox_inv[k] = s->mesh_bounds_invtrans ? s->mesh_bounds_invtrans[16 * (size_t)m + k] : 0.0;
    if (!s->mesh_bounds_invtrans) return pt_fail(c, PT_ERR_ARGUMENT, "mesh_bounds_invtrans missing");
    mi.tri_first = (uint32_t)t0; mi.tri_count = (uint32_t)(t1 - t0);
    mi.blas_root = ref.child; mi.kd_root = -1; mi.kd_extent = 0.0;
    for (int k = 0; k < 12; k++) mi.kd_bbox_inv[k] = 0.0;
    pt_pad_mesh_box(&mb, ext);
    r.mesh_box[m] = mb;
    return PT_OK;
}

// ---- triangles: every mesh expanded to 72-byte vertex records, stand-alone triangles appended; the host's mesh trees
static int pt_upload_pack_triangles(pt_context* c, PtUploadPlan& p) {
    const pt_scene* s = p.s;
    pt_context::Resident& r = p.res;
    p.mesh_tris = s->n_meshes ? (size_t)s->mesh_tri_off[s->n_meshes] : 0;
    p.total_tris = p.mesh_tris + s->n_triangles;
    p.tri_v.resize(p.total_tris * 9); p.tri_n.resize(r.any_normals ? p.total_tris * 9 : 0);
    r.meshes.resize(s->n_meshes); r.mesh_box.resize(s->n_meshes); r.place.resize(s->n_meshes);
    r.blas_leaf = 2;  // triangles per mesh-tree leaf (measured: 2 beats 1, 3 and 4 by 2-5 % on cows / big-soup)
    if (const char* e = getenv("PORTRAYER_BLAS_LEAF")) r.blas_leaf = std::min(std::max(1, atoi(e)), 8);
    const PtBuildPolicy policy = pt_build_policy();
    for (uint32_t m = 0; m < s->n_meshes; m++)
        if (int rc = pt_upload_pack_mesh(c, p, m, policy)) return rc;
    return PT_OK;
}

// One KDMesh tree: its leaf items are local triangle indices - made global here (a leaf belongs to the mesh whose tree reaches it) -, the triangles' padded boxes
// for the walk's pre-cull, and the nodes' bounds bottom-up.
static int pt_upload_pack_kdmesh(pt_context* c, PtUploadPlan& p, uint32_t m, std::vector<int32_t>& owner) {
    const pt_scene* s = p.s;
    const int32_t root = s->mesh_kd_root[m];
    if ((uint32_t)root >= s->n_kdm_nodes) return pt_fail(c, PT_ERR_ARGUMENT, "KDMesh root out of range");
    std::vector<int32_t> todo{root}, visited;
    const double tri_pad = pt_triangle_pad(pt_box_extent(p.res.mesh_box[m]));
    const std::vector<PtKdNode>& mkd = p.mkd;
    while (!todo.empty()) {
        int32_t i = todo.back(); todo.pop_back();
        if (owner[i] >= 0) return pt_fail(c, PT_ERR_ARGUMENT, "KDMesh trees must not share nodes");
        owner[i] = (int32_t)m;
        visited.push_back(i);
        if (mkd[i].axis >= 0) { todo.push_back(mkd[i].front); todo.push_back(mkd[i].back); }
        else for (int32_t k = 0; k < mkd[i].count; k++) {
            int32_t local = s->kdm_items[mkd[i].first + k];
            if (local < 0 || (uint64_t)local >= s->mesh_tri_off[m + 1] - s->mesh_tri_off[m]) return pt_fail(c, PT_ERR_ARGUMENT, "KDMesh leaf triangle out of range");
            const uint64_t g = s->mesh_tri_off[m] + (uint64_t)local;
            p.mkd_items[mkd[i].first + k] = (uint32_t)g;
            float* ib = &p.mkd_item_box[6 * (size_t)(mkd[i].first + k)];  // the triangle's padded box, for the walk's pre-cull
            for (int r = 0; r < 3; r++) {
                const double* v = &p.tri_v[9 * g];
                ib[r] = pt_bvh_detail::round_down(std::min(v[r], std::min(v[3 + r], v[6 + r])) - tri_pad);
                ib[3 + r] = pt_bvh_detail::round_up(std::max(v[r], std::max(v[3 + r], v[6 + r])) + tri_pad);
            }
        }
    }
    for (size_t vi = visited.size(); vi-- > 0;) {  // children were discovered after their parents: bounds bottom-up
        const int32_t i = visited[vi];
        float* b = &p.mkd_box[6 * (size_t)i];
        for (int r = 0; r < 3; r++) { b[r] = (float)PT_BOX_LIMIT; b[3 + r] = -(float)PT_BOX_LIMIT; }
        auto grow = [&](const float* o) { for (int r = 0; r < 3; r++) { b[r] = std::min(b[r], o[r]); b[3 + r] = std::max(b[3 + r], o[3 + r]); } };
        if (mkd[i].axis >= 0) { grow(&p.mkd_box[6 * (size_t)mkd[i].front]); grow(&p.mkd_box[6 * (size_t)mkd[i].back]); }
        else for (int32_t k = 0; k < mkd[i].count; k++) grow(&p.mkd_item_box[6 * (size_t)(mkd[i].first + k)]);
    }
    PtMeshInfo& mi = p.res.meshes[m];
    mi.kd_root = root;
    const double* b = s->mesh_kd_bounds + 6 * (size_t)m;
    double dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
    mi.kd_extent = (dx * dx + dy * dy) + dz * dz;  // bounding_box.rs:95-99
    for (int r = 0; r < 12; r++) mi.kd_bbox_inv[r] = s->mesh_kd_bounds_invtrans[16 * (size_t)m + r];
    p.res.max_kdm_depth = std::max(p.res.max_kdm_depth, s->mesh_kd_depth ? std::max(s->mesh_kd_depth[m], 0) : 24);
    return PT_OK;
}

// ---- KDMesh triangle trees (reference structure) and their cull boxes
static int pt_upload_pack_kdmeshes(pt_context* c, PtUploadPlan& p) {
    const pt_scene* s = p.s;
    if (!(s->mesh_kd_root && s->n_kdm_nodes)) return PT_OK;
    if (!s->kdm_axis || !s->kdm_plane || !s->kdm_front || !s->kdm_back || !s->kdm_first || !s->kdm_count || (s->n_kdm_items && !s->kdm_items) ||
        !s->mesh_kd_bounds || !s->mesh_kd_bounds_invtrans)
        return pt_fail(c, PT_ERR_ARGUMENT, "incomplete KDMesh tree arrays");
    p.mkd.resize(s->n_kdm_nodes);
    for (uint32_t i = 0; i < s->n_kdm_nodes; i++) {
        PtKdNode& k = p.mkd[i];
        k.axis = s->kdm_axis[i]; k.plane = s->kdm_plane[i]; k.front = s->kdm_front[i]; k.back = s->kdm_back[i];
        k.first = s->kdm_first[i]; k.count = s->kdm_count[i]; k.pad = 0; k.pad2[0] = k.pad2[1] = 0.0f; for (int r = 0; r < 6; r++) k.box[r] = 0.0f;
        if (k.axis >= 0) {
            if (k.axis > 2 || k.front < 0 || k.back < 0 || (uint32_t)k.front >= s->n_kdm_nodes || (uint32_t)k.back >= s->n_kdm_nodes)
                return pt_fail(c, PT_ERR_ARGUMENT, "KDMesh tree child out of range");
        } else if (k.first < 0 || k.count < 0 || (uint32_t)(k.first + k.count) > s->n_kdm_items) {
            return pt_fail(c, PT_ERR_ARGUMENT, "KDMesh leaf range out of bounds");
        }
    }
    p.mkd_items.assign(s->n_kdm_items, 0);
    p.mkd_box.assign(6 * (size_t)s->n_kdm_nodes, 0.0f);
    p.mkd_item_box.assign(6 * (size_t)s->n_kdm_items, 0.0f);
    std::vector<int32_t> owner(s->n_kdm_nodes, -1);
    for (uint32_t m = 0; m < s->n_meshes; m++) {
        if (s->mesh_kd_root[m] < 0) continue;
        if (int rc = pt_upload_pack_kdmesh(c, p, m, owner)) return rc;
        p.traits.has_kdmesh = 1;
    }
    for (size_t i = 0; i < p.mkd.size(); i++) for (int r = 0; r < 6; r++) p.mkd[i].box[r] = p.mkd_box[6 * i + r];
    return PT_OK;
}

// ---- nodes: the graph (PT_TRAVERSE_HIER), the matrices, the info words and the world boxes
static int pt_upload_pack_nodes(pt_context* c, PtUploadPlan& p) {
    const pt_scene* s = p.s;
    pt_context::Resident& r = p.res;
    const uint32_t n = s->n_nodes;
    if (r.traverse == PT_TRAVERSE_HIER && n) {
        const uint32_t g = s->n_graph_nodes;
        r.chain_off.assign(s->node_chain_off, s->node_chain_off + n + 1);
        if (r.chain_off[0] != 0) return pt_fail(c, PT_ERR_ARGUMENT, "node_chain_off must start at 0");
        for (uint32_t i = 0; i < n; i++)
            if (r.chain_off[i + 1] <= r.chain_off[i]) return pt_fail(c, PT_ERR_ARGUMENT, "every flattened node needs a non-empty path (it contains at least itself)");
        r.chain.assign(s->node_chain, s->node_chain + r.chain_off[n]);
        for (uint32_t id : r.chain) if (id >= g) return pt_fail(c, PT_ERR_ARGUMENT, "node_chain names a graph node out of range");
        p.dfs_rank.assign(s->node_dfs_rank, s->node_dfs_rank + n);
        pt_pack_graph(n, g, s->graph_trans, s->graph_invtrans, s->graph_normal_trans, r.chain_off, r.chain, p.graph);
    }
    pt_pack_node_matrices(n, s->trans, s->invtrans, s->normal_trans, p.inv, p.fwd, p.nrm);
    for (uint32_t t = 0; t < s->n_triangles; t++)
        for (int k = 0; k < 9; k++) {
            p.tri_v[9 * (p.mesh_tris + t) + k] = s->tri_vertices[9 * (size_t)t + k];
            if (r.any_normals) p.tri_n[9 * (p.mesh_tris + t) + k] = s->tri_normals ? s->tri_normals[9 * (size_t)t + k] : 0.0;
        }
    r.tri_box.resize(s->n_triangles);
    for (uint32_t t = 0; t < s->n_triangles; t++) pt_triangle_model_box(&p.tri_v[9 * (p.mesh_tris + t)], &r.tri_box[t]);
    r.info.resize(4 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        int t = s->prim_type[i];
        uint32_t data = (uint32_t)s->prim_data[i];
        if (t == PT_PRIM_TRIANGLE) data = (uint32_t)(p.mesh_tris + data);
        r.info[4 * (size_t)i] = (uint32_t)t; r.info[4 * (size_t)i + 1] = data;
        r.info[4 * (size_t)i + 2] = (uint32_t)s->prim_flags[i]; r.info[4 * (size_t)i + 3] = (uint32_t)s->material[i];
        if (t == PT_PRIM_MESH || t == PT_PRIM_KDMESH) p.traits.instanced_tris += s->mesh_tri_off[s->prim_data[i] + 1] - s->mesh_tri_off[s->prim_data[i]];
    }
    pt_node_world_boxes(n, s->trans, r.info.data(), r.mesh_box, r.tri_box, p.mesh_tris, p.node_box, p.root_lo, p.root_hi);
    return PT_OK;
}

// ---- the scene-level tree, behind the host's mesh trees: it keeps room for the n - 1 nodes any tree over n leaves can have (pt_scene_update builds its
// trees into the same place); then the edge form of every triangle
static void pt_upload_pack_scene_tree(PtUploadPlan& p) {
    pt_context::Resident& r = p.res;
    const uint32_t n = r.n_nodes;
    r.tlas_leaf = 1;  // primitive tests (f64, ~200 instructions) cost far more than a node visit: measured best on big-scene
    if (const char* e = getenv("PORTRAYER_TLAS_LEAF")) r.tlas_leaf = std::max(1, atoi(e));
    p.tlas_direct = r.tlas_leaf == 1 && n < (1u << 28);
    r.tlas_first = p.bvh.size(); r.tlas_items = p.items.size(); r.tlas_cap = n ? n - 1 : 0;
    std::vector<PtBvhNode> tl_nodes;
    std::vector<uint32_t> tl_items;
    p.tlas = pt_build_scene_tree(p.node_box, r.tlas_leaf, p.tlas_direct, r.tlas_first, r.tlas_items, tl_nodes, tl_items);
    p.bvh.insert(p.bvh.end(), tl_nodes.begin(), tl_nodes.end());
    p.items.insert(p.items.end(), tl_items.begin(), tl_items.end());
    PtBvhNode unused;
    memset(&unused, 0, sizeof unused);
    unused.child0 = unused.child1 = PT_REF_EMPTY;
    p.bvh.resize(r.tlas_first + r.tlas_cap, unused);
    p.tri_e.resize(p.tri_v.size());
    for (size_t t = 0; t < p.total_tris; t++) {
        const double* v = &p.tri_v[9 * t];
        double* e = &p.tri_e[9 * t];
        e[0] = v[0]; e[1] = v[1]; e[2] = v[2];
        e[3] = v[0] - v[3]; e[4] = v[1] - v[4]; e[5] = v[2] - v[5];
        e[6] = v[0] - v[6]; e[7] = v[1] - v[7]; e[8] = v[2] - v[8];
    }
}

// ---- what the tree references can address: the host-built part of the tree arrays and the places of the device-built mesh trees behind it
static int pt_upload_check_tree_size(pt_context* c, PtUploadPlan& p) {
    p.tree_nodes = p.bvh.size(); p.tree_items = p.items.size();
    for (const PtUploadPlan::DeviceMesh& dm : p.device_meshes) {
        const uint32_t count = p.res.meshes[dm.m].tri_count;
        p.tree_nodes += PT_DEVICE_TREE_NODES(count); p.tree_items += PT_DEVICE_TREE_ITEMS(count, p.res.blas_leaf);
    }
    if (p.tree_items >= (1u << 28) || p.tree_nodes >= (1u << 26)) return pt_fail(c, PT_ERR_SCENE, "too many triangles for the 32-bit tree references (a node is addressed by a 32-bit byte offset: 2^26 nodes)");
    return PT_OK;
}

// ---- materials and lights, and what they say about the recursion (PtSceneTraits)
static void pt_upload_pack_shading(PtUploadPlan& p) {
    const pt_scene* s = p.s;
    p.mats.assign(s->materials, s->materials + 10 * (size_t)s->n_materials);
    p.lights.assign(s->lights, s->lights + 15 * (size_t)s->n_lights);
    PtSceneTraits& t = p.traits;
    t.reflective_opaque = 1;
    for (uint32_t m = 0; m < s->n_materials; m++) {
        const double* mat = &p.mats[10 * (size_t)m];
        if (!(mat[7] > 0.0)) continue;
        t.reflective = 1;                        // material.rs:216: reflectivity > 0 spawns children
        if (mat[8] > 0.0) t.glossy = 1;          // glossy reflection (material.rs:221-239)
        if (mat[9] > 0.0) t.reflective_opaque = 0;
    }
    pt_set_light_traits(t, p.lights.data(), s->n_lights);
}

// ---- textures / normal maps (texture.rs), and the check that every mapped material meets texture coordinates
static int pt_upload_pack_textures(pt_context* c, PtUploadPlan& p) {
    const pt_scene* s = p.s;
    for (uint32_t m = 0; m < s->n_materials; m++)
        if ((s->material_texture && s->material_texture[m] >= 0) || (s->material_normal_map && s->material_normal_map[m] >= 0)) p.textured = true;
    if (!p.textured) return PT_OK;
    if (s->n_textures == 0 || !s->texture_size || !s->texture_offset || !s->texture_rgb) return pt_fail(c, PT_ERR_ARGUMENT, "textured material without texture data");
    size_t tex_bytes = 0;
    p.texinfo.resize(s->n_textures);
    for (uint32_t t = 0; t < s->n_textures; t++) {
        PtTexInfo& ti = p.texinfo[t];
        ti.offset = s->texture_offset[t]; ti.width = s->texture_size[2 * t]; ti.height = s->texture_size[2 * t + 1];
        if (ti.width == 0 || ti.height == 0) return pt_fail(c, PT_ERR_ARGUMENT, "empty texture");
        tex_bytes = std::max(tex_bytes, (size_t)ti.offset + 3 * (size_t)ti.width * ti.height);
    }
    p.tex_rgb.assign(s->texture_rgb, s->texture_rgb + tex_bytes);
    p.mat_maps.resize(2 * (size_t)s->n_materials);
    p.uv_trans.resize(9 * (size_t)s->n_materials);
    for (uint32_t m = 0; m < s->n_materials; m++) {
        int32_t a = s->material_texture ? s->material_texture[m] : -1, b = s->material_normal_map ? s->material_normal_map[m] : -1;
        if (a >= (int32_t)s->n_textures || b >= (int32_t)s->n_textures) return pt_fail(c, PT_ERR_ARGUMENT, "texture index out of range");
        p.mat_maps[2 * m] = a < 0 ? -1 : a; p.mat_maps[2 * m + 1] = b < 0 ? -1 : b;
        for (int k = 0; k < 9; k++) p.uv_trans[9 * (size_t)m + k] = s->material_uv_trans ? s->material_uv_trans[9 * (size_t)m + k] : (k % 4 == 0 ? 1.0 : 0.0);
    }
    p.srgb_lut.resize(256);
    for (int k = 0; k < 256; k++) p.srgb_lut[k] = std::pow((double)k / 255.0, PT_GAMMA);  // texture.rs:167: c.powf(GAMMA), c = byte / 255
    p.tri_uv.assign(p.total_tris * 6, 0.0);
    std::vector<uint8_t> tri_has_uv(p.total_tris, 0);
    for (uint32_t m = 0; m < s->n_meshes; m++) {
        if (!(s->mesh_texcoords && s->mesh_has_texcoords && s->mesh_has_texcoords[m])) continue;
        uint64_t v0 = s->mesh_vert_off[m];
        for (uint64_t t = s->mesh_tri_off[m]; t < s->mesh_tri_off[m + 1]; t++) {
            for (int corner = 0; corner < 3; corner++) {
                uint64_t vi = v0 + s->mesh_indices[3 * t + corner];
                p.tri_uv[6 * t + 2 * corner] = s->mesh_texcoords[2 * vi]; p.tri_uv[6 * t + 2 * corner + 1] = s->mesh_texcoords[2 * vi + 1];
            }
            tri_has_uv[t] = 1;
        }
        p.res.place[m].has_uv = true;
    }
    for (uint32_t t = 0; t < s->n_triangles; t++)
        if (s->tri_texcoords && s->tri_has_texcoords && s->tri_has_texcoords[t]) {
            for (int k = 0; k < 6; k++) p.tri_uv[6 * (p.mesh_tris + t) + k] = s->tri_texcoords[6 * (size_t)t + k];
            tri_has_uv[p.mesh_tris + t] = 1;
        }
    // material.rs:133 / :141: the reference panics when a mapped material meets a primitive without texture coordinates
    for (uint32_t i = 0; i < s->n_nodes; i++) {
        int32_t m = s->material[i];
        if (p.mat_maps[2 * m] < 0 && p.mat_maps[2 * m + 1] < 0) continue;
        int t = s->prim_type[i];
        bool ok = t == PT_PRIM_SPHERE || t == PT_PRIM_CUBE || t == PT_PRIM_PLANE;
        if (t == PT_PRIM_TRIANGLE) ok = tri_has_uv[p.mesh_tris + (size_t)s->prim_data[i]];
        if (t == PT_PRIM_MESH || t == PT_PRIM_KDMESH) ok = s->mesh_tri_off[s->prim_data[i] + 1] == s->mesh_tri_off[s->prim_data[i]] || tri_has_uv[s->mesh_tri_off[s->prim_data[i]]];
        if (!ok) return pt_fail(c, PT_ERR_SCENE, "Texture mapping is not supported for this primitive! (material.rs:133,141)");
    }
    return PT_OK;
}

// Every check of pt_scene_upload that the host can decide and everything its host side computes; no HIP call. From the first check of the scene's content on the
// context has no scene, whatever the outcome (a refused upload leaves it without one); pt_upload_commit gives it the new one.
static int pt_upload_prepare(pt_context* c, const pt_scene* s, int traverse, const pt_kdtree* kd, PtUploadPlan& p) {
    if (!c || !s) return PT_ERR_ARGUMENT;
    if (traverse != PT_TRAVERSE_FLAT && traverse != PT_TRAVERSE_KD && traverse != PT_TRAVERSE_HIER)
        return pt_fail(c, PT_ERR_ARGUMENT, "traverse must be PT_TRAVERSE_FLAT, PT_TRAVERSE_KD or PT_TRAVERSE_HIER");
    if (traverse == PT_TRAVERSE_HIER && s->n_nodes &&
        (!s->n_graph_nodes || !s->graph_trans || !s->graph_invtrans || !s->graph_normal_trans || !s->node_chain_off || !s->node_chain || !s->node_dfs_rank))
        return pt_fail(c, PT_ERR_ARGUMENT, "PT_TRAVERSE_HIER needs the scene graph (graph_*, node_chain*, node_dfs_rank)");
    if (traverse == PT_TRAVERSE_KD && !kd) return pt_fail(c, PT_ERR_ARGUMENT, "PT_TRAVERSE_KD needs the host-built k-d tree");
    if (s->n_nodes && (!s->trans || !s->invtrans || !s->normal_trans || !s->prim_type || !s->prim_data || !s->prim_flags || !s->material))
        return pt_fail(c, PT_ERR_ARGUMENT, "null node array");
    c->have_scene = false;
    p.s = s;
    p.verbose = getenv("PORTRAYER_VERBOSE") != nullptr;
    p.t_lap = std::chrono::steady_clock::now();
    pt_context::Resident& r = p.res;
    r.traverse = traverse; r.n_nodes = s->n_nodes; r.n_graph = traverse == PT_TRAVERSE_HIER && s->n_nodes ? s->n_graph_nodes : 0u; r.n_lights = s->n_lights;
    p.traits.traverse = traverse; p.traits.n_nodes = s->n_nodes; p.traits.has_meshes = s->n_meshes > 0;
    int rc;
    if ((rc = pt_upload_check_nodes(c, s, &r.any_normals)) || (rc = pt_upload_pack_triangles(c, p))) return rc;
    p.lap("triangles + mesh trees");
    if ((rc = pt_upload_pack_kdmeshes(c, p)) || (rc = pt_upload_pack_nodes(c, p))) return rc;
    pt_upload_pack_scene_tree(p);
    // ---- k-d tree (reference structure, KD mode)
    if (traverse == PT_TRAVERSE_KD && (rc = pt_pack_kd(c, kd, s->n_nodes, p.node_box, p.kda))) return rc;
    p.lap("scene tree");
    if ((rc = pt_upload_check_tree_size(c, p))) return rc;
    pt_upload_pack_shading(p);
    if ((rc = pt_upload_pack_textures(c, p))) return rc;
    r.mesh_tris = p.mesh_tris;
    r.indices.assign(s->mesh_indices, s->mesh_indices + (p.mesh_tris ? 3 * p.mesh_tris : 0));
    return PT_OK;
}

// The device-built mesh trees, each into its place behind the host-built part of bvh / bvh_items (the triangles are resident).
static int pt_upload_build_device_trees(pt_context* c, PtUploadPlan& p) {
    pt_context::Resident& r = c->res;
    uint32_t node_base = (uint32_t)p.bvh.size(), item_base = (uint32_t)p.items.size();
    float device_ms = 0.0f;
    int rounds = 0, depth = 0;
    for (const PtUploadPlan::DeviceMesh& dm : p.device_meshes) {
        PtDeviceBuildResult built;
        pt_context::Resident::MeshPlace& pl = r.place[dm.m];
        const uint32_t count = r.meshes[dm.m].tri_count;
        pl.node_first = node_base; pl.node_count = PT_DEVICE_TREE_NODES(count); pl.item_first = item_base; pl.item_count = PT_DEVICE_TREE_ITEMS(count, r.blas_leaf);
        if (int rc = pt_build_mesh_tree_in_place(c, pl, r.meshes[dm.m], dm.lo, dm.hi, dm.pad, &built)) return rc;
        node_base += pl.node_count; item_base += pl.item_count;
        device_ms += built.ms; rounds += built.rounds;
    }
    for (const auto& pl : r.place) depth = std::max(depth, pl.depth);
    if (p.verbose && !p.device_meshes.empty()) fprintf(stderr, "[pt_scene_upload] device tree build: %zu mesh(es), %.2f ms, %d clustering rounds, depth %d\n", p.device_meshes.size(), device_ms, rounds, depth);
    return PT_OK;
}

// Triangles and trees: the reserves, the copies, the device's mesh trees, the four-child form and the leaf-order records.
static int pt_upload_commit_trees(pt_context* c, PtUploadPlan& p) {
    int rc;
    if ((rc = pt_upload(c, c->tri_v, p.tri_v)) || (rc = pt_upload(c, c->tri_e, p.tri_e))) return rc;
    // tree arrays: the host-built part first, then room for the device-built mesh trees
    if ((rc = pt_reserve(c, c->bvh, p.tree_nodes * sizeof(PtBvhNode))) || (rc = pt_reserve(c, c->bvh_items, p.tree_items * sizeof(uint32_t)))) return rc;
    if (!p.bvh.empty()) PT_HIP(c, hipMemcpy(c->bvh.p, p.bvh.data(), p.bvh.size() * sizeof(PtBvhNode), hipMemcpyHostToDevice));
    if (!p.items.empty()) PT_HIP(c, hipMemcpy(c->bvh_items.p, p.items.data(), p.items.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    p.lap("upload triangles + host trees");
    if ((rc = pt_upload_build_device_trees(c, p))) return rc;
    p.lap("device mesh trees");
    // the walks read the four-child form of every tree (scene tree and mesh trees alike)
    if ((rc = pt_reserve(c, c->bvh4, std::max<size_t>(p.tree_nodes, 1) * sizeof(PtBvh4Node))) || (rc = pt_queue_collapse4(c, 0, p.tree_nodes))) return rc;
    PT_HIP(c, hipDeviceSynchronize());
    p.lap("four-child form");
    if ((rc = pt_reserve(c, c->tri_leaf, std::max<size_t>(p.tree_items, 1) * 80))) return rc;
    if (p.total_tris && (rc = pt_queue_tri_leaf(c, 0, p.tree_items))) return rc;
    PT_HIP(c, hipDeviceSynchronize());
    p.lap("triangle records in leaf order");
    return PT_OK;
}

// Everything else the kernels read, and the view of it.
static int pt_upload_commit_rest(pt_context* c, PtUploadPlan& p) {
    const pt_scene* s = p.s;
    const pt_context::Resident& r = c->res;
    int rc;
    if ((rc = pt_upload(c, c->g_inv, p.graph.g_inv)) || (rc = pt_upload(c, c->g_fwd, p.graph.g_fwd)) || (rc = pt_upload(c, c->g_nrm, p.graph.g_nrm)) ||
        (rc = pt_upload(c, c->chain_off, r.chain_off)) || (rc = pt_upload(c, c->chain, r.chain)) || (rc = pt_upload(c, c->dfs_rank, p.dfs_rank)) ||
        (rc = pt_upload(c, c->hier_rec, p.graph.hier_rec)) || (rc = pt_upload(c, c->own_inv, p.graph.own_inv)))
        return rc;
    if ((rc = pt_upload(c, c->inv, p.inv)) || (rc = pt_upload(c, c->fwd, p.fwd)) || (rc = pt_upload(c, c->nrm, p.nrm)) ||
        (rc = pt_upload(c, c->info, r.info)) || (rc = pt_upload(c, c->tri_n, p.tri_n)) ||
        (rc = pt_upload(c, c->meshes, r.meshes)) || (rc = pt_upload(c, c->mkd, p.mkd)) ||
        (rc = pt_upload(c, c->mkd_items, p.mkd_items)) || (rc = pt_upload(c, c->mkd_box, p.mkd_box)) || (rc = pt_upload(c, c->mkd_item_box, p.mkd_item_box)))
        return rc;
    if ((rc = pt_upload(c, c->materials, p.mats)) || (rc = pt_upload(c, c->lights, p.lights)) || (rc = pt_upload_mesh_boxes(c, r.mesh_box))) return rc;
    if (p.textured && ((rc = pt_upload(c, c->mat_maps, p.mat_maps)) || (rc = pt_upload(c, c->uv_trans, p.uv_trans)) || (rc = pt_upload(c, c->tex, p.texinfo)) ||
                       (rc = pt_upload(c, c->tex_rgb, p.tex_rgb)) || (rc = pt_upload(c, c->srgb_lut, p.srgb_lut)) || (rc = pt_upload(c, c->tri_uv, p.tri_uv))))
        return rc;
    PtSceneView& v = c->view;
    memset(&v, 0, sizeof v);
    v.n_nodes = r.n_nodes; v.n_lights = s->n_lights;
    v.inv = (const double*)c->inv.p; v.fwd = (const double*)c->fwd.p; v.nrm = (const double*)c->nrm.p;
    v.info = (const uint32_t*)c->info.p; v.tri_v = (const double*)c->tri_v.p; v.tri_e = (const double*)c->tri_e.p; v.tri_leaf = (const double*)c->tri_leaf.p; v.tri_n = (const double*)c->tri_n.p;
    v.meshes = (const PtMeshInfo*)c->meshes.p; v.materials = (const double*)c->materials.p; v.lights = (const double*)c->lights.p;
    for (int k = 0; k < 3; k++) v.ambient[k] = s->ambient[k];
    v.bvh = (const PtBvhNode*)c->bvh.p; v.bvh4 = (const PtBvh4Node*)c->bvh4.p; v.bvh_items = (const uint32_t*)c->bvh_items.p;
    v.tlas_root = p.tlas.child; v.tlas_direct = p.tlas_direct ? 1u : 0u;
    // the octant-sorted slab test inside mesh instances (pt_trace_packet_mesh; round 4, c32: the 1.25 M-triangle scenes +6.0 % / +3.1 %, macho-cows and the
    // mirror scene +0.6 %; PORTRAYER_MESH_OCT=0 walks every triangle tree with the per-lane form again)
    v.mesh_oct = 1u;
    if (const char* e = getenv("PORTRAYER_MESH_OCT")) v.mesh_oct = atoi(e) > 0 ? 1u : 0u;
    if ((rc = pt_upload_kd(c, p.kda, r.traverse == PT_TRAVERSE_KD))) return rc;
    v.mkd = p.mkd.empty() ? nullptr : (const PtKdNode*)c->mkd.p; v.mkd_items = (const uint32_t*)c->mkd_items.p;  // (null without KDMesh trees: the k-d walk then keeps no LDS rows for lane stacks)
    v.mkd_box = p.mkd_box.empty() || getenv("PORTRAYER_KD_NO_CULL") ? nullptr : (const float*)c->mkd_box.p;
    v.mkd_item_box = v.mkd_box ? (const float*)c->mkd_item_box.p : nullptr;
    v.mode = pt_scene_mode(c->traits);
    if (r.traverse == PT_TRAVERSE_HIER) {
        v.g_inv = (const double*)c->g_inv.p; v.g_fwd = (const double*)c->g_fwd.p; v.g_nrm = (const double*)c->g_nrm.p;
        v.chain_off = (const uint32_t*)c->chain_off.p; v.chain = (const uint32_t*)c->chain.p; v.dfs_rank = (const uint32_t*)c->dfs_rank.p;
        v.hier_rec = (const uint32_t*)c->hier_rec.p; v.own_inv = (const double*)c->own_inv.p;
    }
    if (p.textured) {
        v.mat_maps = (const int32_t*)c->mat_maps.p; v.uv_trans = (const double*)c->uv_trans.p; v.tex = (const PtTexInfo*)c->tex.p;
        v.tex_rgb = (const uint8_t*)c->tex_rgb.p; v.srgb_lut = (const double*)c->srgb_lut.p; v.tri_uv = (const double*)c->tri_uv.p;
        std::vector<PtTexView> tv(1);
        tv[0].tex = v.tex; tv[0].tex_rgb = v.tex_rgb; tv[0].uv_trans = v.uv_trans; tv[0].tri_v = v.tri_v; tv[0].tri_uv = v.tri_uv;
        tv[0].mat_maps = v.mat_maps;
        if ((rc = pt_upload(c, c->texview, tv))) return rc;
        v.texview = (const PtTexView*)c->texview.p;
    }
    return PT_OK;
}

// The writes: the context takes the plan's host state (pt_context::Resident, the traits, the root box), then the device gets its arrays. The stack is sized
// here, not in pt_upload_prepare, because the depth of a device-built mesh tree is only known once it is built (the note on pt_update_prepare).
static int pt_upload_commit(pt_context* c, PtUploadPlan& p) {
    PT_HIP(c, hipSetDevice(c->device));
    c->res = std::move(p.res);
    c->res.tree_nodes = p.tree_nodes;
    c->res.collapse_mode = 1;  // how two-child trees become four-child trees (pt_collapse4_kernel): 0 grandchildren, 1 mesh trees opened by area, 2 every tree by area
    if (const char* e = getenv("PORTRAYER_COLLAPSE")) c->res.collapse_mode = strcmp(e, "plain") == 0 ? 0 : (strcmp(e, "area") == 0 ? 2 : 1);
    c->traits = p.traits;
    for (int k = 0; k < 3; k++) { c->root_lo[k] = p.root_lo[k]; c->root_hi[k] = p.root_hi[k]; }
    int rc;
    if ((rc = pt_upload_commit_trees(c, p)) || (rc = pt_upload_commit_rest(c, p))) return rc;
    c->res.below = pt_stack_below(c->res);
    rc = pt_set_stack_cap(c, p.tlas.depth, p.kda.kd_depth);
    p.lap("upload the rest");
    if (rc) return rc;
    c->have_scene = true;
    return PT_OK;
}

extern "C" int pt_scene_upload(pt_context* c, const pt_scene* s, int traverse, const pt_kdtree* kd) {
    PtUploadPlan plan;
    int rc = pt_upload_prepare(c, s, traverse, kd, plan);
    return rc ? rc : pt_upload_commit(c, plan);
}

// ------------------------------------------------------------------------------------------------
// Scene update: the resident scene with new node matrices, lights and ambient light. Everything under a flattened node lives in model space
// (triangle records, mesh trees, KDMesh trees, textures) and stays where it is; what depends on the matrices is recomputed by the functions
// pt_scene_upload uses (above), and the scene-level tree is rebuilt in the place the upload reserved for it - on the host (pt_bvh_build: the
// upload's tree) or on the device (pt_device_build_scene_tree), by the rule mesh trees follow: PORTRAYER_BUILD = host | device | auto,
// auto takes the device from PORTRAYER_BUILD_MIN nodes on (default 65536), device from 16 on; PORTRAYER_TLAS_LEAF != 1: always the host.
// ------------------------------------------------------------------------------------------------
// What an update computes on the host before its first write (pt_update_prepare) and then writes (pt_update_commit). pt_scene_deform runs the same two
// steps around its own writes, with the deformed meshes' new boxes.
struct PtUpdatePlan {
    std::vector<double> inv, fwd, nrm;
    PtGraphArrays graph;
    std::vector<PtBuildBox> node_box;
    double root_lo[3], root_hi[3];
    PtKdArrays kda;
    bool direct = false, on_device = false;
    std::vector<PtBvhNode> tl_nodes;
    std::vector<uint32_t> tl_items;
    PtBvhRef tlas;
};

// the copies and kernels of an update or a deform are not ordered against the context's non-blocking streams
static int pt_refuse_in_flight(pt_context* c) {
    bool in_flight = false;
    for (const PtPass* v : c->passes) in_flight = in_flight || v->pending;
    for (const auto& sl : c->slot) in_flight = in_flight || sl.pending;
    if (in_flight) return pt_fail(c, PT_ERR_ARGUMENT, "a render is in flight: pt_render_finish / pt_aov_finish / pt_rays_finish / pt_radiance_finish first");
    return PT_OK;
}

// Every check of pt_scene_update and everything its host side computes. `mesh_box`: the meshes' padded model boxes the moved scene has (the resident ones,
// or a deform's). Writes nothing to the device; PT_ERR_SCENE leaves the context without a scene, as after a refused upload.
// On the host-build path it does set view.stack_cap (pt_set_stack_cap) from the mesh depths as they are BEFORE the call: for a deform with rebuild = 1
// that is half a check - a mesh tree the rebuild makes deeper is only seen by pt_update_commit, which computes the cap again after the writes and then
// ends with PT_ERR_SCENE and no scene, as the header says.
static int pt_update_prepare(pt_context* c, const pt_scene_motion* mo, const pt_kdtree* kd, const std::vector<PtBuildBox>& mesh_box, PtUpdatePlan& p) {
    if (!c || !mo) return PT_ERR_ARGUMENT;
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    pt_context::Resident& res = c->res;
    const uint32_t n = res.n_nodes;
    if (mo->n_nodes != n) return pt_fail(c, PT_ERR_ARGUMENT, "n_nodes differs from the uploaded scene's");
    if (n && (!mo->trans || !mo->invtrans || !mo->normal_trans)) return pt_fail(c, PT_ERR_ARGUMENT, "null node array");
    if (mo->n_graph_nodes != res.n_graph) return pt_fail(c, PT_ERR_ARGUMENT, "n_graph_nodes differs from the uploaded scene's (0 unless it was uploaded with PT_TRAVERSE_HIER)");
    if (res.n_graph && (!mo->graph_trans || !mo->graph_invtrans || !mo->graph_normal_trans))
        return pt_fail(c, PT_ERR_ARGUMENT, "PT_TRAVERSE_HIER needs the scene graph's matrices (graph_*)");
    if (mo->lights && mo->n_lights != res.n_lights) return pt_fail(c, PT_ERR_ARGUMENT, "n_lights differs from the uploaded scene's");
    if (res.traverse == PT_TRAVERSE_KD && !kd) return pt_fail(c, PT_ERR_ARGUMENT, "PT_TRAVERSE_KD needs the host-built k-d tree");
    if (res.traverse != PT_TRAVERSE_KD && kd) return pt_fail(c, PT_ERR_ARGUMENT, "a k-d tree for a scene that was not uploaded with PT_TRAVERSE_KD");
    if (int rc = pt_refuse_in_flight(c)) return rc;

    // ---- everything the host computes, before the first write
    pt_pack_node_matrices(n, mo->trans, mo->invtrans, mo->normal_trans, p.inv, p.fwd, p.nrm);
    if (res.n_graph) pt_pack_graph(n, res.n_graph, mo->graph_trans, mo->graph_invtrans, mo->graph_normal_trans, res.chain_off, res.chain, p.graph);
    pt_node_world_boxes(n, mo->trans, res.info.data(), mesh_box, res.tri_box, res.mesh_tris, p.node_box, p.root_lo, p.root_hi);
    int rc;
    if (res.traverse == PT_TRAVERSE_KD && (rc = pt_pack_kd(c, kd, n, p.node_box, p.kda))) {
        if (rc == PT_ERR_SCENE) c->have_scene = false;  // as after a refused upload
        return rc;
    }
    p.direct = res.tlas_leaf == 1 && n < (1u << 28);
    p.on_device = p.direct && pt_build_policy().on_device(n);
    p.tlas.child = PT_REF_EMPTY; p.tlas.depth = 0;
    if (!p.on_device) {
        p.tlas = pt_build_scene_tree(p.node_box, res.tlas_leaf, p.direct, res.tlas_first, res.tlas_items, p.tl_nodes, p.tl_items);
        if (p.tl_nodes.size() > res.tlas_cap || p.tl_items.size() > (p.direct ? 0u : n)) return pt_fail(c, PT_ERR_DEVICE, "scene tree larger than its place");  // (a tree over n leaves has at most n - 1 nodes)
        if ((rc = pt_set_stack_cap(c, p.tlas.depth, p.kda.kd_depth))) { c->have_scene = false; return rc; }
    }
    return PT_OK;
}

// ---- writes
static int pt_update_commit(pt_context* c, const pt_scene_motion* mo, PtUpdatePlan& p) {
    pt_context::Resident& res = c->res;
    const uint32_t n = res.n_nodes;
    int rc;
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipDeviceSynchronize());  // passes whose _finish has been called may still have copies queued
    c->have_scene = false;              // until every write below has been made
    if ((rc = pt_upload(c, c->inv, p.inv)) || (rc = pt_upload(c, c->fwd, p.fwd)) || (rc = pt_upload(c, c->nrm, p.nrm))) return rc;
    if (res.n_graph && ((rc = pt_upload(c, c->g_inv, p.graph.g_inv)) || (rc = pt_upload(c, c->g_fwd, p.graph.g_fwd)) || (rc = pt_upload(c, c->g_nrm, p.graph.g_nrm)) ||
                        (rc = pt_upload(c, c->hier_rec, p.graph.hier_rec)) || (rc = pt_upload(c, c->own_inv, p.graph.own_inv))))
        return rc;
    if (res.traverse == PT_TRAVERSE_KD && (rc = pt_upload_kd(c, p.kda, true))) return rc;
    for (int k = 0; k < 3; k++) { c->root_lo[k] = p.root_lo[k]; c->root_hi[k] = p.root_hi[k]; }
    PtSceneView& v = c->view;
    if (mo->lights) {
        std::vector<double> lights(mo->lights, mo->lights + 15 * (size_t)mo->n_lights);
        if ((rc = pt_upload(c, c->lights, lights))) return rc;
        pt_set_light_traits(c->traits, lights.data(), mo->n_lights);
    }
    if (mo->ambient) for (int k = 0; k < 3; k++) v.ambient[k] = mo->ambient[k];
    PtBvhRef tlas = p.tlas;
    if (p.on_device) {
        PtDeviceBuildResult built;
        PT_HIP(c, pt_device_build_scene_tree(n, (const double*)c->fwd.p, (const uint32_t*)c->info.p, (const double*)c->mesh_box_dev.p, (const double*)c->tri_v.p,
                                             p.root_lo, p.root_hi, (PtBvhNode*)c->bvh.p, (uint32_t)res.tlas_first, nullptr, &built));
        tlas.child = built.root; tlas.depth = built.depth;
        if (getenv("PORTRAYER_VERBOSE")) fprintf(stderr, "[pt_scene_update] device scene tree: %u nodes, %.2f ms, %d clustering rounds, depth %d\n", n, built.ms, built.rounds, built.depth);
        res.last_builder = 2; res.last_rounds = built.rounds;
    } else {
        res.last_builder = 1; res.last_rounds = 0;
        if (!p.tl_nodes.empty()) PT_HIP(c, hipMemcpy((PtBvhNode*)c->bvh.p + res.tlas_first, p.tl_nodes.data(), p.tl_nodes.size() * sizeof(PtBvhNode), hipMemcpyHostToDevice));
        if (!p.tl_items.empty()) PT_HIP(c, hipMemcpy((uint32_t*)c->bvh_items.p + res.tlas_items, p.tl_items.data(), p.tl_items.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // the stack of the trees as they are now: the scene-level tree just built and (pt_scene_deform) mesh trees a rebuild may have made deeper
    if ((rc = pt_set_stack_cap(c, tlas.depth, p.kda.kd_depth))) return rc;  // (have_scene stays false)
    if ((rc = pt_queue_collapse4(c, res.tlas_first, res.tlas_first + res.tlas_cap))) return rc;  // the four-child form of the new tree alone, opened as the upload opened it
    PT_HIP(c, hipDeviceSynchronize());
    v.tlas_root = tlas.child;
    c->have_scene = true;
    return PT_OK;
}

extern "C" int pt_scene_update(pt_context* c, const pt_scene_motion* mo, const pt_kdtree* kd) {
    if (!c || !mo) return PT_ERR_ARGUMENT;
    PtUpdatePlan plan;
    int rc = pt_update_prepare(c, mo, kd, c->res.mesh_box, plan);
    if (rc) return rc;
    return pt_update_commit(c, mo, plan);
}

// ------------------------------------------------------------------------------------------------
// Scene deform: new vertices for resident meshes under the topology they were uploaded with, then the update above. Per mesh the host
// computes the box (the upload's function) and copies the vertices; the device expands the triangle records through the resident indices
// (pt_device_expand_mesh), refits the mesh's tree in place or rebuilds it there (pt_device_refit_mesh_tree / pt_device_build_mesh_tree) and re-derives
// the four-child form and the leaf-order records for the mesh's node and item ranges alone. With the vertices already in device memory
// (pt_scene_deform_device) the box is a reduction on the device (pt_device_vertex_box) and the expand kernel reads the caller's buffer in place.
// ------------------------------------------------------------------------------------------------
// One mesh of a deform, wherever its vertices are: pt_mesh_deform's fields with host pointers, pt_mesh_deform_device's with device pointers.
struct PtDeformItem {
    uint32_t mesh;
    const double *positions, *normals, *bounds_invtrans;
    int32_t rebuild;
};

// What keeps a caller's mistake from becoming a GPU fault: `p` must be 8-byte aligned device memory of the context's device whose allocation reaches `bytes`
// beyond it. The context's device is current.
int pt_check_device_pointer(pt_context* c, const void* p, uint64_t bytes, const std::string& what) {
    if ((uintptr_t)p & 7u) return pt_fail(c, PT_ERR_ARGUMENT, what + " is not 8-byte aligned");
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // (pageable host memory: the query itself fails, and leaves its error behind)
        return pt_fail(c, PT_ERR_ARGUMENT, what + " is not device memory (hipPointerGetAttributes does not know the pointer)");
    }
    if (at.type != hipMemoryTypeDevice || at.isManaged)
        return pt_fail(c, PT_ERR_ARGUMENT, what + " is not device memory (host, pinned or managed memory: copy it to the device, or use pt_scene_deform)");
    if (at.device != c->device)
        return pt_fail(c, PT_ERR_ARGUMENT, what + " is memory of device " + std::to_string(at.device) + ", the context is on device " + std::to_string(c->device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess || !base) {
        (void)hipGetLastError();
        return pt_fail(c, PT_ERR_ARGUMENT, what + ": hipMemGetAddressRange does not know the pointer's allocation");
    }
    const uint64_t off = (uint64_t)((const char*)p - (const char*)base);
    if ((const char*)p < (const char*)base || off > size || bytes > size - off)
        return pt_fail(c, PT_ERR_ARGUMENT, what + ": the allocation ends " + std::to_string(size - std::min<uint64_t>(off, size)) + " bytes after the pointer, " + std::to_string(bytes) + " are needed (n_vertices x 24)");
    return PT_OK;
}

// The box and the count of non-finite coordinates of n x 3 f64 in device memory (pt_device_vertex_box): the pointer has passed pt_check_device_pointer, the
// context's device is current and synchronised. One copy brings the result back.
static int pt_vertex_box_on_device(pt_context* c, uint64_t n, const double* d_pos, PtBuildBox* box, uint64_t* non_finite) {
    int rc = pt_reserve(c, c->vbox, (size_t)pt_vertex_box_partials(c->n_cu) * sizeof(PtVboxPartial));
    if (rc) return rc;
    PT_HIP(c, pt_device_vertex_box(d_pos, n, c->n_cu, (PtVboxPartial*)c->vbox.p, nullptr));
    PtVboxPartial got;
    PT_HIP(c, hipMemcpy(&got, c->vbox.p, sizeof got, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) { box->lo[k] = got.v[k]; box->hi[k] = got.v[3 + k]; }
    *non_finite = got.non_finite;
    return PT_OK;
}

extern "C" int pt_vertex_bounds_device(pt_context* c, uint64_t n_vertices, const double* d_positions, double out[6], uint64_t* non_finite) {
    if (!c) return PT_ERR_ARGUMENT;
    if (!out || !non_finite) return pt_fail(c, PT_ERR_ARGUMENT, "out and non_finite are required");
    if (n_vertices > 0xFFFFFFFFull) return pt_fail(c, PT_ERR_ARGUMENT, "n_vertices must be below 2^32");
    PtBuildBox box = pt_bvh_detail::empty_box();
    *non_finite = 0;
    if (n_vertices) {
        if (!d_positions) return pt_fail(c, PT_ERR_ARGUMENT, "d_positions is required");
        PT_HIP(c, hipSetDevice(c->device));
        int rc = pt_check_device_pointer(c, d_positions, n_vertices * 24, "d_positions");
        if (rc) return rc;
        PT_HIP(c, hipDeviceSynchronize());  // behind whatever stream produced the vertices
        if ((rc = pt_vertex_box_on_device(c, n_vertices, d_positions, &box, non_finite))) return rc;
    }
    for (int k = 0; k < 3; k++) { out[k] = box.lo[k]; out[3 + k] = box.hi[k]; }
    return PT_OK;
}

// pt_scene_deform and pt_scene_deform_device: the two differ in where a mesh's box comes from (the host loop / the device reduction behind the pointer check)
// and in which pointer the expand kernel reads (the staging buffer the vertices are copied to / the caller's buffer in place).
static int pt_deform_meshes(pt_context* c, const std::vector<PtDeformItem>& items, bool on_device, const pt_scene_motion* mo, const pt_kdtree* kd) {
    if (!c->have_scene) return pt_fail(c, PT_ERR_NO_SCENE, "no scene uploaded");
    pt_context::Resident& res = c->res;
    const uint32_t n_deforms = (uint32_t)items.size();
    struct NewBox { PtBuildBox vertex, padded; double ext; };
    std::vector<NewBox> nb(n_deforms);
    std::vector<PtBuildBox> mesh_box = res.mesh_box;
    {
        std::vector<uint8_t> named(res.place.size(), 0);
        bool synchronised = false;
        for (uint32_t d = 0; d < n_deforms; d++) {
            const PtDeformItem& df = items[d];
            const std::string at = "deform " + std::to_string(d) + ": ";
            if (!df.positions || !df.bounds_invtrans) return pt_fail(c, PT_ERR_ARGUMENT, at + "positions and bounds_invtrans are required");
            if (df.mesh >= res.place.size()) return pt_fail(c, PT_ERR_ARGUMENT, at + "mesh index out of range");
            if (named[df.mesh]) return pt_fail(c, PT_ERR_ARGUMENT, at + "the mesh is named twice");
            named[df.mesh] = 1;
            const pt_context::Resident::MeshPlace& pl = res.place[df.mesh];
            if (df.normals && !pl.has_normals) return pt_fail(c, PT_ERR_ARGUMENT, at + "normals for a mesh that was uploaded without normals");
            if (res.meshes[df.mesh].kd_root >= 0)
                return pt_fail(c, PT_ERR_ARGUMENT, at + "the mesh has a KDMesh tree, which the host builds from the positions: upload the scene again");
            if (df.rebuild != 0 && df.rebuild != 1) return pt_fail(c, PT_ERR_ARGUMENT, at + "rebuild must be 0 or 1");
            if (df.rebuild && !pl.device_built)
                return pt_fail(c, PT_ERR_ARGUMENT, at + "rebuild = 1 needs a tree the device built at upload (its place has the worst-case size); this one was built on the host");
            bool finite = true;
            if (on_device) {
                nb[d].vertex = pt_bvh_detail::empty_box();
                if (pl.n_verts) {  // (nothing is launched on an empty mesh, and nothing of it is read)
                    int rc = pt_refuse_in_flight(c);
                    if (rc) return rc;
                    PT_HIP(c, hipSetDevice(c->device));
                    if ((rc = pt_check_device_pointer(c, df.positions, (uint64_t)pl.n_verts * 24, at + "d_positions"))) return rc;
                    if (df.normals && (rc = pt_check_device_pointer(c, df.normals, (uint64_t)pl.n_verts * 24, at + "d_normals"))) return rc;
                    if (!synchronised) PT_HIP(c, hipDeviceSynchronize());  // behind whatever stream produced the vertices
                    synchronised = true;
                    uint64_t non_finite = 0;
                    if ((rc = pt_vertex_box_on_device(c, pl.n_verts, df.positions, &nb[d].vertex, &non_finite))) return rc;
                    finite = non_finite == 0;
                }
                nb[d].ext = pt_box_extent(nb[d].vertex);
            } else {
                nb[d].ext = pt_mesh_vertex_box(df.positions, pl.n_verts, &nb[d].vertex);
                for (uint64_t v = 0; v < 3 * (uint64_t)pl.n_verts; v++) finite = finite && std::isfinite(df.positions[v]);
            }
            nb[d].padded = nb[d].vertex;
            pt_pad_mesh_box(&nb[d].padded, nb[d].ext);
            for (int k = 0; k < 3; k++) finite = finite && nb[d].padded.lo[k] >= -PT_BOX_LIMIT && nb[d].padded.hi[k] <= PT_BOX_LIMIT;
            if (!finite) return pt_fail(c, PT_ERR_ARGUMENT, at + "a coordinate is not finite or the mesh's box reaches beyond +-1e18");
            mesh_box[df.mesh] = nb[d].padded;
        }
    }
    PtUpdatePlan plan;
    int rc = pt_update_prepare(c, mo, kd, mesh_box, plan);
    if (rc) return rc;
    if (n_deforms == 0) return pt_update_commit(c, mo, plan);

    // ---- writes
    PT_HIP(c, hipSetDevice(c->device));
    PT_HIP(c, hipDeviceSynchronize());
    c->have_scene = false;  // until every write has been made (pt_update_commit sets it again)
    const bool verbose = getenv("PORTRAYER_VERBOSE") != nullptr;
    if (!res.indices_resident) {
        if ((rc = pt_upload(c, c->mesh_idx, res.indices))) return rc;
        res.indices_resident = true;
    }
    bool any_refit = false;
    size_t stage_bytes = 0;
    for (uint32_t d = 0; d < n_deforms; d++) {
        any_refit = any_refit || !items[d].rebuild;
        stage_bytes = std::max(stage_bytes, (size_t)res.place[items[d].mesh].n_verts * 24 * (items[d].normals ? 2 : 1));
    }
    if (!on_device && (rc = pt_reserve(c, c->deform_stage, stage_bytes))) return rc;  // (vertices in device memory are read where they are)
    if (any_refit && ((rc = pt_reserve(c, c->tree_parent, std::max<size_t>(res.tree_nodes, 1) * 4)) || (rc = pt_reserve(c, c->tree_arrive, std::max<size_t>(res.tree_nodes, 1) * 4)))) return rc;
    const bool write_normals = res.any_normals;  // (tri_n is empty unless a node shades smoothly: the upload then drops the normals it is given, and so does this)
    for (uint32_t d = 0; d < n_deforms; d++) {
        const PtDeformItem& df = items[d];
        pt_context::Resident::MeshPlace& pl = res.place[df.mesh];
        PtMeshInfo& mi = res.meshes[df.mesh];
        const size_t pos_bytes = (size_t)pl.n_verts * 24;
        const double *d_pos = df.positions, *d_nrm = df.normals && write_normals ? df.normals : nullptr;
        if (!on_device) {
            PT_HIP(c, hipMemcpy(c->deform_stage.p, df.positions, pos_bytes, hipMemcpyHostToDevice));
            if (df.normals) PT_HIP(c, hipMemcpy((char*)c->deform_stage.p + pos_bytes, df.normals, pos_bytes, hipMemcpyHostToDevice));
            d_pos = (const double*)c->deform_stage.p;
            if (d_nrm) d_nrm = (const double*)((const char*)c->deform_stage.p + pos_bytes);
        }
        PT_HIP(c, pt_device_expand_mesh((const uint32_t*)c->mesh_idx.p, mi.tri_first, mi.tri_count, d_pos, d_nrm, pl.n_verts, (double*)c->tri_v.p, (double*)c->tri_e.p,
                                        d_nrm ? (double*)c->tri_n.p : nullptr, nullptr));
        const double pad = pt_triangle_pad(nb[d].ext);
        if (df.rebuild) {
            PtDeviceBuildResult built;
            if ((rc = pt_build_mesh_tree_in_place(c, pl, mi, nb[d].vertex.lo, nb[d].vertex.hi, pad, &built))) return rc;
            if (verbose) fprintf(stderr, "[pt_scene_deform] mesh %u rebuilt: %u triangles, %.2f ms, %d clustering rounds, depth %d\n", df.mesh, mi.tri_count, built.ms, built.rounds, built.depth);
        } else if (pl.node_count) {
            if (!pl.parents_valid) {
                PT_HIP(c, pt_device_tree_parents((const PtBvhNode*)c->bvh.p, pl.node_first, pl.node_count, (uint32_t*)c->tree_parent.p, nullptr));
                pl.parents_valid = true;
            }
            PT_HIP(c, pt_device_refit_mesh_tree((PtBvhNode*)c->bvh.p, pl.node_first, pl.node_count, (const uint32_t*)c->bvh_items.p, pl.item_first, pl.item_count,
                                                (const double*)c->tri_v.p, mi.tri_first, mi.tri_count, pad, (const uint32_t*)c->tree_parent.p, (uint32_t*)c->tree_arrive.p, nullptr));
        }
        // what the walks read, for the mesh's node and item ranges alone
        if ((rc = pt_queue_collapse4(c, pl.node_first, (size_t)pl.node_first + pl.node_count)) || (rc = pt_queue_tri_leaf(c, pl.item_first, pl.item_count))) return rc;
        for (int r = 0; r < 12; r++) mi.bbox_inv[r] = df.bounds_invtrans[r];
        res.mesh_box[df.mesh] = nb[d].padded;
        PT_HIP(c, hipStreamSynchronize(nullptr));  // the staging buffer is the next mesh's
    }
    {   // the records the walks and the scene-level build read: PtMeshInfo (bbox_inv, blas_root), the padded boxes; the stack under a scene leaf
        if ((rc = pt_upload(c, c->meshes, res.meshes)) || (rc = pt_upload_mesh_boxes(c, res.mesh_box))) return rc;
        res.below = pt_stack_below(res);
    }
    return pt_update_commit(c, mo, plan);
}

extern "C" int pt_scene_deform(pt_context* c, uint32_t n_deforms, const pt_mesh_deform* deforms, const pt_scene_motion* mo, const pt_kdtree* kd) {
    if (!c || !mo || (n_deforms && !deforms)) return PT_ERR_ARGUMENT;
    std::vector<PtDeformItem> items(n_deforms);
    for (uint32_t d = 0; d < n_deforms; d++) items[d] = PtDeformItem{deforms[d].mesh, deforms[d].positions, deforms[d].normals, deforms[d].bounds_invtrans, deforms[d].rebuild};
    return pt_deform_meshes(c, items, false, mo, kd);
}

extern "C" int pt_scene_deform_device(pt_context* c, uint32_t n_deforms, const pt_mesh_deform_device* deforms, const pt_scene_motion* mo, const pt_kdtree* kd) {
    if (!c || !mo || (n_deforms && !deforms)) return PT_ERR_ARGUMENT;
    std::vector<PtDeformItem> items(n_deforms);
    for (uint32_t d = 0; d < n_deforms; d++) items[d] = PtDeformItem{deforms[d].mesh, deforms[d].d_positions, deforms[d].d_normals, deforms[d].bounds_invtrans, deforms[d].rebuild};
    return pt_deform_meshes(c, items, true, mo, kd);
}

extern "C" int pt_scene_mesh_rebuildable(const pt_context* c, uint32_t mesh) {
    if (!c) return PT_ERR_ARGUMENT;
    if (!c->have_scene) return PT_ERR_NO_SCENE;
    if (mesh >= c->res.place.size()) return PT_ERR_ARGUMENT;
    return c->res.place[mesh].device_built ? 1 : 0;
}

// tests: the bytes of device memory the context's scene buffers hold (an update must not make it grow)
extern "C" uint64_t pt_test_scene_bytes(const pt_context* c) {
    if (!c) return 0;
    const PtBuf* bufs[] = {&c->inv, &c->fwd, &c->nrm, &c->info, &c->tri_v, &c->tri_e, &c->tri_leaf, &c->tri_n, &c->meshes, &c->materials, &c->lights, &c->bvh, &c->bvh4,
                           &c->bvh_items, &c->kd, &c->kd_items, &c->mat_maps, &c->uv_trans, &c->tex, &c->tex_rgb, &c->srgb_lut, &c->tri_uv, &c->texview, &c->mkd, &c->mkd_items,
                           &c->node_box, &c->kd_box, &c->mkd_box, &c->mkd_item_box, &c->kd_ref, &c->g_inv, &c->g_fwd, &c->g_nrm, &c->chain_off, &c->chain, &c->dfs_rank,
                           &c->hier_rec, &c->own_inv, &c->mesh_box_dev, &c->mesh_idx, &c->tree_parent, &c->tree_arrive, &c->deform_stage};
    uint64_t total = 0;
    for (const PtBuf* b : bufs) total += b->bytes;
    return total;
}

extern "C" int pt_test_vertex_box_shape(const pt_context* c, uint64_t out[2]) {
    if (!c || !out) return PT_ERR_ARGUMENT;
    out[0] = PT_VBOX_BLOCK; out[1] = pt_vertex_box_partials(c->n_cu);
    return PT_OK;
}

// tests: out[0] = stack_cap, out[1] = who built the scene-level tree last (0 the upload, 1 an update on the host, 2 an update on the device),
// out[2] = the device build's clustering rounds, out[3] = bytes of the tree buffers (bvh, bvh4, bvh_items)
extern "C" int pt_test_scene_info(const pt_context* c, uint64_t out[4]) {
    if (!c || !out) return PT_ERR_ARGUMENT;
    if (!c->have_scene) return PT_ERR_NO_SCENE;
    out[0] = (uint64_t)c->view.stack_cap; out[1] = (uint64_t)c->res.last_builder; out[2] = (uint64_t)c->res.last_rounds;
    out[3] = c->bvh.bytes + c->bvh4.bytes + c->bvh_items.bytes;
    return PT_OK;
}

