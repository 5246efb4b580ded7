// Device-side build of mesh triangle trees: see pt_build.h.
//
// Parallel locally-ordered clustering (Meister & Bittner, "Parallel Locally-Ordered Clustering for
// Bounding Volume Hierarchy Construction", 2018), bottom-up:
//
//   1. pt_ploc_prepare  per triangle: f64 bounds -> f32 box rounded outward, 63-bit Morton code of the box centre
//   2. rocprim radix sort (key = Morton code, value = triangle) -- library call; sorting is not this path's subject
//   3. repeat until one cluster is left (the clusters stay in Morton order):
//        pt_ploc_nearest  every cluster looks PT_PLOC_RADIUS places to either side for the neighbour whose union
//                         with it has the smallest surface area
//        pt_ploc_merge    clusters that chose each other merge: the lower one becomes the new node (written in the
//                         walk's format: two child boxes + two references), the upper one retires; a node whose
//                         children together hold <= max_leaf triangles becomes a leaf instead
//        rocprim exclusive scan + pt_ploc_compact: close the gaps
//   4. pt_ploc_depth    longest root-to-leaf path (the walk's LDS stack is sized from it)
//
// (A Morton-order tree a la Karras 2012 was measured first: 8.4 ms for 1.25 M triangles but 31 % slower to
// walk than the host's binned-SAH tree, and replacing its upper levels by a host-built SAH tree over
// "treelets" showed the loss sits in the LOWER levels: 2.42 Gray/s with 16-triangle treelets, 1.99 with
// 256, 1.90 without, against 2.74 for the host tree.)
#include "pt_build.h"

#include "../../include/portrayer_hip.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#define PT_BUILD_BLOCK 256
#define PT_PLOC_LEAF 0x80000000u
#define PT_PLOC_NONE 0xFFFFFFFFu
#define PT_PLOC_LIMIT 1e18f  // pt_bvh.h PT_BOX_LIMIT: box coordinates stay finite and within +-1e18
#define PT_PLOC_RADIUS 16

namespace {

__device__ __forceinline__ float pt_box_lo(double v) {
    if (!(v > -1e18)) return -PT_PLOC_LIMIT;  // also NaN
    if (v > 1e18) return PT_PLOC_LIMIT;
    return __double2float_rd(v);
}
__device__ __forceinline__ float pt_box_hi(double v) {
    if (!(v < 1e18)) return PT_PLOC_LIMIT;
    if (v < -1e18) return -PT_PLOC_LIMIT;
    return __double2float_ru(v);
}

__device__ __forceinline__ unsigned long long pt_spread21(unsigned long long x) {  // bit i -> bit 3 i
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__device__ __forceinline__ unsigned long long pt_quantise21(double c, double lo, double inv_ext) {
    double u = (c - lo) * inv_ext * 2097152.0;
    if (!(u > 0.0)) return 0ull;
    if (u >= 2097151.0) return 2097151ull;
    return (unsigned long long)u;
}

struct PtBox6 {
    float v[6];  // lo xyz, hi xyz
};

__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_ploc_prepare(const double* __restrict__ tri_v, uint32_t tri_first, uint32_t n,
                                                                 double lx, double ly, double lz, double ix, double iy, double iz, double pad,
                                                                 unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                 PtBox6* __restrict__ tri_box) {
    uint32_t t = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (t >= n) return;
    const double* v = tri_v + 9 * (size_t)(tri_first + t);
    double lo[3], hi[3];
    PtBox6 b;
    for (int k = 0; k < 3; k++) {
        double a = v[k], bb = v[3 + k], c = v[6 + k];
        lo[k] = fmin(fmin(a, bb), c);
        hi[k] = fmax(fmax(a, bb), c);
        b.v[k] = pt_box_lo(lo[k] - pad);
        b.v[3 + k] = pt_box_hi(hi[k] + pad);
    }
    tri_box[t] = b;
    unsigned long long qx = pt_quantise21(0.5 * (lo[0] + hi[0]), lx, ix);
    unsigned long long qy = pt_quantise21(0.5 * (lo[1] + hi[1]), ly, iy);
    unsigned long long qz = pt_quantise21(0.5 * (lo[2] + hi[2]), lz, iz);
    keys[t] = (pt_spread21(qx) << 2) | (pt_spread21(qy) << 1) | pt_spread21(qz);
    vals[t] = t;
}

// the clusters of the first round: the triangles in Morton order
__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_ploc_init(uint32_t n, const uint32_t* __restrict__ vals, const PtBox6* __restrict__ tri_box,
                                                              uint32_t tri_first, uint32_t* __restrict__ items, uint32_t* __restrict__ cid,
                                                              PtBox6* __restrict__ cbox) {
    uint32_t k = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (k >= n) return;
    items[k] = tri_first + vals[k];
    cid[k] = k | PT_PLOC_LEAF;
    cbox[k] = tri_box[vals[k]];
}

__device__ __forceinline__ float pt_union_area(const PtBox6& a, const PtBox6& b) {
    float dx = fmaxf(a.v[3], b.v[3]) - fminf(a.v[0], b.v[0]);
    float dy = fmaxf(a.v[4], b.v[4]) - fminf(a.v[1], b.v[1]);
    float dz = fmaxf(a.v[5], b.v[5]) - fminf(a.v[2], b.v[2]);
    return dx * dy + dy * dz + dz * dx;
}

__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_ploc_nearest(uint32_t m, int radius, const PtBox6* __restrict__ cbox, uint32_t* __restrict__ nearest) {
    uint32_t i = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (i >= m) return;
    const PtBox6 me = cbox[i];
    int lo = (int)i - radius, hi = (int)i + radius;
    if (lo < 0) lo = 0;
    if (hi > (int)m - 1) hi = (int)m - 1;
    float best = INFINITY;
    uint32_t best_j = i;
    for (int j = lo; j <= hi; j++) {
        if (j == (int)i) continue;
        float a = pt_union_area(me, cbox[j]);
        if (a < best || best_j == i) { best = a; best_j = (uint32_t)j; }  // the first of equal areas; any j if every area is NaN / inf
    }
    nearest[i] = best_j;
}

struct PtPlocOut {  // everything pt_ploc_merge writes for the finished tree
    PtBvhNode* nodes;       // d_nodes + node_base
    uint32_t* items;        // d_items + item_base: [0, n) single triangles in Morton order, then max_leaf slots per node
    uint32_t* leaf_count;   // per node: triangles if the node was turned into a leaf, else 0
    uint32_t* node_parent;  // per node
    uint32_t* leaf_parent;  // per sorted triangle
    uint32_t* counter;      // next free node
    uint32_t node_base, item_base, n;
    int max_leaf;
};

// number of triangles if `id` is a leaf of the final tree (a triangle or a collapsed node), else 0; *first = its items
__device__ __forceinline__ uint32_t pt_ploc_leaf_items(const PtPlocOut& o, uint32_t id, uint32_t* first) {
    if (id & PT_PLOC_LEAF) { *first = id & ~PT_PLOC_LEAF; return 1u; }
    uint32_t c = o.leaf_count[id];
    *first = o.n + (uint32_t)o.max_leaf * id;
    return c;
}
__device__ __forceinline__ uint32_t pt_ploc_ref(const PtPlocOut& o, uint32_t id) {
    uint32_t first, c = pt_ploc_leaf_items(o, id, &first);
    return c ? (PT_REF_LEAF | ((o.item_base + first) << 3) | (c - 1u)) : o.node_base + id;
}

__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_ploc_merge(uint32_t m, const uint32_t* __restrict__ nearest, const uint32_t* __restrict__ cid,
                                                               const PtBox6* __restrict__ cbox, uint32_t* __restrict__ cid_out,
                                                               PtBox6* __restrict__ cbox_out, uint32_t* __restrict__ keep, PtPlocOut o) {
    uint32_t i = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (i >= m) return;
    uint32_t j = nearest[i];
    bool mutual = j != i && nearest[j] == i;
    if (!mutual) { cid_out[i] = cid[i]; cbox_out[i] = cbox[i]; keep[i] = 1u; return; }
    if (i > j) { keep[i] = 0u; return; }
    const uint32_t a = cid[i], b = cid[j];
    const PtBox6 ba = cbox[i], bb = cbox[j];
    const uint32_t node = atomicAdd(o.counter, 1u);
    uint32_t fa, fb, ca = pt_ploc_leaf_items(o, a, &fa), cb = pt_ploc_leaf_items(o, b, &fb);
    if (ca && cb && ca + cb <= (uint32_t)o.max_leaf) {  // a leaf of ca + cb triangles: gather them in the node's own slot
        uint32_t dst = o.n + (uint32_t)o.max_leaf * node;
        for (uint32_t k = 0; k < ca; k++) o.items[dst + k] = o.items[fa + k];
        for (uint32_t k = 0; k < cb; k++) o.items[dst + ca + k] = o.items[fb + k];
        o.leaf_count[node] = ca + cb;
    } else {
        PtBvhNode nd;
        for (int k = 0; k < 3; k++) { nd.lo[k][0] = ba.v[k]; nd.hi[k][0] = ba.v[3 + k]; nd.lo[k][1] = bb.v[k]; nd.hi[k][1] = bb.v[3 + k]; }
        nd.child0 = pt_ploc_ref(o, a);
        nd.child1 = pt_ploc_ref(o, b);
        nd.pad[0] = nd.pad[1] = 0u;
        o.nodes[node] = nd;
        o.leaf_count[node] = 0u;
    }
    if (a & PT_PLOC_LEAF) o.leaf_parent[a & ~PT_PLOC_LEAF] = node; else o.node_parent[a] = node;
    if (b & PT_PLOC_LEAF) o.leaf_parent[b & ~PT_PLOC_LEAF] = node; else o.node_parent[b] = node;
    o.node_parent[node] = PT_PLOC_NONE;
    PtBox6 u;
    for (int k = 0; k < 3; k++) { u.v[k] = fminf(ba.v[k], bb.v[k]); u.v[3 + k] = fmaxf(ba.v[3 + k], bb.v[3 + k]); }
    cid_out[i] = node;
    cbox_out[i] = u;
    keep[i] = 1u;
}

__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_ploc_compact(uint32_t m, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos,
                                                                 const uint32_t* __restrict__ cid_in, const PtBox6* __restrict__ cbox_in,
                                                                 uint32_t* __restrict__ cid, PtBox6* __restrict__ cbox, uint32_t* __restrict__ m_out) {
    uint32_t i = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (i >= m) return;
    if (keep[i]) { cid[pos[i]] = cid_in[i]; cbox[pos[i]] = cbox_in[i]; }
    if (i == m - 1) *m_out = pos[i] + keep[i];
}

// inner nodes on the path from a triangle to the root, + 1
__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_ploc_depth(uint32_t n, const uint32_t* __restrict__ node_parent, const uint32_t* __restrict__ leaf_parent,
                                                               const uint32_t* __restrict__ leaf_count, int* depth) {
    uint32_t k = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    int d = 0;
    if (k < n) {
        d = 1;
        for (uint32_t p = leaf_parent[k]; p != PT_PLOC_NONE; p = node_parent[p]) d += leaf_count[p] ? 0 : 1;
    }
    for (int o = 32; o > 0; o >>= 1) d = max(d, __shfl_xor(d, o));
    if ((threadIdx.x & 63) == 0) atomicMax(depth, d);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// The same clustering over BOXES instead of triangles: the scene-level tree of pt_scene_update (pt_build.h).
// Its leaves are the flattened nodes themselves, named by the leaf reference (PT_REF_LEAF | node << 3, "direct":
// pt_bvh.h), so nothing goes into the items array and a node is never turned into a multi-item leaf. The triangle
// path above is left as it is; pt_ploc_nearest, pt_ploc_compact and pt_ploc_depth serve both.
// ------------------------------------------------------------------------------------------------
namespace {

// Conservative world box of every flattened node, with pt_scene_upload's formulas and paddings (pt_scene.hip: pt_node_world_boxes): the exact box of
// a sphere, the two discs of a cylinder / cone, the transformed padded model box otherwise, a relative pad of 1e-9 on the result; f64, then
// rounded outward to f32. The device's f64 may differ from the host's in the last bits (sqrt, the order of min / max): the 1e-4 model-unit
// padding of every shape dominates that by many orders of magnitude, so the boxes stay conservative and no bit equality with the host's is sought.
__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_node_box_kernel(uint32_t n, const double* __restrict__ fwd, const uint32_t* __restrict__ info,
                                                                    const double* __restrict__ mesh_box, const double* __restrict__ tri_v,
                                                                    PtBox6* __restrict__ out) {
    uint32_t i = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (i >= n) return;
    double M[12];
    for (int k = 0; k < 12; k++) M[k] = fwd[12 * (size_t)i + k];
    const int t = (int)info[4 * (size_t)i];
    const uint32_t data = info[4 * (size_t)i + 1];
    double blo[3], bhi[3], lo[3], hi[3];
    bool boxed = false;
    if (t == PT_PRIM_SPHERE) {
        for (int r = 0; r < 3; r++) {
            double e = 1.0001 * sqrt(M[4 * r] * M[4 * r] + M[4 * r + 1] * M[4 * r + 1] + M[4 * r + 2] * M[4 * r + 2]);
            blo[r] = M[4 * r + 3] - e; bhi[r] = M[4 * r + 3] + e;
        }
        boxed = true;
    } else if (t == PT_PRIM_CYLINDER || t == PT_PRIM_CONE) {  // discs in the model xz-plane at y = +-0.5001
        const double top = t == PT_PRIM_CONE ? 1e-4 : 0.5001;
        for (int r = 0; r < 3; r++) {
            double s = sqrt(M[4 * r] * M[4 * r] + M[4 * r + 2] * M[4 * r + 2]);
            double c0 = M[4 * r + 1] * 0.5001 + M[4 * r + 3], e0 = top * s;
            double c1 = M[4 * r + 1] * -0.5001 + M[4 * r + 3], e1 = 0.5001 * s;
            blo[r] = fmin(fmin(INFINITY, c0 - e0), c1 - e1); bhi[r] = fmax(fmax(-INFINITY, c0 + e0), c1 + e1);
        }
        boxed = true;
    } else if (t == PT_PRIM_PLANE) {
        lo[0] = lo[2] = -0.5001; hi[0] = hi[2] = 0.5001; lo[1] = -1e-4; hi[1] = 1e-4;
    } else if (t == PT_PRIM_MESH || t == PT_PRIM_KDMESH) {  // the mesh's padded model box
        for (int k = 0; k < 3; k++) { lo[k] = mesh_box[6 * (size_t)data + k]; hi[k] = mesh_box[6 * (size_t)data + 3 + k]; }
    } else if (t == PT_PRIM_TRIANGLE) {
        const double* v = tri_v + 9 * (size_t)data;
        double ext = 1e-30;
        for (int k = 0; k < 3; k++) {
            lo[k] = fmin(v[k], fmin(v[3 + k], v[6 + k])); hi[k] = fmax(v[k], fmax(v[3 + k], v[6 + k]));
            ext = fmax(ext, hi[k] - lo[k]);
        }
        for (int k = 0; k < 3; k++) { lo[k] -= 1e-6 * ext; hi[k] += 1e-6 * ext; }
    } else {  // cube
        lo[0] = lo[1] = lo[2] = -0.5001; hi[0] = hi[1] = hi[2] = 0.5001;
    }
    if (!boxed) {
        for (int r = 0; r < 3; r++) { blo[r] = INFINITY; bhi[r] = -INFINITY; }
        for (int c = 0; c < 8; c++) {
            double x = (c & 4) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 1) ? hi[2] : lo[2];
            for (int r = 0; r < 3; r++) {
                double v = M[4 * r] * x + M[4 * r + 1] * y + M[4 * r + 2] * z + M[4 * r + 3];
                blo[r] = fmin(blo[r], v); bhi[r] = fmax(bhi[r], v);
            }
        }
    }
    PtBox6 b;
    for (int k = 0; k < 3; k++) {
        double mag = fmax(fabs(blo[k]), fabs(bhi[k]));
        double pad = 1e-9 * fmax(bhi[k] - blo[k], mag) + 1e-300;
        b.v[k] = pt_box_lo(blo[k] - pad);
        b.v[3 + k] = pt_box_hi(bhi[k] + pad);
    }
    out[i] = b;
}

// Morton code of every box centre inside the root box
__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_ploc_prepare_boxes(const PtBox6* __restrict__ box, uint32_t n, double lx, double ly, double lz,
                                                                       double ix, double iy, double iz, unsigned long long* __restrict__ keys,
                                                                       uint32_t* __restrict__ vals) {
    uint32_t t = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (t >= n) return;
    const PtBox6 b = box[t];
    unsigned long long qx = pt_quantise21(0.5 * ((double)b.v[0] + (double)b.v[3]), lx, ix);
    unsigned long long qy = pt_quantise21(0.5 * ((double)b.v[1] + (double)b.v[4]), ly, iy);
    unsigned long long qz = pt_quantise21(0.5 * ((double)b.v[2] + (double)b.v[5]), lz, iz);
    keys[t] = (pt_spread21(qx) << 2) | (pt_spread21(qy) << 1) | pt_spread21(qz);
    vals[t] = t;
}

// the clusters of the first round: the boxes in Morton order; leaf_item[k] = the flattened node behind sorted place k
__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_ploc_init_boxes(uint32_t n, const uint32_t* __restrict__ vals, const PtBox6* __restrict__ box,
                                                                    uint32_t* __restrict__ leaf_item, uint32_t* __restrict__ cid, PtBox6* __restrict__ cbox) {
    uint32_t k = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (k >= n) return;
    leaf_item[k] = vals[k];
    cid[k] = k | PT_PLOC_LEAF;
    cbox[k] = box[vals[k]];
}

struct PtPlocDirectOut {
    PtBvhNode* nodes;           // d_nodes + node_base: n - 1 of them
    const uint32_t* leaf_item;  // per sorted place: the item its leaf names
    uint32_t* leaf_count;       // per node: 0 (pt_ploc_depth counts every node as an inner one)
    uint32_t* node_parent;
    uint32_t* leaf_parent;
    uint32_t* counter;
    uint32_t node_base;
};

__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_ploc_merge_direct(uint32_t m, const uint32_t* __restrict__ nearest, const uint32_t* __restrict__ cid,
                                                                      const PtBox6* __restrict__ cbox, uint32_t* __restrict__ cid_out,
                                                                      PtBox6* __restrict__ cbox_out, uint32_t* __restrict__ keep, PtPlocDirectOut o) {
    uint32_t i = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (i >= m) return;
    uint32_t j = nearest[i];
    bool mutual = j != i && nearest[j] == i;
    if (!mutual) { cid_out[i] = cid[i]; cbox_out[i] = cbox[i]; keep[i] = 1u; return; }
    if (i > j) { keep[i] = 0u; return; }
    const uint32_t a = cid[i], b = cid[j];
    const PtBox6 ba = cbox[i], bb = cbox[j];
    const uint32_t node = atomicAdd(o.counter, 1u);
    PtBvhNode nd;
    for (int k = 0; k < 3; k++) { nd.lo[k][0] = ba.v[k]; nd.hi[k][0] = ba.v[3 + k]; nd.lo[k][1] = bb.v[k]; nd.hi[k][1] = bb.v[3 + k]; }
    nd.child0 = (a & PT_PLOC_LEAF) ? (PT_REF_LEAF | (o.leaf_item[a & ~PT_PLOC_LEAF] << 3)) : o.node_base + a;
    nd.child1 = (b & PT_PLOC_LEAF) ? (PT_REF_LEAF | (o.leaf_item[b & ~PT_PLOC_LEAF] << 3)) : o.node_base + b;
    nd.pad[0] = nd.pad[1] = 0u;
    o.nodes[node] = nd;
    o.leaf_count[node] = 0u;
    if (a & PT_PLOC_LEAF) o.leaf_parent[a & ~PT_PLOC_LEAF] = node; else o.node_parent[a] = node;
    if (b & PT_PLOC_LEAF) o.leaf_parent[b & ~PT_PLOC_LEAF] = node; else o.node_parent[b] = node;
    o.node_parent[node] = PT_PLOC_NONE;
    PtBox6 u;
    for (int k = 0; k < 3; k++) { u.v[k] = fminf(ba.v[k], bb.v[k]); u.v[3 + k] = fmaxf(ba.v[3 + k], bb.v[3 + k]); }
    cid_out[i] = node;
    cbox_out[i] = u;
    keep[i] = 1u;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// The host side of a build, shared by both: temporaries, sort, the clustering rounds, depth, read-back. What differs - the kernels that key the
// leaves (`prepare`), seed the first round's clusters from the sorted order (`init`) and merge (`merge`) - is passed in.
// ------------------------------------------------------------------------------------------------
namespace {

struct PtPlocWork {  // every temporary of a build, in one allocation
    unsigned long long *keys_in, *keys;
    uint32_t *vals_in, *vals;
    PtBox6* leaf_box;   // per leaf (triangle / scene node), in input order
    PtBox6* cbox[3];    // clusters: current, merged (with gaps), next
    uint32_t* cid[3];
    uint32_t *nearest, *keep, *pos, *leaf_count, *node_parent, *leaf_parent, *leaf_item;
    uint32_t* scalars;  // [0] next node, [1] clusters left, [2] depth
};

struct PtPlocHold {  // what a build must give back however it ends
    char* base = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~PtPlocHold() {
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
        if (base) hipFree(base);
    }
};

#define PT_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

template <class Prepare, class Init, class Merge>
hipError_t pt_ploc_build(uint32_t n, hipStream_t stream, Prepare prepare, Init init, Merge merge, PtDeviceBuildResult* out, uint32_t* root) {
    PtPlocHold hold;
    size_t sort_bytes = 0, scan_bytes = 0;
    PT_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr,
                                     (uint32_t*)nullptr, (size_t)n, 0u, 63u, stream));
    PT_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream));
    const size_t tmp_bytes = std::max(sort_bytes, scan_bytes);
    // one allocation for every temporary, freed before the call returns
    const size_t need = 8192 + tmp_bytes + (size_t)n * (8 + 8 + 4 + 4 + 24 + 3 * 24 + 3 * 4 + 7 * 4);
    PT_TRY(hipMalloc((void**)&hold.base, need));
    size_t used = 0;
    auto take = [&](size_t bytes) { used = (used + 255) & ~(size_t)255; char* p = hold.base + used; used += bytes; return (void*)p; };
    PtPlocWork w;
    w.keys_in = (unsigned long long*)take(8 * (size_t)n); w.keys = (unsigned long long*)take(8 * (size_t)n);
    w.vals_in = (uint32_t*)take(4 * (size_t)n); w.vals = (uint32_t*)take(4 * (size_t)n);
    w.leaf_box = (PtBox6*)take(sizeof(PtBox6) * (size_t)n);
    for (int k = 0; k < 3; k++) w.cbox[k] = (PtBox6*)take(sizeof(PtBox6) * (size_t)n);
    for (int k = 0; k < 3; k++) w.cid[k] = (uint32_t*)take(4 * (size_t)n);
    uint32_t** per_leaf[] = {&w.nearest, &w.keep, &w.pos, &w.leaf_count, &w.node_parent, &w.leaf_parent, &w.leaf_item};
    for (uint32_t** p : per_leaf) *p = (uint32_t*)take(4 * (size_t)n);
    w.scalars = (uint32_t*)take(16);
    void* tmp = take(tmp_bytes);
    if (used > need) return hipErrorOutOfMemory;

    int radius = PT_PLOC_RADIUS;
    if (const char* e = getenv("PORTRAYER_PLOC_RADIUS")) radius = std::min(std::max(atoi(e), 1), 128);

    PT_TRY(hipEventCreate(&hold.e0));
    PT_TRY(hipEventCreate(&hold.e1));
    PT_TRY(hipEventRecord(hold.e0, stream));
    auto blocks = [](uint32_t count) { return dim3((count + PT_BUILD_BLOCK - 1) / PT_BUILD_BLOCK); };
    PT_TRY(hipMemsetAsync(w.scalars, 0, 16, stream));
    prepare(w);
    PT_TRY(hipGetLastError());
    PT_TRY(rocprim::radix_sort_pairs(tmp, sort_bytes, w.keys_in, w.keys, w.vals_in, w.vals, (size_t)n, 0u, 63u, stream));
    init(w);
    PT_TRY(hipGetLastError());

    uint32_t m = n;
    int rounds = 0;
    while (m > 1) {
        if (++rounds > 4096) return hipErrorLaunchFailure;  // every round merges at least the closest pair
        hipLaunchKernelGGL(pt_ploc_nearest, blocks(m), dim3(PT_BUILD_BLOCK), 0, stream, m, radius, w.cbox[0], w.nearest);
        merge(w, m);
        PT_TRY(hipGetLastError());
        PT_TRY(rocprim::exclusive_scan(tmp, scan_bytes, w.keep, w.pos, 0u, (size_t)m, rocprim::plus<uint32_t>(), stream));
        hipLaunchKernelGGL(pt_ploc_compact, blocks(m), dim3(PT_BUILD_BLOCK), 0, stream, m, w.keep, w.pos, w.cid[1], w.cbox[1], w.cid[2], w.cbox[2], w.scalars + 1);
        PT_TRY(hipGetLastError());
        uint32_t left = m;
        PT_TRY(hipMemcpyAsync(&left, w.scalars + 1, 4, hipMemcpyDeviceToHost, stream));
        PT_TRY(hipStreamSynchronize(stream));
        if (left == 0 || left >= m) return hipErrorLaunchFailure;  // (keeps the next round's launches inside the arrays whatever the device answered)
        m = left;
        std::swap(w.cid[0], w.cid[2]);
        std::swap(w.cbox[0], w.cbox[2]);
    }
    hipLaunchKernelGGL(pt_ploc_depth, blocks(n), dim3(PT_BUILD_BLOCK), 0, stream, n, w.node_parent, w.leaf_parent, w.leaf_count, (int*)(w.scalars + 2));
    PT_TRY(hipGetLastError());
    PT_TRY(hipEventRecord(hold.e1, stream));
    uint32_t h[3] = {0, 0, 0};
    *root = 0;
    PT_TRY(hipMemcpyAsync(h, w.scalars, 12, hipMemcpyDeviceToHost, stream));
    PT_TRY(hipMemcpyAsync(root, w.cid[0], 4, hipMemcpyDeviceToHost, stream));
    PT_TRY(hipStreamSynchronize(stream));
    float ms = 0.0f;
    PT_TRY(hipEventElapsedTime(&ms, hold.e0, hold.e1));
    if (h[0] != n - 1 || (*root & PT_PLOC_LEAF) || *root >= n - 1) return hipErrorLaunchFailure;  // a binary tree over n leaves has n - 1 nodes
    out->depth = (int)h[2];
    out->ms = ms;
    out->rounds = rounds;
    return hipSuccess;
}

}  // namespace

hipError_t pt_device_build_mesh_tree(const double* d_tri_v, uint32_t tri_first, uint32_t n, const double lo[3], const double hi[3], double pad, int max_leaf,
                                     PtBvhNode* d_nodes, uint32_t node_base, uint32_t* d_items, uint32_t item_base, hipStream_t stream,
                                     PtDeviceBuildResult* out) {
    if (n < 2 || max_leaf < 1 || max_leaf > 8 || n <= (uint32_t)max_leaf) return hipErrorInvalidValue;
    double inv[3];
    for (int k = 0; k < 3; k++) inv[k] = hi[k] > lo[k] ? 1.0 / (hi[k] - lo[k]) : 0.0;
    const dim3 grid((n + PT_BUILD_BLOCK - 1) / PT_BUILD_BLOCK), block(PT_BUILD_BLOCK);
    uint32_t root = 0;
    hipError_t e = pt_ploc_build(
        n, stream,
        [&](PtPlocWork& w) {
            hipLaunchKernelGGL(pt_ploc_prepare, grid, block, 0, stream, d_tri_v, tri_first, n, lo[0], lo[1], lo[2], inv[0], inv[1], inv[2], pad, w.keys_in, w.vals_in, w.leaf_box);
        },
        [&](PtPlocWork& w) { hipLaunchKernelGGL(pt_ploc_init, grid, block, 0, stream, n, w.vals, w.leaf_box, tri_first, d_items + item_base, w.cid[0], w.cbox[0]); },
        [&](PtPlocWork& w, uint32_t m) {
            PtPlocOut o;
            o.nodes = d_nodes + node_base; o.items = d_items + item_base; o.leaf_count = w.leaf_count; o.node_parent = w.node_parent; o.leaf_parent = w.leaf_parent;
            o.counter = w.scalars; o.node_base = node_base; o.item_base = item_base; o.n = n; o.max_leaf = max_leaf;
            hipLaunchKernelGGL(pt_ploc_merge, dim3((m + PT_BUILD_BLOCK - 1) / PT_BUILD_BLOCK), block, 0, stream, m, w.nearest, w.cid[0], w.cbox[0], w.cid[1], w.cbox[1], w.keep, o);
        },
        out, &root);
    if (e != hipSuccess) return e;
    out->root = node_base + root;  // n > max_leaf: the root is never a leaf
    return hipSuccess;
}

hipError_t pt_device_build_scene_tree(uint32_t n, const double* d_fwd, const uint32_t* d_info, const double* d_mesh_box, const double* d_tri_v,
                                      const double lo[3], const double hi[3], PtBvhNode* d_nodes, uint32_t node_base, hipStream_t stream,
                                      PtDeviceBuildResult* out) {
    if (n < 2 || n >= (1u << 28)) return hipErrorInvalidValue;  // a direct leaf reference holds its node in 28 bits
    double inv[3];
    for (int k = 0; k < 3; k++) inv[k] = hi[k] > lo[k] ? 1.0 / (hi[k] - lo[k]) : 0.0;
    const dim3 grid((n + PT_BUILD_BLOCK - 1) / PT_BUILD_BLOCK), block(PT_BUILD_BLOCK);
    uint32_t root = 0;
    hipError_t e = pt_ploc_build(
        n, stream,
        [&](PtPlocWork& w) {
            hipLaunchKernelGGL(pt_node_box_kernel, grid, block, 0, stream, n, d_fwd, d_info, d_mesh_box, d_tri_v, w.leaf_box);
            hipLaunchKernelGGL(pt_ploc_prepare_boxes, grid, block, 0, stream, w.leaf_box, n, lo[0], lo[1], lo[2], inv[0], inv[1], inv[2], w.keys_in, w.vals_in);
        },
        [&](PtPlocWork& w) { hipLaunchKernelGGL(pt_ploc_init_boxes, grid, block, 0, stream, n, w.vals, w.leaf_box, w.leaf_item, w.cid[0], w.cbox[0]); },
        [&](PtPlocWork& w, uint32_t m) {
            PtPlocDirectOut o;
            o.nodes = d_nodes + node_base; o.leaf_item = w.leaf_item; o.leaf_count = w.leaf_count; o.node_parent = w.node_parent; o.leaf_parent = w.leaf_parent;
            o.counter = w.scalars; o.node_base = node_base;
            hipLaunchKernelGGL(pt_ploc_merge_direct, dim3((m + PT_BUILD_BLOCK - 1) / PT_BUILD_BLOCK), block, 0, stream, m, w.nearest, w.cid[0], w.cbox[0], w.cid[1], w.cbox[1], w.keep, o);
        },
        out, &root);
    if (e != hipSuccess) return e;
    out->root = node_base + root;
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// pt_scene_deform (pt_build.h): triangle records from new vertices, and the refit of a mesh tree whose topology stays.
// ------------------------------------------------------------------------------------------------
namespace {

__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_expand_kernel(const uint32_t* __restrict__ indices, uint32_t tri_first, uint32_t n_tris,
                                                                  const double* __restrict__ pos, const double* __restrict__ nrm, uint32_t n_verts,
                                                                  double* __restrict__ tri_v, double* __restrict__ tri_e, double* __restrict__ tri_n) {
    const uint32_t t = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (t >= n_tris) return;
    const size_t g = (size_t)tri_first + t;
    const uint32_t ia = indices[3 * g], ib = indices[3 * g + 1], ic = indices[3 * g + 2];
    if (ia >= n_verts || ib >= n_verts || ic >= n_verts) return;  // (the upload refuses such a mesh)
    double a[3], b[3], c[3];
    for (int k = 0; k < 3; k++) { a[k] = pos[3 * (size_t)ia + k]; b[k] = pos[3 * (size_t)ib + k]; c[k] = pos[3 * (size_t)ic + k]; }
    double* v = tri_v + 9 * g;
    double* e = tri_e + 9 * g;
    for (int k = 0; k < 3; k++) {
        v[k] = a[k]; v[3 + k] = b[k]; v[6 + k] = c[k];
        e[k] = a[k]; e[3 + k] = a[k] - b[k]; e[6 + k] = a[k] - c[k];
    }
    if (nrm && tri_n) {
        double* n = tri_n + 9 * g;
        for (int k = 0; k < 3; k++) { n[k] = nrm[3 * (size_t)ia + k]; n[3 + k] = nrm[3 * (size_t)ib + k]; n[6 + k] = nrm[3 * (size_t)ic + k]; }
    }
}

__device__ __forceinline__ bool pt_ref_inner(uint32_t ref) { return ref != PT_REF_EMPTY && !(ref & PT_REF_LEAF); }

__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_parent_clear_kernel(uint32_t node_count, uint32_t* __restrict__ parent) {
    const uint32_t k = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (k < node_count) parent[k] = PT_TREE_NO_PARENT;
}

// parent is indexed from the range's first node
__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_parent_kernel(const PtBvhNode* __restrict__ nodes, uint32_t node_first, uint32_t node_count,
                                                                  uint32_t* __restrict__ parent) {
    const uint32_t k = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (k >= node_count) return;
    const uint32_t i = node_first + k;
    const uint32_t child[2] = {nodes[i].child0, nodes[i].child1};
    for (int s = 0; s < 2; s++) {
        const uint32_t c = child[s];
        if (!pt_ref_inner(c) || c < node_first || c - node_first >= node_count || c == i) continue;
        parent[c - node_first] = (i << 1) | (uint32_t)s;
    }
}

struct PtRefitArgs {
    PtBvhNode* nodes;
    const uint32_t* items;
    const double* tri_v;
    const uint32_t* parent;  // from the range's first node
    uint32_t* arrive;        // likewise
    uint32_t node_first, node_count, item_first, item_count, tri_first, tri_count;
    double pad;
};

// the box of a leaf reference's triangles, padded and rounded outward; false: the reference names nothing inside the mesh's ranges
__device__ __forceinline__ bool pt_refit_leaf_box(const PtRefitArgs& a, uint32_t ref, float lo[3], float hi[3]) {
    const uint32_t first = (ref & ~PT_REF_LEAF) >> 3, count = (ref & 7u) + 1u;
    if (first < a.item_first || first - a.item_first > a.item_count || count > a.item_count - (first - a.item_first)) return false;
    double l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool any = false;
    for (uint32_t j = 0; j < count; j++) {
        const uint32_t t = a.items[first + j];
        if (t < a.tri_first || t - a.tri_first >= a.tri_count) continue;
        const double* v = a.tri_v + 9 * (size_t)t;
        for (int k = 0; k < 3; k++) {
            l[k] = fmin(l[k], fmin(fmin(v[k], v[3 + k]), v[6 + k]));
            h[k] = fmax(h[k], fmax(fmax(v[k], v[3 + k]), v[6 + k]));
        }
        any = true;
    }
    if (!any) return false;
    for (int k = 0; k < 3; k++) { lo[k] = pt_box_lo(l[k] - a.pad); hi[k] = pt_box_hi(h[k] + a.pad); }
    return true;
}

__device__ __forceinline__ void pt_refit_store_box(PtBvhNode* nd, uint32_t slot, const float lo[3], const float hi[3]) {
    for (int k = 0; k < 3; k++) { nd->lo[k][slot] = lo[k]; nd->hi[k][slot] = hi[k]; }
}

__device__ __forceinline__ float pt_refit_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(PT_BUILD_BLOCK) pt_refit_kernel(PtRefitArgs a) {
    const uint32_t k0 = blockIdx.x * PT_BUILD_BLOCK + threadIdx.x;
    if (k0 >= a.node_count) return;
    uint32_t k = k0;  // the node this thread stands at, from the range's first
    PtBvhNode* nd = a.nodes + a.node_first + k;
    const uint32_t child[2] = {nd->child0, nd->child1};
    if (child[0] == PT_REF_EMPTY && child[1] == PT_REF_EMPTY) return;  // an entry of the range that the tree does not use
    uint32_t arrivals = 0;
    for (uint32_t s = 0; s < 2; s++) {
        if (pt_ref_inner(child[s])) continue;
        float lo[3], hi[3];
        if (child[s] != PT_REF_EMPTY && pt_refit_leaf_box(a, child[s], lo, hi)) pt_refit_store_box(nd, s, lo, hi);
        arrivals++;
    }
    if (arrivals == 0) return;  // both children are inner nodes: the second of them to finish carries on from here
    // at most one pass per level of the tree: the loop ends at the root or where this thread is the first to arrive
    for (uint32_t level = 0; level <= a.node_count; level++) {
        if (arrivals < 2) {
            __threadfence();  // the box stored above is visible device-wide before the arrival is counted
            if (atomicAdd(a.arrive + k, 1u) == 0u) return;  // the first to arrive: whoever brings the other child continues
            __threadfence();  // ... whose box is read below
        }
        const uint32_t p = a.parent[k];
        if (p == PT_TREE_NO_PARENT) return;  // the root: its own box is the mesh's (PtMeshInfo::bbox_inv)
        const uint32_t pi = p >> 1, slot = p & 1u;
        if (pi < a.node_first || pi - a.node_first >= a.node_count) return;
        const bool used[2] = {nd->child0 != PT_REF_EMPTY, nd->child1 != PT_REF_EMPTY};  // (the references never change)
        float lo[3], hi[3];
        for (int ax = 0; ax < 3; ax++) {
            lo[ax] = PT_PLOC_LIMIT; hi[ax] = -PT_PLOC_LIMIT;
            for (int s = 0; s < 2; s++)
                if (used[s]) { lo[ax] = fminf(lo[ax], pt_refit_load(&nd->lo[ax][s])); hi[ax] = fmaxf(hi[ax], pt_refit_load(&nd->hi[ax][s])); }
        }
        k = pi - a.node_first;
        nd = a.nodes + pi;
        pt_refit_store_box(nd, slot, lo, hi);
        arrivals = 1;
    }
}

}  // namespace

hipError_t pt_device_expand_mesh(const uint32_t* d_indices, uint32_t tri_first, uint32_t n_tris, const double* d_pos, const double* d_nrm, uint32_t n_verts,
                                 double* d_tri_v, double* d_tri_e, double* d_tri_n, hipStream_t stream) {
    if (n_tris == 0) return hipSuccess;
    if (!d_indices || !d_pos || !d_tri_v || !d_tri_e) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_expand_kernel, dim3((n_tris + PT_BUILD_BLOCK - 1) / PT_BUILD_BLOCK), dim3(PT_BUILD_BLOCK), 0, stream, d_indices, tri_first, n_tris, d_pos,
                       d_nrm, n_verts, d_tri_v, d_tri_e, d_tri_n);
    return hipGetLastError();
}

hipError_t pt_device_tree_parents(const PtBvhNode* d_nodes, uint32_t node_first, uint32_t node_count, uint32_t* d_parent, hipStream_t stream) {
    if (node_count == 0) return hipSuccess;
    if (!d_nodes || !d_parent || node_first >= (1u << 30) || node_count >= (1u << 30)) return hipErrorInvalidValue;
    const dim3 grid((node_count + PT_BUILD_BLOCK - 1) / PT_BUILD_BLOCK), block(PT_BUILD_BLOCK);
    hipLaunchKernelGGL(pt_parent_clear_kernel, grid, block, 0, stream, node_count, d_parent + node_first);
    hipLaunchKernelGGL(pt_parent_kernel, grid, block, 0, stream, d_nodes, node_first, node_count, d_parent + node_first);
    return hipGetLastError();
}

hipError_t pt_device_refit_mesh_tree(PtBvhNode* d_nodes, uint32_t node_first, uint32_t node_count, const uint32_t* d_items, uint32_t item_first,
                                     uint32_t item_count, const double* d_tri_v, uint32_t tri_first, uint32_t tri_count, double pad,
                                     const uint32_t* d_parent, uint32_t* d_arrive, hipStream_t stream) {
    if (node_count == 0) return hipSuccess;
    if (!d_nodes || !d_items || !d_tri_v || !d_parent || !d_arrive) return hipErrorInvalidValue;
    PT_TRY(hipMemsetAsync(d_arrive + node_first, 0, 4 * (size_t)node_count, stream));
    PtRefitArgs a;
    a.nodes = d_nodes; a.items = d_items; a.tri_v = d_tri_v; a.parent = d_parent + node_first; a.arrive = d_arrive + node_first;
    a.node_first = node_first; a.node_count = node_count; a.item_first = item_first; a.item_count = item_count; a.tri_first = tri_first; a.tri_count = tri_count;
    a.pad = pad;
    hipLaunchKernelGGL(pt_refit_kernel, dim3((node_count + PT_BUILD_BLOCK - 1) / PT_BUILD_BLOCK), dim3(PT_BUILD_BLOCK), 0, stream, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// pt_device_vertex_box (pt_build.h): the box of vertices that are already in device memory.
// ------------------------------------------------------------------------------------------------
namespace {

struct PtVboxAcc {
    double v[6];
    uint32_t at[6];
    unsigned long long bad;
};

__device__ __forceinline__ void pt_vbox_clear(PtVboxAcc& a) {
#pragma unroll
    for (int k = 0; k < 3; k++) { a.v[k] = INFINITY; a.v[3 + k] = -INFINITY; a.at[k] = a.at[3 + k] = 0xFFFFFFFFu; }
    a.bad = 0ull;
}

// entry k of `a` against (v, at): the smaller (k < 3) or larger value stays, of two equal ones (+0.0 and -0.0 are the pair with different bits) the one
// met first by a loop in ascending vertex order
__device__ __forceinline__ void pt_vbox_take(PtVboxAcc& a, int k, double v, uint32_t at) {
    const bool better = k < 3 ? v < a.v[k] : a.v[k] < v;
    if (better || (v == a.v[k] && at < a.at[k])) { a.v[k] = v; a.at[k] = at; }
}

// the block's accumulators folded into *out: across the wavefront's 64 lanes in registers, then across the block's wavefronts through LDS
__device__ __forceinline__ void pt_vbox_block_reduce(PtVboxAcc a, PtVboxPartial* out) {
    __shared__ PtVboxPartial sh[PT_VBOX_BLOCK / 64];
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const double ov = __shfl_xor(a.v[k], step, 64);
            const uint32_t oat = __shfl_xor(a.at[k], step, 64);
            pt_vbox_take(a, k, ov, oat);
        }
        a.bad += __shfl_xor(a.bad, step, 64);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < 6; k++) { sh[wave].v[k] = a.v[k]; sh[wave].at[k] = a.at[k]; }
        sh[wave].non_finite = a.bad;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    for (uint32_t w = 1; w < PT_VBOX_BLOCK / 64; w++) {
#pragma unroll
        for (int k = 0; k < 6; k++) pt_vbox_take(a, k, sh[w].v[k], sh[w].at[k]);
        a.bad += sh[w].non_finite;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) { out->v[k] = a.v[k]; out->at[k] = a.at[k]; }
    out->non_finite = a.bad;
}

__device__ __forceinline__ double pt_pick3(double x0, double x1, double x2, uint32_t s) { return s == 0u ? x0 : (s == 1u ? x1 : x2); }
__device__ __forceinline__ uint32_t pt_pick3(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t s) { return s == 0u ? x0 : (s == 1u ? x1 : x2); }

// Step s covers vertices [s B, (s + 1) B), B = PT_VBOX_BLOCK: doubles [3 s B, 3 (s + 1) B) of the flat array, read as three rows of B consecutive doubles.
// Element e = j B + thread of a step belongs to vertex s B + e / 3 and - B being 1 mod 3 - to axis (j + thread) % 3: a thread's row j always carries the
// same axis, so it accumulates per row and sorts the rows into axes once, after the loop. Within a thread vertex indices only grow: `<` alone keeps the first.
static_assert(PT_VBOX_BLOCK % 3 == 1 && PT_VBOX_BLOCK % 64 == 0, "the row-to-axis rule of pt_vbox_kernel");
__global__ void __launch_bounds__(PT_VBOX_BLOCK) pt_vbox_kernel(const double* __restrict__ pos, unsigned long long n_verts, uint32_t n_steps,
                                                                PtVboxPartial* __restrict__ partials) {
    const uint32_t tid = threadIdx.x;
    const unsigned long long n_flat = 3ull * n_verts;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t lo_at[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi_at[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    unsigned long long bad = 0ull;
    for (uint32_t s = blockIdx.x; s < n_steps; s += gridDim.x) {
        const unsigned long long v0 = (unsigned long long)s * PT_VBOX_BLOCK;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const uint32_t e = (uint32_t)j * PT_VBOX_BLOCK + tid;
            const unsigned long long flat = 3ull * v0 + e;
            if (flat >= n_flat) continue;
            const double x = pos[flat];
            const uint32_t at = (uint32_t)(v0 + e / 3u);
            if (!(fabs(x) < INFINITY)) { bad++; continue; }  // NaN, +-inf
            if (x < lo[j]) { lo[j] = x; lo_at[j] = at; }
            if (hi[j] < x) { hi[j] = x; hi_at[j] = at; }
        }
    }
    PtVboxAcc a;
    const uint32_t r = tid % 3u;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        const uint32_t row = (k + 3u - r) % 3u;  // the row that carries axis k: (row + tid) % 3 == k
        a.v[k] = pt_pick3(lo[0], lo[1], lo[2], row); a.at[k] = pt_pick3(lo_at[0], lo_at[1], lo_at[2], row);
        a.v[3 + k] = pt_pick3(hi[0], hi[1], hi[2], row); a.at[3 + k] = pt_pick3(hi_at[0], hi_at[1], hi_at[2], row);
    }
    a.bad = bad;
    pt_vbox_block_reduce(a, partials + blockIdx.x);
}

// one block: partials[0 .. n) folded into partials[0] (thread 0 alone reads and, behind the block's barrier, writes that record)
__global__ void __launch_bounds__(PT_VBOX_BLOCK) pt_vbox_fold_kernel(PtVboxPartial* partials, uint32_t n) {
    PtVboxAcc a;
    pt_vbox_clear(a);
    for (uint32_t p = threadIdx.x; p < n; p += PT_VBOX_BLOCK) {
#pragma unroll
        for (int k = 0; k < 6; k++) pt_vbox_take(a, k, partials[p].v[k], partials[p].at[k]);
        a.bad += partials[p].non_finite;
    }
    pt_vbox_block_reduce(a, partials);
}

}  // namespace

hipError_t pt_device_vertex_box(const double* d_pos, uint64_t n_verts, int n_cu, PtVboxPartial* d_partials, hipStream_t stream) {
    if (!d_partials || (n_verts && !d_pos) || n_verts > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t steps = std::max<uint64_t>(1, (n_verts + PT_VBOX_BLOCK - 1) / PT_VBOX_BLOCK);  // (n_verts = 0: one block that loads nothing writes the empty box)
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(steps, pt_vertex_box_partials(n_cu));
    hipLaunchKernelGGL(pt_vbox_kernel, dim3(blocks), dim3(PT_VBOX_BLOCK), 0, stream, d_pos, (unsigned long long)n_verts, (uint32_t)steps, d_partials);
    PT_TRY(hipGetLastError());
    if (blocks > 1) {
        hipLaunchKernelGGL(pt_vbox_fold_kernel, dim3(1), dim3(PT_VBOX_BLOCK), 0, stream, d_partials, blocks);
        PT_TRY(hipGetLastError());
    }
    return hipSuccess;
}
