// fw_bvh.cpp -- host build of a collider mesh's bounding-volume hierarchy (layout: fw_bvh.h).  Binned SAH over triangle
// centroids, an explicit stack (a degenerate mesh cannot run the host out of call stack), preorder node numbering.
#include "fw_bvh.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

struct Prim {
    float lo[3], hi[3], c[3];  // box and centroid of the triangle
    uint32_t tri;              // index into the kept triangles
};

inline float bits_f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

struct Box {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    void grow(const float *l, const float *h) {
        for (int k = 0; k < 3; k++) lo[k] = std::min(lo[k], l[k]), hi[k] = std::max(hi[k], h[k]);
    }
    double area() const {
        if (!(hi[0] >= lo[0])) return 0.0;
        const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
        return x * y + y * z + z * x;
    }
};

struct Item {
    uint32_t b, e;   // prims [b, e)
    int32_t parent;  // -1: the root
    bool right;      // the parent's second child
};

// the one builder behind both entries; keep_all: a deformable mesh (every triangle gets a slot, the refit tables are filled)
int build(const float *xyz, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, bool keep_all, FwBvh *out,
          std::string *err) {
    *out = FwBvh{};
    if (!xyz || !indices || n_vertices == 0 || n_triangles == 0) return *err = "empty mesh", -1;
    if (n_triangles > (1u << 28)) return *err = "more than 2^28 triangles", -1;
    for (size_t i = 0; i < (size_t)n_vertices * 3; i++)
        if (!std::isfinite(xyz[i])) return *err = "non-finite vertex " + std::to_string(i / 3), -1;
    for (size_t i = 0; i < (size_t)n_triangles * 3; i++)
        if (indices[i] >= n_vertices) return *err = "index out of range in triangle " + std::to_string(i / 3), -1;

    // the triangles as the device tests them: v0, e1 = v1 - v0, e2 = v2 - v0 (fp32); zero-area ones dropped
    std::vector<float> tri;  // kept triangles, 12 floats each (original order)
    std::vector<Prim> P;
    tri.reserve((size_t)n_triangles * 12);
    P.reserve(n_triangles);
    std::vector<uint32_t> slot_src;  // keep_all: per kept triangle {its three vertex indices, its original index}
    uint32_t n_live = 0;
    float maxabs = 0.0f;
    for (uint32_t t = 0; t < n_triangles; t++) {
        const float *v[3] = {xyz + 3 * (size_t)indices[3 * (size_t)t], xyz + 3 * (size_t)indices[3 * (size_t)t + 1],
                             xyz + 3 * (size_t)indices[3 * (size_t)t + 2]};
        const float e1[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
        const float e2[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
        // c = cross(e1, e2) in fw_cross's operation order
        const float c[3] = {e1[1] * e2[2] - e2[1] * e1[2], e1[2] * e2[0] - e2[2] * e1[0], e1[0] * e2[1] - e2[0] * e1[1]};
        const float cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
        const bool live = cc > 0.0f && std::isfinite(cc);
        if (!live && !keep_all) continue;
        n_live += live;
        Prim p;
        for (int k = 0; k < 3; k++) {
            p.lo[k] = std::min(v[0][k], std::min(v[1][k], v[2][k]));
            p.hi[k] = std::max(v[0][k], std::max(v[1][k], v[2][k]));
            p.c[k] = (float)(((double)p.lo[k] + p.hi[k]) * 0.5);
            maxabs = std::max(maxabs, std::max(std::fabs(p.lo[k]), std::fabs(p.hi[k])));
        }
        p.tri = (uint32_t)P.size();
        P.push_back(p);
        // (a dropped triangle of a deformable mesh: e1 = e2 = 0, the record no ray hits -- fw_refit.h)
        const float rec[12] = {v[0][0], v[0][1], v[0][2], bits_f(t), live ? e1[0] : 0.0f, live ? e1[1] : 0.0f, live ? e1[2] : 0.0f, 0.0f,
                               live ? e2[0] : 0.0f, live ? e2[1] : 0.0f, live ? e2[2] : 0.0f, 0.0f};
        tri.insert(tri.end(), rec, rec + 12);
        if (keep_all) {
            const uint32_t si[4] = {indices[3 * (size_t)t], indices[3 * (size_t)t + 1], indices[3 * (size_t)t + 2], t};
            slot_src.insert(slot_src.end(), si, si + 4);
        }
    }
    if (n_live == 0) return *err = "no triangle of non-zero area", -1;
    // Every box is grown by `pad` on each side.  The rounding of the slab test and of the triangle test is a few ulps of the
    // terms they subtract -- the ray origin in the mesh's frame against box faces and vertices -- and a ray can only hit the
    // mesh from within max_distance of it, so those terms stay below (largest vertex coordinate + max_distance).  The pad
    // covers that rounding as long as max_distance (a particle's speed times the step) stays below ~1000 times the mesh's
    // largest coordinate -- a 1 m mesh and 1 km per step -- so within that bound the walk never culls a triangle the
    // brute-force test hits.
    const float pad = std::max(1e-4f * maxabs, 1e-30f);

    const uint32_t n = (uint32_t)P.size();
    std::vector<float> &nodes = out->nodes;
    std::vector<int32_t> second;  // per node: index of its second child (-1: a leaf)
    std::vector<int32_t> &parent = out->parent;
    nodes.reserve((size_t)2 * n * 8);
    second.reserve((size_t)2 * n);
    std::vector<uint32_t> leaf_order;
    leaf_order.reserve(n);
    std::vector<Item> stack{{0u, n, -1, false}};
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        const uint32_t idx = (uint32_t)(nodes.size() / 8);
        if (it.parent >= 0 && it.right) second[it.parent] = (int32_t)idx;
        Box box, cbox;
        for (uint32_t i = it.b; i < it.e; i++) box.grow(P[i].lo, P[i].hi), cbox.grow(P[i].c, P[i].c);
        const uint32_t cnt = it.e - it.b;
        uint32_t mid = 0;
        if (cnt > FW_BVH_LEAF) {
            // binned SAH on the three axes; no usable split (all centroids in one bin): the median along the widest axis
            double best = INFINITY;
            int best_axis = -1, best_bin = 0;
            for (int a = 0; a < 3; a++) {
                const double ext = (double)cbox.hi[a] - cbox.lo[a];
                if (!(ext > 0.0)) continue;
                Box bb[FW_BVH_BINS];
                uint32_t bn[FW_BVH_BINS] = {0};
                const double k = FW_BVH_BINS / ext;
                for (uint32_t i = it.b; i < it.e; i++) {
                    const int bi = std::min(std::max((int)(((double)P[i].c[a] - cbox.lo[a]) * k), 0), FW_BVH_BINS - 1);
                    bb[bi].grow(P[i].lo, P[i].hi), bn[bi]++;
                }
                double right_area[FW_BVH_BINS];
                uint32_t right_n[FW_BVH_BINS];
                Box acc;
                uint32_t an = 0;
                for (int s = FW_BVH_BINS - 1; s > 0; s--) {
                    acc.grow(bb[s].lo, bb[s].hi), an += bn[s];
                    right_area[s] = acc.area(), right_n[s] = an;
                }
                Box lacc;
                uint32_t ln = 0;
                for (int s = 1; s < FW_BVH_BINS; s++) {  // split: bins [0, s) | [s, BINS)
                    lacc.grow(bb[s - 1].lo, bb[s - 1].hi), ln += bn[s - 1];
                    if (ln == 0 || right_n[s] == 0) continue;
                    const double cost = lacc.area() * ln + right_area[s] * right_n[s];
                    if (cost < best) best = cost, best_axis = a, best_bin = s;
                }
            }
            if (best_axis >= 0) {
                const int a = best_axis;
                const double k = FW_BVH_BINS / ((double)cbox.hi[a] - cbox.lo[a]);
                const double lo = cbox.lo[a];
                Prim *m = std::partition(P.data() + it.b, P.data() + it.e, [&](const Prim &p) {
                    return std::min(std::max((int)(((double)p.c[a] - lo) * k), 0), FW_BVH_BINS - 1) < best_bin;
                });
                mid = (uint32_t)(m - P.data());
            }
            if (best_axis < 0 || mid == it.b || mid == it.e) {
                int a = 0;
                for (int k2 = 1; k2 < 3; k2++)
                    if ((double)box.hi[k2] - box.lo[k2] > (double)box.hi[a] - box.lo[a]) a = k2;
                mid = it.b + cnt / 2;
                std::nth_element(P.data() + it.b, P.data() + mid, P.data() + it.e,
                                 [a](const Prim &x, const Prim &y) { return x.c[a] < y.c[a]; });
            }
        }
        uint32_t leaf = 0;
        if (cnt <= FW_BVH_LEAF) {
            leaf = ((uint32_t)leaf_order.size() << 4) | cnt;
            for (uint32_t i = it.b; i < it.e; i++) leaf_order.push_back(P[i].tri);
        }
        const float rec[8] = {box.lo[0] - pad, box.lo[1] - pad, box.lo[2] - pad, 0.0f,
                              box.hi[0] + pad, box.hi[1] + pad, box.hi[2] + pad, bits_f(leaf)};
        nodes.insert(nodes.end(), rec, rec + 8);
        second.push_back(-1);
        parent.push_back(it.parent);
        if (!leaf) {  // the first child next (node idx + 1), the second after the first one's subtree
            stack.push_back({mid, it.e, (int32_t)idx, true});
            stack.push_back({it.b, mid, (int32_t)idx, false});
        }
    }
    // escapes: the root's is the node count; an interior node's first child escapes to its second child, the second child to
    // the node's own escape (parents precede their children in preorder)
    const uint32_t n_nodes = (uint32_t)(nodes.size() / 8);
    std::vector<uint32_t> esc(n_nodes, n_nodes);
    for (uint32_t i = 0; i < n_nodes; i++) {
        if (second[i] < 0) continue;
        esc[i + 1] = (uint32_t)second[i];
        esc[second[i]] = esc[i];
    }
    for (uint32_t i = 0; i < n_nodes; i++) nodes[8 * (size_t)i + 3] = bits_f(esc[i]);
    out->tris.resize((size_t)n * 12);
    for (uint32_t i = 0; i < n; i++) memcpy(&out->tris[(size_t)i * 12], &tri[(size_t)leaf_order[i] * 12], 12 * sizeof(float));
    out->n_nodes = n_nodes, out->n_tris = n, out->pad = pad;
    for (int k = 0; k < 3; k++) out->lo[k] = nodes[k], out->hi[k] = nodes[4 + k];
    if (!keep_all) return parent.clear(), 0;
    out->slots.resize((size_t)n * 4);
    for (uint32_t i = 0; i < n; i++) memcpy(&out->slots[(size_t)i * 4], &slot_src[(size_t)leaf_order[i] * 4], 4 * sizeof(uint32_t));
    // the refit's schedule: nodes by height (a leaf: 0; an interior node: 1 + its higher child), so that every node of a level
    // depends on lower levels only.  Children follow their parents in preorder: one pass backwards has the heights.
    std::vector<uint32_t> height(n_nodes, 0u);
    uint32_t top = 0;
    for (uint32_t i = n_nodes; i-- > 1;) {
        height[parent[i]] = std::max(height[parent[i]], height[i] + 1u);
    }
    top = height[0];
    out->level_off.assign((size_t)top + 2, 0u);
    for (uint32_t i = 0; i < n_nodes; i++) out->level_off[height[i] + 1]++;
    for (uint32_t l = 0; l <= top; l++) out->level_off[l + 1] += out->level_off[l];
    out->order.resize(n_nodes);
    std::vector<uint32_t> at(out->level_off.begin(), out->level_off.end() - 1);
    for (uint32_t i = 0; i < n_nodes; i++) out->order[at[height[i]]++] = i;
    return 0;
}

}  // namespace

int fw_bvh_build(const float *xyz, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, FwBvh *out,
                 std::string *err) {
    return build(xyz, n_vertices, indices, n_triangles, false, out, err);
}

int fw_bvh_build_deformable(const float *xyz, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, FwBvh *out,
                            std::string *err) {
    return build(xyz, n_vertices, indices, n_triangles, true, out, err);
}

int64_t fw_bvh_stage_vertices(const float *xyz, const uint8_t *referenced, uint32_t n_vertices, float *dst, float lo[3], float hi[3],
                              float *pad) {
    float maxabs = 0.0f;
    for (int k = 0; k < 3; k++) lo[k] = INFINITY, hi[k] = -INFINITY;
    for (uint32_t v = 0; v < n_vertices; v++) {
        const float x[3] = {xyz[3 * (size_t)v], xyz[3 * (size_t)v + 1], xyz[3 * (size_t)v + 2]};
        if (!std::isfinite(x[0]) || !std::isfinite(x[1]) || !std::isfinite(x[2])) return (int64_t)v;
        if (dst) dst[3 * (size_t)v] = x[0], dst[3 * (size_t)v + 1] = x[1], dst[3 * (size_t)v + 2] = x[2];
        if (!referenced[v]) continue;
        for (int k = 0; k < 3; k++) {
            lo[k] = std::min(lo[k], x[k]), hi[k] = std::max(hi[k], x[k]);
            maxabs = std::max(maxabs, std::fabs(x[k]));
        }
    }
    *pad = std::max(1e-4f * maxabs, 1e-30f);
    for (int k = 0; k < 3; k++) lo[k] = lo[k] - *pad, hi[k] = hi[k] + *pad;
    return -1;
}

void fw_bvh_bounds(const float *xyz, const uint8_t *referenced, uint32_t n_vertices, float lo[3], float hi[3], float *pad) {
    (void)fw_bvh_stage_vertices(xyz, referenced, n_vertices, nullptr, lo, hi, pad);
}
