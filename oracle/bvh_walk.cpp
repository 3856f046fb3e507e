// TEST INFRASTRUCTURE: a host restatement of the f32 box cull of the trace kernel's BVH walk (pvt_trace_kernel.h, mesh
// branch of the node loop), on the REAL tree: it includes pvtrace_amd/csrc/pvt_bvh.h and builds with BvhBuilder::add_mesh.
//
// Restated line for line, in the kernel's order and with the kernel's types (no contraction: -ffp-contract=off):
//   minv[a] = |d_a| < 1e-300 ? 1e300 : 1 / d_a
//   the root box in doubles: ta, tb = (((double)lo_a + c_a) - o_a) * minv[a], ...;  t_near = max(0, min(ta, tb)...),
//       t_far likewise;  t_far < t_near: the walk is over before it starts
//   invf[a] = |d_a| < 1e-20 ? 1e20f : (float)minv[a]
//   oi[a]   = (float)((o_a - c_a) + d_a * t_near) * invf[a]
//   per record: ta = fmaf(lo_a, invf[a], -oi[a]), tb = fmaf(hi_a, invf[a], -oi[a]); tmin = max(0, min(ta, tb)...),
//       tmax = min(inf, max(ta, tb)...);  hit = !(tmax < tmin);  a hit inner record -> its first child, else the skip link
// ONE difference: 1 / d_a here is the compiler's correctly rounded quotient, where the kernel calls rcp_normal (a short
// division sequence it claims to be correctly rounded for ordinary numbers).  It matters only if rcp_normal is not correctly
// rounded for |d_a| >= 1e-300, which tests/test_gpu_mesh_exact.py would show as a lost crossing on the device.
// What is NOT restated because it never changes the set of leaves reached: the copy of the top levels in LDS, the cursors,
// the deferred-leaf queue.
//
// For a batch of rays it answers (i) the faces whose leaf the walk reaches, (ii) which crossings -- given by the caller (the
// exact reference's) or found here by the referee's own brute-force loop over every face in doubles (pvt_oracle_mesh_hits)
// -- lie in a leaf the walk does NOT reach, and (iii) the SLACK of every crossing in every box on its leaf's path to the root,
// on every axis with |d_a| >= 1e-20: the distance along that axis by which the computed slab interval [min(ta, tb),
// max(ta, tb)] still contains the crossing's parameter t - t_near.  The vertices of a face lie inside its boxes, so the exact
// slack is at least the pad; what the f32 arithmetic leaves of the pad is the margin of the cull.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../pvtrace_amd/csrc/pvt_bvh.h"

extern "C" int pvt_oracle_mesh_hits(const double* vertices, const int32_t* faces, int n_faces, const double* o,
                                    const double* d, double* ts, int32_t* tris, int cap);

namespace {

struct Tree {
    std::vector<pvt::BvhNode> nodes;
    std::vector<pvt::MeshTri> tris;
    std::vector<int> parent;      // record -> its parent record (-1: the root)
    std::vector<int> leaf_of;     // face -> its leaf record
    int root = 0, end = 0, depth = 0;
    double centre[3] = {0, 0, 0}, pad = 0.0, diag = 0.0;
};

void build_tree(const double* v, int nv, const int32_t* f, int nf, Tree& T) {
    std::vector<double> normals(3 * (size_t)nf);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < nf; k++) {
        const double *a = v + 3 * (size_t)f[3 * k], *b = v + 3 * (size_t)f[3 * k + 1], *c = v + 3 * (size_t)f[3 * k + 2];
        const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double m = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (int x = 0; x < 3; x++) normals[3 * (size_t)k + x] = n[x] / m;
        for (int corner = 0; corner < 3; corner++)
            for (int x = 0; x < 3; x++) {
                const double p = v[3 * (size_t)f[3 * k + corner] + x];
                lo[x] = std::min(lo[x], p);
                hi[x] = std::max(hi[x], p);
            }
    }
    (void)nv;
    T.diag = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    T.pad = 4e-6 * T.diag + 1e-300;   // (pvt_bvh.h: add_mesh)
    pvt::BvhBuilder builder(v, f, normals.data(), T.nodes, T.tris);
    T.root = builder.add_mesh(0, nf, T.centre);
    T.end = T.nodes[T.root].skip;
    T.parent.assign(T.nodes.size(), -1);
    T.leaf_of.assign((size_t)nf, -1);
    std::vector<std::pair<int, int>> todo{{T.root, 1}};
    while (!todo.empty()) {
        const auto [i, d] = todo.back();
        todo.pop_back();
        T.depth = std::max(T.depth, d);
        const pvt::BvhNode& b = T.nodes[i];
        if (b.link < 0) {
            T.leaf_of[(size_t)T.tris[(size_t)(b.link & pvt::kIndexMask)].face] = i;
        } else {
            for (int c = b.link; c < b.link + 2; c++) { T.parent[c] = i; todo.push_back({c, d + 1}); }
        }
    }
}

struct Walk {
    double t_near = 0.0;
    float oi[3], invf[3];
    bool started = false;
};

// the kernel's preparation of a walk (see the head of this file)
Walk prepare(const Tree& T, const double* oo, const double* dd) {
    Walk W;
    double minv[3];
    for (int a = 0; a < 3; a++) minv[a] = std::fabs(dd[a]) < 1e-300 ? 1e300 : 1.0 / dd[a];
    const pvt::BvhNode& r = T.nodes[T.root];
    double t_near = 0.0, t_far = INFINITY;
    for (int a = 0; a < 3; a++) {
        const double ta = (((double)r.lo[a] + T.centre[a]) - oo[a]) * minv[a], tb = (((double)r.hi[a] + T.centre[a]) - oo[a]) * minv[a];
        t_near = __builtin_fmax(t_near, __builtin_fmin(ta, tb));
        t_far = __builtin_fmin(t_far, __builtin_fmax(ta, tb));
    }
    W.started = !(t_far < t_near);
    W.t_near = t_near;
    for (int a = 0; a < 3; a++) {
        W.invf[a] = std::fabs(dd[a]) < 1e-20 ? 1e20f : (float)minv[a];
        W.oi[a] = (float)((oo[a] - T.centre[a]) + dd[a] * t_near) * W.invf[a];
    }
    return W;
}

inline bool box_hit(const Walk& W, const pvt::BvhNode& b) {
    float tmin = 0.0f, tmax = INFINITY;
    for (int a = 0; a < 3; a++) {
        const float ta = __builtin_fmaf(b.lo[a], W.invf[a], -W.oi[a]), tb = __builtin_fmaf(b.hi[a], W.invf[a], -W.oi[a]);
        tmin = __builtin_fmaxf(tmin, __builtin_fminf(ta, tb));
        tmax = __builtin_fminf(tmax, __builtin_fmaxf(ta, tb));
    }
    return !(tmax < tmin);
}

// marks the faces whose leaf the walk reaches; returns how many
int walk(const Tree& T, const Walk& W, std::vector<int32_t>& reached) {
    reached.clear();
    if (!W.started) return 0;
    int i = T.root;
    while (i != T.end) {
        const pvt::BvhNode& b = T.nodes[i];
        int next = b.skip;
        if (box_hit(W, b)) {
            if (b.link < 0) reached.push_back((int32_t)T.tris[(size_t)(b.link & pvt::kIndexMask)].face);
            else next = b.link;
        }
        i = next;
    }
    return (int)reached.size();
}

// slack of a crossing at parameter t in the boxes from face's leaf up to the root, as a distance along the worst axis
double slack(const Tree& T, const Walk& W, const double* dd, int face, double t, int* worst_axis) {
    const double s = t - W.t_near;
    double least = INFINITY;
    for (int i = T.leaf_of[(size_t)face]; i >= 0; i = T.parent[i]) {
        const pvt::BvhNode& b = T.nodes[i];
        for (int a = 0; a < 3; a++) {
            if (std::fabs(dd[a]) < 1e-20) continue;
            const double ta = (double)__builtin_fmaf(b.lo[a], W.invf[a], -W.oi[a]), tb = (double)__builtin_fmaf(b.hi[a], W.invf[a], -W.oi[a]);
            const double room = std::fmin(s - std::fmin(ta, tb), std::fmax(ta, tb) - s) * std::fabs(dd[a]);
            if (room < least) { least = room; if (worst_axis) *worst_axis = a; }
        }
    }
    return least;
}

}  // namespace

// out[0] crossings that lie in a leaf the walk does not reach, out[1], out[2] the first such ray and face (-1: none);
// out[3] least slack / pad over the crossings checked, out[4..6] its ray, face and axis; out[7] crossings checked;
// out[8] the pad; out[9] leaves reached in all, out[10] the most by one ray; out[11] records in the tree, out[12] its depth.
// cross_*: the crossings to check (ray, face, t), n_cross of them; n_cross < 0: the referee's brute-force loop finds them.
// reached_ptr (n_rays + 1) / reached (reached_cap): the faces reached, ray by ray (nullable).  Returns 0, or -1 when
// `reached` is too small.
extern "C" int pvt_bvh_walk_check(const double* vertices, int n_vertices, const int32_t* faces, int n_faces,
                                  const double* origins, const double* dirs, int n_rays,
                                  const int32_t* cross_ray, const int32_t* cross_face, const double* cross_t, int n_cross,
                                  double* out, int64_t* reached_ptr, int32_t* reached, int64_t reached_cap) {
    Tree T;
    build_tree(vertices, n_vertices, faces, n_faces, T);
    for (int k = 0; k < 13; k++) out[k] = 0.0;
    out[1] = out[2] = out[4] = out[5] = out[6] = -1.0;
    out[3] = INFINITY;
    out[8] = T.pad;
    out[11] = (double)(T.end - T.root);
    out[12] = (double)T.depth;
    std::vector<int64_t> first(n_rays + 1, 0);   // the given crossings, bucketed by ray (they come sorted by ray)
    if (n_cross >= 0) {
        for (int k = 0; k < n_cross; k++) first[cross_ray[k] + 1] += 1;
        for (int j = 0; j < n_rays; j++) first[j + 1] += first[j];
    }
    int rc = 0;
    int64_t fill = 0;
    if (reached_ptr) reached_ptr[0] = 0;
#pragma omp parallel if (!reached_ptr)
    {
        std::vector<int32_t> got, tris((size_t)n_faces);
        std::vector<double> ts((size_t)n_faces);
        std::vector<char> mark((size_t)n_faces, 0);
        double lost = 0, first_ray = -1, first_face = -1, least = INFINITY, l_ray = -1, l_face = -1, l_axis = -1, checked = 0,
               leaves = 0, most = 0;
#pragma omp for schedule(dynamic, 256)
        for (int j = 0; j < n_rays; j++) {
            const double *oo = origins + 3 * (size_t)j, *dd = dirs + 3 * (size_t)j;
            const Walk W = prepare(T, oo, dd);
            const int n = walk(T, W, got);
            leaves += n;
            most = std::max(most, (double)n);
            for (int32_t f : got) mark[(size_t)f] = 1;
            int nc;
            const int32_t* cf;
            const double* ct;
            if (n_cross >= 0) {
                nc = (int)(first[j + 1] - first[j]); cf = cross_face + first[j]; ct = cross_t + first[j];
            } else {
                nc = pvt_oracle_mesh_hits(vertices, faces, n_faces, oo, dd, ts.data(), tris.data(), n_faces);
                cf = tris.data(); ct = ts.data();
            }
            for (int k = 0; k < nc; k++) {
                checked += 1;
                if (!mark[(size_t)cf[k]]) {
                    if (lost == 0) { first_ray = j; first_face = cf[k]; }
                    lost += 1;
                }
                int axis = -1;
                const double room = slack(T, W, dd, cf[k], ct[k], &axis) / T.pad;
                if (room < least) { least = room; l_ray = j; l_face = cf[k]; l_axis = axis; }
            }
            for (int32_t f : got) mark[(size_t)f] = 0;
            if (reached_ptr) {   // (serial in this mode)
                if (reached && fill + n <= reached_cap) std::memcpy(reached + fill, got.data(), sizeof(int32_t) * (size_t)n);
                else if (reached) rc = -1;
                fill += n;
                reached_ptr[j + 1] = fill;
            }
        }
#pragma omp critical
        {
            if (lost > 0 && (out[1] < 0 || first_ray < out[1])) { out[1] = first_ray; out[2] = first_face; }
            out[0] += lost;
            if (least < out[3] || (least == out[3] && l_ray < out[4])) { out[3] = least; out[4] = l_ray; out[5] = l_face; out[6] = l_axis; }
            out[7] += checked;
            out[9] += leaves;
            out[10] = std::max(out[10], most);
        }
    }
    return rc;
}
