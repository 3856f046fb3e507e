// pvt_scene_pack.h — the host half of pvt_scene_create: the scene tables are checked and packed into the two blobs the
// kernel reads (struct Lay in pvt_trace_kernel.h), the BVHs of the meshes and the shortcuts the host can prove.  No HIP
// call: pvt_trace.hip includes this after pvt_trace_kernel.h and uploads what pack_scene returns.
#pragma once

namespace {

// The surface branch asks "is the incidence angle beyond the critical angle?", which the reference evaluates as
// acos(c) > crit (c = the clamped cosine in [0, 1]).  pvt_acos falls as c grows, so there is a threshold c* with
// pvt_acos(c) > crit  <=>  c < c*: found here by bisection over the doubles of [0, 1] with the very pvt_acos the
// device runs, then CHECKED -- pvt_acos is accurate to under an ulp but need not be monotone to the last bit, so
// the 1024 doubles either side of the boundary are all evaluated; farther away the angle differs from crit by
// hundreds of ulps (|d acos / dc| >= 1) and the sign of the comparison cannot depend on the rounding.  NaN = no
// threshold could be proven (the kernel then evaluates the reference's expression); -inf = never total reflection.
double cosine_threshold(double crit) {
    if (!(crit < INFINITY)) return -INFINITY;
    auto beyond = [&](double c) { return pvt_acos(c) > crit; };
    if (!beyond(0.0)) return -INFINITY;     // (not reachable for crit = asin(x) < pi/2; kept for safety)
    if (beyond(1.0)) return NAN;
    auto bits = [](double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; };
    auto from = [](uint64_t u) { double v; std::memcpy(&v, &u, 8); return v; };
    uint64_t lo = bits(0.0), hi = bits(1.0);   // beyond(lo), !beyond(hi); non-negative doubles order like their bits
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (beyond(from(mid))) lo = mid; else hi = mid;
    }
    for (uint64_t k = 1; k <= 1024; k++) {
        if (lo >= k && !beyond(from(lo - k))) return NAN;
        if (hi + k <= bits(1.0) && beyond(from(hi + k))) return NAN;
    }
    return from(hi);   // the smallest cosine that is NOT beyond the critical angle
}

// The node grid of scenes with many nodes (kernel: GRID variants, the walk in the node loop).  Every node but the root
// is filed under the cells that its world-space bounding box, grown by 2m, touches; m = 1e-6 of the scene's extent, many
// orders of magnitude above the rounding of any distance the intersection arithmetic forms (1e-16 of it per
// operation).  What the kernel's early exit relies on, with that margin:
//   * a crossing the reference's arithmetic reports for a node lies inside that node's box grown by m, so some cell the
//     walk has visited by then (the walk's own rounding: 1e-13 of the extent) holds the node;
//   * a node filed under none of the cells visited so far stands clear of the photon by more than m, so a box or a
//     sphere (radius >= 1e-5 of the extent, checked here) is crossed twice or not at all -- never once.
// Returns false (no grid: the plain node loop serves the scene) for scenes it cannot vouch for: few nodes, meshes,
// non-rigid or inconsistent poses, degenerate shapes.
// Negative controls of the grid tests (tests/test_gpu_grid.py, tests/test_node_grid.py) are environment switches read
// when a scene is created, and they produce WRONG physics on purpose: whoever has one set gets told, loudly, every time.
bool dev_switch(const char* name) {
    if (!getenv(name)) return false;
    fprintf(stderr, "[pvtrace_hip] WARNING: %s is set -- the node grid of this scene is built WRONG on purpose (a test's negative "
                    "control); unset it for real work\n", name);
    return true;
}

struct NodeGrid {
    int n[3] = {1, 1, 1};
    double lo[3], hi[3], cell[3], guard = 0.0;
    int words = 1;
    bool odd = false;
    std::vector<unsigned long long> masks;
};
bool plan_node_grid(const PvtSceneTables* t, NodeGrid* g) {
    const int N = t->n_nodes, root = t->root_id;
    if (getenv("PVT_NO_GRID") || N < 8) return false;
    std::vector<double> blo((size_t)N * 3), bhi((size_t)N * 3);
    double extent = 0.0;
    for (int n = 0; n < N; n++) {
        // (a truncated cone: the plain node loop serves its scene -- the `default` cases below, and the grid walk's
        // shape_hits in the kernel, mean "cylinder" and never see one)
        if (t->geom_type[n] == PVT_GEOM_MESH || t->geom_type[n] == PVT_GEOM_FRUSTUM || t->geom_type[n] == PVT_GEOM_POLYHEDRON ||
            t->geom_type[n] == PVT_GEOM_CONICOID) return false;
        const double* w = t->world_to_local + n * 16;
        const double* l = t->local_to_world + n * 16;
        const double* gp = t->geom_params + n * 4;
        double h[3];
        switch (t->geom_type[n]) {
            case PVT_GEOM_BOX: h[0] = 0.5 * gp[0]; h[1] = 0.5 * gp[1]; h[2] = 0.5 * gp[2]; break;
            case PVT_GEOM_SPHERE: h[0] = h[1] = h[2] = gp[0]; break;
            default: h[0] = h[1] = gp[1]; h[2] = 0.5 * gp[0]; break;   // cylinder about z
        }
        for (int a = 0; a < 3; a++)
            if (!(std::isfinite(h[a]) && h[a] > 0.0)) return false;
        // rigid and consistent: world->local is a rotation plus a translation, local->world its inverse
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                double rr = 0.0, wl = 0.0;
                for (int k = 0; k < 3; k++) { rr += w[r * 4 + k] * w[c * 4 + k]; wl += w[r * 4 + k] * l[k * 4 + c]; }
                if (!(std::fabs(rr - (r == c ? 1.0 : 0.0)) < 1e-9) || !(std::fabs(wl - (r == c ? 1.0 : 0.0)) < 1e-9)) return false;
            }
        double back = 0.0;   // world->local of the node's own origin must be the zero vector
        for (int r = 0; r < 3; r++) {
            const double v = w[r * 4] * l[3] + w[r * 4 + 1] * l[7] + w[r * 4 + 2] * l[11] + w[r * 4 + 3];
            back = std::fmax(back, std::fabs(v));
        }
        for (int a = 0; a < 3; a++) {
            const double c = l[a * 4 + 3];
            double hw = t->geom_type[n] == PVT_GEOM_SPHERE ? h[0]
                                                           : std::fabs(l[a * 4]) * h[0] + std::fabs(l[a * 4 + 1]) * h[1] + std::fabs(l[a * 4 + 2]) * h[2];
            hw *= 1.0 + 1e-9;
            if (!std::isfinite(c) || !std::isfinite(hw)) return false;
            blo[(size_t)n * 3 + a] = c - hw; bhi[(size_t)n * 3 + a] = c + hw;
            extent = std::fmax(extent, std::fabs(c) + hw);
        }
        if (!(back <= 1e-9 * (1.0 + extent))) return false;
    }
    if (!(extent > 0.0) || !std::isfinite(extent)) return false;
    const double m = 1e-6 * extent;
    for (int n = 0; n < N; n++) {
        if (n == root || t->geom_type[n] == PVT_GEOM_BOX) continue;
        const double radius = t->geom_type[n] == PVT_GEOM_SPHERE ? t->geom_params[n * 4] : t->geom_params[n * 4 + 1];
        if (!(radius >= 1e-5 * extent)) return false;
        if (t->geom_type[n] == PVT_GEOM_CYLINDER) g->odd = true;
    }
    // (negative controls of tests/test_gpu_grid.py: file the boxes a centimetre too small / leave the walk as soon as
    // any two crossings are known -- results must then differ from the referee's)
    const double grow = dev_switch("PVT_GRID_DEV_SHRINK") ? -1.0 : 2.0 * m;
    for (int a = 0; a < 3; a++) { g->lo[a] = INFINITY; g->hi[a] = -INFINITY; }
    for (int n = 0; n < N; n++) {
        if (n == root) continue;
        for (int a = 0; a < 3; a++) {
            blo[(size_t)n * 3 + a] -= grow; bhi[(size_t)n * 3 + a] += grow;
            g->lo[a] = std::fmin(g->lo[a], blo[(size_t)n * 3 + a] - m);
            g->hi[a] = std::fmax(g->hi[a], bhi[(size_t)n * 3 + a] + m);
        }
    }
    // ---- resolution.  What a photon pays for is the nodes it tests and the cells it steps through, and both depend on
    // how the cells fall on the nodes: on an array of 6 x 6 tiles a 6 x 6 grid (one tile per cell) traces 2.26e9
    // photons/s, 8 x 8 and 15 x 15 grids 1.58e9, 11 x 11 1.93e9 (measured).  So the resolution is CHOSEN: starting from
    // about one cubic cell per node, each axis in turn tries other counts, and a candidate is priced by walking a fixed
    // set of sample rays through it -- the kernel's walk with the nodes' boxes standing in for the shapes: cells
    // visited, nodes tested, exit once two crossings lie before the end of the cells visited.  A wave waits for its
    // slowest lane, so the price is the mean over the dearest quarter of the rays.
    const int W = N > 64 ? 2 : 1;
    auto file_nodes = [&](const int (&dims)[3], double (&cell)[3], std::vector<unsigned long long>& masks) {
        for (int a = 0; a < 3; a++) cell[a] = (g->hi[a] - g->lo[a]) / dims[a];
        masks.assign((size_t)dims[0] * dims[1] * dims[2] * W, 0ull);
        for (int n = 0; n < N; n++) {
            if (n == root) continue;
            int c0[3], c1[3];
            for (int a = 0; a < 3; a++) {   // cells touched, one cell more on either side when a face lies within m of a cell wall
                c0[a] = (int)std::floor((blo[(size_t)n * 3 + a] - m - g->lo[a]) / cell[a]);
                c1[a] = (int)std::floor((bhi[(size_t)n * 3 + a] + m - g->lo[a]) / cell[a]);
                c0[a] = c0[a] < 0 ? 0 : c0[a];
                c1[a] = c1[a] > dims[a] - 1 ? dims[a] - 1 : c1[a];
            }
            for (int z = c0[2]; z <= c1[2]; z++)
                for (int y = c0[1]; y <= c1[1]; y++)
                    for (int x = c0[0]; x <= c1[0]; x++)
                        masks[(((size_t)z * dims[1] + y) * dims[0] + x) * W + (n >> 6)] |= 1ull << (n & 63);
        }
    };
    // sample rays (fixed pseudo-random sequence: the same scene always gets the same grid): from inside a node's box,
    // from a face of one, from anywhere in the grid's box; directions isotropic
    struct Ray { double o[3], d[3]; };
    std::vector<Ray> rays;
    {
        unsigned long long st = 0x9E3779B97F4A7C15ull;
        auto uni = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)(st >> 11) * (1.0 / 9007199254740992.0); };
        std::vector<int> others;
        for (int n = 0; n < N; n++) if (n != root) others.push_back(n);
        for (int k = 0; k < 384; k++) {
            Ray r;
            const int n = others[(size_t)(uni() * others.size()) % others.size()];
            for (int a = 0; a < 3; a++) {
                const double lo = k % 4 == 3 ? g->lo[a] : blo[(size_t)n * 3 + a], hi = k % 4 == 3 ? g->hi[a] : bhi[(size_t)n * 3 + a];
                r.o[a] = lo + uni() * (hi - lo);
            }
            if (k % 4 == 2) { const int a = (int)(uni() * 3) % 3; r.o[a] = uni() < 0.5 ? blo[(size_t)n * 3 + a] + grow : bhi[(size_t)n * 3 + a] - grow; }
            double z = 2.0 * uni() - 1.0, ph = 6.283185307179586 * uni(), s = std::sqrt(1.0 - z * z);
            r.d[0] = s * std::cos(ph); r.d[1] = s * std::sin(ph); r.d[2] = z;
            rays.push_back(r);
        }
    }
    auto price = [&](const int (&dims)[3]) -> double {
        double cell[3];
        std::vector<unsigned long long> masks;
        file_nodes(dims, cell, masks);
        std::vector<double> cost;
        for (const Ray& r : rays) {
            double t_in = 0.0, t_out = INFINITY;
            bool walk = true;
            for (int a = 0; a < 3; a++) {
                if (std::fabs(r.d[a]) < 1e-20) { if (r.o[a] < g->lo[a] || r.o[a] > g->hi[a]) walk = false; continue; }
                const double ta = (g->lo[a] - r.o[a]) / r.d[a], tb = (g->hi[a] - r.o[a]) / r.d[a];
                t_in = std::fmax(t_in, std::fmin(ta, tb)); t_out = std::fmin(t_out, std::fmax(ta, tb));
            }
            if (!(t_in <= t_out)) walk = false;
            int c[3] = {0, 0, 0};
            double tm[3] = {INFINITY, INFINITY, INFINITY};
            for (int a = 0; a < 3 && walk; a++) {
                c[a] = (int)((r.o[a] + r.d[a] * t_in - g->lo[a]) / cell[a]);
                c[a] = c[a] < 0 ? 0 : (c[a] > dims[a] - 1 ? dims[a] - 1 : c[a]);
                if (std::fabs(r.d[a]) >= 1e-20) tm[a] = (g->lo[a] + (c[a] + (r.d[a] < 0 ? 0 : 1)) * cell[a] - r.o[a]) / r.d[a];
            }
            unsigned long long seen[2] = {0ull, 0ull};
            int cells = 0, tests = 0, nh = 0;
            double t1 = INFINITY, t2 = INFINITY;
            while (walk) {
                cells += 1;
                const unsigned long long* mk = &masks[(((size_t)c[2] * dims[1] + c[1]) * dims[0] + c[0]) * W];
                for (int w = 0; w < W; w++) {
                    unsigned long long fresh = mk[w] & ~seen[w];
                    seen[w] |= mk[w];
                    while (fresh) {
                        const int n = w * 64 + __builtin_ctzll(fresh);
                        fresh &= fresh - 1;
                        tests += 1;
                        double te = -INFINITY, tx = INFINITY;   // the ray against the node's box
                        bool miss = false;
                        for (int a = 0; a < 3; a++) {
                            const double lo = blo[(size_t)n * 3 + a], hi = bhi[(size_t)n * 3 + a];
                            if (std::fabs(r.d[a]) < 1e-20) { if (r.o[a] < lo || r.o[a] > hi) miss = true; continue; }
                            const double ta = (lo - r.o[a]) / r.d[a], tb = (hi - r.o[a]) / r.d[a];
                            te = std::fmax(te, std::fmin(ta, tb)); tx = std::fmin(tx, std::fmax(ta, tb));
                        }
                        if (miss || tx < te || !(tx > 0.0)) continue;
                        const double ts[2] = {te, tx};
                        for (int q = te > 0.0 ? 0 : 1; q < 2; q++) {
                            if (ts[q] < t1) { t2 = t1; t1 = ts[q]; } else if (ts[q] < t2) t2 = ts[q];
                            nh += 1;
                        }
                    }
                }
                const double t_cell = std::fmin(tm[0], std::fmin(tm[1], tm[2]));
                const int ax = (tm[0] <= tm[1] && tm[0] <= tm[2]) ? 0 : (tm[1] <= tm[2] ? 1 : 2);
                const int nxt = c[ax] + (r.d[ax] < 0 ? -1 : 1);
                if ((nh >= 2 && t2 + m < t_cell) || !(t_cell < INFINITY) || nxt < 0 || nxt >= dims[ax]) break;
                c[ax] = nxt;
                tm[ax] += cell[ax] / std::fabs(r.d[ax]);
            }
            // a trip of the kernel's walk moves a lane on by one cell AND tests one node
            cost.push_back((double)(cells > tests ? cells : tests) + 0.25 * (cells + tests));
        }
        std::sort(cost.begin(), cost.end());
        double sum = 0.0;
        const size_t from = cost.size() - cost.size() / 4;
        for (size_t i = from; i < cost.size(); i++) sum += cost[i];
        return sum / (double)(cost.size() - from);
    };
    double ext[3], vol = 1.0;
    for (int a = 0; a < 3; a++) { ext[a] = g->hi[a] - g->lo[a]; vol *= ext[a]; }
    constexpr int kMaxCells = 512;   // 8 KB of masks in LDS at two words per cell
    {   // start: about one cell per node, as cubic as the extent allows
        const double target = std::fmin((double)kMaxCells, std::fmax(8.0, 1.0 * (N - 1)));
        double side = std::cbrt(vol / target);
        for (int pass = 0; pass < 200; pass++) {
            long long cells = 1;
            for (int a = 0; a < 3; a++) {
                g->n[a] = (int)std::fmin(64.0, std::fmax(1.0, std::floor(ext[a] / side + 0.5)));
                cells *= g->n[a];
            }
            if ((double)cells <= target * 1.25 && cells <= kMaxCells) break;
            side *= 1.05;
        }
    }
    {   // then: each axis in turn, finer or coarser, where the sampled walk gets clearly cheaper
        double best = price(g->n);
        for (int sweep = 0; sweep < 2; sweep++)
            for (int a = 0; a < 3; a++) {
                const int n0 = g->n[a];
                int pick = n0;
                for (int v = std::max(1, n0 / 2); v <= std::min(64, 2 * n0 + 1); v++) {
                    if (v == n0) continue;
                    int dims[3] = {g->n[0], g->n[1], g->n[2]};
                    dims[a] = v;
                    if ((long long)dims[0] * dims[1] * dims[2] > kMaxCells) break;
                    const double p = price(dims);
                    if (p < best * 0.98) { best = p; pick = v; }   // (a clear gain only: ties keep the coarser grid)
                }
                g->n[a] = pick;
            }
    }
    g->words = W;
    g->guard = dev_switch("PVT_GRID_DEV_GUARD") ? -1e30 : m;
    file_nodes(g->n, g->cell, g->masks);
    return true;
}

// Spectra: RN(1/spacing) when EVERY interval of the abscissae has the same bits and the ordinates keep the quotient
// inside div_known's domain (no -0.0, no extreme magnitudes):
double even_rcp(const double* xs, const double* ys, int n) {
    if (n < 2) return NAN;
    const double w = xs[1] - xs[0];
    if (!(w > 1e-100 && w < 1e100)) return NAN;
    for (int i = 1; i + 1 < n; i++) if (xs[i + 1] - xs[i] != w) return NAN;
    for (int i = 0; i < n; i++) {
        if (ys[i] == 0.0 && std::signbit(ys[i])) return NAN;
        if (!(std::fabs(ys[i]) < 1e100)) return NAN;
        if (i > 0 && ys[i] != ys[i - 1] && std::fabs(ys[i] - ys[i - 1]) < 1e-100) return NAN;
    }
    return 1.0 / w;
}

// The spacing itself when, additionally, xs[i] == xs[0] + i*w bit for bit AND the kernel's arithmetic
// (i = int((x - xs[0]) * rcp), one repair step against the computed neighbours) provably lands on the
// reference's bisection index for every x inside the table: the raw index is monotone in x, so it is enough
// that every abscissa and its two neighbouring doubles come out right (checked here with the device's own
// sequence of operations).  Such a table is stored as its first abscissa alone, without a guide table.
double even_w(const double* xs, int n, double rcp) {
    if (!(rcp == rcp) || n < 2 || n > (1 << 24)) return NAN;
    const double w = xs[1] - xs[0];
    auto grid = [&](int i) { volatile double prod = (double)i * w; volatile double at = xs[0] + prod; return (double)at; };
    for (int i = 0; i < n; i++)
        if (grid(i) != xs[i]) return NAN;   // two roundings, never contracted
    auto lands = [&](double x, int want) {
        volatile double diff = x - xs[0];
        volatile double quot = diff * rcp;
        int i = (int)quot;
        i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
        double xlo = grid(i);
        if (x < xlo) { i -= 1; xlo = grid(i); }
        double xhi = grid(i + 1);
        if (!(x < xhi)) { i += 1; xlo = xhi; xhi = grid(i + 1); }
        return i == want && xlo <= x && x < xhi;
    };
    for (int i = 0; i < n; i++) {   // x0 < x < xl is all the even path ever sees
        const double below = std::nextafter(xs[i], -INFINITY), above = std::nextafter(xs[i], INFINITY);
        if (i > 0 && !lands(below, i - 1)) return NAN;
        if (i > 0 && i < n - 1 && !lands(xs[i], i)) return NAN;
        if (i < n - 1 && !lands(above, i)) return NAN;
    }
    return w;
}

// guide[b] = largest i <= n-2 with xs[i] <= xs[0] + b*(xs[n-1]-xs[0])/(n-1), b = 0..n-1; returns the scale the kernel
// maps x to b with (0: no guide)
double build_guide(const double* xs, int n, int* guide) {
    if (n < 2 || !(xs[n - 1] > xs[0])) return 0.0;
    const int Kb = n - 1;
    int i = 0;
    for (int b = 0; b <= Kb; b++) {
        const double edge = xs[0] + (double)b * ((xs[n - 1] - xs[0]) / (double)Kb);
        while (i + 1 <= n - 2 && xs[i + 1] <= edge) i++;
        guide[b] = i;
    }
    return (double)Kb / (xs[n - 1] - xs[0]);
}

// Everything the scene's device tables are made of, derived from PvtSceneTables alone: the fields of PvtScene of the same
// names, the two blobs (gd, gi) and the BVHs of the meshes (the trees of every mesh node, their triangles, their roots).
struct PackedScene {
    Lay lay{};
    std::vector<double> gd;
    std::vector<int> gi;
    int nd_small = 0, ni_small = 0, n_ctab = 0, n_rtab = 0, n_ptab = 0, lazy_root = 0;
    int rough_d = -1;   // where the nodes' GGX widths start in the double blob (-1: no node is rough)
    bool has_frustum = false;   // a node is a truncated cone (PVT_GEOM_FRUSTUM)
    // convex polyhedra (PvtPolyhedronTables): a node is one (PVT_GEOM_POLYHEDRON).  Their plane rows (nx, ny, nz, h) lie
    // BEHIND everything else in the double blob -- the absorbing coatings' block included -- so every other offset is what
    // it would be without them; such a node's record names its rows in its second and third shape parameter (ND_PARAMS + 1:
    // where they start in the double blob, ND_PARAMS + 2: how many, both as integers in the words' bits), which the host tables leave 0
    bool has_polyhedron = false;
    // solids of revolution of a conic (PVT_GEOM_CONICOID): a node is one.  A node record holds three shape parameters and
    // such a node has four, so (L, p0, p1, p2) lie BEHIND everything else in the double blob, the polyhedra's rows
    // included; the node's record keeps L and names the place in its second shape parameter (ND_PARAMS + 1, an integer in
    // the word's bits)
    bool has_conicoid = false;
    // absorbing coatings (PvtCoatingAbsorbTables; -1: no coating absorbs).  Both blocks lie BEHIND everything the blobs of a
    // scene without them hold, so every other offset is what it would be without them, and are read from where the
    // spectra are read.  cabs_d: in the double blob, one record of kCa doubles (kCa*) per coating row, then the pooled
    // tables (wavelengths, angles in radians, values).  dcand_i: in the int blob, the candidate tables of the eighth
    // recorder selector, PVT_RECX_DETECTED -- one block {start, count, bin[6]} per candidate node (NI_CAND; the blocks of
    // Lay::cand_i keep their seven selectors), then the walked lists; `start` is absolute in the int blob
    int cabs_d = -1, dcand_i = -1;
    // scattering coatings (a coating mode word >= PVT_COAT_LOBE; -1: no coating has a lobe): in the int blob, BEHIND everything
    // else it holds -- the `detected` candidate tables included -- one record of kCl ints (kCl*) per coating row: where the
    // reflection lobe's phase table starts in the double blob (-1: a built-in mode) and its axis, the same of the transmission
    int clobe_i = -1;
    // concentration fields (PvtFieldTables): their own buffer of doubles, read from global memory alone (empty: none).
    // fd[n] = where node n's lattice record starts (-1: none), then the records (kFr* words and one value-table offset
    // per component), then the pooled value tables
    std::vector<double> fd;
    // volume maps (PvtMapTables): their own buffer of doubles, read from global memory alone (empty: none).
    // md[n] = where node n's block starts (-1: the node has no map), then the blocks: kMn* words (the node's map count and
    // its world->local rotation and translation) and one record of kMr words (kMr*) per map.  map_slots: the int64 slots
    // the maps add behind the recorders' bins.  path_maps: one of them is a path-length map (PVT_MAP_PATHLENGTH): the scene's
    // launches run the extension family's kExtPath kernels
    std::vector<double> md;
    long long map_slots = 0;
    bool path_maps = false;
    // ray capture (PvtCaptureTables): per recorder the rows it may keep (0: not captured) and its first row, read from
    // global memory alone (empty: no recorder is captured); capture_rows: the rows of all captures of one tally set
    std::vector<long long> cd;
    long long capture_rows = 0;
    // patterned coatings (PvtCoatingPatternTables): their own buffer, uploaded behind the double blob in its allocation and
    // read from global memory alone (both empty: none).
    // pd[2 k] = where coating row k's pattern record starts in pd (-1: the row has no pattern), pd[2 k + 1] != 0: the row's
    // normal test is skipped; then one record of kPr doubles (kPr*) per pattern.  pmask: the pooled masks, uploaded right
    // behind pd -- a record's kPrMask counts bytes from the start of pd
    std::vector<double> pd;
    std::vector<unsigned char> pmask;
    // aligned components (PvtAlignTables): records in `fd` (created when the scene has no lattice): fd[n] of a node that
    // holds one names a record like a lattice's with shape 0, whose kFrComp + k word names the k-th component's record of
    // kAl doubles in fd (-1: that component is not aligned)
    bool aligned = false;
    double lazy_k = 0.0;
    bool exit_observed = false, fuse_exit = false, grid = false, hist_reads_position = false;
    bool hist_reads_counter = false;   // a histogram axis is a photon event counter (PVT_PROPX_EMISSIONS .. _REFLECTIONS)
    int origin_mask = 0;   // bit k: a histogram axis is launch-origin property PVT_PROPX_ORIGIN_WAVELENGTH + k
    bool lean_ok = false;   // see prove_lean: the scene may run the trace_kernel_lean family ...
    bool lean_even = false; // ... and every spectrum its loop reads is a constant or on a proven even grid (its EVEN kernels)
    const char* lean_why = nullptr;   // the first clause of prove_lean that failed (a literal; null when lean_ok)
    bool solo = false;                // see prove_solo: tally launches with a lazy root may run the trace_kernel_solo entries
    const char* solo_why = nullptr;   // the first clause of prove_solo that failed (a literal; null when solo)
    const char* fuse_why = nullptr;   // the first clause of the fused exit's proof that failed (prove_shortcuts; null when fuse_exit)
    int grid_dims[3] = {0, 0, 0};
    std::vector<pvt::BvhNode> bvh_nodes;
    std::vector<pvt::MeshTri> bvh_tris;
    std::vector<int> bvh_roots;
};

// ---- One record of a scene's inputs.  Every pvt_scene_create* entry, pvt_scene_lean_check and the host-buffer path fill
// one and hand it to create_scene / pack_scene: the table structs (t always; the others NULL = the scene has none) and
// what the calling entry KNOWS.  An entry from before an extension keeps refusing what that extension added, with the
// message it always had: a recorder selector beyond Knows::max_selector ("recorder selector out of range"), a histogram
// property beyond max_prop ("histogram property out of range": the kernel reads column `prop` of its tally queue, so an id
// beyond the ones it parks would read past the queue), a geometry type beyond max_geom ("unknown geometry type"), a coating
// mode word beyond max_coat_mode ("coating mode out of range": 1 = the built-in modes alone, the entries from before the
// scattering coatings).
struct Knows {
    int max_selector, max_prop, max_geom;   // the last recorder selector, histogram property and geometry type known
    int max_coat_mode = 1;                  // the largest coat_reflect_mode / coat_transmit_mode word taken
};

struct SceneInputs {
    const PvtSceneTables* t = nullptr;             // the scene tables
    const PvtIndexTables* x = nullptr;             // refractive-index tables n(lambda)
    const PvtPhaseTables* ph = nullptr;            // phase-function tables
    const PvtSurfaceTables* rs = nullptr;          // the nodes' surface roughness
    const PvtFieldTables* fr = nullptr;            // concentration fields
    const PvtMapTables* mp = nullptr;              // volume maps
    const PvtCaptureTables* cp = nullptr;          // ray captures
    const PvtCoatingAbsorbTables* ab = nullptr;    // the coatings' absorptivities
    const PvtCoatingPatternTables* pt = nullptr;   // where the coatings cover
    Knows knows{};
    const PvtAlignTables* al = nullptr;            // aligned components (behind `knows`: the older entries' records stay as written)
    const PvtPolyhedronTables* pl = nullptr;       // convex polyhedra
};

// The levels an entry can know, one row each.  A new entry that knows more gets a new row; nothing else names these limits.
//                                 last selector      last property          last geometry        used by
constexpr Knows kKnowsBeforeAbsorb{PVT_REC_EXIT,      PVT_PROP_Z,            PVT_GEOM_MESH};     // pvt_scene_create .. pvt_scene_create_capture
constexpr Knows kKnowsAbsorb      {PVT_RECX_DETECTED, PVT_PROPX_REFLECTIONS, PVT_GEOM_MESH};     // pvt_scene_create_absorb
constexpr Knows kKnowsOrigin      {PVT_RECX_DETECTED, PVT_PROPX_ORIGIN_Z,    PVT_GEOM_FRUSTUM};  // pvt_scene_create_origin, _pattern, _aligned, pvt_scene_lean_check
constexpr Knows kKnowsPolyhedra   {PVT_RECX_DETECTED, PVT_PROPX_ORIGIN_Z,    PVT_GEOM_CONICOID, 0x7fffffff};  // pvt_scene_create_polyhedra (the polyhedron, the conicoid after it, then the scattering coatings)
constexpr Knows kKnowsHostBuffer  {PVT_REC_EXIT,      PVT_PROP_Z,            PVT_GEOM_FRUSTUM};  // pvt_trace_bundle*: pvt_scene_create, but a truncated cone is taken

// ---- validation: every index into a table that the packer follows on the host or the kernel on the device, checked
// before anything else is read.  One function per table struct; validate_tables calls them in the order that decides
// which refusal a scene with two faults meets.
// n values, finite and strictly increasing
bool increasing_finite(const double* v, long long n) {
    for (long long i = 0; i < n; i++)
        if (!std::isfinite(v[i]) || (i > 0 && !(v[i] > v[i - 1]))) return false;
    return true;
}
// n angles in [0, 90] degrees, strictly increasing
bool increasing_angles(const double* v, long long n) {
    for (long long i = 0; i < n; i++)
        if (!(v[i] >= 0.0 && v[i] <= 90.0) || (i > 0 && !(v[i] > v[i - 1]))) return false;
    return true;
}
// n values in [0, 1] (a NaN is not)
bool within_unit(const double* v, long long n) {
    for (long long i = 0; i < n; i++)
        if (!(v[i] >= 0.0 && v[i] <= 1.0)) return false;
    return true;
}
// runs [start, start + count) into a table of `size` rows
bool bad_run(long long start, long long count, long long size) { return count < 0 || start < 0 || start + count > size; }

// Tables of values on a wavelength x angle grid, pooled: the coating reflectivity tables of PvtSceneTables and the
// absorptivity tables of PvtCoatingAbsorbTables are the same thing under different field names.
struct GridTables {
    int n_tables;
    const int32_t *nw, *na, *wl_start, *angle_start, *value_start;
    long long n_wavelength, n_angle, n_value;
    const double *wavelength, *angle, *value;
    long long doubles(int j) const { return (long long)nw[j] + na[j] + (long long)nw[j] * na[j]; }
};
GridTables grid_tables(const PvtSceneTables* t) {
    return {t->n_coat_tables, t->ctab_nw, t->ctab_na, t->ctab_wl_start, t->ctab_angle_start, t->ctab_value_start,
            t->n_ctab_wavelength, t->n_ctab_angle, t->n_ctab_value, t->ctab_wavelength, t->ctab_angle, t->ctab_value};
}
GridTables grid_tables(const PvtCoatingAbsorbTables* ab) {
    return {ab->n_tables, ab->table_nw, ab->table_na, ab->wl_start, ab->angle_start, ab->value_start,
            ab->n_wavelength, ab->n_angle, ab->n_value, ab->wavelength, ab->angle, ab->value};
}
struct GridMessages { const char *range, *wavelengths, *angles, *values, *total; };
// Every table's ranges, axes and values, then the doubles of all of them (`total`: what the caller places besides)
int validate_grid_tables(const GridTables& g, long long total, const GridMessages& m) {
    for (int j = 0; j < g.n_tables; j++) {
        const long long nw = g.nw[j], na = g.na[j];
        const long long w0 = g.wl_start[j], a0 = g.angle_start[j], v0 = g.value_start[j];
        if (nw < 1 || na < 1 || w0 < 0 || a0 < 0 || v0 < 0 || w0 + nw > g.n_wavelength || a0 + na > g.n_angle ||
            v0 + nw * na > g.n_value)
            return fail(PVT_ERR_INVALID, m.range);
        if (!increasing_finite(g.wavelength + w0, nw)) return fail(PVT_ERR_INVALID, m.wavelengths);
        if (!increasing_angles(g.angle + a0, na)) return fail(PVT_ERR_INVALID, m.angles);
        if (!within_unit(g.value + v0, nw * na)) return fail(PVT_ERR_INVALID, m.values);
        total += nw + na + nw * na;
    }
    if (total > (1ll << 27)) return fail(PVT_ERR_INVALID, m.total);
    return PVT_OK;
}
// Table j where the blob keeps it, at d: wavelengths (nm), angles (radians: the kernel compares pvt_acos of the cosine),
// values -- GridTables::doubles(j) doubles
void put_grid_table(const GridTables& g, int j, double* d) {
    constexpr double kRadPerDeg = 3.14159265358979323846 / 180.0;
    const int nw = g.nw[j], na = g.na[j];
    for (int i = 0; i < nw; i++) d[i] = g.wavelength[g.wl_start[j] + i];
    for (int i = 0; i < na; i++) d[nw + i] = g.angle[g.angle_start[j] + i] * kRadPerDeg;
    for (int i = 0; i < na * nw; i++) d[nw + na + i] = g.value[g.value_start[j] + i];
}

// A conicoid's ends (include/pvtrace_hip.h): the Horner values of q at -half and +half and the slack 2^-40 * S, with the
// operations of geometry.Conicoid._ends
struct ConicoidEnds { double half, q_lo, q_hi, slack; };
ConicoidEnds conicoid_ends(const double* gp) {
    const double L = gp[0], p0 = gp[1], p1 = gp[2], p2 = gp[3];
    const double half = 0.5 * L;
    const double S = (std::fabs(p0) + std::fabs(p1) * half) + (std::fabs(p2) * half) * half;
    return {half, p0 + (p1 + p2 * (-half)) * (-half), p0 + (p1 + p2 * half) * half, 0x1p-40 * S};
}
// What is wrong with (L, p0, p1, p2), or null: geometry.Conicoid.parameter_problem, test for test and word for word
const char* conicoid_problem(const double* gp) {
    const double L = gp[0], p0 = gp[1], p1 = gp[2], p2 = gp[3];
    if (!(std::isfinite(L) && std::isfinite(p0) && std::isfinite(p1) && std::isfinite(p2)))
        return "conicoid: length and profile (p0, p1, p2) must be finite numbers";
    if (!(L > 0.0)) return "conicoid: length must be > 0";
    const ConicoidEnds e = conicoid_ends(gp);
    bool inside = p0 > 0.0;
    if (p2 > 0.0) {
        const double zv = -0.5 * p1 / p2;
        if (-e.half < zv && zv < e.half && !(p0 + (p1 + p2 * zv) * zv > e.slack)) inside = false;
    }
    if (!inside) return "conicoid: q(z) must be > 0 inside (-L/2, L/2): the solid has no interior or is pinched";
    if (e.q_lo < -e.slack || e.q_hi < -e.slack) return "conicoid: q(z) is negative at an end";
    if (p1 * p1 - 4.0 * p0 * p2 < -0x1p-40 * (p1 * p1 + 4.0 * std::fabs(p0 * p2)))
        return "conicoid: the solid is not convex (p1*p1 - 4*p0*p2 < 0: sqrt(q) is not concave)";
    return nullptr;
}

// the core tables, first part: the root, the geometry of every node and the meshes
int validate_nodes(const PvtSceneTables* t, const Knows& knows) {
    const int N = t->n_nodes;
    if (t->root_id < 0 || t->root_id >= N) return fail(PVT_ERR_INVALID, "root node out of range");
    for (int n = 0; n < N; n++) {
        const int g = t->geom_type[n];
        if (g < PVT_GEOM_BOX || g > knows.max_geom) return fail(PVT_ERR_INVALID, "unknown geometry type");
        if (g == PVT_GEOM_FRUSTUM) {   // (length, radius_bottom, radius_top): the kernel divides by the first
            const double* gp = t->geom_params + n * 4;
            if (!(std::isfinite(gp[0]) && gp[0] > 0.0)) return fail(PVT_ERR_INVALID, "frustum: length must be finite and > 0");
            if (!(std::isfinite(gp[1]) && std::isfinite(gp[2]) && gp[1] >= 0.0 && gp[2] >= 0.0))
                return fail(PVT_ERR_INVALID, "frustum: radii must be finite and >= 0");
            if (gp[1] == 0.0 && gp[2] == 0.0) return fail(PVT_ERR_INVALID, "frustum: radii must not both be 0");
        }
        if (g == PVT_GEOM_CONICOID) {   // (L, p0, p1, p2): the rules and the messages of geometry.Conicoid.parameter_problem
            const char* problem = conicoid_problem(t->geom_params + n * 4);
            if (problem) return fail(PVT_ERR_INVALID, problem);
        }
        if (g != PVT_GEOM_MESH) continue;
        if (!t->mesh_face_start || !t->mesh_face_count || !t->mesh_vertices || !t->mesh_faces || !t->mesh_normals)
            return fail(PVT_ERR_INVALID, "mesh node without mesh tables");
        const long long f0 = t->mesh_face_start[n], fc = t->mesh_face_count[n];
        if (fc <= 0 || f0 < 0 || f0 + fc > t->n_mesh_faces) return fail(PVT_ERR_INVALID, "mesh face range out of bounds");
        if (t->n_mesh_faces >= (1 << 27)) return fail(PVT_ERR_INVALID, "more than 2^27 mesh faces in one scene");
        for (long long k = 3 * f0; k < 3 * (f0 + fc); k++)
            if (t->mesh_faces[k] < 0 || t->mesh_faces[k] >= t->n_mesh_vertices)
                return fail(PVT_ERR_INVALID, "mesh face indexes a missing vertex");
    }
    return PVT_OK;
}

// coating reflectivity tables (the fields appended to the v13 struct)
int validate_coating_tables(const PvtSceneTables* t) {
    const int K = t->n_coatings, NT = t->n_coat_tables;
    if (K <= 0 || NT == 0) return PVT_OK;
    if (NT < 0 || !t->coat_table || !t->ctab_nw || !t->ctab_na || !t->ctab_wl_start || !t->ctab_angle_start ||
        !t->ctab_value_start || !t->ctab_wavelength || !t->ctab_angle || !t->ctab_value)
        return fail(PVT_ERR_INVALID, "coating tables: missing arrays");
    const int rc = validate_grid_tables(grid_tables(t), 0,
                                        {"coating tables: axis or value range out of bounds",
                                         "coating tables: wavelengths must be finite and strictly increasing",
                                         "coating tables: angles must be strictly increasing, in [0, 90] degrees",
                                         "coating tables: values must be in [0, 1]",
                                         "coating tables: more than 2^27 doubles"});
    if (rc != PVT_OK) return rc;
    for (int k = 0; k < K; k++)
        if (t->coat_table[k] < -1 || t->coat_table[k] >= NT) return fail(PVT_ERR_INVALID, "coating row names a missing table");
    return PVT_OK;
}

// the nodes' refractive indices
int validate_indices(const PvtSceneTables* t) {
    for (int n = 0; n < t->n_nodes; n++) {   // (the known-divisor division is proven for these)
        const double v = t->refractive_index[n];
        if (!(std::isfinite(v) && v > 1e-100 && v < 1e100)) return fail(PVT_ERR_INVALID, "refractive indices must be finite and positive");
    }
    return PVT_OK;
}

// refractive-index tables n(lambda) (PvtIndexTables, pvt_scene_create_ex)
int validate_index_tables(const PvtSceneTables* t, const PvtIndexTables* x) {
    if (!x || x->n_tables == 0) return PVT_OK;
    const int N = t->n_nodes, NT = x->n_tables;
    if (NT < 0 || !x->node_table || !x->table_n || !x->table_start || !x->wavelength || !x->value)
        return fail(PVT_ERR_INVALID, "index tables: missing arrays");
    for (int n = 0; n < N; n++)
        if (x->node_table[n] < -1 || x->node_table[n] >= NT) return fail(PVT_ERR_INVALID, "index tables: node names a missing table");
    long long total = 0;
    for (int j = 0; j < NT; j++) {
        const long long np = x->table_n[j], p0 = x->table_start[j];
        if (np < 1 || p0 < 0 || p0 + np > x->n_points) return fail(PVT_ERR_INVALID, "index tables: point range out of bounds");
        if (!increasing_finite(x->wavelength + p0, np))
            return fail(PVT_ERR_INVALID, "index tables: wavelengths must be finite and strictly increasing");
        for (long long i = 0; i < np; i++) {   // (the bounds of the scalar indices: the lanes divide by these)
            const double v = x->value[p0 + i];
            if (!(std::isfinite(v) && v > 1e-100 && v < 1e100)) return fail(PVT_ERR_INVALID, "index tables: values must be finite and positive, in (1e-100, 1e100)");
        }
        total += 2 * np;
    }
    if (total > (1ll << 27)) return fail(PVT_ERR_INVALID, "index tables: more than 2^27 doubles");
    return PVT_OK;
}

// phase-function tables (PvtPhaseTables, pvt_scene_create_phase): a component tagged PVT_PHASE_TABLE names one, and
// only such a component does; without the struct the tag is refused
int validate_phase_tables(const PvtSceneTables* t, const PvtPhaseTables* ph) {
    const int C = t->n_components;
    const int NP = ph ? ph->n_tables : 0;
    if (NP < 0 || (NP > 0 && (!ph->comp_table || !ph->table_nw || !ph->table_nmu || !ph->wl_start || !ph->mu_start ||
                              !ph->cdf_start || !ph->wavelength || !ph->mu || !ph->cdf)))
        return fail(PVT_ERR_INVALID, "phase tables: missing arrays");
    for (int c = 0; c < C; c++) {
        const bool tagged = t->comp_phase_type[c] == PVT_PHASE_TABLE;
        if (tagged && NP == 0)
            return fail(PVT_ERR_INVALID, "a component has a tabulated phase function (PVT_PHASE_TABLE): pass its tables to pvt_scene_create_phase");
        if (NP > 0 && (ph->comp_table[c] < -1 || ph->comp_table[c] >= NP)) return fail(PVT_ERR_INVALID, "phase tables: component names a missing table");
        if (NP > 0 && tagged != (ph->comp_table[c] >= 0))
            return fail(PVT_ERR_INVALID, "phase tables: a component names a table exactly when it is tagged PVT_PHASE_TABLE");
    }
    long long total = 0;
    for (int j = 0; j < NP; j++) {
        const long long nw = ph->table_nw[j], nm = ph->table_nmu[j];
        const long long w0 = ph->wl_start[j], m0 = ph->mu_start[j], c0 = ph->cdf_start[j];
        if (nw < 1 || nm < 2 || w0 < 0 || m0 < 0 || c0 < 0 || w0 + nw > ph->n_wavelength || m0 + nm > ph->n_points ||
            c0 + nw * nm > ph->n_cdf)
            return fail(PVT_ERR_INVALID, "phase tables: wavelength, mu or CDF range out of bounds");
        if (!increasing_finite(ph->wavelength + w0, nw))
            return fail(PVT_ERR_INVALID, "phase tables: wavelengths must be finite and strictly increasing");
        const double* mu = ph->mu + m0;
        if (mu[0] != -1.0 || mu[nm - 1] != 1.0) return fail(PVT_ERR_INVALID, "phase tables: the mu axis must run from exactly -1 to exactly 1");
        for (long long i = 1; i < nm; i++)
            if (!(mu[i] > mu[i - 1])) return fail(PVT_ERR_INVALID, "phase tables: the mu axis must be strictly increasing");
        for (long long r = 0; r < nw; r++) {
            const double* cdf = ph->cdf + c0 + r * nm;
            if (cdf[0] != 0.0 || cdf[nm - 1] != 1.0) return fail(PVT_ERR_INVALID, "phase tables: every CDF row must run from exactly 0 to exactly 1");
            for (long long i = 1; i < nm; i++)
                if (!(cdf[i] >= cdf[i - 1])) return fail(PVT_ERR_INVALID, "phase tables: every CDF row must be non-decreasing");
        }
        total += 2 + nw + nm + nw * nm;
    }
    if (total > (1ll << 27)) return fail(PVT_ERR_INVALID, "phase tables: more than 2^27 doubles");
    return PVT_OK;
}

// the emitter and its tabulated sources (PvtSourceTables, pvt_scene_set_sources; `src` null: pvt_scene_set_emitter, which
// knows the built-in type words only).  A light names a grid exactly when it is tagged PVT_POS_GRID, a table exactly when
// it is tagged PVT_DIR_TABLE; the grids' messages are the Python PositionGrid's
constexpr long long kSourceGridCells = 1ll << 22;
int validate_sources(const PvtEmitterTables* e, const PvtSourceTables* src) {
    if (!e || e->n_lights <= 0) return fail(PVT_ERR_INVALID, "bad emitter");
    const int Lt = e->n_lights;
    if (!e->wl_type || !e->pos_type || !e->dir_type) return fail(PVT_ERR_INVALID, "emitter: missing arrays");
    const int pos_top = src ? PVT_POS_GRID : PVT_POS_CUBE, dir_top = src ? PVT_DIR_TABLE : PVT_DIR_HG;
    for (int i = 0; i < Lt; i++)
        if (e->wl_type[i] < 0 || e->wl_type[i] > PVT_WL_SPECTRUM_HIST || e->pos_type[i] < 0 || e->pos_type[i] > pos_top ||
            e->dir_type[i] < 0 || e->dir_type[i] > dir_top)
            return fail(PVT_ERR_INVALID, "emitter type out of range");
    if (!src) return PVT_OK;
    if (!e->wl_value || !e->pos_param || !e->dir_param || !e->light_to_world) return fail(PVT_ERR_INVALID, "emitter: missing arrays");
    const int G = src->n_grids, T = src->n_tables;
    if (src->n_lights != Lt || !src->light_grid || !src->light_table)
        return fail(PVT_ERR_INVALID, "source tables: need one grid and one table index per light");
    if (G < 0 || T < 0 || (G > 0 && (!src->grid_shape || !src->grid_bounded || !src->grid_lower || !src->grid_h ||
                                     !src->grid_cdf_start || !src->grid_cdf)) ||
        (T > 0 && (!src->table_nw || !src->table_nmu || !src->table_wl_start || !src->table_mu_start || !src->table_cdf_start ||
                   !src->table_wavelength || !src->table_mu || !src->table_cdf)))
        return fail(PVT_ERR_INVALID, "source tables: missing arrays");
    for (int i = 0; i < Lt; i++) {
        const int g = src->light_grid[i], t = src->light_table[i];
        if (g < -1 || g >= G) return fail(PVT_ERR_INVALID, "source tables: light names a missing grid");
        if (t < -1 || t >= T) return fail(PVT_ERR_INVALID, "source tables: light names a missing table");
        if ((e->pos_type[i] == PVT_POS_GRID) != (g >= 0))
            return fail(PVT_ERR_INVALID, "source tables: a light names a grid exactly when it is tagged PVT_POS_GRID");
        if ((e->dir_type[i] == PVT_DIR_TABLE) != (t >= 0))
            return fail(PVT_ERR_INVALID, "source tables: a light names a table exactly when it is tagged PVT_DIR_TABLE");
    }
    long long total = 0;
    for (int g = 0; g < G; g++) {
        long long cells = 1;
        for (int a = 0; a < 3; a++) {
            const long long n = src->grid_shape[g * 3 + a];
            if (n < 1) return fail(PVT_ERR_INVALID, "position grid: shape must be >= 1 on each axis");
            cells *= n;
            if (cells > kSourceGridCells) return fail(PVT_ERR_INVALID, "position grid: more than 2^22 cells");
            const double lo = src->grid_lower[g * 3 + a], h = src->grid_h[g * 3 + a];
            if (src->grid_bounded[g * 3 + a] == 0) {
                if (n != 1) return fail(PVT_ERR_INVALID, "position grid: only an axis with one cell may be unbounded");
                continue;
            }
            if (!(std::isfinite(lo) && std::isfinite(h))) return fail(PVT_ERR_INVALID, "position grid: lower and upper must be finite");
            if (!(h > 0.0)) return fail(PVT_ERR_INVALID, "position grid: needs lower < upper on each axis");
        }
        const long long c0 = src->grid_cdf_start[g];
        if (c0 < 0 || c0 + cells + 1 > src->n_grid_cdf) return fail(PVT_ERR_INVALID, "position grid: CDF range out of bounds");
        const double* cdf = src->grid_cdf + c0;
        for (long long k = 0; k <= cells; k++)
            if (!std::isfinite(cdf[k]) || (k > 0 && !(cdf[k] >= cdf[k - 1])))
                return fail(PVT_ERR_INVALID, "position grid: weights must be finite and >= 0");
        if (cdf[0] != 0.0 || cdf[cells] != 1.0)
            return fail(PVT_ERR_INVALID, "position grid: the CDF must run from exactly 0 to exactly 1");
        total += kSgCdf + cells + 1;
    }
    for (int j = 0; j < T; j++) {
        const long long nw = src->table_nw[j], nm = src->table_nmu[j];
        const long long w0 = src->table_wl_start[j], m0 = src->table_mu_start[j], c0 = src->table_cdf_start[j];
        if (nw < 1 || nm < 2 || w0 < 0 || m0 < 0 || c0 < 0 || w0 + nw > src->n_table_wavelength || m0 + nm > src->n_table_mu ||
            c0 + nw * nm > src->n_table_cdf)
            return fail(PVT_ERR_INVALID, "direction table: wavelength, mu or CDF range out of bounds");
        if (!increasing_finite(src->table_wavelength + w0, nw))
            return fail(PVT_ERR_INVALID, "direction table: wavelengths must be finite and strictly increasing");
        const double* mu = src->table_mu + m0;
        if (mu[0] != -1.0 || mu[nm - 1] != 1.0) return fail(PVT_ERR_INVALID, "direction table: the mu axis must run from exactly -1 to exactly 1");
        for (long long i = 1; i < nm; i++)
            if (!(mu[i] > mu[i - 1])) return fail(PVT_ERR_INVALID, "direction table: the mu axis must be strictly increasing");
        for (long long r = 0; r < nw; r++) {
            const double* cdf = src->table_cdf + c0 + r * nm;
            if (cdf[0] != 0.0 || cdf[nm - 1] != 1.0) return fail(PVT_ERR_INVALID, "direction table: every CDF row must run from exactly 0 to exactly 1");
            for (long long i = 1; i < nm; i++)
                if (!(cdf[i] >= cdf[i - 1])) return fail(PVT_ERR_INVALID, "direction table: every CDF row must be non-decreasing");
        }
        total += 2 + nw + nm + nw * nm;
    }
    if (total > (1ll << 27)) return fail(PVT_ERR_INVALID, "source tables: more than 2^27 doubles");
    return PVT_OK;
}

// rough interfaces (PvtSurfaceTables, pvt_scene_create_rough): one finite GGX width 0 <= alpha <= 1 per node
int validate_surface_tables(const PvtSceneTables* t, const PvtSurfaceTables* rs) {
    if (!rs || rs->n_nodes == 0) return PVT_OK;
    const int N = t->n_nodes;
    if (rs->n_nodes != N || !rs->node_roughness) return fail(PVT_ERR_INVALID, "surface tables: need one roughness per node");
    if (!within_unit(rs->node_roughness, N)) return fail(PVT_ERR_INVALID, "surface tables: roughness must be finite and within [0, 1]");
    return PVT_OK;
}

// concentration fields (PvtFieldTables, pvt_scene_create_field): lattices, value tables and who uses which
int validate_field_tables(const PvtSceneTables* t, const PvtFieldTables* fr) {
    if (!fr || fr->n_nodes == 0) return PVT_OK;
    const int N = t->n_nodes, C = t->n_components;
    const int F = fr->n_fields, V = fr->n_values;
    if (fr->n_nodes != N || !fr->node_field) return fail(PVT_ERR_INVALID, "field tables: need one lattice index per node");
    if (F < 0 || (F > 0 && (!fr->field_shape || !fr->field_lower || !fr->field_upper)))
        return fail(PVT_ERR_INVALID, "field tables: lattice arrays missing");
    for (int n = 0; n < N; n++)
        if (fr->node_field[n] < -1 || fr->node_field[n] >= F) return fail(PVT_ERR_INVALID, "field tables: lattice index out of range");
    if (fr->node_field[t->root_id] >= 0) return fail(PVT_ERR_INVALID, "field tables: the root node cannot carry a lattice");
    for (int f = 0; f < F; f++)
        for (int a = 0; a < 3; a++) {
            if (fr->field_shape[f * 3 + a] < 1) return fail(PVT_ERR_INVALID, "field tables: lattice shape must be >= 1 on each axis");
            const double lo = fr->field_lower[f * 3 + a], hi = fr->field_upper[f * 3 + a];
            if (!(std::isfinite(lo) && std::isfinite(hi))) return fail(PVT_ERR_INVALID, "field tables: lattice bounds must be finite");
            if (!(lo < hi)) return fail(PVT_ERR_INVALID, "field tables: lattice lower must be < upper on each axis");
        }
    if (fr->n_components != C || (C > 0 && !fr->comp_values))
        return fail(PVT_ERR_INVALID, "field tables: need one value-table index per component");
    if (V < 0 || fr->n_points < 0 || (V > 0 && (!fr->values_start || !fr->values_count)) || (fr->n_points > 0 && !fr->values))
        return fail(PVT_ERR_INVALID, "field tables: value-table arrays missing");
    for (int c = 0; c < C; c++)
        if (fr->comp_values[c] < -1 || fr->comp_values[c] >= V) return fail(PVT_ERR_INVALID, "field tables: value-table index out of range");
    for (int v = 0; v < V; v++)
        if (bad_run(fr->values_start[v], fr->values_count[v], fr->n_points) || fr->values_count[v] < 1)
            return fail(PVT_ERR_INVALID, "field tables: value-table run out of range");
    for (int i = 0; i < fr->n_points; i++)
        if (!std::isfinite(fr->values[i])) return fail(PVT_ERR_INVALID, "field tables: values must be finite");
    for (int i = 0; i < fr->n_points; i++)
        if (fr->values[i] < 0.0) return fail(PVT_ERR_INVALID, "field tables: values must be >= 0");
    // every component of a node with a lattice names a value table of exactly that lattice's size; the buffer the
    // kernel indexes with int stays within int32
    long long words = N;
    for (int n = 0; n < N; n++) {
        const int f = fr->node_field[n];
        if (f < 0) continue;
        const long long cells = (long long)fr->field_shape[f * 3] * fr->field_shape[f * 3 + 1] * fr->field_shape[f * 3 + 2];
        if (cells > 0x7fffffffLL) return fail(PVT_ERR_INVALID, "field tables: a lattice of more than 2^31 - 1 cells");
        words += kFrComp + t->comp_count[n];
        for (int k = 0; k < t->comp_count[n]; k++) {
            const int c = t->comp_start[n] + k;
            if (c < 0 || c >= C) return fail(PVT_ERR_INVALID, "component run out of range");
            const int v = fr->comp_values[c];
            if (v < 0) return fail(PVT_ERR_INVALID, "field tables: every component of a node with a lattice needs values");
            if (fr->values_count[v] != cells)
                return fail(PVT_ERR_INVALID, "field tables: a value table's length must equal its node's lattice size");
        }
    }
    words += fr->n_points;
    if (words > 0x7fffffffLL) return fail(PVT_ERR_INVALID, "field tables: more doubles than int32 offsets can index");
    return PVT_OK;
}

// volume maps (PvtMapTables, pvt_scene_create_maps): whose maps they are, what they count and where
int validate_map_tables(const PvtSceneTables* t, const PvtMapTables* mp) {
    if (!mp || mp->n_nodes == 0 || mp->n_maps == 0) return PVT_OK;
    const int N = t->n_nodes, C = t->n_components, M = mp->n_maps;
    if (mp->n_nodes != N || !mp->node_map_start || !mp->node_map_count)
        return fail(PVT_ERR_INVALID, "map tables: need one map run per node");
    if (M < 0 || !mp->map_kind || !mp->map_component || !mp->map_shape || !mp->map_lower || !mp->map_h || !mp->map_nw ||
        !mp->map_wl_start || !mp->map_wl_stop || !mp->map_offset)
        return fail(PVT_ERR_INVALID, "map tables: map arrays missing");
    long long next = 0;
    for (int n = 0; n < N; n++) {
        if (bad_run(mp->node_map_start[n], mp->node_map_count[n], M)) return fail(PVT_ERR_INVALID, "map tables: map run of a node out of range");
        if (mp->node_map_start[n] != next) return fail(PVT_ERR_INVALID, "map tables: the nodes' map runs must tile the maps in node order");
        next += mp->node_map_count[n];
    }
    if (next != M) return fail(PVT_ERR_INVALID, "map tables: the nodes' map runs must tile the maps in node order");
    if (mp->node_map_count[t->root_id] > 0) return fail(PVT_ERR_INVALID, "map tables: the root node cannot carry a map");
    long long slots = 0;
    for (int n = 0; n < N; n++)
        for (int m = mp->node_map_start[n]; m < mp->node_map_start[n] + mp->node_map_count[n]; m++) {
            const int kind = mp->map_kind[m];
            if (kind != PVT_EV_ABSORB && kind != PVT_EV_EMIT && kind != PVT_EV_SCATTER && kind != PVT_EV_NONRADIATIVE && kind != PVT_EV_REACT &&
                kind != PVT_MAP_PATHLENGTH)
                return fail(PVT_ERR_INVALID, "map tables: map kind must be ABSORB, EMIT, SCATTER, NONRADIATIVE, REACT or PVT_MAP_PATHLENGTH");
            const int c = mp->map_component[m];
            if (kind == PVT_MAP_PATHLENGTH && c != -1)
                return fail(PVT_ERR_INVALID, "map tables: a path-length map takes no component filter (map_component must be -1)");
            if (c < -1 || (c >= 0 && (bad_run(t->comp_start[n], t->comp_count[n], C) || c < t->comp_start[n] || c >= t->comp_start[n] + t->comp_count[n])))
                return fail(PVT_ERR_INVALID, "map tables: map component must be -1 or a component of the map's node");
            long long cells = 1;
            for (int a = 0; a < 3; a++) {
                if (mp->map_shape[m * 3 + a] < 1) return fail(PVT_ERR_INVALID, "map tables: map shape must be >= 1 on each axis");
                if (!std::isfinite(mp->map_lower[m * 3 + a])) return fail(PVT_ERR_INVALID, "map tables: map lower bounds must be finite");
                const double h = mp->map_h[m * 3 + a];
                if (!(std::isfinite(h) && h > 0.0)) return fail(PVT_ERR_INVALID, "map tables: map cell widths must be finite and > 0");
                cells *= mp->map_shape[m * 3 + a];
                if (cells > PVT_MAX_MAP_SLOTS) return fail(PVT_ERR_INVALID, "map tables: more than 2^26 map slots");
            }
            const int nw = mp->map_nw[m];
            if (nw < 0) return fail(PVT_ERR_INVALID, "map tables: wavelength bins must be >= 0");
            if (nw > 0) {
                const double lo = mp->map_wl_start[m], hi = mp->map_wl_stop[m];
                if (!(std::isfinite(lo) && std::isfinite(hi))) return fail(PVT_ERR_INVALID, "map tables: wavelength range must be finite");
                if (!(lo < hi)) return fail(PVT_ERR_INVALID, "map tables: wavelength range needs start < stop");
                cells *= nw;
            }
            if (mp->map_offset[m] != slots) return fail(PVT_ERR_INVALID, "map tables: map offsets must pack the maps one after the other");
            slots += cells + 1;
            if (slots > PVT_MAX_MAP_SLOTS) return fail(PVT_ERR_INVALID, "map tables: more than 2^26 map slots");
        }
    if (mp->map_slots != slots) return fail(PVT_ERR_INVALID, "map tables: map_slots must be the sum of the maps' slots");
    return PVT_OK;
}

// ray capture (PvtCaptureTables, pvt_scene_create_capture): how many rows each recorder keeps and where
int validate_capture_tables(const PvtSceneTables* t, const PvtCaptureTables* cp) {
    if (!cp || cp->n_recorders == 0 || cp->capture_rows == 0) return PVT_OK;
    const int R = t->n_recorders;
    if (cp->n_recorders != R) return fail(PVT_ERR_INVALID, "capture tables: need one capacity per recorder");
    if (!cp->rec_capture_capacity || !cp->rec_capture_start) return fail(PVT_ERR_INVALID, "capture tables: capture arrays missing");
    long long rows = 0;
    for (int r = 0; r < R; r++) {
        const long long cap = cp->rec_capture_capacity[r];
        if (cap < 0) return fail(PVT_ERR_INVALID, "capture tables: a capacity must be >= 0");
        if (cap > PVT_MAX_CAPTURE_ROWS) return fail(PVT_ERR_INVALID, "capture tables: more than 2^24 capture rows");
        if (cp->rec_capture_start[r] != rows) return fail(PVT_ERR_INVALID, "capture tables: capture starts must pack the captures one after the other");
        rows += cap;
        if (rows > PVT_MAX_CAPTURE_ROWS) return fail(PVT_ERR_INVALID, "capture tables: more than 2^24 capture rows");
    }
    if (cp->capture_rows != rows) return fail(PVT_ERR_INVALID, "capture tables: capture_rows must be the sum of the capacities");
    return PVT_OK;
}

// absorbing coatings (PvtCoatingAbsorbTables, pvt_scene_create_absorb): a scalar A per coating row, tables for some
int validate_absorb_tables(const PvtSceneTables* t, const PvtCoatingAbsorbTables* ab) {
    if (!ab || ab->n_coatings == 0) return PVT_OK;
    const int K = t->n_coatings;
    if (ab->n_coatings != K || !ab->coat_absorptivity) return fail(PVT_ERR_INVALID, "absorb tables: need one absorptivity per coating");
    for (int k = 0; k < K; k++) {
        const double a = ab->coat_absorptivity[k];
        if (!std::isfinite(a)) return fail(PVT_ERR_INVALID, "absorb tables: absorptivity must be finite");
        if (!(a >= 0.0 && a <= 1.0)) return fail(PVT_ERR_INVALID, "absorb tables: absorptivity must be within [0, 1]");
    }
    const int NT = ab->n_tables;
    if (NT < 0 || (NT > 0 && (!ab->coat_table || !ab->table_nw || !ab->table_na || !ab->wl_start || !ab->angle_start ||
                              !ab->value_start || !ab->wavelength || !ab->angle || !ab->value)))
        return fail(PVT_ERR_INVALID, "absorb tables: missing arrays");
    const int rc = validate_grid_tables(grid_tables(ab), (long long)K * kCa,
                                        {"absorb tables: axis or value range out of bounds",
                                         "absorb tables: wavelengths must be finite and strictly increasing",
                                         "absorb tables: angles must be strictly increasing, in [0, 90] degrees",
                                         "absorb tables: values must be finite and within [0, 1]",
                                         "absorb tables: more than 2^27 doubles"});
    if (rc != PVT_OK) return rc;
    for (int k = 0; k < K && NT > 0; k++)
        if (ab->coat_table[k] < -1 || ab->coat_table[k] >= NT) return fail(PVT_ERR_INVALID, "absorb tables: coating row names a missing table");
    return PVT_OK;
}

// the core tables, last part: the ranges of components, coatings, spectra, recorders and histograms
int validate_ranges(const PvtSceneTables* t, const Knows& knows) {
    const int N = t->n_nodes, C = t->n_components, R = t->n_recorders, H = t->n_hists, K = t->n_coatings;
    for (int n = 0; n < N; n++) {
        if (bad_run(t->comp_start[n], t->comp_count[n], C)) return fail(PVT_ERR_INVALID, "component range of a node out of bounds");
        if (K > 0 && bad_run(t->coat_start[n], t->coat_count[n], K)) return fail(PVT_ERR_INVALID, "coating range of a node out of bounds");
    }
    for (int c = 0; c < C; c++) {
        if (bad_run(t->comp_abs_start[c], t->comp_abs_n[c], t->n_abs))
            return fail(PVT_ERR_INVALID, "absorption spectrum range of a component out of bounds");
        if (bad_run(t->comp_ems_start[c], t->comp_ems_n[c], t->n_ems))
            return fail(PVT_ERR_INVALID, "emission spectrum range of a component out of bounds");
    }
    for (int r = 0; r < R; r++) {
        if (t->rec_node[r] < 0 || t->rec_node[r] >= N) return fail(PVT_ERR_INVALID, "recorder on a missing node");
        if (t->rec_event[r] < 0 || t->rec_event[r] > knows.max_selector) return fail(PVT_ERR_INVALID, "recorder selector out of range");
        if (bad_run(t->rec_hist_start[r], t->rec_hist_n[r], H)) return fail(PVT_ERR_INVALID, "histogram range of a recorder out of bounds");
    }
    for (int h = 0; h < H; h++)
        if (t->hist_prop_a[h] < 0 || t->hist_prop_a[h] > knows.max_prop || t->hist_prop_b[h] < -1 || t->hist_prop_b[h] > knows.max_prop)
            return fail(PVT_ERR_INVALID, "histogram property out of range");
    for (int h = 0; h < H; h++) {   // bins hist_offset + [0, na) (1-D) or + [0, na * nb) (2-D) of the tally
        const long long bins = (long long)std::max(t->hist_na[h], 0) * (t->hist_prop_b[h] >= 0 ? std::max(t->hist_nb[h], 0) : 1);
        if (bins > 0 && bad_run(t->hist_offset[h], bins, t->total_bins)) return fail(PVT_ERR_INVALID, "histogram bins out of range of total_bins");
    }
    return PVT_OK;
}

// The order is behaviour: the first check that fails names the refusal.  The core tables are checked in two parts, around
// the extension structs.  (Pattern tables are checked by pack_patterns, on a scene pack_scene has accepted.)
// the coatings' mode words: a built-in mode, or -- for an entry that takes them -- a lobe (PVT_COAT_LOBE + 4 table + axis)
// whose table lies in the phase tables (validated before this) and whose axis is one its slot takes
int validate_coating_modes(const SceneInputs& in) {
    const PvtSceneTables* t = in.t;
    const int NP = in.ph ? in.ph->n_tables : 0;
    for (int k = 0; k < t->n_coatings; k++)
        for (int slot = 0; slot < 2; slot++) {
            const int m = slot == 0 ? t->coat_reflect_mode[k] : t->coat_transmit_mode[k];
            if (m == 0 || m == 1) continue;
            if (m < PVT_COAT_LOBE || m > in.knows.max_coat_mode) return fail(PVT_ERR_INVALID, "coating mode out of range");
            const int table = (m - PVT_COAT_LOBE) >> 2, axis = (m - PVT_COAT_LOBE) & 3;
            if (NP <= 0) return fail(PVT_ERR_INVALID, "coating lobe without phase tables");
            if (table >= NP) return fail(PVT_ERR_INVALID, "coating lobe names a missing phase table");
            if (slot == 0 && axis != PVT_LOBE_NORMAL && axis != PVT_LOBE_SPECULAR)
                return fail(PVT_ERR_INVALID, "coating lobe axis not legal for a reflection");
            if (slot == 1 && axis != PVT_LOBE_NORMAL && axis != PVT_LOBE_REFRACTED && axis != PVT_LOBE_STRAIGHT)
                return fail(PVT_ERR_INVALID, "coating lobe axis not legal for a transmission");
        }
    return PVT_OK;
}

int validate_tables(const SceneInputs& in) {
    const PvtSceneTables* t = in.t;
    int rc = validate_nodes(t, in.knows);
    if (rc == PVT_OK) rc = validate_coating_tables(t);
    if (rc == PVT_OK) rc = validate_indices(t);
    if (rc == PVT_OK) rc = validate_index_tables(t, in.x);
    if (rc == PVT_OK) rc = validate_phase_tables(t, in.ph);
    if (rc == PVT_OK) rc = validate_surface_tables(t, in.rs);
    if (rc == PVT_OK) rc = validate_field_tables(t, in.fr);
    if (rc == PVT_OK) rc = validate_map_tables(t, in.mp);
    if (rc == PVT_OK) rc = validate_capture_tables(t, in.cp);
    if (rc == PVT_OK) rc = validate_absorb_tables(t, in.ab);
    if (rc == PVT_OK) rc = validate_ranges(t, in.knows);
    if (rc == PVT_OK) rc = validate_coating_modes(in);
    return rc;
}

// unrotated: the 3x3 blocks of both matrices of a node are the identity, bit for bit (+0.0 off the diagonal)
bool unrotated(const PvtSceneTables* t, int n) {
    const double one = 1.0, zero = 0.0;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const double* want = r == c ? &one : &zero;
            if (std::memcmp(&t->world_to_local[n * 16 + r * 4 + c], want, 8) != 0) return false;
            if (std::memcmp(&t->local_to_world[n * 16 + r * 4 + c], want, 8) != 0) return false;
        }
    return true;
}

// ---- classes: what many nodes have in common is stored once (see the enums next to struct Lay) ----
struct Classes {
    std::vector<int> rot_class, rot_first;   // rotation classes and the first node of each
    std::vector<int> idx_class, idx_first;   // refractive-index classes and the first node of each
    bool by_node = false;                    // Lay::by_node
};

Classes classify_nodes(const SceneInputs& in) {
    const PvtSceneTables* t = in.t;
    const PvtIndexTables* x = in.x;
    const int N = t->n_nodes;
    Classes k;
    // rotation classes: nodes whose two 3x3 blocks have the same bits share a record (and, in the wave-uniform
    // node loop, the local direction and its reciprocals)
    k.rot_class.resize(N);
    for (int n = 0; n < N; n++) {
        int cls = -1;
        for (size_t e = 0; e < k.rot_first.size() && cls < 0; e++) {
            bool same = true;
            for (int r = 0; r < 3 && same; r++)
                for (int c = 0; c < 3 && same; c++)
                    same = std::memcmp(&t->world_to_local[n * 16 + r * 4 + c], &t->world_to_local[k.rot_first[e] * 16 + r * 4 + c], 8) == 0 &&
                           std::memcmp(&t->local_to_world[n * 16 + r * 4 + c], &t->local_to_world[k.rot_first[e] * 16 + r * 4 + c], 8) == 0;
            if (same) cls = (int)e;
        }
        if (cls < 0) { cls = (int)k.rot_first.size(); k.rot_first.push_back(n); }
        k.rot_class[n] = cls;
    }
    // refractive-index classes (bit-identical indices and the same index table: a dispersive node never shares a class
    // with a scalar one)
    auto table_of = [&](int n) { return x && x->n_tables > 0 ? x->node_table[n] : -1; };
    k.idx_class.resize(N);
    for (int n = 0; n < N; n++) {
        int cls = -1;
        for (size_t e = 0; e < k.idx_first.size() && cls < 0; e++)
            if (std::memcmp(&t->refractive_index[k.idx_first[e]], &t->refractive_index[n], 8) == 0 && table_of(k.idx_first[e]) == table_of(n))
                cls = (int)e;
        if (cls < 0) { cls = (int)k.idx_first.size(); k.idx_first.push_back(n); }
        k.idx_class[n] = cls;
    }
    // scenes of few nodes: classes, component records and candidate blocks numbered like the nodes / the reference's ids
    // (Lay::by_node: the lanes index the tables without reading NI_NCLS / NI_CREC / NI_CAND first)
    k.by_node = N <= 16;
    if (k.by_node) {
        k.idx_first.resize(N);
        for (int n = 0; n < N; n++) k.idx_class[n] = k.idx_first[n] = n;
    }
    return k;
}

// ---- pooled spectra.  The reference keeps one set of tables per component of every node (compiler.py:160-215); a
// scene of many nodes made of the same material repeats them.  Here a table that has the bits of an earlier one
// (abscissae, ordinates, sampling mode) is that earlier one: the 121 tiles of an LSC array share ONE absorption and
// ONE emission table.  Every table is searched by its abscissae (absorption x -> y, emission x -> cdf); an emission
// table is also searched by its CDF (cdf -> x).
struct SearchedTable {
    const double *xs, *ys;
    int n;
    bool hist, emission;
    double rcp, rcp_c, w;   // even_rcp of xs (and of the CDF as abscissae), even_w of xs: NaN where not proven
    int x, y;               // xs / ys, counted from the start of the spectra (a compact table keeps xs[0] alone)
    int gx, gc;             // guide tables of xs / of the CDF, counted from the start of the guides (-1: none)
};

struct Spectra {
    std::vector<SearchedTable> tables;
    std::vector<int> abs_of, ems_of;   // the table of component c's absorption / emission
    int len = 0, guide_len = 0;        // doubles of the spectra, ints of their guide tables

    int add(const double* xs, const double* ys, int n, bool hist, bool emission) {
        for (size_t e = 0; e < tables.size(); e++) {
            const SearchedTable& o = tables[e];
            if (o.emission == emission && o.n == n && o.hist == hist && std::memcmp(o.xs, xs, (size_t)n * 8) == 0 &&
                std::memcmp(o.ys, ys, (size_t)n * 8) == 0)
                return (int)e;
        }
        SearchedTable s{xs, ys, n, hist, emission};
        s.rcp = even_rcp(xs, ys, n);
        s.rcp_c = emission ? even_rcp(ys, xs, n) : NAN;
        s.w = hist ? NAN : even_w(xs, n, s.rcp);
        const bool compact = s.w == s.w;   // (even_w: n >= 2)
        s.x = len; len += compact ? 1 : n;
        s.y = len; len += n;
        s.gx = compact ? -1 : guide_len; guide_len += compact ? 0 : n;   // guide tables only for the arrays that are searched
        s.gc = emission ? guide_len : -1; guide_len += emission ? n : 0;
        tables.push_back(s);
        return (int)tables.size() - 1;
    }
};

Spectra pool_spectra(const PvtSceneTables* t) {
    const int C = t->n_components;
    Spectra sp;
    sp.abs_of.resize(C);
    sp.ems_of.resize(C);
    for (int c = 0; c < C; c++) {
        sp.abs_of[c] = sp.add(t->abs_x + t->comp_abs_start[c], t->abs_y + t->comp_abs_start[c], t->comp_abs_n[c],
                              t->comp_abs_hist && t->comp_abs_hist[c], false);
        sp.ems_of[c] = sp.add(t->ems_x + t->comp_ems_start[c], t->ems_cdf + t->comp_ems_start[c], t->comp_ems_n[c],
                              t->comp_ems_hist && t->comp_ems_hist[c], true);
    }
    return sp;
}

// ---- component RECORDS: the components of a node are a run of records; a node whose run has the contents of an
// earlier node's run shares it (NI_CREC).  Component IDS (events, `source`, recorder filters) stay the reference's.
struct Records {
    std::vector<int> node_crec, rec_comp;   // rec_comp[r] = the component id whose fields record r holds
    std::vector<int> node_cand;             // recorder candidate block of a node (-1: nobody listens to it)
    int n_cand = 0;
};

Records component_records(const SceneInputs& in, const Spectra& sp, bool by_node) {
    const PvtSceneTables* t = in.t;
    const PvtPhaseTables* ph = in.ph;
    const int N = t->n_nodes, C = t->n_components, R = t->n_recorders;
    auto table_of = [&](int c) { return ph && ph->n_tables > 0 ? ph->comp_table[c] : -1; };
    auto same_component = [&](int c, int e) {
        return t->comp_type[c] == t->comp_type[e] && t->comp_phase_type[c] == t->comp_phase_type[e] && table_of(c) == table_of(e) &&
               std::memcmp(&t->comp_qy[c], &t->comp_qy[e], 8) == 0 && std::memcmp(&t->comp_tau_rad[c], &t->comp_tau_rad[e], 8) == 0 &&
               std::memcmp(&t->comp_tau_nr[c], &t->comp_tau_nr[e], 8) == 0 &&
               std::memcmp(&t->comp_phase_param[c], &t->comp_phase_param[e], 8) == 0 &&
               sp.abs_of[c] == sp.abs_of[e] && sp.ems_of[c] == sp.ems_of[e];
    };
    Records recs;
    recs.node_crec.assign(N, 0);
    recs.node_cand.assign(N, -1);
    if (by_node) {   // one record per component id: NI_CREC == NI_CSTART, which the kernel relies on
        for (int n = 0; n < N; n++) recs.node_crec[n] = t->comp_start[n];
        for (int c = 0; c < C; c++) recs.rec_comp.push_back(c);
        for (int n = 0; n < N; n++) recs.node_cand[n] = n;
        recs.n_cand = N;
        return recs;
    }
    for (int n = 0; n < N; n++) {
        const int c0 = t->comp_start[n], cc = t->comp_count[n];
        int found = -1;
        for (int e = 0; e < n && found < 0; e++) {
            if (t->comp_count[e] != cc) continue;
            bool same = true;
            for (int k = 0; k < cc && same; k++) same = same_component(c0 + k, t->comp_start[e] + k);
            if (same) found = recs.node_crec[e];
        }
        if (found < 0) {
            found = (int)recs.rec_comp.size();
            for (int k = 0; k < cc; k++) recs.rec_comp.push_back(c0 + k);
        }
        recs.node_crec[n] = found;
    }
    // recorder candidate blocks: only for the nodes somebody listens to
    for (int r = 0; r < R; r++)
        if (recs.node_cand[t->rec_node[r]] < 0) recs.node_cand[t->rec_node[r]] = recs.n_cand++;
    return recs;
}

// ---- layout: fixed-stride records, then the pooled spectra.  The small tables come first in the blob -- records, then
// critical angles, rotation classes, index classes and the node grid -- and the spectra last: when a scene's spectra are
// too large for LDS, a workgroup still stages everything before `spec_d` (KArgs::nd_lds; the guide tables are the tail
// of the int blob in the same way).  Sizes p->gd / p->gi; returns where each coating reflectivity table goes, in
// *rtab_at where each refractive-index table goes and in *ptab_at where each phase-function table goes (p->rough_d, set by
// the caller when some node is rough, is moved to where the nodes' GGX widths go).
std::vector<int> lay_out(const SceneInputs& in, const Classes& k, const Spectra& sp, const Records& recs, const NodeGrid& grid,
                         PackedScene* p, std::vector<int>* rtab_at, std::vector<int>* ptab_at) {
    const PvtSceneTables* t = in.t;
    const PvtIndexTables* x = in.x;
    const PvtPhaseTables* ph = in.ph;
    const int N = t->n_nodes, R = t->n_recorders, H = t->n_hists, K = t->n_coatings;
    const int M = (int)k.idx_first.size(), Q = (int)k.rot_first.size(), CR = (int)recs.rec_comp.size();
    Lay& lay = p->lay;
    lay.comp_d = N * ND;
    lay.rec_d = lay.comp_d + CR * CD;
    lay.hist_d = lay.rec_d + R * RD;
    lay.coat_d = lay.hist_d + H * HD;
    const int small_d = lay.coat_d + K * KD;
    constexpr int kCritClasses = 16;
    lay.n_cls = M;
    lay.crit_d = M <= kCritClasses ? small_d : -1;
    lay.ccrit_d = lay.crit_d >= 0 ? lay.crit_d + M * M : -1;
    lay.rot_d = small_d + (lay.crit_d >= 0 ? 2 * M * M : 0);
    lay.ncls_d = lay.rot_d + Q * RT;
    lay.by_node = k.by_node ? 1 : 0;
    // (scenes with index tables) the index classes' dispersion records follow theirs: M x {where the class's table
    // starts in the double blob, its points (0: the class is scalar)}, as doubles
    const int disp = p->n_rtab > 0 ? M * 2 : 0;
    lay.grid_d = p->grid ? lay.ncls_d + M * 2 + disp : -1;
    p->nd_small = lay.ncls_d + M * 2 + disp + (p->grid ? 14 + (int)grid.masks.size() : 0);
    // coating reflectivity tables (KI_T*): their axes and values follow the spectra, so they go wherever the spectra go
    // (LDS with the whole blob, else global memory) and a scene without them lays out exactly as before
    int spec_end = p->nd_small + sp.len;
    const GridTables ctabs = grid_tables(t);
    std::vector<int> ctab_at(p->n_ctab);
    for (int j = 0; j < p->n_ctab; j++) {
        ctab_at[j] = spec_end;
        spec_end += (int)ctabs.doubles(j);
    }
    // refractive-index tables (wavelengths, then values) likewise, after the coating tables
    rtab_at->assign(p->n_rtab, 0);
    for (int j = 0; j < p->n_rtab; j++) {
        (*rtab_at)[j] = spec_end;
        spec_end += 2 * x->table_n[j];
    }
    // phase-function tables likewise, after the index tables: {n_wavelength, n_mu} as doubles, the wavelengths, the mu
    // axis, then the CDF rows (row-major) -- the record the kernel's PVT_PHASE_TABLE branch reads from CD_PHASE on
    ptab_at->assign(p->n_ptab, 0);
    for (int j = 0; j < p->n_ptab; j++) {
        (*ptab_at)[j] = spec_end;
        spec_end += 2 + ph->table_nw[j] + ph->table_nmu[j] + ph->table_nw[j] * ph->table_nmu[j];
    }
    // (scenes with a rough node) the GGX width alpha of every node, after the phase-function tables: the kernel's
    // UF_ROUGH lanes read their hit node's from where the spectra are read
    if (p->rough_d >= 0) {
        p->rough_d = spec_end;
        spec_end += N;
    }
    p->gd.assign((size_t)spec_end + 1, 0.0);
    lay.comp_i = N * NI;
    lay.rec_i = lay.comp_i + CR * CI;
    lay.hist_i = lay.rec_i + R * RI;
    lay.coat_i = lay.hist_i + H * HI;
    lay.cand_i = lay.coat_i + K * KI;
    lay.cand_list = lay.cand_i + recs.n_cand * 7 * 8;
    p->ni_small = lay.cand_list + R;   // guide tables: one entry per table point, per searched array
    p->gi.assign((size_t)p->ni_small + (size_t)sp.guide_len + 1, 0);
    return ctab_at;
}

// Recorders grouped by the (node, selector) they listen to.  A facet recorder whose facet has a clearly dominant
// component, alone in its (axis, sign) bin, goes to the bin table; the rest (no facet, oblique facets, bin collisions)
// to the walked list, ascending id.
// (`detected`: the blocks and lists of the eighth selector, PVT_RECX_DETECTED, at PackedScene::dcand_i instead -- one block
// per candidate node, the lists behind the blocks, `start` absolute in the int blob.)
void fill_candidates(const PvtSceneTables* t, const Records& recs, PackedScene* p, bool detected = false) {
    const int N = t->n_nodes, R = t->n_recorders;
    auto bin_of = [&](int r) -> int {
        if (!t->rec_has_facet[r]) return -1;
        const double* f = t->rec_facet + r * 3;
        const double a[3] = {std::fabs(f[0]), std::fabs(f[1]), std::fabs(f[2])};
        int k = (a[0] >= a[1] && a[0] >= a[2]) ? 0 : (a[1] >= a[2] ? 1 : 2);
        const double other = std::fmax(a[(k + 1) % 3], a[(k + 2) % 3]);
        // any normal within atol of the facet must have the same dominant axis and sign
        if (!(a[k] - other > 4.0 * t->rec_atol[r] + 1e-9) || !(a[k] > 2.0 * t->rec_atol[r])) return -1;
        return k * 2 + (f[k] > 0.0 ? 1 : 0);
    };
    auto unfiltered = [&](int r) { return !t->rec_source_mode || t->rec_source_mode[r] == 0; };
    auto axis_facet = [&](int r, int b) {
        const double* f = t->rec_facet + r * 3;
        for (int a = 0; a < 3; a++)
            if (f[a] != (a == b / 2 ? (b % 2 ? 1.0 : -1.0) : 0.0)) return false;
        return t->rec_atol[r] >= 0.0;
    };
    const int sel0 = detected ? PVT_RECX_DETECTED : 0, sel1 = detected ? PVT_RECX_DETECTED + 1 : 7;
    const int list0 = detected ? p->dcand_i + recs.n_cand * 8 : p->lay.cand_list;
    int at = detected ? list0 : 0;   // (the lists of Lay::cand_list count from its start)
    for (int node = 0; node < N; node++) {
        if (recs.node_cand[node] < 0) continue;
        // kRecPlain on an entry: the lane need not read the recorder's row at all -- no source filter, and either no
        // facet, or a facet that IS the bin's axis (exactly +-1 on it, zeros elsewhere) on an unrotated box, whose
        // world normals are exactly such unit vectors: |facet - normal| is exactly 0 for every normal of the bin
        const bool exact_normals = t->geom_type[node] == PVT_GEOM_BOX && unrotated(t, node);
        for (int sel = sel0; sel < sel1; sel++) {
            int* rec = detected ? p->gi.data() + p->dcand_i + recs.node_cand[node] * 8
                                : p->gi.data() + p->lay.cand_i + (recs.node_cand[node] * 7 + sel) * 8;
            rec[0] = at;
            int owner[6] = {-1, -1, -1, -1, -1, -1};
            bool clash[6] = {false, false, false, false, false, false};
            auto listens = [&](int r) { return t->rec_node[r] == node && t->rec_event[r] == sel; };
            for (int r = 0; r < R; r++) {
                const int b = listens(r) ? bin_of(r) : -1;
                if (b >= 0) { if (owner[b] >= 0) clash[b] = true; else owner[b] = r; }
            }
            for (int b = 0; b < 6; b++) {
                rec[2 + b] = (owner[b] >= 0 && !clash[b]) ? owner[b] : -1;
                if (rec[2 + b] >= 0 && exact_normals && unfiltered(owner[b]) && axis_facet(owner[b], b)) rec[2 + b] |= kRecPlain;
            }
            for (int r = 0; r < R; r++) {
                if (!listens(r)) continue;
                const int b = bin_of(r);
                if (b >= 0 && !clash[b]) continue;  // served by the bin table
                p->gi[(detected ? 0 : list0) + at++] = r | ((unfiltered(r) && !t->rec_has_facet[r]) ? kRecPlain : 0);
            }
            rec[1] = at - rec[0];
        }
    }
}

// ---- fill: every record, table and guide table of the two blobs, and the BVHs of the meshes
int fill(const SceneInputs& in, const Classes& k, const Spectra& sp, const Records& recs, const NodeGrid& grid,
         const std::vector<int>& ctab_at, const std::vector<int>& rtab_at, const std::vector<int>& ptab_at, PackedScene* p) {
    const PvtSceneTables* t = in.t;
    const PvtIndexTables* x = in.x;
    const PvtPhaseTables* ph = in.ph;
    const PvtSurfaceTables* rs = in.rs;
    const int N = t->n_nodes, R = t->n_recorders, H = t->n_hists, K = t->n_coatings;
    const int M = (int)k.idx_first.size(), Q = (int)k.rot_first.size();
    const Lay& lay = p->lay;
    std::vector<double>& gd = p->gd;
    std::vector<int>& gi = p->gi;
    if (p->grid) {
        double* d = gd.data() + lay.grid_d;
        for (int a = 0; a < 3; a++) { d[a] = grid.lo[a]; d[3 + a] = grid.hi[a]; d[6 + a] = grid.cell[a]; d[9 + a] = 1.0 / grid.cell[a]; }
        d[12] = grid.guard;
        const unsigned long long bits = (unsigned long long)grid.n[0] | ((unsigned long long)grid.n[1] << 8) | ((unsigned long long)grid.n[2] << 16) |
                                        ((unsigned long long)grid.words << 24) | ((unsigned long long)(grid.odd ? 1 : 0) << 28);
        std::memcpy(&d[13], &bits, 8);
        std::memcpy(&d[14], grid.masks.data(), grid.masks.size() * 8);
    }
    // index table of each class (-1: scalar)
    auto class_table = [&](int m) { return p->n_rtab > 0 ? x->node_table[k.idx_first[m]] : -1; };
    // (PVT_NO_COS_THRESHOLD: no finite threshold counts as proven, so every such pair takes the kernel's computed arm --
    // the reference's own expression, same results -- and the scene is not lean: prove_lean's last clause)
    const bool no_threshold = getenv("PVT_NO_COS_THRESHOLD") != nullptr;
    if (lay.crit_d >= 0)
        for (int c = 0; c < M; c++)
            for (int a = 0; a < M; a++) {
                const double n1 = t->refractive_index[k.idx_first[c]], n2 = t->refractive_index[k.idx_first[a]];
                double crit = n2 < n1 ? pvt_asin(n2 / n1) : INFINITY;   // same pvt_asin as the device
                // a pair with a dispersive side has no angle of its own: NaN sends its lanes to the computed branch
                if (class_table(c) >= 0 || class_table(a) >= 0) crit = NAN;
                gd[lay.crit_d + c * M + a] = crit;
                gd[lay.ccrit_d + c * M + a] = crit != crit || (no_threshold && crit < INFINITY) ? NAN : cosine_threshold(crit);
            }
    for (int q = 0; q < Q; q++) {
        double* d = gd.data() + lay.rot_d + q * RT;
        const int n = k.rot_first[q];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                d[RT_W2L + r * 3 + c] = t->world_to_local[n * 16 + r * 4 + c];
                d[RT_L2W + r * 3 + c] = t->local_to_world[n * 16 + r * 4 + c];
            }
    }
    for (int m = 0; m < M; m++) {
        gd[lay.ncls_d + m * 2] = t->refractive_index[k.idx_first[m]];
        gd[lay.ncls_d + m * 2 + 1] = 1.0 / t->refractive_index[k.idx_first[m]];
        if (p->n_rtab > 0) {
            const int j = class_table(m);
            gd[lay.ncls_d + M * 2 + m * 2] = j >= 0 ? rtab_at[j] : 0;
            gd[lay.ncls_d + M * 2 + m * 2 + 1] = j >= 0 ? x->table_n[j] : 0;
        }
    }
    for (int j = 0; j < p->n_rtab; j++) {   // wavelengths (nm), then the indices
        const int np = x->table_n[j], p0 = x->table_start[j];
        double* d = gd.data() + rtab_at[j];
        for (int i = 0; i < np; i++) d[i] = x->wavelength[p0 + i];
        for (int i = 0; i < np; i++) d[np + i] = x->value[p0 + i];
    }
    for (int j = 0; j < p->n_ptab; j++) {   // {n_wavelength, n_mu}, wavelengths (nm), mu axis, CDF rows
        const int nw = ph->table_nw[j], nm = ph->table_nmu[j];
        double* d = gd.data() + ptab_at[j];
        d[0] = nw;
        d[1] = nm;
        for (int i = 0; i < nw; i++) d[2 + i] = ph->wavelength[ph->wl_start[j] + i];
        for (int i = 0; i < nm; i++) d[2 + nw + i] = ph->mu[ph->mu_start[j] + i];
        for (int i = 0; i < nw * nm; i++) d[2 + nw + nm + i] = ph->cdf[ph->cdf_start[j] + i];
    }
    if (p->rough_d >= 0)
        for (int n = 0; n < N; n++) gd[p->rough_d + n] = rs->node_roughness[n];
    fill_candidates(t, recs, p);
    for (int n = 0; n < N; n++) {
        double* d = gd.data() + n * ND;
        for (int r = 0; r < 3; r++) d[ND_T + r] = t->world_to_local[n * 16 + r * 4 + 3];
        for (int c = 0; c < 3; c++) d[ND_PARAMS + c] = t->geom_params[n * 4 + c];
        const unsigned long long bits = (unsigned long long)(unsigned int)((unrotated(t, n) ? 1 : 0) | (t->geom_type[n] << 8)) |
                                        ((unsigned long long)(unsigned int)k.rot_class[n] << 32);
        std::memcpy(&d[ND_BITS], &bits, 8);
        d[ND_N] = t->refractive_index[n];
        int* q = gi.data() + n * NI;
        q[NI_SURF] = t->surface_type[n];
        q[NI_CSTART] = t->comp_start[n];
        q[NI_CCOUNT] = t->comp_count[n];
        q[NI_CREC] = recs.node_crec[n];
        q[NI_KSTART] = K > 0 ? t->coat_start[n] : 0;
        q[NI_KCOUNT] = K > 0 ? t->coat_count[n] : 0;
        q[NI_MESH] = -1;
        q[NI_CAND] = recs.node_cand[n];
        q[NI_NCLS] = k.idx_class[n];
        if (t->geom_type[n] == PVT_GEOM_MESH) {
            double centre[3];
            q[NI_MESH] = pvt::BvhBuilder(t->mesh_vertices, t->mesh_faces, t->mesh_normals, p->bvh_nodes, p->bvh_tris)
                             .add_mesh(t->mesh_face_start[n], t->mesh_face_count[n], centre);
            p->bvh_roots.push_back(q[NI_MESH]);
            for (int c = 0; c < 3; c++) d[ND_PARAMS + c] = centre[c];   // a mesh has no shape parameters: the point its boxes are relative to
        }
    }
    if (p->bvh_nodes.size() >= ((size_t)1 << 26) || p->bvh_tris.size() >= ((size_t)1 << 26))
        return fail(PVT_ERR_INVALID, "meshes too large: the walk's cursors and leaf references hold 2^26 records / triangles");
    // the spectra, once per distinct table (a compact table keeps its first abscissa only), and their guide tables
    const int spec_d = p->nd_small, guide0 = p->ni_small;
    std::vector<double> scale_x(sp.tables.size()), scale_c(sp.tables.size());
    for (size_t e = 0; e < sp.tables.size(); e++) {
        const SearchedTable& s = sp.tables[e];
        scale_x[e] = s.gx >= 0 ? build_guide(s.xs, s.n, &gi[guide0 + s.gx]) : 0.0;
        scale_c[e] = s.gc >= 0 ? build_guide(s.ys, s.n, &gi[guide0 + s.gc]) : 0.0;
        std::copy(s.xs, s.xs + (s.gx >= 0 ? s.n : 1), &gd[spec_d + s.x]);
        std::copy(s.ys, s.ys + s.n, &gd[spec_d + s.y]);
    }
    for (size_t r = 0; r < recs.rec_comp.size(); r++) {
        const int c = recs.rec_comp[r];
        const SearchedTable &ab = sp.tables[sp.abs_of[c]], &em = sp.tables[sp.ems_of[c]];
        double* d = gd.data() + lay.comp_d + r * CD;
        d[CD_QY] = t->comp_qy[c]; d[CD_TAU_RAD] = t->comp_tau_rad[c]; d[CD_TAU_NR] = t->comp_tau_nr[c];
        d[CD_PHASE] = t->comp_phase_param[c];
        int* q = gi.data() + lay.comp_i + r * CI;
        q[CI_TYPE] = t->comp_type[c];
        q[CI_PHASE] = t->comp_phase_type[c];
        if (t->comp_phase_type[c] == PVT_PHASE_LAMBERTIAN) {
            // The Lambertian phase function, theta = asin(sqrt(p1)), IS the cone's theta = asin(sqrt(p1) sin(theta_max)) at
            // theta_max = pi/2 -- same two draws in the same order -- provided sin(pi/2) is the double 1.0 in the
            // kernel's arithmetic (x * 1.0 is exact); checked here with the very function the kernel calls.
            const double half_pi = 1.5707963267948966;
            if (pvt_sin(half_pi) != 1.0) return fail(PVT_ERR_INVALID, "pvt_sin(pi/2) != 1: the Lambertian phase function cannot be lowered to a cone");
            d[CD_PHASE] = half_pi;
            q[CI_PHASE] = PVT_PHASE_CONE;
        }
        if (t->comp_phase_type[c] == PVT_PHASE_TABLE) d[CD_PHASE] = ptab_at[ph->comp_table[c]];   // where its table starts
        // absolute offsets into the blobs; -1: no guide table, never dereferenced
        q[CI_ABS_X] = spec_d + ab.x; q[CI_ABS_Y] = spec_d + ab.y; q[CI_ABS_N] = ab.n; q[CI_ABS_HIST] = ab.hist;
        q[CI_EMS_X] = spec_d + em.x; q[CI_EMS_CDF] = spec_d + em.y; q[CI_EMS_N] = em.n; q[CI_EMS_HIST] = em.hist;
        q[CI_ABS_G] = ab.gx < 0 ? -1 : guide0 + ab.gx; q[CI_EMS_GX] = em.gx < 0 ? -1 : guide0 + em.gx; q[CI_EMS_GC] = guide0 + em.gc;
        d[CD_ABS_RCP] = ab.rcp; d[CD_ABS_W] = ab.w; d[CD_ABS_SCALE] = scale_x[sp.abs_of[c]];
        d[CD_EMS_RCP_X] = em.rcp; d[CD_EMS_RCP_C] = em.rcp_c; d[CD_EMS_W] = em.w;
        d[CD_EMS_SCALE_X] = scale_x[sp.ems_of[c]]; d[CD_EMS_SCALE_C] = scale_c[sp.ems_of[c]];
    }
    for (int r = 0; r < R; r++) {
        double* d = gd.data() + lay.rec_d + r * RD;
        for (int a = 0; a < 3; a++) d[RD_FACET + a] = t->rec_facet[r * 3 + a];
        d[RD_ATOL] = t->rec_atol[r];
        int* q = gi.data() + lay.rec_i + r * RI;
        q[RI_NODE] = t->rec_node[r];
        q[RI_EVENT] = t->rec_event[r];
        q[RI_HAS_FACET] = t->rec_has_facet[r];
        q[RI_HSTART] = t->rec_hist_start[r];
        q[RI_HN] = t->rec_hist_n[r];
        q[RI_SRC_MODE] = t->rec_source_mode ? t->rec_source_mode[r] : 0;
        q[RI_SRC_ID] = t->rec_source_id ? t->rec_source_id[r] : -1;
    }
    auto rcp_or_nan = [](double width) {   // NaN: the kernel divides for real
        return (std::isfinite(width) && std::fabs(width) > 1e-290 && std::fabs(width) < 1e290) ? 1.0 / width : NAN;
    };
    for (int h = 0; h < H; h++) {
        double* d = gd.data() + lay.hist_d + h * HD;
        d[HD_LO_A] = t->hist_lo_a[h]; d[HD_HI_A] = t->hist_hi_a[h];
        d[HD_LO_B] = t->hist_lo_b[h]; d[HD_HI_B] = t->hist_hi_b[h];
        d[HD_RA] = rcp_or_nan(t->hist_hi_a[h] - t->hist_lo_a[h]);
        d[HD_RB] = rcp_or_nan(t->hist_hi_b[h] - t->hist_lo_b[h]);
        int* q = gi.data() + lay.hist_i + h * HI;
        q[HI_PA] = t->hist_prop_a[h]; q[HI_PB] = t->hist_prop_b[h];
        q[HI_NA] = t->hist_na[h]; q[HI_NB] = t->hist_nb[h]; q[HI_OFF] = t->hist_offset[h];
        for (const int prop : {t->hist_prop_a[h], t->hist_prop_b[h]}) {
            if (prop >= PVT_PROP_X && prop <= PVT_PROP_Z) p->hist_reads_position = true;
            if (prop >= PVT_PROPX_EMISSIONS && prop <= PVT_PROPX_REFLECTIONS) p->hist_reads_counter = true;
            if (prop >= PVT_PROPX_ORIGIN_WAVELENGTH && prop <= PVT_PROPX_ORIGIN_Z) p->origin_mask |= 1 << (prop - PVT_PROPX_ORIGIN_WAVELENGTH);
        }
    }
    for (int c = 0; c < K; c++) {
        double* d = gd.data() + lay.coat_d + c * KD;
        for (int a = 0; a < 3; a++) {
            d[KD_FACET + a] = t->coat_facet[c * 3 + a];
            d[KD_LO + a] = t->coat_lo[c * 3 + a];
            d[KD_HI + a] = t->coat_hi[c * 3 + a];
        }
        d[KD_REFL] = t->coat_reflectivity[c];
        int* q = gi.data() + lay.coat_i + c * KI;
        // (a lobe's word is replaced by its stand-in among the built-in modes, whose body leaves the lobe's axis in the
        // photon's direction and decides what holds beyond the critical angle: specular for a reflection; Fresnel for a
        // transmission about "refracted", matched for one about "normal" or "straight" -- pack_lobes keeps table and axis)
        const int rm = t->coat_reflect_mode[c], tm = t->coat_transmit_mode[c];
        q[KI_RMODE] = rm >= PVT_COAT_LOBE ? 0 : rm;
        q[KI_TMODE] = tm >= PVT_COAT_LOBE ? (((tm - PVT_COAT_LOBE) & 3) == PVT_LOBE_REFRACTED ? 0 : 1) : tm;
        const int j = p->n_ctab > 0 ? t->coat_table[c] : -1;
        q[KI_TNW] = j >= 0 ? t->ctab_nw[j] : 0;   // 0: no table
        q[KI_TNA] = j >= 0 ? t->ctab_na[j] : 0;
        q[KI_TW] = j >= 0 ? ctab_at[j] : 0;
        q[KI_TA] = j >= 0 ? ctab_at[j] + t->ctab_nw[j] : 0;
        q[KI_TV] = j >= 0 ? ctab_at[j] + t->ctab_nw[j] + t->ctab_na[j] : 0;
    }
    for (int j = 0; j < p->n_ctab; j++) put_grid_table(grid_tables(t), j, gd.data() + ctab_at[j]);
    return PVT_OK;
}

void prove_shortcuts(const PvtSceneTables* t, PackedScene* p) {
    const int N = t->n_nodes, R = t->n_recorders, root = t->root_id;
    for (int r = 0; r < R; r++)
        if (t->rec_node[r] == root && t->rec_event[r] == PVT_REC_EXIT) p->exit_observed = true;
    // Lazy root (kernel node loop): the root is a box or a sphere and every other node lies strictly inside it,
    // its bounding sphere clearing the root's surface by a margin -- then a ray from inside the root meets every
    // other node's surface strictly before the root's.
    if (!getenv("PVT_NO_LAZY_ROOT") && (t->geom_type[root] == PVT_GEOM_BOX || t->geom_type[root] == PVT_GEOM_SPHERE)) {
        const double* w2l = t->world_to_local + root * 16;
        const double* rp = t->geom_params + root * 4;
        const bool box = t->geom_type[root] == PVT_GEOM_BOX;
        const double scale = box ? std::fmax(rp[0], std::fmax(rp[1], rp[2])) : rp[0];
        const double margin = 1e-6 * scale + 1e-9;
        bool inside = std::isfinite(scale) && scale > 0.0;
        for (int n = 0; n < N && inside; n++) {
            if (n == root) continue;
            const double* l2w = t->local_to_world + n * 16;
            const double* gp = t->geom_params + n * 4;
            double radius;   // of a sphere about the node's origin that holds the whole shape
            switch (t->geom_type[n]) {
                case PVT_GEOM_BOX: radius = 0.5 * std::sqrt(gp[0] * gp[0] + gp[1] * gp[1] + gp[2] * gp[2]); break;
                case PVT_GEOM_SPHERE: radius = gp[0]; break;
                case PVT_GEOM_CYLINDER: radius = std::sqrt(gp[1] * gp[1] + 0.25 * gp[0] * gp[0]); break;
                case PVT_GEOM_FRUSTUM: {
                    const double rmax = std::fmax(gp[1], gp[2]);
                    radius = std::sqrt(rmax * rmax + 0.25 * gp[0] * gp[0]);
                    break;
                }
                case PVT_GEOM_POLYHEDRON: radius = gp[0]; break;   // (its bounding radius: validate_polyhedra)
                case PVT_GEOM_CONICOID: {   // sqrt(max of q on [-half, half] + half^2): the ends, and the vertex of a q that opens downwards
                    const ConicoidEnds e = conicoid_ends(gp);
                    double qmax = std::fmax(e.q_lo, e.q_hi);
                    const double zv = gp[3] < 0.0 ? -0.5 * gp[2] / gp[3] : INFINITY;
                    if (-e.half < zv && zv < e.half) qmax = std::fmax(qmax, gp[1] + (gp[2] + gp[3] * zv) * zv);
                    radius = std::sqrt(qmax + e.half * e.half);
                    break;
                }
                default: radius = INFINITY; break;   // (mesh scenes never take this path)
            }
            radius *= 1.0 + 1e-12;
            double c[3];   // the node's origin in the root's frame
            for (int a = 0; a < 3; a++)
                c[a] = w2l[a * 4] * l2w[3] + w2l[a * 4 + 1] * l2w[7] + w2l[a * 4 + 2] * l2w[11] + w2l[a * 4 + 3];
            if (box) {
                for (int a = 0; a < 3; a++)
                    if (!(0.5 * rp[a] - std::fabs(c[a]) - radius > margin)) inside = false;
            } else {
                if (!(rp[0] - std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) - radius > margin)) inside = false;
            }
        }
        if (inside) {
            p->lazy_root = box ? 1 : 2;
            p->lazy_k = box ? 0.0 : 1.0 / (2.0 * rp[0]);
        }
    }
    // Fused exit (kernel surface branch): the scene is ONE unrotated box inside a lazy root whose medium neither
    // absorbs nor is listened to -- a photon that leaves the box's surface outwards can only leave the scene.
    // (the first clause that fails is named for pvt_scene_solo_check: fuse_why, null when fuse_exit holds)
    const char* why = nullptr;
    auto refuse = [&](const char* clause) { if (!why) why = clause; };
    if (N != 2) refuse("not exactly one node inside the root");
    else if (!p->lazy_root) refuse("the root is no box or sphere that strictly holds the child (or PVT_NO_LAZY_ROOT is set)");
    else if (getenv("PVT_NO_FUSED_EXIT")) refuse("the fused exit is switched off (PVT_NO_FUSED_EXIT)");
    else {
        const int child = 1 - root;
        if (t->geom_type[child] != PVT_GEOM_BOX || !unrotated(t, child)) refuse("the child is no unrotated box");
        if (t->comp_count[root] != 0) refuse("a component in the root");
        for (int r = 0; r < R; r++)
            if (t->rec_node[r] == root) refuse("a recorder on the root");
    }
    p->fuse_why = why;
    p->fuse_exit = why == nullptr;
}

// Lean scenes (kernel: trace_body's LEAN, the trace_kernel_lean family): every fact that variant holds as a constant,
// read back from the PACKED tables -- the words the kernel itself would have asked -- so that whoever fills them, Python
// or a C caller, gets the same answer.  One clause per fact; tests/test_lean_variant.py breaks each in turn.
//   * no extension: no coating (so no reflectivity table), no index table, no phase table, no rough node, no
//     concentration field, no volume map; no mesh, no node grid;
//   * few nodes (Lay::by_node), every one of them unrotated, hence one rotation class, and a box -- but for the root,
//     which may be a sphere as well (the reference's test and benchmark scenes stand in a spherical world);
//   * per container at most two components, each an absorber or a luminophore with the isotropic phase function;
//   * no spectrum the loop reads is a histogram, and each is sampled on an even grid: absorption x -> y of every
//     component, emission x -> cdf and cdf -> x of every luminophore.  Two kinds.  Where every one of them is a constant
//     (one point) or even BIT FOR BIT (even_w: CD_*_W a number) the scene is `lean_even` and runs the EVEN kernels
//     (interp_clamped's kInterpEven / kInterpByGuide: no guide bracket, no bisection).  A grid that is even only up to
//     rounding -- np.linspace(300, 1000, 200), the reference's benchmark slab: the spacing is no double -- cannot take the
//     arithmetic path (the divisor of its intervals is not one known number), so its scene runs the family's other
//     kernels, which search the tables as the generic ones do (kInterpNoHist).  A grid that is not even at all
//     (abscissae off x0 + i (xl - x0) / (n - 1) by more than 1e-9 of the spacing) is not the plain kind: generic family.
//     That last clause is the definition of the class, not something the kernel relies on;
//   * at most 64 recorders, and every entry of the candidate tables carries kRecPlain (no source filter, nothing to
//     compare with the normal);
//   * every entry of the cosine-threshold table (Lay::ccrit_d) is a number: whichever (container, adjacent) pair of index
//     classes a crossing brings up, total reflection is decided by comparing the cosine with a proven threshold, and the
//     lean kernels do not hold the arm that evaluates acos and asin instead.  (An entry is NaN only where
//     cosine_threshold could prove none; PVT_NO_COS_THRESHOLD makes every finite one NaN, for tests.)
constexpr const char* kLeanNoThreshold = "an index pair without a proven critical-angle threshold";
void prove_lean(const PvtSceneTables* t, PackedScene* p) {
    const Lay& lay = p->lay;
    const std::vector<double>& gd = p->gd;
    const std::vector<int>& gi = p->gi;
    const int N = t->n_nodes, R = t->n_recorders;
    bool all_even = true;
    // n abscissae stored at gd[at ...]: an even grid up to rounding
    auto nearly_even = [&](int at, int n) {
        const double x0 = gd[(size_t)at], step = (gd[(size_t)at + n - 1] - x0) / (double)(n - 1);
        if (!(step > 0.0) || !std::isfinite(step)) return false;
        for (int i = 0; i < n; i++)
            if (!(std::fabs(gd[(size_t)at + i] - (x0 + (double)i * step)) <= 1e-9 * step)) return false;
        return true;
    };
    // a searched table (CI_*_X, n points, its even_w in `w`): 2 = a constant or even bit for bit, 1 = even up to rounding, 0
    auto grid_kind = [&](int at, int n, double w) { return (n == 1 || w == w) ? 2 : (nearly_even(at, n) ? 1 : 0); };
    bool ok = t->n_coatings == 0 && p->n_ctab == 0 && p->n_rtab == 0 && p->n_ptab == 0 && p->rough_d < 0 && !p->has_frustum && !p->has_polyhedron && !p->has_conicoid && p->fd.empty() &&
              p->md.empty() && p->cd.empty() && p->bvh_nodes.empty() && !p->grid && lay.by_node == 1 && R <= 64;
    // (the first clause that fails is named for pvt_scene_lean_check)
    const char* why = ok ? nullptr : "an extension, a mesh, a node grid, or too many nodes or recorders";
    auto refuse = [&](const char* clause) { if (ok) why = clause; ok = false; };
    for (int n = 0; n < N && ok; n++) {
        unsigned long long bits;
        std::memcpy(&bits, &gd[(size_t)n * ND + ND_BITS], 8);
        const bool ident = (bits & 1ull) != 0;
        const int geom = (int)(((unsigned int)bits >> 8) & 0xffu), rot_class = (int)(unsigned int)(bits >> 32);
        const int* q = gi.data() + n * NI;
        const bool shape_ok = geom == PVT_GEOM_BOX || (geom == PVT_GEOM_SPHERE && n == t->root_id);
        if (!ident || !shape_ok || rot_class != 0 || q[NI_KCOUNT] != 0 || q[NI_CCOUNT] > 2) refuse("a node that is no unrotated box, or holds more than two components");
        for (int k = 0; k < q[NI_CCOUNT] && ok; k++) {
            const int* ci = gi.data() + lay.comp_i + (q[NI_CREC] + k) * CI;
            const double* cd = gd.data() + lay.comp_d + (q[NI_CREC] + k) * CD;
            const bool luminophore = ci[CI_TYPE] == PVT_COMP_LUMINOPHORE;
            if (!luminophore && ci[CI_TYPE] != PVT_COMP_ABSORBER) refuse("a component that is neither an absorber nor a luminophore");
            if (ci[CI_PHASE] != PVT_PHASE_ISOTROPIC) refuse("a phase function that is not isotropic");
            const int ka = ci[CI_ABS_HIST] != 0 ? 0 : grid_kind(ci[CI_ABS_X], ci[CI_ABS_N], cd[CD_ABS_W]);
            const int ke = !luminophore ? 2 : (ci[CI_EMS_HIST] != 0 ? 0 : grid_kind(ci[CI_EMS_X], ci[CI_EMS_N], cd[CD_EMS_W]));
            if (ka == 0 || ke == 0) refuse("a spectrum that is a histogram or off the even grid");
            if (ka != 2 || ke != 2) all_even = false;
        }
    }
    for (int block = 0; block < N * 7 && ok; block++) {   // (by_node: one candidate block per node and selector)
        const int* rec = gi.data() + lay.cand_i + block * 8;
        for (int b = 0; b < 6; b++)
            if (rec[2 + b] >= 0 && !(rec[2 + b] & kRecPlain)) refuse("a recorder entry that is not plain");
        for (int j = 0; j < rec[1]; j++)
            if (!(gi[(size_t)lay.cand_list + rec[0] + j] & kRecPlain)) refuse("a recorder entry that is not plain");
    }
    // (with by_node the classes are few enough for the tables: crit_d >= 0; a NaN means cosine_threshold could not prove one)
    if (ok && lay.ccrit_d < 0) refuse(kLeanNoThreshold);
    for (int e = 0; e < lay.n_cls * lay.n_cls && ok; e++)
        if (gd[(size_t)lay.ccrit_d + e] != gd[(size_t)lay.ccrit_d + e]) refuse(kLeanNoThreshold);
    p->lean_why = why;
    p->lean_ok = ok;
    p->lean_even = ok && all_even;
}

// Solo scenes (kernel: trace_body's SOLO, the trace_kernel_solo entries): a lean scene that moreover has the fused exit --
// ONE unrotated box inside a lazy root (a box or a sphere) that holds no component and carries no recorder -- with its few
// nodes numbered as they are (Lay::by_node).  The node stage of such a scene has three outcomes (inside the box, outside
// and hitting it, outside and missing it), which the SOLO form selects instead of folding crossings.  Both facts are the
// ones prove_shortcuts and prove_lean have established; the clauses below only name which of them a scene fails, in the
// order a reader would ask (pvt_scene_solo_check); the fused exit's own clauses are named where they are decided, in
// prove_shortcuts (PackedScene::fuse_why).  Whether a LAUNCH is solo is the host's decision on top of this: it
// also needs `lazy_root` and `fuse_exit` in the launch's arguments -- a tally launch, nobody observing exits.
void prove_solo(const PvtSceneTables*, PackedScene* p) {
    const char* why = nullptr;
    auto refuse = [&](const char* clause) { if (!why) why = clause; };
    if (!p->lean_ok) refuse("the scene is not lean");
    if (!p->fuse_exit) refuse(p->fuse_why ? p->fuse_why : "the fused exit is not proven");
    if (p->lay.by_node != 1) refuse("the nodes are not numbered as they are (Lay::by_node)");
    p->solo_why = why;
    p->solo = why == nullptr;
}

// The field buffer p->fd (validated tables; left empty when no node carries a lattice): per node where its record starts,
// then per fielded node its record -- shape, lower, cell widths h = (upper - lower) / n, the world->local rotation and
// translation of world_to_local (the doubles the node record and rotation classes hold) and, per component in the node's
// order, where its value table starts -- then each value table once.
void pack_fields(const SceneInputs& in, PackedScene* p) {
    const PvtSceneTables* t = in.t;
    const PvtFieldTables* fr = in.fr;
    p->fd.clear();
    if (!fr || fr->n_nodes == 0) return;
    const int N = t->n_nodes;
    bool any = false;
    for (int n = 0; n < N; n++) any = any || fr->node_field[n] >= 0;
    if (!any) return;
    std::vector<double>& fd = p->fd;
    fd.assign((size_t)N, -1.0);
    for (int n = 0; n < N; n++) {
        const int f = fr->node_field[n];
        if (f < 0) continue;
        fd[(size_t)n] = (double)fd.size();
        const size_t at = fd.size();
        fd.resize(at + kFrComp + (size_t)t->comp_count[n], 0.0);
        double* r = fd.data() + at;
        for (int a = 0; a < 3; a++) {
            const double lo = fr->field_lower[f * 3 + a], hi = fr->field_upper[f * 3 + a];
            const int na = fr->field_shape[f * 3 + a];
            r[kFrShape + a] = (double)na;
            r[kFrLower + a] = lo;
            r[kFrH + a] = (hi - lo) / (double)na;
            for (int c = 0; c < 3; c++) r[kFrRot + a * 3 + c] = t->world_to_local[n * 16 + a * 4 + c];
            r[kFrT + a] = t->world_to_local[n * 16 + a * 4 + 3];
        }
    }
    std::vector<long long> value_at((size_t)fr->n_values, -1);
    for (int n = 0; n < N; n++) {
        if (fr->node_field[n] < 0) continue;
        const size_t at = (size_t)fd[(size_t)n];
        for (int k = 0; k < t->comp_count[n]; k++) {
            const int v = fr->comp_values[t->comp_start[n] + k];
            if (value_at[(size_t)v] < 0) {
                value_at[(size_t)v] = (long long)fd.size();
                const double* src = fr->values + fr->values_start[v];
                fd.insert(fd.end(), src, src + fr->values_count[v]);
            }
            fd[at + kFrComp + (size_t)k] = (double)value_at[(size_t)v];
        }
    }
}

// The map buffer p->md (validated tables; left empty without maps): per node where its block starts, then per node with
// maps its block -- the map count, the world->local rotation and translation of world_to_local (the doubles a field
// record holds), how many of the maps are path-length maps (the marker the kernel asks before it walks) -- and per map
// its record: kind, component, shape, lower, cell widths, wavelength bins and range, first slot.
void pack_maps(const SceneInputs& in, PackedScene* p) {
    const PvtSceneTables* t = in.t;
    const PvtMapTables* mp = in.mp;
    p->md.clear();
    p->map_slots = 0;
    p->path_maps = false;
    if (!mp || mp->n_nodes == 0 || mp->n_maps == 0) return;
    const int N = t->n_nodes;
    std::vector<double>& md = p->md;
    md.assign((size_t)N, -1.0);
    for (int n = 0; n < N; n++) {
        const int count = mp->node_map_count[n];
        if (count == 0) continue;
        md[(size_t)n] = (double)md.size();
        const size_t at = md.size();
        md.resize(at + kMnRec + (size_t)count * kMr, 0.0);
        double* r = md.data() + at;
        r[kMnCount] = (double)count;
        for (int a = 0; a < 3; a++) {
            for (int c = 0; c < 3; c++) r[kMnRot + a * 3 + c] = t->world_to_local[n * 16 + a * 4 + c];
            r[kMnT + a] = t->world_to_local[n * 16 + a * 4 + 3];
        }
        for (int k = 0; k < count; k++) {
            const int m = mp->node_map_start[n] + k;
            double* q = r + kMnRec + k * kMr;
            q[kMrKind] = (double)mp->map_kind[m];
            if (mp->map_kind[m] == PVT_MAP_PATHLENGTH) { r[kMnPath] += 1.0; p->path_maps = true; }
            q[kMrComp] = (double)mp->map_component[m];
            for (int a = 0; a < 3; a++) {
                q[kMrShape + a] = (double)mp->map_shape[m * 3 + a];
                q[kMrLower + a] = mp->map_lower[m * 3 + a];
                q[kMrH + a] = mp->map_h[m * 3 + a];
            }
            q[kMrNw] = (double)mp->map_nw[m];
            q[kMrWlo] = mp->map_wl_start[m];
            q[kMrWhi] = mp->map_wl_stop[m];
            q[kMrOff] = (double)mp->map_offset[m];   // (< 2^26: exact)
        }
    }
    p->map_slots = mp->map_slots;
}

// The capture table p->cd (validated tables; left empty when no recorder is captured): capacity and first row per recorder.
void pack_captures(const SceneInputs& in, PackedScene* p) {
    const PvtSceneTables* t = in.t;
    const PvtCaptureTables* cp = in.cp;
    p->cd.clear();
    p->capture_rows = 0;
    if (!cp || cp->n_recorders == 0 || cp->capture_rows == 0) return;
    for (int r = 0; r < t->n_recorders; r++) {
        p->cd.push_back(cp->rec_capture_capacity[r]);
        p->cd.push_back(cp->rec_capture_start[r]);
    }
    p->capture_rows = cp->capture_rows;
}

// Absorbing coatings (validated tables; nothing is placed when no coating absorbs): the records and tables of
// PackedScene::cabs_d appended to the double blob, the candidate tables of the `detected` selector (PackedScene::dcand_i)
// to the int blob -- behind everything the scene holds without them, so no other offset moves.
void pack_absorb(const SceneInputs& in, const Records& recs, PackedScene* p) {
    const PvtSceneTables* t = in.t;
    const PvtCoatingAbsorbTables* ab = in.ab;
    p->cabs_d = -1;
    p->dcand_i = -1;
    if (!ab || ab->n_coatings == 0) return;
    const int K = t->n_coatings, NT = ab->n_tables;
    bool any = false;
    for (int k = 0; k < K; k++) any = any || ab->coat_absorptivity[k] > 0.0 || (NT > 0 && ab->coat_table[k] >= 0);
    if (!any) return;
    std::vector<double>& gd = p->gd;
    p->cabs_d = (int)gd.size();
    gd.resize(gd.size() + (size_t)K * kCa, 0.0);
    const GridTables atabs = grid_tables(ab);
    std::vector<int> tab_at((size_t)(NT > 0 ? NT : 0), -1);
    for (int k = 0; k < K; k++) {
        const int j = NT > 0 ? ab->coat_table[k] : -1;
        if (j >= 0 && tab_at[(size_t)j] < 0) {   // (a reflectivity table's layout)
            tab_at[(size_t)j] = (int)gd.size();
            gd.resize(gd.size() + (size_t)atabs.doubles(j));
            put_grid_table(atabs, j, gd.data() + tab_at[(size_t)j]);
        }
        double* d = gd.data() + p->cabs_d + (size_t)k * kCa;
        d[kCaA] = ab->coat_absorptivity[k];
        d[kCaNw] = j >= 0 ? ab->table_nw[j] : 0;   // 0: no table
        d[kCaNa] = j >= 0 ? ab->table_na[j] : 0;
        d[kCaTab] = j >= 0 ? tab_at[(size_t)j] : 0;
    }
    gd.push_back(0.0);   // (the blob's spare last element, as before)
    std::vector<int>& gi = p->gi;
    p->dcand_i = (int)gi.size();
    gi.resize(gi.size() + (size_t)recs.n_cand * 8 + (size_t)t->n_recorders + 1, 0);
    fill_candidates(t, recs, p, true);
}

// Patterned coatings (PvtCoatingPatternTables, pvt_scene_create_pattern; called on a scene pack_scene has accepted, before
// anything is uploaded): every index the kernel follows is checked, then PackedScene::pd and ::pmask are filled.  Both stay
// empty -- the scene is then exactly the one without the struct -- when no row has a pattern or an any-facet flag.
int pack_patterns(const SceneInputs& in, PackedScene* p) {
    const PvtSceneTables* t = in.t;
    const PvtCoatingPatternTables* pt = in.pt;
    p->pd.clear();
    p->pmask.clear();
    if (!pt || pt->n_coatings == 0) return PVT_OK;
    const int K = t->n_coatings, P = pt->n_patterns;
    if (pt->n_coatings != K || !pt->coat_any_facet || !pt->coat_pattern)
        return fail(PVT_ERR_INVALID, "pattern tables: need one flag and one pattern id per coating");
    if (P < 0 || pt->n_mask < 0 || pt->n_mask > (1ll << 26)) return fail(PVT_ERR_INVALID, "pattern tables: more than 2^26 mask cells");
    if (P > 0 && (!pt->shape || !pt->bounded || !pt->lower || !pt->h || !pt->mask_start || !pt->mask))
        return fail(PVT_ERR_INVALID, "pattern tables: missing arrays");
    for (int j = 0; j < P; j++) {
        long long cells = 1;
        for (int a = 0; a < 3; a++) {
            const long long n = pt->shape[j * 3 + a];
            if (n < 1) return fail(PVT_ERR_INVALID, "pattern tables: shape must be >= 1 on each axis");
            cells *= n;
            if (cells > (1ll << 26)) return fail(PVT_ERR_INVALID, "pattern tables: more than 2^26 mask cells");
            if (pt->bounded[j * 3 + a] == 0) {
                if (n != 1) return fail(PVT_ERR_INVALID, "pattern tables: an unbounded axis has one cell");
                continue;
            }
            const double h = pt->h[j * 3 + a];
            if (!std::isfinite(pt->lower[j * 3 + a])) return fail(PVT_ERR_INVALID, "pattern tables: lower bounds must be finite");
            if (!(std::isfinite(h) && h > 0.0)) return fail(PVT_ERR_INVALID, "pattern tables: cell widths must be finite and > 0");
        }
        const long long m0 = pt->mask_start[j];
        if (m0 < 0 || m0 > pt->n_mask || cells > pt->n_mask - m0) return fail(PVT_ERR_INVALID, "pattern tables: mask range out of bounds");
    }
    bool any = false;
    for (int k = 0; k < K; k++) {
        if (pt->coat_pattern[k] < -1 || pt->coat_pattern[k] >= P) return fail(PVT_ERR_INVALID, "pattern tables: coating row names a missing pattern");
        any = any || pt->coat_pattern[k] >= 0 || pt->coat_any_facet[k] != 0;
    }
    if (!any) return PVT_OK;
    std::vector<double>& pd = p->pd;
    pd.assign((size_t)2 * K + (size_t)P * kPr, 0.0);
    const double mask_at = (double)(pd.size() * sizeof(double));   // (< 2^53: exact)
    for (int k = 0; k < K; k++) {
        pd[(size_t)2 * k] = pt->coat_pattern[k] >= 0 ? (double)(2 * K + pt->coat_pattern[k] * kPr) : -1.0;
        pd[(size_t)2 * k + 1] = pt->coat_any_facet[k] != 0 ? 1.0 : 0.0;
    }
    for (int j = 0; j < P; j++) {
        double* q = pd.data() + (size_t)2 * K + (size_t)j * kPr;
        for (int a = 0; a < 3; a++) {
            const bool bounded = pt->bounded[j * 3 + a] != 0;
            q[kPrShape + a] = (double)pt->shape[j * 3 + a];
            q[kPrBounded + a] = bounded ? 1.0 : 0.0;
            q[kPrLower + a] = bounded ? pt->lower[j * 3 + a] : 0.0;
            q[kPrH + a] = bounded ? pt->h[j * 3 + a] : 1.0;
        }
        q[kPrMask] = mask_at + (double)pt->mask_start[j];
    }
    p->pmask.assign(pt->mask, pt->mask + pt->n_mask);
    if (p->pmask.empty()) p->pmask.push_back(0);   // (flags alone: the buffer still ends in a byte)
    return PVT_OK;
}

// Aligned components (PvtAlignTables, pvt_scene_create_aligned; called on a scene pack_scene has accepted, before anything
// is uploaded): every value the kernel reads is checked, each failure with its own message, then PackedScene::ad is filled.
// It stays empty -- the scene is then exactly the one without the struct -- when no component names a record.
int pack_align(const SceneInputs& in, PackedScene* p) {
    const PvtSceneTables* t = in.t;
    const PvtAlignTables* al = in.al;
    p->aligned = false;
    if (!al || al->n_components == 0) return PVT_OK;
    const int C = t->n_components, N = t->n_nodes, R = al->n_records;
    if (al->n_components != C || !al->comp_align) return fail(PVT_ERR_INVALID, "align tables: need one record index per component");
    if (R < 0 || (R > 0 && (!al->axis || !al->abs_order || !al->emit_table))) return fail(PVT_ERR_INVALID, "align tables: missing arrays");
    bool any = false;
    for (int c = 0; c < C; c++) {
        if (al->comp_align[c] < -1 || al->comp_align[c] >= R) return fail(PVT_ERR_INVALID, "align tables: component names a missing record");
        any = any || al->comp_align[c] >= 0;
    }
    if (!any) return PVT_OK;
    const PvtPhaseTables* ph = in.ph;
    const int NP = ph ? ph->n_tables : 0;
    for (int r = 0; r < R; r++) {
        const double x = al->axis[r * 3], y = al->axis[r * 3 + 1], z = al->axis[r * 3 + 2];
        const double len2 = (x * x + y * y) + z * z;
        if (!(std::isfinite(len2) && std::fabs(len2 - 1.0) <= 1e-12)) return fail(PVT_ERR_INVALID, "align tables: every axis must be a unit vector within 1e-12");
        const double s = al->abs_order[r];
        if (!std::isfinite(s)) return fail(PVT_ERR_INVALID, "align tables: absorption orders must be finite");
        if (!(s >= -0.5 && s <= 1.0)) return fail(PVT_ERR_INVALID, "align tables: absorption orders must lie in [-0.5, 1]");
        const int j = al->emit_table[r];
        if (j < -1 || j >= NP) return fail(PVT_ERR_INVALID, "align tables: emission table outside the phase tables");
        if (j >= 0 && ph->table_nw[j] != 1) return fail(PVT_ERR_INVALID, "align tables: an emission table must have a single row");
    }
    for (int n = 0; n < N; n++)
        for (int k = 0; k < t->comp_count[n]; k++) {
            const int c = t->comp_start[n] + k;
            if (c < 0 || c >= C) return fail(PVT_ERR_INVALID, "component run out of range");
            const int r = al->comp_align[c];
            if (r < 0) continue;
            if (n == t->root_id) return fail(PVT_ERR_INVALID, "align tables: the root node cannot hold an aligned component");
            if (in.fr && in.fr->n_nodes == N && in.fr->node_field[n] >= 0)
                return fail(PVT_ERR_INVALID, "align tables: an aligned component in a node with a concentration field is out of scope");
            const int j = al->emit_table[r];
            if (j >= 0 && (t->comp_phase_type[c] != PVT_PHASE_TABLE || ph->comp_table[c] != j))
                return fail(PVT_ERR_INVALID, "align tables: a component's emission table must be the phase table it names");
        }
    std::vector<double>& fd = p->fd;
    if (fd.empty()) fd.assign((size_t)N, -1.0);
    long long words = (long long)fd.size();
    for (int n = 0; n < N; n++) words += kFrComp + (long long)t->comp_count[n] * (1 + kAl);
    if (words > 0x7fffffffLL) return fail(PVT_ERR_INVALID, "align tables: more doubles than int32 offsets can index");
    for (int n = 0; n < N; n++) {
        bool holds = false;
        for (int k = 0; k < t->comp_count[n]; k++) holds = holds || al->comp_align[t->comp_start[n] + k] >= 0;
        if (!holds) continue;
        const size_t at = fd.size();
        fd[(size_t)n] = (double)at;
        fd.resize(at + kFrComp + (size_t)t->comp_count[n], 0.0);   // (kFrShape stays 0: no lattice)
        for (int k = 0; k < t->comp_count[n]; k++) {
            const int r = al->comp_align[t->comp_start[n] + k];
            if (r < 0) { fd[at + kFrComp + (size_t)k] = -1.0; continue; }
            const size_t q = fd.size();
            fd[at + kFrComp + (size_t)k] = (double)q;
            fd.resize(q + kAl, 0.0);
            fd[q + kAlOn] = 1.0;
            for (int a = 0; a < 3; a++) fd[q + kAlAxis + a] = al->axis[r * 3 + a];
            fd[q + kAlOrder] = al->abs_order[r];
            fd[q + kAlEmit] = al->emit_table[r] >= 0 ? 1.0 : 0.0;
        }
    }
    p->aligned = true;
    return PVT_OK;
}

// Convex polyhedra (PvtPolyhedronTables, pvt_scene_create_polyhedra): every value the kernel reads, checked before anything
// is packed, each failure with its own message.  A scene with no node of the type needs no struct and reads none.
int validate_polyhedra(const SceneInputs& in) {
    const PvtSceneTables* t = in.t;
    const PvtPolyhedronTables* pl = in.pl;
    const int N = t->n_nodes;
    for (int n = 0; n < N; n++) {
        if (t->geom_type[n] != PVT_GEOM_POLYHEDRON) continue;
        if (!pl || pl->n_nodes == 0) return fail(PVT_ERR_INVALID, "polyhedron node without polyhedron tables");
        if (pl->n_nodes != N || !pl->node_plane_start || !pl->node_plane_count || !pl->planes || pl->n_planes < 0)
            return fail(PVT_ERR_INVALID, "polyhedron tables: need one run of planes per node");
        const long long start = pl->node_plane_start[n], count = pl->node_plane_count[n];
        if (count < 4 || count > PVT_MAX_POLYHEDRON_PLANES) return fail(PVT_ERR_INVALID, "polyhedron tables: a node needs 4 to 64 planes");
        if (bad_run(start, count, pl->n_planes)) return fail(PVT_ERR_INVALID, "polyhedron tables: plane range outside the pool");
        for (long long k = start; k < start + count; k++) {
            const double* r = pl->planes + k * 4;
            if (!(std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]) && std::isfinite(r[3])))
                return fail(PVT_ERR_INVALID, "polyhedron tables: plane rows must be finite");
            const double len = std::sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
            if (!(std::fabs(len - 1.0) <= 1e-12)) return fail(PVT_ERR_INVALID, "polyhedron tables: every normal must be a unit vector within 1e-12");
        }
        const double radius = t->geom_params[n * 4];
        if (!(std::isfinite(radius) && radius > 0.0)) return fail(PVT_ERR_INVALID, "polyhedron: bounding radius must be finite and > 0");
    }
    return PVT_OK;
}

// ... and placed (validated tables): the rows of every such node appended to the double blob, its record told where
void pack_polyhedra(const SceneInputs& in, PackedScene* p) {
    const PvtSceneTables* t = in.t;
    p->has_polyhedron = false;
    for (int n = 0; n < t->n_nodes; n++) {
        if (t->geom_type[n] != PVT_GEOM_POLYHEDRON) continue;
        p->has_polyhedron = true;
        const int start = in.pl->node_plane_start[n], count = in.pl->node_plane_count[n];
        double* d = p->gd.data() + (size_t)n * ND;
        const unsigned long long at = (unsigned long long)p->gd.size(), rows = (unsigned long long)count;
        std::memcpy(&d[ND_PARAMS + 1], &at, 8);     // (integers in the words' bits, like ND_BITS: the kernel converts nothing)
        std::memcpy(&d[ND_PARAMS + 2], &rows, 8);
        p->gd.insert(p->gd.end(), in.pl->planes + (size_t)start * 4, in.pl->planes + (size_t)(start + count) * 4);
    }
    if (p->has_polyhedron) p->gd.push_back(0.0);   // (the blob's spare last element, as before)
}

// Conicoids (validated parameters): the four of every such node appended to the double blob, its record told where
void pack_conicoids(const SceneInputs& in, PackedScene* p) {
    const PvtSceneTables* t = in.t;
    p->has_conicoid = false;
    for (int n = 0; n < t->n_nodes; n++) {
        if (t->geom_type[n] != PVT_GEOM_CONICOID) continue;
        p->has_conicoid = true;
        double* d = p->gd.data() + (size_t)n * ND;
        const unsigned long long at = (unsigned long long)p->gd.size();
        std::memcpy(&d[ND_PARAMS + 1], &at, 8);     // (an integer in the word's bits, as a polyhedron's)
        d[ND_PARAMS + 2] = 0.0;
        p->gd.insert(p->gd.end(), t->geom_params + (size_t)n * 4, t->geom_params + (size_t)n * 4 + 4);
    }
    if (p->has_conicoid) p->gd.push_back(0.0);   // (the blob's spare last element, as before)
}

// The scene's inputs (n_nodes and n_recorders already checked by the caller; the pattern tables are pack_patterns') -> *p.
// No HIP call.
int pack_scene(const SceneInputs& in, PackedScene* p) {
    const PvtSceneTables* t = in.t;
    const PvtIndexTables* x = in.x;
    const PvtPhaseTables* ph = in.ph;
    const PvtSurfaceTables* rs = in.rs;
    int rc = validate_tables(in);
    if (rc != PVT_OK) return rc;
    rc = validate_polyhedra(in);
    if (rc != PVT_OK) return rc;
    const Classes classes = classify_nodes(in);
    Spectra spectra = pool_spectra(t);
    const Records records = component_records(in, spectra, classes.by_node);
    NodeGrid grid;
    p->grid = plan_node_grid(t, &grid);
    for (int a = 0; a < 3; a++) p->grid_dims[a] = p->grid ? grid.n[a] : 0;
    p->n_ctab = t->n_coatings > 0 ? t->n_coat_tables : 0;
    p->n_rtab = 0;   // (a table no node uses is validated, never placed)
    if (x)
        for (int n = 0; n < t->n_nodes; n++)
            if (x->n_tables > 0 && x->node_table[n] >= 0) p->n_rtab = x->n_tables;
    p->n_ptab = 0;   // (likewise: a table no component and no coating lobe uses is validated, never placed)
    if (ph)
        for (int c = 0; c < t->n_components; c++)
            if (ph->n_tables > 0 && ph->comp_table[c] >= 0) p->n_ptab = ph->n_tables;
    bool lobes = false;
    for (int k = 0; k < t->n_coatings; k++)
        lobes = lobes || t->coat_reflect_mode[k] >= PVT_COAT_LOBE || t->coat_transmit_mode[k] >= PVT_COAT_LOBE;
    if (lobes) p->n_ptab = ph->n_tables;   // (validated: the phase tables are there)
    p->rough_d = -1;   // (a struct of zeros places nothing: the scene lays out as a smooth one)
    if (rs && rs->n_nodes > 0)
        for (int n = 0; n < t->n_nodes; n++)
            if (rs->node_roughness[n] > 0.0) p->rough_d = 0;
    p->has_frustum = false;
    for (int n = 0; n < t->n_nodes; n++)
        if (t->geom_type[n] == PVT_GEOM_FRUSTUM) p->has_frustum = true;
    std::vector<int> rtab_at, ptab_at;
    const std::vector<int> ctab_at = lay_out(in, classes, spectra, records, grid, p, &rtab_at, &ptab_at);
    rc = fill(in, classes, spectra, records, grid, ctab_at, rtab_at, ptab_at, p);
    if (rc != PVT_OK) return rc;
    pack_fields(in, p);
    pack_maps(in, p);
    pack_captures(in, p);
    pack_absorb(in, records, p);
    p->clobe_i = -1;
    if (lobes) {   // (validated words) the rows' lobe records, behind everything else in the int blob
        std::vector<int>& gi = p->gi;
        p->clobe_i = (int)gi.size();
        gi.resize(gi.size() + (size_t)t->n_coatings * kCl + 1, 0);   // (and the blob's spare last element, as before)
        for (int k = 0; k < t->n_coatings; k++) {
            int* q = gi.data() + p->clobe_i + (size_t)k * kCl;
            const int rm = t->coat_reflect_mode[k] - PVT_COAT_LOBE, tm = t->coat_transmit_mode[k] - PVT_COAT_LOBE;
            q[kClRTab] = rm >= 0 ? ptab_at[(size_t)(rm >> 2)] : -1;
            q[kClRAxis] = rm >= 0 ? (rm & 3) : 0;
            q[kClTTab] = tm >= 0 ? ptab_at[(size_t)(tm >> 2)] : -1;
            q[kClTAxis] = tm >= 0 ? (tm & 3) : 0;
        }
    }
    pack_polyhedra(in, p);
    pack_conicoids(in, p);
    prove_shortcuts(t, p);
    prove_lean(t, p);
    prove_solo(t, p);
    return PVT_OK;
}

}  // namespace
