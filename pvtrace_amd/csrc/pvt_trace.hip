// pvt_trace.hip — the photon loop of pvtrace on CDNA4 (gfx950), and the C ABI
// declared in include/pvtrace_hip.h.
//
// What it replaces: reference pvtrace/engine/_kernel.pyx trace_one / trace_bundle
// (:603-1115), i.e. the per-photon while-alive loop behind engine.simulate().
// This is not a translation of that file: the reference walks one ray per CPU
// thread through per-thread scratch arrays; here
//
//   * one wavefront LANE owns one live photon; a persistent workgroup keeps all
//     64 lanes of each wave busy by refilling dead lanes from a global ray
//     cursor (wave-level ballot + prefix rank, one atomic per 64 rays);
//   * the scene tables (a few KB) are packed once into two blobs in HBM and
//     staged into LDS per workgroup; wave-uniform reads (the node loop, the
//     recorder loop) go through the scalar cache from the global copy, lane-
//     divergent reads (spectra binary search, per-lane node rows) hit LDS;
//   * hit classification is streaming (nearest / second nearest / container are
//     folded while the nodes are intersected) — no per-ray hit arrays;
//   * every lane's event (row to log, recorder to tally) is deferred to ONE
//     re-converged block at the end of the step instead of being emitted from
//     each divergent branch;
//   * recorders accumulate in LDS (integer + f64 atomics) and are flushed with
//     one global atomic per slot per workgroup; the statistics of first
//     crossings (angle, sums, histograms) are parked 64 per wave and computed
//     together;
//   * what the host can prove about a scene is decided once, not per photon:
//     arithmetic table indices on even grids (the abscissae are not even stored),
//     cosine thresholds for total internal reflection, the world node visited
//     lazily, photons that can only leave the scene ended where they leave the
//     last box (tally launches; each with a proof obligation checked per lane
//     where one is needed);
//   * all arithmetic is FP64 with FMA contraction off and the transcendental
//     functions of pvt_math.h, so a photon's whole history is bit-identical to
//     the CPU referee (oracle/pvt_oracle.c, math_mode 1).
//
// No MFMA: there is no dense contraction anywhere on this path.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <chrono>
#include <dlfcn.h>
#include <string>
#include <thread>
#include <type_traits>
#include <mutex>
#include <vector>

#include "../../include/pvtrace_hip.h"
#include "pvt_math.h"
#include "pvt_bvh.h"

#include "pvt_trace_kernel.h"

namespace {

// ============================================================== host side
thread_local std::string g_error;

int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}
#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(PVT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#if PVT_TIMELINE
constexpr int kTlLaunches = 48, kTlWgs = 1024;
constexpr size_t kTlBytes = (size_t)kTlLaunches * kTlWgs * kWaves * 8 * 8;
unsigned long long* g_timeline = nullptr;
int g_tl_launch = 0, g_tl_grid[kTlLaunches] = {0};
long long g_tl_n[kTlLaunches] = {0};
void timeline_dump();
#endif

template <class T>
int push(std::vector<T>& blob, const T* src, size_t n) {
    int at = (int)blob.size();
    if (n && src) blob.insert(blob.end(), src, src + n);
    return at;
}

}  // namespace

#include "pvt_scene_pack.h"

struct PvtScene {
    int device = 0;
    Lay lay{};
    EmitOff eoff{};
    int nd = 0, ni = 0;
    int nd_small = 0, ni_small = 0;   // ... of which everything but the spectra / their guide tables (the blobs' heads)
    int n_nodes = 0, root = 0, n_rec = 0, total_bins = 0, n_coat = 0, n_ctab = 0, n_rtab = 0, n_lights = 0;
    int rough_d = -1;                   // where the nodes' GGX widths start in the double blob (-1: no rough node)
    bool has_frustum = false;           // a node is a truncated cone (PVT_GEOM_FRUSTUM): only the extension family traces one
    bool has_polyhedron = false;        // a node is a convex polyhedron (PVT_GEOM_POLYHEDRON): likewise
    bool has_conicoid = false;          // a node is a solid of revolution of a conic (PVT_GEOM_CONICOID): likewise
    int clobe_i = -1;                   // scattering coatings: the coating rows' lobe records in the int blob (KArgs::clobe_i; -1 = no coating has a lobe)
    int cabs_d = -1, dcand_i = -1;      // absorbing coatings: their records in the double blob, the `detected` candidate tables in the int blob (-1: none)
    double* d_fd = nullptr;             // the concentration fields (KArgs::fd), null = no node carries a lattice
    double* d_md = nullptr;             // the volume maps' records (KArgs::md), null = the scene has no map
    int pd_d = -1;                      // the coating patterns' flags, records and masks: where they start behind the double blob, in its allocation (KArgs::pd_d; -1 = no coating has a pattern or covers any normal)
    int al_d = -1;                      // >= 0: the scene has aligned components, their records lie in d_fd and its launches run the family's kExtAligned kernels (-1 = no component is aligned)
    long long map_slots = 0;            // int64 slots the maps add behind the recorders' bins (pvt_scene_map_slots)
    bool path_maps = false;             // one of the maps is a path-length map (PVT_MAP_PATHLENGTH): the scene's launches run the family's kExtPath kernels
    long long* d_cd = nullptr;          // ray capture: capacity and first row per recorder (KArgs::cap_tab), null = none captured
    long long capture_rows = 0;         // rows of all captures of one tally set (pvt_scene_capture_rows)
    double* d_gd = nullptr;
    int* d_gi = nullptr;
    double* d_ed = nullptr;
    int* d_ei = nullptr;
    pvt::BvhNode* d_bvh = nullptr;      // triangle meshes: BVH nodes + gathered triangles
    pvt::MeshTri* d_tris = nullptr;
    pvt::BvhNode* d_bvh_top = nullptr;  // the top levels of the trees as a workgroup copies them to LDS (pvt_bvh.h: stage_top)
    int top_n = 0;                      // ... records of it
    int meshq = 0;                      // leaves a lane of a mesh walk notes in LDS before their triangles are tested (1 or kMeshQ)
    unsigned int* d_set_cursor = nullptr;   // kCursorSlots x kMaxSets cursors: launches with tally sets
    unsigned long long* d_counters = nullptr;   // step counters and clocks: 64 rows x 8 words (KArgs::counters, pvt_scene_counters / _clock)
    unsigned long long* d_stamp = nullptr;      // kCursorSlots x {start, end} of a stream's last launch, 100 MHz ticks (KArgs::stamp)
    unsigned int* d_cursor = nullptr;   // kCursorSlots cursors (64 B apart), one per stream: launches on
                                        // different streams may overlap, each needs its own
    std::mutex slot_mutex;              // launches on one stream are ordered and may share a cursor;
    std::vector<hipStream_t> slot_of;   // index = cursor slot owned by that stream
    // pvt_trace_device with column arrays: the kernel's 128-byte event records are staged here (one buffer per
    // stream slot, grown on demand, at most `stage_limit` bytes: larger logs are traced in several launches)
    std::vector<unsigned long long*> stage;
    std::vector<size_t> stage_bytes;
    size_t stage_limit = (size_t)1 << 30;
    // photons carried from launch to launch of a stream (PVT_FLAG_CARRY_OUT; see KArgs::carry_in): per stream slot
    // two buffers (the launch that resumes one may park into the other) and which of them holds parked photons
    struct Carry {
        unsigned long long* buf[2] = {nullptr, nullptr};
        int parity = 0;            // the NEXT launch parks into buf[parity]
        int phase = 0;             // ... and uses cursor block `phase` of the slot's three (see trace_launch)
        bool pending = false;      // buf[parity ^ 1] holds photons parked by the previous launch
        long long bound = 0;       // at most this many
        int maxsteps = 0, emit_method = 0;   // ... under these rules: the launch that resumes them must trace by the same
    };
    std::vector<Carry> carry;
    // device emission: per stream slot, [7][64] doubles per wave of the launch (KArgs::emit_pool), grown on demand
    std::vector<double*> emit_pool;
    std::vector<size_t> emit_pool_bytes;
    // launch origin: per stream slot, [lanes of the launch][kOriginWords] doubles (KArgs::origin_store), grown on demand
    std::vector<double*> origin_store;
    std::vector<size_t> origin_store_bytes;
    unsigned int carry_cap = 0;    // photons one buffer holds (a launch of more lanes than that does not park)
    int num_cu = 0;
    int last_grid = 0, last_lds = 0;
    size_t lds_limit = 0;
    int lazy_root = 0;              // 1 box / 2 sphere root that strictly contains every other node (see the kernel's node loop)
    double lazy_k = 0.0;            // sphere root: 1 / (2 radius)
    bool exit_observed = false;     // a recorder listens to (root, exit)
    bool grid = false;              // the scene has a node grid (many nodes; see plan_node_grid)
    int grid_dims[3] = {0, 0, 0};
    bool fuse_exit = false;         // see prove_shortcuts: photons leaving the only child's surface outwards are done
    bool hist_reads_position = false;   // a histogram axis is x, y or z
    bool hist_reads_counter = false;    // a histogram axis is a photon event counter
    int origin_mask = 0;                // bit k: a histogram axis is PVT_PROPX_ORIGIN_WAVELENGTH + k (KArgs::origin)
    // KArgs::count: 0 the scene counts nothing, 1 its photons carry their event counters (a captured recorder), 2 a histogram
    // reads one as well
    int counting() const { return hist_reads_counter ? 2 : d_cd ? 1 : 0; }
    bool lean_ok = false;           // see prove_lean: launches with the tables in LDS run the trace_kernel_lean family ...
    bool lean_even = false;         // ... its EVEN kernels (every spectrum a constant or on a proven even grid)
    int last_variant = -1;          // PVT_VARIANT_* of the last launch (-1: none yet)
    bool solo = false;              // see prove_solo: tally launches with `lazy_root` and `fuse_exit` run the trace_kernel_solo entries
    bool last_solo = false;         // ... whether the last launch did (Variant::solo)
    bool last_park = false;         // ... and whether it ran the family's parking entry (Variant::park)
};

extern "C" {

int pvt_abi_version(void) { return PVT_ABI_VERSION; }
const char* pvt_last_error(void) { return g_error.c_str(); }

int pvt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The emitter's blobs, and behind them the records of its tabulated sources (`src` null: none; validated by the caller):
// a PVT_POS_GRID light's pos_param[0] and a PVT_DIR_TABLE light's dir_param are overwritten with where its grid's (kSg*)
// and its table's record ({n_wavelength, n_mu}, wavelengths, mu, CDF rows: what phase_table_turn reads) start in `ed`.
static int pack_emitter(PvtScene* s, const PvtEmitterTables* e, const PvtSourceTables* src) {
    HIP_TRY(hipSetDevice(s->device));
    std::vector<double> ed;
    std::vector<int> ei;
    EmitOff o{};
    const int Lt = e->n_lights;
    o.wl_value = push(ed, e->wl_value, Lt);
    o.pos_param = push(ed, e->pos_param, (size_t)Lt * 3);
    o.dir_param = push(ed, e->dir_param, Lt);
    o.l2w = push(ed, e->light_to_world, (size_t)Lt * 16);
    o.spec_x = push(ed, e->spec_x, e->n_spec);
    o.spec_cdf = push(ed, e->spec_cdf, e->n_spec);
    o.wl_type = push(ei, e->wl_type, Lt);
    o.wl_spec_start = push(ei, e->wl_spec_start, Lt);
    o.wl_spec_n = push(ei, e->wl_spec_n, Lt);
    o.pos_type = push(ei, e->pos_type, Lt);
    o.dir_type = push(ei, e->dir_type, Lt);
    if (src) {
        std::vector<int> grid_at(src->n_grids > 0 ? src->n_grids : 0), table_at(src->n_tables > 0 ? src->n_tables : 0);
        for (int g = 0; g < src->n_grids; g++) {
            grid_at[g] = (int)ed.size();
            size_t cells = 1;
            for (int a = 0; a < 3; a++) { ed.push_back((double)src->grid_shape[g * 3 + a]); cells *= (size_t)src->grid_shape[g * 3 + a]; }
            for (int a = 0; a < 3; a++) ed.push_back(src->grid_bounded[g * 3 + a] != 0 ? 1.0 : 0.0);
            push(ed, src->grid_lower + g * 3, 3);
            push(ed, src->grid_h + g * 3, 3);
            push(ed, src->grid_cdf + src->grid_cdf_start[g], cells + 1);
        }
        for (int j = 0; j < src->n_tables; j++) {
            table_at[j] = (int)ed.size();
            const size_t nw = (size_t)src->table_nw[j], nm = (size_t)src->table_nmu[j];
            ed.push_back((double)nw);
            ed.push_back((double)nm);
            push(ed, src->table_wavelength + src->table_wl_start[j], nw);
            push(ed, src->table_mu + src->table_mu_start[j], nm);
            push(ed, src->table_cdf + src->table_cdf_start[j], nw * nm);
        }
        for (int i = 0; i < Lt; i++) {
            if (src->light_grid[i] >= 0) ed[o.pos_param + (size_t)i * 3] = (double)grid_at[src->light_grid[i]];
            if (src->light_table[i] >= 0) ed[o.dir_param + i] = (double)table_at[src->light_table[i]];
        }
    }
    ed.push_back(0.0);
    ei.push_back(0);
    if (s->d_ed) { (void)hipFree(s->d_ed); s->d_ed = nullptr; }
    if (s->d_ei) { (void)hipFree(s->d_ei); s->d_ei = nullptr; }
    HIP_TRY(hipMalloc(&s->d_ed, ed.size() * sizeof(double)));
    HIP_TRY(hipMalloc(&s->d_ei, ei.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(s->d_ed, ed.data(), ed.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_ei, ei.data(), ei.size() * sizeof(int), hipMemcpyHostToDevice));
    s->eoff = o;
    s->n_lights = Lt;
    return PVT_OK;
}

int pvt_sources_check(const PvtEmitterTables* e, const PvtSourceTables* src) { return validate_sources(e, src); }

int pvt_scene_set_emitter(PvtScene* s, const PvtEmitterTables* e) {
    if (!s || !e || e->n_lights <= 0) return fail(PVT_ERR_INVALID, "bad emitter");
    const int rc = validate_sources(e, nullptr);
    return rc != PVT_OK ? rc : pack_emitter(s, e, nullptr);
}

int pvt_scene_set_sources(PvtScene* s, const PvtEmitterTables* e, const PvtSourceTables* src) {
    if (!s || !e || e->n_lights <= 0) return fail(PVT_ERR_INVALID, "bad emitter");
    const int rc = validate_sources(e, src);
    return rc != PVT_OK ? rc : pack_emitter(s, e, src);
}

void pvt_scene_destroy(PvtScene* s) {
    if (!s) return;
#if PVT_TIMELINE
    timeline_dump();
#endif
    (void)hipSetDevice(s->device);
    if (s->d_gd) (void)hipFree(s->d_gd);
    if (s->d_fd) (void)hipFree(s->d_fd);
    if (s->d_md) (void)hipFree(s->d_md);
    if (s->d_cd) (void)hipFree(s->d_cd);
    if (s->d_gi) (void)hipFree(s->d_gi);
    if (s->d_ed) (void)hipFree(s->d_ed);
    if (s->d_ei) (void)hipFree(s->d_ei);
    if (s->d_cursor) (void)hipFree(s->d_cursor);
    if (s->d_set_cursor) (void)hipFree(s->d_set_cursor);
    if (s->d_counters) (void)hipFree(s->d_counters);
    if (s->d_stamp) (void)hipFree(s->d_stamp);
    if (s->d_bvh) (void)hipFree(s->d_bvh);
    if (s->d_bvh_top) (void)hipFree(s->d_bvh_top);
    if (s->d_tris) (void)hipFree(s->d_tris);
    for (auto* b : s->stage) if (b) (void)hipFree(b);
    for (auto& c : s->carry) for (auto* b : c.buf) if (b) (void)hipFree(b);
    for (auto* b : s->emit_pool) if (b) (void)hipFree(b);
    for (auto* b : s->origin_store) if (b) (void)hipFree(b);
    delete s;
}

}  // extern "C"

namespace {

KArgs base_args(const PvtScene* s, const PvtTraceParams* p) {
    KArgs a{};
    a.gd = s->d_gd; a.gi = s->d_gi; a.ed = s->d_ed; a.ei = s->d_ei;
    a.bvh = s->d_bvh; a.tris = s->d_tris;
    a.lay = s->lay; a.eoff = s->eoff;
    a.nd = s->nd; a.ni = s->ni;
    a.nd_lds = 0; a.ni_lds = 0;
    a.n_nodes = s->n_nodes; a.root = s->root; a.n_rec = s->n_rec; a.total_bins = s->total_bins;
    a.n_coat = s->n_coat; a.n_ctab = s->n_ctab; a.n_rtab = s->n_rtab; a.n_lights = s->n_lights;
    a.rough_d = s->rough_d;
    a.cabs_d = s->cabs_d; a.dcand_i = s->dcand_i;
    a.clobe_i = s->clobe_i;
    a.fd = s->d_fd;
    a.md = s->d_md;
    a.pd_d = s->pd_d;
    a.cap_tab = s->d_cd;
    a.cap_total = s->capture_rows;
    a.count = s->counting();
    a.origin = s->origin_mask;
    a.n_rays = (unsigned int)p->n_rays;
    a.cursor = s->d_cursor;
    a.counters = s->d_counters;
    a.seed = p->seed + p->ray_offset;
    a.emit_seed = p->emit_seed;
    a.ray_offset = p->ray_offset;
    a.maxsteps = p->maxsteps; a.max_events = p->max_events; a.emit_method = p->emit_method;
    a.record_every = p->record_every;
    return a;
}

// cursor / staging slot of a stream (launches on one stream are ordered and share it); -1, and the error said, when all are taken
int slot_of_stream(PvtScene* s, hipStream_t st) {
    std::lock_guard<std::mutex> lock(s->slot_mutex);
    size_t slot = 0;
    while (slot < s->slot_of.size() && s->slot_of[slot] != st) slot++;
    if (slot == s->slot_of.size()) {
        if (slot >= (size_t)kCursorSlots)
            return fail(-1, "more than 64 HIP streams are tracing this scene; create one scene per group of streams");
        s->slot_of.push_back(st);
        s->stage.push_back(nullptr);
        s->stage_bytes.push_back(0);
        s->carry.emplace_back();
        s->emit_pool.push_back(nullptr);
        s->emit_pool_bytes.push_back(0);
        s->origin_store.push_back(nullptr);
        s->origin_store_bytes.push_back(0);
    }
    return (int)slot;
}

int check_trace_args(PvtScene* s, const PvtRays* rays, const PvtTraceParams* p, const PvtTallies* tl) {
    if (!s || !p || !tl) return fail(PVT_ERR_INVALID, "null argument");
    if (p->n_rays < 0 || p->n_rays > 0x7fffffffLL)
        return fail(PVT_ERR_INVALID, "n_rays must fit in 31 bits per bundle");
    if (p->max_events < 2 && p->record_every > 0) return fail(PVT_ERR_INVALID, "max_events must be >= 2");
    if (!rays && !s->d_ed && p->n_rays > 0) return fail(PVT_ERR_INVALID, "no rays and no emitter");
    if ((p->flags & PVT_FLAG_CARRY_OUT) && (p->record_every > 0 || p->tally_bundle > 0))
        return fail(PVT_ERR_INVALID, "PVT_FLAG_CARRY_OUT is for plain tally launches (record_every == 0, no tally sets)");
    if (p->tally_bundle > 0 && p->record_every > 0) return fail(PVT_ERR_INVALID, "tally_bundle needs record_every == 0");
    // (photon event counters: kCountBits each, no saturation in the loop -- a step writes at most kCountRowsPerStep rows of one
    // counted kind, a photon takes at most maxsteps steps)
    if (s->counting() && (long long)p->maxsteps * kCountRowsPerStep > (1LL << kCountBits) - 1)
        return fail(PVT_ERR_INVALID, "maxsteps too large for the photon event counters of this scene (a counter histogram or a "
                                     "captured recorder): at most " + std::to_string(((1LL << kCountBits) - 1) / kCountRowsPerStep));
    return PVT_OK;
}

// Where a launch reads the scene tables from (the kernels' TAB_LDS): global memory, LDS, or LDS for the blobs' heads only.
enum class Tab { Global = 0, Lds = 1, Heads = 2 };

// LDS of a launch: recorder accumulators + control words, tables if they fit, bins if they fit, then the drain-phase
// consolidation buffer (kXSlots photon states, also the seed pools) within 40 KB: `bytes`.  Mesh walks add the lanes'
// noted leaves (at `meshq_off`), then the copy of the trees' top levels (at `top_off`): `total`.  These two
// (`s->meshq`, `s->top_n`) are reserved first, so that what is decided here still fits with them.
struct LdsPlan { size_t bytes; Tab tab; int bins_in_lds, xslots, tq_pos; bool ok; int meshq_off, top_off; size_t total; };
LdsPlan plan_lds(const PvtScene* s, bool record) {
    LdsPlan lp{0, Tab::Global, 0, 0, 0, true, -1, 0, 0};
    const size_t reserved = (size_t)s->meshq * kBlock * 4 + (size_t)s->top_n * sizeof(pvt::BvhNode);
    const size_t acc_bytes = (size_t)s->n_rec * (8 * 8 + 8) + (size_t)((s->n_rec + 1) & ~1) * 4 + CTL_WORDS * 4;
    const size_t tab_bytes = (size_t)s->nd * 8 + (size_t)((s->ni + 1) & ~1) * 4;
    const size_t bins_bytes = ((size_t)s->total_bins * 4 + 7) & ~(size_t)7;
    const size_t lds_limit = s->lds_limit - reserved;
    const size_t budget = (64 * 1024 < s->lds_limit ? 64 * 1024 : s->lds_limit) - reserved;  // keep >= 2 workgroups per CU
    // per-wave queues of first crossings awaiting their statistics (kernel: tally_flush)
    lp.tq_pos = s->hist_reads_position ? 1 : 0;
    // (a histogram that reads an event counter: one more column, the packed counters)
    // (... that reads a launch origin: one more for each origin that IS read, not kOriginWords -- LDS, as for the packed word)
    const size_t tq_bytes = (size_t)kWaves * kTallyQ * (((lp.tq_pos ? 7 : 4) + (s->hist_reads_counter ? 1 : 0) + __builtin_popcount((unsigned)s->origin_mask)) * 8 + 4);
    if (acc_bytes + tq_bytes > lds_limit) { lp.ok = false; return lp; }
    // (PVT_TABLES: developer / test switch -- "global": no tables in LDS, "heads": never the spectra)
    const char* force = getenv("PVT_TABLES");
    // spectra too large for LDS: everything else -- node, component and recorder records, class tables -- still is staged
    // (the blobs' heads; the spectra and their guide tables are read from global memory; mesh scenes stage all or none)
    const size_t small_bytes = (size_t)s->nd_small * 8 + (size_t)((s->ni_small + 1) & ~1) * 4;
    if (acc_bytes + tq_bytes + tab_bytes <= budget && !force) lp.tab = Tab::Lds;
    else if (s->meshq == 0 && acc_bytes + tq_bytes + small_bytes <= 40 * 1024 && acc_bytes + tq_bytes + small_bytes <= budget &&
             !(force && force[0] == 'g')) lp.tab = Tab::Heads;
    size_t lds = acc_bytes + tq_bytes + (lp.tab == Tab::Lds ? tab_bytes : lp.tab == Tab::Heads ? small_bytes : 0);
    lp.bins_in_lds = (lds + bins_bytes <= budget) ? 1 : 0;
    if (lp.bins_in_lds) lds += bins_bytes;
    // (a scene that counts: the global ray index, which captures read, and the event counters)
    // (one that reads a launch origin: its kOriginWords words; a buffer that no longer fits is done without, as ever)
    const size_t xw = xbuf_words(s->n_rec <= 64 ? 1 : 4, record, s->counting(), s->origin_mask != 0);
    const size_t xbytes = (size_t)kXSlots * xw * 8;
    // (mesh scenes do without: measured, repacking a draining workgroup buys their launches nothing, and the 9 KB hold
    // another level of the trees' top)
    if (s->meshq == 0 && lds + xbytes <= 40 * 1024 && lds + xbytes <= lds_limit) {
        lp.xslots = kXSlots;
        lds += xbytes;
    }
    lp.total = lp.bytes = (lds + 15) & ~(size_t)15;
    if (s->meshq) {
        lp.meshq_off = (int)lp.total;
        lp.total += (size_t)s->meshq * kBlock * 4;
        lp.top_off = (int)lp.total;
        lp.total += (size_t)s->top_n * sizeof(pvt::BvhNode);
    }
    return lp;
}

// Which kernel a launch runs: decided once, here.  `family` is what pvt_scene_variant reports; the other members are
// the template arguments of that family's entry points.
// `carry_out`: the launch parks its survivors for its successor -- its FINAL value, after bind_carry has had its say (a
// launch too wide to park finishes its own photons, and needs a kernel that can).
// `shortcuts`: the launch's arguments carry both `lazy_root` and `fuse_exit` (a tally launch, nobody observing exits).
struct Variant { int family; bool record; Tab tab; int seenw; bool emit, mesh, grid, even, align, path, park, solo; };
Variant choose_variant(const PvtScene* s, const LdsPlan& lp, bool record, bool emit, bool carry_out = false, bool shortcuts = false) {
    Variant v{};
    v.record = record; v.emit = emit; v.tab = lp.tab;
    v.seenw = s->n_rec <= 64 ? 1 : 4;
    v.mesh = s->d_bvh != nullptr;
    v.grid = lp.tab == Tab::Lds && s->lay.grid_d >= 0 && !v.mesh;   // many nodes: per-lane walk of the node grid
    // a rough node, a concentration field, a volume map, a captured recorder, an absorbing coating or a histogram of a
    // photon event counter or of the launch origin, a truncated cone, a polyhedron, a conicoid, an aligned component or a scattering coating: the extension family, split as
    // the plain ones
    const bool extension = s->has_frustum || s->has_polyhedron || s->has_conicoid || s->rough_d >= 0 || s->d_fd || s->d_md || s->d_cd || s->cabs_d >= 0 || s->counting() || s->origin_mask || s->pd_d >= 0 || s->al_d >= 0 || s->clobe_i >= 0;
    const bool lean = lp.tab == Tab::Lds && s->lean_ok && v.seenw == 1;   // plain scenes (prove_lean)
    v.align = s->al_d >= 0;   // (the extension family's kernels that hold the aligned components' code)
    v.path = s->path_maps;    // (... and those that hold the path-length maps' walk on top of it)
    v.family = extension ? PVT_VARIANT_ROUGH : v.mesh ? PVT_VARIANT_MESH : v.grid ? PVT_VARIANT_GRID : lean ? PVT_VARIANT_LEAN : PVT_VARIANT_W4;
    v.even = v.family == PVT_VARIANT_LEAN && s->lean_even;
    v.park = v.family == PVT_VARIANT_LEAN && !record && carry_out;   // (the entries compiled without the drain and the tail)
    v.solo = v.family == PVT_VARIANT_LEAN && !record && s->solo && shortcuts;   // (one box in a lazy root: the closed-form node stage)
    return v;
}

// A run-time value as a template argument: f is called with it as a std::integral_constant.
using Kernel = void (*)(KArgs);
template <class F> Kernel with_bool(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> Kernel with_tab(Tab t, F f) {
    return t == Tab::Lds ? f(std::integral_constant<int, 1>{}) : t == Tab::Heads ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 0>{});
}

#ifndef PVT_DEV_VARIANTS
#define PVT_DEV_VARIANTS 0   // developer builds (fast compile): 1 the plain-scene kernels, 2 the mesh kernels, of `narrow` launches only
#endif
// The entry point of a variant, null where this build has none.  A new family is a new case here (and in choose_variant).
Kernel kernel_of(const Variant& v) {
    return with_bool(v.record, [&](auto record) { return with_bool(v.emit, [&](auto emit) { return with_bool(v.seenw == 4, [&](auto wide) {
    return with_tab(v.tab, [&](auto tab) -> Kernel {
        constexpr bool R = decltype(record)::value, E = decltype(emit)::value;
        constexpr int W = decltype(wide)::value ? 4 : 1, T = decltype(tab)::value, dev = PVT_DEV_VARIANTS;
        constexpr bool narrow = T == 1 && W == 1 && !E;   // tables in LDS, <= 64 recorders, given rays
        constexpr bool has_rough = dev == 0;
        constexpr bool has_mesh = T != 2 && (dev == 0 || (dev == 2 && narrow));   // (mesh scenes stage all their tables or none)
        constexpr bool has_grid = T == 1 && (dev == 0 || (dev == 1 && narrow));
        constexpr bool has_lean = T == 1 && W == 1 && (dev == 0 || (dev == 1 && narrow && !R));
        constexpr bool has_w4 = dev == 0 || (dev == 1 && narrow);
        switch (v.family) {
        case PVT_VARIANT_ROUGH:
            if constexpr (has_rough) {
                if (v.path) {   // (the family's kernels compiled with the path-length maps' walk, the aligned components' code included)
                    if constexpr (T == 1) if (v.grid) return trace_kernel_rough_grid<R, W, E, kExtPath>;
                    if constexpr (T != 2) if (v.mesh) return trace_kernel_rough<R, T, W, E, true, kExtPath>;
                    if (!v.mesh) return trace_kernel_rough_w4<R, T, W, E, kExtPath>;
                    break;
                }
                if (v.align) {   // (the family's kernels compiled with the aligned components' code)
                    if constexpr (T == 1) if (v.grid) return trace_kernel_rough_grid<R, W, E, kExtAligned>;
                    if constexpr (T != 2) if (v.mesh) return trace_kernel_rough<R, T, W, E, true, kExtAligned>;
                    if (!v.mesh) return trace_kernel_rough_w4<R, T, W, E, kExtAligned>;
                    break;
                }
                if constexpr (T == 1) if (v.grid) return trace_kernel_rough_grid<R, W, E>;
                if constexpr (T != 2) if (v.mesh) return trace_kernel_rough<R, T, W, E, true>;
                if (!v.mesh) return trace_kernel_rough_w4<R, T, W, E>;
            }
            break;
        case PVT_VARIANT_MESH:
            if constexpr (has_mesh) return trace_kernel<R, T, W, E, true>;
            break;
        case PVT_VARIANT_GRID:
            if constexpr (has_grid) return trace_kernel_grid<R, W, E>;
            break;
        case PVT_VARIANT_LEAN:
            if constexpr (has_lean && !R) if (v.solo) {
                if (v.park) { if (v.even) return trace_kernel_solo_park<E, true>; return trace_kernel_solo_park<E, false>; }
                if (v.even) return trace_kernel_solo_fin<E, true>;
                return trace_kernel_solo_fin<E, false>;
            }
            if constexpr (has_lean && !R) if (v.park) { if (v.even) return trace_kernel_lean_park<E, true>; return trace_kernel_lean_park<E, false>; }
            if constexpr (has_lean) { if (v.even) return trace_kernel_lean_w4<R, E, true>; return trace_kernel_lean_w4<R, E, false>; }
            break;
        case PVT_VARIANT_W4:
            if constexpr (has_w4) return trace_kernel_w4<R, T, W, E>;
            break;
        }
        return nullptr;
    }); }); }); });
}

// Photons parked by the previous launch on the stream wait for this one: it must be able to finish them, by their rules.
int check_carried(const PvtScene::Carry& carry, const PvtTraceParams* p) {
    if (p->record_every > 0 || p->tally_bundle > 0)
        return fail(PVT_ERR_INVALID, "photons parked by the previous launch on this stream (PVT_FLAG_CARRY_OUT) are waiting: "
                                     "finish them with a plain tally launch (n_rays may be 0) first");
    if (p->maxsteps != carry.maxsteps || p->emit_method != carry.emit_method)
        return fail(PVT_ERR_INVALID, "photons parked by the previous launch on this stream were traced with maxsteps " +
                                     std::to_string(carry.maxsteps) + ", emit_method " + std::to_string(carry.emit_method) +
                                     "; this launch asks for " + std::to_string(p->maxsteps) + ", " + std::to_string(p->emit_method) +
                                     ": finish them under their own rules first (a launch with n_rays = 0 and the old values), or drop "
                                     "them with pvt_scene_carry_discard");
    return PVT_OK;
}

// The tally sets a launch asks for (0: none), PVT_OK if they are well formed.
int check_tally_sets(const PvtScene* s, const PvtTraceParams* p, long long* n_sets) {
    *n_sets = 0;
    if (p->tally_bundle <= 0) return PVT_OK;
    *n_sets = (p->n_rays + p->tally_bundle - 1) / p->tally_bundle;
    if (p->tally_bundle > 0x7fffffffLL || *n_sets > kMaxSets) return fail(PVT_ERR_INVALID, "at most 1024 tally sets per launch");
    if (p->tally_stride_i64 < 0 || p->tally_stride_f64 < 0) return fail(PVT_ERR_INVALID, "negative tally stride");
    if (s->map_slots > 0 && *n_sets > 1 && p->tally_stride_i64 < (long long)s->total_bins + s->map_slots)
        return fail(PVT_ERR_INVALID, "tally stride shorter than the bins and the volume maps' slots of a set");
    return PVT_OK;
}

// Workgroups of the persistent grid: enough to fill every CU a few times over, never more than the rays can feed.
// With tally sets (which it binds in `a`) a workgroup serves one set: the same total, split evenly over the sets.
long long size_grid(const PvtScene* s, const PvtTraceParams* p, long long carried, long long n_sets, KArgs& a) {
    long long blocks_for_rays = (p->n_rays + carried + kBlock - 1) / kBlock;
    double per_cu = p->workgroups_per_cu > 0 ? (double)p->workgroups_per_cu : 4.0;
    long long grid = (long long)((double)s->num_cu * per_cu);
    if (grid > blocks_for_rays) grid = blocks_for_rays;
    if (grid < 1) grid = 1;
    // Every wave resumes the slice of the parked photons that its index names (64 per wave, the kernel's refill); the
    // launch that parked them put at most 64 per wave of ITS grid: this launch must not be narrower, or slices beyond
    // its last wave would depend on the claim cursor being asked often enough (workgroups_per_cu 4, then 1)
    if (grid * kBlock < carried) grid = (carried + kBlock - 1) / kBlock;
    if (n_sets) {
        long long per_set = grid / n_sets;
        const long long for_rays = (p->tally_bundle + kBlock - 1) / kBlock;
        if (per_set > for_rays) per_set = for_rays;
        if (per_set < 1) per_set = 1;
        grid = per_set * n_sets;
        a.set_size = (unsigned int)p->tally_bundle;
        a.wgs_per_set = (int)per_set;
        a.set_stride_i = p->tally_stride_i64;
        a.set_stride_d = p->tally_stride_f64;
    }
    return grid;
}

// Carried photons: the stream's two buffers (allocated at first use) -- this launch resumes from one and parks into
// the other -- and where its predecessor counted what it parked.  Clears `carry_out` for a launch too wide to park.
int bind_carry(PvtScene* s, PvtScene::Carry& carry, unsigned int* blocks, long long grid, bool carry_in, bool* carry_out, KArgs& a) {
    if (!s->carry_cap) s->carry_cap = (unsigned int)((long long)s->num_cu * 4 * kBlock);
    if (grid * kBlock > (long long)s->carry_cap) *carry_out = false;   // an unusually wide launch finishes its own photons
    const size_t bytes = (size_t)s->carry_cap * carry_words(s->counting(), s->origin_mask != 0) * 8;
    for (int q = 0; q < 2; q++)
        if (!carry.buf[q]) HIP_TRY(hipMalloc(&carry.buf[q], bytes));
    a.carry_cap = s->carry_cap;
    a.carry_in = carry.buf[carry.parity ^ 1];
    a.carry_out = carry.buf[carry.parity];
    a.carry_in_count = blocks + 4 * ((carry.phase + 2) % 3) + 2;
    a.carry_flags = (carry_in ? 1 : 0) | (*carry_out ? 2 : 0);
    return PVT_OK;
}

// Device emission: the stream's pool of [7][64] doubles per wave of the launch, grown to the widest grid seen.
int grow_emit_pool(PvtScene* s, size_t slot, long long grid, hipStream_t st, KArgs& a) {
    const size_t need = (size_t)grid * kWaves * 7 * 64 * sizeof(double);
    if (s->emit_pool_bytes[slot] < need) {
        // (growth is rare -- the grid of a stream's launches is stable -- and the launch before this one on the stream may
        // still be reading the old buffer)
        if (s->emit_pool[slot]) { HIP_TRY(hipStreamSynchronize(st)); (void)hipFree(s->emit_pool[slot]); s->emit_pool[slot] = nullptr; s->emit_pool_bytes[slot] = 0; }
        const size_t usual = (size_t)s->num_cu * 4 * kWaves * 7 * 64 * sizeof(double);
        const size_t bytes = need < usual ? usual : need;
        HIP_TRY(hipMalloc(&s->emit_pool[slot], bytes));
        s->emit_pool_bytes[slot] = bytes;
    }
    a.emit_pool = s->emit_pool[slot];
    return PVT_OK;
}

// Launch origin: the stream's side store of [grid x kBlock][kOriginWords] doubles, grown to the widest grid seen.  The kernel
// indexes it by the launch's own grid, so any buffer at least that large serves.
int grow_origin_store(PvtScene* s, size_t slot, long long grid, hipStream_t st, KArgs& a) {
    const size_t need = (size_t)grid * kBlock * kOriginWords * sizeof(double);
    if (s->origin_store_bytes[slot] < need) {   // (rare, and the launch before this one on the stream may still use the old buffer)
        if (s->origin_store[slot]) { HIP_TRY(hipStreamSynchronize(st)); (void)hipFree(s->origin_store[slot]); s->origin_store[slot] = nullptr; s->origin_store_bytes[slot] = 0; }
        const size_t usual = (size_t)s->num_cu * 4 * kBlock * kOriginWords * sizeof(double);
        const size_t bytes = need < usual ? usual : need;
        HIP_TRY(hipMalloc(&s->origin_store[slot], bytes));
        s->origin_store_bytes[slot] = bytes;
    }
    a.origin_store = s->origin_store[slot];
    return PVT_OK;
}

#if PVT_STATS
// developer build: waits for the launch and prints its counters (KArgs::cursor points at them)
void dump_stats(const KArgs& a, hipStream_t st) {
    unsigned long long c[32];
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(c, a.cursor, 256, hipMemcpyDeviceToHost);
    fprintf(stderr, "[pvt stats] waves %llu  wave-iterations %llu (drain %llu)  lane-steps %llu (drain %llu)  "
            "mean live lanes/iter %.1f (bulk %.1f, drain %.1f)  iters/wave %.1f (drain %.1f)\n",
            c[5], c[1], c[3], c[2], c[4], (double)c[2] / c[1], (double)(c[2] - c[4]) / (double)(c[1] - c[3] + 1e-9),
            (double)c[4] / (c[3] + 1e-9), (double)c[1] / c[5], (double)c[3] / c[5]);
    fprintf(stderr, "[pvt stats] solo-wave cycles: refill %llu nodes %llu absorb %llu frame %llu trig %llu surface %llu tally %llu (solo waves %llu)\n",
            c[9], c[10], c[11], c[12], c[13], c[14], c[15], c[16]);
    const double bi = (double)(c[1] - c[3]) + 1e-9;
    if (a.lay.grid_d >= 0)
        fprintf(stderr, "[pvt stats] grid walk per wave-iteration: cell rounds %.2f  node-test trips %.2f  (lanes per trip %.1f, lanes per cell round %.1f)\n",
                (double)c[25] / c[1], (double)c[26] / c[1], (double)c[27] / (c[26] + 1e-9), (double)c[28] / (c[25] + 1e-9));
    if (a.bvh)
        fprintf(stderr, "[pvt stats] mesh walk per wave-iteration: box trips %.2f (lanes per trip %.1f)  triangle trips %.2f (lanes per trip %.1f);  per lane-step: boxes %.2f triangles %.2f\n",
                (double)c[25] / c[1], (double)c[26] / (c[25] + 1e-9), (double)c[27] / c[1], (double)c[28] / (c[27] + 1e-9),
                (double)c[26] / c[2], (double)c[28] / c[2]);
    fprintf(stderr, "[pvt stats] bulk lanes/iteration: live %.1f absorbed %.1f re-emitted %.1f surface %.1f exit %.1f terminal-selector %.1f terminal %.1f\n",
            c[17] / bi, c[18] / bi, c[19] / bi, c[20] / bi, c[21] / bi, c[22] / bi, c[23] / bi);
}
#endif

// Enqueue ONE trace kernel.  `log_rows` / `log_counts`: the event records of the recorded rays (device memory,
// null when record_every == 0); counts are cleared here.
int trace_launch(PvtScene* s, const PvtRays* rays, const PvtTraceParams* p, const PvtTallies* tl,
                 unsigned long long* log_rows, int* log_counts, hipStream_t st, const PvtCaptures* cap = nullptr) {
    const int slot = slot_of_stream(s, st);
    if (slot < 0) return PVT_ERR_INVALID;
    PvtScene::Carry& carry = s->carry[(size_t)slot];
    const bool carry_in = carry.pending;
    if (p->n_rays == 0 && !carry_in) return PVT_OK;
    int rc = carry_in ? check_carried(carry, p) : PVT_OK;
    if (rc != PVT_OK) return rc;
    long long n_sets = 0;
    if ((rc = check_tally_sets(s, p, &n_sets)) != PVT_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));

    KArgs a = base_args(s, p);
    a.stamp = s->d_stamp + 2 * (size_t)slot;
    if (rays) { a.pos = rays->position; a.dir = rays->direction; a.wl = rays->wavelength; }
    a.rec_distinct = reinterpret_cast<long long*>(tl->rec_distinct);
    a.rec_crossings = reinterpret_cast<long long*>(tl->rec_crossings);
    a.rec_sums = tl->rec_sums;
    a.rec_bins = reinterpret_cast<long long*>(tl->rec_bins);
    if (cap && s->d_cd) {   // (without them the launch keeps no rows; a scene without captures ignores them)
        if (!cap->rows || !cap->cursors) return fail(PVT_ERR_INVALID, "capture buffers missing");
        a.cap_rows = reinterpret_cast<unsigned long long*>(cap->rows);
        a.cap_cursor = reinterpret_cast<unsigned long long*>(cap->cursors);
    }
    const bool record = p->record_every > 0;
    // nobody looks at where a photon leaves the scene: the root's distance is only needed to ORDER crossings
    a.lazy_root = (!record && !s->exit_observed && !s->d_bvh) ? s->lazy_root : 0;
    a.lazy_tail = s->d_bvh ? 0 : s->lazy_root;
    a.fuse_exit = (a.lazy_root && s->fuse_exit) ? 1 : 0;
    a.lazy_k = s->lazy_k;
    if (record) {
        if (!log_rows || !log_counts) return fail(PVT_ERR_INVALID, "record_every > 0 needs an event log");
        a.log_rows = log_rows;
        a.log_counts = log_counts;
        const size_t nrec = (size_t)((p->n_rays + p->record_every - 1) / p->record_every);
        HIP_TRY(hipMemsetAsync(log_counts, 0, nrec * 4, st));
    }
    // the cursor belongs to the stream: two launches can only overlap on different streams.  A slot holds THREE
    // blocks {ray cursor, claim cursor of the resumed photons, count of the photons parked} used in rotation:
    // launch L counts in block L mod 3, reads how many photons its predecessor parked from block L-1, and clears
    // block L+1 for its successor (all zero at scene creation) -- so no fill kernel sits between two launches
    unsigned int* const blocks = s->d_cursor + 16 * slot;
    if (n_sets) {
        a.cursor = s->d_set_cursor + (size_t)kMaxSets * slot;
        HIP_TRY(hipMemsetAsync(a.cursor, 0, (size_t)n_sets * 4, st));
    } else {
        a.cursor = blocks + 4 * carry.phase;
        a.cursor_next = blocks + 4 * ((carry.phase + 1) % 3);
    }
#if PVT_STATS
    static unsigned long long* g_stats = nullptr;
    if (!g_stats) (void)hipMalloc(&g_stats, 256);
    (void)hipMemsetAsync(g_stats, 0, 256, st);
    a.cursor = reinterpret_cast<unsigned int*>(g_stats);  // dev build: counters live in their own buffer
    a.cursor_next = nullptr;
#endif

    const LdsPlan lp = plan_lds(s, record);
    if (!lp.ok) return fail(PVT_ERR_INVALID, "recorder accumulators exceed LDS");
    a.tq_pos = lp.tq_pos;
    a.bins_in_lds = lp.bins_in_lds;
    a.xslots = lp.xslots;
    if (lp.tab == Tab::Heads) { a.nd_lds = s->nd_small; a.ni_lds = s->ni_small; }
    a.meshq_off = lp.meshq_off;
    a.top_off = lp.top_off; a.top_n = s->top_n; a.bvh_top = s->d_bvh_top;
    if (a.bvh && lp.total > s->lds_limit) return fail(PVT_ERR_INVALID, "mesh staging exceeds LDS");

    const long long grid = size_grid(s, p, carry_in ? carry.bound : 0, n_sets, a);
    s->last_grid = (int)grid;
    s->last_lds = (int)lp.total;
    bool carry_out = (p->flags & PVT_FLAG_CARRY_OUT) != 0 && !record && !n_sets;
    if ((carry_in || carry_out) && (rc = bind_carry(s, carry, blocks, grid, carry_in, &carry_out, a)) != PVT_OK) return rc;

#if PVT_TIMELINE
    // developer build: the first kTlLaunches launches after PVT_TIMELINE_FROM each get a region of the stamp buffer;
    // nothing is synchronised (launches overlap as usual); pvt_timeline_dump() writes the file
    if (getenv("PVT_TIMELINE_FILE")) {
        if (!g_timeline) { (void)hipMalloc(&g_timeline, kTlBytes); (void)hipMemset(g_timeline, 0, kTlBytes); }
        const int from = getenv("PVT_TIMELINE_FROM") ? atoi(getenv("PVT_TIMELINE_FROM")) : 0;
        const int k = g_tl_launch++ - from;
        if (k >= 0 && k < kTlLaunches && grid <= kTlWgs) {
            a.timeline = g_timeline + (size_t)k * kTlWgs * kWaves * 8;
            g_tl_grid[k] = (int)grid; g_tl_n[k] = p->n_rays;
        }
    }
#endif
    const bool emit = rays == nullptr && s->d_ed != nullptr;
    if (emit && (rc = grow_emit_pool(s, (size_t)slot, grid, st, a)) != PVT_OK) return rc;
    if (s->origin_mask && (rc = grow_origin_store(s, (size_t)slot, grid, st, a)) != PVT_OK) return rc;
    const Variant v = choose_variant(s, lp, record, emit, carry_out, a.lazy_root != 0 && a.fuse_exit != 0);
    s->last_variant = v.family;
    s->last_solo = v.solo;
    s->last_park = v.park;
    hipError_t e = hipErrorNotSupported;
    if (const Kernel kernel = kernel_of(v)) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kBlock), lp.total, st, a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(PVT_ERR_HIP, std::string("trace_kernel launch: ") + hipGetErrorString(e));
    if (!n_sets) carry.phase = (carry.phase + 1) % 3;
    if (carry_in || carry_out) {
        carry.pending = carry_out;
        carry.bound = carry_out ? grid * kBlock : 0;
        carry.maxsteps = p->maxsteps;
        carry.emit_method = p->emit_method;
        carry.parity ^= 1;
    }
#if PVT_STATS
    dump_stats(a, st);
#endif
    return PVT_OK;
}

#if PVT_TIMELINE
void timeline_dump() {
    const char* path = getenv("PVT_TIMELINE_FILE");
    if (!path || !g_timeline) return;
    (void)hipDeviceSynchronize();
    std::vector<unsigned long long> host(kTlBytes / 8);
    (void)hipMemcpy(host.data(), g_timeline, kTlBytes, hipMemcpyDeviceToHost);
    if (FILE* fp = fopen(path, "wb")) {
        for (int k = 0; k < kTlLaunches; k++) {
            if (!g_tl_grid[k]) continue;
            unsigned long long head[4] = {0xABCDull, (unsigned long long)k, (unsigned long long)g_tl_grid[k], (unsigned long long)g_tl_n[k]};
            fwrite(head, 8, 4, fp);
            fwrite(host.data() + (size_t)k * kTlWgs * kWaves * 8, 8, (size_t)g_tl_grid[k] * kWaves * 8, fp);
        }
        fclose(fp);
    }
}
#endif

int unpack_launch(const unsigned long long* rows, const int* counts, long long n_recorded, int max_events,
                  const PvtEventLog* out, bool prefill, hipStream_t st) {
    if (n_recorded <= 0) return PVT_OK;
    const int rays_per_block = max_events >= kBlock ? 1 : kBlock / max_events;
    const long long gx = (n_recorded + rays_per_block - 1) / rays_per_block;
    const int gy = rays_per_block > 1 ? 1 : (max_events + kBlock - 1) / kBlock;
    if (gx > 0x7fffffffLL) return fail(PVT_ERR_INVALID, "too many recorded rays for one unpack launch");
    hipLaunchKernelGGL(unpack_log_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kBlock), 0, st, rows, counts, *out,
                       n_recorded, max_events, rays_per_block, prefill ? 1 : 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(PVT_ERR_HIP, std::string("unpack_log_kernel launch: ") + hipGetErrorString(e));
    return PVT_OK;
}

// What every pvt_scene_create* entry does with the record of its inputs (SceneInputs and the levels an entry can know:
// pvt_scene_pack.h).
int create_scene(const SceneInputs& in, int device, PvtScene** out);

}  // namespace

extern "C" {

int pvt_scene_create(const PvtSceneTables* t, int device, PvtScene** out) {
    return create_scene({t, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kKnowsBeforeAbsorb}, device, out);
}

int pvt_scene_create_ex(const PvtSceneTables* t, const PvtIndexTables* x, int device, PvtScene** out) {
    return create_scene({t, x, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kKnowsBeforeAbsorb}, device, out);
}

int pvt_scene_create_phase(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph, int device, PvtScene** out) {
    return create_scene({t, x, ph, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kKnowsBeforeAbsorb}, device, out);
}

int pvt_scene_create_rough(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph,
                           const PvtSurfaceTables* rs, int device, PvtScene** out) {
    return create_scene({t, x, ph, rs, nullptr, nullptr, nullptr, nullptr, nullptr, kKnowsBeforeAbsorb}, device, out);
}

int pvt_scene_create_field(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph,
                           const PvtSurfaceTables* rs, const PvtFieldTables* fr, int device, PvtScene** out) {
    return create_scene({t, x, ph, rs, fr, nullptr, nullptr, nullptr, nullptr, kKnowsBeforeAbsorb}, device, out);
}

int64_t pvt_scene_map_slots(const PvtScene* s) { return s ? (int64_t)s->map_slots : 0; }

int pvt_scene_create_maps(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph,
                          const PvtSurfaceTables* rs, const PvtFieldTables* fr, const PvtMapTables* mp, int device,
                          PvtScene** out) {
    return create_scene({t, x, ph, rs, fr, mp, nullptr, nullptr, nullptr, kKnowsBeforeAbsorb}, device, out);
}

int64_t pvt_scene_capture_rows(const PvtScene* s) { return s ? (int64_t)s->capture_rows : 0; }

int pvt_scene_create_capture(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph,
                             const PvtSurfaceTables* rs, const PvtFieldTables* fr, const PvtMapTables* mp,
                             const PvtCaptureTables* cp, int device, PvtScene** out) {
    return create_scene({t, x, ph, rs, fr, mp, cp, nullptr, nullptr, kKnowsBeforeAbsorb}, device, out);
}

int pvt_scene_create_absorb(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph,
                            const PvtSurfaceTables* rs, const PvtFieldTables* fr, const PvtMapTables* mp,
                            const PvtCaptureTables* cp, const PvtCoatingAbsorbTables* ab, int device, PvtScene** out) {
    return create_scene({t, x, ph, rs, fr, mp, cp, ab, nullptr, kKnowsAbsorb}, device, out);
}

int pvt_scene_create_origin(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph,
                            const PvtSurfaceTables* rs, const PvtFieldTables* fr, const PvtMapTables* mp,
                            const PvtCaptureTables* cp, const PvtCoatingAbsorbTables* ab, int device, PvtScene** out) {
    return create_scene({t, x, ph, rs, fr, mp, cp, ab, nullptr, kKnowsOrigin}, device, out);
}

int pvt_scene_create_pattern(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph,
                             const PvtSurfaceTables* rs, const PvtFieldTables* fr, const PvtMapTables* mp,
                             const PvtCaptureTables* cp, const PvtCoatingAbsorbTables* ab, const PvtCoatingPatternTables* pt,
                             int device, PvtScene** out) {
    return create_scene({t, x, ph, rs, fr, mp, cp, ab, pt, kKnowsOrigin}, device, out);
}

int pvt_scene_create_aligned(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph,
                             const PvtSurfaceTables* rs, const PvtFieldTables* fr, const PvtMapTables* mp,
                             const PvtCaptureTables* cp, const PvtCoatingAbsorbTables* ab, const PvtCoatingPatternTables* pt,
                             const PvtAlignTables* al, int device, PvtScene** out) {
    return create_scene({t, x, ph, rs, fr, mp, cp, ab, pt, kKnowsOrigin, al}, device, out);
}

int pvt_scene_create_polyhedra(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph,
                               const PvtSurfaceTables* rs, const PvtFieldTables* fr, const PvtMapTables* mp,
                               const PvtCaptureTables* cp, const PvtCoatingAbsorbTables* ab, const PvtCoatingPatternTables* pt,
                               const PvtAlignTables* al, const PvtPolyhedronTables* pl, int device, PvtScene** out) {
    return create_scene({t, x, ph, rs, fr, mp, cp, ab, pt, kKnowsPolyhedra, al, pl}, device, out);
}

}  // extern "C"

namespace {

int create_scene(const SceneInputs& in, int device, PvtScene** out) {
    const PvtSceneTables* t = in.t;
    if (!t || !out) return fail(PVT_ERR_INVALID, "null argument");
    if (t->n_nodes <= 0) return fail(PVT_ERR_INVALID, "scene has no nodes");
    if (t->n_nodes > PVT_MAX_NODES) return fail(PVT_ERR_TOO_MANY_NODES, "more than 128 geometry nodes");
    if (t->n_recorders > PVT_MAX_RECORDERS) return fail(PVT_ERR_INVALID, "more than 256 recorders");
    if (pvt_device_count() <= device) return fail(PVT_ERR_NO_DEVICE, "no such HIP device");
    HIP_TRY(hipSetDevice(device));
    PackedScene packed;
    int rc = pack_scene(in, &packed);
    if (rc != PVT_OK) return rc;
    rc = pack_patterns(in, &packed);   // (validated before anything is uploaded)
    if (rc != PVT_OK) return rc;
    rc = pack_align(in, &packed);      // (likewise)
    if (rc != PVT_OK) return rc;

    // owned until every upload has succeeded: a failing HIP call must not leak the scene
    struct Owner {
        PvtScene* p;
        ~Owner() { if (p) pvt_scene_destroy(p); }
    } owner{new PvtScene()};
    PvtScene* s = owner.p;
    s->stage.reserve(kCursorSlots); s->stage_bytes.reserve(kCursorSlots); s->carry.reserve(kCursorSlots);   // (references stay valid)
    s->emit_pool.reserve(kCursorSlots); s->emit_pool_bytes.reserve(kCursorSlots);
    s->origin_store.reserve(kCursorSlots); s->origin_store_bytes.reserve(kCursorSlots);
    s->device = device;
    s->lay = packed.lay;
    s->nd = (int)packed.gd.size(); s->ni = (int)packed.gi.size();
    s->nd_small = packed.nd_small; s->ni_small = packed.ni_small;
    s->n_nodes = t->n_nodes; s->root = t->root_id; s->n_rec = t->n_recorders;
    s->total_bins = t->total_bins; s->n_coat = t->n_coatings; s->n_ctab = packed.n_ctab; s->n_rtab = packed.n_rtab;
    s->rough_d = packed.rough_d;
    s->has_frustum = packed.has_frustum;
    s->has_polyhedron = packed.has_polyhedron;
    s->has_conicoid = packed.has_conicoid;
    s->cabs_d = packed.cabs_d; s->dcand_i = packed.dcand_i;
    s->clobe_i = packed.clobe_i;
    s->lazy_root = packed.lazy_root; s->lazy_k = packed.lazy_k;
    s->exit_observed = packed.exit_observed; s->fuse_exit = packed.fuse_exit; s->hist_reads_position = packed.hist_reads_position;
    s->hist_reads_counter = packed.hist_reads_counter;
    s->origin_mask = packed.origin_mask;
    s->grid = packed.grid;
    s->lean_ok = packed.lean_ok && !getenv("PVT_NO_LEAN");   // (PVT_NO_LEAN: the generic family, for parity tests and A/B runs)
    s->lean_even = s->lean_ok && packed.lean_even;
    s->solo = s->lean_ok && packed.solo && !getenv("PVT_NO_SOLO");   // (PVT_NO_SOLO: the lean family's own entries, for parity tests and A/B runs)
    for (int a = 0; a < 3; a++) s->grid_dims[a] = packed.grid_dims[a];
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    s->num_cu = prop.multiProcessorCount;
    s->lds_limit = prop.sharedMemPerBlock;
    if (const char* env = getenv("PVT_STAGE_BYTES")) s->stage_limit = (size_t)atoll(env);   // (tests: force several launches)
    // (the coating patterns' buffer, when there is one, lies behind the blob in the same allocation: beyond `nd`, never staged)
    HIP_TRY(hipMalloc(&s->d_gd, (packed.gd.size() + packed.pd.size()) * sizeof(double) + packed.pmask.size()));
    HIP_TRY(hipMalloc(&s->d_gi, packed.gi.size() * sizeof(int)));
    HIP_TRY(hipMalloc(&s->d_cursor, 64 * kCursorSlots + 256));   // + room for the PVT_STATS counters
    HIP_TRY(hipMemset(s->d_cursor, 0, 64 * kCursorSlots + 256));
    HIP_TRY(hipMalloc(&s->d_set_cursor, (size_t)kCursorSlots * kMaxSets * 4));
    HIP_TRY(hipMalloc(&s->d_counters, 64 * 8 * 8));
    HIP_TRY(hipMemset(s->d_counters, 0, 64 * 8 * 8));
    HIP_TRY(hipMalloc(&s->d_stamp, (size_t)kCursorSlots * 2 * 8));
    HIP_TRY(hipMemset(s->d_stamp, 0, (size_t)kCursorSlots * 2 * 8));
    if (!packed.bvh_nodes.empty()) {
        // a lane of a walk notes kMeshQ leaves before their triangles are tested -- one, in trees of a handful of records
        // (the kernel applies the same rule per tree)
        s->meshq = 1;
        for (int r : packed.bvh_roots)
            if (packed.bvh_nodes[r].skip - r > 16) s->meshq = kMeshQ;   // (15 records and the unused one after the root)
        // The top levels of the trees go to LDS (pvt_bvh.h: stage_top), as many records as leave four workgroups per CU
        // -- the mesh variants' four waves per SIMD -- their LDS in either kind of launch (tallies / histories).
        const LdsPlan tally = plan_lds(s, false), hist = plan_lds(s, true);
        const size_t other = (tally.bytes > hist.bytes ? tally.bytes : hist.bytes) + (size_t)s->meshq * kBlock * 4;
        const size_t per_wg = (size_t)39 * 1024 * 4 / kMeshWaves;
        size_t room = tally.ok && hist.ok && other < per_wg ? per_wg - other : 0;
        if (room > 32 * 1024) room = 32 * 1024;
        if (const char* env = getenv("PVT_MESH_TOP_BYTES")) {   // (developer override, never past the room computed above; 0: no copy)
            const size_t asked = (size_t)atoll(env);
            room = asked < room ? asked : room;
        }
        std::vector<pvt::BvhNode> top;
        pvt::stage_top(packed.bvh_nodes, packed.bvh_roots, room / sizeof(pvt::BvhNode), top);
        s->top_n = (int)top.size();
        // what was planned without the copy must still hold with it (plan_lds reserves the copy first): same table
        // placement, everything inside the LDS of a workgroup
        const LdsPlan tally2 = plan_lds(s, false), hist2 = plan_lds(s, true);
        if (tally2.ok != tally.ok || hist2.ok != hist.ok || tally2.tab != tally.tab || hist2.tab != hist.tab ||
            tally2.total > s->lds_limit || hist2.total > s->lds_limit)
            return fail(PVT_ERR_INVALID, "internal: the LDS plan of a mesh scene changed when the copy of its trees' top levels was added");
        if (s->top_n > 0) {
            HIP_TRY(hipMalloc(&s->d_bvh_top, top.size() * sizeof(pvt::BvhNode)));
            HIP_TRY(hipMemcpy(s->d_bvh_top, top.data(), top.size() * sizeof(pvt::BvhNode), hipMemcpyHostToDevice));
        }
        packed.bvh_nodes.push_back(pvt::BvhNode{});   // (one record past the end, kept for walks that fetch ahead)
        HIP_TRY(hipMalloc(&s->d_bvh, packed.bvh_nodes.size() * sizeof(pvt::BvhNode)));
        HIP_TRY(hipMalloc(&s->d_tris, packed.bvh_tris.size() * sizeof(pvt::MeshTri)));
        HIP_TRY(hipMemcpy(s->d_bvh, packed.bvh_nodes.data(), packed.bvh_nodes.size() * sizeof(pvt::BvhNode), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->d_tris, packed.bvh_tris.data(), packed.bvh_tris.size() * sizeof(pvt::MeshTri), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(s->d_gd, packed.gd.data(), packed.gd.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_gi, packed.gi.data(), packed.gi.size() * sizeof(int), hipMemcpyHostToDevice));
    if (!packed.fd.empty()) {   // (global memory only: no launch stages it in LDS)
        HIP_TRY(hipMalloc(&s->d_fd, packed.fd.size() * sizeof(double)));
        HIP_TRY(hipMemcpy(s->d_fd, packed.fd.data(), packed.fd.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (!packed.md.empty()) {   // (global memory only, like the fields)
        HIP_TRY(hipMalloc(&s->d_md, packed.md.size() * sizeof(double)));
        HIP_TRY(hipMemcpy(s->d_md, packed.md.data(), packed.md.size() * sizeof(double), hipMemcpyHostToDevice));
        s->map_slots = packed.map_slots;
        s->path_maps = packed.path_maps;
    }
    if (!packed.pd.empty()) {   // (global memory only: flags and records, the masks right behind them)
        const size_t head = packed.pd.size() * sizeof(double);
        double* d_pd = s->d_gd + packed.gd.size();
        HIP_TRY(hipMemcpy(d_pd, packed.pd.data(), head, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(reinterpret_cast<unsigned char*>(d_pd) + head, packed.pmask.data(), packed.pmask.size(), hipMemcpyHostToDevice));
        s->pd_d = (int)packed.gd.size();
    }
    if (packed.aligned) s->al_d = 0;   // (their records were placed in packed.fd, uploaded above)
    if (!packed.cd.empty()) {
        HIP_TRY(hipMalloc(&s->d_cd, packed.cd.size() * sizeof(long long)));
        HIP_TRY(hipMemcpy(s->d_cd, packed.cd.data(), packed.cd.size() * sizeof(long long), hipMemcpyHostToDevice));
        s->capture_rows = packed.capture_rows;
    }
    owner.p = nullptr;
    *out = s;
    return PVT_OK;
}

}  // namespace

extern "C" {

int pvt_trace_device_records(PvtScene* s, const PvtRays* rays, const PvtTraceParams* p, const PvtTallies* tl,
                             const PvtEventRecords* rec, void* stream) {
    return pvt_trace_device_capture(s, rays, p, tl, rec, nullptr, stream);
}

int pvt_trace_device_capture(PvtScene* s, const PvtRays* rays, const PvtTraceParams* p, const PvtTallies* tl,
                             const PvtEventRecords* rec, const PvtCaptures* cap, void* stream) {
    int rc = check_trace_args(s, rays, p, tl);
    if (rc != PVT_OK) return rc;
    if (p->record_every > 0 && (!rec || !rec->rows || !rec->counts))
        return fail(PVT_ERR_INVALID, "record_every > 0 needs event records");
    return trace_launch(s, rays, p, tl, rec ? reinterpret_cast<unsigned long long*>(rec->rows) : nullptr, rec ? rec->counts : nullptr,
                        reinterpret_cast<hipStream_t>(stream), cap);
}

int pvt_scene_carry_pending(PvtScene* s, void* stream) {
    if (!s) return 0;
    std::lock_guard<std::mutex> lock(s->slot_mutex);
    for (size_t k = 0; k < s->slot_of.size(); k++)
        if (s->slot_of[k] == reinterpret_cast<hipStream_t>(stream)) return s->carry[k].pending ? 1 : 0;
    return 0;
}

int pvt_scene_carry_discard(PvtScene* s, void* stream) {
    if (!s) return fail(PVT_ERR_INVALID, "null scene");
    std::lock_guard<std::mutex> lock(s->slot_mutex);
    for (size_t k = 0; k < s->slot_of.size(); k++)
        if (s->slot_of[k] == reinterpret_cast<hipStream_t>(stream)) {
            // the parked photons are simply forgotten: the next launch on the stream starts from its own rays (the cursor
            // blocks keep rotating; the count the abandoned launch left behind is never read)
            s->carry[k].pending = false;
            s->carry[k].bound = 0;
        }
    return PVT_OK;
}

int pvt_scene_trim(PvtScene* s) {
    if (!s) return fail(PVT_ERR_INVALID, "null scene");
    std::lock_guard<std::mutex> lock(s->slot_mutex);
    bool any = false;
    for (auto* b : s->stage) any = any || b != nullptr;
    if (any) {
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipDeviceSynchronize());   // (an unpack pass may still read a staging buffer)
        for (size_t k = 0; k < s->stage.size(); k++)
            if (s->stage[k]) { (void)hipFree(s->stage[k]); s->stage[k] = nullptr; s->stage_bytes[k] = 0; }
    }
    for (auto& c : s->carry) { c.pending = false; c.bound = 0; }   // a scene put aside carries nobody's photons
    return PVT_OK;
}

int pvt_unpack_records_device(const PvtEventRecords* rec, int64_t n_recorded, int32_t max_events,
                              const PvtEventLog* out, int prefill, void* stream) {
    if (!rec || !out || !rec->rows || !rec->counts || n_recorded < 0 || max_events < 1)
        return fail(PVT_ERR_INVALID, "bad unpack arguments");
    return unpack_launch(reinterpret_cast<const unsigned long long*>(rec->rows), rec->counts, n_recorded, max_events, out, prefill != 0,
                         reinterpret_cast<hipStream_t>(stream));
}

// Column arrays on the device: the records are staged in a buffer of the scene (one per stream) and unpacked by
// a second kernel, which also writes the reference's fill values into the rows no event reached.  A log too
// large for the staging limit is traced in several launches over consecutive ray ranges (each a multiple of
// record_every, so the rows and RNG streams are those of the single launch).
int pvt_trace_device(PvtScene* s, const PvtRays* rays, const PvtTraceParams* p, const PvtTallies* tl,
                     const PvtEventLog* log, void* stream) {
    int rc = check_trace_args(s, rays, p, tl);
    if (rc != PVT_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (p->record_every <= 0) return trace_launch(s, rays, p, tl, nullptr, nullptr, st);
    if (!log) return fail(PVT_ERR_INVALID, "record_every > 0 needs an event log");
    if (p->n_rays == 0) return PVT_OK;
    HIP_TRY(hipSetDevice(s->device));
    const int slot = slot_of_stream(s, st);
    if (slot < 0) return PVT_ERR_INVALID;
    const long long every = p->record_every, me = p->max_events;
    const long long nrec = (p->n_rays + every - 1) / every;
    const size_t row_bytes = (size_t)kRecWords * 8;
    // recorded rays per launch under the staging limit
    long long per_launch = (long long)(s->stage_limit / (row_bytes * (size_t)me));
    if (per_launch < 1) per_launch = 1;
    if (per_launch > nrec) per_launch = nrec;
    const size_t need = (size_t)per_launch * (size_t)me * row_bytes;
    if (s->stage_bytes[slot] < need) {
        // (a stream-ordered free would do; growth is rare and the buffer may still be read by an unpack in flight)
        if (s->stage[slot]) { HIP_TRY(hipStreamSynchronize(st)); (void)hipFree(s->stage[slot]); s->stage[slot] = nullptr; s->stage_bytes[slot] = 0; }
        HIP_TRY(hipMalloc(&s->stage[slot], need));
        s->stage_bytes[slot] = need;
    }
    const bool prefill = !(p->flags & PVT_FLAG_NO_LOG_PREFILL);
    for (long long j0 = 0; j0 < nrec; j0 += per_launch) {
        const long long j1 = j0 + per_launch < nrec ? j0 + per_launch : nrec;
        const long long r0 = j0 * every, r1 = j1 * every < p->n_rays ? j1 * every : p->n_rays;
        PvtTraceParams q = *p;
        q.n_rays = r1 - r0;
        q.ray_offset = p->ray_offset + (uint64_t)r0;
        PvtRays sub{};
        if (rays) sub = PvtRays{rays->position + 3 * r0, rays->direction + 3 * r0, rays->wavelength + r0};
        rc = trace_launch(s, rays ? &sub : nullptr, &q, tl, s->stage[slot], log->counts + j0, st);
        if (rc != PVT_OK) return rc;
        const long long row0 = j0 * me;
        PvtEventLog out{log->counts + j0, log->kind + row0, log->hit + row0, log->container + row0, log->adjacent + row0,
                        log->component + row0, log->source + row0, log->position + 3 * row0, log->direction + 3 * row0,
                        log->normal + 3 * row0, log->wavelength + row0, log->travelled + row0, log->duration + row0};
        if (prefill) {
            // the fill values go down as plain memsets (full-width stores: measured 1.6 x the rate of filling from
            // the unpack kernel's per-row stores); the unpack pass then writes the rows that hold events
            const size_t rows = (size_t)(j1 - j0) * (size_t)me;
            HIP_TRY(hipMemsetAsync(out.kind, 0, rows, st));
            HIP_TRY(hipMemsetAsync(out.hit, 0xFF, rows * 4, st));
            HIP_TRY(hipMemsetAsync(out.container, 0xFF, rows * 4, st));
            HIP_TRY(hipMemsetAsync(out.adjacent, 0xFF, rows * 4, st));
            HIP_TRY(hipMemsetAsync(out.component, 0xFF, rows * 4, st));
            HIP_TRY(hipMemsetAsync(out.source, 0xFF, rows * 4, st));
            HIP_TRY(hipMemsetAsync(out.position, 0, rows * 24, st));
            HIP_TRY(hipMemsetAsync(out.direction, 0, rows * 24, st));
            HIP_TRY(hipMemsetAsync(out.normal, 0, rows * 24, st));
            HIP_TRY(hipMemsetAsync(out.wavelength, 0, rows * 8, st));
            HIP_TRY(hipMemsetAsync(out.travelled, 0, rows * 8, st));
            HIP_TRY(hipMemsetAsync(out.duration, 0, rows * 8, st));
        }
        rc = unpack_launch(s->stage[slot], log->counts + j0, j1 - j0, (int)me, &out, false, st);
        if (rc != PVT_OK) return rc;
    }
    return PVT_OK;
}

int pvt_emit_device(PvtScene* s, const PvtTraceParams* p, double* position, double* direction,
                    double* wavelength, void* stream) {
    if (!s || !p || !s->d_ed) return fail(PVT_ERR_INVALID, "scene has no emitter");
    if (p->n_rays <= 0) return PVT_OK;
    if (p->n_rays > 0x7fffffffLL) return fail(PVT_ERR_INVALID, "n_rays must fit in 31 bits per bundle");
    HIP_TRY(hipSetDevice(s->device));
    KArgs a = base_args(s, p);
    int grid = (int)((p->n_rays + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(emit_kernel, dim3(grid), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), a,
                       position, direction, wavelength);
    HIP_TRY(hipGetLastError());
    return PVT_OK;
}

int pvt_selftest_math(int fn, const double* x_host, double* y_host, int64_t n, int device) {
    if (!x_host || !y_host || n < 0) return fail(PVT_ERR_INVALID, "bad argument");
    if (n == 0) return PVT_OK;
    if (pvt_device_count() <= device) return fail(PVT_ERR_NO_DEVICE, "no such HIP device");
    HIP_TRY(hipSetDevice(device));
    double *dx = nullptr, *dy = nullptr;
    HIP_TRY(hipMalloc(&dx, (size_t)n * 8));
    HIP_TRY(hipMalloc(&dy, (size_t)n * 8));
    HIP_TRY(hipMemcpy(dx, x_host, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(math_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, fn, dx, dy,
                       (long long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(y_host, dy, (size_t)n * 8, hipMemcpyDeviceToHost));
    (void)hipFree(dx);
    (void)hipFree(dy);
    return PVT_OK;
}

int pvt_scene_counters(PvtScene* s, uint64_t* out, int reset) {
    if (!s || !out) return fail(PVT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    unsigned long long rows[64 * 8];
    HIP_TRY(hipMemcpy(rows, s->d_counters, sizeof rows, hipMemcpyDeviceToHost));   // (orders after the launches on the null stream only)
    for (int k = 0; k < 4; k++) out[k] = 0;
    for (int r = 0; r < 64; r++)
        for (int k = 0; k < 4; k++) out[k] += rows[r * 8 + k];
    if (reset) HIP_TRY(hipMemset(s->d_counters, 0, sizeof rows));
    return PVT_OK;
}

int pvt_scene_clock(PvtScene* s, uint64_t* out) {
    if (!s || !out) return fail(PVT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    unsigned long long rows[64 * 8];
    HIP_TRY(hipMemcpy(rows, s->d_counters, sizeof rows, hipMemcpyDeviceToHost));
    out[0] = out[1] = 0;
    for (int r = 0; r < 64; r++) { out[0] += rows[r * 8 + 4]; out[1] += rows[r * 8 + 5]; }
    return PVT_OK;
}

int pvt_scene_launch_span(PvtScene* s, void* stream, uint64_t* out) {
    if (!s || !out) return fail(PVT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    out[0] = out[1] = 0;
    size_t k = 0;
    {
        std::lock_guard<std::mutex> lock(s->slot_mutex);
        while (k < s->slot_of.size() && s->slot_of[k] != reinterpret_cast<hipStream_t>(stream)) k++;
        if (k == s->slot_of.size()) return fail(PVT_ERR_INVALID, "no launch on this stream yet");
    }
    HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    HIP_TRY(hipMemcpy(out, s->d_stamp + 2 * k, 16, hipMemcpyDeviceToHost));
    return PVT_OK;
}

int pvt_scene_launch_info(PvtScene* s, int32_t* grid, int32_t* block, int32_t* lds_bytes) {
    if (!s) return fail(PVT_ERR_INVALID, "null scene");
    if (grid) *grid = s->last_grid;
    if (block) *block = kBlock;
    if (lds_bytes) *lds_bytes = s->last_lds;
    return PVT_OK;
}

int pvt_scene_variant(PvtScene* s) {
    if (!s) return fail(PVT_ERR_INVALID, "null scene");
    if (s->last_variant >= 0) return s->last_variant;
    return choose_variant(s, plan_lds(s, false), false, false).family;
}

int pvt_scene_entry(PvtScene* s) {
    if (!s) return fail(PVT_ERR_INVALID, "null scene");
    return s->last_park ? PVT_ENTRY_PARK : PVT_ENTRY_USUAL;
}

int pvt_scene_solo(PvtScene* s) {
    if (!s) return fail(PVT_ERR_INVALID, "null scene");
    return s->last_solo ? 1 : 0;
}

int pvt_scene_lean_check(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph, const PvtSurfaceTables* rs,
                         const PvtFieldTables* fr, const PvtMapTables* mp, int32_t* lean) {
    if (!t || !lean) return fail(PVT_ERR_INVALID, "null argument");
    if (t->n_nodes <= 0 || t->n_nodes > PVT_MAX_NODES || t->n_recorders > PVT_MAX_RECORDERS) return fail(PVT_ERR_INVALID, "bad argument");
    PackedScene packed;
    const int rc = pack_scene({t, x, ph, rs, fr, mp, nullptr, nullptr, nullptr, kKnowsOrigin}, &packed);
    if (rc != PVT_OK) return rc;
    *lean = packed.lean_ok ? (packed.lean_even ? 2 : 1) : 0;
    // (no failure: the call is answered; pvt_last_error() names the first clause of prove_lean the scene does not meet)
    if (!packed.lean_ok) g_error = std::string("not lean: ") + (packed.lean_why ? packed.lean_why : "unknown");
    return PVT_OK;
}

int pvt_scene_solo_check(const PvtSceneTables* t, const PvtIndexTables* x, const PvtPhaseTables* ph, const PvtSurfaceTables* rs,
                         const PvtFieldTables* fr, const PvtMapTables* mp, int32_t* solo) {
    if (!t || !solo) return fail(PVT_ERR_INVALID, "null argument");
    if (t->n_nodes <= 0 || t->n_nodes > PVT_MAX_NODES || t->n_recorders > PVT_MAX_RECORDERS) return fail(PVT_ERR_INVALID, "bad argument");
    PackedScene packed;
    const int rc = pack_scene({t, x, ph, rs, fr, mp, nullptr, nullptr, nullptr, kKnowsOrigin}, &packed);
    if (rc != PVT_OK) return rc;
    const bool off = getenv("PVT_NO_SOLO") != nullptr;   // (as at scene creation)
    *solo = packed.solo && !off ? 1 : 0;
    // (no failure: the call is answered; pvt_last_error() names the first clause of prove_solo the scene does not meet)
    if (!*solo) g_error = std::string("not solo: ") + (off ? "PVT_NO_SOLO is set" : packed.solo_why ? packed.solo_why : "unknown");
    return PVT_OK;
}

int pvt_mesh_bvh_check(const PvtSceneTables* t, int32_t node, int32_t* n_bvh_nodes, int32_t* n_leaves,
                       int32_t* depth_out) {
    if (!t || node < 0 || node >= t->n_nodes || t->geom_type[node] != PVT_GEOM_MESH)
        return fail(PVT_ERR_INVALID, "not a mesh node");
    const int f0 = t->mesh_face_start[node], fc = t->mesh_face_count[node];
    if (fc <= 0 || f0 < 0 || f0 + fc > t->n_mesh_faces) return fail(PVT_ERR_INVALID, "mesh face range out of bounds");
    std::vector<pvt::BvhNode> nodes;
    std::vector<pvt::MeshTri> tris;
    double centre[3];
    const int root = pvt::BvhBuilder(t->mesh_vertices, t->mesh_faces, t->mesh_normals, nodes, tris).add_mesh(f0, fc, centre);
    if (root != 0 || nodes.size() < 2 || nodes[0].skip != (int)nodes.size()) return fail(PVT_ERR_INVALID, "root skip link");
    std::vector<int> seen(fc, 0);
    int leaves = 0, records = 0, max_depth = 0;
    // from the root down (an explicit stack of {record, parent, depth, the skip link it must carry})
    struct Open { int id, parent, depth, skip; };
    std::vector<Open> todo{{0, -1, 1, (int)nodes.size()}};
    std::vector<char> visited(nodes.size(), 0);
    while (!todo.empty()) {
        const Open o = todo.back();
        todo.pop_back();
        if (o.id < 0 || o.id >= (int)nodes.size() || visited[o.id]++) return fail(PVT_ERR_INVALID, "child link out of range or shared");
        const pvt::BvhNode& b = nodes[o.id];
        records += 1;
        max_depth = std::max(max_depth, o.depth);
        if (b.skip != o.skip) return fail(PVT_ERR_INVALID, "skip link: a left child's is its sibling, a right child's its parent's");
        for (int a = 0; a < 3; a++) {
            if (!(b.lo[a] <= b.hi[a])) return fail(PVT_ERR_INVALID, "empty box");
            if (o.parent >= 0 && (b.lo[a] < nodes[o.parent].lo[a] || b.hi[a] > nodes[o.parent].hi[a]))
                return fail(PVT_ERR_INVALID, "child box not inside its parent");
        }
        if (b.link < 0) {
            leaves += 1;
            const int tri = b.link & pvt::kIndexMask;
            if (tri >= (int)tris.size()) return fail(PVT_ERR_INVALID, "triangle record out of range");
            const pvt::MeshTri& tr = tris[tri];
            const long long local = tr.face - f0;
            if (local < 0 || local >= fc || seen[local]++) return fail(PVT_ERR_INVALID, "face missing or duplicated");
            for (int c = 0; c < 3; c++)
                for (int a = 0; a < 3; a++) {
                    if (tr.v[3 * c + a] != t->mesh_vertices[3 * (size_t)t->mesh_faces[3 * (size_t)tr.face + c] + a])
                        return fail(PVT_ERR_INVALID, "gathered vertex differs from the table");
                    if (tr.v[3 * c + a] - centre[a] < b.lo[a] || tr.v[3 * c + a] - centre[a] > b.hi[a])
                        return fail(PVT_ERR_INVALID, "triangle outside its leaf box");
                }
        } else {
            const int c = b.link;
            if (c <= o.id || (c & 1) != 0) return fail(PVT_ERR_INVALID, "children not a pair on one 64-byte line after their parent");
            todo.push_back({c + 1, o.id, o.depth + 1, o.skip});
            todo.push_back({c, o.id, o.depth + 1, c + 1});
        }
    }
    for (int k = 0; k < fc; k++) if (seen[k] != 1) return fail(PVT_ERR_INVALID, "face missing from the tree");
    if (records + 1 != (int)nodes.size() || visited[1]) return fail(PVT_ERR_INVALID, "records outside the tree");   // (one unused record follows the root)
    // the copy of the top levels for LDS (pvt_bvh.h: stage_top), at several budgets: a walk through the cursors that hits
    // every box must name the records the plain walk names, in its order, and a miss must lead where the plain skip link leads
    auto replay = [](const std::vector<pvt::BvhNode>& plain, const std::vector<pvt::BvhNode>& staged,
                     const std::vector<pvt::BvhNode>& top, int root) -> const char* {
        const int end = plain[root].skip;
        std::vector<int> cursor_of((size_t)(end - root) + 1, -1);
        cursor_of[(size_t)(end - root)] = end;
        std::vector<int> order;
        int c = pvt::first_cursor(staged, root);
        for (int i = root; i != end; i = pvt::next_cursor(plain[i], true)) {
            if (c == end) return "staged walk ends early";
            if ((c & pvt::kTopFlag) ? (size_t)(c & pvt::kIndexMask) >= top.size() : (c < root || c >= end)) return "cursor out of range";
            if (cursor_of[(size_t)(i - root)] >= 0) return "plain walk visits a record twice";
            cursor_of[(size_t)(i - root)] = c;
            order.push_back(i);
            const pvt::BvhNode& rec = pvt::at_cursor(staged, top, c);
            for (int a = 0; a < 3; a++)
                if (rec.lo[a] != plain[i].lo[a] || rec.hi[a] != plain[i].hi[a]) return "staged walk out of order";
            if ((plain[i].link < 0) != (rec.link < 0) || (plain[i].link < 0 && rec.link != plain[i].link)) return "staged leaf differs";
            c = pvt::next_cursor(rec, true);
            if (order.size() > (size_t)(end - root)) return "plain walk does not end";
        }
        if (c != end) return "staged walk does not end at the tree's end";
        for (int i : order) {
            const pvt::BvhNode& rec = pvt::at_cursor(staged, top, cursor_of[(size_t)(i - root)]);
            if (pvt::next_cursor(rec, false) != cursor_of[(size_t)(plain[i].skip - root)]) return "staged skip link differs";
        }
        return nullptr;
    };
    for (size_t budget : {(size_t)3, (size_t)7, (size_t)64, (size_t)768, nodes.size()}) {
        std::vector<pvt::BvhNode> staged = nodes, top;
        pvt::stage_top(staged, std::vector<int>{0}, budget, top);
        if (top.size() > budget) return fail(PVT_ERR_INVALID, "copy of the top levels exceeds its budget");
        if (const char* what = replay(nodes, staged, top, 0)) return fail(PVT_ERR_INVALID, what);
    }
    // ... and ALL the scene's meshes staged together, as scene creation does (the budget is shared out, slots run on from
    // tree to tree): every tree still walks like its plain self
    {
        std::vector<pvt::BvhNode> all;
        std::vector<pvt::MeshTri> all_tris;
        std::vector<int> roots;
        for (int n = 0; n < t->n_nodes; n++)
            if (t->geom_type[n] == PVT_GEOM_MESH)
                roots.push_back(pvt::BvhBuilder(t->mesh_vertices, t->mesh_faces, t->mesh_normals, all, all_tris)
                                    .add_mesh(t->mesh_face_start[n], t->mesh_face_count[n]));
        for (size_t budget : {(size_t)0, (size_t)10, (size_t)100, (size_t)512, all.size()}) {
            std::vector<pvt::BvhNode> staged = all, top;
            pvt::stage_top(staged, roots, budget, top);
            if (top.size() > budget) return fail(PVT_ERR_INVALID, "shared copy of the top levels exceeds its budget");
            for (int r : roots)
                if (const char* what = replay(all, staged, top, r)) return fail(PVT_ERR_INVALID, what);
        }
    }
    if (n_bvh_nodes) *n_bvh_nodes = (int32_t)records;
    if (n_leaves) *n_leaves = leaves;
    if (depth_out) *depth_out = max_depth;
    return PVT_OK;
}

}  // extern "C"

namespace {

thread_local int g_last_multi_reduce = 0;   // 0 none yet, 1 host sum, 2 RCCL on the devices (pvt_last_multi_reduce)

// RCCL, loaded at run time (no link dependency: a process that already holds an RCCL -- PyTorch's -- keeps using
// that copy): ncclReduce of `counts[k]` elements of bufs[k][r] (rank r = entry r of `devs`) into rank 0, all in
// one group.
// Returns 0 = summed on the devices, 1 = RCCL unavailable (nothing enqueued: the caller may sum on the host),
// 2 = a call failed AFTER reduces had been enqueued (shard 0's buffers may hold partial sums: an error, no fall-back).
// Communicators are kept per device list (ncclCommInitAll costs far more than reducing a few KB).
int rccl_reduce_to_first(const std::vector<int>& devs, const std::vector<void*> (&bufs)[4], const size_t (&counts)[4],
                         const bool (&is_f64)[4], std::string* why) {
    typedef int (*InitAll)(void**, int, const int*);
    typedef int (*Reduce)(const void*, void*, size_t, int, int, int, void*, hipStream_t);
    typedef int (*Void)();
    static void* lib = nullptr;
    static InitAll init_all = nullptr; static Reduce reduce = nullptr; static Void group_start = nullptr, group_end = nullptr;
    static std::vector<std::pair<std::vector<int>, std::vector<void*>>> comm_cache;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (!lib) {
        const char* names[] = {getenv("PVT_RCCL_LIB"), "librccl.so", "librccl.so.1"};
        for (const char* nm : names) if (nm && !lib) lib = dlopen(nm, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);   // a copy already mapped
        for (const char* nm : names) if (nm && !lib) lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { *why = std::string("dlopen(librccl): ") + dlerror(); return 1; }
        init_all = (InitAll)dlsym(lib, "ncclCommInitAll"); reduce = (Reduce)dlsym(lib, "ncclReduce");
        group_start = (Void)dlsym(lib, "ncclGroupStart"); group_end = (Void)dlsym(lib, "ncclGroupEnd");
    }
    if (!init_all || !reduce || !group_start || !group_end) { *why = "RCCL symbols missing"; return 1; }
    const int n = (int)devs.size();
    std::vector<void*>* comms = nullptr;
    for (auto& entry : comm_cache) if (entry.first == devs) comms = &entry.second;
    if (!comms) {
        std::vector<void*> fresh((size_t)n, nullptr);
        if (int e = init_all(fresh.data(), n, devs.data())) { *why = "ncclCommInitAll failed with " + std::to_string(e); return 1; }
        comm_cache.emplace_back(devs, fresh);   // (kept for the life of the process)
        comms = &comm_cache.back().second;
    }
    constexpr int kInt64 = 4, kFloat64 = 8, kSum = 0;   // rccl.h: ncclInt64, ncclFloat64, ncclSum
    if (group_start()) { *why = "ncclGroupStart failed"; return 1; }
    bool ok = true;
    for (int k = 0; k < 4 && ok; k++) {
        if (!counts[k]) continue;
        for (int r = 0; r < n && ok; r++) {
            (void)hipSetDevice(devs[(size_t)r]);
            if (reduce(bufs[k][(size_t)r], bufs[k][(size_t)r], counts[k], is_f64[k] ? kFloat64 : kInt64, kSum, 0, (*comms)[(size_t)r], nullptr)) ok = false;
        }
    }
    if (group_end()) ok = false;
    for (int r = 0; r < n; r++) {
        (void)hipSetDevice(devs[(size_t)r]);
        if (hipStreamSynchronize(nullptr) != hipSuccess) ok = false;
    }
    if (!ok) { *why = "an RCCL call failed after reduces had been enqueued"; return 2; }
    return 0;
}

constexpr size_t kChunkRays = 524288;   // rays per upload chunk of a host-buffer bundle (28 MB: ~0.5 ms of PCIe; a chunk costs ~70 us of host time)

// PVT_HOST_PHASES=1 (developer switch): where the milliseconds of a host-buffer call go, on stderr
struct PhaseClock {
    bool on = getenv("PVT_HOST_PHASES") != nullptr;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    std::string line;
    void mark(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        char buf[64];
        snprintf(buf, sizeof buf, " %s %.3f", what, std::chrono::duration<double, std::milli>(now - last).count());
        line += buf;
        last = now;
    }
    void report(size_t n, size_t chunks) const {
        if (on) fprintf(stderr, "[pvt host phases] n %zu chunks %zu ms:%s\n", n, chunks, line.c_str());
    }
};

// The device block of a host-buffer call (rays + tallies) is kept for the next call on the device: freeing 56 MB and
// allocating them again is a quarter of a millisecond per call, an eighth of a 10^6-photon pvt_trace_bundle
// (profiles/r06_host_bundle.txt).  ONE block per device, at most kArenaKeep bytes, handed to one call at a time (a call
// that finds it taken, or too small, allocates its own); pvt_release_cached_memory() frees what is kept.
constexpr size_t kArenaKeep = (size_t)1 << 30;
struct ArenaCache {
    struct Kept { int device; void* ptr; size_t bytes; };
    static std::mutex& mutex() { static std::mutex m; return m; }
    static std::vector<Kept>& kept() { static std::vector<Kept> k; return k; }
    static void* take(int device, size_t bytes, size_t* got) {
        std::lock_guard<std::mutex> lock(mutex());
        auto& k = kept();
        for (size_t i = 0; i < k.size(); i++)
            if (k[i].device == device && k[i].bytes >= bytes) {
                void* p = k[i].ptr;
                *got = k[i].bytes;
                k.erase(k.begin() + (long)i);
                return p;
            }
        return nullptr;
    }
    // -> the block the caller must free itself (the one handed in, or the smaller one it displaced), or null
    static void* give(int device, void* ptr, size_t bytes) {
        if (bytes > kArenaKeep || getenv("PVT_NO_HOST_CACHE")) return ptr;
        std::lock_guard<std::mutex> lock(mutex());
        auto& k = kept();
        for (size_t i = 0; i < k.size(); i++)
            if (k[i].device == device) {
                if (k[i].bytes >= bytes) return ptr;
                void* old = k[i].ptr;
                k[i] = Kept{device, ptr, bytes};
                return old;
            }
        k.push_back(Kept{device, ptr, bytes});
        return nullptr;
    }
    static void release_all() {
        std::vector<Kept> mine;
        {
            std::lock_guard<std::mutex> lock(mutex());
            mine.swap(kept());
        }
        for (auto& b : mine) { (void)hipSetDevice(b.device); (void)hipFree(b.ptr); }
    }
};

// The streams and events of one host-buffer call, taken from a per-device pool (creating and destroying four streams
// per call costs more than tracing a small bundle) and handed back by the destructor.
struct StreamSet {
    hipStream_t copy = nullptr, trace[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev0 = nullptr, ev1 = nullptr, arrived = nullptr;
    int n_trace = 0, device = -1;
    struct Pooled { int device; hipStream_t copy, trace[3]; hipEvent_t ev0, ev1, arrived; };
    static std::mutex& mutex() { static std::mutex m; return m; }
    static std::vector<Pooled>& pool() { static std::vector<Pooled> p; return p; }

    hipError_t open(int dev, int want_trace) {
        device = dev;
        n_trace = want_trace;
        {
            std::lock_guard<std::mutex> lock(mutex());
            auto& p = pool();
            for (size_t k = 0; k < p.size(); k++)
                if (p[k].device == dev) {
                    copy = p[k].copy; ev0 = p[k].ev0; ev1 = p[k].ev1; arrived = p[k].arrived;
                    for (int q = 0; q < 3; q++) trace[q] = p[k].trace[q];
                    p.erase(p.begin() + (long)k);
                    return hipSuccess;
                }
        }
        hipError_t e = hipStreamCreateWithFlags(&copy, hipStreamNonBlocking);
        for (int q = 0; q < 3 && e == hipSuccess; q++) e = hipStreamCreateWithFlags(&trace[q], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreate(&ev0);
        if (e == hipSuccess) e = hipEventCreate(&ev1);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&arrived, hipEventDisableTiming);
        return e;
    }
    ~StreamSet() {
        if (!copy || !trace[0] || !trace[1] || !trace[2] || !ev0 || !ev1 || !arrived) return;   // (a failed open: leaked, once)
        // nothing of this call may still be running on streams the next call will be handed
        (void)hipStreamSynchronize(copy);
        for (int q = 0; q < 3; q++) (void)hipStreamSynchronize(trace[q]);
        std::lock_guard<std::mutex> lock(mutex());
        pool().push_back(Pooled{device, copy, {trace[0], trace[1], trace[2]}, ev0, ev1, arrived});
    }
};

// One host-buffer bundle on one device, in phases (pvt_trace_bundle runs them back to back; pvt_trace_bundle_multi
// runs one per device and can sum the tallies on the devices in between): upload + trace, fetch the tallies, fetch
// the event log.
struct HostBundle {
    PvtScene* scene = nullptr;
    std::vector<void*> bufs;
    const PvtSceneTables* tables = nullptr;
    PvtTraceParams params{};            // (a copy: a shard's parameters live as long as its bundle)
    const PvtTraceParams* p = &params;
    size_t nR = 0, nB = 0, R = 1, B = 1, n_sets = 1, si = 0, sd = 0;
    void *t_i[3] = {nullptr, nullptr, nullptr}, *t_d = nullptr;   // distinct | crossings | bins, sums (device)
    unsigned long long* rows = nullptr;                             // event records (device)
    int* counts = nullptr;
    size_t nrec = 0;
    double ms = 0.0;
    PhaseClock clock;
    size_t n_chunks = 1;
    char* arena = nullptr;              // tallies | rays | counts of the log, one block (ArenaCache)
    size_t arena_bytes = 0, tally_bytes = 0;
    int arena_device = -1;

    ~HostBundle() {
        if (scene) (void)hipSetDevice(scene->device);
        for (void* b : bufs) (void)hipFree(b);
        if (arena)
            if (void* mine = ArenaCache::give(arena_device, arena, arena_bytes)) (void)hipFree(mine);
        clock.mark("free");
        if (scene) pvt_scene_destroy(scene);
        clock.mark("scene-destroy");
        clock.report((size_t)params.n_rays, n_chunks);
    }
    hipError_t dalloc(size_t bytes, void** out) {
        hipError_t e = hipMalloc(out, bytes ? bytes : 8);
        if (e == hipSuccess) bufs.push_back(*out);
        return e;
    }
    hipError_t move(void* dst, const void* src, size_t pitch_elems, size_t width_elems, hipMemcpyKind kind) const {
        if (width_elems == 0) return hipSuccess;
        if (n_sets == 1) return hipMemcpy(dst, src, width_elems * 8, kind);
        return hipMemcpy2D(dst, pitch_elems * 8, src, pitch_elems * 8, width_elems * 8, n_sets, kind);
    }

    // scene + rays + tallies (seeded with `seed`, or zero) on `device`, trace enqueued and finished.
    //
    // The rays cross PCIe in CHUNKS and a chunk is traced while the next one is still on its way: the copies go down
    // one stream, each chunk's launch waits for its own copy and runs on one of three trace streams used in turn (the
    // drain tail of one launch -- a few long histories -- is covered by the bulk of the next), ray i keeps the
    // stream seed + ray_offset + i whatever chunk carries it, every launch adds into the same tallies with atomics and
    // writes the event-log rows of its own rays (inner chunk boundaries are multiples of record_every).  One upload
    // followed by one launch left the GPU idle for the whole upload: 56 MB at the link's ~50 GB/s is 1.1 ms, the trace
    // of those 10^6 photons 0.65 ms (profiles/r06_host_io.txt).
    int trace(const PvtSceneTables* tb, const PvtEmitterTables* emitter, const PvtRays* rays, const PvtTraceParams* pp,
              const PvtTallies* seed, bool want_log, int device) {
        tables = tb;
        params = *pp;
        params.flags &= ~(int64_t)PVT_FLAG_CARRY_OUT;   // a scene that lives for one call has no next launch to carry photons to
        int rc = create_scene({tables, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, kKnowsHostBuffer}, device, &scene);
        if (rc != PVT_OK) return rc;
        if (emitter) {
            rc = pvt_scene_set_emitter(scene, emitter);
            if (rc != PVT_OK) return rc;
        }
        clock.mark("scene");
        const size_t n = (size_t)p->n_rays;
        nR = (size_t)tables->n_recorders; nB = (size_t)tables->total_bins;
        R = nR > 0 ? nR : 1; B = nB > 0 ? nB : 1;
        // tally sets (PvtTraceParams.tally_bundle): the device copies keep the caller's strides, slices move as
        // 2-D copies (one row per set)
        n_sets = p->tally_bundle > 0 ? (size_t)((p->n_rays + p->tally_bundle - 1) / p->tally_bundle) : 1;
        si = n_sets > 1 ? (size_t)p->tally_stride_i64 : 0; sd = n_sets > 1 ? (size_t)p->tally_stride_f64 : 0;
        if (n_sets > 1 && (si < R || si < B || sd < R * 8)) return fail(PVT_ERR_INVALID, "tally strides smaller than a set");
        if (p->record_every > 0 && !want_log) return fail(PVT_ERR_INVALID, "record_every > 0 needs an event log");
        // ONE allocation for the rays, the tallies and the counts of the log (allocating and freeing device memory is a
        // large part of a small call); the event records, which can be gigabytes, have their own
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t bytes_i[3] = {((n_sets - 1) * si + R) * 8, ((n_sets - 1) * si + R) * 8, ((n_sets - 1) * si + B) * 8};
        const size_t bytes_d = ((n_sets - 1) * sd + R * 8) * 8;
        nrec = p->record_every > 0 ? (size_t)((p->n_rays + p->record_every - 1) / p->record_every) : 0;
        tally_bytes = up(bytes_i[0]) + up(bytes_i[1]) + up(bytes_i[2]) + up(bytes_d);
        const size_t ray_bytes = rays ? up(n * 24) * 2 + up(n * 8) : 0;
        const size_t need = tally_bytes + ray_bytes + up(nrec * 4);
        arena_device = device;
        arena = (char*)ArenaCache::take(device, need, &arena_bytes);
        if (!arena) {
            HIP_TRY(hipMalloc((void**)&arena, need));
            arena_bytes = need;
        }
        char* at = arena;
        for (int k = 0; k < 3; k++) { t_i[k] = at; at += up(bytes_i[k]); }
        t_d = at; at += up(bytes_d);
        char *dp = nullptr, *dd = nullptr, *dw = nullptr;
        if (rays) { dp = at; at += up(n * 24); dd = at; at += up(n * 24); dw = at; at += up(n * 8); }
        if (nrec) {
            counts = (int*)at; at += up(nrec * 4);
            void* b1;
            HIP_TRY(dalloc(nrec * (size_t)p->max_events * kRecWords * 8, &b1));
            rows = (unsigned long long*)b1;
        }
        clock.mark("alloc");
        // The trace ADDS into the caller's tallies: the device copies start from them.  A caller who hands in zeros (the
        // reference's trace_bundle always starts from zero, _kernel.pyx:1035-1047) costs a fill on the first trace stream,
        // no transfer; the other trace streams wait for that fill.
        bool seeded = false;
        if (seed) {
            auto any = [&](const void* base, size_t stride_elems, size_t width_elems) {
                for (size_t j = 0; j < n_sets && !seeded; j++) {
                    const unsigned long long* w = (const unsigned long long*)base + j * stride_elems;
                    for (size_t q = 0; q < width_elems; q++)
                        if (w[q]) { seeded = true; break; }
                }
            };
            any(seed->rec_distinct, si, nR); any(seed->rec_crossings, si, nR);
            any(seed->rec_sums, sd, nR * 8); any(seed->rec_bins, si, nB);
        }
        if (seeded) {
            HIP_TRY(hipMemset(arena, 0, tally_bytes));
            HIP_TRY(move(t_i[0], seed->rec_distinct, si, nR, hipMemcpyHostToDevice));
            HIP_TRY(move(t_i[1], seed->rec_crossings, si, nR, hipMemcpyHostToDevice));
            HIP_TRY(move(t_d, seed->rec_sums, sd, nR * 8, hipMemcpyHostToDevice));
            HIP_TRY(move(t_i[2], seed->rec_bins, si, nB, hipMemcpyHostToDevice));
            HIP_TRY(hipDeviceSynchronize());   // (these ran on the null stream; the streams below do not wait for it)
        }
        PvtTallies dt{(int64_t*)t_i[0], (int64_t*)t_i[1], (double*)t_d, (int64_t*)t_i[2]};

        // chunks: about kChunkRays rays each, inner boundaries on multiples of record_every; a launch with tally sets
        // indexes its sets from its first ray and is not split
        size_t chunk = n;
        if (rays && n_sets == 1 && n > 0) {
            size_t want = n >= kChunkRays + kChunkRays / 2 ? kChunkRays : n;
            if (const char* env = getenv("PVT_HOST_CHUNK_RAYS")) {   // (tests: 0 = one upload and one launch, k = chunks of k rays)
                const long long k = atoll(env);
                want = k > 0 ? (size_t)k : n;
            }
            if (p->record_every > 1) {   // inner boundaries on multiples of record_every: a chunk's recorded rays are whole rows of the log
                const size_t re = (size_t)p->record_every;
                want = (want + re - 1) / re * re;
            }
            chunk = want < n ? want : n;
        }
        n_chunks = n ? (n + chunk - 1) / chunk : 1;
        StreamSet ss;
        HIP_TRY(ss.open(device, n_chunks > 1 ? 3 : 1));
        if (!seeded) {
            HIP_TRY(hipMemsetAsync(arena, 0, tally_bytes, ss.trace[0]));
            HIP_TRY(hipEventRecord(ss.arrived, ss.trace[0]));
            for (int k = 1; k < ss.n_trace; k++) HIP_TRY(hipStreamWaitEvent(ss.trace[k], ss.arrived, 0));
        }
        clock.mark("tallies");
        HIP_TRY(hipEventRecord(ss.ev0, ss.trace[0]));
        for (size_t k = 0; k < n_chunks && n > 0; k++) {   // (an empty bundle launches nothing)
            const size_t lo = k * chunk, hi = lo + chunk < n ? lo + chunk : n;
            hipStream_t st = ss.trace[k % ss.n_trace];
            PvtRays drays{};
            if (rays) {
                HIP_TRY(hipMemcpyAsync(dp + lo * 24, rays->position + lo * 3, (hi - lo) * 24, hipMemcpyHostToDevice, ss.copy));
                HIP_TRY(hipMemcpyAsync(dd + lo * 24, rays->direction + lo * 3, (hi - lo) * 24, hipMemcpyHostToDevice, ss.copy));
                HIP_TRY(hipMemcpyAsync(dw + lo * 8, rays->wavelength + lo, (hi - lo) * 8, hipMemcpyHostToDevice, ss.copy));
                HIP_TRY(hipEventRecord(ss.arrived, ss.copy));
                HIP_TRY(hipStreamWaitEvent(st, ss.arrived, 0));
                drays = PvtRays{(const double*)(dp + lo * 24), (const double*)(dd + lo * 24), (const double*)(dw + lo * 8)};
            }
            PvtTraceParams pk = params;
            pk.n_rays = (int64_t)(hi - lo);
            pk.ray_offset = params.ray_offset + (uint64_t)lo;
            PvtEventRecords rec{};
            if (nrec) {
                const size_t j0 = lo / (size_t)p->record_every;   // (lo is a multiple of record_every)
                rec = PvtEventRecords{counts + j0, reinterpret_cast<uint64_t*>(rows + j0 * (size_t)p->max_events * kRecWords)};
            }
            rc = pvt_trace_device_records(scene, rays ? &drays : nullptr, &pk, &dt, nrec ? &rec : nullptr, st);
            if (rc != PVT_OK) return rc;
        }
        clock.mark("enqueue");
        for (int k = 1; k < ss.n_trace; k++) {   // the last event waits for every trace stream
            HIP_TRY(hipEventRecord(ss.arrived, ss.trace[k]));
            HIP_TRY(hipStreamWaitEvent(ss.trace[0], ss.arrived, 0));
        }
        HIP_TRY(hipEventRecord(ss.ev1, ss.trace[0]));
        HIP_TRY(hipEventSynchronize(ss.ev1));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ss.ev0, ss.ev1));
        ms = t;   // (several chunks: from the start of the upload to the end of the last launch)
        clock.mark("wait");
        return PVT_OK;
    }

    int fetch_tallies(const PvtTallies* out) {
        HIP_TRY(hipSetDevice(scene->device));
        if (n_sets == 1) {   // the four arrays lie side by side in the block: one transfer, four host copies
            std::vector<char> host(tally_bytes);
            HIP_TRY(hipMemcpy(host.data(), arena, tally_bytes, hipMemcpyDeviceToHost));
            std::memcpy(out->rec_distinct, host.data() + ((char*)t_i[0] - arena), nR * 8);
            std::memcpy(out->rec_crossings, host.data() + ((char*)t_i[1] - arena), nR * 8);
            std::memcpy(out->rec_sums, host.data() + ((char*)t_d - arena), nR * 8 * 8);
            std::memcpy(out->rec_bins, host.data() + ((char*)t_i[2] - arena), nB * 8);
            clock.mark("fetch-tallies");
            return PVT_OK;
        }
        HIP_TRY(move(out->rec_distinct, t_i[0], si, nR, hipMemcpyDeviceToHost));
        HIP_TRY(move(out->rec_crossings, t_i[1], si, nR, hipMemcpyDeviceToHost));
        HIP_TRY(move(out->rec_sums, t_d, sd, nR * 8, hipMemcpyDeviceToHost));
        HIP_TRY(move(out->rec_bins, t_i[2], si, nB, hipMemcpyDeviceToHost));
        clock.mark("fetch-tallies");
        return PVT_OK;
    }

    // The event log: the caller's column arrays get the reference's fill values on the host (memset / fill), the
    // records the rays wrote cross PCIe PACKED -- `counts[j]` rows of recorded ray j, gathered on the device -- and
    // are scattered into the columns by this thread.  (Moving the dense columns costs 117 bytes x max_events per
    // recorded ray over PCIe, of which a ray writes a dozen rows: 15 GB for the reference's README case.)
    int fetch_log(const PvtEventLog* log) {
        if (!(p->record_every > 0)) return PVT_OK;
        HIP_TRY(hipSetDevice(scene->device));
        const size_t me = (size_t)p->max_events, total_rows = nrec * me;
        HIP_TRY(hipMemcpy(log->counts, counts, nrec * 4, hipMemcpyDeviceToHost));
        std::vector<long long> first(nrec + 1, 0);
        for (size_t j = 0; j < nrec; j++) first[j + 1] = first[j] + log->counts[j];
        const size_t used = (size_t)first[nrec];
        std::memset(log->kind, 0, total_rows);
        std::memset(log->hit, 0xFF, total_rows * 4); std::memset(log->container, 0xFF, total_rows * 4);
        std::memset(log->adjacent, 0xFF, total_rows * 4); std::memset(log->component, 0xFF, total_rows * 4);
        std::memset(log->source, 0xFF, total_rows * 4);
        std::memset(log->position, 0, total_rows * 24); std::memset(log->direction, 0, total_rows * 24);
        std::memset(log->normal, 0, total_rows * 24);
        std::memset(log->wavelength, 0, total_rows * 8); std::memset(log->travelled, 0, total_rows * 8);
        std::memset(log->duration, 0, total_rows * 8);
        if (!used) return PVT_OK;
        void *d_first, *d_packed;
        HIP_TRY(dalloc((nrec + 1) * 8, &d_first));
        HIP_TRY(dalloc(used * kRecWords * 8, &d_packed));
        HIP_TRY(hipMemcpy(d_first, first.data(), (nrec + 1) * 8, hipMemcpyHostToDevice));
        const int rays_per_block = me >= (size_t)kBlock ? 1 : (int)((size_t)kBlock / me);
        const long long gx = ((long long)nrec + rays_per_block - 1) / rays_per_block;
        const int gy = rays_per_block > 1 ? 1 : (int)((me + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(pack_log_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kBlock), 0, nullptr, rows, counts,
                           (const long long*)d_first, (unsigned long long*)d_packed, (long long)nrec, (int)me, rays_per_block);
        HIP_TRY(hipGetLastError());
        std::vector<unsigned long long> packed(used * kRecWords);
        HIP_TRY(hipMemcpy(packed.data(), d_packed, used * kRecWords * 8, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < nrec; j++) {
            const unsigned long long* r = packed.data() + (size_t)first[j] * kRecWords;
            size_t row = j * me;
            for (int k = 0; k < log->counts[j]; k++, r += kRecWords, row++) {
                log->hit[row] = (int32_t)(uint32_t)r[0]; log->container[row] = (int32_t)(uint32_t)(r[0] >> 32);
                log->adjacent[row] = (int32_t)(uint32_t)r[1]; log->component[row] = (int32_t)(uint32_t)(r[1] >> 32);
                log->source[row] = (int32_t)(uint32_t)r[2]; log->kind[row] = (uint8_t)(r[2] >> 32);
                std::memcpy(log->position + 3 * row, r + 3, 24);
                std::memcpy(log->direction + 3 * row, r + 6, 24);
                std::memcpy(log->normal + 3 * row, r + 9, 24);
                std::memcpy(log->wavelength + row, r + 12, 8);
                std::memcpy(log->travelled + row, r + 13, 8);
                std::memcpy(log->duration + row, r + 14, 8);
            }
        }
        return PVT_OK;
    }
};

}  // namespace

extern "C" {

// Host-buffer entry: the literal stand-in for _kernel.trace_bundle.
int pvt_trace_bundle(const PvtSceneTables* tables, const PvtEmitterTables* emitter, const PvtRays* rays,
                     const PvtTraceParams* p, const PvtTallies* tl, const PvtEventLog* log, int device,
                     double* kernel_ms) {
    if (!tables || !p || !tl) return fail(PVT_ERR_INVALID, "null argument");
    HostBundle hb;
    int rc = hb.trace(tables, emitter, rays, p, tl, log != nullptr, device);
    if (rc != PVT_OK) return rc;
    if (kernel_ms) *kernel_ms = hb.ms;
    rc = hb.fetch_tallies(tl);
    if (rc != PVT_OK) return rc;
    return hb.fetch_log(log);
}

void pvt_release_cached_memory(void) { ArenaCache::release_all(); }

int pvt_shard_range(int64_t n_rays, int shard, int n_shards, int64_t align, int64_t* start, int64_t* stop) {
    if (n_rays < 0 || n_shards <= 0 || shard < 0 || shard >= n_shards || !start || !stop)
        return fail(PVT_ERR_INVALID, "bad shard arguments");
    if (align < 1) align = 1;
    auto edge = [&](int r) -> int64_t {
        if (r <= 0) return 0;
        if (r >= n_shards) return n_rays;
        // n_rays * r fits: n_rays < 2^31 per bundle in practice, and __int128 keeps the general case exact
        const int64_t e = (int64_t)(((__int128)n_rays * r) / n_shards);
        return (e / align) * align;
    };
    *start = edge(shard);
    *stop = edge(shard + 1);
    return PVT_OK;
}

int pvt_trace_bundle_multi(const PvtSceneTables* tables, const PvtEmitterTables* emitter, const PvtRays* rays,
                           const PvtTraceParams* p, const PvtTallies* tl, const PvtEventLog* log,
                           const int* devices, int n_devices, double* kernel_ms) {
    if (!tables || !p || !tl || !devices || n_devices <= 0) return fail(PVT_ERR_INVALID, "null argument");
    if (p->record_every > 0 && !log) return fail(PVT_ERR_INVALID, "record_every > 0 needs an event log");
    const int ndev = pvt_device_count();
    for (int g = 0; g < n_devices; g++)
        if (devices[g] < 0 || devices[g] >= ndev) return fail(PVT_ERR_NO_DEVICE, "no such HIP device in the device list");
    const char* how = getenv("PVT_MULTI_REDUCE");   // "host": never RCCL; "rccl": also for a single device (self-test)
    const bool force_rccl = how && std::string(how) == "rccl", never_rccl = how && std::string(how) == "host";
    if (n_devices == 1 && !force_rccl) return pvt_trace_bundle(tables, emitter, rays, p, tl, log, devices[0], kernel_ms);
    // the shards below own ONE tally set each (R / B / R*8 elements) and shard edges ignore bundle boundaries
    if (p->tally_bundle > 0)
        return fail(PVT_ERR_INVALID, "tally_bundle is not supported over a device list; trace the group on one device");

    const size_t nR = (size_t)tables->n_recorders, nB = (size_t)tables->total_bins;
    struct Shard {
        int rc = PVT_OK;
        std::string error;
        bool traced = false;
        HostBundle hb;
    };
    std::vector<Shard> shards((size_t)n_devices);
    auto parallel = [&](auto&& body) {   // one host thread per device-list entry
        std::vector<std::thread> workers;
        for (int g = 0; g < n_devices; g++)
            workers.emplace_back([&, g]() {
                Shard& sh = shards[(size_t)g];
                if (sh.rc == PVT_OK) sh.rc = body(sh, g);
                if (sh.rc != PVT_OK && sh.error.empty()) sh.error = g_error;   // thread-local: carry it to the caller's thread
            });
        for (auto& w : workers) w.join();
    };
    auto first_error = [&]() -> int {
        for (int g = 0; g < n_devices; g++)
            if (shards[(size_t)g].rc != PVT_OK)
                return fail(shards[(size_t)g].rc, "shard " + std::to_string(g) + " on device " + std::to_string(devices[g]) + ": " + shards[(size_t)g].error);
        return PVT_OK;
    };
    // 1. every shard: its own scene, rays, zeroed tallies and event records on its device; traced to completion
    parallel([&](Shard& sh, int g) -> int {
        int64_t start = 0, stop = 0;
        int rc = pvt_shard_range(p->n_rays, g, n_devices, p->record_every, &start, &stop);
        if (rc != PVT_OK || stop <= start) return rc;
        PvtTraceParams q = *p;
        q.n_rays = stop - start;
        q.ray_offset = p->ray_offset + (uint64_t)start;
        PvtRays r{};
        if (rays) r = PvtRays{rays->position + 3 * start, rays->direction + 3 * start, rays->wavelength + start};
        // (the shard's params must outlive the bundle: keep a copy inside it)
        sh.traced = true;
        return sh.hb.trace(tables, emitter, rays ? &r : nullptr, &q, nullptr, log != nullptr, devices[g]);
    });
    int rc = first_error();
    // 2. the tallies: summed ON THE DEVICES with RCCL (one communicator per device-list entry, ncclReduce to the
    //    first shard) when every entry is a different GPU and the library can be loaded -- else on the host
    bool on_device = false;
    std::vector<int> live;
    for (int g = 0; g < n_devices; g++) if (shards[(size_t)g].traced) live.push_back(g);
    if (rc == PVT_OK && !never_rccl && !live.empty() && (live.size() > 1 || force_rccl)) {
        bool distinct = true;
        for (size_t x = 0; x < live.size(); x++)
            for (size_t y = x + 1; y < live.size(); y++)
                if (devices[live[x]] == devices[live[y]]) distinct = false;
        if (distinct) {
            std::vector<int> devs;
            std::vector<void*> bufs[4];
            for (int g : live) {
                devs.push_back(devices[g]);
                HostBundle& hb = shards[(size_t)g].hb;
                bufs[0].push_back(hb.t_i[0]); bufs[1].push_back(hb.t_i[1]); bufs[2].push_back(hb.t_i[2]); bufs[3].push_back(hb.t_d);
            }
            const size_t counts[4] = {nR, nR, nB, nR * 8};
            const bool is_f64[4] = {false, false, false, true};
            std::string why;
            const int how_it_went = rccl_reduce_to_first(devs, bufs, counts, is_f64, &why);
            on_device = how_it_went == 0;
            if (how_it_went == 2) rc = fail(PVT_ERR_HIP, "summing the shards' tallies with RCCL failed midway (" + why + "); the first shard's buffers "
                                                        "may hold partial sums, so nothing is returned");
            else if (!on_device && force_rccl) rc = fail(PVT_ERR_HIP, "RCCL reduce requested (PVT_MULTI_REDUCE=rccl) but unavailable: " + why);
        }
    }
    g_last_multi_reduce = on_device ? 2 : 1;
    // 3. tallies to the host (one shard's after a device-side sum, every shard's otherwise), added to the caller's
    if (rc == PVT_OK) {
        std::vector<int64_t> distinct(nR ? nR : 1), crossings(nR ? nR : 1), bins(nB ? nB : 1);
        std::vector<double> sums(nR ? nR * 8 : 1);
        for (size_t x = 0; x < live.size() && rc == PVT_OK; x++) {
            if (on_device && x > 0) break;
            PvtTallies t{distinct.data(), crossings.data(), sums.data(), bins.data()};
            rc = shards[(size_t)live[x]].hb.fetch_tallies(&t);
            if (rc != PVT_OK) break;
            for (size_t i = 0; i < nR; i++) { tl->rec_distinct[i] += distinct[i]; tl->rec_crossings[i] += crossings[i]; }
            for (size_t i = 0; i < nR * 8; i++) tl->rec_sums[i] += sums[i];
            for (size_t i = 0; i < nB; i++) tl->rec_bins[i] += bins[i];
        }
    }
    // 4. each shard's rows of the event log, into the caller's arrays (inner shard edges are multiples of record_every)
    if (rc == PVT_OK && p->record_every > 0) {
        parallel([&](Shard& sh, int g) -> int {
            if (!sh.traced) return PVT_OK;
            int64_t start = 0, stop = 0;
            (void)pvt_shard_range(p->n_rays, g, n_devices, p->record_every, &start, &stop);
            const int64_t j0 = start / p->record_every, row0 = j0 * p->max_events;
            PvtEventLog l{log->counts + j0, log->kind + row0, log->hit + row0, log->container + row0,
                          log->adjacent + row0, log->component + row0, log->source + row0,
                          log->position + 3 * row0, log->direction + 3 * row0, log->normal + 3 * row0,
                          log->wavelength + row0, log->travelled + row0, log->duration + row0};
            return sh.hb.fetch_log(&l);
        });
        rc = first_error();
    }
    double longest = 0.0;
    for (int g : live) {
        if (shards[(size_t)g].hb.ms > longest) longest = shards[(size_t)g].hb.ms;
    }
    if (kernel_ms) *kernel_ms = longest;
    return rc;
}

int pvt_last_multi_reduce(void) { return g_last_multi_reduce; }

int pvt_node_grid_plan(const PvtSceneTables* t, int32_t* dims, double* lo, double* cell, double* guard, int32_t* odd,
                       uint64_t* masks, int64_t masks_cap) {
    if (!t || !dims || t->n_nodes <= 0 || t->n_nodes > PVT_MAX_NODES) return fail(PVT_ERR_INVALID, "bad argument");
    NodeGrid g;
    const bool on = plan_node_grid(t, &g);
    for (int a = 0; a < 3; a++) {
        dims[a] = on ? g.n[a] : 0;
        if (lo) lo[a] = on ? g.lo[a] : 0.0;
        if (cell) cell[a] = on ? g.cell[a] : 0.0;
    }
    if (guard) *guard = on ? g.guard : 0.0;
    if (odd) *odd = on && g.odd ? 1 : 0;
    if (on && masks) {
        const size_t cells = (size_t)g.n[0] * g.n[1] * g.n[2];
        for (size_t c = 0; c < cells; c++)
            for (int w = 0; w < 2; w++)
                if ((int64_t)(c * 2 + w) < masks_cap) masks[c * 2 + w] = w < g.words ? g.masks[c * g.words + w] : 0ull;
    }
    return PVT_OK;
}

}  // extern "C"
