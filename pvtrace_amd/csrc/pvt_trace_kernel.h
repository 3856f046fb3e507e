// pvt_trace_kernel.h -- device side of the photon engine: the scene-record layout shared
// with the host packer (enums + `Lay` + `KArgs`), the per-ray RNG, table lookups, the emitter
// and the trace kernel itself.  Included once, by pvt_trace.hip (which holds the design
// overview, the host-side packing and the C ABI).
#pragma once
// Developer switches (build-time; everything else that used to be one is a constant now -- the experiments behind them are
// closed, docs/history.md): PVT_STATS (tools/: -DPVT_STATS=1 builds print per-launch lane statistics), PVT_TIMELINE (per-wave
// stamps), and PVT_DEV_VARIANTS in pvt_trace.hip (fast developer builds of a few variants).
constexpr int kMeshWaves = 4;   // waves per SIMD the mesh variants are held to (registers: 512 / waves; LDS per workgroup: 160 KB / waves)
#ifndef PVT_STATS
#define PVT_STATS 0
#endif
// Developer-only: every wave writes wall-clock stamps (start, tables staged, first step, cursor dry, end) and its
// iteration count to KArgs::timeline (tools/gpu_wave_timeline.py)
#ifndef PVT_TIMELINE
#define PVT_TIMELINE 0
#endif

namespace {

constexpr int kBlock = 256;          // 4 wavefronts
constexpr int kChunk = 64;           // rays a wave seeds and hands out at a time
constexpr int kEndClaim = 64;   // rays per claim in the last two rounds of a launch (see the refill)
constexpr int kClaim = kChunk;   // rays a wave claims per cursor atomic: every wave of a launch adds to the SAME
                                     // word, and a device-scope atomic that returns a value costs the wave a round trip
                                     // through the fabric; claiming several chunks at once takes the cursor off the critical
                                     // path -- measured (round 3): 1, 2 and 4 chunks per claim give the same throughput at
                                     // 10^6 and 4 10^6 photons per launch, serial and pipelined: the cursor is NOT a bottleneck
constexpr int kWaves = kBlock / 64;
constexpr int kCursorSlots = 64;     // distinct HIP streams that may trace one scene concurrently
constexpr int kMaxSets = 1024;       // tally sets (bundles of a stream) one launch may serve
constexpr int kRecPlain = 1 << 30;   // flag on a recorder id in the candidate tables: matches without reading its row (host: scene_create)
constexpr int kTallyQ = 64;          // first crossings a wave parks before it computes their statistics together
constexpr int kXSlots = 72;          // LDS photon-state slots used to repack a draining workgroup (>= 64: the
                                     // last stage packs the survivors into one wave; >= 69 so that the 8 KB of
                                     // per-wave seed pools fit in the same region); small enough that FIVE
                                     // workgroups' LDS fit a CU, so a fresh workgroup of the next launch can
                                     // start while draining ones still hold theirs (+6 % on pipelined bundles)
// workgroup control words in LDS
enum { CTL_EXHAUSTED = 0, CTL_DONE = 1, CTL_IN = 2, CTL_LIVE = 6, CTL_COUNT = 16, CTL_CLOCK = 22, CTL_WORDS = 26 };   // (CTL_COUNT: three u64 sums, see KArgs::counters; CTL_CLOCK: two u64 stamps, see KArgs::stamp)
constexpr double kEps = 2.220446049250313e-13;       // _kernel.pyx:29
constexpr double kAlphaZero = 1e-8;                  // :32
constexpr double kCcm = 2.99792458e10;               // :33
constexpr double kPi = 3.14159265358979323846;
constexpr unsigned long long kEmitSalt = 0xA5A5A5A55A5A5A5Aull;

// Scene blobs are arrays of fixed-stride RECORDS (one double blob, one int32 blob), so a
// table element is addressed as base + index*stride + field with compile-time strides
// and fields; only the eight record bases below live in SGPRs (node records start at 0).
// Node records are what a photon reads of the node it is in / hits / tests, and what the intersection loop reads of
// EVERY node: 64 bytes (one scalar load in the wave-uniform loop; a stride of 72 bytes, meant to spread the per-lane
// reads of the grid walk over the LDS banks, gained 1 % there and cost the headline scene an integer multiply per
// record address).
// Rotations, refractive-index reciprocals and critical angles live in small side tables indexed by CLASS (nodes with
// bit-identical rotations / refractive indices share an entry), so a scene of 120 tiles costs 12 KB of LDS, not 56.
enum { ND_T = 0, ND_PARAMS = 3, ND_BITS = 6, ND_N = 7, ND = 8 };  // node doubles: translation of world->local, three shape
                                                                 // parameters (a shape with four keeps them behind the blob), one word of {bit 0: the
                                                                 // rotation is the identity, bit for bit; bits 8-15: geometry
                                                                 // type; high half: rotation class}, refractive index
enum { NI_SURF = 0, NI_CSTART, NI_CCOUNT, NI_CREC, NI_KSTART, NI_KCOUNT, NI_MESH, NI_CAND, NI_NCLS, NI };  // node ints (NI_CSTART: id of the
                                                                 // node's first component, what events and recorders name;
                                                                 // NI_CREC: its first component RECORD -- identical components
                                                                 // share records; NI_MESH: BVH root, -1 = none; NI_CAND: block of
                                                                 // the recorder candidate tables, -1 = nobody listens to the node;
                                                                 // NI_NCLS: refractive-index class)
enum { RT_W2L = 0, RT_L2W = 9, RT = 18 };                         // Lay::rot_d records: the 3x3 blocks of world->local and local->world
enum { kFrShape = 0, kFrLower = 3, kFrH = 6, kFrRot = 9, kFrT = 18, kFrComp = 21 };   // a fielded node's record in KArgs::fd:
                                                                 // shape, lower, cell widths, world->local rotation (row-major)
                                                                 // and translation, then one value-table offset per component
enum { kMnCount = 0, kMnRot = 1, kMnT = 10, kMnPath = 13, kMnRec = 14 };   // a mapped node's block in KArgs::md: its map count, world->local
                                                                 // rotation (row-major) and translation, how many of its maps are
                                                                 // path-length maps (the marker path_map_call's caller asks), then
                                                                 // its map records
enum { kMrKind = 0, kMrComp, kMrShape, kMrLower = 5, kMrH = 8, kMrNw = 11, kMrWlo, kMrWhi, kMrOff, kMr = 16 };   // a map record: event
                                                                 // kind (a PVT_EV_* or PVT_MAP_PATHLENGTH), component (-1: any), shape, lower, cell widths,
                                                                 // wavelength bins (0: no axis) and range, first slot
enum { CD_QY = 0, CD_TAU_RAD, CD_TAU_NR, CD_PHASE, CD_ABS_SCALE, CD_EMS_SCALE_X, CD_EMS_SCALE_C,
       CD_ABS_RCP, CD_EMS_RCP_X, CD_EMS_RCP_C, CD_ABS_W, CD_EMS_W, CD };   // component doubles (*_RCP: RN(1/spacing) of an evenly spaced table, else NaN;
                                                            // *_W: the spacing w when additionally xs[i] == xs[0] + i*w bit for bit, else NaN)
enum { CI_TYPE = 0, CI_PHASE, CI_ABS_X, CI_ABS_Y, CI_ABS_N, CI_EMS_X, CI_EMS_CDF, CI_EMS_N,
       CI_ABS_G, CI_EMS_GX, CI_EMS_GC, CI_ABS_HIST, CI_EMS_HIST, CI };  // *_G*: guide tables; *_HIST: step tables
enum { RD_FACET = 0, RD_ATOL = 3, RD = 4 };                                     // recorder
enum { RI_NODE = 0, RI_EVENT, RI_HAS_FACET, RI_HSTART, RI_HN, RI_SRC_MODE, RI_SRC_ID, RI };
enum { HD_LO_A = 0, HD_HI_A, HD_LO_B, HD_HI_B, HD_RA, HD_RB, HD };               // histogram (RA/RB: RN(1/(hi-lo)), NaN = divide)
enum { HI_PA = 0, HI_PB, HI_NA, HI_NB, HI_OFF, HI };
enum { KD_FACET = 0, KD_LO = 3, KD_HI = 6, KD_REFL = 9, KD = 10 };              // coating
enum { KI_RMODE = 0, KI_TMODE, KI_TNW, KI_TNA, KI_TW, KI_TA, KI_TV, KI };   // KI_T*: reflectivity table R(wavelength, angle) --
                                                                 // its axis lengths (KI_TNW = 0: none) and where its wavelengths,
                                                                 // angles (radians) and values (row-major by angle) start in
                                                                 // the double blob, after the spectra
enum { kCaA = 0, kCaNw, kCaNa, kCaTab, kCa };   // an absorbing scene's record per coating row at KArgs::cabs_d: the scalar
                                                                 // absorptivity, its table's axis lengths (kCaNw = 0: none) and
                                                                 // where the table starts in the double blob (wavelengths, angles
                                                                 // in radians, values row-major by angle)
enum { kClRTab = 0, kClRAxis, kClTTab, kClTAxis, kCl };   // a scattering coating's record per coating row at KArgs::clobe_i:
                                                                 // where the reflection lobe's table starts in the double blob
                                                                 // (-1: the row reflects by a built-in mode) and its axis
                                                                 // (PVT_LOBE_*), the same of the transmission lobe
enum { kPrShape = 0, kPrBounded = 3, kPrLower = 6, kPrH = 9, kPrMask = 12, kPr = 13 };   // a coating pattern's record at KArgs::pd_d:
                                                                 // shape, per axis 1 = bounded (else index 0), lower, cell
                                                                 // widths, and where its mask starts, in BYTES from pd
enum { kSgShape = 0, kSgBounded = 3, kSgLower = 6, kSgH = 9, kSgCdf = 12 };   // a position grid's record in the emitter's double
                                                                 // blob (a PVT_POS_GRID light's pos_param[0] names where it
                                                                 // starts): shape, per axis 1 = bounded (else the coordinate
                                                                 // is 0 and no draw is taken), lower, cell widths, then the
                                                                 // CDF of cells + 1 entries

struct Lay {  // record bases (elements) inside the blobs; spectra follow the records and are
              // addressed by absolute offsets stored in the component records
    int comp_d, rec_d, hist_d, coat_d;
    int comp_i, rec_i, hist_i, coat_i;
    int cand_i;     // per node that carries recorders (NI_CAND) 7 x {start, count, bin[6]}: recorders that can fire
                    // for a (node, selector): a list to walk + facet recorders found by normal bin
    int cand_list;  // recorder ids, ascending within each (node, selector)
    int crit_d;     // (n_cls x n_cls) critical angles asin(n[a]/n[c]) (+inf where n[a] >= n[c]) by refractive-index
                    // class, or -1 when the scene has too many distinct indices for the table
    int ccrit_d;    // same shape: the cosine below which pvt_acos(cosine) exceeds that angle (host-proven
                    // threshold, NaN where it could not be proven, -inf where there is no critical angle)
    int grid_d;     // the node grid of scenes with many nodes (-1 = none; GRID variants): {lo[3], hi[3], cell[3], 1/cell[3],
                    // guard, one word of {nx | ny << 8 | nz << 16 | 64-bit words per cell << 24 | odd << 28}}, then per
                    // cell the bit mask of the nodes filed under it (x fastest)
    int rot_d;      // rotation classes x RT doubles (every node has one; the identity's is only read by the Lambertian branch)
    int ncls_d;     // refractive-index classes x {n, RN(1/n)}; in scenes with index tables (KArgs::n_rtab) followed by
                    // n_cls x {where the class's table n(lambda) starts in the double blob, its points (0: scalar class)}
    int n_cls;      // refractive-index classes (side of the crit tables)
    int by_node;    // 1: a scene of few nodes -- index classes and recorder candidate blocks are numbered like the nodes, so the
                    // lanes index the tables by node without reading NI_NCLS / NI_CAND first (one dependent LDS read fewer
                    // in the surface branch and in the tally: the headline scene)
};

struct EmitOff {  // emitter blobs (global only; read once per photon)
    int wl_value, pos_param, dir_param, l2w, spec_x, spec_cdf;         // doubles
    int wl_type, wl_spec_start, wl_spec_n, pos_type, dir_type;        // int32
};

struct KArgs {
    const double* gd;   // scene double blob (HBM)
    const int* gi;      // scene int blob
    const double* ed;   // emitter blobs (may be null)
    const int* ei;
    const pvt::BvhNode* bvh;    // triangle meshes (null when the scene has none): stay in HBM/L2
    const pvt::MeshTri* tris;
    Lay lay;
    EmitOff eoff;
    int nd, ni;         // blob lengths
    int nd_lds, ni_lds; // (variants whose tables do not fit LDS) heads of the blobs that are staged all the same: everything
                        // but the spectra and their guide tables (0: nothing)
    int n_nodes, root, n_rec, total_bins, n_coat, n_ctab, n_rtab, n_lights;   // n_ctab: coating reflectivity tables,
                                                                               // n_rtab: refractive-index tables
    // rays in (null -> device emission)
    const double* pos;
    const double* dir;
    const double* wl;
    unsigned int n_rays;
    // Scattering coatings (include/pvtrace_hip.h, "Scattering coatings"): where the coating rows' lobe records start in the
    // int blob -- kCl words per row, behind everything else the blob holds and read from where the guide tables are read;
    // -1 = no coating has a lobe (UF_CLOBE off).  (It stands where the struct had four bytes of padding: no other member
    // moves and the argument block keeps its size.)
    int clobe_i;
    unsigned int* cursor;   // [0] ray cursor, [1] claim cursor of resumed photons, [2] photons parked; (PVT_STATS builds) [2..] u64 counters
    unsigned int* cursor_next;   // the block the NEXT launch on this stream will use: cleared by this launch (no memset
                                 // kernel between launches: a one-workgroup fill cannot start while persistent workgroups
                                 // hold every slot of the chip, and the launch behind it waits with it); null = leave alone
    unsigned long long seed;       // + ray_offset folded in by the host
    unsigned long long emit_seed;  // + nothing; global index added per ray
    unsigned long long ray_offset;
    int maxsteps, max_events, emit_method;
    // Photon event counters (see `hcount` in trace_body): 0 = the scene counts nothing (UF_COUNT off); 1 = every photon
    // carries its counters -- a recorder is captured, a histogram reads one; 2 = moreover a histogram reads one, and queued
    // first crossings carry the packed word in one more column.  (It stands where the struct had four bytes of padding:
    // no other member moves and the argument block keeps its size.)
    int count;
    long long record_every;
    // outputs
    long long* rec_distinct;
    long long* rec_crossings;
    double* rec_sums;
    long long* rec_bins;
    // event log of the recorded rays: one 128-byte RECORD per event (see log_row), record of event k of recorded
    // ray j at row j*max_events + k; log_counts[j] = events written.  The reference's column arrays are made from
    // these by unpack_log_kernel.
    unsigned long long* log_rows;
    int* log_counts;
    // tally sets (0 = the launch is one bundle): rays [j*set_size, (j+1)*set_size) are bundle j of a stream of
    // equal bundles; a workgroup serves ONE set (its own ray cursor, its own slice of the tally arrays)
    unsigned int set_size;
    int wgs_per_set;
    long long set_stride_i, set_stride_d;   // elements between consecutive sets in rec_distinct/crossings/bins and rec_sums
    // The root is visited LAST and only by the lanes that need its exact distance (0 = off; 1 = box root,
    // 2 = sphere root, `lazy_k` = 1/(2 radius)); see the node loop
    int lazy_root;
    // Absorbing coatings (pvt_scene_create_absorb): where the coating rows' absorptivity records (kCa*) and tables start in
    // the double blob, read from where the spectra are read; -1 = no coating absorbs (UF_CABS off).  (It and `dcand_i`
    // below stand where the struct had four bytes of padding: no other member moves and the argument block keeps its size.)
    int cabs_d;
    double lazy_k;
    // 1: the scene is one unrotated box inside a lazy root with an empty, unobserved medium; a photon that leaves
    // the box's surface outwards, provably clear of it, is finished (see the surface branch)
    int fuse_exit;
    int bins_in_lds;
    int xslots;   // photon-state slots in LDS for drain-phase consolidation (0 = off)
    int tq_pos;   // 1: a histogram reads x, y or z -- queued first crossings carry the local position too
    // Photons carried from launch to launch of a stream of bundles (tally launches; PVT_FLAG_CARRY_OUT): a wave
    // that finds the ray cursor dry PARKS its live photons -- complete state, one record of kCarryStride u64 words
    // per photon -- in `carry_out` (count in cursor[2], one atomic per wave) and retires; the next
    // launch on the stream hands them to its lanes first (`carry_in`, count `*carry_in_count`, claimed through
    // cursor[1]) before it touches its own rays.  A launch then has no drain phase: the low-occupancy iterations at
    // the end of every bundle (a fifth of all wave-iterations of a 10^6-photon launch) run once per JOB.
    unsigned long long* carry_in;
    unsigned long long* carry_out;
    const unsigned int* carry_in_count;
    unsigned int carry_cap;
    int carry_flags;   // 1: resume parked photons first   2: park at exhaustion
    unsigned long long* timeline;   // (PVT_TIMELINE builds) 8 words per wave
    // Device emission (EMIT variants): a wave samples the 64 rays of a chunk when it CLAIMS the chunk -- every lane busy,
    // and the sampler's code (a fifth of the kernel's text) out of the step loop -- and parks them in its own
    // [7][64] doubles here (position, direction, wavelength; global memory, L2-resident); refilled lanes read theirs.
    double* emit_pool;
    // Mesh walks: byte offset in LDS of the workgroup's [kMeshQ][kBlock] words of noted leaves (-1: none)
    int meshq_off;
    // Mesh walks: the TOP of every tree (pvt_bvh.h: stage_top) is copied to LDS when a launch starts -- `top_n` records
    // from `bvh_top` to byte offset `top_off`; cursors with pvt::kTopFlag set index that copy
    int top_off, top_n;
    // Absorbing coatings: where the candidate tables of the PVT_RECX_DETECTED selector start in the int blob, behind the
    // guide tables and read from where those are read; -1 with cabs_d
    int dcand_i;
    const pvt::BvhNode* bvh_top;
    // Step counters of the scene, always on (pvt_scene_counters): 64 rows (blockIdx & 63) of eight u64 words
    //   [0] wave-iterations: trips of the photon loop in which a wave stepped its lanes
    //   [1] lane-steps: live lanes summed over those trips = the reference's loop count `_kernel.pyx:655` summed over the
    //       photons, except for [2]
    //   [2] fused exits: photons finished one step early by the fused exit (their last, empty step is not run)
    //   [3] waves retired
    //   [4] shader-clock cycles and [5] 100 MHz ticks, summed over the workgroups' lives (see `stamp`)
    // Kept per LANE in three vector registers (the loop is short of scalar ones): one add per trip, one when a photon
    // ends (its own step count `count` is what is added), one in the fused exit; summed in LDS when a wave retires, four
    // atomics per workgroup.  null = off.
    unsigned long long* counters;
    // Clocks of the launch, always on, read on the GPU itself (a pair of HIP events also times whatever the HOST does between
    // recording them: a descheduled thread reads as kernel time).  Thread 0 of every workgroup reads the constant 100 MHz
    // clock (s_memrealtime) and the shader clock (s_memtime) when the workgroup has staged its tables, its last wave reads
    // them again when it leaves: rows [4] / [5] of `counters` sum the shader cycles / the 100 MHz ticks of the workgroups'
    // lives (their ratio is the shader clock the launches ran at), and `stamp` -- two words per HIP stream -- gets the
    // 100 MHz time at which workgroup 0 started (a plain store) and the latest at which a workgroup left (atomic max):
    // after the stream is synchronised, the GPU-side span of its last launch (pvt_scene_launch_span).  null = off.
    unsigned long long* stamp;
    // The tail function's own lazy root (same codes as `lazy_root`, which is 0 when somebody looks at where photons leave
    // the scene -- an event log, an `exit` recorder): there the root's crossing is skipped only when another crossing is known
    // to lie before it, and worked out exactly when it is the nearest one -- among a lone wave's few photons hardly ever.
    int lazy_tail;
    // Rough interfaces (pvt_scene_create_rough): where the nodes' GGX widths alpha start in the double blob, read from
    // where the spectra are read; -1 = no node is rough (UF_ROUGH off)
    int rough_d;
    // Concentration fields (pvt_scene_create_field): the field buffer in global memory -- fd[n] = where node n's lattice
    // record starts (-1: none), the records (kFr*), the value tables; null = no node carries a lattice (UF_FIELD off)
    const double* fd;
    // Volume maps (pvt_scene_create_maps): the map buffer in global memory -- md[n] = where node n's block starts (-1: no
    // map), the blocks (kMn*, kMr*); null = the scene has no map (UF_VMAP off).  The counts are the int64 slots behind the
    // recorders' bins: rec_bins[total_bins ...] of the lane's tally set
    const double* md;
    // Ray capture (pvt_scene_create_capture): cap_tab[2 r] = the rows recorder r may keep (0: not captured) and
    // cap_tab[2 r + 1] = its first row; null = no recorder of the scene is captured (UF_CAPTURE off).  cap_rows / cap_cursor:
    // the launch's row buffer (kCapWords u64 words per row, cap_total rows per tally set) and its cursors (n_rec int64 per
    // tally set, never reset by the kernel); null = this launch keeps no rows
    const long long* cap_tab;
    unsigned long long* cap_rows;
    unsigned long long* cap_cursor;
    long long cap_total;
    // Launch origin (pvt_scene_create_origin; see `origin_put` in trace_body): bit k = a histogram reads property
    // PVT_PROPX_ORIGIN_WAVELENGTH + k (0 = none: UF_ORIGIN off) -- queued first crossings carry one more column per bit --
    // and the launch's side store, [lanes of the launch][kOriginWords] doubles in global memory (null with origin == 0)
    int origin;
    // Patterned coatings (pvt_scene_create_pattern): where the pattern buffer pd starts, in doubles from `gd` -- it lies in
    // the double blob's allocation but BEYOND its `nd` elements, so no launch stages it in LDS: global memory alone.
    // pd[2 c] = where coating row c's pattern record starts (-1: the row has no pattern), pd[2 c + 1] != 0: the row covers
    // any normal; the records (kPr*); behind them the masks, one byte per cell; -1 = no row has a pattern or the flag
    // (UF_CPAT off).  (It stands where the struct had four bytes of padding: no other member moves and the argument block
    // keeps its size.)
    int pd_d;
    double* origin_store;
};
static_assert(offsetof(KArgs, clobe_i) % 8 == 4 && offsetof(KArgs, cursor) == offsetof(KArgs, clobe_i) + 4, "KArgs::clobe_i fills padding");
// Aligned components (PvtAlignTables) live in KArgs::fd: fd[n] of a node that holds one names a record like a lattice's whose
// kFrShape words are 0 (a lattice has >= 1 cell per axis) and whose kFrComp + k word names, for the node's k-th component,
// where in fd its record of kAl doubles starts (-1: the component is not aligned): kAlOn != 0, the director in the root's
// frame, the absorption order S_a, kAlEmit != 0 = the component's phase table is sampled about the director
// What the extension family's kernels are compiled for (trace_body's ROUGH): kExtOff the other families, kExtRough the
// family as it is for every scene without alignment, kExtAligned the same with the aligned components' code (UF_ALIGN),
// kExtPath that again with the walk of the path-length maps at the advance site (UF_PMAP; path_map_call) -- the family's
// fullest kernels: a scene with a path-length map runs them whether it has aligned components or not
enum { kExtOff = 0, kExtRough = 1, kExtAligned = 2, kExtPath = 3 };
enum { kAlOn = 0, kAlAxis = 1, kAlOrder = 4, kAlEmit = 5, kAl = 6 };
constexpr int kCapWords = 12;  // u64 words of a captured row (PvtCaptures): index, position, direction, wavelength, path, clock,
                               // source | recorder << 32, the photon's event counters (kCountBits each)
constexpr int kMeshQ = 8;    // leaves a lane notes before its triangles are tested
constexpr int kCarryBase = 14;     // u64 words of a parked photon before its seen-mask
constexpr int kCarryStride = 18;   // words per parked photon (room for the four-word mask of scenes with > 64 recorders)
constexpr int kCountWords = 2;     // ... more of a scene that counts (KArgs::count; a captured recorder makes it one): the photon's
                                   // global ray index (captures read it), then its event counters
constexpr int kOriginWords = 4;    // the launch origin of a photon: wavelength, x, y, z of its GENERATE row.  A scene that reads one
                                   // (KArgs::origin) moves them with the photon: kOriginWords more words per exchange-buffer slot
                                   // and per parked photon, BEHIND the ray index and the counters where the scene counts too
// How many u64 words a photon on the move takes: in a slot of the LDS exchange buffer and as a parked photon's record.  The
// kernel lays both out by these and the host sizes both by them (plan_lds, bind_carry); trace_body's PVT_PHOTON_PUT /
// PVT_PHOTON_GET say which word is what.
constexpr int xbuf_words(int seenw, bool record, bool counting, bool origin) {
    return kCarryBase + seenw + (record ? 1 : 0) + (counting ? kCountWords : 0) + (origin ? kOriginWords : 0);
}
constexpr int carry_words(bool counting, bool origin) { return (counting ? kCarryStride + kCountWords : kCarryStride) + (origin ? kOriginWords : 0); }
static_assert(xbuf_words(1, false, false, false) == 15 && xbuf_words(4, false, false, false) == 18 && xbuf_words(1, true, false, false) == 16 &&
              xbuf_words(4, true, true, true) == 25, "a buffer slot: 15 or 18 words, + 1 with a history, + 2 counting, + 4 with an origin");
static_assert(carry_words(false, false) == 18 && carry_words(true, false) == 20 && carry_words(false, true) == 22 && carry_words(true, true) == 24,
              "a parked photon: 18, 20, 22 or 24 words");
static_assert(kCarryBase + 4 <= kCarryStride, "a parked photon's record has room for the four-word mask");
// (trace_body works a record's length out flag by flag -- each flag read and turned into its words before the next is read:
// handed to carry_words together, the two reads move the scalar spills of the extension family's tally kernels -- so the
// terms it adds are held to the function here)
static_assert(carry_words(true, false) == kCarryStride + kCountWords && carry_words(false, true) == kCarryStride + kOriginWords &&
              carry_words(true, true) == kCarryStride + kCountWords + kOriginWords, "trace_body's record length is carry_words'");
constexpr int kCountBits = 20;   // one event counter in the packed word: emissions | scatterings << 20 | reflections << 40.  A step
                                 // writes at most ONE row of a counted kind (kCountRowsPerStep), so no counter passes `maxsteps`;
                                 // the host refuses a launch whose maxsteps could overflow a field: the loop never saturates
constexpr int kCountRowsPerStep = 1;

// ------------------------------------------------------------------ RNG
struct Rng {
    unsigned long long s0, s1, s2, s3;
};
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long& st) {
    st += 0x9E3779B97F4A7C15ull;
    unsigned long long z = st;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ void rng_seed(Rng& r, unsigned long long seed) {
    unsigned long long st = seed;
    r.s0 = splitmix64(st);
    r.s1 = splitmix64(st);
    r.s2 = splitmix64(st);
    r.s3 = splitmix64(st);
}
__device__ __forceinline__ double rng_uniform(Rng& r) {
    unsigned long long result = r.s0 + r.s3;
    unsigned long long t = r.s1 << 17;
    r.s2 ^= r.s0;
    r.s3 ^= r.s1;
    r.s1 ^= r.s2;
    r.s0 ^= r.s3;
    r.s2 ^= t;
    r.s3 = (r.s3 << 45) | (r.s3 >> 19);
    // (double)(result >> 11) * 2^-53, as the reference writes it, is exact at every step (a 53-bit integer,
    // then a power of two); so is this split into the top 32 and the next 21 bits, one conversion shorter
    const double hi = (double)(unsigned int)(result >> 32), lo = (double)(unsigned int)((unsigned int)result >> 11);
    return __builtin_fma(lo, 1.0 / 9007199254740992.0, hi * (1.0 / 4294967296.0));
}

// RN(1/x) for a finite normal x whose reciprocal is normal too: the compiler's IEEE division sequence
// (reciprocal estimate, two Newton steps, quotient, residual, final fused correction) without the operand
// scaling and the special-case fix-up that only matter outside that range -- same intermediate values, same
// result, four instructions fewer.  Zero, infinities and NaN come out as garbage (callers never use them).
// (div_normal and sqrt_normal, the same idea for quotients and square roots, stand in pvt_math.h: the range-proven
// functions there are built on them.)
__device__ __forceinline__ double sqrt1m2_normal(double c) { return sqrt_normal((1.0 - c) * (1.0 + c)); }   // pvt_sqrt1m2
__device__ __forceinline__ double rcp_normal(double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    return __builtin_fma(e, r, r);
}

// ------------------------------------------------------------ table access
// TAB_LDS (0 / 1 / 2): divergent reads come from global memory / from the LDS copy of the blobs / records and class
// tables from LDS (the heads of the blobs, KArgs::nd_lds) and the spectra with their guide tables -- too large to
// stage -- from global memory; uniform reads always come
// from the global blob so the compiler can use scalar loads.
// Read-only scene blobs viewed through the CONSTANT address space: a load whose
// address is wave-uniform then becomes an s_load through the scalar cache (SGPR result,
// no VGPR address arithmetic) instead of a 64-lane global_load of one address.  The
// blobs are never written while a trace kernel runs, which is what makes this legal.
typedef const __attribute__((address_space(4))) double* CDoubles;
typedef const __attribute__((address_space(4))) int* CInts;

template <int TAB_LDS>
struct Tables {
    CDoubles gd;
    CInts gi;
    const double* ld;  // LDS copies (TAB_LDS != 0)
    const int* li;
    const double* __restrict__ hd;
    const int* __restrict__ hi;
    __device__ __forceinline__ double du(int i) const { return gd[i]; }  // uniform index
    __device__ __forceinline__ int iu(int i) const { return gi[i]; }
    // per-lane index: records and class tables (dv / iv), spectra and their guide tables (sd / si)
    __device__ __forceinline__ double dv(int i) const { return TAB_LDS != 0 ? ld[i] : hd[i]; }
    __device__ __forceinline__ int iv(int i) const { return TAB_LDS != 0 ? li[i] : hi[i]; }
    __device__ __forceinline__ double sd(int i) const { return TAB_LDS == 1 ? ld[i] : hd[i]; }
    __device__ __forceinline__ int si(int i) const { return TAB_LDS == 1 ? li[i] : hi[i]; }
};

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ double dot3(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// RN(x / y) for a divisor known in advance, given z = RN(1/y) computed once on the host:
// five multiply-adds instead of the ~25-instruction IEEE division expansion.  q1 = RN(x z) is
// within 1.5 ulp of x/y; one residual correction (r = x - q y, exact up to a rounding that
// cannot matter at that magnitude) makes q2 the rounding of a value within 2^-52 ulp of x/y, hence
// a faithful quotient; Markstein's theorem (z correctly rounded, q faithful, residual by FMA)
// then makes the second correction EXACTLY RN(x/y).  Preconditions: y, z finite non-zero
// normal, x finite, no underflow of the quotient (durations, indices and bin coordinates are
// many orders of magnitude inside the normal range).  A zero x may come back with the other
// sign (every use adds it or truncates it).  `tests/test_gpu_parity.py` checks the sequence
// against the host's division on random and adversarial operands.
__device__ __forceinline__ double div_known(double x, double y, double z) {
    double q = x * z;
    double r = __builtin_fma(-q, y, x);
    q = __builtin_fma(r, z, q);
    r = __builtin_fma(-q, y, x);
    return __builtin_fma(r, z, q);
}
constexpr double kRcpCcm = 1.0 / kCcm;   // correctly rounded by the compiler

// np.interp-like clamped interpolation (_kernel.pyx:219-238).  The reference bisects the
// whole table for `lo` = the largest index with xs[lo] <= x; that index is unique, so any
// search that finds it gives identical results.  Here a host-built guide table (n buckets of
// equal width over [xs[0], xs[n-1]], entry b = largest i with xs[i] <= left edge of bucket b)
// brackets the answer to a bucket first, the bracket is VALIDATED against the table (falls
// back to the full range if rounding put x in a neighbouring bucket), and the same bisection
// runs inside the bracket: typically 0-1 steps instead of ~log2(n) dependent LDS reads.
// `w` (NaN = no): the abscissae are xs[0] + i*w bit for bit AND every interval has the bits
// of w (both checked by the host), so the reference's index is found by arithmetic — no table
// walk, no dependent LDS reads — and validated against the (computed) neighbours.  `yw` likewise for
// the ordinates (the inverse-CDF lookup returns wavelengths of an evenly spaced grid).
// `KIND` (the lean variants, whose host has proven it of every table of the scene): kInterpAny = decided here, per call, by
// `hist`, `w` and `yw`; kInterpEven = not a histogram, and w is a number unless n == 1 (a constant); kInterpByGuide = not
// a histogram, w NaN, and yw a number unless n == 1 (the inverse-CDF lookup of an emission table whose wavelengths are an
// even grid).  A known kind is the same path with its run-time tests and the other paths left out.
enum { kInterpAny = 0, kInterpEven, kInterpByGuide, kInterpNoHist };   // (kInterpNoHist: kInterpAny of a table that is no histogram)
enum { kLeanOff = 0, kLeanSearched, kLeanEven };   // trace_body's LEAN
template <int TAB_LDS, int KIND = kInterpAny>
__device__ __forceinline__ double interp_clamped(const Tables<TAB_LDS>& T, double x, int xs, int ys, int n,
                                                 int guide, double scale, int hist, double rcp,
                                                 double w = __builtin_nan(""), double yw = __builtin_nan("")) {
    auto end = [&](int i) { return T.sd(i); };
    if (n == 1) return end(ys);
    constexpr bool kAny = KIND == kInterpAny;   // (the generic variants: every test below stands where and as it always stood)
    // a table on a proven even grid (w, yw) is stored as its first value: the last one is computed, same bits
    constexpr bool kNoHist = KIND == kInterpNoHist;
    const bool even = KIND == kInterpEven || (kAny && !hist && w == w) || (kNoHist && w == w);
    const double x0 = end(xs), xl = even ? x0 + (double)(n - 1) * w : end(xs + n - 1);
    if (x <= x0) return end(ys);
    if ((kAny && hist) ? x > xl : x >= xl) return (KIND == kInterpByGuide || ((kAny || kNoHist) && yw == yw)) ? end(ys) + (double)(n - 1) * yw : end(ys + n - 1);  // step tables search x == xl (plateaus)
    if (even) {
        // the host has checked, with this very sequence of operations, that it lands on the reference's
        // bisection index for every x of the table (pvt_trace.hip: even_w)
        int i = (int)((x - x0) * rcp);   // in [0, n-1] for x0 < x < xl; n-1 (x a rounding below xl) is repaired below
        double xlo = x0 + (double)i * w, xhi = x0 + (double)(i + 1) * w;
        // the product is within an ulp or two of the true quotient: only an x within rounding of a grid point can
        // come out one interval off, and the wave skips the repair unless one of its lanes holds such an x
        if (__ballot(x < xlo || !(x < xhi)) != 0ull) {
            if (x < xlo) { i -= 1; xhi = xlo; xlo = x0 + (double)i * w; }
            else if (!(x < xhi)) { i += 1; xlo = xhi; xhi = x0 + (double)(i + 1) * w; }
        }
        const double ylo = T.sd(ys + i), yhi = T.sd(ys + i + 1);
        return ylo + div_known((yhi - ylo) * (x - xlo), xhi - xlo, rcp);
    }
    int b = (int)((x - x0) * scale);
    b = b < 0 ? 0 : (b > n - 2 ? n - 2 : b);
    int lo = T.si(guide + b), hi = T.si(guide + b + 1) + 1;
    if (hi > n - 1) hi = n - 1;
    // the abscissae travel with the indices, so nothing is re-read after the search
    double xlo = T.sd(xs + lo), xhi = T.sd(xs + hi);
    if (kAny && hist) {
        // histogram-sampled table (extension; Python Distribution's hist branch): the value of
        // the first abscissa >= x, i.e. ys[#{xs_i < x}] — same bracket, strict comparison
        if (!(xlo < x)) lo = 0;          // xs[0] < x is known here
        if (!(x <= xhi)) hi = n - 1;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (T.sd(xs + mid) < x) lo = mid; else hi = mid;
        }
        return T.sd(ys + hi);
    }
    if (__ballot(!(xlo <= x) || !(x < xhi)) != 0ull) {   // (rounding put some lane's x in a neighbouring bucket: rare)
        if (!(xlo <= x)) { lo = 0; xlo = x0; }
        if (!(x < xhi)) { hi = n - 1; xhi = xl; }
    }
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const double xm = T.sd(xs + mid);
        if (xm <= x) { lo = mid; xlo = xm; } else { hi = mid; xhi = xm; }
    }
    double ylo, yhi;
    if (KIND == kInterpByGuide || ((kAny || kNoHist) && yw == yw)) {   // ordinates of an evenly spaced grid: computed, same bits as the table's
        const double y0 = end(ys);
        ylo = y0 + (double)lo * yw; yhi = y0 + (double)hi * yw;
    } else {
        ylo = T.sd(ys + lo); yhi = T.sd(ys + hi);
    }
    if (xhi == xlo) return ylo;
    // evenly spaced abscissae (every interval has the same bits, checked by the host): the
    // divisor is known in advance, see div_known
    const double num = (yhi - ylo) * (x - xlo), width = xhi - xlo;
    return ylo + (rcp == rcp ? div_known(num, width, rcp) : num / width);
}
// Coating reflectivity tables (KI_T*; the Python ReflectivityTable.at is the same arithmetic): piecewise linear in the
// wavelength, then in the angle of incidence, clamped at both ends of each axis, each step a + t (b - a) so that a table
// holding a constant gives exactly that constant.  [lo, hi] brackets x (lo == hi at and beyond the ends, t = 0).
__device__ __forceinline__ void coat_bracket(const double* xs, int n, double x, int& lo, int& hi, double& t) {
    lo = 0; hi = 0; t = 0.0;
    if (!(x > xs[0])) return;
    if (!(x < xs[n - 1])) { lo = n - 1; hi = n - 1; return; }
    int a = 0, b = n - 1;   // xs[a] <= x < xs[b]
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (xs[m] <= x) a = m; else b = m;
    }
    const double xa = xs[a];
    lo = a; hi = b; t = (x - xa) / (xs[b] - xa);
}
// R at wavelength `wl` and incidence cosine `c1` of the table whose wavelengths (nw), angles in radians (na) and values
// (na x nw) start at `wls`, `angs`, `vals` (LDS or global memory); the angle is pvt_acos(c1), the arc cosine the
// recorders' `angle` property uses
__device__ __forceinline__ double coat_table_r(const double* wls, int nw, const double* angs, int na, const double* vals,
                                               double wl, double c1) {
    int w0, w1, a0, a1;
    double tw, ta;
    coat_bracket(wls, nw, wl, w0, w1, tw);
    coat_bracket(angs, na, pvt_acos(c1), a0, a1, ta);
    const double* v0 = vals + a0 * nw;
    const double* v1 = vals + a1 * nw;
    const double p0 = v0[w0], r0 = p0 + tw * (v0[w1] - p0);
    const double p1 = v1[w0], r1 = p1 + tw * (v1[w1] - p1);
    return r0 + ta * (r1 - r0);
}
// The same as a FUNCTION, for the kernels of mesh scenes: inlined there, the lookup costs their history variants some
// eighty more spilled registers (it costs the kernels of analytic scenes none, so they inline it).
__device__ __attribute__((noinline)) double coat_table_r_call(const double* wls, int nw, const double* angs, int na,
                                                              const double* vals, double wl, double c1) {
    return coat_table_r(wls, nw, angs, na, vals, wl, c1);
}

// Absorbing coatings (PvtCoatingAbsorbTables; the Python Coating docstring states the rule): A of coating row `coat` at
// wavelength `wl` and incidence cosine `c1` -- the row's scalar, or its table walked as coat_table_r walks a reflectivity
// table.  `tab` is the blob the spectra are read from, `recs` the rows' records (kCa*) in it.  A FUNCTION, like
// rough_event_call: inlined, the table walk would live in the step loop of every extension variant.
__device__ __attribute__((noinline)) double coat_absorb_call(const double* tab, const double* recs, int coat, double wl, double c1) {
    const double* r = recs + coat * kCa;
    const int nw = (int)r[kCaNw];
    if (nw == 0) return r[kCaA];
    const int na = (int)r[kCaNa];
    const double* wls = tab + (int)r[kCaTab];
    return coat_table_r(wls, nw, wls + nw, na, wls + nw + na, wl, c1);
}

// Patterned coatings (PvtCoatingPatternTables; the Python Coating docstring states the rule, pattern_cell is the same
// arithmetic): does coating row `c`, whose region holds the local point (lx, ly, lz), cover it?  `facet_ok`: the row's
// normal test passed -- the row's any-facet flag pd[2 c + 1] overrules a failed one.  A row without a pattern
// (pd[2 c] < 0) then covers; else per bounded axis floor((p - lower) / h) must lie in 0 .. n - 1, or the point is outside
// and not covered (a NaN coordinate fails every comparison), and ONE byte load from global memory answers, slot
// (ix ny + iy) nz + iz.  A FUNCTION, like coat_absorb_call: the coating loop's register allocation does not see it.
__device__ __attribute__((noinline)) int coat_pattern_call(const double* __restrict__ pd, int c, int facet_ok, double lx, double ly,
                                                           double lz) {
    if (!facet_ok && pd[2 * c + 1] == 0.0) return 0;
    const int at = (int)pd[2 * c];
    if (at < 0) return 1;
    const double* __restrict__ q = pd + at;
    double fx = 0.0, fy = 0.0, fz = 0.0;
    if (q[kPrBounded] != 0.0) fx = __builtin_floor((lx - q[kPrLower]) / q[kPrH]);
    if (q[kPrBounded + 1] != 0.0) fy = __builtin_floor((ly - q[kPrLower + 1]) / q[kPrH + 1]);
    if (q[kPrBounded + 2] != 0.0) fz = __builtin_floor((lz - q[kPrLower + 2]) / q[kPrH + 2]);
    const double nx = q[kPrShape], ny = q[kPrShape + 1], nz = q[kPrShape + 2];
    const bool inside = fx >= 0.0 && fx <= nx - 1.0 && fy >= 0.0 && fy <= ny - 1.0 && fz >= 0.0 && fz <= nz - 1.0;
    if (!inside) return 0;
    const long long slot = ((long long)fx * (long long)ny + (long long)fy) * (long long)nz + (long long)fz;
    return reinterpret_cast<const unsigned char*>(pd)[(long long)q[kPrMask] + slot] != 0 ? 1 : 0;
}

// Refractive-index tables n(lambda) (the Python RefractiveIndexTable.at is the same arithmetic): `np` wavelengths, then
// `np` indices, from `xs` (LDS or global memory); piecewise linear, clamped at both ends, a + t (b - a)
__device__ __forceinline__ double index_table_n(const double* xs, int np, double wl) {
    int lo, hi;
    double t;
    coat_bracket(xs, np, wl, lo, hi, t);
    const double a = xs[np + lo];
    return a + t * (xs[np + hi] - a);
}
// The whole lookup of a node of index class k as a FUNCTION: `recs` points at the classes' {table offset, points}
// records, `tab` at the blob the tables are read from.  Inlined at its three sites, the lookup (never taken there: the
// flag is off) put 1.5 KB into the step loop of the headline scene and cost it 1.3 % of its throughput; called, the
// sites add 0.5 KB and the throughput is the parent's within the noise of an alternating A/B.  (The 256-recorder
// tally variants inline it: with a call one of their vector registers goes to scratch.)
__device__ __attribute__((noinline)) double index_class_n_call(const double* recs, const double* tab, int k, double n, double wl) {
    const int np = (int)recs[2 * k + 1];
    if (np == 0) return n;
    return index_table_n(tab + (int)recs[2 * k], np, wl);
}

// Tabulated phase functions (PVT_PHASE_TABLE; include/pvtrace_hip.h states the contract, the Python
// PhaseFunctionTable samples the same way): the new direction about the incoming one `d` from the draws u1 (the row;
// read only when the table has several), u2 (the polar cosine) and u3 (the azimuth).  `tab` is the table's record in
// the blob the spectra are read from: {n_wavelength, n_mu}, the wavelengths, the mu axis, the CDF rows.  A FUNCTION,
// entered only by lanes whose component has a table, so the scenes without one keep the step loop they had; the
// 256-recorder variants of analytic scenes inline it instead (with a call one of their vector registers goes to scratch).
__device__ __forceinline__ V3 phase_table_turn(const double* tab, double wl, double u1, double u2, double u3,
                                               double dx, double dy, double dz) {
    const int nw = (int)tab[0], nm = (int)tab[1];
    const double* mus = tab + 2 + nw;
    const double* cdf = mus + nm;
    if (nw > 1) {   // row k + 1 with probability t, else row k (t = 0 at and beyond the ends)
        int lo, hi;
        double t;
        coat_bracket(tab + 2, nw, wl, lo, hi, t);
        cdf += (u1 < t ? hi : lo) * nm;
    }
    int a = 0, b = nm - 1;   // cdf[a] <= u2 < cdf[b]: cdf[0] = 0 <= u2 < 1 = cdf[nm - 1]
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (cdf[m] <= u2) a = m; else b = m;
    }
    const double ca = cdf[a], ma = mus[a];
    double mu = ma + (u2 - ca) / (cdf[b] - ca) * (mus[b] - ma);
    mu = __builtin_fmin(__builtin_fmax(mu, -1.0), 1.0);
    const double st = sqrt1m2_normal(mu);
    double sp, cp;
    pvt_sincos2pi(u3, &sp, &cp);
    // the orthonormal basis about d of Duff et al. 2017, branch-free
    const double s = __builtin_copysign(1.0, dz);
    const double ra = -1.0 / (s + dz);
    const double rb = dx * dy * ra;
    const V3 e1{1.0 + s * dx * dx * ra, s * rb, -s * dx};
    const V3 e2{rb, s + dy * dy * ra, -dy};
    return V3{mu * dx + st * (cp * e1.x + sp * e2.x), mu * dy + st * (cp * e1.y + sp * e2.y),
              mu * dz + st * (cp * e1.z + sp * e2.z)};
}
__device__ __attribute__((noinline)) V3 phase_table_turn_call(const double* tab, double wl, double u1, double u2, double u3,
                                                              double dx, double dy, double dz) {
    return phase_table_turn(tab, wl, u1, u2, u3, dx, dy, dz);
}

// Scattering coatings (include/pvtrace_hip.h, "Scattering coatings"; the Python ScatterLobe states the same rule): the
// direction of a photon that a lobe coating has just reflected or transmitted.  `tab` is the lobe's phase table in the
// blob the spectra are read from; (ax, ay, az) is what the built-in body of the row's stand-in mode has left in `dir` --
// the specular direction, the Snell direction, or d itself -- and the axis unless `normal_axis`, when N_out = (nx, ny, nz)
// is (rule 3); u1 (drawn by the caller only when the table has several rows), u2, u3 are rule 4's draws; the fold of
// rule 5 is applied here.  A FUNCTION, called only from the trace_kernel_rough* variants, and there only by the lanes of
// a scene with a lobe (UF_CLOBE) that stand on a lobe row.
__device__ __attribute__((noinline)) V3 coat_lobe_call(const double* tab, int normal_axis, double wl, double u1, double u2, double u3,
                                                        double ax, double ay, double az, double nx, double ny, double nz) {
    if (normal_axis) { ax = nx; ay = ny; az = nz; }
    V3 o = phase_table_turn(tab, wl, u1, u2, u3, ax, ay, az);
    const double t = (o.x * nx + o.y * ny) + o.z * nz;
    if (t < 0.0) {
        const double t2 = 2.0 * t;
        o = V3{o.x - t2 * nx, o.y - t2 * ny, o.z - t2 * nz};
    }
    return o;
}

// Truncated cones (PVT_GEOM_FRUSTUM; include/pvtrace_hip.h states the arithmetic, geometry.Frustum performs the same
// operations in the same order): the four candidate distances of the ray (o, d) in the node's frame, in fold order -- side
// root, side root, -z cap, +z cap -- a candidate that is no crossing being 0 (never > kEps).  With r0 == r1 every
// intermediate of the general branch is the capped cylinder's.  A FUNCTION, called only from the trace_kernel_rough*
// variants: the plain families carry none of it.
struct FrustumHits { double t[4]; };
__device__ __forceinline__ FrustumHits frustum_hits(double length, double r0, double r1, double ox, double oy, double oz,
                                                    double dx, double dy, double dz) {
    FrustumHits h{{0.0, 0.0, 0.0, 0.0}};
    const double half = 0.5 * length, rm = 0.5 * (r0 + r1), k = (r1 - r0) / length;
    const double e = rm + k * oz, f = k * dz, s = dx * dx + dy * dy;
    const double ff = f * f;
    const double a = s - ff;
    const double b = 2.0 * ((ox * dx + oy * dy) - e * f);
    const double c = (ox * ox + oy * oy) - e * e;
    const double disc = b * b - 4.0 * a * c;
    if (disc >= 0.0) {
        const double sq = pvt_sqrt(disc);
        double ta = 0.0, tb = 0.0;
        bool has_a = true, has_b = true;
        if (pvt_fabs(a) > 0x1p-20 * (s + ff)) {
            ta = (-b - sq) / (2.0 * a);
            tb = (-b + sq) / (2.0 * a);
        } else {   // the ray runs nearly along a generator: the roots without the cancellation
            const double q = -0.5 * (b + __builtin_copysign(sq, b));
            has_a = q != 0.0;
            has_b = pvt_fabs(a) > 1e-300;
            if (has_a) ta = c / q;
            if (has_b) tb = q / a;
        }
        double z = oz + ta * dz;
        if (has_a && z > -half && z < half) h.t[0] = ta;
        z = oz + tb * dz;
        if (has_b && z > -half && z < half) h.t[1] = tb;
    }
    if (pvt_fabs(dz) > 1e-300) {
        double t = (-half - oz) / dz;
        double x = ox + t * dx, y = oy + t * dy;
        if (x * x + y * y <= r0 * r0) h.t[2] = t;
        t = (half - oz) / dz;
        x = ox + t * dx;
        y = oy + t * dy;
        if (x * x + y * y <= r1 * r1) h.t[3] = t;
    }
    return h;
}
// ... and the outward normal at the point p of its surface: the cylinder's cap rule, then the gradient of the side
__device__ __forceinline__ V3 frustum_normal(double length, double r0, double r1, double px, double py, double pz) {
    const double half = 0.5 * length;
    const double tol = 1e-8 + 1e-5 * pvt_fabs(half);
    if (pvt_fabs(pz + half) <= tol) return V3{0.0, 0.0, -1.0};
    if (pvt_fabs(pz - half) <= tol) return V3{0.0, 0.0, 1.0};
    const double rm = 0.5 * (r0 + r1), k = (r1 - r0) / length;
    const double rz = rm + k * pz;
    const double w = k * rz;
    const double m = pvt_sqrt((px * px + py * py) + w * w);
    return V3{px / m, py / m, (-w) / m};
}

// Convex polyhedra (PVT_GEOM_POLYHEDRON; include/pvtrace_hip.h states the rule, geometry.Polyhedron performs the same
// operations in the same order): the two candidate distances of the ray (o, d) in the node's frame -- entry, then exit -- a
// candidate that is no crossing being 0 (never > kEps), as in FrustumHits.  `planes`: the node's `count` rows (nx, ny, nz, h)
// in the double blob, global memory.  In the node loop the node is the wave's, so the rows sit at a wave-uniform address
// and come through the scalar cache, 32 bytes a row; the loop's state is tin, tout and miss.  One IEEE division per plane
// is the price of agreeing with the host bit for bit.  FUNCTIONS, called only from the trace_kernel_rough* variants: the
// plain families carry none of it.
struct PolyhedronHits { double t[2]; };
__device__ __attribute__((noinline)) PolyhedronHits polyhedron_hits_call(CDoubles planes, int count, double ox, double oy, double oz,
                                                                         double dx, double dy, double dz) {
    // (a function's arguments arrive in vector registers; the node is the wave's, so the rows' address and their count are
    // the same in every lane: said here, the rows come through the scalar cache and the loop is the wave's, not the lanes')
    const unsigned long long addr = (unsigned long long)planes;
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)addr);
    const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(addr >> 32));
    const CDoubles rows = (CDoubles)(((unsigned long long)hi << 32) | (unsigned long long)lo);
    const int n = __builtin_amdgcn_readfirstlane(count);
    double tin = -INFINITY, tout = INFINITY;
    bool miss = false;
    for (int k = 0; k < n; k++) {
        const double nx = rows[4 * k], ny = rows[4 * k + 1], nz = rows[4 * k + 2], h = rows[4 * k + 3];
        const double den = (nx * dx + ny * dy) + nz * dz;
        const double num = h - ((nx * ox + ny * oy) + nz * oz);
        if (pvt_fabs(den) < 1e-300) {
            if (num < 0.0) miss = true;
            continue;
        }
        const double t = num / den;
        if (den < 0.0) tin = __builtin_fmax(tin, t);
        else tout = __builtin_fmin(tout, t);
    }
    PolyhedronHits hits{{0.0, 0.0}};
    if (!miss && !(tout < tin)) {
        if (pvt_fabs(tin) < INFINITY) hits.t[0] = tin;
        if (pvt_fabs(tout) < INFINITY) hits.t[1] = tout;
    }
    return hits;
}
// ... and the outward normal at the point p of its surface: the row nearest to p, the first of equals; here the node is
// the lane's own, so are the rows
__device__ __attribute__((noinline)) V3 polyhedron_normal_call(const double* planes, int count, double px, double py, double pz) {
    double best = INFINITY;
    V3 n{0.0, 0.0, 0.0};
    for (int k = 0; k < count; k++) {
        const double nx = planes[4 * k], ny = planes[4 * k + 1], nz = planes[4 * k + 2], h = planes[4 * k + 3];
        const double dist = pvt_fabs(((nx * px + ny * py) + nz * pz) - h);
        if (dist < best) { best = dist; n = V3{nx, ny, nz}; }
    }
    return n;
}

// Solids of revolution of a conic (PVT_GEOM_CONICOID; include/pvtrace_hip.h states the arithmetic, geometry.Conicoid
// performs the same operations in the same order): the four candidate distances of the ray (o, d) in the node's frame, in
// fold order -- root, root, -z cap, +z cap -- a candidate that is no crossing being 0 (never > kEps), as FrustumHits.  ONE
// branch, always the roots without the cancellation: a near-paraxial ray onto a paraboloid has a -> 0.  An end where q is
// within 2^-40 S of zero is a pole and has no cap.  FUNCTIONS, called only from the trace_kernel_rough* variants: the plain
// families carry none of it.
__device__ __forceinline__ FrustumHits conicoid_hits(double length, double p0, double p1, double p2, double ox, double oy,
                                                     double oz, double dx, double dy, double dz) {
    FrustumHits h{{0.0, 0.0, 0.0, 0.0}};
    const double half = 0.5 * length, g = 0.5 * p1 + p2 * oz, s = dx * dx + dy * dy;
    const double a = s - (p2 * dz) * dz;
    const double b = 2.0 * ((ox * dx + oy * dy) - g * dz);
    const double c = (ox * ox + oy * oy) - (p0 + (p1 + p2 * oz) * oz);
    const double disc = b * b - 4.0 * a * c;
    if (disc >= 0.0) {
        const double sq = pvt_sqrt(disc);
        const double qq = -0.5 * (b + __builtin_copysign(sq, b));
        const bool has_a = qq != 0.0, has_b = pvt_fabs(a) > 1e-300;
        double ta = 0.0, tb = 0.0;
        if (has_a) ta = c / qq;
        if (has_b) tb = qq / a;
        double z = oz + ta * dz;
        if (has_a && z > -half && z < half) h.t[0] = ta;
        z = oz + tb * dz;
        if (has_b && z > -half && z < half) h.t[1] = tb;
    }
    if (pvt_fabs(dz) > 1e-300) {
        const double slack = 0x1p-40 * ((pvt_fabs(p0) + pvt_fabs(p1) * half) + (pvt_fabs(p2) * half) * half);
        const double q_lo = p0 + (p1 + p2 * (-half)) * (-half), q_hi = p0 + (p1 + p2 * half) * half;
        if (!(q_lo <= slack)) {
            const double t = (-half - oz) / dz;
            const double x = ox + t * dx, y = oy + t * dy;
            if (x * x + y * y <= q_lo) h.t[2] = t;
        }
        if (!(q_hi <= slack)) {
            const double t = (half - oz) / dz;
            const double x = ox + t * dx, y = oy + t * dy;
            if (x * x + y * y <= q_hi) h.t[3] = t;
        }
    }
    return h;
}
// ... and the outward normal at the point p of its surface: the cap rule at an end that is no pole, then the gradient
__device__ __forceinline__ V3 conicoid_normal(double length, double p0, double p1, double p2, double px, double py, double pz) {
    const double half = 0.5 * length;
    const double tol = 1e-8 + 1e-5 * pvt_fabs(half);
    const double slack = 0x1p-40 * ((pvt_fabs(p0) + pvt_fabs(p1) * half) + (pvt_fabs(p2) * half) * half);
    const double q_lo = p0 + (p1 + p2 * (-half)) * (-half), q_hi = p0 + (p1 + p2 * half) * half;
    if (!(q_lo <= slack) && pvt_fabs(pz + half) <= tol) return V3{0.0, 0.0, -1.0};
    if (!(q_hi <= slack) && pvt_fabs(pz - half) <= tol) return V3{0.0, 0.0, 1.0};
    const double w = 0.5 * p1 + p2 * pz;
    const double m = pvt_sqrt((px * px + py * py) + w * w);
    return V3{px / m, py / m, (-w) / m};
}

// The ONE pair of out-of-line entries of the two quadrics of revolution, so that the step loop of the trace_kernel_rough*
// variants holds one call in the node loop and one at the normal site for both shapes, as it did for the truncated cone
// alone: (g0, g1, g2, g3) = (L, r0, r1, NaN) of a truncated cone, (L, p0, p1, p2) of a conicoid -- no conicoid has a NaN, the
// packer refuses it.  In the node loop the node is the wave's, so is the shape: the function says so (a function's
// arguments arrive in vector registers) and branches on the first active lane's word, a scalar branch.
__device__ __attribute__((noinline)) FrustumHits quadric_hits_call(double g0, double g1, double g2, double g3, double ox, double oy,
                                                                   double oz, double dx, double dy, double dz) {
    const unsigned int top = __builtin_amdgcn_readfirstlane((unsigned int)(pvt_d2u(g3) >> 32));
    if ((top & 0x7ff00000u) == 0x7ff00000u) return frustum_hits(g0, g1, g2, ox, oy, oz, dx, dy, dz);
    return conicoid_hits(g0, g1, g2, g3, ox, oy, oz, dx, dy, dz);
}
// ... and the normal: here the hit node is the lane's own, so is the branch
__device__ __attribute__((noinline)) V3 quadric_normal_call(double g0, double g1, double g2, double g3, double px, double py, double pz) {
    if (g3 != g3) return frustum_normal(g0, g1, g2, px, py, pz);
    return conicoid_normal(g0, g1, g2, g3, px, py, pz);
}

// Rough interfaces (PvtSurfaceTables; include/pvtrace_hip.h states the contract, the Python FresnelSurfaceDelegate samples
// the same way): one surface event of a lane whose hit node is rough where no coating covers it (UF_ROUGH) -- the draws
// u_a, u_b, the microfacet normal m from the GGX distribution of visible normals of width `alpha` (Heitz 2018) about the
// geometric normal `n` (either orientation) facing the photon, Fresnel about m, the draw u when R > 0, the reflected or
// refracted direction about m and the fold.  The photon's random stream goes in and comes back by value (a reference
// would put it in scratch).  A FUNCTION, called only from the trace_kernel_rough* variants.
struct RoughEvent {
    double dx, dy, dz;                   // the new direction
    unsigned long long s0, s1, s2, s3;   // the photon's random stream after the event's draws
    int reflect;                         // 1: REFLECT, 0: TRANSMIT
};
__device__ __attribute__((noinline)) RoughEvent rough_event_call(double alpha, double nx, double ny, double nz, double dx, double dy,
                                                        double dz, double n1, double n2, unsigned long long s0,
                                                        unsigned long long s1, unsigned long long s2, unsigned long long s3) {
    Rng rng{s0, s1, s2, s3};
    const double ua = rng_uniform(rng);
    const double ub = rng_uniform(rng);
    // N: the geometric normal facing the photon (d.N < 0); (e1, e2) the basis of Duff et al. 2017 about it
    const double o = nx * dx + ny * dy + nz * dz > 0.0 ? -1.0 : 1.0;
    const V3 N{o * nx, o * ny, o * nz};
    const double s = __builtin_copysign(1.0, N.z);
    const double ra = -1.0 / (s + N.z);
    const double rb = N.x * N.y * ra;
    const V3 e1{1.0 + s * N.x * N.x * ra, s * rb, -s * N.x};
    const V3 e2{rb, s + N.y * N.y * ra, -N.y};
    const V3 d{dx, dy, dz};
    // v = -d in the frame, stretched by alpha: the hemisphere configuration
    double hx = -alpha * dot3(d, e1), hy = -alpha * dot3(d, e2), hz = -dot3(d, N);
    double il = 1.0 / pvt_sqrt(hx * hx + hy * hy + hz * hz);
    hx *= il; hy *= il; hz *= il;
    const double lensq = hx * hx + hy * hy;
    double t1x = 1.0, t1y = 0.0;
    if (lensq > 0.0) {
        const double it = 1.0 / pvt_sqrt(lensq);
        t1x = -hy * it;
        t1y = hx * it;
    }
    const double t2x = -hz * t1y, t2y = hz * t1x, t2z = hx * t1y - hy * t1x;   // Vh x T1 (T1.z = 0)
    const double r = pvt_sqrt(ua);
    double sp, cp;
    pvt_sincos2pi(ub, &sp, &cp);
    const double t1 = r * cp, sw = 0.5 * (1.0 + hz);
    const double t2 = (1.0 - sw) * pvt_sqrt(__builtin_fmax(0.0, 1.0 - t1 * t1)) + sw * r * sp;
    const double tz = pvt_sqrt(__builtin_fmax(0.0, 1.0 - t1 * t1 - t2 * t2));
    double lx = alpha * (t1 * t1x + t2 * t2x + tz * hx), ly = alpha * (t1 * t1y + t2 * t2y + tz * hy);
    double lz = __builtin_fmax(0.0, t2 * t2z + tz * hz);
    il = 1.0 / pvt_sqrt(lx * lx + ly * ly + lz * lz);
    lx *= il; ly *= il; lz *= il;
    const V3 m{lx * e1.x + ly * e2.x + lz * N.x, lx * e1.y + ly * e2.y + lz * N.y, lx * e1.z + ly * e2.z + lz * N.z};
    // Fresnel about m (the smooth branch's Hecht formula), 1 under total internal reflection about m
    const double dm = dot3(d, m);   // -(v.m)
    const double c = __builtin_fmin(__builtin_fmax(-dm, 0.0), 1.0);
    const double q = n1 / n2 * pvt_sqrt((1.0 - c) * (1.0 + c));
    double R = 1.0;
    if (q < 1.0) {
        const double k = pvt_sqrt(1.0 - q * q);
        const double as = (n1 * c - n2 * k) / (n1 * c + n2 * k), ap = (n1 * k - n2 * c) / (n1 * k + n2 * c);
        R = 0.5 * (as * as + ap * ap);
    }
    double u = 1.0;
    if (R > 0.0) u = rng_uniform(rng);
    RoughEvent e;
    e.reflect = u < R ? 1 : 0;
    V3 t;
    if (e.reflect) {
        t = V3{dx - 2.0 * dm * m.x, dy - 2.0 * dm * m.y, dz - 2.0 * dm * m.z};
    } else {   // Snell, vector form, about -m (the microfacet normal along the ray)
        const double n = n1 / n2;
        const double k = pvt_sqrt(__builtin_fmax(0.0, 1.0 - n * n * (1.0 - c * c))) - n * c;
        t = V3{n * dx - k * m.x, n * dy - k * m.y, n * dz - k * m.z};
    }
    // fold: back across the tangent plane when on the wrong side of the geometric normal (N faces the photon)
    const double tn = dot3(t, N);
    if (e.reflect ? tn < 0.0 : tn > 0.0) t = V3{t.x - 2.0 * tn * N.x, t.y - 2.0 * tn * N.y, t.z - 2.0 * tn * N.z};
    e.dx = t.x; e.dy = t.y; e.dz = t.z;
    e.s0 = rng.s0; e.s1 = rng.s1; e.s2 = rng.s2; e.s3 = rng.s3;
    return e;
}

// Aligned components (PvtAlignTables; include/pvtrace_hip.h states the rule, the Python Alignment follows the same): the
// factor f = 1.0 - S (1.5 (mu mu) - 0.5) of the component whose record is `r`, mu = (dx nx + dy ny) + dz nz clamped to
// [-1, 1] -- these operations in this order (the build has no FMA contraction).
__device__ __forceinline__ double align_factor(const double* __restrict__ r, double dx, double dy, double dz) {
    double mu = (dx * r[kAlAxis] + dy * r[kAlAxis + 1]) + dz * r[kAlAxis + 2];
    mu = __builtin_fmin(__builtin_fmax(mu, -1.0), 1.0);
    return 1.0 - r[kAlOrder] * (1.5 * (mu * mu) - 0.5);
}
// The scaled coefficients of a lane whose container holds an aligned component (`r`: the container's record in fd):
// sum_k alpha_k(wl) f_k in component order and its first partial sum, for the depth and the component pick.  The
// coefficients are looked up as the caller looks them up (ci0 / cd0: the records of the node's first component); a
// component without alignment is not multiplied, and orders of 0 give f = 1.0 exactly, so such a container gets the
// caller's sums bit for bit.  A FUNCTION, called only from field_march_call, which the trace_kernel_rough* variants call.
struct AlignScale {
    double alpha;   // sum_k alpha_k f_k
    double pre0;    // alpha_0 f_0
};
template <int TAB_LDS>
__device__ __attribute__((noinline)) AlignScale align_scale_call(Tables<TAB_LDS> T, const double* __restrict__ fd, const double* __restrict__ r,
                                                                 int ci0, int cd0, int ccount, double wl, double dx, double dy, double dz) {
    double sum = 0.0, p0 = 0.0;
    for (int k = 0; k < ccount; k++) {
        const int ci = ci0 + k * CI, cd = cd0 + k * CD;
        double term = interp_clamped<TAB_LDS>(T, wl, T.iv(ci + CI_ABS_X), T.iv(ci + CI_ABS_Y), T.iv(ci + CI_ABS_N), T.iv(ci + CI_ABS_G),
                                              T.dv(cd + CD_ABS_SCALE), T.iv(ci + CI_ABS_HIST), T.dv(cd + CD_ABS_RCP), T.dv(cd + CD_ABS_W));
        const int at = (int)r[kFrComp + k];
        if (at >= 0) term = term * align_factor(fd + at, dx, dy, dz);
        sum += term;
        if (k == 0) p0 = sum;
    }
    return AlignScale{sum, p0};
}
// ... the pick's walk beyond two components, in a scene with aligned components (UF_ALIGN): `term` of the k-th component of
// the container whose record starts at fd + frec times its factor along the photon's direction, or, in a container with
// a lattice, times the cell's concentration as ever
__device__ __forceinline__ double align_term(const double* __restrict__ fd, int frec, int k, int fcell, double term, double dx, double dy,
                                             double dz) {
    const int at = (int)fd[frec + kFrComp + k];
    if (fd[frec + kFrShape] != 0.0) return term * fd[at + fcell];
    return at >= 0 ? term * align_factor(fd + at, dx, dy, dz) : term;
}
// ... and the emission: the axis the phase table of the k-th component of that container is sampled about -- its director
// when its record says so (kAlEmit), else what the caller holds (the incoming direction)
__device__ __forceinline__ void align_axis(const double* __restrict__ fd, int frec, int k, double& ax, double& ay, double& az) {
    if (frec < 0 || fd[frec + kFrShape] != 0.0) return;
    const int at = (int)fd[frec + kFrComp + k];
    if (at < 0 || fd[at + kAlEmit] == 0.0) return;
    ax = fd[at + kAlAxis]; ay = fd[at + kAlAxis + 1]; az = fd[at + kAlAxis + 2];
}

// Concentration fields (PvtFieldTables; include/pvtrace_hip.h states the contract, the Python ConcentrationGrid marches
// the same way): the free path of a lane whose container carries a lattice (UF_FIELD).  From the photon's position, cell
// by cell along its direction up to the surface distance t0, the optical depth sum alpha_cell * segment grows until it
// reaches tau* = `tau`; alpha_cell = sum_k alpha_k(wl) c_k[cell] in component order.  The node's world->local transform
// and lattice come from its record at fd + frec; the components' coefficients are looked up as the caller looks them up
// (ci0 / cd0: the records of the node's first component).  Returns where the photon is absorbed (INFINITY: it reaches
// the surface) and that cell's alpha_cell, first partial sum and index, for the component pick.  A 1 x 1 x 1 lattice of
// value 1 gives the caller's alpha and depth bit for bit.  A FUNCTION, called only from the trace_kernel_rough* variants.
struct FieldMarch {
    double depth;   // where the photon is absorbed, INFINITY = not before t0
    double alpha;   // alpha_cell of the cell it is absorbed in ...
    double pre0;    // ... the first partial sum of that cell's coefficients ...
    int cell;       // ... and the cell's index into the value tables
};
template <int TAB_LDS, bool ALIGNED>
__device__ __attribute__((noinline)) FieldMarch field_march_call(Tables<TAB_LDS> T, const double* __restrict__ fd, int frec, int ci0,
                                                                 int cd0, int ccount, double wl, double px, double py, double pz,
                                                                 double dx, double dy, double dz, double tau, double t0) {
    const double* __restrict__ r = fd + frec;
    if constexpr (ALIGNED) {   // (only the kExtAligned kernels' instantiation: the others call the function as it ever was)
        if (r[kFrShape] == 0.0) {
            // (PvtAlignTables) no lattice: a container with an aligned component.  The depth over the scaled sum, +inf when
            // that is exactly 0 (the general division below 1e-250, as in the march: a factor near its zero makes tiny sums)
            const AlignScale as = align_scale_call<TAB_LDS>(T, fd, r, ci0, cd0, ccount, wl, dx, dy, dz);
            const double d = as.alpha == 0.0 ? INFINITY : (as.alpha > 1e-250 ? div_normal(tau, as.alpha) : tau / as.alpha);
            return FieldMarch{d, as.alpha, as.pre0, 0};
        }
    }
    auto coef = [&](int k) -> double {
        const int ci = ci0 + k * CI, cd = cd0 + k * CD;
        return interp_clamped<TAB_LDS>(T, wl, T.iv(ci + CI_ABS_X), T.iv(ci + CI_ABS_Y), T.iv(ci + CI_ABS_N), T.iv(ci + CI_ABS_G),
                                       T.dv(cd + CD_ABS_SCALE), T.iv(ci + CI_ABS_HIST), T.dv(cd + CD_ABS_RCP), T.dv(cd + CD_ABS_W));
    };
    // the first two components' coefficients and value tables are held; further ones are looked up per cell
    const double a0 = ccount > 0 ? coef(0) : 0.0, a1 = ccount > 1 ? coef(1) : 0.0;
    const int v0 = ccount > 0 ? (int)r[kFrComp] : 0, v1 = ccount > 1 ? (int)r[kFrComp + 1] : 0;
    // one axis of the lattice in the node's frame: the photon's coordinate and direction, the cell it starts in (clamped
    // into the lattice) and the distance to the next interior plane ahead (INFINITY: none)
    struct Axis {
        double p, d, lo, h, t;
        int n, c, step;
        __device__ double next() const {
            const int i = step > 0 ? c + 1 : c;   // the plane ahead: lower + i h, interior when 1 <= i <= n - 1
            if (step == 0 || i < 1 || i > n - 1) return INFINITY;
            return (lo + (double)i * h - p) / d;
        }
    };
    auto axis = [&](int a) -> Axis {
        Axis x;
        x.p = r[kFrRot + 3 * a] * px + r[kFrRot + 3 * a + 1] * py + r[kFrRot + 3 * a + 2] * pz + r[kFrT + a];
        x.d = r[kFrRot + 3 * a] * dx + r[kFrRot + 3 * a + 1] * dy + r[kFrRot + 3 * a + 2] * dz;
        x.lo = r[kFrLower + a];
        x.h = r[kFrH + a];
        x.n = (int)r[kFrShape + a];
        const double f = __builtin_floor((x.p - x.lo) / x.h);
        x.c = (int)__builtin_fmin(__builtin_fmax(f, 0.0), (double)(x.n - 1));   // (NaN: cell 0)
        x.step = x.d > 0.0 ? 1 : (x.d < 0.0 ? -1 : 0);
        x.t = x.next();
        return x;
    };
    Axis X = axis(0), Y = axis(1), Z = axis(2);
    double s = 0.0, tin = 0.0;
    for (;;) {
        const int cell = (X.c * Y.n + Y.c) * Z.n + Z.c;
        double ac = 0.0, p0 = 0.0;
        for (int k = 0; k < ccount; k++) {
            const double ak = k == 0 ? a0 : (k == 1 ? a1 : coef(k));
            const int vk = k == 0 ? v0 : (k == 1 ? v1 : (int)r[kFrComp + k]);
            ac += ak * fd[vk + cell];
            if (k == 0) p0 = ac;
        }
        // (a plane that rounding puts a hair behind the photon is crossed at zero length)
        const double tmin = __builtin_fmin(__builtin_fmin(X.t, Y.t), Z.t);
        const double sout = __builtin_fmax(__builtin_fmin(tmin, t0), s);
        if (ac > 0.0) {
            const double q = __builtin_fmax(tau - tin, 0.0);
            const double d = s + (ac > 1e-250 ? div_normal(q, ac) : q / ac);
            if (d < sout) return FieldMarch{d, ac, p0, cell};
            tin += ac * (sout - s);
        }
        if (!(sout < t0)) break;
        // the nearest plane is crossed (ties: one axis per pass, the others at zero length)
        if (X.t == tmin) { X.c += X.step; X.t = X.next(); }
        else if (Y.t == tmin) { Y.c += Y.step; Y.t = Y.next(); }
        else { Z.c += Z.step; Z.t = Z.next(); }
        s = sout;
    }
    return FieldMarch{INFINITY, 0.0, 0.0, 0};
}

// Volume maps (PvtMapTables; include/pvtrace_hip.h states the contract, the Python VolumeMap and tally.map_histories bin the
// same way): the tally of a lane that has just been absorbed in `container` (UF_VMAP).  The ABSORB event and the one
// event that followed it -- `kind`: EMIT, SCATTER, NONRADIATIVE or REACT, decided by component `comp` -- lie at the same
// point (px, py, pz), so the local point p = R x + t is formed once, as ((R0 x + R1 y) + R2 z) + t without FMA, from the
// node's block at md[container].  Every map of the node whose kind and component match takes ONE no-return 64-bit integer
// atomic in global memory: on slot ((ix ny + iy) nz + iz) nw + iw when floor((p - lower) / h) lies in 0 .. n - 1 on the
// three axes and the wavelength bin (w_in, the wavelength the photon arrived with; w_out, the emitted one, for EMIT) in
// 0 .. nw - 1, else on the map's `outside` slot, the one behind its cells.  `slots`: where the maps' block of the lane's
// tally set starts.  A FUNCTION, called only from the trace_kernel_rough* variants.
__device__ __attribute__((noinline)) void volume_map_call(const double* __restrict__ md, unsigned long long* __restrict__ slots,
                                                          int container, int comp, int kind, double px, double py, double pz,
                                                          double w_in, double w_out) {
    const int at = (int)md[container];
    if (at < 0) return;
    const double* __restrict__ r = md + at;
    const int count = (int)r[kMnCount];
    const double lx = ((r[kMnRot + 0] * px + r[kMnRot + 1] * py) + r[kMnRot + 2] * pz) + r[kMnT + 0];
    const double ly = ((r[kMnRot + 3] * px + r[kMnRot + 4] * py) + r[kMnRot + 5] * pz) + r[kMnT + 1];
    const double lz = ((r[kMnRot + 6] * px + r[kMnRot + 7] * py) + r[kMnRot + 8] * pz) + r[kMnT + 2];
    for (int m = 0; m < count; m++) {
        const double* __restrict__ q = r + kMnRec + m * kMr;
        const int mk = (int)q[kMrKind], mc = (int)q[kMrComp];
        if ((mk != PVT_EV_ABSORB && mk != kind) || (mc >= 0 && mc != comp)) continue;
        const double nx = q[kMrShape], ny = q[kMrShape + 1], nz = q[kMrShape + 2];
        const double fx = __builtin_floor((lx - q[kMrLower]) / q[kMrH]);
        const double fy = __builtin_floor((ly - q[kMrLower + 1]) / q[kMrH + 1]);
        const double fz = __builtin_floor((lz - q[kMrLower + 2]) / q[kMrH + 2]);
        // (a NaN coordinate fails every comparison: outside)
        bool inside = fx >= 0.0 && fx <= nx - 1.0 && fy >= 0.0 && fy <= ny - 1.0 && fz >= 0.0 && fz <= nz - 1.0;
        const int nw = (int)q[kMrNw];
        const long long nwc = nw > 0 ? nw : 1;
        long long iw = 0;
        if (nw > 0) {   // a Histogram's rule: truncation of (w - start) / (stop - start) * bins, in range 0 .. bins - 1
            const double w = mk == PVT_EV_EMIT ? w_out : w_in;
            const double qw = (w - q[kMrWlo]) / (q[kMrWhi] - q[kMrWlo]) * (double)nw;
            inside = inside && qw > -1.0 && qw < (double)nw;
            if (inside) iw = (long long)qw;
        }
        const long long cells = (long long)nx * (long long)ny * (long long)nz * nwc;
        long long slot = cells;   // (`outside`)
        if (inside) slot = (((long long)fx * (long long)ny + (long long)fy) * (long long)nz + (long long)fz) * nwc + iw;
        atomicAdd(slots + (long long)q[kMrOff] + slot, 1ull);
    }
}

// Path-length maps (PvtMapTables, map kind PVT_MAP_PATHLENGTH; include/pvtrace_hip.h states the contract, the Python VolumeMap
// and tally.map_histories walk the same way, operation for operation; the build has no FMA contraction): one SEGMENT of a
// lane -- from the world position (px, py, pz) along the unit direction (dx, dy, dz) for `len` = the advance, while its
// container is the node whose block is `r` (kMn*) -- laid into every path-length map of that node.  The local start and
// direction are formed once, ((R0 x + R1 y) + R2 z) + t and (R0 dx + R1 dy) + R2 dz.  Per map the walk is field_march_call's,
// on a lattice that has one half-infinite slab more on either side of each axis (cells -1 and n: nothing is clamped, the map
// may be smaller than its node): a piece of length l adds k = (int64)(l 2^30 + 0.5) units with ONE no-return 64-bit integer
// atomic in global memory, on the cell's slot when the cell lies in the lattice and the wavelength `wl` the photon travels
// with in the map's range, else on the map's `outside` slot; k = 0 adds nothing.  `slots`: where the maps' block of the
// lane's tally set starts.  A FUNCTION, called only from the kExtPath kernels' advance site.
__device__ __attribute__((noinline)) void path_map_call(const double* __restrict__ r, unsigned long long* __restrict__ slots,
                                                        double px, double py, double pz, double dx, double dy, double dz,
                                                        double len, double wl) {
    if (!(len > 0.0) || !(len < INFINITY)) return;   // (NaN, <= 0 or infinite: nothing)
    const int count = (int)r[kMnCount];
    const double lpx = ((r[kMnRot + 0] * px + r[kMnRot + 1] * py) + r[kMnRot + 2] * pz) + r[kMnT + 0];
    const double lpy = ((r[kMnRot + 3] * px + r[kMnRot + 4] * py) + r[kMnRot + 5] * pz) + r[kMnT + 1];
    const double lpz = ((r[kMnRot + 6] * px + r[kMnRot + 7] * py) + r[kMnRot + 8] * pz) + r[kMnT + 2];
    const double lux = (r[kMnRot + 0] * dx + r[kMnRot + 1] * dy) + r[kMnRot + 2] * dz;
    const double luy = (r[kMnRot + 3] * dx + r[kMnRot + 4] * dy) + r[kMnRot + 5] * dz;
    const double luz = (r[kMnRot + 6] * dx + r[kMnRot + 7] * dy) + r[kMnRot + 8] * dz;
    // one axis of the lattice in the node's frame: the cell the segment is in (-1 and n: the slabs outside) and the
    // parameter of the plane ahead (INFINITY: none)
    struct Axis {
        double p, d, lo, h, t;
        int n, c, step;
        __device__ double next() const {
            const int i = step > 0 ? c + 1 : c;   // the plane ahead: lower + i h, there when 0 <= i <= n
            if (step == 0 || i < 0 || i > n) return INFINITY;
            return (lo + (double)i * h - p) / d;
        }
    };
    for (int m = 0; m < count; m++) {
        const double* __restrict__ q = r + kMnRec + m * kMr;
        if ((int)q[kMrKind] != PVT_MAP_PATHLENGTH) continue;
        const int nw = (int)q[kMrNw];
        const long long nwc = nw > 0 ? nw : 1;
        bool wl_in = true;
        long long iw = 0;
        if (nw > 0) {   // a Histogram's rule, as in volume_map_call; out of range: the whole segment goes to `outside`
            const double qw = (wl - q[kMrWlo]) / (q[kMrWhi] - q[kMrWlo]) * (double)nw;
            wl_in = qw > -1.0 && qw < (double)nw;
            if (wl_in) iw = (long long)qw;
        }
        auto axis = [&](int a, double p, double d) -> Axis {
            Axis x;
            x.p = p; x.d = d;
            x.lo = q[kMrLower + a];
            x.h = q[kMrH + a];
            x.n = (int)q[kMrShape + a];
            const double f = __builtin_floor((x.p - x.lo) / x.h);
            x.c = (int)__builtin_fmin(__builtin_fmax(f, -1.0), (double)x.n);   // (NaN: cell -1)
            x.step = x.d > 0.0 ? 1 : (x.d < 0.0 ? -1 : 0);
            x.t = x.next();
            return x;
        };
        Axis X = axis(0, lpx, lux), Y = axis(1, lpy, luy), Z = axis(2, lpz, luz);
        unsigned long long* __restrict__ base = slots + (long long)q[kMrOff];
        const long long outside = (long long)X.n * (long long)Y.n * (long long)Z.n * nwc;
        double s = 0.0;
        for (;;) {
            // (a plane that rounding puts a hair behind the segment's start is crossed at zero length)
            const double tmin = __builtin_fmin(__builtin_fmin(X.t, Y.t), Z.t);
            const double sout = __builtin_fmax(__builtin_fmin(tmin, len), s);
            const long long k = (long long)((sout - s) * 1073741824.0 + 0.5);
            if (k != 0) {
                const bool inside = wl_in && X.c >= 0 && X.c < X.n && Y.c >= 0 && Y.c < Y.n && Z.c >= 0 && Z.c < Z.n;
                const long long slot = inside ? (((long long)X.c * Y.n + Y.c) * Z.n + Z.c) * nwc + iw : outside;
                atomicAdd(base + slot, (unsigned long long)k);
            }
            if (!(sout < len)) break;
            // the nearest plane is crossed (ties: one axis per pass, X then Y then Z, the others at zero length)
            if (X.t == tmin) { X.c += X.step; X.t = X.next(); }
            else if (Y.t == tmin) { Y.c += Y.step; Y.t = Y.next(); }
            else { Z.c += Z.step; Z.t = Z.next(); }
            s = sout;
        }
    }
}

// same, tables in global memory (emitter spectra)
__device__ __forceinline__ double interp_global(const double* xs, const double* ys, int n, double x) {
    if (n == 1) return ys[0];
    if (x <= xs[0]) return ys[0];
    if (x >= xs[n - 1]) return ys[n - 1];
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (xs[mid] <= x) lo = mid; else hi = mid;
    }
    if (xs[hi] == xs[lo]) return ys[lo];
    return ys[lo] + (ys[hi] - ys[lo]) * (x - xs[lo]) / (xs[hi] - xs[lo]);
}

__device__ __forceinline__ V3 sphere_direction(double theta, double phi) {
    double st, ct, sp, cp;
    pvt_sincos(theta, &st, &ct);
    pvt_sincos(phi, &sp, &cp);
    return V3{st * cp, st * sp, ct};
}

// Cosine-weighted direction about +z from two draws (material/utils.py:176-186: theta = asin(sqrt(p1)), phi = 2 pi p2,
// then sin / cos of both): the compositions evaluated directly, as everywhere else in portable arithmetic --
// sin(asin s) = s, cos(asin s) = pvt_sqrt1m2(s), sin / cos(2 pi u) = pvt_sincos2pi(u).
__device__ __forceinline__ V3 lambert_direction(double p1, double p2) {
    const double st = pvt_sqrt(p1), ct = sqrt1m2_normal(st);
    double sp, cp;
    pvt_sincos2pi(p2, &sp, &cp);
    return V3{st * cp, st * sp, ct};
}

// phase functions (_kernel.pyx:455-476); draw order is part of the contract
__device__ __forceinline__ V3 sample_phase(int type, double param, Rng& rng) {
    // the polar angle is sampled through its cosine (HG, isotropic) or its sine (cone); the other one is the
    // composition sin(acos c) = cos(asin c) = pvt_sqrt1m2(c) (pvt_math.h) -- no acos / asin / sincos of theta
    // (the azimuth is 2 pi `turn`: its sine and cosine come from pvt_sincos2pi, exact quadrant reduction)
    double turn, cos_t, sin_t;
    if (type == PVT_PHASE_HG && pvt_fabs(param) >= kEps) {
        double g = param;
        double g1 = rng_uniform(rng);
        double s = 2.0 * g1 - 1.0;
        double q = (1.0 - g * g) / (1.0 + g * s);
        cos_t = 1.0 / (2.0 * g) * (1.0 + g * g - q * q);
        // the quotient cancels for small |g| and at the ends of the draw grid and may leave [-1, 1] by a few ulp, where
        // the reference's acos is NaN: clamped, as the table turn's cosine is (an in-range value keeps its bits)
        cos_t = __builtin_fmin(__builtin_fmax(cos_t, -1.0), 1.0);
        turn = rng_uniform(rng);
        sin_t = pvt_sqrt1m2(cos_t);
    } else if (type == PVT_PHASE_CONE) {
        double g1 = rng_uniform(rng), g2 = rng_uniform(rng);
        sin_t = pvt_sqrt(g1) * pvt_sin(param);
        turn = g2;
        cos_t = pvt_sqrt1m2(sin_t);
    } else {
        double g1 = rng_uniform(rng), g2 = rng_uniform(rng);
        turn = g1;
        cos_t = 2.0 * g2 - 1.0;
        sin_t = pvt_sqrt1m2(cos_t);
    }
    double sp, cp;
    pvt_sincos2pi(turn, &sp, &cp);
    return V3{sin_t * cp, sin_t * sp, cos_t};
}

// ----------------------------------------------------------- emission
// Tabulated sources (include/pvtrace_hip.h, PvtSourceTables; the Python PositionGrid states the same rule): the local
// launch position of a PVT_POS_GRID light from its record `g` (kSg*).  One draw picks the cell by the bisection the phase
// tables use, cdf[a] <= u < cdf[b], so a cell of zero weight is never chosen; then one draw per bounded axis, x, y, z.
__device__ __forceinline__ V3 emit_grid_position(const double* g, Rng& rng) {
    const int ny = (int)g[kSgShape + 1], nz = (int)g[kSgShape + 2];
    const double* cdf = g + kSgCdf;
    const double u = rng_uniform(rng);
    int a = 0, b = (int)g[kSgShape] * ny * nz;
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (cdf[m] <= u) a = m; else b = m;
    }
    const int iz = a % nz, ixy = a / nz;
    const int iy = ixy % ny, ix = ixy / ny;
    V3 p{0.0, 0.0, 0.0};
    if (g[kSgBounded] != 0.0) p.x = g[kSgLower] + ((double)ix + rng_uniform(rng)) * g[kSgH];
    if (g[kSgBounded + 1] != 0.0) p.y = g[kSgLower + 1] + ((double)iy + rng_uniform(rng)) * g[kSgH + 1];
    if (g[kSgBounded + 2] != 0.0) p.z = g[kSgLower + 2] + ((double)iz + rng_uniform(rng)) * g[kSgH + 2];
    return p;
}
// ... and the local direction of a PVT_DIR_TABLE light: `phase_table_turn` about the light's +z on the table's first row
// (a wavelength below every row's takes it), u1 drawn whenever the table has several rows.
__device__ __forceinline__ V3 emit_table_direction(const double* tab, Rng& rng) {
    const double u1 = (int)tab[0] > 1 ? rng_uniform(rng) : 0.0;
    const double u2 = rng_uniform(rng);
    const double u3 = rng_uniform(rng);
    return phase_table_turn(tab, -__builtin_inf(), u1, u2, u3, 0.0, 0.0, 1.0);
}

// One ray from its own stream (mirrors oracle pvt_oracle_emit; distributions of
// reference pvtrace/engine/emit.py:22-89).
__device__ __forceinline__ void emit_one(const KArgs& A, unsigned long long gi, V3& pos, V3& dir, double& wl) {
    const double* ed = A.ed;
    const int* ei = A.ei;
    const EmitOff& E = A.eoff;
    Rng rng;
    rng_seed(rng, (A.emit_seed + gi) ^ kEmitSalt);
    int li = (int)(gi % (unsigned long long)A.n_lights);
    const int wt = ei[E.wl_type + li];
    if (wt == PVT_WL_SPECTRUM || wt == PVT_WL_SPECTRUM_HIST) {
        double u = rng_uniform(rng);
        int s = ei[E.wl_spec_start + li];
        const int n = ei[E.wl_spec_n + li];
        if (wt == PVT_WL_SPECTRUM_HIST) {
            // histogram-sampled spectrum: the abscissa at index #{cdf_i < u} (numpy.searchsorted, left), the last one
            // when u lies above the table (pvtrace/material/distribution.py:171-176)
            const double* cdf = ed + E.spec_cdf + s;
            int lo = 0, hi = n;   // cdf[i] < u for i < lo, cdf[i] >= u for i >= hi
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cdf[mid] < u) lo = mid + 1; else hi = mid;
            }
            wl = ed[E.spec_x + s + (lo < n ? lo : n - 1)];
        } else {
            wl = interp_global(ed + E.spec_cdf + s, ed + E.spec_x + s, n, u);
        }
    } else {
        wl = ed[E.wl_value + li];
    }
    V3 lp{0.0, 0.0, 0.0}, ld{0.0, 0.0, 1.0};
    const double* pp = ed + E.pos_param + li * 3;
    int pt = ei[E.pos_type + li];
    if (pt == PVT_POS_RECT) {
        lp.x = -pp[0] + 2.0 * pp[0] * rng_uniform(rng);
        lp.y = -pp[1] + 2.0 * pp[1] * rng_uniform(rng);
    } else if (pt == PVT_POS_CIRCLE) {
        double ang = 2.0 * kPi * rng_uniform(rng);
        double rad = pvt_sqrt(rng_uniform(rng)) * pp[0];
        double s, c;
        pvt_sincos(ang, &s, &c);
        lp.x = rad * c;
        lp.y = rad * s;
    } else if (pt == PVT_POS_CUBE) {
        lp.x = -pp[0] + 2.0 * pp[0] * rng_uniform(rng);
        lp.y = -pp[1] + 2.0 * pp[1] * rng_uniform(rng);
        lp.z = -pp[2] + 2.0 * pp[2] * rng_uniform(rng);
    } else if (pt == PVT_POS_GRID) {
        lp = emit_grid_position(ed + (int)pp[0], rng);   // (the packer wrote where the grid's record lies)
    }
    double prm = ed[E.dir_param + li];
    int dt = ei[E.dir_type + li];
    if (dt == PVT_DIR_CONE) ld = sample_phase(PVT_PHASE_CONE, prm, rng);
    else if (dt == PVT_DIR_ISOTROPIC) ld = sample_phase(PVT_PHASE_ISOTROPIC, 0.0, rng);
    else if (dt == PVT_DIR_HG) ld = sample_phase(PVT_PHASE_HG, prm, rng);
    else if (dt == PVT_DIR_LAMBERTIAN) {
        double p1 = rng_uniform(rng), p2 = rng_uniform(rng);
        ld = lambert_direction(p1, p2);
    } else if (dt == PVT_DIR_TABLE) {
        ld = emit_table_direction(ed + (int)prm, rng);   // (... and where the table's)
    }
    const double* m = ed + E.l2w + li * 16;
    pos.x = m[0] * lp.x + m[1] * lp.y + m[2] * lp.z + m[3];
    pos.y = m[4] * lp.x + m[5] * lp.y + m[6] * lp.z + m[7];
    pos.z = m[8] * lp.x + m[9] * lp.y + m[10] * lp.z + m[11];
    dir.x = m[0] * ld.x + m[1] * ld.y + m[2] * ld.z;
    dir.y = m[4] * ld.x + m[5] * ld.y + m[6] * ld.z;
    dir.z = m[8] * ld.x + m[9] * ld.y + m[10] * ld.z;
}

// The sampler as a FUNCTION (trace kernels, device emission): called by the wave that claims a chunk of rays, once per 64
// rays -- its 15 KB of code then sit beside the trace kernel's text instead of inside it (every EMIT variant as large
// as its array-input twin plus a call), at the price of the caller's live registers going through scratch around the call.
__device__ __attribute__((noinline)) void emit_chunk(const KArgs* A, unsigned long long gi, double* pool) {
    V3 ep, ed;
    double ew;
    emit_one(*A, gi, ep, ed, ew);
    pool[0] = ep.x; pool[64] = ep.y; pool[128] = ep.z;
    pool[192] = ed.x; pool[256] = ed.y; pool[320] = ed.z;
    pool[384] = ew;
}
// The parking entries' own copy (trace_kernel_lean_park): a function is compiled for the most demanding occupancy among
// its callers, and theirs -- five waves per SIMD -- would re-schedule the sampler under every other family as well.
__device__ __attribute__((noinline)) void emit_chunk_park(const KArgs* A, unsigned long long gi, double* pool) {
    V3 ep, ed;
    double ew;
    emit_one(*A, gi, ep, ed, ew);
    pool[0] = ep.x; pool[64] = ep.y; pool[128] = ep.z;
    pool[192] = ed.x; pool[256] = ed.y; pool[320] = ed.z;
    pool[384] = ew;
}

__global__ void __launch_bounds__(kBlock) emit_kernel(KArgs A, double* opos, double* odir, double* owl) {
    unsigned int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n_rays) return;
    V3 p, d;
    double wl;
    emit_one(A, A.ray_offset + i, p, d, wl);
    opos[i * 3] = p.x; opos[i * 3 + 1] = p.y; opos[i * 3 + 2] = p.z;
    odir[i * 3] = d.x; odir[i * 3 + 1] = d.y; odir[i * 3 + 2] = d.z;
    owl[i] = wl;
}

// Self-test hook: evaluates one elementary function per element on the device so the
// tests can prove the premise of the whole parity scheme (IEEE divide / sqrt and the
// pvt_math.h functions produce the same bits on gfx950 as on the host).
__global__ void __launch_bounds__(kBlock) math_kernel(int fn, const double* x, double* y, long long n) {
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double v = x[i], r;
    switch (fn) {
        case 0: r = pvt_log(v); break;
        case 1: r = pvt_sin(v); break;
        case 2: r = pvt_cos(v); break;
        case 3: r = pvt_asin(v); break;
        case 4: r = pvt_acos(v); break;
        case 5: r = pvt_sqrt(v); break;
        case 6: r = 1.0 / v; break;
        case 7: { double s, c; pvt_sincos(v, &s, &c); r = s * c; break; }
        case 8: { Rng g; rng_seed(g, (unsigned long long)v); rng_uniform(g); r = rng_uniform(g); break; }
        case 9: r = v / (v + 3.0); break;
        case 10: r = div_known(v, kCcm, kRcpCcm); break;
        case 11: r = div_known(v, 1.5, 1.0 / 1.5); break;
        case 12: r = div_known(v, 800.0 - 400.0, 1.0 / (800.0 - 400.0)); break;
        case 14: { double sn, cs; pvt_sincos2pi(v, &sn, &cs); r = sn; break; }
        case 15: { double sn, cs; pvt_sincos2pi(v, &sn, &cs); r = cs; break; }
        case 16: r = pvt_sqrt1m2(v); break;
        case 17: r = rcp_normal(v); break;
        case 18: r = div_normal(v, v * 0.7310585786300049 + 0.25); break;
        case 19: r = sqrt_normal(v); break;
        case 20: r = pvt_log_unit(v); break;    // (v = k 2^-53, 1 <= k <= 2^53)
        case 21: r = pvt_acos_unit(v); break;   // (v in [0, 1])
        default: { double d = v * 0.7310585786300049 + 0.25; r = div_known(v, d, 1.0 / d); break; }
    }
    y[i] = r;
}

// ----------------------------------------------------------- event log
// One event = one 128-byte record = one cache line, written by its lane with eight 16-byte stores:
//   words (u64)  0: hit | container<<32   1: adjacent | component<<32   2: source | kind<<32
//                3-5 position   6-8 direction   9-11 normal (zeros when the event has none)
//                12 wavelength  13 travelled  14 duration  15 row index (j*max_events + k)
// The reference keeps thirteen column arrays indexed [ray][event] (_kernel.pyx:562-597, :1035-1047); written
// from 64 lanes that follow 64 different rays, every 1-, 4-, 8- and 24-byte column store lands in a memory
// sector of its own (measured: 4.2 x the algorithmic bytes reach HBM).  A record is one full line instead; the
// column arrays, for callers that want them on the device, are made by unpack_log_kernel below with
// consecutive lanes on consecutive rows.
constexpr int kRecWords = 16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 pack_dd(double a, double b) {
    const unsigned long long ua = pvt_d2u(a), ub = pvt_d2u(b);
    return u32x4{(unsigned int)ua, (unsigned int)(ua >> 32), (unsigned int)ub, (unsigned int)(ub >> 32)};
}
// Ray capture (PvtCaptureTables / PvtCaptures; include/pvtrace_hip.h states the contract): the lanes of one tally trip whose
// photon has just matched recorder `r` for the first time (`push`) append one row each to the recorder's capture.  Rows are
// reserved per WAVE: the lanes are grouped by recorder, one lane of each group adds the group's size to the recorder's
// cursor -- one 64-bit atomic per wave per recorder per trip, not one per lane on one address -- and every lane writes its
// whole row at the rank its ballot gives it.  A row beyond the capacity is not written; the cursor counts it all the same.
// `rows` / `cursor`: the row buffer and the cursors of the lane's tally set.  A FUNCTION, called only from the
// trace_kernel_rough* variants, by every lane of the wave.
__device__ __attribute__((noinline)) void capture_call(const long long* __restrict__ tab, unsigned long long* __restrict__ rows,
                                                       unsigned long long* __restrict__ cursor, bool push, int r,
                                                       unsigned long long index, double px, double py, double pz, double dx,
                                                       double dy, double dz, double wl, double travelled, double duration,
                                                       int source, unsigned long long counters) {
    long long cap = 0, start = 0;
    if (push) { cap = tab[2 * r]; start = tab[2 * r + 1]; }
    bool want = cap > 0;
    for (;;) {
        const unsigned long long todo = __ballot(want);
        if (todo == 0ull) break;
        const int leader = __builtin_ctzll(todo);
        const int r0 = __builtin_amdgcn_readlane(r, leader);
        const bool mine = want && r == r0;
        const unsigned long long group = __ballot(mine);
        const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(group >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)group, 0u));
        unsigned long long base = 0ull;
        if (mine && rank == 0u) base = atomicAdd(cursor + r0, (unsigned long long)__popcll(group));
        const unsigned int lo = __builtin_amdgcn_readlane((unsigned int)base, leader);
        const unsigned int hi = __builtin_amdgcn_readlane((unsigned int)(base >> 32), leader);
        if (mine) {
            const long long at = (long long)(((unsigned long long)hi << 32) | lo) + rank;
            if (at < cap) {
                u32x4* dst = reinterpret_cast<u32x4*>(rows + (start + at) * kCapWords);
                dst[0] = u32x4{(unsigned int)index, (unsigned int)(index >> 32), (unsigned int)pvt_d2u(px), (unsigned int)(pvt_d2u(px) >> 32)};
                dst[1] = pack_dd(py, pz);
                dst[2] = pack_dd(dx, dy);
                dst[3] = pack_dd(dz, wl);
                dst[4] = pack_dd(travelled, duration);
                dst[5] = u32x4{(unsigned int)source, (unsigned int)r, (unsigned int)counters, (unsigned int)(counters >> 32)};
            }
            want = false;
        }
    }
}

// The kernel-argument segment through a pointer the compiler cannot trace back to it (the empty `asm`): what is read through
// it is a scalar load at the point of use.  A pointer or a launch invariant that only a rare path reads -- the ray arrays, the
// emission pool, the log, the carry buffers, the origin store -- is re-read this way where it is used: kept as a loop
// invariant it would sit in two scalar registers the loop is short of (spilled to VGPR lanes, each use a v_readlane), and
// scalar loads cost the vector pipe nothing.  Of a KERNEL only: inside a called function the intrinsic returns garbage
// (measured, ROCm 7.0) -- the tail function hands in the segment it was given (`A` there IS the segment, see tail_run).
// (`PVT_KERNEL_ARGS_OPAQUE(ak);` declares the pointer.  A macro: as a __forceinline__ function returning the pointer the same
// two statements move the scalar spills of two tally kernels of the extension family, docs/history.md)
typedef const __attribute__((address_space(4))) KArgs* KArgsSegment;
#define PVT_OPAQUE_POINTER(ak) asm volatile("" : "+s"(ak))
#define PVT_KERNEL_ARGS_OPAQUE(ak) KArgsSegment ak = (KArgsSegment)__builtin_amdgcn_kernarg_segment_ptr(); PVT_OPAQUE_POINTER(ak)

// (VIA_A: in the tail function, see above)
template <bool RECORD, bool VIA_A = false>
__device__ __forceinline__ void log_row(const KArgs& A, int rec_slot, int& nev, int kind, int hit,
                                        int container, int adjacent, int component, int source,
                                        const V3& pos, const V3& dir, bool has_normal, const V3& nrm,
                                        double wl, double travelled, double duration) {
    if constexpr (RECORD) {
        if (rec_slot < 0 || nev >= A.max_events) return;   // rec_slot: index of the recorded ray, -1 = not recorded
        const long long row = (long long)rec_slot * A.max_events + nev;
        // (the log pointer: read where it is used, not held across the whole loop)
        KArgsSegment ak = VIA_A ? (KArgsSegment)(unsigned long long)&A : (KArgsSegment)__builtin_amdgcn_kernarg_segment_ptr();
        PVT_OPAQUE_POINTER(ak);
        u32x4* dst = reinterpret_cast<u32x4*>(ak->log_rows + row * kRecWords);
        const unsigned long long p0 = pvt_d2u(pos.x);
        const V3 n = has_normal ? nrm : V3{0.0, 0.0, 0.0};
        dst[0] = u32x4{(unsigned int)hit, (unsigned int)container, (unsigned int)adjacent, (unsigned int)component};
        dst[1] = u32x4{(unsigned int)source, (unsigned int)kind, (unsigned int)p0, (unsigned int)(p0 >> 32)};
        dst[2] = pack_dd(pos.y, pos.z);
        dst[3] = pack_dd(dir.x, dir.y);
        dst[4] = pack_dd(dir.z, n.x);
        dst[5] = pack_dd(n.y, n.z);
        dst[6] = pack_dd(wl, travelled);
        dst[7] = pack_dd(duration, pvt_u2d((unsigned long long)row));
        nev += 1;
    }
}

// Records -> the reference's column arrays (PvtEventLog), one thread per row, consecutive lanes on consecutive
// rows of the same recorded ray, so every column is written in contiguous runs.  Rows a ray did not write
// (k >= counts[j]) get the reference's fill values (0, ids -1; _kernel.pyx:1035-1047) when `prefill`, else they
// are left alone.  grid.x walks the recorded rays (`rays_per_block` each), grid.y the events in chunks of 256.
__global__ void __launch_bounds__(kBlock) unpack_log_kernel(const unsigned long long* __restrict__ rows_in,
                                                            const int* __restrict__ counts, PvtEventLog out,
                                                            long long n_recorded, int max_events, int rays_per_block,
                                                            int prefill) {
    const int t = threadIdx.x;
    const int jr = rays_per_block > 1 ? t / max_events : 0;
    const int k = (rays_per_block > 1 ? t - jr * max_events : t) + (int)blockIdx.y * kBlock;
    const long long j = (long long)blockIdx.x * rays_per_block + jr;
    if (jr >= rays_per_block || j >= n_recorded || k >= max_events) return;
    const bool valid = k < counts[j];
    if (!valid && !prefill) return;
    const long long row = j * max_events + k;
    u32x4 q[8];
    if (valid) {
        const u32x4* src = reinterpret_cast<const u32x4*>(rows_in + row * kRecWords);
#pragma unroll
        for (int i = 0; i < 8; i++) q[i] = __builtin_nontemporal_load(src + i);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) q[i] = u32x4{0u, 0u, 0u, 0u};
        q[0] = u32x4{~0u, ~0u, ~0u, ~0u};
        q[1].x = ~0u;
    }
    auto dd = [&](int word) -> double {   // u64 word `word` of the record as a double
        const u32x4 v = q[word >> 1];
        const unsigned long long u = (word & 1) ? ((unsigned long long)v.w << 32 | v.z) : ((unsigned long long)v.y << 32 | v.x);
        return pvt_u2d(u);
    };
    out.hit[row] = (int)q[0].x; out.container[row] = (int)q[0].y;
    out.adjacent[row] = (int)q[0].z; out.component[row] = (int)q[0].w;
    out.source[row] = (int)q[1].x; out.kind[row] = (uint8_t)q[1].y;
    out.position[row * 3] = dd(3); out.position[row * 3 + 1] = dd(4); out.position[row * 3 + 2] = dd(5);
    out.direction[row * 3] = dd(6); out.direction[row * 3 + 1] = dd(7); out.direction[row * 3 + 2] = dd(8);
    out.normal[row * 3] = dd(9); out.normal[row * 3 + 1] = dd(10); out.normal[row * 3 + 2] = dd(11);
    out.wavelength[row] = dd(12); out.travelled[row] = dd(13); out.duration[row] = dd(14);
}

// Records -> PACKED records: the counts[j] rows of recorded ray j, rays one after the other (`first[j]` = rows of the
// rays before j, an exclusive prefix sum made by the host); same thread mapping as unpack_log_kernel.  What the
// host-buffer entry moves over PCIe.
__global__ void __launch_bounds__(kBlock) pack_log_kernel(const unsigned long long* __restrict__ rows_in,
                                                          const int* __restrict__ counts, const long long* __restrict__ first,
                                                          unsigned long long* __restrict__ packed, long long n_recorded,
                                                          int max_events, int rays_per_block) {
    const int t = threadIdx.x;
    const int jr = rays_per_block > 1 ? t / max_events : 0;
    const int k = (rays_per_block > 1 ? t - jr * max_events : t) + (int)blockIdx.y * kBlock;
    const long long j = (long long)blockIdx.x * rays_per_block + jr;
    if (jr >= rays_per_block || j >= n_recorded || k >= max_events || k >= counts[j]) return;
    const u32x4* src = reinterpret_cast<const u32x4*>(rows_in + (j * max_events + k) * kRecWords);
    u32x4* dst = reinterpret_cast<u32x4*>(packed + (first[j] + k) * kRecWords);
#pragma unroll
    for (int i = 0; i < 8; i++) dst[i] = __builtin_nontemporal_load(src + i);
}

// LDS accumulator layout (per workgroup), after the table copies:
//   f64 sums[n_rec*8] | u64 cross[n_rec] | u32 distinct[n_rec] | u32 bins[total_bins] (if they fit)
struct Accum {
    unsigned int* cross;
    unsigned int* distinct;
    double* sums;
    unsigned int* bins;  // null -> straight to global
};

template <int SEENW>
struct Seen {
    unsigned long long w[SEENW];
};

// --------------------------------------------------------------- kernel
// MESH: the scene has triangle-mesh nodes.  The BVH walk costs ~35 VGPRs, so scenes made of
// analytic shapes run the variant compiled without it (one more wave per SIMD).
// GRID: scenes of many nodes -- every lane finds the nodes its ray can cross through a uniform grid (see the node loop).
// TAIL: the same loop as a FUNCTION for the last wave of a draining workgroup (`tail_run`, below): no rays to claim, no
// rendezvous -- it takes the `tail_total` photons its caller left in the exchange buffer and steps them until none is left.
template <bool RECORD, int TAB_LDS, int SEENW, bool MESH, bool GRID, int ROUGH = 0, int LEAN = 0>
__device__ void tail_run(const KArgs* kernel_args, int total, unsigned int lds);
// (the SOLO instantiation of the same loop, for the trace_kernel_solo_fin entries: a function of its own, so that
// tail_run's instantiations keep their names)
#ifndef PVT_SOLO_TAIL
#define PVT_SOLO_TAIL 1   // the tail function takes the closed-form node stage too (0: the node loop alone, the A/B of profiles/solo_step.md)
#endif
template <int LEAN>
__device__ void tail_run_solo(const KArgs* kernel_args, int total, unsigned int lds);

// A wave leaves its workgroup: the LAST one to do so adds the workgroup's accumulators (LDS) to the launch's outputs -- one
// global atomic per non-zero slot -- and its step counters to the scene's.  (No closing barrier: retiring waves must never
// be counted by the drain-phase rendezvous barriers of the waves still running.)  A function of its own, given nothing but
// the kernel's argument pointer (made a scalar and a pointer to constant memory again, as in tail_run): where the
// accumulators lie in LDS is worked out here, from the same quantities trace_body lays them out by.
template <int TAB_LDS>
__device__ __attribute__((noinline)) void leave_workgroup(const KArgs* kernel_args) {
    extern __shared__ double smem[];
    const unsigned long long bits = (unsigned long long)kernel_args;
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)bits), hi = __builtin_amdgcn_readfirstlane((unsigned int)(bits >> 32));
    const KArgsSegment ak = (KArgsSegment)(((unsigned long long)hi << 32) | lo);
    const KArgs& A = *(const KArgs*)ak;
    const int lane = threadIdx.x & 63;
    // (the layout of trace_body: tables | sums | crossings | distinct | bins | control words)
    const int nd_lds = TAB_LDS == 1 ? A.nd : TAB_LDS == 2 ? A.nd_lds : 0;
    const int ni_stage = TAB_LDS == 1 ? A.ni : TAB_LDS == 2 ? A.ni_lds : 0;
    const int ni_lds = (ni_stage + 1) & ~1;
    int* lds_i = reinterpret_cast<int*>(smem + nd_lds);
    double* acc_sums = reinterpret_cast<double*>(lds_i + ni_lds);
    unsigned long long* acc_cross = reinterpret_cast<unsigned long long*>(acc_sums + A.n_rec * 8);
    unsigned int* acc_distinct = reinterpret_cast<unsigned int*>(acc_cross + A.n_rec);
    unsigned int* acc_bins = acc_distinct + ((A.n_rec + 1) & ~1);
    int* ctl = reinterpret_cast<int*>(acc_bins + ((A.bins_in_lds ? A.total_bins : 0) + 1 & ~1));
    const unsigned int set = A.set_size ? blockIdx.x / (unsigned int)A.wgs_per_set : 0u;
    __threadfence_block();
    int order = 0;
    if (lane == 0) order = atomicAdd(&ctl[CTL_DONE], 1);
    order = __builtin_amdgcn_readfirstlane(order);
    if (order != kWaves - 1) return;
    __threadfence_block();
    {
        unsigned long long* ctr = A.counters;
        if (ctr && lane < 4) {
            const unsigned long long* cnt = reinterpret_cast<const unsigned long long*>(ctl + CTL_COUNT);
            const unsigned long long v = lane == 3 ? (unsigned long long)kWaves : cnt[lane];
            if (v) atomicAdd(ctr + (blockIdx.x & 63u) * 8u + lane, v);
        }
        if (lane == 0) {   // the workgroup's life on both clocks (KArgs::stamp)
            const unsigned long long* t0 = reinterpret_cast<const unsigned long long*>(ctl + CTL_CLOCK);
            const unsigned long long real = wall_clock64(), cyc = __builtin_readcyclecounter();
            if (ctr) {
                atomicAdd(ctr + (blockIdx.x & 63u) * 8u + 4u, cyc - t0[1]);
                atomicAdd(ctr + (blockIdx.x & 63u) * 8u + 5u, real - t0[0]);
            }
            if (A.stamp) atomicMax(A.stamp + 1, real);
        }
    }
    unsigned long long* const out_distinct = reinterpret_cast<unsigned long long*>(A.rec_distinct) + (long long)set * A.set_stride_i;
    unsigned long long* const out_crossings = reinterpret_cast<unsigned long long*>(A.rec_crossings) + (long long)set * A.set_stride_i;
    unsigned long long* const out_bins = reinterpret_cast<unsigned long long*>(A.rec_bins) + (long long)set * A.set_stride_i;
    double* const out_sums = A.rec_sums + (long long)set * A.set_stride_d;
    for (int i = lane; i < A.n_rec; i += 64) {
        const unsigned long long c = acc_cross[i];
        const unsigned int d = acc_distinct[i];
        if (c) atomicAdd(out_crossings + i, c);
        if (d) atomicAdd(out_distinct + i, (unsigned long long)d);
    }
    for (int i = lane; i < A.n_rec * 8; i += 64) {
        double v = acc_sums[i];
        if (v != 0.0) atomicAdd(out_sums + i, v);
    }
    if (A.bins_in_lds)
        for (int i = lane; i < A.total_bins; i += 64) {
            unsigned int v = acc_bins[i];
            if (v) atomicAdd(out_bins + i, (unsigned long long)v);
        }
}

template <bool RECORD, int TAB_LDS, int SEENW, bool EMIT, bool MESH, bool GRID = false, bool TAIL = false, int ROUGH = 0,
          int LEAN = 0, bool PARK = false, bool SOLO = false>
__device__ __forceinline__ void trace_body(const KArgs& A, int tail_total = 0, unsigned int tail_lds = 0u) {
    // LEAN (the trace_kernel_lean family): the scene is of the plain kind the host proves at its creation (pvt_scene_pack.h:
    // prove_lean) -- unrotated boxes (in a world that is a box or a sphere) holding absorbers and isotropic luminophores, spectra on even grids, no coating, no
    // extension table, every recorder entry plain.  What those facts decide is a constant here instead of a question
    // asked of the tables in every trip: the code they make unreachable is left out, everything that remains is the
    // generic variant's, operation for operation.
    static_assert(!LEAN || (!MESH && !GRID && !ROUGH && TAB_LDS == 1 && SEENW == 1), "the lean variants: plain scenes only");
    // PARK (the trace_kernel_lean_park entries): the launch parks its survivors for its successor on the stream --
    // `carry_flags & 2`, which the host has decided before it chooses the kernel, is a constant true here.  A wave that finds
    // the ray cursor dry parks and leaves, so the launch can reach neither the drain rendezvous nor the tail function: they
    // are not compiled, and the registers and the call frame that only `tail_run` asks for are not the kernel's.  Draws,
    // refill order and the resuming of carried photons are the other entries', operation for operation.
    static_assert(!PARK || (LEAN && !RECORD && !TAIL), "the parking form: tally launches of the lean family only");
    // SOLO (the trace_kernel_solo entries): moreover the scene is ONE unrotated box inside a lazy root that holds nothing and
    // that nobody listens to (pvt_scene_pack.h: prove_solo), and the launch has `lazy_root` and `fuse_exit`.  The node stage of
    // a trip is then one of three outcomes that two comparisons on the slab test decide: see "SOLO" there.  The node loop
    // stays in the text: a wave with a lane the closed form does not cover runs it for that trip.
    static_assert(!SOLO || (LEAN && !RECORD), "the solo form: tally launches of the lean family only");
    extern __shared__ double smem_of_kernel[];
    // (In a called function the address of the kernel's dynamic LDS is looked up in a table in memory wherever it is used --
    // six scalar loads and waits per step of the tail function, measured in its ISA; the kernel hands it over instead.)
    double* const smem = TAIL ? (double*)(__attribute__((address_space(3))) double*)(unsigned long long)tail_lds
                              : (double*)smem_of_kernel;
    // A wave alone waits out every scalar-cache round trip too: what the loop asks of the kernel's arguments time and again
    // is held in registers by the tail function (the kernels' own loop re-reads them where it needs them: a scalar load
    // costs it nothing, a register does).
    // (interp_clamped; LEAN: kLeanSearched = no histogram, kLeanEven = moreover every spectrum constant or on a proven even grid)
    constexpr int kAbsKind = LEAN == kLeanEven ? kInterpEven : LEAN ? kInterpNoHist : kInterpAny;
    constexpr int kCdfKind = LEAN == kLeanEven ? kInterpByGuide : LEAN ? kInterpNoHist : kInterpAny;
    auto held = [](int v) __attribute__((always_inline)) -> int {
        if constexpr (TAIL) asm volatile("" : "+s"(v));
        return v;
    };
    const int k_root = held(A.root), k_maxsteps = held(A.maxsteps), k_nodes = held(A.n_nodes);
#if PVT_TIMELINE
    unsigned long long tl_t[6] = {(unsigned long long)wall_clock64(), 0, 0, 0, 0, 0};
    unsigned long long tl_iters = 0;
    const unsigned long long tl_c0 = __builtin_readcyclecounter();   // shader clock (s_memtime); wall_clock64 is the constant 100 MHz one
#endif
    Lay L = A.lay;
    if constexpr (TAIL) {   // (every field the step reads, resident)
        L.comp_d = held(L.comp_d); L.rec_d = held(L.rec_d); L.hist_d = held(L.hist_d); L.coat_d = held(L.coat_d);
        L.comp_i = held(L.comp_i); L.rec_i = held(L.rec_i); L.hist_i = held(L.hist_i); L.coat_i = held(L.coat_i);
        L.cand_i = held(L.cand_i); L.cand_list = held(L.cand_list); L.crit_d = held(L.crit_d); L.ccrit_d = held(L.ccrit_d);
        L.grid_d = held(L.grid_d); L.rot_d = held(L.rot_d); L.ncls_d = held(L.ncls_d); L.n_cls = held(L.n_cls);
    }
    // Launch constants that the loop only asks yes/no questions of, in ONE scalar register.  Kept as separate
    // conditions each becomes a 64-bit lane mask that the allocator holds (spills) for the whole loop; `uf(bit)`
    // re-derives the answer from the word where it is asked (the empty asm keeps the compiler from hoisting it).
    enum { UF_COATED = 0, UF_FUSE_EXIT, UF_CRIT, UF_HAS_REC, UF_TQ_POS, UF_BINS_LDS, UF_EMIT_FULL, UF_EMIT_KT, UF_LAZY1, UF_LAZY2, UF_BY_NODE,
           UF_TAIL_LAZY1, UF_TAIL_LAZY2, UF_CTAB, UF_DISP, UF_ROUGH, UF_FIELD, UF_VMAP, UF_CAPTURE, UF_CABS, UF_COUNT, UF_TQ_COUNT, UF_ORIGIN, UF_CPAT, UF_ALIGN, UF_PMAP, UF_CLOBE };
    unsigned int uflags_ =
        (A.n_coat > 0 ? 1u << UF_COATED : 0u) | (A.fuse_exit != 0 ? 1u << UF_FUSE_EXIT : 0u) | (L.crit_d >= 0 ? 1u << UF_CRIT : 0u) |
        (A.n_rec > 0 ? 1u << UF_HAS_REC : 0u) | (A.tq_pos ? 1u << UF_TQ_POS : 0u) | (A.bins_in_lds ? 1u << UF_BINS_LDS : 0u) |
        (A.emit_method == PVT_EMIT_FULL ? 1u << UF_EMIT_FULL : 0u) | (A.emit_method == PVT_EMIT_KT ? 1u << UF_EMIT_KT : 0u) |
        (A.lazy_root == 1 ? 1u << UF_LAZY1 : 0u) | (A.lazy_root == 2 ? 1u << UF_LAZY2 : 0u) | (L.by_node ? 1u << UF_BY_NODE : 0u) |
        (A.n_ctab > 0 ? 1u << UF_CTAB : 0u) | (A.n_rtab > 0 ? 1u << UF_DISP : 0u) |
        (ROUGH && A.rough_d >= 0 ? 1u << UF_ROUGH : 0u) |   // (only the rough variants read rough_d ...
        (ROUGH && A.fd != nullptr ? 1u << UF_FIELD : 0u) |  // ... and fd ...
        (ROUGH && A.md != nullptr ? 1u << UF_VMAP : 0u) |   // ... and md ...
        (ROUGH && A.cap_tab != nullptr ? 1u << UF_CAPTURE : 0u) |   // ... and cap_tab ...
        (ROUGH && A.cabs_d >= 0 ? 1u << UF_CABS : 0u) |   // ... and cabs_d ...
        (ROUGH && A.count >= 1 ? 1u << UF_COUNT : 0u) | (ROUGH && A.count >= 2 ? 1u << UF_TQ_COUNT : 0u) |   // ... and count ...
        (ROUGH && A.origin != 0 ? 1u << UF_ORIGIN : 0u) |   // ... and origin ...
        (ROUGH && A.pd_d >= 0 ? 1u << UF_CPAT : 0u) |   // ... and pd_d ...
        (ROUGH >= kExtAligned ? 1u << UF_ALIGN : 0u) |   // ... UF_ALIGN is the kernel's own: compiled in, not read ...
        (ROUGH == kExtPath && A.md != nullptr ? 1u << UF_PMAP : 0u) |   // ... UF_PMAP too: the kExtPath kernels of a scene with maps ...
        (ROUGH && A.clobe_i >= 0 ? 1u << UF_CLOBE : 0u);   // ... and clobe_i)
    if constexpr (TAIL) {   // (only where the launch itself has no lazy root: see KArgs::lazy_tail)
        if (A.lazy_root == 0) uflags_ |= (A.lazy_tail == 1 ? 1u << UF_TAIL_LAZY1 : 0u) | (A.lazy_tail == 2 ? 1u << UF_TAIL_LAZY2 : 0u);
    }
    const unsigned int uflags = uflags_;
    auto uf = [&](int bit) -> bool {
        if constexpr (LEAN != kLeanOff) {   // (proven: no coating, no table of an extension; few nodes, numbered as they are)
            if (bit == UF_COATED || bit == UF_CTAB || bit == UF_DISP || bit == UF_ROUGH || bit == UF_FIELD || bit == UF_VMAP || bit == UF_CAPTURE || bit == UF_CABS || bit == UF_COUNT || bit == UF_TQ_COUNT || bit == UF_ORIGIN || bit == UF_CPAT || bit == UF_ALIGN || bit == UF_PMAP || bit == UF_CLOBE) return false;
            if (bit == UF_BY_NODE || bit == UF_CRIT) return true;   // (UF_CRIT: the threshold table is there and holds no NaN)
        }
        unsigned int f = uflags;
        asm volatile("" : "+s"(f));
        return ((f >> bit) & 1u) != 0u;
    };
    // The logarithm of a draw, log(1 - rng_uniform()): the lean bodies take pvt_log_unit, which is pvt_log on exactly
    // those arguments without the special cases none of them can reach -- the same bits, half the instructions.
    auto log_draw = [](double x) __attribute__((always_inline)) -> double {
        if constexpr (LEAN != kLeanOff) return pvt_log_unit(x);
        else return pvt_log(x);
    };

    // ---- stage tables + zero accumulators --------------------------------
    double* lds_d = smem;
    const int nd_lds = TAB_LDS == 1 ? A.nd : TAB_LDS == 2 ? A.nd_lds : 0;
    const int ni_stage = TAB_LDS == 1 ? A.ni : TAB_LDS == 2 ? A.ni_lds : 0;
    const int ni_lds = (ni_stage + 1) & ~1;  // keep 8-byte alignment after the ints
    int* lds_i = reinterpret_cast<int*>(lds_d + nd_lds);
    double* acc_sums = reinterpret_cast<double*>(lds_i + ni_lds);
    // crossings are 64-bit: a trapped photon crosses surfaces up to `maxsteps` times, and a persistent
    // workgroup of a 2^31-photon launch sees millions of photons (distinct rays and bins are bounded by them)
    unsigned long long* acc_cross = reinterpret_cast<unsigned long long*>(acc_sums + A.n_rec * 8);
    unsigned int* acc_distinct = reinterpret_cast<unsigned int*>(acc_cross + A.n_rec);
    unsigned int* acc_bins = acc_distinct + ((A.n_rec + 1) & ~1);   // (keeps what follows 8-byte aligned)
    int* ctl = reinterpret_cast<int*>(acc_bins + ((A.bins_in_lds ? A.total_bins : 0) + 1 & ~1));
    unsigned long long* xbuf = reinterpret_cast<unsigned long long*>(ctl + CTL_WORDS);  // [x_words][xslots] u64 words (see PVT_PHOTON_PUT)
    // per-wave queue of first crossings awaiting their statistics: [4 (+3 with positions)][kTallyQ] doubles
    // + [kTallyQ] recorder ids
    constexpr int kXWords = xbuf_words(SEENW, RECORD, false, false);
    // (scenes that count, KArgs::count -- a captured recorder makes a scene one: two more words per slot, the photon's global ray
    // index, which captures read, and its event counters; the rough variants alone)
    // (scenes that read a launch origin, KArgs::origin: kOriginWords more behind those)
    const int x_words = xbuf_words(SEENW, RECORD, ROUGH && A.count != 0, ROUGH && A.origin != 0);
    // (a histogram reads a counter: one more column, the packed word, behind the positions' or in their place; one reads a
    // launch origin: one more column behind that for each origin that IS read, in the order of their ids)
    const int tq_doubles = (A.tq_pos ? 7 : 4) + (ROUGH && A.count >= 2 ? 1 : 0) + (ROUGH ? __builtin_popcount((unsigned int)A.origin & 15u) : 0);
    const int tq_count_at = (A.tq_pos ? 7 : 4) * kTallyQ;
    double* const tq_d = reinterpret_cast<double*>(xbuf + x_words * A.xslots) + (threadIdx.x >> 6) * (tq_doubles * kTallyQ);
    int* const tq_r = reinterpret_cast<int*>(reinterpret_cast<double*>(xbuf + x_words * A.xslots) + kWaves * tq_doubles * kTallyQ)
                      + (threadIdx.x >> 6) * kTallyQ;
    int tq_n = 0;   // wave-uniform
    if constexpr (!TAIL) {   // (the tail function finds the workgroup's LDS as its caller left it)
    if (threadIdx.x < CTL_WORDS) ctl[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 4 && A.cursor_next) A.cursor_next[threadIdx.x] = 0u;
    if constexpr (MESH) {   // the top of the triangle trees (two 16-byte words per record)
        typedef unsigned int Word4 __attribute__((ext_vector_type(4)));
        Word4* dst = reinterpret_cast<Word4*>(reinterpret_cast<char*>(smem) + A.top_off);
        const Word4* src = reinterpret_cast<const Word4*>(A.bvh_top);
        for (int i = threadIdx.x; i < A.top_n * 2; i += kBlock) dst[i] = src[i];
    }
    if constexpr (TAB_LDS != 0) {
        for (int i = threadIdx.x; i < nd_lds; i += kBlock) lds_d[i] = A.gd[i];
        for (int i = threadIdx.x; i < ni_stage; i += kBlock) lds_i[i] = A.gi[i];
    }
    for (int i = threadIdx.x; i < A.n_rec * 8; i += kBlock) acc_sums[i] = 0.0;
    for (int i = threadIdx.x; i < A.n_rec; i += kBlock) { acc_cross[i] = 0ull; acc_distinct[i] = 0u; }
    if (A.bins_in_lds)
        for (int i = threadIdx.x; i < A.total_bins; i += kBlock) acc_bins[i] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) {   // (KArgs::stamp; read again by the last wave to leave, in leave_workgroup)
        unsigned long long* t0 = reinterpret_cast<unsigned long long*>(ctl + CTL_CLOCK);
        t0[0] = wall_clock64(); t0[1] = __builtin_readcyclecounter();
        if (blockIdx.x == 0 && A.stamp) A.stamp[0] = t0[0];
    }
    }
#if PVT_TIMELINE
    tl_t[1] = wall_clock64();
#endif

    Tables<TAB_LDS> T{(CDoubles)A.gd, (CInts)A.gi, TAB_LDS != 0 ? lds_d : A.gd, TAB_LDS != 0 ? lds_i : A.gi, A.gd, A.gi};

    // a node's flag word, read by the lane (see ND_BITS)
    auto node_bits = [&](int node) -> unsigned long long { return pvt_d2u(T.dv(node * ND + ND_BITS)); };
    auto node_ident = [](unsigned long long bits) -> bool { return LEAN || (bits & 1ull) != 0; };
    // (lean: boxes, and a root that may be a sphere -- whatever is not a sphere is a box)
    auto node_geom = [](unsigned long long bits) -> int {
        const int g = (int)(((unsigned int)bits >> 8) & 0xffu);
        return LEAN ? (g == PVT_GEOM_SPHERE ? (int)PVT_GEOM_SPHERE : (int)PVT_GEOM_BOX) : g;
    };
    auto node_rot = [&](unsigned long long bits) -> int { return L.rot_d + (int)(unsigned int)(bits >> 32) * RT; };

    // Forward crossings (t > kEps) of one analytic shape by the ray (o, d) in the shape's own frame, each handed to
    // `fold` in the reference's order (_kernel.pyx:245-345).  `inv`: 1/d per axis (boxes only).  The shape parameters
    // are scalars in the wave-uniform node loop and per-lane values in the grid walk: same operations either way.
    auto shape_hits = [](int gt, double g0, double g1, double g2, const V3& o, const V3& d, double inv0, double inv1, double inv2,
                         auto&& fold) __attribute__((always_inline)) {
        if (gt == PVT_GEOM_BOX) {  // slab test (:245-276)
            double tmin = -INFINITY, tmax = INFINITY;
            bool miss = false;
            const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, gpar[3] = {g0, g1, g2}, inv[3] = {inv0, inv1, inv2};
            // a ray parallel to a pair of faces (a direction component below 1e-300) takes the reference's
            // inside/outside test for that axis; the wave only runs the general form when a lane holds one
            if (__ballot(pvt_fabs(dd[0]) < 1e-300 || pvt_fabs(dd[1]) < 1e-300 || pvt_fabs(dd[2]) < 1e-300) == 0ull) {
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const double sz = gpar[a];
                    const double ta = (-0.5 * sz - oo[a]) * inv[a], tb = (0.5 * sz - oo[a]) * inv[a];
                    tmin = __builtin_fmax(tmin, __builtin_fmin(ta, tb));
                    tmax = __builtin_fmin(tmax, __builtin_fmax(ta, tb));
                }
            } else
#pragma unroll
            for (int a = 0; a < 3; a++) {
                double sz = gpar[a];
                double lo = -0.5 * sz, hi = 0.5 * sz;
                if (pvt_fabs(dd[a]) < 1e-300) {
                    if (oo[a] < lo || oo[a] > hi) miss = true;
                } else {
                    // (the reference swaps ta, tb into order and keeps the largest entry / smallest exit
                    // distance: min and max of finite numbers, which is what these are)
                    const double ta = (lo - oo[a]) * inv[a], tb = (hi - oo[a]) * inv[a];
                    tmin = __builtin_fmax(tmin, __builtin_fmin(ta, tb));
                    tmax = __builtin_fmin(tmax, __builtin_fmax(ta, tb));
                }
            }
            if (!miss && !(tmax < tmin)) {
                if (tmin > kEps) fold(tmin);
                if (tmax > kEps) fold(tmax);
            }
        } else if (gt == PVT_GEOM_SPHERE) {  // (:279-298)
            double radius = g0;
            double a = dot3(d, d), b = 2.0 * dot3(d, o), c = dot3(o, o) - radius * radius;
            double disc = b * b - 4.0 * a * c;
            if (!(disc < 0.0)) {
                double sq = pvt_sqrt(disc);
                double t = (-b - sq) / (2.0 * a);
                if (t > kEps) fold(t);
                t = (-b + sq) / (2.0 * a);
                if (t > kEps) fold(t);
            }
        } else {  // capped z cylinder (:301-345) -- (a truncated cone never comes here: its scene gets no node grid, plan_node_grid)
            double half = 0.5 * g0, radius = g1;
            double a = d.x * d.x + d.y * d.y;
            if (a > 1e-300) {
                double b = 2.0 * (o.x * d.x + o.y * d.y);
                double c = o.x * o.x + o.y * o.y - radius * radius;
                double disc = b * b - 4.0 * a * c;
                if (disc >= 0.0) {
                    double sq = pvt_sqrt(disc);
                    double t = (-b - sq) / (2.0 * a);
                    double z = o.z + t * d.z;
                    if (z > -half && z < half && t > kEps) fold(t);
                    t = (-b + sq) / (2.0 * a);
                    z = o.z + t * d.z;
                    if (z > -half && z < half && t > kEps) fold(t);
                }
            }
            if (pvt_fabs(d.z) > 1e-300) {
                double t = (-half - o.z) / d.z;
                double x = o.x + t * d.x, y = o.y + t * d.y;
                if (x * x + y * y <= radius * radius && t > kEps) fold(t);
                t = (half - o.z) / d.z;
                x = o.x + t * d.x;
                y = o.y + t * d.y;
                if (x * x + y * y <= radius * radius && t > kEps) fold(t);
            }
        }
    };

    const int lane = threadIdx.x & 63;
    // rank of this lane among the set bits of a wave mask: the bits below it, counted by the mbcnt pair
    auto rank_in = [](unsigned long long mask) -> unsigned int {
        return __builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
    };

    // ---- the rays this workgroup draws from: the whole launch, or its tally set (wave-uniform) ------
    const unsigned int set = A.set_size ? blockIdx.x / (unsigned int)A.wgs_per_set : 0u;
    const unsigned int ray_lo = set * A.set_size;
    const unsigned int n_local = A.set_size ? (A.n_rays - ray_lo < A.set_size ? A.n_rays - ray_lo : A.set_size) : A.n_rays;
    unsigned int* const cursor = A.cursor + set;

    // ---- per-photon state --------------------------------------------------
    bool alive = false;
    V3 pos{0, 0, 0}, dir{0, 0, 1};
    double wl = 0.0, travelled = 0.0, duration = 0.0;
    Rng rng{0, 0, 0, 0};
    int count = 0, source = -1, nev = 0;
    unsigned long long gidx = 0ull;   // (rough variants, UF_CAPTURE) the photon's global ray index, ray_offset + i: travels with it
    // (rough variants, UF_COUNT) the photon's event counters, kCountBits each: the EMIT | SCATTER << 20 | REFLECT << 40 rows of its
    // history so far.  Zero at the claim, it travels with the photon wherever `gidx` does and is advanced AFTER a step's
    // tally, from the kind of the row the step wrote last: a recorder sees the photon as it arrives (include/pvtrace_hip.h)
    unsigned long long hcount = 0ull;
    // (rough variants, UF_ORIGIN) the photon's launch origin -- wavelength, x, y, z of its GENERATE row, the position in the root's
    // frame as the ray arrays hold it.  Written ONCE, when the lane claims the ray, read only at a recorder's first match, and
    // moved wherever `gidx` moves: it lives in no register across the loop but in this lane's words of a side store in global
    // memory (KArgs::origin_store, L2-resident as the emission pool is), [lane of the launch][kOriginWords].  A lane reads back
    // only what it wrote itself; a photon changes lanes through the exchange buffer or a carry record, which hold the words.
    // (the kernel re-reads the pointer from its argument segment where it is used, as it does the ray pointers: held, it would
    // cost the loop two scalar registers.  The tail function reads it through `A`, which there IS the segment, handed over by
    // the caller: the kernel-argument intrinsic returns garbage inside a called function, see tail_run)
    auto origin_slot = [&]() __attribute__((always_inline)) -> double* {   // this lane's kOriginWords doubles, side by side
        double* store;
        if constexpr (TAIL) {
            store = A.origin_store;
        } else {
            PVT_KERNEL_ARGS_OPAQUE(ak);
            store = ak->origin_store;
        }
        return store + ((unsigned long long)blockIdx.x * kBlock + (unsigned long long)threadIdx.x) * kOriginWords;
    };
    auto origin_put = [&](double w, double x, double y, double z) __attribute__((always_inline)) {
        double* o = origin_slot();
        o[0] = w; o[1] = x; o[2] = y; o[3] = z;
    };
    // (KArgs::origin, likewise)
    auto origin_mask = [&]() __attribute__((always_inline)) -> unsigned int {
        if constexpr (TAIL) {
            return (unsigned int)A.origin;
        } else {
            PVT_KERNEL_ARGS_OPAQUE(ak);
            return (unsigned int)ak->origin;
        }
    };
    unsigned int c_iters = 0u, c_steps = 0u, c_fused = 0u;   // this lane's share of the step counters (KArgs::counters)
    // (tail function) the absorption coefficients this lane's photon met last: container, wavelength bits, sum, first term
    // -- kept in LDS, in the exchange buffer the function was handed its photons through (free once they are read): four
    // words per lane, read together (one wait) where two table lookups stood; in registers they were seven more than the
    // function has (the hit node's record, below, went to scratch for them)
    int ac_node = -1;
    unsigned long long ac_wl = 0ull;
    double ac_alpha = 0.0, ac_pre0 = 0.0;
    unsigned long long* const ac_lds = xbuf + lane;   // [4][64] words: container, wavelength bits, sum, first term
    // (tail function) the record of the node this step's nearest crossing lies on, and the Fresnel constants of the pair
    // (container, adjacent), read in one go right after the node loop
    V3 hr_t{0, 0, 0}, hr_g{0, 0, 0};
    unsigned long long hr_bits = 0ull;
    int hr_surf = 0;
    double hr_n2 = 0.0, hr_rn2 = 0.0, hr_cc = 0.0;
    constexpr bool kHoist = TAIL;
    constexpr bool kClassRegions = LEAN != kLeanOff;   // (lean) the step's class-keyed bodies: one divergent region per lane class
    // (scenes with index tables, UF_DISP) the refractive index of `node` at the photon's wavelength: its class's table
    // n(lambda), or `n`, the node's scalar index, when the class has none (a dispersive node has a class of its own)
    auto index_at = [&](int node, double n) -> double {
        const int k = uf(UF_BY_NODE) ? node : T.iv(node * NI + NI_NCLS);
        const int q = L.ncls_d + 2 * L.n_cls;
        const double* tab = TAB_LDS == 1 ? T.ld : T.hd;   // (where the spectra are read from)
        if constexpr (MESH || SEENW == 1) return index_class_n_call((TAB_LDS != 0 ? T.ld : T.hd) + q, tab, k, n, wl);
        const int np = (int)T.dv(q + 2 * k + 1);
        if (np == 0) return n;
        return index_table_n(tab + (int)T.dv(q + 2 * k), np, wl);
    };
    int rec_slot = -1;   // recorded rays: index among them (row block rec_slot * max_events), else -1
    Seen<SEENW> seen;
#pragma unroll
    for (int w = 0; w < SEENW; w++) seen.w[w] = 0ull;
    // ---- a photon on the move: ONE put and ONE get -------------------------
    // Everything that travels with a photon when it changes lanes -- through the LDS exchange buffer (the drain's repacking, the
    // hand-over to the tail function) or through a carry record (parked for the next launch) -- is written by PVT_PHOTON_PUT
    // and read by PVT_PHOTON_GET, and by nothing else: a word that is to travel is added HERE, to both, and to the word counts
    // (xbuf_words / carry_words).  `word(k)` names word k of the place: PVT_SLOT_WORD for the buffer (column-major, stride
    // kXSlots: constant offsets in the LDS instructions), PVT_SRC_WORD / PVT_DST_WORD for a carry record (photon-major: one
    // base address, every word at an immediate offset).  The core -- words 0 to 13, then the seen-mask from word kCarryBase,
    // then the history cursor of a RECORD launch (the buffer alone: a history launch carries nothing) -- stands at the same
    // words in both.  What the rough variants add stands behind `base`, and that is the layouts' ONLY difference: kXWords in
    // the buffer, kCarryStride in a record (whose mask always has room for four words).  Behind `base`: the global ray
    // index and the event counters (kCountWords, UF_CAPTURE / UF_COUNT), then the launch origin (kOriginWords, UF_ORIGIN; it
    // lives in the lane's side store, see origin_slot, not in a register).
    // MACROS over the loop's own variables, and a bare block each, because every other form was measured to move the
    // kernels' registers or code (docs/history.md): a helper that takes the variables by reference costs every kernel scalar
    // spills, called or not; one that takes and returns them by value reorders the kernels it is inlined into and moves the
    // extension family's spills; so does a lambda for `word`.  As they stand the six sites compile to the very code they
    // compiled to spelled out.
#define PVT_SLOT_WORD(k) xbuf[(k) * kXSlots + slot]
#define PVT_SRC_WORD(k) src[k]
#define PVT_DST_WORD(k) dst[k]
#define PVT_PHOTON_PUT(word, base) { \
        word(0) = pvt_d2u(pos.x); word(1) = pvt_d2u(pos.y); word(2) = pvt_d2u(pos.z); \
        word(3) = pvt_d2u(dir.x); word(4) = pvt_d2u(dir.y); word(5) = pvt_d2u(dir.z); \
        word(6) = pvt_d2u(wl); word(7) = pvt_d2u(travelled); word(8) = pvt_d2u(duration); \
        word(9) = rng.s0; word(10) = rng.s1; word(11) = rng.s2; word(12) = rng.s3; \
        word(13) = (unsigned long long)(unsigned int)count | ((unsigned long long)(unsigned int)source << 32); \
        _Pragma("unroll") \
        for (int w = 0; w < SEENW; w++) word(kCarryBase + w) = seen.w[w]; \
        if constexpr (RECORD) { \
            word(kCarryBase + SEENW) = (unsigned long long)(unsigned int)rec_slot | ((unsigned long long)(unsigned int)nev << 32); \
        } \
        if constexpr (ROUGH) { \
            if (uf(UF_CAPTURE)) word(base) = gidx; \
            if (uf(UF_COUNT)) word((base) + 1) = hcount; \
            if (uf(UF_ORIGIN)) { \
                const int at = uf(UF_COUNT) ? (base) + kCountWords : (base);   /* (wave-uniform) */ \
                const double* o = origin_slot(); \
                _Pragma("unroll") \
                for (int k = 0; k < kOriginWords; k++) word(at + k) = pvt_d2u(o[k]); \
            } \
        } \
    }
#define PVT_PHOTON_GET(word, base) { \
        pos = V3{pvt_u2d(word(0)), pvt_u2d(word(1)), pvt_u2d(word(2))}; \
        dir = V3{pvt_u2d(word(3)), pvt_u2d(word(4)), pvt_u2d(word(5))}; \
        wl = pvt_u2d(word(6)); travelled = pvt_u2d(word(7)); duration = pvt_u2d(word(8)); \
        rng.s0 = word(9); rng.s1 = word(10); rng.s2 = word(11); rng.s3 = word(12); \
        const unsigned long long cs_ = word(13); \
        count = (int)(unsigned int)cs_; \
        source = (int)(unsigned int)(cs_ >> 32); \
        _Pragma("unroll") \
        for (int w = 0; w < SEENW; w++) seen.w[w] = word(kCarryBase + w); \
        if constexpr (RECORD) { \
            const unsigned long long rn_ = word(kCarryBase + SEENW); \
            rec_slot = (int)(unsigned int)rn_; \
            nev = (int)(unsigned int)(rn_ >> 32); \
        } \
        if constexpr (ROUGH) { \
            if (uf(UF_CAPTURE)) gidx = word(base); \
            if (uf(UF_COUNT)) hcount = word((base) + 1); \
            if (uf(UF_ORIGIN)) { \
                const int at = uf(UF_COUNT) ? (base) + kCountWords : (base); \
                origin_put(pvt_u2d(word(at)), pvt_u2d(word(at + 1)), pvt_u2d(word(at + 2)), pvt_u2d(word(at + 3))); \
            } \
        } \
    }

#if PVT_STATS
    unsigned long long st_iters = 0, st_lane_steps = 0, st_drain_iters = 0, st_drain_lane_steps = 0;
    unsigned long long st_t[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_mark = 0;
#define PVT_MARK(k) do { unsigned long long now_ = __builtin_readcyclecounter(); if (ws & WS_SOLO) st_t[k] += now_ - st_mark; st_mark = now_; } while (0)
    unsigned long long st_c[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // bulk-phase lane counts per section
    unsigned long long st_g[4] = {0, 0, 0, 0};   // grid walk: cell rounds, node-test trips (per wave), node tests, cell steps (per lane)
#define PVT_COUNT(k, pred) do { unsigned long long b_ = __ballot(pred); if (!(ws & WS_EXHAUSTED)) st_c[k] += __popcll(b_); } while (0)
#else
#define PVT_MARK(k) do {} while (0)
#define PVT_COUNT(k, pred) do {} while (0)
#endif
    // wave-uniform ray window claimed from the global cursor
    // (the waves of a launch -- of a tally set -- are numbered; wave k owns rays [k kClaim, (k+1) kClaim) and parked
    // photons [64 k, 64 k + 64) without asking, everything beyond is claimed from the cursors)
    const unsigned int wgs_in_set = A.set_size ? (unsigned int)A.wgs_per_set : gridDim.x;
    const unsigned int waves_in_set = wgs_in_set * kWaves;
    const unsigned int wave_in_set = (blockIdx.x - set * (A.set_size ? (unsigned int)A.wgs_per_set : 0u)) * kWaves +
                                     (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned int w_first = wave_in_set * (unsigned int)kClaim;
    unsigned int w_next = w_first, w_end = w_first, w_base = 0;
    unsigned int w_claim_end = w_first < n_local ? (n_local - w_first < (unsigned int)kClaim ? n_local : w_first + kClaim) : w_first;
    unsigned int c_next = 0, c_end = 0;   // window of parked photons
    // The wave's own yes/no state, one bit each in ONE scalar register (as separate flags each is a 64-bit lane mask
    // held -- or spilled -- across the whole loop): the ray cursor is dry; that has been counted in the workgroup;
    // in the drain rendezvous; last wave standing; parked photons may still be waiting; first claim of them
    enum { WS_EXHAUSTED = 1, WS_COUNTED = 2, WS_REGIME = 4, WS_SOLO = 8, WS_CARRY_IN = 16, WS_C_FIRST = 32 };
    unsigned int ws = WS_C_FIRST | ((!RECORD && (A.carry_flags & 1) != 0) ? WS_CARRY_IN : 0u);
    // Per-wave pool of ready-made RNG states for the claimed chunk (4 x 64 u64 = 2 KB).  It lives
    // in the photon-exchange buffer: that buffer is first used when ALL waves of the workgroup
    // have run the cursor dry, i.e. after every pool has been consumed.
    const bool seed_pool = A.xslots * (14 + SEENW) >= kWaves * 4 * 64;
    const int pool_at = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * 4 * 64;   // wave-uniform
    // drain-phase consolidation state (all wave-uniform)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int members = 0, parity = 0;
    int tail_n = 0;   // photons this wave hands to the tail function when it leaves the loop (0: none)
    // (mesh scenes never repack a draining workgroup -- KArgs::xslots is 0 there -- and the history variant of the grid walk
    // has no register to spare for the call: both keep their last wave in this loop)
    constexpr bool kTailCall = !TAIL && !MESH && !(GRID && RECORD) && !PARK;

    // Statistics of the parked first crossings, one lane per record: the recorder's distinct count, the
    // eight running sums (the angle is acos of the parked cosine; 1.0 -> exactly 0 for events without a
    // normal) and its histograms.  Runs when the queue cannot take another trip, i.e. with ~60 busy lanes
    // instead of the handful that cross a recorder in any one step, and once more when the wave retires.
    auto tally_flush = [&]() {
        if (lane < tq_n) {
            const int r = tq_r[lane];
            // (the parked cosine is t_cos, clamped to [0, 1] where the step forms it: pvt_acos_unit's domain)
            const double q_wl = tq_d[lane], q_angle = pvt_acos_unit(tq_d[kTallyQ + lane]);
            const double q_duration = tq_d[2 * kTallyQ + lane], q_travelled = tq_d[3 * kTallyQ + lane];
            const int ri = L.rec_i + r * RI;
            atomicAdd(&acc_distinct[r], 1u);
            double* sp = acc_sums + r * 8;
            atomicAdd(&sp[0], q_wl); atomicAdd(&sp[1], q_wl * q_wl);
            atomicAdd(&sp[2], q_angle); atomicAdd(&sp[3], q_angle * q_angle);
            atomicAdd(&sp[4], q_duration); atomicAdd(&sp[5], q_duration * q_duration);
            atomicAdd(&sp[6], q_travelled); atomicAdd(&sp[7], q_travelled * q_travelled);
            const int h0 = T.iv(ri + RI_HSTART), h1 = h0 + T.iv(ri + RI_HN);
            for (int h = h0; h < h1; h++) {
                const int hi_ = L.hist_i + h * HI, hd_ = L.hist_d + h * HD;
                const int pa = T.iv(hi_ + HI_PA), pb = T.iv(hi_ + HI_PB);
                const int na = T.iv(hi_ + HI_NA), nb = T.iv(hi_ + HI_NB);
                auto prop = [&](int pr) -> double {
                    if (pr < 4) return pr == 0 ? q_wl : pr == 1 ? q_angle : pr == 2 ? q_duration : q_travelled;
                    if constexpr (ROUGH) {
                        // a launch origin (ids 10-13; the host lets none in unless its bit of KArgs::origin is set): its column
                        if (pr >= 10)
                            return tq_d[tq_count_at + ((uf(UF_TQ_COUNT) ? 1 : 0) + __builtin_popcount(origin_mask() & ((1u << (pr - 10)) - 1u))) * kTallyQ + lane];
                        // an event counter (ids 7-9; the host lets none in unless UF_TQ_COUNT): its field of the packed word
                        if (pr >= 7)
                            return (double)(unsigned int)((pvt_d2u(tq_d[tq_count_at + lane]) >> ((pr - 7) * kCountBits)) & ((1u << kCountBits) - 1u));
                    }
                    return tq_d[pr * kTallyQ + lane];   // x, y, z in the recorder node's frame (A.tq_pos)
                };
                const double la = T.dv(hd_ + HD_LO_A), ha = T.dv(hd_ + HD_HI_A);
                const double ra = T.dv(hd_ + HD_RA);
                const double qa = ra == ra ? div_known(prop(pa) - la, ha - la, ra) : (prop(pa) - la) / (ha - la);
                const int ia = (int)(qa * na);
                if (ia < 0 || ia >= na) continue;
                int slot = T.iv(hi_ + HI_OFF) + ia;
                if (pb >= 0) {
                    const double lb = T.dv(hd_ + HD_LO_B), hb = T.dv(hd_ + HD_HI_B);
                    const double rb = T.dv(hd_ + HD_RB);
                    const double qb = rb == rb ? div_known(prop(pb) - lb, hb - lb, rb) : (prop(pb) - lb) / (hb - lb);
                    const int ib = (int)(qb * nb);
                    if (ib < 0 || ib >= nb) continue;
                    slot = T.iv(hi_ + HI_OFF) + ia * nb + ib;
                }
                if (uf(UF_BINS_LDS)) atomicAdd(&acc_bins[slot], 1u);
                else atomicAdd(reinterpret_cast<unsigned long long*>(A.rec_bins) + (long long)set * A.set_stride_i + slot, 1ull);
            }
        }
        tq_n = 0;
    };
    if constexpr (TAIL) {   // the photons the caller left in the exchange buffer, one per lane
        const int slot = lane;
        ws = WS_EXHAUSTED | WS_COUNTED | WS_SOLO;
        alive = slot < tail_total;
        if (alive) {
            PVT_PHOTON_GET(PVT_SLOT_WORD, kXWords)
        }
    }
    if constexpr (TAIL) ac_lds[0] = ~0ull;   // (nothing known yet; after the reads above, same wave: in order)
    for (;;) {
        if constexpr (TAIL) {
            if (__ballot(alive) == 0ull) break;
        }
        if constexpr (!TAIL) {
        // ================= refill dead lanes ==============================
        unsigned long long need = __ballot(!alive);
        if constexpr (!RECORD) {
            // photons parked by the previous launch on this stream come first (see KArgs::carry_in).  They are handed
            // out like rays, 64 at a time: every wave starts with the slice its index names (no atomic -- the previous
            // launch parked at most 64 per wave, so with an equal or larger grid that is all of them); only what lies
            // beyond is claimed through the claim cursor, one atomic per 64.  (A claim per refill, for just the lanes
            // that died in the last step, put a queue of ~10^5 same-address atomics in front of every step: measured
            // 21 us per iteration instead of 11.)
            if ((ws & WS_CARRY_IN) && need != 0ull) {
                PVT_KERNEL_ARGS_OPAQUE(ak);
                const unsigned int have = *ak->carry_in_count;
                if (c_next >= c_end) {
                    unsigned int b = ~0u;
                    if (ws & WS_C_FIRST) {
                        ws &= ~(unsigned int)WS_C_FIRST;
                        b = wave_in_set * 64u;
                    } else if (have > waves_in_set * 64u) {
                        if (lane == 0) b = atomicAdd(cursor + 1, 64u);
                        b = __builtin_amdgcn_readfirstlane(b) + waves_in_set * 64u;
                    }
                    if (b >= have) {
                        ws &= ~(unsigned int)WS_CARRY_IN;
                    } else {
                        c_next = b;
                        c_end = have - b < 64u ? have : b + 64u;
                    }
                }
                if (ws & WS_CARRY_IN) {
                    const unsigned int want = __popcll(need), got = c_end - c_next < want ? c_end - c_next : want;
                    const unsigned int rank = rank_in(need);
                    if (!alive && rank < got) {
                        const unsigned long long* src = ak->carry_in + (unsigned long long)(c_next + rank) * ((ROUGH && uf(UF_COUNT) ? kCarryStride + kCountWords : kCarryStride) + (ROUGH && uf(UF_ORIGIN) ? kOriginWords : 0));
                        PVT_PHOTON_GET(PVT_SRC_WORD, kCarryStride)
                        nev = 0;
                        alive = true;
                    }
                    c_next += got;
                    need = __ballot(!alive);
                }
            }
        }
        for (int pass = 0; pass < 2 && need != 0ull; pass++) {
            if (w_next >= w_end) {
                if (ws & WS_EXHAUSTED) break;
                unsigned int b = w_end;          // next chunk of the rays this wave has claimed ...
                if (b >= w_claim_end) {          // ... or a new claim (the first one is the wave's own index: no atomic;
                                                 // 4096 waves starting together on ONE word cost the launch ~50 us)
                    // (Smaller claims towards the end of the rays -- a wave that takes the last 64 rays runs some six
                    // iterations longer than its neighbours, which found the cursor dry -- were measured and NOT kept:
                    // with claims of 32 / 16 rays in the last two rounds the pipelined bench lost 4 % / 13 %, the extra
                    // same-address atomics cost more than the ragged end.  Between two claims of a wave every other
                    // wave claims about once, so the cursor stands near w_claim_end + waves x 64 now.)
                    const unsigned int claim = (n_local - w_claim_end > 2u * waves_in_set * (unsigned int)kClaim || w_claim_end > n_local)
                                                   ? (unsigned int)kClaim : (unsigned int)kEndClaim;
                    unsigned int c = 0;
                    if (lane == 0) c = atomicAdd(cursor, claim);
                    c = __builtin_amdgcn_readfirstlane(c) + waves_in_set * (unsigned int)kClaim;
                    if (c >= n_local) { ws |= WS_EXHAUSTED; break; }
                    b = c;
                    w_claim_end = (n_local - c < claim) ? n_local : c + claim;
                }
                w_next = b;
                w_end = (w_claim_end - b < (unsigned int)kChunk) ? w_claim_end : b + kChunk;
                w_base = b;
                if constexpr (EMIT) {
                    // sample the whole chunk now (see KArgs::emit_pool); the stores are read back by lanes of this very
                    // wave, later in program order
                    PVT_KERNEL_ARGS_OPAQUE(ak);
                    unsigned int lane_here = (unsigned int)lane;
                    asm volatile("" : "+v"(lane_here));
                    if (b + lane_here < w_end) {
                        double* pool = ak->emit_pool + ((unsigned long long)blockIdx.x * kWaves + (unsigned long long)wave) * (7 * 64) + lane_here;
                        const unsigned long long gi_ = A.ray_offset + (unsigned long long)ray_lo + (unsigned long long)b + (unsigned long long)lane_here;
                        if constexpr (PARK) emit_chunk_park((const KArgs*)ak, gi_, pool);
                        else emit_chunk((const KArgs*)ak, gi_, pool);
                    }
                }
                // (GIVEN rays are not staged like this.  Copying a chunk's 64 rays into the pool here, coalesced, and
                // refilling from L2 was built and measured for the lean kernels: 2.4 % slower than reading the arrays in
                // the refill, in 10 of 10 alternated runs -- the other waves of the SIMD already cover the refill's
                // misses, and the copy is seven more loads and stores per chunk.  profiles/staged_refill.md)
                if (seed_pool) {
                    // Seed the whole chunk NOW, with every lane busy, instead of inside each later
                    // refill with only the dead lanes active (8 64-bit multiplies per seed): lane l
                    // prepares the stream of ray b + l and parks it in this wave's slice of LDS.
                    // (the lane number behind an opaque copy: hoisted out of the loop, seed + ray_lo + lane would sit in two
                    // vector registers for the whole kernel, which has none to spare)
                    unsigned int lane_here = (unsigned int)lane;
                    asm volatile("" : "+v"(lane_here));
                    unsigned long long st = A.seed + (unsigned long long)ray_lo + (unsigned long long)b + (unsigned long long)lane_here;
#pragma unroll
                    for (int k = 0; k < 4; k++) {   // one word at a time: keeps the live range short
                        xbuf[pool_at + k * 64 + lane] = splitmix64(st);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            unsigned int avail = w_end - w_next;
            unsigned int rank = rank_in(need);
            unsigned int want = __popcll(need);
            if (!alive && rank < avail) {
                const unsigned int il = w_next + rank;   // index within the set
                const unsigned int i = ray_lo + il;      // index within the launch
                if constexpr (EMIT) {
                    PVT_KERNEL_ARGS_OPAQUE(ak);
                    const double* pool = ak->emit_pool + ((unsigned long long)blockIdx.x * kWaves + (unsigned long long)wave) * (7 * 64) + (il - w_base);
                    pos = V3{pool[0], pool[64], pool[128]};
                    dir = V3{pool[192], pool[256], pool[320]};
                    wl = pool[384];
                } else {
                    // The three ray pointers are read from the kernel-argument segment HERE, through a pointer
                    // the compiler cannot trace back to it: kept as loop invariants they would sit in six
                    // scalar registers the loop is short of (spilled to VGPR lanes, each use a VALU
                    // v_readlane); scalar loads cost the vector pipe nothing.
                    PVT_KERNEL_ARGS_OPAQUE(ak);
                    const double* rp = ak->pos;
                    const double* rd = ak->dir;
                    const double* rw = ak->wl;
                    pos = V3{rp[i * 3ull], rp[i * 3ull + 1], rp[i * 3ull + 2]};
                    dir = V3{rd[i * 3ull], rd[i * 3ull + 1], rd[i * 3ull + 2]};
                    wl = rw[i];
                }
                if (seed_pool) {
                    const int k = pool_at + (int)(il - w_base);
                    rng.s0 = xbuf[k]; rng.s1 = xbuf[k + 64]; rng.s2 = xbuf[k + 128]; rng.s3 = xbuf[k + 192];
                } else {
                    rng_seed(rng, A.seed + (unsigned long long)i);
                }
                travelled = 0.0;
                duration = 0.0;
                count = 0;
                source = -1;
                nev = 0;
                if constexpr (ROUGH) {
                    if (uf(UF_CAPTURE)) gidx = A.ray_offset + (unsigned long long)i;
                    if (uf(UF_COUNT)) hcount = 0ull;
                    if (uf(UF_ORIGIN)) origin_put(wl, pos.x, pos.y, pos.z);   // (as read above: the GENERATE row's values)
                }
#pragma unroll
                for (int w = 0; w < SEENW; w++) seen.w[w] = 0ull;
                alive = true;
                if constexpr (RECORD) {
                    rec_slot = -1;
                    if (A.record_every > 0 && (long long)i % A.record_every == 0) rec_slot = (int)((long long)i / A.record_every);
                    log_row<RECORD, TAIL>(A, rec_slot, nev, PVT_EV_GENERATE, -1, -1, -1, -1, source, pos, dir, false,
                                    pos, wl, travelled, duration);
                }
            }
            w_next += (want < avail) ? want : avail;
            need = __ballot(!alive);
        }
        // ================= drain: repack the workgroup's survivors ==========
        // Once the ray cursor is dry a wave can only lose lanes; with 4 waves per workgroup
        // each at a handful of live lanes, most issue slots would be spent on idle lanes
        // (measured: 55 % of all wave-iterations of a 10^6-photon launch ran at 11 live lanes).
        // So when ALL waves of the workgroup are draining they rendezvous each iteration
        // (s_barrier), publish their live counts, and as soon as the survivors fit into fewer
        // waves every live photon's state is moved through LDS into the lowest waves and the
        // emptied waves retire.  Which lane carries a photon never affects its history (RNG
        // stream, seen-mask and log rows travel with it), so results stay bit-identical.
        if constexpr (!RECORD) {
            if ((ws & WS_EXHAUSTED) && (PARK || (A.carry_flags & 2))) {
                // no rays left for this wave: its live photons are parked for the next launch on the stream
                const unsigned long long live_mask = __ballot(alive);
                if (live_mask != 0ull) {
                    PVT_KERNEL_ARGS_OPAQUE(ak);
                    unsigned int b = 0;
                    if (lane == 0) b = atomicAdd(cursor + 2, (unsigned int)__popcll(live_mask));
                    b = __builtin_amdgcn_readfirstlane(b);
                    const unsigned int at = b + rank_in(live_mask);
                    if (alive && at < ak->carry_cap) {
                        unsigned long long* dst = ak->carry_out + (unsigned long long)at * ((ROUGH && uf(UF_COUNT) ? kCarryStride + kCountWords : kCarryStride) + (ROUGH && uf(UF_ORIGIN) ? kOriginWords : 0));
                        PVT_PHOTON_PUT(PVT_DST_WORD, kCarryStride)
                    }
                    alive = false;   // (the wave leaves through the "nothing alive, no rays left" exit below)
                }
            }
        }
        if constexpr (PARK) {
            // (parked above, or nothing was alive: either way the wave is done -- the exit the other entries take through
            // "nothing alive, no rays left", without the workgroup's count of dry waves that only the drain reads)
            if (ws & WS_EXHAUSTED) break;
            if (__ballot(alive) == 0ull) break;
        } else {
        if ((ws & (WS_EXHAUSTED | WS_COUNTED)) == WS_EXHAUSTED) {
            ws |= WS_COUNTED;
            if (lane == 0) atomicAdd(&ctl[CTL_EXHAUSTED], 1);
        }
        if (!(ws & WS_REGIME)) {
            if (__ballot(alive) == 0ull) break;  // wave drained and cursor exhausted
            // (values read back from LDS are made scalars explicitly -- readfirstlane -- so that the state they
            // decide stays in scalar registers)
            if (A.xslots > 0 && (ws & (WS_EXHAUSTED | WS_SOLO)) == WS_EXHAUSTED &&
                __builtin_amdgcn_readfirstlane(__hip_atomic_load(&ctl[CTL_EXHAUSTED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == kWaves) {
                ws |= WS_REGIME;
                if (lane == 0) ctl[CTL_IN + wave] = 1;
                __syncthreads();  // R0: everybody still running is now in lock-step
                members = __builtin_amdgcn_readfirstlane((ctl[CTL_IN] ? 1 : 0) | (ctl[CTL_IN + 1] ? 2 : 0) | (ctl[CTL_IN + 2] ? 4 : 0) |
                                                         (ctl[CTL_IN + 3] ? 8 : 0));
            }
        }
        if (ws & WS_REGIME) {
            const unsigned long long live_mask = __ballot(alive);
            const int live = __popcll(live_mask);
            int* live_tab = ctl + CTL_LIVE + parity * kWaves;  // double-buffered by iteration parity
            parity ^= 1;
            if (lane == 0) live_tab[wave] = live;
            __syncthreads();  // A
            int l[kWaves], total = 0, nw = 0, before = 0, pos_in_set = 0;
#pragma unroll
            for (int w = 0; w < kWaves; w++) {
                l[w] = ((members >> w) & 1) ? __builtin_amdgcn_readfirstlane(live_tab[w]) : 0;
                if (l[w] == 0) members &= ~(1 << w);  // that wave retires now (it sees its own 0)
                else {
                    if (w < wave) { before += l[w]; pos_in_set += 1; }
                    total += l[w];
                    nw += 1;
                }
            }
            if (live == 0) break;
            if (nw == 1) {
                ws = (ws & ~(unsigned int)WS_REGIME) | WS_SOLO;  // last wave standing: no more rendezvous
                // ... and no more rays: the rest of its photons' histories runs in the tail function (the loop without
                // the refill and the rendezvous, a function of its own: it cannot move this loop's registers); the
                // photons go through the exchange buffer, as in a consolidation
                if constexpr (kTailCall) {
                    if (alive) {
                        const int slot = (int)rank_in(live_mask);
                        PVT_PHOTON_PUT(PVT_SLOT_WORD, kXWords)
                    }
                    tail_n = live;   // (the call itself comes after the loop: nothing of the loop is live across it)
                    alive = false;
                    break;
                }
            } else if (total <= 64 * (nw - 1) && total <= A.xslots) {
                if (alive) {
                    const int slot = before + (int)rank_in(live_mask);
                    PVT_PHOTON_PUT(PVT_SLOT_WORD, kXWords)
                }
                __syncthreads();  // B
                const int keep = (total + 63) >> 6;  // waves that stay, lowest ids of the set
                if (pos_in_set >= keep) { alive = false; break; }
                if constexpr (kTailCall) {
                    if (keep == 1) {   // the survivors fit one wave: this one, in the tail function (see above)
                        tail_n = total;
                        alive = false;
                        break;
                    }
                }
                const int slot = pos_in_set * 64 + lane;
                alive = slot < total;
                if (alive) {
                    PVT_PHOTON_GET(PVT_SLOT_WORD, kXWords)
                }
                // the set shrinks to its `keep` lowest members
                int kept = 0, m2 = 0;
#pragma unroll
                for (int w = 0; w < kWaves; w++)
                    if (((members >> w) & 1) && kept < keep) { m2 |= 1 << w; kept += 1; }
                members = m2;
                if (keep == 1) ws = (ws & ~(unsigned int)WS_REGIME) | WS_SOLO;
            }
        }
        }   // (!PARK)
        }   // (!TAIL)
#if PVT_STATS
        {
            unsigned long long live = __popcll(__ballot(alive));
            st_iters += 1; st_lane_steps += live;
            if (ws & WS_EXHAUSTED) { st_drain_iters += 1; st_drain_lane_steps += live; }
        }
#endif

        c_iters += 1u;
#if PVT_TIMELINE
        if (tl_iters == 0) tl_t[2] = wall_clock64();
        if ((ws & WS_EXHAUSTED) && tl_t[3] == 0) tl_t[3] = wall_clock64();
        tl_iters += 1;
#endif
        PVT_MARK(0);  // refill + drain bookkeeping
        PVT_COUNT(0, alive);
        // ================= one step for every live lane ==================
        // deferred event of this step
        int ev_kind = -1, ev_hit = -1, ev_container = -1, ev_adjacent = -1, ev_component = -1;
        bool ev_normal = false, terminal = false;
        int t_sel = -1, t_node = -1;
        bool t_normal = false;
        double t_cos = 1.0;   // cosine of the angle the tallies record (acos is taken when a recorder needs it)
        V3 nrm{0, 0, 0};
        int tri1 = -1;   // triangle record of the nearest crossing when it lies on a mesh
        bool em = false;   // re-emitted in this step

        // ---- stage 1: where does the ray go?  (every live lane) ------------------------------------
        // Lane classes for the rest of the step; the divergent bodies below are keyed on them.
        enum { CLS_NONE = 0, CLS_SURF, CLS_EXIT, CLS_ABS };
        int cls = CLS_NONE;
        int hit = -1, container = -1, adjacent = -1;
        double t0 = 0.0;
        bool pend = false;   // reaches the exit / absorption / surface decision
        if (alive) {
            count += 1;
            bool budget_kill = false;
            if constexpr (RECORD) budget_kill = (rec_slot >= 0 && nev >= A.max_events - 1);
            if (budget_kill) {
                // event budget exhausted: KILL row, no tally (_kernel.pyx:658-663)
                ev_kind = PVT_EV_KILL;
                terminal = true;
            } else {
                // ---- intersect every node, fold nearest/second/container ----
                int nhits = 0, n1 = -1, n2 = -1, cnode = -1;
                tri1 = -1;
                double t1 = INFINITY, t2 = INFINITY, cbest = INFINITY;
                int c2node = -1;            // (mesh scenes) the next-nearest node that holds the ray
                double c2best = INFINITY;
                V3 d{0, 0, 0};
                double inv[3] = {0, 0, 0};
                bool inv_ok = false;   // wave-uniform
                int rot = -1;          // rotation class of `d` (wave-uniform)
                // The root last.  Every photon is inside the root, which therefore contributes exactly one
                // forward crossing, farther than any crossing of a node that lies strictly inside it (the
                // host has checked that with a margin: no ties, so the visiting order cannot matter).  All the
                // rest of the step needs from that crossing is its ORDER among the others -- unless it is the
                // nearest one (the photon leaves the scene) and somebody looks at where it leaves (an event
                // log, an `exit` recorder), in which case this launch was not given `lazy_root`.  So the lanes
                // compare the crossings they have with a cheap lower bound of the root's distance -- the
                // distance to the root's nearest face -- and only the lanes it cannot decide for pay for the
                // root's intersection; in a typical scene (a 5 cm slab in a 5 m world) none ever does.
                // (tail function: also where exits are looked at -- `lazy_exact`: the root's own distance is worked out whenever
                // it is the nearest crossing, i.e. the photon leaves the scene)
                const bool lazy_exact = TAIL && !MESH && (uf(UF_TAIL_LAZY1) || uf(UF_TAIL_LAZY2));
                const int lazy_root = MESH ? 0 : (lazy_exact ? (uf(UF_TAIL_LAZY1) ? 1 : 2)
                                                              : (RECORD ? 0 : (uf(UF_LAZY1) ? 1 : (uf(UF_LAZY2) ? 2 : 0))));   // wave-uniform
                // Grid scenes fold a crossing by the key (t, node): what the reference's first-minimum scans over its hit
                // list (nodes ascending) come to, whatever the order the nodes are visited in.  Written as selects of
                // VALUES: as branches that assign, the compiler merges the assignments into stores through a selected
                // POINTER, and nearest / second-nearest then live in scratch memory.
                // (Every captured variable is read ONCE, up front, and written once at the end: a lambda's body is optimised
                // before it is inlined, while its captures are still pointers, and a choice between two of them read in
                // different branches becomes a load through a chosen pointer -- which pins them to memory for good.)
                auto fold_by_key = [&](double t, int node, int& nl, double& tfirst) __attribute__((always_inline)) {
                    const double a1 = t1, a2 = t2, tf = tfirst;
                    const int m1 = n1, m2 = n2, have = nhits, l = nl;
                    const bool none = have == 0;
                    const bool nearest = none || t < a1 || (t == a1 && node < m1);
                    const bool second = !nearest && (m2 < 0 || t < a2 || (t == a2 && node < m2));
                    const bool shift = nearest && !none;
                    tfirst = l == 0 ? t : tf;
                    nl = l + 1;
                    t1 = nearest ? t : a1;
                    n1 = nearest ? node : m1;
                    t2 = shift ? a1 : (second ? t : a2);
                    n2 = shift ? m1 : (second ? node : m2);
                    nhits = have + 1;
                };
                if constexpr (GRID) {
                    // ---- scenes of many nodes: every lane looks up ITS candidates in a uniform grid over the nodes -----
                    // The reference intersects every node in every step (_kernel.pyx:666-680).  A node the ray does not
                    // cross contributes nothing to that loop, and all the step needs of the others is the nearest and
                    // the second-nearest crossing and the nearest node crossed exactly once.  The host files every
                    // node but the root under the cells of a grid that its bounding box (grown by a margin far above
                    // rounding) touches; a lane walks the cells its ray passes, front to back (3-D DDA), and runs the
                    // reference's own intersection arithmetic on the nodes it finds there, each once.  Crossings are
                    // folded by (t, node) -- the order the reference's first-minimum scans imply -- so the visiting
                    // order cannot matter.  The walk ends where the ray leaves the grid, or earlier: once two
                    // crossings lie nearer than the end of the cells visited (by `guard`, the margin again), every
                    // node not yet seen has all its crossings beyond them -- it cannot be the nearest or the second
                    // -- and lies clear of the photon, so a convex box or sphere is crossed twice or not at all and
                    // cannot hold the ray either.  (A cylinder grazed at the rim of a cap may come out with ONE
                    // crossing in the reference's arithmetic, _kernel.pyx:301-345: scenes with cylinders -- `odd` --
                    // additionally walk on until the cells visited reach past the container found so far.)
                    const int gb = L.grid_d;
                    const unsigned long long gbits = pvt_d2u(T.du(gb + 13));   // nx | ny << 8 | nz << 16 | words << 24 | odd << 28
                    const double guard = T.du(gb + 12);
                    // (everything the walk keeps is a named scalar: a local array that is selected from or passed by reference
                    // ends up in scratch memory, and a scratch access is a trip to the memory system in the middle of the walk)
                    const double invw0 = rcp_normal(dir.x), invw1 = rcp_normal(dir.y), invw2 = rcp_normal(dir.z);
                    const double invw[3] = {invw0, invw1, invw2};   // (set-up only, fully unrolled)
                    const double pw[3] = {pos.x, pos.y, pos.z}, dw[3] = {dir.x, dir.y, dir.z};
                    // the ray against the grid's box (a direction component this small moves the photon by less than
                    // rounding over the whole scene: treated as parallel)
                    double t_in = 0.0, t_out = INFINITY;
                    bool walk = true;
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const double lo = T.du(gb + a), hi = T.du(gb + 3 + a);
                        if (pvt_fabs(dw[a]) < 1e-20) {
                            if (pw[a] < lo || pw[a] > hi) walk = false;
                        } else {
                            const double ta = (lo - pw[a]) * invw[a], tb = (hi - pw[a]) * invw[a];
                            t_in = __builtin_fmax(t_in, __builtin_fmin(ta, tb));
                            t_out = __builtin_fmin(t_out, __builtin_fmax(ta, tb));
                        }
                    }
                    if (!(t_in <= t_out)) walk = false;
                    // first cell, the distance at which the ray leaves it along each axis, steps left along each axis
                    double tm0 = INFINITY, tm1 = INFINITY, tm2 = INFINITY;
                    unsigned int remv = 0;   // steps left: x | y << 8 | z << 16; bits 24-26: the ray runs towards lower indices
                    int ci = 0;
                    {
                        int stride = 1;
#pragma unroll
                        for (int a = 0; a < 3; a++) {
                            const int na = (int)((unsigned int)(gbits >> (8 * a)) & 0xffu);
                            const double lo = T.du(gb + a), cell = T.du(gb + 6 + a), rcell = T.du(gb + 9 + a);
                            const double at = pw[a] + dw[a] * t_in;
                            int c = (int)((at - lo) * rcell);
                            c = c < 0 ? 0 : (c > na - 1 ? na - 1 : c);
                            const bool par = pvt_fabs(dw[a]) < 1e-20, neg = dw[a] < 0.0;
                            const double tma = par ? INFINITY : ((lo + (double)(c + (neg ? 0 : 1)) * cell) - pw[a]) * invw[a];
                            if (a == 0) tm0 = tma; else if (a == 1) tm1 = tma; else tm2 = tma;
                            remv |= (unsigned int)(neg ? c : na - 1 - c) << (8 * a);
                            if (neg) remv |= 1u << (24 + a);
                            ci += c * stride;
                            stride *= na;
                        }
                    }
                    const int words = (int)((unsigned int)(gbits >> 24) & 0xfu);
                    const bool odd = ((gbits >> 28) & 1ull) != 0;
                    unsigned long long seen_lo = 0ull, seen_hi = 0ull;   // nodes this lane has tested in this step
                    // (always_inline: a closure that is CALLED holds pointers to the variables it captured, which then live in
                    // scratch memory)
                    // one node, tested by this lane alone (the records come from LDS with per-lane addresses)
                    // One node, tested by this lane alone (records from LDS with per-lane addresses).  The root comes last
                    // and goes through here too -- with the lazy shortcut of the plain node loop below, when the launch
                    // has it -- so the intersection code exists once in the kernel's text.
                    auto visit = [&](int node) __attribute__((always_inline)) {
                        const int hn = node * ND;
                        const double tx = T.dv(hn + ND_T), ty = T.dv(hn + ND_T + 1), tz = T.dv(hn + ND_T + 2);
                        const double g0 = T.dv(hn + ND_PARAMS), g1 = T.dv(hn + ND_PARAMS + 1), g2 = T.dv(hn + ND_PARAMS + 2);
                        const unsigned long long hb = pvt_d2u(T.dv(hn + ND_BITS));
                        int gt = (int)(((unsigned int)hb >> 8) & 0xffu);
                        V3 o, dl;
                        double il0, il1, il2;
                        if ((hb & 1ull) != 0) {
                            o.x = pos.x + tx; o.y = pos.y + ty; o.z = pos.z + tz;
                            dl = dir;
                            il0 = invw0; il1 = invw1; il2 = invw2;
                        } else {
                            const int rm = L.rot_d + (int)(unsigned int)(hb >> 32) * RT + RT_W2L;
                            o.x = T.dv(rm + 0) * pos.x + T.dv(rm + 1) * pos.y + T.dv(rm + 2) * pos.z + tx;
                            o.y = T.dv(rm + 3) * pos.x + T.dv(rm + 4) * pos.y + T.dv(rm + 5) * pos.z + ty;
                            o.z = T.dv(rm + 6) * pos.x + T.dv(rm + 7) * pos.y + T.dv(rm + 8) * pos.z + tz;
                            dl.x = T.dv(rm + 0) * dir.x + T.dv(rm + 1) * dir.y + T.dv(rm + 2) * dir.z;
                            dl.y = T.dv(rm + 3) * dir.x + T.dv(rm + 4) * dir.y + T.dv(rm + 5) * dir.z;
                            dl.z = T.dv(rm + 6) * dir.x + T.dv(rm + 7) * dir.y + T.dv(rm + 8) * dir.z;
                            il0 = rcp_normal(dl.x); il1 = rcp_normal(dl.y); il2 = rcp_normal(dl.z);
                        }
                        bool root_known = false;
                        if (lazy_root && node == k_root) {   // (see the plain node loop: same bound, same conditions)
                            double bound;
                            if (lazy_root == 1) {
                                bound = __builtin_fmin(__builtin_fmin(0.5 * g0 - pvt_fabs(o.x), 0.5 * g1 - pvt_fabs(o.y)), 0.5 * g2 - pvt_fabs(o.z));
                            } else {
                                bound = (g0 * g0 - dot3(o, o)) * A.lazy_k;
                            }
                            const bool undecided = !(bound > 0.0) || (nhits > 0 && !(t1 < bound)) || (nhits >= 2 && !(t2 < bound)) ||
                                                   (cnode >= 0 && !(cbest < bound)) || (lazy_exact && nhits == 0);
                            {   // one more crossing, behind all the others: nearest only if there is no other
                                const double a1 = t1, a2 = t2;
                                const int m1 = n1, m2 = n2, have = nhits, cn = cnode;
                                const bool known = !undecided;
                                t1 = known && have == 0 ? bound : a1; n1 = known && have == 0 ? node : m1;
                                t2 = known && have == 1 ? INFINITY : a2; n2 = known && have == 1 ? node : m2;
                                nhits = have + (known ? 1 : 0);
                                cnode = known && cn < 0 ? node : cn;   // crossed once: it holds the ray unless a nearer node does
                                root_known = known;
                                gt = known ? -1 : gt;   // nothing to intersect
                            }
                        }
                        int nl = 0;
                        double tfirst = 0.0;
                        auto fold = [&](double t) __attribute__((always_inline)) { fold_by_key(t, node, nl, tfirst); };
                        if (gt >= 0) shape_hits(gt, g0, g1, g2, o, dl, il0, il1, il2, fold);
                        {
                            const double cb = cbest;
                            const int cn = cnode;
                            const bool holds = nl == 1 && !root_known && (tfirst < cb || (tfirst == cb && node < cn));
                            cbest = holds ? tfirst : cb;
                            cnode = holds ? node : cn;
                        }
                    };
                    auto next_cell = [&]() __attribute__((always_inline)) {   // leave the current cell: done, or on to the next one
                        const double t_cell = __builtin_fmin(tm0, __builtin_fmin(tm1, tm2));   // the ray leaves the cell here
                        const bool enough = nhits >= 2 && t2 + guard < t_cell && (!odd || (cnode >= 0 && cbest + guard < t_cell));
                        const int ax = (tm0 <= tm1 && tm0 <= tm2) ? 0 : (tm1 <= tm2 ? 1 : 2);
                        const unsigned int left = (remv >> (8 * ax)) & 0xffu;
                        if (enough || left == 0u || !(t_cell < INFINITY)) {
                            walk = false;
                        } else {
                            remv -= 1u << (8 * ax);
                            const int nx = (int)((unsigned int)gbits & 0xffu), ny = (int)((unsigned int)(gbits >> 8) & 0xffu);
                            const int stride = ax == 0 ? 1 : (ax == 1 ? nx : nx * ny);
                            ci += ((remv >> (24 + ax)) & 1u) ? -stride : stride;
                            if (ax == 0) tm0 = __builtin_fma(pvt_fabs(invw0), T.du(gb + 6), tm0);
                            else if (ax == 1) tm1 = __builtin_fma(pvt_fabs(invw1), T.du(gb + 7), tm1);
                            else tm2 = __builtin_fma(pvt_fabs(invw2), T.du(gb + 8), tm2);
                        }
                    };
                    // Every lane at its own pace.  A trip: a lane whose current cell holds nothing it has not tested moves on to
                    // its next cell (or out of the walk); then it tests ONE node -- of the cell it is in now or, the walk
                    // over, the root.  (Both halves run in every trip of a wave anyway, its lanes being at different points.)
                    bool root_todo = true;
                    auto untested = [&](unsigned long long& m_lo, unsigned long long& m_hi) __attribute__((always_inline)) {
                        const int at = gb + 14 + ci * words;
                        m_lo = pvt_d2u(T.dv(at)) & ~seen_lo;
                        m_hi = words > 1 ? pvt_d2u(T.dv(at + 1)) & ~seen_hi : 0ull;
                    };
                    for (;;) {
                        if (__ballot(walk || root_todo) == 0ull) break;
                        unsigned long long m_lo = 0ull, m_hi = 0ull;
                        if (walk) {
                            untested(m_lo, m_hi);
                            if ((m_lo | m_hi) == 0ull) {
                                next_cell();
                                if (walk) untested(m_lo, m_hi);
                            }
                        }
                        bool test = false;
                        int node = k_root;
                        if (m_lo != 0ull) { node = __builtin_ctzll(m_lo); seen_lo |= m_lo & (0ull - m_lo); test = true; }
                        else if (m_hi != 0ull) { node = 64 + __builtin_ctzll(m_hi); seen_hi |= m_hi & (0ull - m_hi); test = true; }
                        else if (!walk && root_todo) { root_todo = false; test = true; }
#if PVT_STATS
                        st_g[0] += 1; st_g[1] += 1; st_g[2] += __popcll(__ballot(test)); st_g[3] += __popcll(__ballot(!test));
#endif
                        if (test) visit(node);
                    }
                }
                // (grid scenes have visited every node they need by now)
                // ---- SOLO: the two-node stage in closed form ------------------------------------------------------------
                // The scene is one unrotated box (`child`) in a lazy root, and this launch has `lazy_root` (prove_solo, and
                // the host's choice of the entry).  What the loop below does for such a scene, pass by pass -- it visits the
                // child first (k = 0: the only node that is not the root), the root last:
                //   child, nhits == 0 on entry.  The slab test gives tmin <= tmax (a miss, tmax < tmin, folds nothing: such a
                //   lane sends its wave to the loop itself, below).  With e = tmin > kEps and x = tmax > kEps, e implies x.
                //     e && x : fold(tmin) finds nhits == 0: t1 = tmin, n1 = child, tfirst = tmin, nl = 1.  fold(tmax):
                //              `tmax < t1` is false (tmax >= tmin, a tie included), n2 < 0: t2 = tmax, n2 = child, nl = 2.
                //              nl != 1: the child does not hold the ray; cnode stays -1.  nhits = 2.
                //     !e && x: fold(tmax) alone: t1 = tmax, n1 = child, nl = 1, tfirst = tmax < cbest = inf: cnode = child,
                //              cbest = tmax.  nhits = 1.  (tmax == inf would leave cnode at -1 -- and fails `t1 < bound`
                //              below: undecided, the loop itself.)
                //     neither: nothing folded: nhits = 0, cnode = -1.
                //   root, lazy.  undecided = !(bound > 0) || (nhits > 0 && !(t1 < bound)) || (nhits >= 2 && !(t2 < bound)) ||
                //   (cnode >= 0 && !(cbest < bound)) -- `lazy_exact` is false: this launch has its own lazy root -- which is,
                //   in the three cases, !(bound > 0) || (e && !(tmin < bound)) || (x && !(tmax < bound)): t1 is tmin when e,
                //   else tmax when x; t2 is tmax when e; cbest is tmax when !e && x.  Decided, the root adds one crossing
                //   behind all the others and is intersected with nothing (nl = 0: it cannot become the container by `holds`):
                //     e && x : nhits = 3, n1 = n2 = child, cnode = root (it was -1).
                //     !e && x: nhits = 2, n2 = root (t2 = inf), cnode stays child.
                //     neither: nhits = 1, t1 = bound, n1 = root, cnode = root.
                //   the selection after the loop: hit = n1, t0 = t1; nhits == 1: container = hit, adjacent = -1; else
                //   container = cnode (>= 0 in both cases), adjacent = (container == hit) ? n2 : hit:
                //     e && x : hit = child, t0 = tmin, container = root,  adjacent = child
                //     !e && x: hit = child, t0 = tmax, container = child, adjacent = root
                //     neither: hit = root,  t0 = bound, container = root, adjacent = -1      (nhits is never 0: not terminal)
                // Same operations on the same operands in the same order as the loop's (translation, three rcp_normal, the slab
                // arm for rays parallel to no face, the bound): the same bits.  A wave any of whose lanes is undecided, holds a
                // direction component below 1e-300 or misses the slab (tmax < tmin) runs the loop itself for that trip.
                // The three outcomes are handed to the selection after the loop as the values the folds would have left in
                // n1, t1, n2, cnode -- and nhits as 2 or 1, all that selection asks of a count that is not 0 -- and the loop
                // runs no pass: nothing of the closed form is live across the loop or the selection.
                // (The root's number behind an opaque copy: the two records' addresses are worked out in the trip, as the
                // loop works out its node's -- left to the compiler they are launch invariants held in scalar registers for the
                // whole kernel, which the parking entries do not have to spare.)
                int loop_nodes = k_nodes;   // passes of the node loop in this trip (wave-uniform)
                if constexpr (SOLO && (!TAIL || PVT_SOLO_TAIL)) {
                    int kr = k_root;
                    asm volatile("" : "+s"(kr));
                    const int child = 1 - kr;
                    const int hc = child * ND, hr = kr * ND;
                    const double cx = T.du(hc + ND_T), cy = T.du(hc + ND_T + 1), cz = T.du(hc + ND_T + 2);
                    const double cg[3] = {T.du(hc + ND_PARAMS), T.du(hc + ND_PARAMS + 1), T.du(hc + ND_PARAMS + 2)};
                    const double oo[3] = {pos.x + cx, pos.y + cy, pos.z + cz}, dd[3] = {dir.x, dir.y, dir.z};
                    double tmin = -INFINITY, tmax = INFINITY;
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const double ia = rcp_normal(dd[a]);   // (garbage below 1e-300: the wave takes the loop)
                        const double sz = cg[a];
                        const double ta = (-0.5 * sz - oo[a]) * ia, tb = (0.5 * sz - oo[a]) * ia;
                        tmin = __builtin_fmax(tmin, __builtin_fmin(ta, tb));
                        tmax = __builtin_fmin(tmax, __builtin_fmax(ta, tb));
                    }
                    V3 ro;
                    ro.x = pos.x + T.du(hr + ND_T); ro.y = pos.y + T.du(hr + ND_T + 1); ro.z = pos.z + T.du(hr + ND_T + 2);
                    const double rg0 = T.du(hr + ND_PARAMS), rg1 = T.du(hr + ND_PARAMS + 1), rg2 = T.du(hr + ND_PARAMS + 2);
                    double bound;
                    if (uf(UF_LAZY1)) {
                        const double mx = 0.5 * rg0 - pvt_fabs(ro.x), my = 0.5 * rg1 - pvt_fabs(ro.y), mz = 0.5 * rg2 - pvt_fabs(ro.z);
                        bound = __builtin_fmin(__builtin_fmin(mx, my), mz);
                    } else {
                        bound = (rg0 * rg0 - dot3(ro, ro)) * A.lazy_k;
                    }
                    const bool e = tmin > kEps, x = tmax > kEps;
                    const bool undecided = !(bound > 0.0) || (e && !(tmin < bound)) || (x && !(tmax < bound));
                    const bool parallel = pvt_fabs(dd[0]) < 1e-300 || pvt_fabs(dd[1]) < 1e-300 || pvt_fabs(dd[2]) < 1e-300;
                    if (__ballot(undecided || parallel || tmax < tmin) == 0ull) {
                        n1 = x ? child : kr;
                        t1 = e ? tmin : (x ? tmax : bound);
                        n2 = kr;                             // (read only where the child holds the ray: !e && x)
                        cnode = (x && !e) ? child : kr;
                        nhits = x ? 2 : 1;
                        loop_nodes = 0;
                    }
                }
                for (int k = 0; k < (GRID ? 0 : (SOLO ? loop_nodes : k_nodes)); k++) {
                    const int node = !lazy_root ? k : (k == k_nodes - 1 ? k_root : (k < k_root ? k : k + 1));
                    // An unrotated node (identity rotation, bit for bit -- the usual case) only translates:
                    // 1*x + 0*y + 0*z + t equals x + t up to the sign of a zero, which no comparison,
                    // quotient or stored value below can see.
                    // the node's 64-byte record: one scalar load, all of it in SGPRs
                    const int hn = node * ND;
                    const double tx = T.du(hn + ND_T), ty = T.du(hn + ND_T + 1), tz = T.du(hn + ND_T + 2);
                    const double gpar[3] = {T.du(hn + ND_PARAMS), T.du(hn + ND_PARAMS + 1), T.du(hn + ND_PARAMS + 2)};
                    const unsigned long long hbits = pvt_d2u(T.du(hn + ND_BITS));
                    const bool ident = node_ident(hbits);   // wave-uniform
                    const int rc = LEAN ? 0 : (int)(unsigned int)(hbits >> 32);   // rotation class (lean: the identity is the only one)
                    V3 o;
                    if (ident) {
                        o.x = pos.x + tx; o.y = pos.y + ty; o.z = pos.z + tz;
                    } else {
                        const int rm = L.rot_d + rc * RT + RT_W2L;
                        o.x = T.du(rm + 0) * pos.x + T.du(rm + 1) * pos.y + T.du(rm + 2) * pos.z + tx;
                        o.y = T.du(rm + 3) * pos.x + T.du(rm + 4) * pos.y + T.du(rm + 5) * pos.z + ty;
                        o.z = T.du(rm + 6) * pos.x + T.du(rm + 7) * pos.y + T.du(rm + 8) * pos.z + tz;
                    }
                    // Nodes whose world->local rotations are bit-identical (the host files them under the
                    // first such node) see the same local direction: it and its reciprocals are reused.
                    if (rc != rot) {
                        if (ident) {
                            d = dir;
                        } else {
                            const int rm = L.rot_d + rc * RT + RT_W2L;
                            d.x = T.du(rm + 0) * dir.x + T.du(rm + 1) * dir.y + T.du(rm + 2) * dir.z;
                            d.y = T.du(rm + 3) * dir.x + T.du(rm + 4) * dir.y + T.du(rm + 5) * dir.z;
                            d.z = T.du(rm + 6) * dir.x + T.du(rm + 7) * dir.y + T.du(rm + 8) * dir.z;
                        }
                        rot = rc;
                        inv_ok = false;
                    }
                const int gt = node_geom(hbits);
                // Hits are folded as they are found, in the reference's (node, k)
                // order, so no per-ray hit list exists; the tie-breaks equal the
                // reference's argmin scans over its hit arrays (:684-714).
                int nl = 0;
                double tfirst = 0.0;
                bool root_known = false;   // this lane's root crossing is accounted for without its distance
                if (lazy_root && node == k_root) {
                    double bound;   // <= distance to the root's surface along any direction
                    if (lazy_root == 1) {
                        const double mx = 0.5 * gpar[0] - pvt_fabs(o.x), my = 0.5 * gpar[1] - pvt_fabs(o.y),
                                     mz = 0.5 * gpar[2] - pvt_fabs(o.z);
                        bound = __builtin_fmin(__builtin_fmin(mx, my), mz);
                    } else {   // (R^2 - |o|^2) / (2R) <= R - |o|
                        const double radius = gpar[0];
                        bound = (radius * radius - dot3(o, o)) * A.lazy_k;
                    }
                    const bool undecided = !(bound > 0.0) || (nhits > 0 && !(t1 < bound)) || (nhits >= 2 && !(t2 < bound)) ||
                                           (cnode >= 0 && !(cbest < bound)) || (lazy_exact && nhits == 0);
                    if (!undecided) {
                        // one more crossing, behind all the others: nearest only if there is no other
                        if (nhits == 0) { t1 = bound; n1 = node; }
                        else if (nhits == 1) { t2 = INFINITY; n2 = node; }
                        nhits += 1;
                        if (cnode < 0) cnode = node;   // crossed once: it holds the ray unless a nearer node does
                        root_known = true;
                    }
                }
                auto fold = [&](double t) __attribute__((always_inline)) {
                    if (nl == 0) tfirst = t;
                    nl += 1;
                    if (nhits == 0) { t1 = t; n1 = node; }
                    else if (t < t1) { t2 = t1; n2 = n1; t1 = t; n1 = node; }
                    else if (n2 < 0 || t < t2) { t2 = t; n2 = node; }
                    nhits += 1;
                };
                if (root_known) {
                    // nothing to intersect
                } else if (MESH && gt == PVT_GEOM_MESH) {
                    // EXTENSION (no reference counterpart, see include/pvtrace_hip.h): every
                    // forward crossing of the node's triangles, found by a stack-free walk of
                    // the BVH (pvt_bvh.h).  Crossings of one mesh are ordered by
                    // (t, face) so the result does not depend on the walk order.
                    const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
                    const double ax = pvt_fabs(d.x), ay = pvt_fabs(d.y), az = pvt_fabs(d.z);
                    const int kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
                    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
                    auto pick = [](const double* v, int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); };
                    const double dz = pick(dd, kz);
                    if (dz < 0.0) { int tmp = kx; kx = ky; ky = tmp; }
                    // (the shear constants feed the exact triangle test: the short division sequences give RN(x / dz) and RN(1 / dz)
                    // bit for bit when dz -- the dominant direction component -- is an ordinary number and the numerators are zero
                    // or not tiny, which a wave checks once; anything else takes the general divisions)
                    double shx, shy, shz;
                    {
                        const double sx_ = pick(dd, kx), sy_ = pick(dd, ky);
                        auto ordinary = [](double x) { return x == 0.0 || (pvt_fabs(x) > 1e-280 && pvt_fabs(x) < 1e280); };
                        if (__ballot(!(pvt_fabs(dz) > 1e-100 && pvt_fabs(dz) < 1e100) || !ordinary(sx_) || !ordinary(sy_)) == 0ull) {
                            shx = div_normal(sx_, dz); shy = div_normal(sy_, dz); shz = rcp_normal(dz);
                        } else {
                            shx = sx_ / dz; shy = sy_ / dz; shz = 1.0 / dz;
                        }
                    }
                    // Box culling only has to be conservative (a false hit costs a triangle test, a
                    // false miss would lose a crossing).  A ray parallel to a slab gets a huge finite
                    // reciprocal instead of inf: inside the slab the two plane distances then have
                    // opposite signs (interval covers everything), outside the same sign (pushed out
                    // of range, or a harmless false hit), and 0 * inf = NaN can never arise.
                    double minv[3];
#pragma unroll
                    for (int a = 0; a < 3; a++) minv[a] = pvt_fabs(dd[a]) < 1e-300 ? 1e300 : rcp_normal(dd[a]);   // (culling only)
                    long long f1 = -1, f2 = -1;   // faces of this node's entries in (t1, t2)
                    int i = T.iu(node * NI + NI_MESH);
                    // (the two table pointers in registers for the walk: the build keeps loop invariants where they are used --
                    // good for the photon loop as a whole, but here that is a scalar load of the kernel argument, and a wait
                    // for it, in every iteration of the walk)
                    const pvt::BvhNode* bvh = A.bvh;
                    const pvt::MeshTri* tris = A.tris;
                    asm volatile("" : "+s"(bvh), "+s"(tris));
                    // The walk waits for its records more than it computes (a wave of the 20 480-face ball: 62 % of its cycles,
                    // ~1 000 per box): the top levels of every tree -- where every ray passes -- are read from a copy in LDS
                    // (pvt_bvh.h: stage_top).  A cursor is the index of a record in global memory, or kTopFlag | slot in
                    // that copy; skip links are stored in the same form, the walk is over when the cursor equals the
                    // tree's end.
                    const pvt::BvhNode* const ltop = reinterpret_cast<const pvt::BvhNode*>(reinterpret_cast<const char*>(smem) + A.top_off);
                    // (records in global memory through a buffer descriptor: the address of a record is its byte offset, one
                    // shift, instead of a 64-bit multiply-add, and the loads do not count as LDS traffic to wait for)
                    const __amdgpu_buffer_rsrc_t brec = __builtin_amdgcn_make_buffer_rsrc(const_cast<pvt::BvhNode*>(bvh), 0, -1, 0x00020000);
                    auto record_at = [&](int index) __attribute__((always_inline)) {
                        typedef unsigned int Word4 __attribute__((ext_vector_type(4)));
                        struct Pair { Word4 a, b; } w;
                        w.a = __builtin_amdgcn_raw_buffer_load_b128(brec, index << 5, 0, 0);
                        w.b = __builtin_amdgcn_raw_buffer_load_b128(brec, (index << 5) + 16, 0, 0);
                        return __builtin_bit_cast(pvt::BvhNode, w);
                    };
                    // (the root's record -- its box, the tree's end, where its copy is -- through the scalar cache: the node is the wave's)
                    const __attribute__((address_space(4))) pvt::BvhNode* const rootp =
                        (const __attribute__((address_space(4))) pvt::BvhNode*)(A.bvh + i);
                    const float rlo[3] = {rootp->lo[0], rootp->lo[1], rootp->lo[2]}, rhi[3] = {rootp->hi[0], rootp->hi[1], rootp->hi[2]};
                    const int end = rootp->skip, rlink = rootp->link;
                    const int n_records = end - i;   // (before the cursor moves to the copy)
                    pvt::BvhNode b;
                    // The boxes are tested in f32, relative to the mesh's centre (the node's parameter slots) and from where
                    // the ray ENTERS the root box -- every quantity then has the mesh's own size, the test's rounding displaces
                    // a plane by < 5e-7 of the mesh's diagonal, and the host pads every box by 4e-6 of it (pvt_bvh.h).
                    float oi[3], invf[3];   // (a plane's distance is fma(plane, 1/d, -(o/d)): o/d once per walk)
                    {
                        double t_near = 0.0, t_far = INFINITY;
                        const double cc[3] = {gpar[0], gpar[1], gpar[2]};
#pragma unroll
                        for (int a = 0; a < 3; a++) {
                            const double ta = (((double)rlo[a] + cc[a]) - oo[a]) * minv[a], tb = (((double)rhi[a] + cc[a]) - oo[a]) * minv[a];
                            t_near = __builtin_fmax(t_near, __builtin_fmin(ta, tb));
                            t_far = __builtin_fmin(t_far, __builtin_fmax(ta, tb));
                        }
                        if (rlink >= 0 && (rlink & pvt::kTopFlag) != 0) {   // the tree has a copy in LDS: the root's slot precedes its children's
                            i = rlink - 1;
                            b = ltop[i & pvt::kIndexMask];
                        } else {
                            b = record_at(i);
                        }
                        if (t_far < t_near) i = end;   // the ray misses the mesh's box altogether
#pragma unroll
                        for (int a = 0; a < 3; a++) {
                            invf[a] = pvt_fabs(dd[a]) < 1e-20 ? 1e20f : (float)minv[a];   // (a component this small: the ray is parallel to the pair of planes)
                            oi[a] = (float)((oo[a] - cc[a]) + dd[a] * t_near) * invf[a];
                        }
                    }
                    // The triangle tests are DEFERRED: a lane that reaches a leaf only notes it (four slots in registers) and
                    // walks on until its slots are full; when every lane of the wave has stopped -- slots full or walk
                    // over -- the notes are worked off together, every lane on one of its leaves at once, and the walks
                    // resume.  Tested inside the walk, the watertight
                    // test (185 vector instructions against the 50 of a box) ran in four iterations out of five for
                    // the one or two lanes that happened to stand at a leaf.  (Crossings are ordered by (t, face): the
                    // order they are found in does not matter.)
                    // (A mesh of a few triangles -- a tree of a handful of nodes, leaves of up to eight triangles -- has no
                    // walk to speak of to keep going: its leaves are tested as they are met.  Wave-uniform: the node is.)
                    // (the notes live in LDS, one column per lane: in registers they were a shift register whose copies the
                    // compiler carried through every path of the walk -- 14 moves per box)
                    unsigned int* const mq = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(smem) + A.meshq_off) + threadIdx.x;
                    int qn = 0;
                    const int qcap = n_records <= 16 ? 1 : kMeshQ;
                    for (;;) {
                        // ---- walk: every lane goes on until its walk is over or its slots are full
                        for (;;) {
                            const bool go = i != end && qn < qcap;
                            if (__ballot(go) == 0ull || __popcll(__ballot(i != end && qn >= qcap)) >= 4) break;   // (lanes with full leaf slots that end a walk phase: 1 / 4 / 16 measured within 3 %)
#if PVT_STATS
                            if (MESH) { st_g[0] += 1; st_g[1] += __popcll(__ballot(go)); }
#endif
                            if (go) {
                                float tmin = 0.0f, tmax = INFINITY;
#pragma unroll
                                for (int a = 0; a < 3; a++) {
                                    const float ta = __builtin_fmaf(b.lo[a], invf[a], -oi[a]), tb = __builtin_fmaf(b.hi[a], invf[a], -oi[a]);
                                    tmin = __builtin_fmaxf(tmin, __builtin_fminf(ta, tb));
                                    tmax = __builtin_fminf(tmax, __builtin_fmaxf(ta, tb));
                                }
                                // the successor: after a miss and after a leaf the skip link, after a hit of an inner record its first
                                // child (whose own skip link is its sibling, in the same 64-byte line)
                                int next = b.skip;
                                if (!(tmax < tmin)) {
                                    if (b.link < 0) {   // a leaf: its triangle later (the newest note first: any order will do)
                                        mq[qn * kBlock] = (unsigned int)b.link;
                                        qn += 1;
                                    } else {
                                        next = b.link;
                                    }
                                }
                                i = next;
                                if (i != end) {
                                    if (i & pvt::kTopFlag) b = ltop[i & pvt::kIndexMask];
                                    else b = record_at(i);
                                }
                            }
                        }
                        // ---- the noted leaves, every lane on one of its own at a time
                        while (__ballot(qn > 0) != 0ull) {
                            if (qn > 0) {
                                qn -= 1;
                                const int leaf = (int)mq[qn * kBlock];
                                constexpr int tn = 1;   // (one triangle per leaf: pvt_bvh.h)
                                const int tri_start = leaf & pvt::kIndexMask;
                                const pvt::MeshTri* tr = tris + tri_start;
                                for (int k = 0; k < tn; k++, tr++) {
#if PVT_STATS
                                    if (MESH) { st_g[2] += 1; st_g[3] += __popcll(__ballot(true)); }
#endif
                                    double va[3], vb[3], vc[3];
#pragma unroll
                                    for (int a = 0; a < 3; a++) {
                                        va[a] = tr->v[a] - oo[a]; vb[a] = tr->v[3 + a] - oo[a]; vc[a] = tr->v[6 + a] - oo[a];
                                    }
                                    const double az_ = pick(va, kz), bz_ = pick(vb, kz), cz_ = pick(vc, kz);
                                    const double axs = pick(va, kx) - shx * az_, ays = pick(va, ky) - shy * az_;
                                    const double bxs = pick(vb, kx) - shx * bz_, bys = pick(vb, ky) - shy * bz_;
                                    const double cxs = pick(vc, kx) - shx * cz_, cys = pick(vc, ky) - shy * cz_;
                                    const double u = cxs * bys - cys * bxs;
                                    const double v = axs * cys - ays * cxs;
                                    const double w = bxs * ays - bys * axs;
                                    // (one flag instead of a chain of exits: every lane of the trip is on a triangle of its own, and each
                                    // early exit was a pair of exec-mask instructions and a branch for all of them)
                                    const double det = u + v + w;
                                    bool ok = !((u < 0.0 || v < 0.0 || w < 0.0) && (u > 0.0 || v > 0.0 || w > 0.0)) && det != 0.0;
                                    // exact zeros of an edge function (a ray through an edge or a vertex): the ownership rule, only when a
                                    // lane of the wave has one
                                    if (__ballot(ok && (u == 0.0 || v == 0.0 || w == 0.0)) != 0ull) {
                                        const double sg = det < 0.0 ? -1.0 : 1.0;
                                        auto owned = [](double gx, double gy) { return gx > 0.0 || (gx == 0.0 && gy > 0.0); };
                                        if (u == 0.0 && !owned(sg * (cys - bys), sg * (bxs - cxs))) ok = false;
                                        if (v == 0.0 && !owned(sg * (ays - cys), sg * (cxs - axs))) ok = false;
                                        if (w == 0.0 && !owned(sg * (bys - ays), sg * (axs - bxs))) ok = false;
                                    }
                                    if (!ok) continue;
                                    const double t = (u * (shz * az_) + v * (shz * bz_) + w * (shz * cz_)) / det;
                                    if (!(t > kEps)) continue;
                                    const long long face = tr->face;
                                    const int tri = tri_start + k;
                                    if (nl == 0 || t < tfirst) tfirst = t;
                                    nl += 1;
                                    if (nhits == 0) { t1 = t; n1 = node; tri1 = tri; f1 = face; }
                                    else if (t < t1 || (t == t1 && f1 >= 0 && face < f1)) {
                                        t2 = t1; n2 = n1; f2 = f1; t1 = t; n1 = node; tri1 = tri; f1 = face;
                                    } else if (n2 < 0 || t < t2 || (t == t2 && f2 >= 0 && face < f2)) { t2 = t; n2 = node; f2 = face; }
                                    nhits += 1;
                                }
                            }
                        }
                        if (__ballot(i != end) == 0ull) break;
                    }
                } else if (gt == PVT_GEOM_BOX) {  // slab test (_kernel.pyx:245-276)
                double tmin = -INFINITY, tmax = INFINITY;
                bool miss = false;
                const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
                if (!inv_ok) {   // 1/d per axis, shared by consecutive nodes whose rotations have the same bits
#pragma unroll
                    for (int a = 0; a < 3; a++) inv[a] = rcp_normal(dd[a]);   // 1/d (garbage below 1e-300: never used)
                    inv_ok = true;
                }
                // a ray parallel to a pair of faces (a direction component below 1e-300) takes the reference's
                // inside/outside test for that axis; the wave only runs the general form when a lane holds one
                if (__ballot(pvt_fabs(dd[0]) < 1e-300 || pvt_fabs(dd[1]) < 1e-300 || pvt_fabs(dd[2]) < 1e-300) == 0ull) {
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const double sz = gpar[a];
                        const double ta = (-0.5 * sz - oo[a]) * inv[a], tb = (0.5 * sz - oo[a]) * inv[a];
                        tmin = __builtin_fmax(tmin, __builtin_fmin(ta, tb));
                        tmax = __builtin_fmin(tmax, __builtin_fmax(ta, tb));
                    }
                } else
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    double sz = gpar[a];
                    double lo = -0.5 * sz, hi = 0.5 * sz;
                    if (pvt_fabs(dd[a]) < 1e-300) {
                        if (oo[a] < lo || oo[a] > hi) miss = true;
                    } else {
                        // (the reference swaps ta, tb into order and keeps the largest entry / smallest exit
                        // distance: min and max of finite numbers, which is what these are)
                        const double ta = (lo - oo[a]) * inv[a], tb = (hi - oo[a]) * inv[a];
                        tmin = __builtin_fmax(tmin, __builtin_fmin(ta, tb));
                        tmax = __builtin_fmin(tmax, __builtin_fmax(ta, tb));
                    }
                }
                if (!miss && !(tmax < tmin)) {
                    if (tmin > kEps) fold(tmin);
                    if (tmax > kEps) fold(tmax);
                }
            } else if (gt == PVT_GEOM_SPHERE) {  // (:279-298)
                    double radius = gpar[0];
                    double a = dot3(d, d), b = 2.0 * dot3(d, o), c = dot3(o, o) - radius * radius;
                    double disc = b * b - 4.0 * a * c;
                    if (!(disc < 0.0)) {
                        double sq = pvt_sqrt(disc);
                        double t = (-b - sq) / (2.0 * a);
                        if (t > kEps) fold(t);
                        t = (-b + sq) / (2.0 * a);
                        if (t > kEps) fold(t);
                    }
                } else if (ROUGH && (gt == PVT_GEOM_FRUSTUM || gt == PVT_GEOM_CONICOID)) {   // EXTENSION: truncated cone, conicoid (quadric_hits_call; no node grid holds one)
                    // (a conicoid's record names where its four parameters lie in the double blob -- pack_conicoids; the node is
                    // the wave's, so they come through the scalar cache; a truncated cone has three and a NaN for the fourth)
                    double q0 = gpar[0], q1 = gpar[1], q2 = gpar[2], q3 = __builtin_nan("");
                    if (gt == PVT_GEOM_CONICOID) {
                        const CDoubles cq = T.gd + (int)pvt_d2u(gpar[1]);
                        q0 = cq[0]; q1 = cq[1]; q2 = cq[2]; q3 = cq[3];
                    }
                    const FrustumHits fh = quadric_hits_call(q0, q1, q2, q3, o.x, o.y, o.z, d.x, d.y, d.z);
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (fh.t[j] > kEps) fold(fh.t[j]);
                } else if (ROUGH && gt == PVT_GEOM_POLYHEDRON) {   // EXTENSION: convex polyhedron (polyhedron_hits_call; no node grid holds one)
                    // (the node's record names its rows: where they start in the double blob, how many, as integers in the words' bits -- pack_polyhedra)
                    const PolyhedronHits ph = polyhedron_hits_call(T.gd + (int)pvt_d2u(gpar[1]), (int)pvt_d2u(gpar[2]), o.x, o.y, o.z, d.x, d.y, d.z);
                    if (ph.t[0] > kEps) fold(ph.t[0]);
                    if (ph.t[1] > kEps) fold(ph.t[1]);
                } else {  // capped z cylinder (:301-345)
                    double half = 0.5 * gpar[0], radius = gpar[1];
                    double a = d.x * d.x + d.y * d.y;
                    if (a > 1e-300) {
                        double b = 2.0 * (o.x * d.x + o.y * d.y);
                        double c = o.x * o.x + o.y * o.y - radius * radius;
                        double disc = b * b - 4.0 * a * c;
                        if (disc >= 0.0) {
                            double sq = pvt_sqrt(disc);
                            double t = (-b - sq) / (2.0 * a);
                            double z = o.z + t * d.z;
                            if (z > -half && z < half && t > kEps) fold(t);
                            t = (-b + sq) / (2.0 * a);
                            z = o.z + t * d.z;
                            if (z > -half && z < half && t > kEps) fold(t);
                        }
                    }
                    if (pvt_fabs(d.z) > 1e-300) {
                        double t = (-half - o.z) / d.z;
                        double x = o.x + t * d.x, y = o.y + t * d.y;
                        if (x * x + y * y <= radius * radius && t > kEps) fold(t);
                        t = (half - o.z) / d.z;
                        x = o.x + t * d.x;
                        y = o.y + t * d.y;
                        if (x * x + y * y <= radius * radius && t > kEps) fold(t);
                    }
                }
                    // The container is the nearest node the ray starts inside of: crossed exactly once for the
                    // reference's convex shapes (:696-706); a triangle mesh may be non-convex, so it holds the
                    // ray when it is crossed an ODD number of times (extension; Mesh.contains semantics,
                    // pvtrace/geometry/mesh.py:29-32)
                    const bool holds = (MESH && gt == PVT_GEOM_MESH) ? (nl & 1) != 0 : nl == 1;
                    if (holds && !root_known) {
                        if (tfirst < cbest) {
                            if constexpr (MESH) { c2best = cbest; c2node = cnode; }
                            cbest = tfirst; cnode = node;
                        } else if (MESH && tfirst < c2best) { c2best = tfirst; c2node = node; }
                    }
                }

                PVT_MARK(1);  // node loop
                if (nhits == 0) {
                    terminal = true;  // nothing ahead: the ray vanishes silently (:681-682)
                } else {
                    hit = n1;
                    t0 = t1;
                    if (nhits == 1) { container = hit; adjacent = -1; }
                    else {
                        container = (cnode >= 0) ? cnode : hit;
                        adjacent = (container == hit) ? n2 : hit;
                        if constexpr (MESH) {
                            // leaving a mesh: the second-nearest crossing may be the same (non-convex) mesh
                            // again; what lies beyond the surface is the next node that holds the ray
                            if (container == hit && c2node >= 0 && node_geom(node_bits(hit)) == PVT_GEOM_MESH) adjacent = c2node;
                        }
                    }
                    ev_container = container;
                    if (count > k_maxsteps) {  // (:716-723)
                        ev_kind = PVT_EV_KILL;
                        terminal = true;
                        t_sel = PVT_REC_KILLED; t_node = container;
                    } else {
                        pend = true;
                    }
                }
            }
        }
        // ---- container properties + volume absorption coefficient (:746-760) -----------------------
        // (node and component records are per-lane LDS reads)
        // alpha = sum of the components' coefficients; the running partial sums ARE the cumulative
        // thresholds the reference recomputes when it picks the absorbing component (:768-781): the first
        // one is kept (it decides for containers of two components; more are re-walked when a lane needs it)
        double alpha = 0.0, pre0 = 0.0, n_container = 1.0;
        int cbase = 0, ccount = 0, crec = 0;   // first component id, count, first component record (identical components share records)
        if (pend) {
            n_container = T.dv(container * ND + ND_N);
            if (uf(UF_DISP)) n_container = index_at(container, n_container);
            cbase = T.iv(container * NI + NI_CSTART); ccount = T.iv(container * NI + NI_CCOUNT);
            if (uf(UF_BY_NODE)) crec = cbase;   // (scenes of few nodes keep one record per component id)
            else crec = T.iv(container * NI + NI_CREC);
            // (tail function: a wave alone on its SIMD waits out every LDS round trip in full, and the records the rest of the
            // step needs -- the hit node's, the far side's refractive index, the pair's Fresnel constants -- are all
            // addressed by what the node loop has just found: read together HERE they cost one wait instead of five spread
            // over the step; the same words, so the same bits)
            if constexpr (TAIL) {
                const int hn = hit * ND;
                hr_t = V3{T.dv(hn + ND_T), T.dv(hn + ND_T + 1), T.dv(hn + ND_T + 2)};
                hr_g = V3{T.dv(hn + ND_PARAMS), T.dv(hn + ND_PARAMS + 1), T.dv(hn + ND_PARAMS + 2)};
                hr_bits = pvt_d2u(T.dv(hn + ND_BITS));
                hr_surf = T.iv(hit * NI + NI_SURF);
                if (adjacent >= 0) {
                    int kc = container, ka = adjacent;
                    if (!uf(UF_BY_NODE)) { kc = T.iv(container * NI + NI_NCLS); ka = T.iv(adjacent * NI + NI_NCLS); }
                    hr_n2 = T.dv(adjacent * ND + ND_N);
                    hr_rn2 = T.dv(L.ncls_d + ka * 2 + 1);
                    hr_cc = uf(UF_CRIT) ? T.dv(L.ccrit_d + kc * L.n_cls + ka) : __builtin_nan("");
                    if (uf(UF_DISP)) { hr_n2 = index_at(adjacent, hr_n2); hr_rn2 = div_normal(1.0, hr_n2); }
                }
            }
            // (tail function: a photon that bounces inside one body keeps its wavelength, and with it the coefficients of
            // the step before -- the same table values, read once instead of once per bounce; not in the kernels' own loop,
            // where the seven registers cost more than the lookups: docs/history.md, round 4)
            bool known = false;
            if constexpr (TAIL) {
                ac_node = (int)(unsigned int)ac_lds[0]; ac_wl = ac_lds[64];
                ac_alpha = pvt_u2d(ac_lds[128]); ac_pre0 = pvt_u2d(ac_lds[192]);
            }
            if constexpr (TAIL) known = container == ac_node && pvt_d2u(wl) == ac_wl;
            if (hit != k_root && !known) {
                for (int k = 0; k < ccount; k++) {
                    const int ci = L.comp_i + (crec + k) * CI, cd = L.comp_d + (crec + k) * CD;
                    alpha += interp_clamped<TAB_LDS, kAbsKind>(T, wl, T.iv(ci + CI_ABS_X), T.iv(ci + CI_ABS_Y), T.iv(ci + CI_ABS_N),
                                                            T.iv(ci + CI_ABS_G), T.dv(cd + CD_ABS_SCALE), T.iv(ci + CI_ABS_HIST),
                                                            T.dv(cd + CD_ABS_RCP), T.dv(cd + CD_ABS_W));
                    if (k == 0) pre0 = alpha;
                }
                if constexpr (TAIL) {
                    ac_lds[0] = (unsigned long long)(unsigned int)container; ac_lds[64] = pvt_d2u(wl);
                    ac_lds[128] = pvt_d2u(alpha); ac_lds[192] = pvt_d2u(pre0);
                }
            }
            if constexpr (TAIL) {
                if (known && hit != k_root) { alpha = ac_alpha; pre0 = ac_pre0; }
            }
        }
        int comp = -1;
        int frec = -1, fcell = 0;   // (scenes with a lattice) the container's field record, the cell absorbed in
        if (pend) {
            // free path in the container (no draw when the photon leaves the scene or the medium is clear), then
            // ONE advance for all three outcomes: to the absorption point if that comes first, else to the surface
            double depth = INFINITY;
            if constexpr (!ROUGH) {
                if (hit != k_root && alpha > kAlphaZero) depth = div_normal(-log_draw(1.0 - rng_uniform(rng)), alpha);
            } else {
                // (the variants of scenes with a rough node or a lattice) the same draw on the unscaled sum; a container
                // with a lattice marches its cells to tau* (PvtFieldTables), and the pick below divides that cell's
                // coefficients.  (The tail's alpha cache holds the unscaled sums, which stay right for the draw.)
                if (hit != k_root && alpha > kAlphaZero) {
                    const double tau = -log_draw(1.0 - rng_uniform(rng));
                    if (uf(UF_FIELD)) frec = (int)A.fd[container];
                    if (frec >= 0) {
                        const FieldMarch fm = field_march_call<TAB_LDS, ROUGH >= kExtAligned>(T, A.fd, frec, L.comp_i + crec * CI, L.comp_d + crec * CD, ccount,
                                                                        wl, pos.x, pos.y, pos.z, dir.x, dir.y, dir.z, tau, t0);
                        depth = fm.depth;
                        if (fm.depth < t0) { alpha = fm.alpha; pre0 = fm.pre0; fcell = fm.cell; }
                    } else {
                        depth = div_normal(tau, alpha);
                    }
                }
            }
            {
                const double adv = __builtin_fmin(depth, t0);   // (depth == t0 is a surface event: same value)
                if constexpr (ROUGH == kExtPath) {
                    // ---- path-length maps (PvtMapTables, PVT_MAP_PATHLENGTH): the segment pos -> pos + adv dir, BEFORE the
                    // advance, is laid cell by cell into the path-length maps of `container` -- only for the lanes whose
                    // container's block says it has one (kMnPath), in the maps' block of the lane's tally set
                    if (uf(UF_PMAP)) {
                        const int mat = (int)A.md[container];
                        if (mat >= 0 && A.md[mat + kMnPath] != 0.0)
                            path_map_call(A.md + mat, reinterpret_cast<unsigned long long*>(A.rec_bins) + (long long)set * A.set_stride_i + A.total_bins,
                                          pos.x, pos.y, pos.z, dir.x, dir.y, dir.z, adv, wl);
                    }
                }
                pos.x = pos.x + dir.x * adv; pos.y = pos.y + dir.y * adv; pos.z = pos.z + dir.z * adv;
                travelled += adv;
                duration += div_known(adv * n_container, kCcm, kRcpCcm);
            }
            if constexpr (kClassRegions) {
                // (lean) the three outcomes as selects of VALUES (see fold_by_key): each nested body is a handful of
                // moves, and a divergent `if` around it costs three scalar instructions and a branch that a wave of 64
                // mixed photons never takes.  The absorbed lanes' draws wait for the one region of their class below.
                const bool leaves = hit == k_root;                            // leaves the scene (:728-744)
                const bool absorbed = !leaves && depth < t0;                  // absorbed (:762-832)
                const bool surface = !leaves && !absorbed && adjacent >= 0;   // surface interaction (:834-895)
                const bool malformed = !leaves && !absorbed && adjacent < 0;  // malformed scene (:840-845)
                cls = leaves ? (int)CLS_EXIT : absorbed ? (int)CLS_ABS : surface ? (int)CLS_SURF : (int)CLS_NONE;
                ev_kind = leaves ? (int)PVT_EV_EXIT : malformed ? (int)PVT_EV_KILL : ev_kind;
                ev_hit = absorbed ? ev_hit : hit;
                ev_adjacent = (leaves || surface) ? adjacent : ev_adjacent;
                terminal = terminal || leaves || malformed;
                t_sel = leaves ? (int)PVT_REC_EXIT : t_sel;
                t_node = (leaves || surface) ? hit : t_node;
                t_normal = t_normal || leaves || surface;
                ev_normal = ev_normal || surface;
            } else if (hit == k_root) {  // leaves the scene (:728-744)
                ev_kind = PVT_EV_EXIT; ev_hit = hit; ev_adjacent = adjacent;
                terminal = true;
                t_sel = PVT_REC_EXIT; t_node = hit; t_normal = true;
                cls = CLS_EXIT;
            } else {
                if (depth < t0) {  // absorbed (:762-832)
                    const double target = rng_uniform(rng) * alpha;
                    comp = cbase;
                    if (ccount <= 2) {
                        // (the reference walks the cumulative coefficients; with two components the first
                        // partial sum decides, and the last component takes what is left, :768-781)
                        comp = (ccount == 2 && !(target <= pre0)) ? cbase + 1 : cbase;
                    } else {
                        double running = 0.0;
                        for (int k = 0; k < ccount; k++) {
                            const int ci = L.comp_i + (crec + k) * CI, cd = L.comp_d + (crec + k) * CD;
                            double term = interp_clamped<TAB_LDS>(T, wl, T.iv(ci + CI_ABS_X), T.iv(ci + CI_ABS_Y), T.iv(ci + CI_ABS_N),
                                                                  T.iv(ci + CI_ABS_G), T.dv(cd + CD_ABS_SCALE), T.iv(ci + CI_ABS_HIST),
                                                                  T.dv(cd + CD_ABS_RCP), T.dv(cd + CD_ABS_W));
                            if constexpr (ROUGH) {   // (a lattice: the cell's concentration of the component)
                                if (frec >= 0) {   // (... or, PvtAlignTables, the component's factor along the photon's direction)
                                    if constexpr (ROUGH >= kExtAligned) term = align_term(A.fd, frec, k, fcell, term, dir.x, dir.y, dir.z);
                                    else term = term * A.fd[(int)A.fd[frec + kFrComp + k] + fcell];
                                }
                            }
                            running += term;
                            if (target <= running) { comp = cbase + k; break; }
                        }
                    }
                    log_row<RECORD, TAIL>(A, rec_slot, nev, PVT_EV_ABSORB, -1, container, -1, comp, source, pos,
                                    dir, false, pos, wl, travelled, duration);
                    ev_component = comp;
                    cls = CLS_ABS;
                } else {
                    // ---- surface interaction (:834-895) ---------
                    ev_hit = hit;
                    if (adjacent < 0) {  // malformed scene (:840-845)
                        ev_kind = PVT_EV_KILL;
                        terminal = true;
                    } else {
                        ev_adjacent = adjacent;
                        t_node = hit; t_normal = true; ev_normal = true;
                        cls = CLS_SURF;
                    }
                }
            }
        }
        // ---- the absorbing component decides (:783-832): one pass per distinct component of the wave,
        // its record in SGPRs
        const double wl_abs = wl;   // (volume maps: the wavelength the ABSORB row holds; unused in the smooth variants)
        if constexpr (kClassRegions) {
            // (lean) ONE divergent region for the absorbed lanes: the component pick, the quantum-yield draw, the emission
            // draws in the reference's order and the lifetime draw -- every draw under the condition it has in the
            // generic body below, so the lane's stream is the same; the two ends of the component's decision differ
            // in five values, which are selects; the emission method is wave-uniform and stays a scalar branch.
            // (absorbers and luminophores only, isotropic, no table, at most two components: prove_lean)
            if (cls == CLS_ABS) {
                const double target = rng_uniform(rng) * alpha;
                // (the reference walks the cumulative coefficients; with two components the first partial sum
                // decides, and the last component takes what is left, :768-781)
                comp = (ccount == 2 && !(target <= pre0)) ? cbase + 1 : cbase;
                log_row<RECORD, TAIL>(A, rec_slot, nev, PVT_EV_ABSORB, -1, container, -1, comp, source, pos,
                                dir, false, pos, wl, travelled, duration);
                ev_component = comp;
                const int cr = crec + (comp - cbase);
                const int ci = L.comp_i + cr * CI, cd = L.comp_d + cr * CD;
                bool radiative = false;
                if (T.iv(ci + CI_TYPE) == PVT_COMP_LUMINOPHORE) radiative = rng_uniform(rng) < T.dv(cd + CD_QY);
                const double tau = T.dv(cd + (radiative ? (int)CD_TAU_RAD : (int)CD_TAU_NR));
                ev_kind = radiative ? (int)PVT_EV_EMIT : (int)PVT_EV_NONRADIATIVE;
                t_sel = radiative ? t_sel : (int)PVT_REC_LOST;
                t_node = radiative ? t_node : container;
                terminal = terminal || !radiative;
                if (radiative) {
                    // isotropic (_kernel.pyx:455-476): azimuth 2 pi g1, cosine of the polar angle 2 g2 - 1
                    const double g1 = rng_uniform(rng), g2 = rng_uniform(rng);
                    const double em_c = 2.0 * g2 - 1.0;
                    const double em_s = sqrt1m2_normal(em_c);
                    double sp, cp;
                    pvt_sincos2pi(g1, &sp, &cp);
                    dir = V3{em_s * cp, em_s * sp, em_c};
                    em = true;
                    source = comp;
                    const int ex = T.iv(ci + CI_EMS_X), ec = T.iv(ci + CI_EMS_CDF), en = T.iv(ci + CI_EMS_N);
                    const int eh = T.iv(ci + CI_EMS_HIST);
                    const double ew = T.dv(cd + CD_EMS_W);
                    double p1;
                    if (uf(UF_EMIT_FULL)) {
                        p1 = 0.0;
                    } else {
                        double e_nm = wl;
                        if (uf(UF_EMIT_KT)) {
                            const double kb_ev = 1.380649e-23 / 1.60217662e-19;
                            double e_ev = div_normal(1240.0, e_nm) + 1.5 * kb_ev * 300.0;
                            e_nm = div_normal(1240.0, e_ev);
                        }
                        p1 = interp_clamped<TAB_LDS, kAbsKind>(T, e_nm, ex, ec, en, T.iv(ci + CI_EMS_GX), T.dv(cd + CD_EMS_SCALE_X),
                                                                          eh, T.dv(cd + CD_EMS_RCP_X), ew);
                    }
                    const double gamma = p1 + (1.0 - p1) * rng_uniform(rng);
                    wl = interp_clamped<TAB_LDS, kCdfKind>(T, gamma, ec, ex, en, T.iv(ci + CI_EMS_GC), T.dv(cd + CD_EMS_SCALE_C), eh,
                                                                T.dv(cd + CD_EMS_RCP_C), __builtin_nan(""), eh ? __builtin_nan("") : ew);
                }
                // radiative / non-radiative lifetime: the last draw of either end
                if (tau > 0.0) duration += -log_draw(1.0 - rng_uniform(rng)) * tau;
            }
        } else {
            const int cu = comp;                       // the component's id (what the event and `source` name) ...
            const bool mine = cls == CLS_ABS;
            const int cr = mine ? crec + (comp - cbase) : 0;   // ... and its record
            const int ci = L.comp_i + cr * CI, cd = L.comp_d + cr * CD;
            const int ctype = T.iv(ci + CI_TYPE);
            if (mine) {
                bool radiative = false;
                if (ctype == PVT_COMP_SCATTERER || ctype == PVT_COMP_LUMINOPHORE)
                    radiative = rng_uniform(rng) < T.dv(cd + CD_QY);
                double tau = 0.0;
                if (radiative) {
                    // phase function (_kernel.pyx:455-476): the draws, in the reference's order, give the
                    // cosine (or sine) of the polar angle; its partner is the composition pvt_sqrt1m2; the
                    // azimuth is 2 pi `em_turn` (pvt_sincos2pi); the new direction is written here, before the
                    // event is logged at the end of the step
                    double em_s, em_c, em_turn;
                    const int pt = T.iv(ci + CI_PHASE);
                    const double pp = T.dv(cd + CD_PHASE);
                    // a tabulated phase function: CD_PHASE is where its record starts, with the spectra.  (A
                    // wave-uniform "the scene has tables" flag in front of the lane test put a vector register of the
                    // 256-recorder tally variants in scratch; without it the headline variant keeps its registers.)
                    const bool tabled = pt == PVT_PHASE_TABLE;
                    const double* ptab = (TAB_LDS == 1 ? T.ld : T.hd) + (tabled ? (int)pp : 0);
                    double u1 = 0.0, u3 = 0.0;
                    if (pt == PVT_PHASE_HG && pvt_fabs(pp) >= kEps) {
                        double g1 = rng_uniform(rng);
                        double sg = 2.0 * g1 - 1.0;
                        double q = (1.0 - pp * pp) / (1.0 + pp * sg);
                        em_c = 1.0 / (2.0 * pp) * (1.0 + pp * pp - q * q);
                        em_c = __builtin_fmin(__builtin_fmax(em_c, -1.0), 1.0);   // (sample_phase: NaN in the reference)
                        em_turn = rng_uniform(rng);
                        em_s = sqrt1m2_normal(em_c);
                    } else if (pt == PVT_PHASE_CONE) {
                        double g1 = rng_uniform(rng), g2 = rng_uniform(rng);
                        em_s = pvt_sqrt(g1) * pvt_sin(pp);
                        em_turn = g2;
                        em_c = sqrt1m2_normal(em_s);
                    } else {
                        // isotropic; a table draws its row u1 first (when it has several), then these two are its u2
                        // (em_turn) and u3: one set of draw sites for both
                        if (tabled && ptab[0] > 1.0) u1 = rng_uniform(rng);
                        double g1 = rng_uniform(rng), g2 = rng_uniform(rng);
                        em_turn = g1;
                        em_c = 2.0 * g2 - 1.0;
                        em_s = sqrt1m2_normal(em_c);
                        u3 = g2;
                    }
                    if (tabled) {   // about the incoming direction (PvtPhaseTables)
                        if constexpr (ROUGH >= kExtAligned) {   // ... or about the director of an aligned emitter (PvtAlignTables)
                            double ax = dir.x, ay = dir.y, az = dir.z;
                            align_axis(A.fd, frec, cu - cbase, ax, ay, az);
                            if constexpr (MESH || SEENW == 1) dir = phase_table_turn_call(ptab, wl, u1, em_turn, u3, ax, ay, az);
                            else dir = phase_table_turn(ptab, wl, u1, em_turn, u3, ax, ay, az);
                        } else {
                            if constexpr (MESH || SEENW == 1) dir = phase_table_turn_call(ptab, wl, u1, em_turn, u3, dir.x, dir.y, dir.z);
                            else dir = phase_table_turn(ptab, wl, u1, em_turn, u3, dir.x, dir.y, dir.z);
                        }
                    } else {
                        double sp, cp;
                        pvt_sincos2pi(em_turn, &sp, &cp);
                        dir = V3{em_s * cp, em_s * sp, em_c};
                    }
                    em = true;
                    source = cu;
                    if (ctype == PVT_COMP_LUMINOPHORE) {
                        const int ex = T.iv(ci + CI_EMS_X), ec = T.iv(ci + CI_EMS_CDF), en = T.iv(ci + CI_EMS_N);
                        const int eh = T.iv(ci + CI_EMS_HIST);
                        const double ew = T.dv(cd + CD_EMS_W);
                        double p1;
                        if (uf(UF_EMIT_FULL)) {
                            p1 = 0.0;
                        } else {
                            double e_nm = wl;
                            if (uf(UF_EMIT_KT)) {
                                const double kb_ev = 1.380649e-23 / 1.60217662e-19;
                                double e_ev = div_normal(1240.0, e_nm) + 1.5 * kb_ev * 300.0;
                                e_nm = div_normal(1240.0, e_ev);
                            }
                            p1 = interp_clamped<TAB_LDS, kAbsKind>(T, e_nm, ex, ec, en, T.iv(ci + CI_EMS_GX), T.dv(cd + CD_EMS_SCALE_X),
                                                                              eh, T.dv(cd + CD_EMS_RCP_X), ew);
                        }
                        double gamma = p1 + (1.0 - p1) * rng_uniform(rng);
                        wl = interp_clamped<TAB_LDS, kCdfKind>(T, gamma, ec, ex, en, T.iv(ci + CI_EMS_GC), T.dv(cd + CD_EMS_SCALE_C), eh,
                                                                    T.dv(cd + CD_EMS_RCP_C), __builtin_nan(""), eh ? __builtin_nan("") : ew);
                        tau = T.dv(cd + CD_TAU_RAD);
                        ev_kind = PVT_EV_EMIT;
                    } else {
                        ev_kind = PVT_EV_SCATTER;
                    }
                } else {
                    tau = T.dv(cd + CD_TAU_NR);
                    if (ctype == PVT_COMP_REACTOR) { ev_kind = PVT_EV_REACT; t_sel = PVT_REC_REACTED; }
                    else { ev_kind = PVT_EV_NONRADIATIVE; t_sel = PVT_REC_LOST; }
                    t_node = container;
                    terminal = true;
                }
                // radiative / non-radiative lifetime: the last draw of either branch
                if (tau > 0.0) duration += -log_draw(1.0 - rng_uniform(rng)) * tau;
            }
        }

        if constexpr (ROUGH) {
            // ---- volume maps (PvtMapTables): the ABSORB event and the one the component decided on, both at `pos` in
            // `container`, are counted in the node's maps -- every event, in the maps' block of the lane's tally set
            if (uf(UF_VMAP)) {
                if (cls == CLS_ABS)
                    volume_map_call(A.md, reinterpret_cast<unsigned long long*>(A.rec_bins) + (long long)set * A.set_stride_i + A.total_bins,
                                    container, comp, ev_kind, pos.x, pos.y, pos.z, wl_abs, wl);
            }
        }
        PVT_MARK(2);  // classification + absorption + emission draws
        PVT_COUNT(1, alive && ev_component >= 0);            // absorbed
        PVT_COUNT(2, em);                                    // re-emitted
        PVT_COUNT(3, alive && t_normal && ev_kind != PVT_EV_EXIT);   // surface
        PVT_COUNT(4, alive && ev_kind == PVT_EV_EXIT);       // exit
        PVT_COUNT(5, alive && t_sel >= 0);                   // has a tally selector already (terminal kinds)
        PVT_COUNT(6, alive && terminal);
        // ---- local point + outward world normal of the node the event refers to.
        // Shared by EXIT and surface events (re-converged: one copy of the code).
        // Both are pure functions of (t_node, pos, tri1), so the coating / Lambertian code and the
        // x,y,z histogram axes RECOMPUTE them where needed (same arithmetic, same bits) instead of
        // keeping 12 VGPRs alive across the transcendental sites, the register-pressure peak.
        auto local_point = [&]() -> V3 {
            if constexpr (kHoist) {
                if (t_normal) {   // (an event with a normal refers to the node that was hit: its record is in registers)
                    if (node_ident(hr_bits)) return V3{pos.x + hr_t.x, pos.y + hr_t.y, pos.z + hr_t.z};
                    const int m = node_rot(hr_bits) + RT_W2L;
                    return V3{T.dv(m + 0) * pos.x + T.dv(m + 1) * pos.y + T.dv(m + 2) * pos.z + hr_t.x,
                              T.dv(m + 3) * pos.x + T.dv(m + 4) * pos.y + T.dv(m + 5) * pos.z + hr_t.y,
                              T.dv(m + 6) * pos.x + T.dv(m + 7) * pos.y + T.dv(m + 8) * pos.z + hr_t.z};
                }
            }
            const int tr = t_node * ND + ND_T;
            const unsigned long long tb = node_bits(t_node);
            if (node_ident(tb))   // unrotated node: translate only
                return V3{pos.x + T.dv(tr), pos.y + T.dv(tr + 1), pos.z + T.dv(tr + 2)};
            const int m = node_rot(tb) + RT_W2L;
            return V3{T.dv(m + 0) * pos.x + T.dv(m + 1) * pos.y + T.dv(m + 2) * pos.z + T.dv(tr),
                      T.dv(m + 3) * pos.x + T.dv(m + 4) * pos.y + T.dv(m + 5) * pos.z + T.dv(tr + 1),
                      T.dv(m + 6) * pos.x + T.dv(m + 7) * pos.y + T.dv(m + 8) * pos.z + T.dv(tr + 2)};
        };
        auto local_normal = [&](const V3& lp) -> V3 {   // outward normal (_kernel.pyx:359-400)
            const int gp = t_node * ND + ND_PARAMS;
            // (every caller stands at a surface event: the node is the one that was hit -- tail function: its record is in registers)
            const int gt = kHoist ? node_geom(hr_bits) : node_geom(node_bits(t_node));
            auto param = [&](int a) -> double {
                if constexpr (kHoist) return a == 0 ? hr_g.x : (a == 1 ? hr_g.y : hr_g.z);
                return T.dv(gp + a);
            };
            if (MESH && gt == PVT_GEOM_MESH) {   // face normal of the crossed triangle (geometry/mesh.py:63-86)
                const pvt::MeshTri* tr = A.tris + tri1;
                return V3{tr->n[0], tr->n[1], tr->n[2]};
            }
            if (gt == PVT_GEOM_BOX) {
                // The reference scans -x, +x, -y, +y, -z, +z for the face nearest to the point, a later face
                // winning only when strictly nearer (_kernel.pyx:359-377).  Per axis that is the smaller of
                // |p + h| and |p - h| (the + face only when strictly smaller), and across axes the first
                // smallest: the same six distances and the same comparisons, without the running triple.
                const double hx = 0.5 * param(0), hy = 0.5 * param(1), hz = 0.5 * param(2);
                const double mx = pvt_fabs(lp.x - (-1.0) * hx), px = pvt_fabs(lp.x - hx);
                const double my = pvt_fabs(lp.y - (-1.0) * hy), py = pvt_fabs(lp.y - hy);
                const double mz = pvt_fabs(lp.z - (-1.0) * hz), pz = pvt_fabs(lp.z - hz);
                const double cx = __builtin_fmin(px, mx), cy = __builtin_fmin(py, my), cz = __builtin_fmin(pz, mz);   // (no NaNs here)
                const bool use_y = cy < cx;
                const double cxy = __builtin_fmin(cy, cx);
                const bool use_z = cz < cxy;
                const double sx = px < mx ? 1.0 : -1.0, sy = py < my ? 1.0 : -1.0, sz = pz < mz ? 1.0 : -1.0;
                return V3{(!use_y && !use_z) ? sx : 0.0, (use_y && !use_z) ? sy : 0.0, use_z ? sz : 0.0};
            }
            if (gt == PVT_GEOM_SPHERE) {
                double mag = pvt_sqrt(dot3(lp, lp));
                return V3{lp.x / mag, lp.y / mag, lp.z / mag};
            }
            if (ROUGH && !GRID && (gt == PVT_GEOM_FRUSTUM || gt == PVT_GEOM_CONICOID)) {   // (no node grid holds either: plan_node_grid)
                // (a conicoid's four parameters from global memory, the node being the lane's own)
                double q0 = param(0), q1 = param(1), q2 = param(2), q3 = __builtin_nan("");
                if (gt == PVT_GEOM_CONICOID) {
                    const double* cq = T.hd + (int)pvt_d2u(q1);
                    q0 = cq[0]; q1 = cq[1]; q2 = cq[2]; q3 = cq[3];
                }
                return quadric_normal_call(q0, q1, q2, q3, lp.x, lp.y, lp.z);
            }
            if (ROUGH && !GRID && gt == PVT_GEOM_POLYHEDRON)   // (likewise; the rows from global memory, where the spectra of large scenes are read)
                return polyhedron_normal_call(T.hd + (int)pvt_d2u(param(1)), (int)pvt_d2u(param(2)), lp.x, lp.y, lp.z);
            double half = 0.5 * param(0);
            double tol = 1e-8 + 1e-5 * pvt_fabs(half);
            if (pvt_fabs(lp.z + half) <= tol) return V3{0.0, 0.0, -1.0};
            if (pvt_fabs(lp.z - half) <= tol) return V3{0.0, 0.0, 1.0};
            double r = pvt_sqrt(lp.x * lp.x + lp.y * lp.y);
            return V3{lp.x / r, lp.y / r, 0.0};
        };
        if (alive && t_normal) {
            const V3 nloc = local_normal(local_point());
            const unsigned long long tb = kHoist ? hr_bits : node_bits(t_node);
            if (node_ident(tb)) {
                nrm = nloc;
            } else {
                const int q = node_rot(tb) + RT_L2W;
                nrm.x = T.dv(q + 0) * nloc.x + T.dv(q + 1) * nloc.y + T.dv(q + 2) * nloc.z;
                nrm.y = T.dv(q + 3) * nloc.x + T.dv(q + 4) * nloc.y + T.dv(q + 5) * nloc.z;
                nrm.z = T.dv(q + 6) * nloc.x + T.dv(q + 7) * nloc.y + T.dv(q + 8) * nloc.z;
            }
            if constexpr (MESH) {
                // EXTENSION (meshes): a flight of thousands of length units ends short of the face, or beyond it, by the
                // rounding of its length -- ulp(t) / 2, 4.5e-13 at t = 3 755 -- which is more than kEps: from there the next
                // intersection would find the SAME face ahead and cross it a second time.  The landing point is put back on
                // the face's plane along the ray when it is off it by more than kEps / 4 (never in a scene of ordinary size:
                // there the distance is a few 1e-16, and nothing changes).  oracle/pvt_oracle.c does the same, bit for bit.
                if (ev_kind != PVT_EV_EXIT && node_geom(tb) == PVT_GEOM_MESH) {
                    const V3 lp = local_point();
                    const pvt::MeshTri* tr = A.tris + tri1;
                    const double off = ((lp.x - tr->v[0]) * nloc.x + (lp.y - tr->v[1]) * nloc.y) + (lp.z - tr->v[2]) * nloc.z;
                    const double back = -off / dot3(nrm, dir);
                    // (only what the flight's own rounding explains, a few ulp of its length: a larger distance -- a grazing ray
                    // on a sliver, whose stored normal is itself only so good -- stays as it is; flights of ordinary length never get here)
                    if (pvt_fabs(back) > 0.25 * kEps && pvt_fabs(back) < 2e-15 * t0) {
                        pos.x = pos.x + dir.x * back; pos.y = pos.y + dir.y * back; pos.z = pos.z + dir.z * back;
                        travelled += back;
                    }
                }
            }
        }

        PVT_MARK(3);  // frame + normal
        // ---- incidence geometry -----------------------------------------------------
        // Fresnel's formulas take the cosine of the incidence angle (the dot product itself) and its sine (the
        // composition pvt_sqrt1m2); the comparison with the critical angle is a comparison of cosines (host-
        // proven threshold); the ANGLE is only what recorders accumulate, so its acos is taken when a first
        // crossing is tallied (a queue of 64 per wave, below).
        const bool surf = alive && t_normal && ev_kind != PVT_EV_EXIT;
        bool flip = false;       // the normal is used flipped along the ray (nf = -nrm)
        double ddot = 0.0;       // nf . dir, before the clamp
        double ac_arg = 1.0;
        if (alive && t_normal) {
            if (ev_kind == PVT_EV_EXIT) {
                ac_arg = __builtin_fmin(pvt_fabs(dot3(nrm, dir)), 1.0);
            } else {
                ddot = dot3(nrm, dir);
                if (ddot < 0.0) {   // flip the normal along the ray; its dot product is then the negation, bit for bit
                    flip = true;
                    ddot = -ddot;
                }
                ac_arg = __builtin_fmin(ddot, 1.0);   // (non-negative after the flip; the reference also clamps at -1)
            }
        }
        if (alive && t_normal) t_cos = ac_arg;
        const bool fres = surf && (kHoist ? hr_surf : T.iv(ev_hit * NI + NI_SURF)) == PVT_SURF_FRESNEL;
        const double c1 = ac_arg, s1 = fres ? sqrt1m2_normal(ac_arg) : 0.0;   // cos / sin of the incidence angle

        PVT_MARK(4);  // cosines of the incidence / exit angle
        if (surf) {
            // ---- Fresnel / coating decision at the surface (:865-895) ------------
            const int hit = ev_hit, container = ev_container, adjacent = ev_adjacent;
            double r = 0.0, n1 = 0.0, n2 = 0.0, rn2 = 0.0;
            if (fres) {  // unpolarised Fresnel, 1.0 beyond the critical angle (:406-419)
                // (tail function: the container's index was read for the clock, the far side's and the pair's constants with
                // the hit node's record -- all right after the node loop)
                n1 = kHoist ? n_container : T.dv(container * ND + ND_N);
                n2 = kHoist ? hr_n2 : T.dv(adjacent * ND + ND_N);
                // what depends on the refractive indices alone is tabulated per pair of index CLASSES
                int kc = container, ka = adjacent;
                if (!kHoist && !uf(UF_BY_NODE)) { kc = T.iv(container * NI + NI_NCLS); ka = T.iv(adjacent * NI + NI_NCLS); }
                const int ncls_d = L.ncls_d, n_cls = L.n_cls;
                rn2 = kHoist ? hr_rn2 : T.dv(ncls_d + ka * 2 + 1);
                if (!kHoist && uf(UF_DISP)) {   // (the tail function has looked them up with the records above)
                    n1 = n_container;               // (the clock's: the same node at the same wavelength)
                    n2 = index_at(adjacent, n2);
                    rn2 = div_normal(1.0, n2);
                }
                // critical angle asin(n2/n1): a function of the node pair, tabulated by the host
                // with the same pvt_asin (small scenes), else computed here
                bool tir;
                // (the reference compares acos(c1) with the critical angle; the host has turned that into a
                // comparison of c1 itself wherever it could prove the two agree for every double)
                const bool crit_tab = uf(UF_CRIT);
                const double cc = kHoist ? hr_cc : (crit_tab ? T.dv(L.ccrit_d + kc * n_cls + ka) : __builtin_nan(""));
                // (lean: every pair the scene can produce has a proven threshold -- prove_lean's last clause -- so the
                // arm that evaluates the reference's expression is not compiled)
                if (LEAN != kLeanOff || cc == cc) tir = c1 < cc;
                else {   // (rare: the threshold could not be proven, or the scene has too many indices for the tables)
                    if (kHoist && !uf(UF_BY_NODE)) { kc = T.iv(container * NI + NI_NCLS); ka = T.iv(adjacent * NI + NI_NCLS); }
                    // (a pair with a dispersive side has a NaN angle in the table: its quotient is formed here, with n at
                    // the photon's wavelength)
                    const double crit = crit_tab ? T.dv(L.crit_d + kc * n_cls + ka) : __builtin_nan("");
                    if (crit == crit) tir = pvt_acos(c1) > crit;
                    else tir = n2 < n1 && pvt_acos(c1) > pvt_asin(uf(UF_DISP) ? div_normal(n2, n1) : div_known(n2, n1, T.dv(ncls_d + kc * 2 + 1)));
                }
                if (tir) {
                    r = 1.0;
                } else {
                    double q = div_known(n1, n2, rn2) * s1;
                    double k = sqrt_normal(1.0 - q * q);
                    double rs1 = n1 * c1 - n2 * k, rs2 = n1 * c1 + n2 * k;
                    const double as = div_normal(rs1, rs2);   // (the reference writes each quotient twice)
                    double rs = as * as;
                    double rp1 = n1 * k - n2 * c1, rp2 = n1 * k + n2 * c1;
                    const double ap = div_normal(rp1, rp2);
                    double rp = ap * ap;
                    r = 0.5 * (rs + rp);
                }
            }
            int coat = -1;
            if (uf(UF_COATED) && fres) {
                const int cs = T.iv(hit * NI + NI_KSTART), ce = cs + T.iv(hit * NI + NI_KCOUNT);
                // (only the lanes whose node carries coatings; on an unrotated node the normal in the node's frame IS the
                // world normal computed above, bit for bit -- the same local_normal, not rotated -- so it is not recomputed)
                V3 lpos{0, 0, 0}, nloc = nrm;
                if (cs < ce) {
                    lpos = local_point();
                    if (!node_ident(kHoist ? hr_bits : node_bits(hit))) nloc = local_normal(lpos);
                }
                const double nl3[3] = {nloc.x, nloc.y, nloc.z}, pl3[3] = {lpos.x, lpos.y, lpos.z};
                for (int c = cs; c < ce && coat < 0; c++) {
                    bool ok = true;
                    bool okf = true;   // (the extension variants keep the facet's answer apart: a row may cover any normal)
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        double f = T.dv(L.coat_d + c * KD + KD_FACET + a);
                        if (pvt_fabs(nl3[a] - f) > 1e-8 + 1e-5 * pvt_fabs(f)) {
                            if constexpr (ROUGH) okf = false;
                            else ok = false;
                        }
                        if (!(pl3[a] > T.dv(L.coat_d + c * KD + KD_LO + a) && pl3[a] < T.dv(L.coat_d + c * KD + KD_HI + a))) ok = false;
                    }
                    if constexpr (ROUGH) {
                        // (scenes with a patterned coating, PvtCoatingPatternTables) a row whose region holds the point: its
                        // any-facet flag may overrule the normal test, and its pattern, if it has one, must have the cell set
                        if (uf(UF_CPAT)) {
                            if (ok) ok = coat_pattern_call(A.gd + A.pd_d, c, okf ? 1 : 0, lpos.x, lpos.y, lpos.z) != 0;
                        } else {
                            ok = ok && okf;
                        }
                    }
                    if (ok) coat = c;
                }
                if (coat >= 0) {
                    // a coating sets the reflectivity -- except beyond the critical angle when it
                    // transmits by Fresnel refraction: no refracted ray exists there
                    double cr = T.dv(L.coat_d + coat * KD + KD_REFL);
                    const bool keep_tir = r == 1.0 && T.iv(L.coat_i + coat * KI + KI_TMODE) != 1;
                    if (uf(UF_CTAB) && !keep_tir) {   // (scenes with reflectivity tables only) R(wavelength, angle of incidence)
                        const int q = L.coat_i + coat * KI, nw = T.iv(q + KI_TNW);
                        if (nw > 0) {
                            const double* tab = TAB_LDS == 1 ? T.ld : T.hd;   // (where the spectra are read from)
                            const double *wls = tab + T.iv(q + KI_TW), *angs = tab + T.iv(q + KI_TA), *vals = tab + T.iv(q + KI_TV);
                            const int na = T.iv(q + KI_TNA);
                            if constexpr (MESH) cr = coat_table_r_call(wls, nw, angs, na, vals, wl, c1);
                            else cr = coat_table_r(wls, nw, angs, na, vals, wl, c1);
                        }
                    }
                    if (cr >= 0.0 && !keep_tir) r = cr;
                }
            }
            // (scenes with a rough node) a microfacet normal m for lanes whose hit node is rough and whose point no coating
            // covers: Fresnel about m, then the direction about m (PvtSurfaceTables); draws u_a, u_b before u
            bool rough = false, rough_reflect = false;
            if constexpr (ROUGH) {   // (the variants of scenes with a rough node only: the smooth ones keep their step loop)
              if (uf(UF_ROUGH) && fres && coat < 0) {
                const double alpha = T.sd(A.rough_d + hit);
                if (alpha > 0.0) {
                    const RoughEvent e = rough_event_call(alpha, nrm.x, nrm.y, nrm.z, dir.x, dir.y, dir.z, n1, n2, rng.s0, rng.s1,
                                                          rng.s2, rng.s3);
                    dir = V3{e.dx, e.dy, e.dz};
                    rng = Rng{e.s0, e.s1, e.s2, e.s3};
                    rough = true;
                    rough_reflect = e.reflect != 0;
                }
              }
            }
            // (scenes with an absorbing coating) A of the coating that covers the point (PvtCoatingAbsorbTables): the draw is
            // taken when R > 0 or A > 0, and u in [R, R + A) ends the photon here.  Beyond the critical angle on a coating
            // with Fresnel transmission R is 1 and no u reaches A.
            double ab = 0.0;
            if constexpr (ROUGH) {
                if (uf(UF_CABS) && coat >= 0) {
                    const double* tab = TAB_LDS == 1 ? T.ld : T.hd;   // (where the spectra are read from)
                    ab = coat_absorb_call(tab, tab + A.cabs_d, coat, wl, c1);
                }
            }
            double u = 1.0;
            if ((r > 0.0 || (ROUGH && ab > 0.0)) && !rough) u = rng_uniform(rng);
            if (rough ? rough_reflect : u < r) {
                bool lamb = false;
                if (coat >= 0) lamb = T.iv(L.coat_i + coat * KI + KI_RMODE) == 1;
                if (lamb) {
                    // cosine-weighted about the incoming side's normal, in the node frame
                    double side = dot3(nrm, dir) < 0.0 ? 1.0 : -1.0;
                    V3 nloc = nrm;   // (unrotated node: the world normal is the local one)
                    if (!node_ident(node_bits(hit))) nloc = local_normal(local_point());
                    V3 mm{side * nloc.x, side * nloc.y, side * nloc.z};
                    double p1 = rng_uniform(rng), p2 = rng_uniform(rng);
                    V3 sd = lambert_direction(p1, p2);
                    double sign = mm.z < 0.0 ? -1.0 : 1.0;
                    double a = -1.0 / (sign + mm.z);
                    double b = mm.x * mm.y * a;
                    V3 t1v{1.0 + sign * mm.x * mm.x * a, sign * b, -sign * mm.x};
                    V3 t2v{b, sign + mm.y * mm.y * a, -mm.y};
                    V3 dl{sd.x * t1v.x + sd.y * t2v.x + sd.z * mm.x, sd.x * t1v.y + sd.y * t2v.y + sd.z * mm.y,
                          sd.x * t1v.z + sd.y * t2v.z + sd.z * mm.z};
                    const int q = node_rot(node_bits(hit)) + RT_L2W;
                    dir.x = T.dv(q + 0) * dl.x + T.dv(q + 1) * dl.y + T.dv(q + 2) * dl.z;
                    dir.y = T.dv(q + 3) * dl.x + T.dv(q + 4) * dl.y + T.dv(q + 5) * dl.z;
                    dir.z = T.dv(q + 6) * dl.x + T.dv(q + 7) * dl.y + T.dv(q + 8) * dl.z;
                } else if (!rough) {  // specular (:422-433): nf is nrm flipped along dir, dd their dot product (formed above)
                    const V3 nf{flip ? -nrm.x : nrm.x, flip ? -nrm.y : nrm.y, flip ? -nrm.z : nrm.z};
                    const double dd = ddot;
                    dir = V3{dir.x - 2.0 * dd * nf.x, dir.y - 2.0 * dd * nf.y, dir.z - 2.0 * dd * nf.z};
                }
                ev_kind = PVT_EV_REFLECT;
                t_sel = (container != hit) ? PVT_REC_REFLECTED : -1;
            } else if (ROUGH && ab > 0.0 && u < r + ab) {
                // absorbed by the coating: a terminal surface row with the incoming direction, tallied by the hit node's
                // `detected` recorders; the lane ends as after NONRADIATIVE
                ev_kind = PVT_EV_DETECT;
                t_sel = PVT_RECX_DETECTED;
                terminal = true;
            } else {
                bool matched = false;
                if (coat >= 0) matched = T.iv(L.coat_i + coat * KI + KI_TMODE) == 1;
                if (fres && !matched && !rough) {  // Snell, vector form (:436-446)
                    double n = div_known(n1, n2, rn2);
                    const V3 nf{flip ? -nrm.x : nrm.x, flip ? -nrm.y : nrm.y, flip ? -nrm.z : nrm.z};
                    const double dd = ddot;   // dir . nf
                    double c = sqrt_normal(1.0 - n * n * (1.0 - dd * dd));
                    double sign = dd < 0.0 ? -1.0 : 1.0;
                    double k = sign * (c - sign * n * dd);
                    dir = V3{n * dir.x + k * nf.x, n * dir.y + k * nf.y, n * dir.z + k * nf.z};
                }
                ev_kind = PVT_EV_TRANSMIT;
                t_sel = (container == hit) ? PVT_REC_ESCAPING : PVT_REC_ENTERING;
            }
            // (scenes with a scattering coating) a row whose mode is a lobe: the body above has run the row's stand-in
            // mode -- specular; Fresnel for a lobe about "refracted", matched for one about "normal" or "straight" -- and
            // left the axis in `dir`; the lobe's draws follow u (include/pvtrace_hip.h, "Scattering coatings")
            if constexpr (ROUGH) {
                if (uf(UF_CLOBE) && coat >= 0 && ev_kind != PVT_EV_DETECT) {
                    const bool tr = ev_kind == PVT_EV_TRANSMIT;
                    const int q = A.clobe_i + coat * kCl + (tr ? kClTTab : kClRTab);
                    const int at = T.si(q);
                    if (at >= 0) {
                        const double* tab = (TAB_LDS == 1 ? T.ld : T.hd) + at;
                        const bool out = flip != tr;   // N_out = s N for a reflection, -s N for a transmission; s = +1 where N . d < 0 (`flip`)
                        const double so = out ? 1.0 : -1.0;
                        double u1 = 0.0;
                        if (tab[0] > 1.0) u1 = rng_uniform(rng);
                        const double u2 = rng_uniform(rng), u3 = rng_uniform(rng);
                        dir = coat_lobe_call(tab, T.si(q + 1) == PVT_LOBE_NORMAL ? 1 : 0, wl, u1, u2, u3, dir.x, dir.y, dir.z,
                                             so * nrm.x, so * nrm.y, so * nrm.z);
                    }
                }
            }
            // Fused exit (tally launches of a scene that is ONE unrotated box in an empty, unobserved world; the
            // host sets the flag).  A photon that has just been sent away from the box's surface on the OUTSIDE
            // can only leave the scene: its next step would find no crossing of the (convex) box, one crossing of
            // the root, draw nothing (the world has no absorber), log nothing and fire no recorder (nobody
            // listens to the root) -- so it ends here and its lane is refilled a step earlier.  "No crossing of
            // the box" is not taken on trust: the reference's slab test would see, on the face's axis, the
            // distances (h - s*o_a) / |d_a| =: g / dn to the plane the photon stands on (a rounding error that may
            // have either sign) and a negative one to the plane behind it, so the box's far distance is at most
            // g / dn -- below kEps, hence ignored (_kernel.pyx:271-276), whenever g <= kEps/2 * dn; g is formed
            // with the very operations the next step would use (o = pos + t, h = 0.5 * size).  A photon that
            // cannot be cleared this way (grazing departures) simply takes its next step.
            // (A photon a coating absorbed was sent nowhere: the test below names the two kinds it is written for.)
            if (!RECORD && !MESH && uf(UF_FUSE_EXIT) && !terminal && count < k_maxsteps && (!ROUGH || ev_kind != PVT_EV_DETECT) &&
                (ev_kind == PVT_EV_REFLECT ? container == k_root : adjacent == k_root)) {
                const V3 lp = local_point();
                const int gp = hit * ND + ND_PARAMS;
                const double h = kHoist ? 0.5 * (pvt_fabs(nrm.x) * hr_g.x + pvt_fabs(nrm.y) * hr_g.y + pvt_fabs(nrm.z) * hr_g.z)
                                        : 0.5 * (pvt_fabs(nrm.x) * T.dv(gp) + pvt_fabs(nrm.y) * T.dv(gp + 1) + pvt_fabs(nrm.z) * T.dv(gp + 2));
                const double g = h - dot3(nrm, lp), dn = dot3(nrm, dir);
                if (dn > 0.0 && g <= (0.5 * kEps) * dn) {
                    terminal = true;
                    c_fused += 1u;
                }
            }
        }

        PVT_MARK(5);  // fresnel / reflect / refract
        // ================= deferred event: log row + tallies ==============
        if (alive && ev_kind >= 0)
            log_row<RECORD, TAIL>(A, rec_slot, nev, ev_kind, ev_hit, ev_container, ev_adjacent, ev_component, source, pos,
                            dir, ev_normal, nrm, wl, travelled, duration);

        // Lane-parallel tally.  Each lane walks the (host-precomputed) list of recorders that
        // can fire for ITS (node, selector) — different lanes handle different recorders in
        // the same trip — reading the recorder rows from LDS with per-lane addresses and
        // adding into the workgroup accumulators with per-lane LDS atomics (hardware
        // serialises same-address lanes; no wave-uniform recorder loop, no scalar-load
        // chains, no software scan).  Recorder order per lane is ascending, as in the
        // reference's loop (_kernel.pyx:517-556).
        if (uf(UF_HAS_REC)) {
            // Facet recorders whose facets have distinct dominant axes (the usual "one recorder
            // per box face") are found in O(1): the host files each under the bin (dominant axis,
            // sign) of its facet, the lane looks up the bin of ITS normal and verifies that one
            // recorder with the full tolerance test (its first trip).  Everything else is walked.
            int cs = 0, cn = 0, rbin = -1;
            if (alive && t_sel >= 0) {
                int cb = t_node;       // the node's block of the candidate tables
                bool listened = true;
                if (!uf(UF_BY_NODE)) {   // (scenes of many nodes: only the nodes somebody listens to have one)
                    cb = T.iv(t_node * NI + NI_CAND);
                    listened = cb >= 0;
                    cb = listened ? cb : 0;
                }
                // (the eighth selector, PVT_RECX_DETECTED: its blocks -- one per candidate node -- and lists lie behind the
                // guide tables at KArgs::dcand_i, its `start` absolute in the int blob)
                const bool det = ROUGH && t_sel == PVT_RECX_DETECTED;
                const int key = det ? A.dcand_i + cb * 8 : L.cand_i + (cb * 7 + t_sel) * 8;
                if (listened) {
                    cs = det ? T.si(key) - L.cand_list : T.iv(key);
                    cn = det ? T.si(key + 1) : T.iv(key + 1);
                }
                if (listened && t_normal) {
                    const double ax = pvt_fabs(nrm.x), ay = pvt_fabs(nrm.y), az = pvt_fabs(nrm.z);
                    int b = (ax >= ay && ax >= az) ? (nrm.x > 0.0 ? 1 : 0)
                          : (ay >= az)             ? (nrm.y > 0.0 ? 3 : 2)
                                                   : (nrm.z > 0.0 ? 5 : 4);
                    rbin = det ? T.si(key + 2 + b) : T.iv(key + 2 + b);
                }
            }
            // trip t of a lane: its bin recorder first (if any), then its list -- so lanes served by
            // the bin table and lanes served by a list share the same trips
            const int nb = rbin >= 0 ? 1 : 0, ntrips = nb + cn;
            for (int j = 0;; j++) {
                const unsigned long long trip = __ballot(j < ntrips);
                if (trip == 0ull) break;
                if (tq_n + __popcll(trip) > kTallyQ) tally_flush();   // room for one record per lane of this trip
                bool push = false;
                int push_r = 0;
                if (j < ntrips) {
                    const int entry = j < nb ? rbin : (ROUGH && t_sel == PVT_RECX_DETECTED) ? T.si(L.cand_list + cs + j - nb)
                                                                                           : T.iv(L.cand_list + cs + j - nb);
                    const int r = entry & (kRecPlain - 1);
                    const int ri = L.rec_i + r * RI;
                    bool match = true;
                    const bool plain = LEAN || (entry & kRecPlain) != 0;   // nothing to check (see kRecPlain; lean: every entry)
                    const int smode = plain ? 0 : T.iv(ri + RI_SRC_MODE);  // source filter (extension)
                    if (smode != 0) {
                        if (smode == 1) match = source < 0;
                        else if (smode == 2) match = source >= 0;
                        else match = source == T.iv(ri + RI_SRC_ID);
                    }
                    if (!plain && match && T.iv(ri + RI_HAS_FACET) != 0) {
                        const int rd = L.rec_d + r * RD;
                        const double atol = T.dv(rd + RD_ATOL);
                        if (!t_normal) match = false;
                        else if (pvt_fabs(T.dv(rd + RD_FACET) - nrm.x) > atol) match = false;
                        else if (pvt_fabs(T.dv(rd + RD_FACET + 1) - nrm.y) > atol) match = false;
                        else if (pvt_fabs(T.dv(rd + RD_FACET + 2) - nrm.z) > atol) match = false;
                    }
                    if (match) {
                        atomicAdd(&acc_cross[r], 1ull);
                        const unsigned long long bit = 1ull << (r & 63);
                        bool first;
                        if constexpr (SEENW == 1) {
                            first = !(seen.w[0] & bit);
                            seen.w[0] |= bit;
                        } else {
                            const int w = r >> 6;
                            const unsigned long long cur = w == 0 ? seen.w[0] : w == 1 ? seen.w[1] : w == 2 ? seen.w[2] : seen.w[3];
                            first = !(cur & bit);
                            if (w == 0) seen.w[0] |= bit; else if (w == 1) seen.w[1] |= bit;
                            else if (w == 2) seen.w[2] |= bit; else seen.w[3] |= bit;
                        }
                        push = first;
                        push_r = r;
                    }
                }
                // A first crossing is parked (recorder, wavelength, cosine, times[, local position]); the queue is
                // wave-private, so plain LDS stores at ranks of a ballot are all it takes.
                const unsigned long long pm = __ballot(push);
                if (pm != 0ull) {
                    const int at = tq_n + (int)rank_in(pm);
                    if (push) {
                        tq_r[at] = push_r;
                        tq_d[at] = wl; tq_d[kTallyQ + at] = t_cos; tq_d[2 * kTallyQ + at] = duration; tq_d[3 * kTallyQ + at] = travelled;
                        if (uf(UF_TQ_POS)) {
                            const V3 lpos = local_point();   // position in the recorder node's frame
                            tq_d[4 * kTallyQ + at] = lpos.x; tq_d[5 * kTallyQ + at] = lpos.y; tq_d[6 * kTallyQ + at] = lpos.z;
                        }
                        if constexpr (ROUGH) {
                            if (uf(UF_TQ_COUNT)) tq_d[tq_count_at + at] = pvt_u2d(hcount);   // (the counters before this step's row)
                            if (uf(UF_ORIGIN)) {   // the origins that are read, each in its column behind the counters'
                                const double* o = origin_slot();
                                const unsigned int read = origin_mask();
                                int col = tq_count_at + (uf(UF_TQ_COUNT) ? kTallyQ : 0);
#pragma unroll
                                for (int k = 0; k < kOriginWords; k++)
                                    if ((read >> k) & 1u) { tq_d[col + at] = o[k]; col += kTallyQ; }
                            }
                        }
                    }
                    tq_n += __popcll(pm);
                    if constexpr (ROUGH) {
                        // ---- ray capture (PvtCaptureTables): the first matches of this trip, appended to their recorders' rows
                        // with the values the event's log row holds
                        if (uf(UF_CAPTURE)) {
                            if (A.cap_rows != nullptr)
                                capture_call(A.cap_tab, A.cap_rows + (long long)set * A.cap_total * kCapWords,
                                             A.cap_cursor + (long long)set * A.n_rec, push, push_r, gidx, pos.x, pos.y, pos.z,
                                             dir.x, dir.y, dir.z, wl, travelled, duration, source, hcount);
                        }
                    }
                }
            }
        }

        if constexpr (ROUGH) {
            // ---- photon event counters: the row this step wrote last, counted now that the tally has seen the photon as it
            // arrived (an ABSORB row before it is of no counted kind: at most one counted row per step, kCountRowsPerStep)
            if (uf(UF_COUNT)) {
                if (alive && ev_kind == PVT_EV_EMIT) hcount += 1ull;
                if (alive && ev_kind == PVT_EV_SCATTER) hcount += 1ull << kCountBits;
                if (alive && ev_kind == PVT_EV_REFLECT) hcount += 1ull << (2 * kCountBits);
            }
        }
        PVT_MARK(6);  // log + tally
        if (alive && terminal) {
            if constexpr (RECORD) {
                if (rec_slot >= 0) A.log_counts[rec_slot] = nev;
            }
            c_steps += (unsigned int)count;   // the trips this photon took, in whichever launches and lanes
            alive = false;
        }
    }

#if PVT_STATS
    if (lane == 0) {
        unsigned long long* c = reinterpret_cast<unsigned long long*>(A.cursor) + 1;
        atomicAdd(c + 0, st_iters); atomicAdd(c + 1, st_lane_steps);
        atomicAdd(c + 2, st_drain_iters); atomicAdd(c + 3, st_drain_lane_steps);
        atomicAdd(c + 4, 1ull);
        for (int k = 0; k < 7; k++) atomicAdd(c + 8 + k, st_t[k]);
        atomicAdd(c + 15, (ws & WS_SOLO) ? 1ull : 0ull);
        for (int k = 0; k < 8; k++) atomicAdd(c + 16 + k, st_c[k]);
        for (int k = 0; k < 4; k++) atomicAdd(c + 24 + k, st_g[k]);
    }
#endif
#if PVT_TIMELINE
    if (!TAIL && A.timeline && lane == 0) {
        unsigned long long* o = A.timeline + ((unsigned long long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * 8;
        o[0] = tl_t[0]; o[1] = tl_t[1]; o[2] = tl_t[2]; o[3] = tl_t[3]; o[4] = wall_clock64(); o[5] = tl_iters;
        // (word 7: valid | the wave ended as the last of its workgroup << 1 | HW_ID register << 32: wave slot, SIMD, CU, SE)
        o[6] = __builtin_readcyclecounter() - tl_c0;
        // (the XCC_ID register, hwreg 20, says which of the eight dies: bits 2-5 of this word)
        o[7] = 1ull | ((ws & WS_SOLO) || tail_n > 0 ? 2ull : 0ull) | ((unsigned long long)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 15u) << 2) |
               ((unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) << 32);
    }
#endif
    tally_flush();   // the first crossings still parked
    {   // this wave's share of the step counters, into the workgroup's sums
        unsigned long long* const cnt = reinterpret_cast<unsigned long long*>(ctl + CTL_COUNT);
        if (lane == 0) atomicAdd(cnt, (unsigned long long)c_iters);
        atomicAdd(cnt + 1, (unsigned long long)c_steps);
        atomicAdd(cnt + 2, (unsigned long long)c_fused);
    }
#if PVT_TIMELINE
    if constexpr (TAIL) {   // (the caller has written the wave's record: word 1 becomes when this function was entered, 4 when it
                            // returns, 5 gets its trips << 32)
        if (A.timeline && lane == 0) {
            unsigned long long* o = A.timeline + ((unsigned long long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * 8;
            o[1] = tl_t[0]; o[4] = wall_clock64(); o[5] |= tl_iters << 32;
        }
    }
#endif
    if constexpr (TAIL) return;   // (the caller leaves the workgroup)
    // The rest of its photons' histories, when this wave was the last of a draining workgroup (see the drain), then the
    // workgroup's epilogue -- both as FUNCTIONS, called here at the very end: nothing of the loop above is live across either
    // call, so the loop's register allocation does not know of them (a value that were live across a call would be spilled
    // where it is defined and reloaded where it is used, the loop included), and what the epilogue needs -- the
    // accumulators' places in LDS, the tally set, the output pointers -- is worked out inside it instead of being held
    // (or spilled) for the kernel's whole life.
    {
        const KArgsSegment ak = (KArgsSegment)__builtin_amdgcn_kernarg_segment_ptr();
        if constexpr (kTailCall) {
            if (tail_n > 0) {
                // (behind an opaque copy: every caller passes the same address expression, which interprocedural constant
                // propagation would otherwise put back into the callee -- table lookups and all)
                unsigned int lds_at = (unsigned int)(unsigned long long)(__attribute__((address_space(3))) double*)smem_of_kernel;
                asm volatile("" : "+s"(lds_at));
                if constexpr (SOLO) tail_run_solo<LEAN>((const KArgs*)ak, tail_n, lds_at);
                else tail_run<RECORD, TAB_LDS, SEENW, MESH, GRID, ROUGH, LEAN>((const KArgs*)ak, tail_n, lds_at);
            }
        }
        leave_workgroup<TAB_LDS>((const KArgs*)ak);
    }

}

// The last wave of a draining workgroup finishes its photons here (see the drain in trace_body): the step loop alone, as a
// function -- the kernels' own loop keeps its registers whatever this one needs, and what is specific to a wave that runs
// alone on its SIMD (every step is latency, nothing overlaps) can be done here without a price on the bulk.
template <bool RECORD, int TAB_LDS, int SEENW, bool MESH, bool GRID, int ROUGH, int LEAN>
__device__ __attribute__((noinline)) void tail_run(const KArgs* kernel_args, int total, unsigned int lds) {
    // The kernel's arguments, read where the kernel itself reads them.  The pointer arrives in vector registers: it is made
    // a scalar again (readfirstlane) and a pointer into the constant address space, so that the fields come through the
    // scalar cache and what is decided by them stays wave-uniform.  (The kernel-argument intrinsic itself returns garbage
    // inside a called function -- build/probe, ROCm 7.0 -- hence the explicit argument.)
    const unsigned long long bits = (unsigned long long)kernel_args;
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)bits), hi = __builtin_amdgcn_readfirstlane((unsigned int)(bits >> 32));
    const KArgsSegment ak = (KArgsSegment)(((unsigned long long)hi << 32) | lo);
    trace_body<RECORD, TAB_LDS, SEENW, false, MESH, GRID, true, ROUGH, LEAN>(*(const KArgs*)ak, __builtin_amdgcn_readfirstlane(total),
                                                                __builtin_amdgcn_readfirstlane(lds));
}

template <int LEAN>
__device__ __attribute__((noinline)) void tail_run_solo(const KArgs* kernel_args, int total, unsigned int lds) {
    const unsigned long long bits = (unsigned long long)kernel_args;   // (see tail_run)
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)bits), hi = __builtin_amdgcn_readfirstlane((unsigned int)(bits >> 32));
    const KArgsSegment ak = (KArgsSegment)(((unsigned long long)hi << 32) | lo);
    trace_body<false, 1, 1, false, false, false, true, 0, LEAN, false, true>(*(const KArgs*)ak, __builtin_amdgcn_readfirstlane(total),
                                                                         __builtin_amdgcn_readfirstlane(lds));
}

// Entry points.  Every variant runs four waves per SIMD.  Scenes of analytic shapes, tally launches and
// history-keeping ones alike, need 108-118 registers, none spilled (the build switches machine-level loop-invariant
// code motion off, which had kept every constant of the loop in a register of its own -- with it the history variants
// needed 144 registers and ran three waves; at four they are 3-10 % faster).  Mesh variants would take 144-154
// registers: held to 128 they park about sixty values in scratch around the BVH walk (photon state the walk does not
// touch), and the fourth wave is worth more than that costs -- the walk is a chain of dependent loads: +8 ... +19 % in
// the pipelined stream, 3.1 -> 2.7 ms for a single 10^6-photon launch on the 327 680-face ball (five waves: worse).
template <bool RECORD, int TAB_LDS, int SEENW, bool EMIT, bool MESH>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kMeshWaves, kMeshWaves))) trace_kernel(KArgs A) {
    trace_body<RECORD, TAB_LDS, SEENW, EMIT, MESH>(A);
}
template <bool RECORD, int TAB_LDS, int SEENW, bool EMIT>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) trace_kernel_w4(KArgs A) {
    trace_body<RECORD, TAB_LDS, SEENW, EMIT, false>(A);
}
template <bool RECORD, int SEENW, bool EMIT>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) trace_kernel_grid(KArgs A) {
    trace_body<RECORD, 1, SEENW, EMIT, false, true>(A);
}
// The same three families for scenes with a rough node (KArgs::rough_d >= 0) or a concentration field (KArgs::fd): the
// microfacet sampler of the surface branch and the field march of the volume branch are compiled into these alone, so the
// smooth variants keep their registers, spills and text bit for bit.  (A call of
// the sampler from the smooth loop spilled 20-30 vector registers of every variant: the surface branch holds more values
// than the callee-saved registers take.)
template <bool RECORD, int TAB_LDS, int SEENW, bool EMIT, bool MESH, int EXT = kExtRough>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kMeshWaves, kMeshWaves))) trace_kernel_rough(KArgs A) {
    trace_body<RECORD, TAB_LDS, SEENW, EMIT, MESH, false, false, EXT>(A);
}
template <bool RECORD, int TAB_LDS, int SEENW, bool EMIT, int EXT = kExtRough>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) trace_kernel_rough_w4(KArgs A) {
    trace_body<RECORD, TAB_LDS, SEENW, EMIT, false, false, false, EXT>(A);
}
template <bool RECORD, int SEENW, bool EMIT, int EXT = kExtRough>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) trace_kernel_rough_grid(KArgs A) {
    trace_body<RECORD, 1, SEENW, EMIT, false, true, false, EXT>(A);
}
// The lean family (trace_body's LEAN): scenes the host has proven plain -- see prove_lean.  Tables in LDS, at most 64
// recorders, no mesh, no node grid, no rough / field / map extension.
// EVEN: moreover every spectrum is a constant or lies on a proven even grid (the headline's kind); without it the tables
// are searched as in the generic variants, step tables aside.
template <bool RECORD, bool EMIT, bool EVEN>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) trace_kernel_lean_w4(KArgs A) {
    trace_body<RECORD, 1, 1, EMIT, false, false, false, false, EVEN ? kLeanEven : kLeanSearched>(A);
}
// The lean family's tally launches that park (trace_body's PARK): the step loop alone decides their registers.
#ifndef PVT_PARK_WAVES
#define PVT_PARK_WAVES 5
#endif
template <bool EMIT, bool EVEN>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(PVT_PARK_WAVES, PVT_PARK_WAVES))) trace_kernel_lean_park(KArgs A) {
    trace_body<false, 1, 1, EMIT, false, false, false, false, EVEN ? kLeanEven : kLeanSearched, true>(A);
}
// The solo entries (trace_body's SOLO): tally launches of a lean scene that is one box in a lazy root, see prove_solo.
// `park` as trace_kernel_lean_park (five waves, no drain, no tail), `fin` as trace_kernel_lean_w4 (the drain and the tail).
template <bool EMIT, bool EVEN>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(PVT_PARK_WAVES, PVT_PARK_WAVES))) trace_kernel_solo_park(KArgs A) {
    trace_body<false, 1, 1, EMIT, false, false, false, false, EVEN ? kLeanEven : kLeanSearched, true, true>(A);
}
template <bool EMIT, bool EVEN>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) trace_kernel_solo_fin(KArgs A) {
    trace_body<false, 1, 1, EMIT, false, false, false, false, EVEN ? kLeanEven : kLeanSearched, false, true>(A);
}

}  // namespace
