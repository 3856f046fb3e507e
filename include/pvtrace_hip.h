/* pvtrace_hip.h — C ABI of the MI355X photon-tracing engine (libpvtrace_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of pvtrace: the native call
 *     _kernel.trace_bundle(compiled, positions, directions, wavelengths, seed,
 *                          maxsteps, max_events, emit_method, num_threads,
 *                          record_every) -> dict
 * (reference pvtrace/engine/_kernel.pyx:903-1115), which engine.simulate()
 * (pvtrace/engine/api.py:197-246) wraps.  Plain pointers and sizes only; no
 * torch / numpy / HIP types appear in any signature.  INTEGRATION.md shows the
 * ctypes stub a pvtrace maintainer would add.
 *
 * Table layouts, dtypes and tag values are exactly the reference's
 * CompiledScene (pvtrace/engine/compiler.py:25-50, :75-204) so the same arrays
 * can be handed to either engine.  All matrices are row-major 4x4 doubles.
 */
#ifndef PVTRACE_HIP_H
#define PVTRACE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVT_ABI_VERSION 13

/* limits (reference _kernel.pyx:65-68) */
#define PVT_MAX_NODES 128
#define PVT_MAX_RECORDERS 256
#define PVT_MAX_HITS 512

/* event codes == pvtrace.light.event.Event (reference light/event.py:7-16) */
enum {
    PVT_EV_GENERATE = 0, PVT_EV_REFLECT = 1, PVT_EV_TRANSMIT = 2, PVT_EV_ABSORB = 3,
    PVT_EV_NONRADIATIVE = 4, PVT_EV_SCATTER = 5, PVT_EV_EMIT = 6, PVT_EV_EXIT = 7,
    PVT_EV_REACT = 8, PVT_EV_KILL = 9,
    /* EXTENSION within v13 (the reference has no such event): absorbed at a surface by a coating's absorptivity
     * (PvtCoatingAbsorbTables); a terminal surface row */
    PVT_EV_DETECT = 10
};
/* geometry / surface / component / phase / emit-method tags (compiler.py:25-48) */
enum { PVT_GEOM_BOX = 0, PVT_GEOM_SPHERE = 1, PVT_GEOM_CYLINDER = 2, PVT_GEOM_MESH = 3,
       /* EXTENSION (the reference has no such shape): a truncated cone, see below */
       PVT_GEOM_FRUSTUM = 4,
       /* EXTENSION (the reference has no such shape): a convex polyhedron, a table of planes, see PvtPolyhedronTables */
       PVT_GEOM_POLYHEDRON = 5,
       /* EXTENSION (the reference has no such shape): a solid of revolution of a conic, see below */
       PVT_GEOM_CONICOID = 6 };
/* PVT_GEOM_FRUSTUM: a truncated cone along the node's z axis, centred on its origin; geom_params = (length L,
 * radius_bottom r0 at z = -L/2, radius_top r1 at z = +L/2, 0).  L finite and > 0; r0, r1 finite and >= 0, not both 0
 * (else PVT_ERR_INVALID).  Convex, so the container rule of the analytic shapes applies unchanged.  The arithmetic is
 * fixed -- IEEE double, no contraction, correctly rounded division and square root -- and pvtrace_amd.geometry.Frustum
 * performs the same operations in the same order, so host and device agree bit for bit:
 *     half = 0.5*L;  rm = 0.5*(r0 + r1);  k = (r1 - r0)/L
 *     e = rm + k*o.z;  f = k*d.z;  s = d.x*d.x + d.y*d.y
 *     a = s - f*f;  b = 2.0*((o.x*d.x + o.y*d.y) - e*f);  c = (o.x*o.x + o.y*o.y) - e*e;  disc = b*b - 4.0*a*c
 *   side, disc >= 0 and fabs(a) > 0x1p-20*(s + f*f):  sq = sqrt(disc);  t = (-b - sq)/(2.0*a), then (-b + sq)/(2.0*a)
 *     (with r0 == r1 every intermediate is the capped cylinder's);
 *   side, disc >= 0 otherwise (the ray runs nearly along a generator):  q = -0.5*(b + copysign(sq, b));
 *     t = c/q where q != 0, then t = q/a where fabs(a) > 1e-300;
 *   a root counts when z = o.z + t*d.z has -half < z < half and t > EPS;
 *   caps, fabs(d.z) > 1e-300: t = (-half - o.z)/d.z with x*x + y*y <= r0*r0, then t = (half - o.z)/d.z with r1, t > EPS;
 *   normal: tol = 1e-8 + 1e-5*fabs(half); fabs(p.z + half) <= tol: (0,0,-1); fabs(p.z - half) <= tol: (0,0,1); else
 *     rz = rm + k*p.z, w = k*rz, m = sqrt((p.x*p.x + p.y*p.y) + w*w), n = (p.x/m, p.y/m, (-w)/m).
 * Additive under ABI 13.  A scene with such a node runs the PVT_VARIANT_ROUGH family (with or without meshes), is never
 * lean, and gets no node grid.  Which entry takes the type: pvt_scene_create_origin, pvt_scene_lean_check and the
 * host-buffer entries; every older pvt_scene_create* entry refuses it as before ("unknown geometry type"), as they refuse
 * the extension selectors and properties -- no entry was added. */
/* PVT_GEOM_CONICOID: the solid of revolution { x*x + y*y < q(z), -L/2 < z < L/2 } of the conic q(z) = p0 + p1*z + p2*z*z,
 * along the node's z axis, centred on its origin; geom_params = (L, p0, p1, p2).  Ellipsoids and spheroids, spherical caps
 * (dome and plano-convex lenses), paraboloids, convex hyperboloid sheets; the cylinder and the cone as degenerate cases.
 * The parameters must be finite, L > 0, q > 0 on the open interval, q(+-L/2) >= -2^-40*S with
 * S = |p0| + |p1|*half + |p2|*half*half, and the solid convex: sqrt(q) is concave exactly when p1*p1 - 4*p0*p2 >= 0, and
 * a profile with p1*p1 - 4*p0*p2 < -2^-40*(p1*p1 + 4|p0*p2|) is refused (a cone written as (rm + k*z)^2 is not, for one
 * rounding).  Each problem is PVT_ERR_INVALID with its own message.  Convex, so the container rule of the analytic
 * shapes applies unchanged.  An end with q(+-half) <= 2^-40*S is a POLE: it has no cap, no
 * cap candidate and no cap normal.
 * The arithmetic.  Host and device perform the same operations in the same order, in IEEE double, with no contraction and
 * correctly rounded `/` and square root:
 *     half = 0.5*L;  g = 0.5*p1 + p2*o.z;  s = d.x*d.x + d.y*d.y
 *     a = s - (p2*d.z)*d.z
 *     b = 2.0*((o.x*d.x + o.y*d.y) - g*d.z)
 *     c = (o.x*o.x + o.y*o.y) - (p0 + (p1 + p2*o.z)*o.z)
 *     disc = b*b - 4.0*a*c
 *     if disc >= 0:
 *         sq = sqrt(disc);  qq = -0.5*(b + copysign(sq, b))
 *         if qq != 0:            t = c/qq
 *         if fabs(a) > 1e-300:   t = qq/a
 * ONE branch: always the cancellation-free roots.  A root is a crossing when z = o.z + t*d.z has -half < z < half
 * strictly and t > EPS_ZERO, in the order written.
 * Caps follow, -z then +z.  Each is tried when fabs(d.z) > 1e-300 and that end is no pole: t = (-+half - o.z)/d.z;
 * x = o.x + t*d.x, y likewise; the cap is a candidate when x*x + y*y <= q_end, q_end being the Horner value
 * p0 + (p1 + p2*z_end)*z_end, and t > EPS_ZERO.
 * Normal, with tol = 1e-8 + 1e-5*fabs(half): at an end that is no pole, fabs(p.z -+ half) <= tol gives (0, 0, -+1), -z
 * first; otherwise w = 0.5*p1 + p2*p.z, m = sqrt((p.x*p.x + p.y*p.y) + w*w), n = (p.x/m, p.y/m, (-w)/m).
 * Additive under ABI 13.  A node record holds three shape parameters, so the four of such a node lie behind everything
 * else in the scene's double blob and the record names where (as the plane rows of a polyhedron).  A scene with such a
 * node runs the PVT_VARIANT_ROUGH family (with or without meshes), is never lean, and gets no node grid.  Which entry
 * takes the type: pvt_scene_create_polyhedra alone, with or without polyhedron tables; every older pvt_scene_create*
 * entry, pvt_scene_lean_check and the host-buffer pvt_trace_bundle* entries refuse it as "unknown geometry type" -- no
 * entry was added. */
enum { PVT_SURF_FRESNEL = 0, PVT_SURF_NULL = 1 };
enum { PVT_COMP_ABSORBER = 0, PVT_COMP_SCATTERER = 1, PVT_COMP_LUMINOPHORE = 2, PVT_COMP_REACTOR = 3 };
/* The built-in phase functions, about +z of the WORLD frame (a component) or of the light's frame (PVT_DIR_*), on two
 * draws in stream order (_kernel.pyx:455-476).  PVT_PHASE_HG with |g| >= 2.220446049250313e-13: s = 2 u0 - 1,
 * q = (1 - g g) / (1 + g s), cos = (1 / (2 g)) ((1 + g g) - q q), azimuth 2 pi u1.  PVT_PHASE_CONE: sin = sqrt(u0)
 * sin(theta_max), azimuth 2 pi u1.  Otherwise (isotropic, and HG below that |g|): azimuth 2 pi u0, cos = 2 u1 - 1.  The
 * partner of the sine / cosine is sqrt((1 - c)(1 + c)); the direction is (sin cos(az), sin sin(az), cos).
 * DEPARTURE from the reference: the HG cosine cancels for small |g| and at the ends of the draw grid and can leave
 * [-1, 1] by a few ulp (g = 0.3 at u0 = 0 gives a cosine below -1; about one draw in 10^5 at |g| <= 1e-10), where the
 * reference's acos is NaN.  It is clamped to [-1, 1] before its sine is formed, as the table turn's cosine is.  An
 * in-range value keeps its bits, so the engine departs from the reference only where the reference returns NaN -- the
 * precedent of the critical-angle rule.  tests/exact_emission.py restates all of this and holds every implementation. */
enum { PVT_PHASE_ISOTROPIC = 0, PVT_PHASE_HG = 1, PVT_PHASE_CONE = 2,
       /* EXTENSION (the reference engine rejects it, compiler.py:300-310; its Python path and its scene-spec parser have it,
        * material/utils.py:176-186, cli/parse.py:166-167): cosine-weighted about +z, theta = asin(sqrt(p1)), phi = 2 pi p2 */
       PVT_PHASE_LAMBERTIAN = 3,
       /* EXTENSION within v13: a tabulated phase function (PvtPhaseTables), sampled about the INCOMING direction;
        * only pvt_scene_create_phase takes it */
       PVT_PHASE_TABLE = 4 };
enum { PVT_EMIT_KT = 0, PVT_EMIT_REDSHIFT = 1, PVT_EMIT_FULL = 2 };
/* recorder selectors (engine/recorder.py:45-53) */
enum {
    PVT_REC_ENTERING = 0, PVT_REC_ESCAPING = 1, PVT_REC_REFLECTED = 2, PVT_REC_LOST = 3,
    PVT_REC_REACTED = 4, PVT_REC_KILLED = 5, PVT_REC_EXIT = 6
};
/* EXTENSION within v13: the selector of a recorder that counts the photons a coating of its node absorbed (PVT_EV_DETECT),
 * from either side; a surface selector owned by the node that was HIT.  Spelled outside the enum above, which lists the
 * reference's selectors and nothing else (tests/test_golden_units.py holds every constant of that enum to the reference's
 * dict): the Python side keeps it in recorder.EXTENSION_EVENTS for the same reason. */
#define PVT_RECX_DETECTED 7
/* histogram properties (engine/recorder.py:33-41): what hist_prop_a / hist_prop_b name */
enum {
    PVT_PROP_WAVELENGTH = 0, PVT_PROP_ANGLE = 1, PVT_PROP_DURATION = 2, PVT_PROP_PATHLENGTH = 3,
    PVT_PROP_X = 4, PVT_PROP_Y = 5, PVT_PROP_Z = 6
};
/* EXTENSION within v13 -- photon event counters.  Spelled outside the enum above for the reason PVT_RECX_DETECTED is; the
 * Python side keeps them in recorder.EXTENSION_PROPERTIES.  The contract (the Python Histogram and CapturedRays docstrings
 * state the same; the kernel and engine.tally both follow it):
 *  1. A photon carries three counters, all zero when a light emits it: emissions, scatterings and reflections, the rows of
 *     kind PVT_EV_EMIT, PVT_EV_SCATTER and PVT_EV_REFLECT in its history -- REFLECT at every node, from either side, whether
 *     Fresnel, total internal, coating, rough or Lambertian.
 *  2. At a matching event a counter's value is the number of such rows that STRICTLY PRECEDE the matching row in the ray's
 *     full history: the counters describe the photon as it arrives.  A PVT_REC_REFLECTED recorder sees 0 at a ray's first
 *     reflection.
 *  3. A histogram bins the counter as the double of the same value, by the rule of every other property.  No moments are
 *     added: rec_sums keeps its eight sums per recorder.
 *  4. The counters draw no random number and change no other result: a scene that uses them traces the same histories and
 *     the same other tallies, bit for bit.
 *  5. The values do not depend on launch geometry, carrying, tally-set grouping, the device list or which code finishes a
 *     photon.
 * A scene COUNTS when a histogram reads a counter or a recorder is captured (word 11 of a captured row holds them).  Its
 * launches run the PVT_VARIANT_ROUGH family; each counter is a 20-bit field and a step writes at most one row of a counted
 * kind, so a launch of a counting scene with maxsteps > 2^20 - 1 is refused (PVT_ERR_INVALID) and the loop never
 * saturates.  Which entry takes the ids: pvt_scene_create_absorb, whose acceptance was extended -- no entry was added.
 * Every older pvt_scene_create* entry, and with them the host-buffer entries, refuse an id above PVT_PROP_Z ("histogram
 * property out of range"); before this check nothing looked at the ids, and one past 6 read beyond the kernel's tally
 * queue. */
#define PVT_PROPX_EMISSIONS 7
#define PVT_PROPX_SCATTERINGS 8
#define PVT_PROPX_REFLECTIONS 9
/* EXTENSION within v13 -- launch origin: the photon as it was LAUNCHED, where every property above describes it at the
 * event.  The Python side keeps the ids in recorder.ORIGIN_PROPERTIES.  The contract (the Python Histogram docstring states
 * the same; the kernel and engine.tally both follow it):
 *  1. A photon carries four doubles: the wavelength and the position of its GENERATE row, bit for bit what the launch's
 *     ray arrays (PvtRays) hold for it or what device emission sampled.  They are fixed when a lane claims the ray and
 *     never recomputed.
 *  2. The position is in the scene ROOT's frame, the frame lights emit in and the event log stores -- deliberately NOT in
 *     the recorder node's frame, unlike PVT_PROP_X .. PVT_PROP_Z: bins stay exact against the launch arrays, with no
 *     transform in between.  For an untransformed node the two frames agree.
 *  3. A histogram bins them by the unchanged rule of every other property, at the recorder's first match.
 *  4. They draw no random number and change no other result, bit for bit.
 *  5. They do not depend on launch geometry, carrying, tally-set grouping, the device list or which code finishes a photon.
 *  6. No moments are added, no capture columns (the 96-byte row stays), and no recorder filters by them.
 * A scene that reads one runs the PVT_VARIANT_ROUGH family; reading origins alone makes a scene count nothing (no limit on
 * maxsteps).  Which entry takes the ids: pvt_scene_create_origin alone.  Every older pvt_scene_create* entry,
 * pvt_scene_create_absorb included, and the host-buffer entries refuse them ("histogram property out of range"). */
#define PVT_PROPX_ORIGIN_WAVELENGTH 10
#define PVT_PROPX_ORIGIN_X 11
#define PVT_PROPX_ORIGIN_Y 12
#define PVT_PROPX_ORIGIN_Z 13
/* error codes (negative returns) */
enum {
    PVT_OK = 0,
    PVT_ERR_INVALID = -1,     /* bad argument; maps to ValueError            */
    PVT_ERR_TOO_MANY_NODES = -2, /* > PVT_MAX_NODES; reference raises ValueError (_kernel.pyx:929-930) */
    PVT_ERR_HIP = -3,         /* HIP runtime failure; see pvt_last_error()   */
    PVT_ERR_NO_DEVICE = -4
};

/* ---- scene tables: HOST pointers, read once by pvt_scene_create ---------
 * Field-for-field the attributes _kernel.trace_bundle reads off `compiled`
 * (_kernel.pyx:933-1017), plus the coating extension (coat_*), which the
 * reference engine has no counterpart for (its compiler rejects non-Fresnel
 * delegates, compiler.py:237-247).  n_coatings may be 0 with NULL coat_* rows. */
typedef struct PvtSceneTables {
    int32_t n_nodes, root_id, n_components, n_abs, n_ems;
    int32_t n_recorders, n_hists, total_bins, n_coatings,
            n_coat_tables;   /* reflectivity tables of the coatings (the ctab_* fields at the end; was reserved, 0) */
    /* per node */
    const int32_t* geom_type;
    const double* geom_params;      /* (n_nodes,4) box: sx,sy,sz  sphere: r  cyl: length, radius */
    const double* local_to_world;   /* (n_nodes,4,4) */
    const double* world_to_local;   /* (n_nodes,4,4) */
    const double* refractive_index;
    const int32_t* surface_type;
    const int32_t* comp_start;
    const int32_t* comp_count;
    const int32_t* coat_start;
    const int32_t* coat_count;
    /* per component */
    const int32_t* comp_type;
    const double* comp_qy;
    const double* comp_tau_rad;
    const double* comp_tau_nr;
    const int32_t* comp_phase_type;
    const double* comp_phase_param;
    const int32_t* comp_abs_start;
    const int32_t* comp_abs_n;
    const int32_t* comp_ems_start;
    const int32_t* comp_ems_n;
    /* pooled spectra */
    const double* abs_x;            /* (n_abs) */
    const double* abs_y;
    const double* ems_x;            /* (n_ems) */
    const double* ems_cdf;
    /* recorders */
    const int32_t* rec_node;
    const int32_t* rec_event;
    const int32_t* rec_has_facet;
    const double* rec_facet;        /* (max(n_recorders,1),3) */
    const double* rec_atol;
    const int32_t* rec_hist_start;
    const int32_t* rec_hist_n;
    /* histograms */
    const int32_t* hist_prop_a;     /* PVT_PROP_*; PVT_PROPX_* through the entries that know them */
    const int32_t* hist_prop_b;     /* -1: 1-D */
    const int32_t* hist_na;
    const int32_t* hist_nb;
    const double* hist_lo_a;
    const double* hist_hi_a;
    const double* hist_lo_b;
    const double* hist_hi_b;
    const int32_t* hist_offset;
    /* coatings (extension) */
    const double* coat_facet;       /* (n_coatings,3) local-frame outward normal */
    const double* coat_lo;          /* (n_coatings,3) open local AABB, -inf/inf = unbounded */
    const double* coat_hi;
    const double* coat_reflectivity;/* <0: keep Fresnel */
    const int32_t* coat_reflect_mode;   /* 0 specular, 1 lambertian; >= PVT_COAT_LOBE: a lobe ("Scattering coatings" below) */
    const int32_t* coat_transmit_mode;  /* 0 Fresnel refraction, 1 index matched; >= PVT_COAT_LOBE: a lobe */
    /* recorder source filter (extension; NULL = no filter): 0 any, 1 photons emitted by a
     * light (source id < 0), 2 by any component, 3 by component rec_source_id */
    const int32_t* rec_source_mode;
    const int32_t* rec_source_id;
    /* histogram-sampled spectra (extension; NULL = all interpolated).  The reference engine
     * rejects hist=True distributions (compiler.py:274-279, :313-317); semantics follow the
     * Python Distribution's hist branch (material/distribution.py:82-84, :127-129, :171-176):
     * value(x) = y[#{x_i < x}], sample(p) = x[#{cdf_i < p}], no interpolation. */
    const int32_t* comp_abs_hist;
    const int32_t* comp_ems_hist;
    /* triangle meshes (extension; geom_type PVT_GEOM_MESH).  The reference engine rejects
     * Mesh nodes (compiler.py:220-223); its Python tracer traces them through trimesh
     * (geometry/mesh.py:44-61).  Semantics here: every forward crossing (t > EPS) of the
     * node-local ray with a face is a hit, exactly as for the analytic shapes, so the
     * container rule (_kernel.pyx:684-714) applies unchanged; the normal of a hit is the
     * face normal (geometry/mesh.py:63-86).  The ray/triangle test is the watertight
     * shear-and-edge-function test with a half-plane tie rule for exact zeros, so a ray
     * through a shared edge or vertex crosses the surface exactly once.  Vertices are in
     * the node's local frame (already centred on the centre of mass, mesh.py:17). */
    int32_t n_mesh_vertices, n_mesh_faces;
    const int32_t* mesh_face_start; /* (n_nodes) first face of the node's mesh, 0 if none */
    const int32_t* mesh_face_count; /* (n_nodes) 0 for non-mesh nodes */
    const double* mesh_vertices;    /* (n_mesh_vertices,3) pooled */
    const int32_t* mesh_faces;      /* (n_mesh_faces,3) indices into the pooled vertices */
    const double* mesh_normals;     /* (n_mesh_faces,3) outward unit face normals */
    /* coating reflectivity tables (extension, appended within v13).  A coating row with coat_table[k] >= 0 reflects
     * with R(lambda, theta) of that table instead of coat_reflectivity[k]: lambda the photon's current wavelength (nm),
     * theta the angle of incidence from the normal on the side the photon arrives from; piecewise-linear in lambda,
     * then in theta, clamped at both ends of each axis, each step a + t (b - a).  Beyond the critical angle a coating
     * with Fresnel transmission still reflects totally.  A caller that leaves n_coat_tables 0 may pass a struct that
     * ends at mesh_normals (the size before these fields): nothing past it is read. */
    const int32_t* coat_table;          /* (n_coatings) table of each coating row, -1 = none */
    int32_t n_ctab_wavelength, n_ctab_angle, n_ctab_value, reserved1;   /* lengths of the three pools */
    const int32_t* ctab_nw;             /* (n_coat_tables) wavelengths of the table, >= 1 */
    const int32_t* ctab_na;             /* (n_coat_tables) angles of the table, >= 1 */
    const int32_t* ctab_wl_start;       /* (n_coat_tables) first wavelength in ctab_wavelength */
    const int32_t* ctab_angle_start;    /* (n_coat_tables) first angle in ctab_angle */
    const int32_t* ctab_value_start;    /* (n_coat_tables) first value in ctab_value: na x nw, row-major by angle */
    const double* ctab_wavelength;      /* pooled, nm, strictly increasing per table */
    const double* ctab_angle;           /* pooled, degrees in [0, 90], strictly increasing per table */
    const double* ctab_value;           /* pooled reflectivities in [0, 1] */
} PvtSceneTables;

/* ---- refractive-index tables n(lambda): dispersion (extension within v13, passed to pvt_scene_create_ex) -----------
 * A node with node_table[i] >= 0 refracts with n(lambda) of that table instead of refractive_index[i]: lambda the
 * photon's current wavelength (nm), piecewise-linear, clamped at both ends, each step a + t (b - a), so a table
 * holding a constant gives exactly that constant.  It is read wherever the index is: Fresnel reflectivity, the
 * critical angle and Snell refraction on either side of a surface, and the clock (duration += d n / c, the phase
 * index).  refractive_index[i] of such a node stays a finite positive number (the flattener stores n at the table's
 * first wavelength); the tracer does not use it.  These tables are a separate struct so that PvtSceneTables keeps
 * the length old callers pass. */
typedef struct PvtIndexTables {
    int32_t n_tables;               /* 0 = no dispersion (as a NULL struct) */
    int32_t n_points;               /* length of the wavelength and value pools */
    const int32_t* node_table;      /* (n_nodes) table of each node, -1 = its scalar refractive_index */
    const int32_t* table_n;         /* (n_tables) points of each table, >= 1 */
    const int32_t* table_start;     /* (n_tables) first point of each table in the pools */
    const double* wavelength;       /* (n_points) pooled, nm, finite and strictly increasing per table */
    const double* value;            /* (n_points) pooled indices, finite and positive */
} PvtIndexTables;

/* ---- tabulated phase functions p(theta) (extension within v13, passed to pvt_scene_create_phase) ------------------
 * A component with comp_phase_type PVT_PHASE_TABLE names table comp_table[c] (its comp_phase_param is not read); every
 * other component has comp_table -1.  Unlike the built-ins, which draw about world +z, a table draws the scattering
 * angle about the photon's incoming direction d.  The sampling contract (the Python PhaseFunctionTable is the same):
 *  1. Axis and CDF: mu_j = cos(theta_j) ascending from exactly -1 to exactly 1 (n_mu >= 2 points); each of the
 *     n_wavelength rows is the trapezoid integral of p in mu with a leading 0, divided by its last entry: it rises
 *     (non-decreasing) from exactly 0 to exactly 1.
 *  2. Row, only when n_wavelength > 1: lambda (the photon's current wavelength, nm) clamped into the table's range;
 *     k with lambda_k <= lambda < lambda_k+1, t = (lambda - lambda_k) / (lambda_k+1 - lambda_k) (t = 0 at either
 *     clamped end: the first row below the range, the last above); draw u1, row k+1 if u1 < t, else row k.  u1 is
 *     drawn whenever n_wavelength > 1.
 *  3. Polar angle: draw u2; j = the first segment with C_j+1 > u2 (binary search; zero-mass segments are never chosen);
 *     mu = mu_j + (u2 - C_j) / (C_j+1 - C_j) (mu_j+1 - mu_j), clamped to [-1, 1].
 *  4. Azimuth: draw u3; (sin phi, cos phi) = pvt_sincos2pi(u3); d' = mu d + sqrt(1 - mu^2) (cos phi e1 + sin phi e2),
 *     with the basis of Duff et al. 2017 about d = (x, y, z): s = copysign(1, z), a = -1 / (s + z), b = x y a,
 *     e1 = (1 + s x^2 a, s b, -s x), e2 = (b, s + y^2 a, -y).
 *  5. Draw order: u1 (if drawn), u2, u3 in place of the built-ins' phase draws; a luminophore's wavelength and
 *     delay draws follow as before.
 * A separate struct so that PvtSceneTables and PvtIndexTables keep the lengths old callers pass. */
typedef struct PvtPhaseTables {
    int32_t n_tables;               /* 0 = none (as a NULL struct) */
    int32_t n_points;               /* length of the mu pool */
    int32_t n_wavelength, n_cdf;    /* lengths of the wavelength and CDF pools */
    const int32_t* comp_table;      /* (n_components) table of each component, -1 = a built-in phase function */
    const int32_t* table_nw;        /* (n_tables) rows (wavelengths) of each table, >= 1 */
    const int32_t* table_nmu;       /* (n_tables) mu points of each table, >= 2 */
    const int32_t* wl_start;        /* (n_tables) first wavelength of each table in `wavelength` */
    const int32_t* mu_start;        /* (n_tables) first point of each table in `mu` */
    const int32_t* cdf_start;       /* (n_tables) first CDF entry of each table in `cdf` (nw x nmu, row-major) */
    const double* wavelength;       /* pooled row wavelengths, nm, finite and strictly increasing per table */
    const double* mu;               /* pooled mu axes */
    const double* cdf;              /* pooled CDF rows */
} PvtPhaseTables;

/* ---- rough interfaces (extension within v13, passed to pvt_scene_create_rough) ------------------------------------
 * node_roughness[n] is the GGX (Trowbridge-Reitz) width alpha, finite and 0 <= alpha <= 1, of node n's surface: the
 * HIT node's alpha applies, at points that no coating covers (a covered point behaves as a smooth one, no draw); a
 * NULL struct, n_nodes 0 or every alpha 0 is exactly pvt_scene_create_phase.  The sampling contract (the Python
 * FresnelSurfaceDelegate(roughness=...) is the same):
 *  1. Frame: N is the geometric normal at the hit turned to face the photon (d.N < 0), v = -d, (e1, e2) the basis of
 *     Duff et al. 2017 about N (the expressions of the phase-table contract above), v_l = (v.e1, v.e2, v.N).
 *  2. Microfacet normal (the GGX distribution of visible normals, Heitz 2018, JCGT 7(4)): draw u_a, then u_b;
 *     Vh = normalize(alpha v_l.x, alpha v_l.y, v_l.z); T1 = (-Vh.y, Vh.x, 0) / sqrt(Vh.x^2 + Vh.y^2), (1, 0, 0) when
 *     that sum is 0; T2 = Vh x T1; r = sqrt(u_a), (sin phi, cos phi) = pvt_sincos2pi(u_b); t1 = r cos phi,
 *     s = (1 + Vh.z) / 2, t2 = (1 - s) sqrt(1 - t1^2) + s r sin phi; Nh = t1 T1 + t2 T2 + sqrt(max(0, 1 - t1^2 - t2^2)) Vh;
 *     m_l = normalize(alpha Nh.x, alpha Nh.y, max(0, Nh.z)); m = m_l.x e1 + m_l.y e2 + m_l.z N (v.m > 0).
 *  3. Fresnel about m: cos theta_m = v.m clamped to [0, 1], n1 and n2 at the photon's wavelength, the smooth branch's
 *     Hecht formula; R = 1 where q = n1 / n2 sin theta_m >= 1 (total internal reflection about m).
 *  4. Decision: the reflect-or-transmit draw u as for a smooth interface, only when R > 0.
 *  5. Direction: reflection d' = d - 2 (d.m) m; transmission by the smooth branch's vector form of Snell's law with m
 *     in place of the normal.
 *  6. Fold: a reflected d' with d'.N < 0, or a transmitted d' with d'.N > 0, is mirrored across the tangent plane:
 *     d' <- d' - 2 (d'.N) N (no draw).
 *  7. Draw order: u_a, u_b, then u (if R > 0); event kinds, recorder selectors and the logged normal (the geometric
 *     one) follow the smooth rules.
 * A separate struct so that PvtSceneTables, PvtIndexTables and PvtPhaseTables keep the lengths old callers pass. */
typedef struct PvtSurfaceTables {
    int32_t n_nodes;                /* 0 = none (as a NULL struct), else the scene's n_nodes */
    const double* node_roughness;   /* (n_nodes) GGX alpha of each node's surface, 0 = smooth */
} PvtSurfaceTables;

/* ---- concentration fields (extension within v13, passed to pvt_scene_create_field) --------------------------------
 * A node with node_field[n] >= 0 carries lattice node_field[n]: shape (nx, ny, nz), each >= 1, and finite bounds
 * lower < upper on each axis, in the node's own frame (the frame of its world_to_local).  Each component c of such a
 * node names a value table comp_values[c] of nx ny nz finite values >= 0 (index (ix ny + iy) nz + iz); the components of
 * an unfielded node are not read.  The root node carries no lattice.  The absorption contract (the Python
 * ConcentrationGrid is the same):
 *  1. Cells: h = (upper - lower) / n per axis; a point p lies in cell clamp(floor((p - lower) / h), 0, n - 1) per axis,
 *     so a point outside the box takes the nearest edge cell.  Only the interior planes lower + i h, i = 1 .. n - 1,
 *     are crossed.
 *  2. Coefficient of a cell: alpha_cell = sum_k alpha_k(lambda) c_k[cell], summed in component order.
 *  3. Draw: tau* = -ln(1 - u), drawn as for an unfielded container, on the UNSCALED sum sum_k alpha_k(lambda).
 *  4. March: from the photon's position (s = 0) along its direction up to the surface distance t0, cell by cell; a
 *     cell entered at s_in with accumulated depth tau_in and left at s_out (the next plane crossed, or t0) absorbs at
 *     s_in + (tau* - tau_in) / alpha_cell when that is < s_out; else tau_in grows by alpha_cell (s_out - s_in).  Cells
 *     with alpha_cell = 0 add nothing.  No absorption before t0: the photon reaches the surface.
 *  5. Component: the draw and the cumulative rule of an unfielded container over alpha_k c_k[cell] of the cell the
 *     march absorbed in (not a cell derived again from the rounded position).
 * A 1 x 1 x 1 lattice of value 1 has no interior planes: the march is (tau* - 0) / alpha with the same alpha, and such
 * a scene traces bit for bit as one without fields.  A NULL struct, n_nodes 0 or every node_field -1 is exactly
 * pvt_scene_create_rough.  Field values live in global memory, outside the tables a launch stages in LDS.  A separate
 * struct so that the other table structs keep the lengths old callers pass. */
typedef struct PvtFieldTables {
    int32_t n_nodes;                /* 0 = none (as a NULL struct), else the scene's n_nodes */
    int32_t n_fields;               /* lattices */
    const int32_t* node_field;      /* (n_nodes) lattice of each node, -1 = none */
    const int32_t* field_shape;     /* (n_fields, 3) nx, ny, nz, each >= 1 */
    const double* field_lower;      /* (n_fields, 3) finite, < field_upper on each axis */
    const double* field_upper;      /* (n_fields, 3) */
    int32_t n_components;           /* the scene's n_components */
    int32_t n_values;               /* value tables */
    const int32_t* comp_values;     /* (n_components) value table of each component, -1 = none */
    const int32_t* values_start;    /* (n_values) first value of each table in `values` */
    const int32_t* values_count;    /* (n_values) length of each table: nx ny nz of every lattice that uses it */
    int32_t n_points;               /* length of the value pool */
    int32_t reserved;
    const double* values;           /* (n_points) pooled relative concentrations, finite and >= 0 */
} PvtFieldTables;

/* ---- volume maps (extension within v13, passed to pvt_scene_create_maps) -------------------------------------------
 * Per-voxel integer tallies of the volume events of a node: maps [node_map_start[n], + node_map_count[n]) belong to node
 * n (the runs tile the maps in node order; the root carries none).  A map counts EVERY event of its kind whose container
 * is its node (the `crossings` rule of a recorder, not first-per-ray): map_kind is PVT_EV_ABSORB, PVT_EV_EMIT,
 * PVT_EV_SCATTER, PVT_EV_NONRADIATIVE or PVT_EV_REACT; map_component >= 0 keeps only the events whose component column is
 * that component (one of the node's own).  The contract (the Python VolumeMap and engine.tally.map_histories are the same):
 *  1. The local point is p = R x + t, x the event's world position, bit for bit the `position` of its log row.
 *  2. R and t are the node's rows of PvtSceneTables.world_to_local (what a concentration field's record copies).
 *  3. Each coordinate is evaluated as ((R[a][0] x + R[a][1] y) + R[a][2] z) + t[a], without FMA.
 *  4. Per axis h = (upper - lower) / n (map_h, computed once by whoever fills the tables) and
 *     i = floor((p - lower) / h).
 *  5. The event is inside when 0 <= i <= n - 1 on all three axes and the wavelength bin, if any (map_nw > 0), is in
 *     range: iw = trunc((w - start) / (stop - start) * nw), a Histogram's rule, inside when 0 <= iw <= nw - 1; w is the
 *     wavelength column of the event's row (the incoming wavelength for ABSORB / NONRADIATIVE / REACT / SCATTER, the new
 *     one for EMIT).
 *  6. The slot is ((ix ny + iy) nz + iz) nw' + iw, nw' = max(nw, 1), iw = 0 without a wavelength axis.
 *  7. Every other matching event adds one to the map's single `outside` slot, slot nx ny nz nw' of the map.
 *  8. No clamping: a map may be a region of interest smaller than its node.
 *  9. Hence the sum of a map's slots, `outside` included, is the number of matching events in the node.
 * Where the counts live: map m owns the nx ny nz nw' + 1 int64 slots from map_offset[m] (the maps packed one after the
 * other in map order, map_slots in all, at most PVT_MAX_MAP_SLOTS) of a block that FOLLOWS the recorders' bins:
 * PvtTallies.rec_bins of a scene with maps has total_bins + map_slots elements (pvt_scene_map_slots), the maps' block
 * starting at element total_bins; total_bins keeps the reference's meaning, and tally sets, carried launches and
 * reductions move the maps with the bins.  The kernel adds one to a slot per event with a 64-bit integer atomic in
 * global memory (never staged in LDS, whatever the recorders' bins do), so the counts are exact and independent of
 * summation order, launch geometry, carrying and GPU count.  Map records live in global memory of their own, outside the
 * tables a launch stages in LDS.  A NULL struct, n_nodes 0 or n_maps 0 is exactly pvt_scene_create_field.
 *
 * PATH-LENGTH maps (map_kind PVT_MAP_PATHLENGTH, a value that is no PVT_EV_*; map_component must be -1): not events but the
 * path photons travel in each voxel, the track-length estimator of the fluence, as fixed-point integers -- one count is
 * PVT_FLUENCE_UNIT = 2^-30 of the scene's length unit, so these maps are as exact and as independent of summation order,
 * launch geometry, carrying and GPU count as the others.  They own slots of the same block, laid out the same way.  The
 * contract (the Python VolumeMap and engine.tally.map_histories walk the same way; the kernel and the host follow it
 * operation for operation, without FMA):
 *  1. A SEGMENT is one advance of a photon: from world position x along unit direction d for length L, while the photon's
 *     container is the map's node.  A segment with non-finite L, or L <= 0, adds nothing.
 *  2. Local start: p_a = ((R[a][0] x + R[a][1] y) + R[a][2] z) + t[a].
 *  3. Local direction: u_a = (R[a][0] dx + R[a][1] dy) + R[a][2] dz.
 *  4. R and t are the node's rows of PvtSceneTables.world_to_local.
 *  5. Per axis the planes are lower_a + i h_a for i = 0 .. n_a, written `lower + (double)i * h`.  The cell index c_a runs
 *     over -1 .. n_a; -1 and n_a are the two half-infinite slabs outside the lattice.
 *  6. Start: c_a = clamp(floor((p_a - lower_a) / h_a), -1, n_a).  A NaN gives -1.
 *  7. step_a is the sign of u_a; 0 means the axis never crosses.
 *  8. The plane ahead is i = c_a + 1 for a positive step and i = c_a for a negative one; it exists when 0 <= i <= n_a, and
 *     its parameter is (lower_a + i h_a - p_a) / u_a.  Otherwise the parameter is +inf.
 *  9. The loop is that of the concentration fields' march.  Start with s = 0.  In each pass tmin is the least of the three
 *     parameters; sout = max(min(tmin, L), s); the piece sout - s belongs to the current cell; stop when !(sout < L);
 *     otherwise cross ONE axis whose parameter equals tmin -- ties in the order X, then Y, then Z, the others follow at
 *     zero length -- and then s = sout.
 * 10. A piece of length l adds k = (int64)(l * 2^30 + 0.5).  Nothing is added when k = 0.
 * 11. The piece goes to slot ((cx ny + cy) nz + cz) nw' + iw when every c_a is in 0 .. n_a - 1 and the wavelength bin is in
 *     range, otherwise to the map's single `outside` slot.
 * 12. With a wavelength axis iw is a Histogram's bin (rule 5 above) of the wavelength the photon travels with; out of range
 *     means the whole segment goes to `outside`.
 * 13. No clamping: a map may be smaller than its node.
 * 14. Hence (sum of all slots) * PVT_FLUENCE_UNIT is the path length travelled inside the node, to within half a unit per
 *     piece.  A slot wraps at 2^63 units, about 8.6e9 length units; the `outside` slot of a small map in a large node is
 *     the first to get there.
 * The kernel adds k to a slot with one no-return 64-bit integer atomic in global memory per non-zero piece.  Event maps do
 * not see these records (no event's kind equals PVT_MAP_PATHLENGTH), and a scene without one runs the kernels it ran. */
#define PVT_MAX_MAP_SLOTS (1LL << 26)
#define PVT_MAP_PATHLENGTH 100           /* map_kind of a path-length map: no PVT_EV_* has this value */
#define PVT_FLUENCE_UNIT 9.31322574615478515625e-10   /* 2^-30: the length one count of a path-length map stands for */
typedef struct PvtMapTables {
    int32_t n_nodes;                /* 0 = none (as a NULL struct), else the scene's n_nodes */
    int32_t n_maps;
    const int32_t* node_map_start;  /* (n_nodes) first map of each node */
    const int32_t* node_map_count;  /* (n_nodes) its maps; the runs tile [0, n_maps) in node order */
    const int32_t* map_kind;        /* (n_maps) PVT_EV_ABSORB / EMIT / SCATTER / NONRADIATIVE / REACT, or PVT_MAP_PATHLENGTH */
    const int32_t* map_component;   /* (n_maps) component id (one of the node's), -1 = any (PVT_MAP_PATHLENGTH: -1 only) */
    const int32_t* map_shape;       /* (n_maps, 3) nx, ny, nz, each >= 1 */
    const double* map_lower;        /* (n_maps, 3) finite */
    const double* map_h;            /* (n_maps, 3) cell widths (upper - lower) / n, finite and > 0 */
    const int32_t* map_nw;          /* (n_maps) wavelength bins, 0 = no wavelength axis */
    const double* map_wl_start;     /* (n_maps) finite, < map_wl_stop where map_nw > 0 */
    const double* map_wl_stop;      /* (n_maps) */
    const int64_t* map_offset;      /* (n_maps) first slot of each map in the maps' block */
    int64_t map_slots;              /* slots of all maps, `outside` slots included */
} PvtMapTables;

/* ---- ray capture (extension within v13, passed to pvt_scene_create_capture) -----------------------------------------
 * The rays behind a recorder's `rays` count: recorder r with rec_capture_capacity[r] > 0 keeps one ROW for each ray's
 * first match of that recorder -- the very event that adds to rec_distinct, the moment sums and the histograms -- up to
 * that many rows; rec_capture_start[r] is its first row in the launch's row buffer (the captures packed one after the
 * other in recorder order, capture_rows in all, at most PVT_MAX_CAPTURE_ROWS = 2^24: 1.5 GiB of rows per tally set).
 * A row is a fixed-stride record of PVT_CAPTURE_ROW_WORDS = 12 uint64 words (96 bytes, little endian), written whole by
 * the lane that follows the photon:
 *   word 0     the global ray index, ray_offset + i (int64): the ray's RNG stream is seed + index
 *   words 1-3  position, 4-6 direction, 7 wavelength, 8 path (travelled), 9 clock (duration): bit for bit the columns
 *              of the event's row in the event log
 *   word 10    source (int32, low half: the photon's current source id as the recorder `source` filter sees it, -1 = a
 *              light) | recorder id (high half)
 *   word 11    the photon's event counters as it arrives at that event (PVT_PROPX_*: the rows that strictly precede the
 *              event's row), 20 bits each: emissions | scatterings << 20 | reflections << 40
 * Where the rows and cursors live: caller-owned DEVICE memory handed over per launch (PvtCaptures).  Tally set j of a
 * launch owns rows [j capture_rows, (j + 1) capture_rows) and cursors [j n_recorders, (j + 1) n_recorders); cursors[r]
 * (int64, one per recorder; those of recorders without capture stay untouched) counts the first matches of recorder r
 * -- it equals what the launches added to rec_distinct[r].  The kernel never resets a cursor: the caller zeroes it, and
 * a photon carried into the next launch (PVT_FLAG_CARRY_OUT) appends to the same capture when that launch is given the
 * same buffers.  Rows are reserved per wave (one 64-bit atomic per wave, recorder and tally trip), so their order in
 * the buffer is unspecified.  The contract (the Python CapturedRays and engine.tally.capture_histories state the same):
 *  1. While cursors[r] <= capacity the row set is exact: sorted by index it does not depend on launch geometry,
 *     carrying, tally-set grouping or the device list.
 *  2. Beyond the capacity later arrivals are dropped (the cursor still counts them): min(cursor, capacity) rows are
 *     written, every one a correct row, indices unique.
 *  3. Which rows survive an overflow is unspecified.
 * Capture launches run the PVT_VARIANT_ROUGH family.  A NULL struct, n_recorders 0 or capture_rows 0 is exactly
 * pvt_scene_create_maps. */
#define PVT_MAX_CAPTURE_ROWS (1LL << 24)
#define PVT_CAPTURE_ROW_WORDS 12
typedef struct PvtCaptureTables {
    int32_t n_recorders;                  /* 0 = none (as a NULL struct), else the scene's n_recorders */
    const int64_t* rec_capture_capacity;  /* (n_recorders) rows the recorder may keep, 0 = not captured */
    const int64_t* rec_capture_start;     /* (n_recorders) its first row: the running sum of the capacities */
    int64_t capture_rows;                 /* sum of the capacities */
} PvtCaptureTables;

/* ---- absorbing coatings (extension within v13, passed to pvt_scene_create_absorb) -----------------------------------
 * coat_absorptivity[k] is the probability A that a photon ARRIVING at a point covered by coating row k is absorbed there
 * -- per incident photon, like the EQE of a solar cell, not a share of what was not reflected; a row with coat_table[k] >= 0
 * takes A(lambda, theta) of that table instead, laid out, looked up and clamped as the reflectivity tables of
 * PvtSceneTables (ctab_*): lambda the photon's current wavelength, theta the angle of incidence.  The contract (the Python
 * Coating docstring states the same; the kernel and the host tracer both follow it):
 *  1. R is what the surface branch computes for the point without absorption: Fresnel, or the coating's scalar or table
 *     value; beyond the critical angle R stays 1 unless the coating's transmission is index matched.
 *  2. A is the coating's absorptivity at the photon's current wavelength and the angle of incidence the reflectivity table
 *     uses (the same arc cosine of the same cosine).
 *  3. One uniform draw u decides, the draw that decides reflection, taken when R > 0 or A > 0: u < R reflects; else
 *     u < R + A (one double addition) absorbs; else the photon is transmitted.
 *  4. Where R + A > 1 the absorbed share is 1 - R and nothing is transmitted (Fresnel R near grazing incidence).
 *  5. Beyond the critical angle on a coating with Fresnel transmission R = 1: the photon is totally reflected and A never
 *     applies.  An absorber bonded to the surface is reflectivity 0 with index-matched transmission.
 * An absorbed photon writes one PVT_EV_DETECT row and ends, as after PVT_EV_NONRADIATIVE: hit, container and adjacent as a
 * REFLECT or TRANSMIT row at that point would have them, the position the hit point, the direction the INCOMING one,
 * unchanged, the normal as logged for surface events, wavelength, path and clock as at arrival.  A recorder with selector
 * PVT_RECX_DETECTED on the node that was hit counts it, with facet, source filter, histograms and capture as for the
 * other surface selectors (its angle from the incoming direction and the normal).  No photon draws an additional random
 * number: a coating with A = 0 traces bit for bit as one without, and a point with A > 0 whose R is exactly 0 takes the
 * one draw it would not take otherwise.  A covered point of a rough node behaves as a smooth one, as before.  Launches of
 * such a scene run the PVT_VARIANT_ROUGH family; the host-buffer entries know no absorbing coatings.  A NULL struct,
 * n_coatings 0 or every A zero with no table is exactly pvt_scene_create_capture.  A separate struct so that the other
 * table structs keep the lengths old callers pass. */
typedef struct PvtCoatingAbsorbTables {
    int32_t n_coatings;                 /* 0 = none (as a NULL struct), else the scene's n_coatings */
    int32_t n_tables;                   /* absorptivity tables */
    const double* coat_absorptivity;    /* (n_coatings) scalar A of each coating row, finite and in [0, 1]; 0 = absorbs nothing */
    const int32_t* coat_table;          /* (n_coatings) table of each coating row, -1 = its scalar A (NULL when n_tables is 0) */
    int32_t n_wavelength, n_angle, n_value, reserved;   /* lengths of the three pools */
    const int32_t* table_nw;            /* (n_tables) wavelengths of the table, >= 1 */
    const int32_t* table_na;            /* (n_tables) angles of the table, >= 1 */
    const int32_t* wl_start;            /* (n_tables) first wavelength in `wavelength` */
    const int32_t* angle_start;         /* (n_tables) first angle in `angle` */
    const int32_t* value_start;         /* (n_tables) first value in `value`: na x nw, row-major by angle */
    const double* wavelength;           /* pooled, nm, finite and strictly increasing per table */
    const double* angle;                /* pooled, degrees in [0, 90], strictly increasing per table */
    const double* value;                /* pooled absorptivities, finite and in [0, 1] */
} PvtCoatingAbsorbTables;

/* ---- patterned coatings (extension within v13, passed to pvt_scene_create_pattern) ----------------------------------
 * Where a coating covers.  coat_any_facet[k] != 0 skips the normal test of coating row k (its coat_facet is ignored: a
 * flag of the row, no magic normal); coat_pattern[k] >= 0 names the mask lattice of the row, in the node's own frame, the
 * frame coat_lo / coat_hi are in.  The rule (the Python Coating docstring states the same; the kernel and the host
 * delegate both follow it):
 *  1. A coating covers a point when all three hold: its facet matches (or the row's any-facet flag is set); its region
 *     contains the point; it has no pattern, or the point's cell is set.
 *  2. The point is the local point the coating match already uses: pos + t on an unrotated node, the row products
 *     ((R0 x + R1 y) + R2 z) + t otherwise, without FMA (what the volume maps' rules 1-3 state).
 *  3. Per bounded axis h = (upper - lower) / n and i = floor((p - lower) / h).  The point is inside when
 *     0 <= i <= n - 1 on every bounded axis.  The slot is (ix ny + iy) nz + iz.
 *  4. A point outside the lattice is not covered.  There is no clamping: a pattern may be smaller than its face.
 *  5. The first covering coating wins.  Several coatings with disjoint masks give a palette.
 *  6. The decision draws no random number.  A pattern of all ones whose lattice contains the face traces bit for bit as
 *     the same coating without a pattern; a pattern of all zeros traces bit for bit as the scene with that coating
 *     removed.  Coverage is binary: a dot pattern is rendered into the mask at the resolution it needs.
 *  7. Roughness keeps its rule: it applies where no coating covers, so the holes of a pattern on a rough node are rough.
 * An axis with bounded == 0 has one cell and index 0 for every point; its lower and h are not read.  The masks live in
 * global memory, outside what a launch stages in LDS; a covered-or-not decision is one byte load.  Launches of such a
 * scene run the PVT_VARIANT_ROUGH family; the host-buffer entries know no patterns.  A NULL struct, n_coatings 0, or no
 * row with a pattern or an any-facet flag is exactly pvt_scene_create_origin.  A separate struct so that the other table
 * structs keep the lengths old callers pass. */
typedef struct PvtCoatingPatternTables {
    int32_t n_coatings;                 /* 0 = none (as a NULL struct), else the scene's n_coatings */
    int32_t n_patterns;                 /* mask lattices */
    const int32_t* coat_any_facet;      /* (n_coatings) != 0: the row's normal test is skipped */
    const int32_t* coat_pattern;        /* (n_coatings) pattern of each coating row, -1 = none */
    const int32_t* shape;               /* (n_patterns,3) cells per axis, >= 1 */
    const int32_t* bounded;             /* (n_patterns,3) 0 = the axis is unbounded and has one cell */
    const double* lower;                /* (n_patterns,3) lower bound per bounded axis, finite */
    const double* h;                    /* (n_patterns,3) cell width per bounded axis, finite and > 0 */
    const int64_t* mask_start;          /* (n_patterns) first byte of the pattern's mask in `mask`: nx ny nz bytes, z fastest */
    const uint8_t* mask;                /* pooled masks, != 0 = the cell is covered */
    int64_t n_mask;                     /* bytes in `mask`, at most 2^26 */
} PvtCoatingPatternTables;

/* ---- aligned components (extension within v13, passed to pvt_scene_create_aligned) -----------------------------------
 * Uniaxial alignment of a component's transition dipoles about a director n with order parameter S = <P2>: dichroic
 * absorption and dipole emission.  No polarisation is tracked: both laws are the average over unpolarised light, so the
 * polarisation memory between a dipole emission and the next absorption is ignored.  With mu = d . n, the absorption of
 * unpolarised light travelling along d and the emission density along d are f(mu; S) = 1 - S P2(mu), P2(mu) = 1.5 mu^2 - 0.5,
 * -0.5 <= S <= 1.  comp_align[c] >= 0 names the record of component c.  The absorption rule (the Python Alignment docstring
 * states the same; the kernel and the host tracer both follow it):
 *  1. The flattener lowers each aligned component's director ONCE to the scene root's frame as a unit vector n_w: with
 *     the rows R0, R1, R2 of the node's rotation to the root, n_w,i = (Ri,0 nx + Ri,1 ny) + Ri,2 nz, then divided by
 *     sqrt((x x + y y) + z z) of the result, without FMA.  `axis` holds n_w.
 *  2. At the free-path site mu_k = (dx nx + dy ny) + dz nz, without FMA, clamped to [-1, 1].
 *  3. f_k = 1.0 - S_k (1.5 (mu_k mu_k) - 0.5), exactly these operations in this order.
 *  4. A component without alignment has f_k = 1 and is not multiplied.
 *  5. The depth draw happens where and when an unaligned container draws, on the UNSCALED sum of alpha_k(lambda) >
 *     the clear-medium threshold (the decision of the concentration fields): S = 1 along the director does not change
 *     who draws.
 *  6. tau* = -ln(1 - u); the depth is tau* / sum_k alpha_k f_k through the division the site already uses.
 *  7. The depth is +inf when the scaled sum is exactly 0.
 *  8. The component is picked by the unaligned walk over alpha_k f_k, the two-component shortcut on the first partial
 *     sum included.
 *  9. The tail function's cache of coefficient sums holds UNSCALED sums keyed by container and wavelength; a container
 *     with an aligned component forms its scaled sum anew every step, from the direction the photon has then.
 * The emission rule: emit_table[r] >= 0 names the SINGLE-ROW phase table (PvtPhaseTables) that holds f(mu; S_e) on uniform
 * mu nodes from exactly -1 to exactly 1; the component is tagged PVT_PHASE_TABLE and names that table, and the kernel
 * samples it by the phase tables' rule with n_w as the axis instead of the incoming direction.  A single row draws no u1
 * and the two isotropic draw sites serve as u2 and u3: an aligned emission consumes exactly the draws an isotropic one does.
 * Refused: an aligned component in a node with a concentration field (the march would need the factors: out of scope) or
 * in the root.  The records lie in global memory beside the concentration fields', outside what a launch stages in LDS.
 * Launches of such a scene run the PVT_VARIANT_ROUGH family; the host-buffer entries know no alignment.  The older
 * pvt_scene_create* entries cannot be handed this struct, and that is their refusal: nothing in PvtSceneTables says that a
 * component is aligned, so a scene lowered for this entry and given to an older one is the scene WITHOUT alignment (a
 * component tagged PVT_PHASE_TABLE is then sampled about the incoming ray, as PvtPhaseTables states); a caller that has
 * alignment tables must call this entry.  A NULL struct, n_components 0, or no component with a record is exactly
 * pvt_scene_create_pattern. */
typedef struct PvtAlignTables {
    int32_t n_components;               /* 0 = none (as a NULL struct), else the scene's n_components */
    int32_t n_records;                  /* alignment records */
    const int32_t* comp_align;          /* (n_components) record of each component, -1 = not aligned */
    const double* axis;                 /* (n_records,3) the director in the root's frame, a unit vector within 1e-12 */
    const double* abs_order;            /* (n_records) S_a, finite and in [-0.5, 1] */
    const int32_t* emit_table;          /* (n_records) the single-row phase table of f(mu; S_e), -1 = S_e is 0 */
} PvtAlignTables;

/* ---- Scattering coatings (extension within v13, taken by pvt_scene_create_polyhedra; no struct of their own) ---------
 * A coat_reflect_mode / coat_transmit_mode word of PVT_COAT_LOBE + 4 table + axis sends the reflected / transmitted light
 * into a tabulated lobe: `table` names a table of PvtPhaseTables, `axis` is one of PVT_LOBE_*.  A reflection takes
 * PVT_LOBE_NORMAL or PVT_LOBE_SPECULAR, a transmission PVT_LOBE_NORMAL, PVT_LOBE_REFRACTED or PVT_LOBE_STRAIGHT.  The rule
 * of a scattering coating (the Python ScatterLobe docstring states the same; the kernel and the host delegate both follow
 * it):
 *  1. Coverage, R, A and the one outcome draw u are untouched: rules 1-5 of the absorbing coating and the rules of
 *     where a coating covers.  Beyond the critical angle a transmission lobe about "refracted" behaves as "fresnel": R
 *     stays 1.  Beyond the critical angle a lobe about "normal" or "straight" behaves as "matched": the coating's R
 *     applies.
 *  2. The outgoing normal.  With N the logged geometric normal and d the incoming direction, s = +1 if N . d < 0, else
 *     -1.  N_out = s N for a reflection and -s N for a transmission.
 *  3. The axis a.  "normal": N_out.  "specular": d - 2 (d . N) N, as the specular body forms it.  "refracted": the
 *     Snell direction, as the Fresnel body forms it, at the indices of the photon's wavelength.  "straight": d.
 *  4. The draws come after u: u1 (only when the table has more than one wavelength row), u2 and u3.  Steps 2-4 of the
 *     `PhaseFunctionTable` contract are applied about a at the photon's current wavelength, in the world frame, with
 *     no FMA, and give d'.
 *  5. The fold: if d' . N_out < 0, then d' <- d' - 2 (d' . N_out) N_out.  The fold takes no draw.  Exactly 0 stays.
 *  6. Event kind, recorder selector, the logged normal, the `reflections` counter, `Event.DETECT` and the rule that
 *     roughness applies only where no coating covers stay as for the built-in modes.
 * (The dot product of the fold is (x x' + y y') + z z' and each component of the fold d' - (2 t) N_out, without FMA.)
 * The packer checks, before anything is uploaded: the phase tables are there ("coating lobe without phase tables"), the
 * table lies in them ("coating lobe names a missing phase table"), the axis is one its slot takes ("coating lobe axis not
 * legal for a reflection" / "... for a transmission").  Every entry before pvt_scene_create_polyhedra, pvt_scene_lean_check
 * and the host-buffer entries refuse a mode word above 1 ("coating mode out of range"); every entry refuses a negative one
 * and one in 2 .. PVT_COAT_LOBE - 1 with the same message.  Launches of a scene with a lobe run the PVT_VARIANT_ROUGH
 * family.  A scene whose words are all 0 or 1 packs and traces exactly as before. */
#define PVT_COAT_LOBE 16
enum { PVT_LOBE_NORMAL = 0, PVT_LOBE_SPECULAR = 1, PVT_LOBE_REFRACTED = 2, PVT_LOBE_STRAIGHT = 3 };

/* ---- convex polyhedra (extension within v13, passed to pvt_scene_create_polyhedra) ---------------------------------
 * PVT_GEOM_POLYHEDRON: the intersection of half-spaces; geom_params = (bounding radius, 0, 0, 0), the bounding radius being
 * the largest vertex norm (finite and > 0, else PVT_ERR_INVALID).  Node n's planes are the rows
 * planes[node_plane_start[n] .. + node_plane_count[n]) of (nx, ny, nz, h), 4 <= count <= PVT_MAX_POLYHEDRON_PLANES = 64,
 * every row finite with | |n| - 1 | <= 1e-12.  The rule, in the words of pvtrace_amd.geometry.Polyhedron:
 *
 * The solid is { p : n_k.p < h_k for all k } in the node's own frame.  It need not contain the node's origin.
 * The constructor normalises each row once: it divides the row by |n|.  From then on the stored doubles are the shape,
 * bit for bit, on the host and on the GPU.
 *
 * Crossing distances of a ray (o, d) in the node's frame use IEEE double, no contraction and correctly rounded
 * division.  Planes are taken in index order:
 *
 *     tin = -inf; tout = +inf; miss = false
 *     for k:  den = (nx*d.x + ny*d.y) + nz*d.z
 *             num = h - ((nx*o.x + ny*o.y) + nz*o.z)
 *             if fabs(den) < 1e-300:  if num < 0: miss = true;  continue
 *             t = num / den
 *             if den < 0:  tin = fmax(tin, t)   else  tout = fmin(tout, t)
 *     if !miss and !(tout < tin): candidates tin, then tout; each counts when finite and > EPS
 *
 * This is the box's rule, `!(tmax < tmin)` included.  A plane nearly parallel to the ray is harmless whichever sign its
 * `den` rounds to.  An origin inside that plane gives a large t of the matching sense.  An origin outside gives a miss
 * either way.
 *
 * The solid is convex, so the container rule of the analytic shapes (`nl == 1`) applies unchanged.
 *
 * Normal at a surface point p: the row k* that minimises fabs(((nx*p.x + ny*p.y) + nz*p.z) - h), the first minimum
 * winning.  The normal is (nx, ny, nz) of k*, as stored.
 *
 * Additive under ABI 13.  The plane rows lie behind everything else in the scene's double blob and are read from global
 * memory; a scene with such a node runs the PVT_VARIANT_ROUGH family (with or without meshes), is never lean, and gets
 * no node grid.  The library checks the table, not the solid: that the planes bound a solid with no redundant plane is
 * the caller's business (the Python class refuses anything else).  Which entry takes the type: pvt_scene_create_polyhedra
 * alone; every older pvt_scene_create* entry, pvt_scene_lean_check and the host-buffer pvt_trace_bundle* entries (which
 * have no way to receive the table) refuse it as "unknown geometry type".  Out of scope: non-convex solids, more than 64
 * planes, the node grid and the lean family for such scenes, the host-buffer entries, a face index as a recorder
 * property. */
#define PVT_MAX_POLYHEDRON_PLANES 64
typedef struct PvtPolyhedronTables {
    int32_t n_nodes;                    /* 0 = none (as a NULL struct), else the scene's n_nodes */
    const int32_t* node_plane_start;    /* (n_nodes) first row of the node's planes in `planes` */
    const int32_t* node_plane_count;    /* (n_nodes) rows of the node, 4 .. 64; ignored for nodes of another type */
    int32_t n_planes;                   /* rows in `planes` */
    const double* planes;               /* (n_planes,4) rows (nx, ny, nz, h), unit normals within 1e-12 */
} PvtPolyhedronTables;

/* capture buffers of one launch (DEVICE pointers): `rows` holds sets x capture_rows x PVT_CAPTURE_ROW_WORDS uint64,
 * `cursors` sets x n_recorders int64, sets = the tally sets of the launch (1 without tally_bundle).  Word 11 of a row:
 * emissions | scatterings << 20 | reflections << 40, the photon's event counters (PVT_PROPX_*) */
typedef struct PvtCaptures {
    uint64_t* rows;
    int64_t* cursors;
} PvtCaptures;

/* ---- optional device-side emission (replaces the Python/numpy emitter,
 * reference pvtrace/engine/emit.py:22-134).  Ray i is emitted by light
 * i % n_lights (scene.emit round-robin, scene/scene.py:141-151) from its own
 * RNG stream keyed by (emit_seed, global ray index): ((emit_seed + gi) mod 2^64) xor 0xA5A5A5A55A5A5A5A.
 * Draw order: the wavelength (a spectrum light only: PVT_WL_SPECTRUM interpolates (cdf, x) at u, the knot at or
 * below u found with <=, x[0] for u <= cdf[0], the last x for u >= the last cdf; PVT_WL_SPECTRUM_HIST below), then the
 * position (-p + 2 p u per axis; the disc: angle RN(2 pi) u first, then radius sqrt(u) r), then the direction (the
 * built-in phase functions above; PVT_DIR_LAMBERTIAN: sin = sqrt(u0), azimuth 2 pi u1).  Local -> world:
 * ((m0 x + m1 y) + m2 z) + m3 per row, no fused multiply-add.  tests/exact_emission.py holds the referee, the host
 * sampler and the three compiled copies of the kernel's emitter to this rule ray by ray. */
enum { PVT_WL_CONSTANT = 0, PVT_WL_SPECTRUM = 1,
       PVT_WL_SPECTRUM_HIST = 2 /* histogram-sampled Distribution (material/distribution.py:171-176): x[#{cdf_i < u}], no interpolation */ };
enum { PVT_POS_POINT = 0, PVT_POS_RECT = 1, PVT_POS_CIRCLE = 2, PVT_POS_CUBE = 3,
       PVT_POS_GRID = 4 /* EXTENSION within v13: a weight lattice (PvtSourceTables), pvt_scene_set_sources only */ };
enum { PVT_DIR_Z = 0, PVT_DIR_CONE = 1, PVT_DIR_ISOTROPIC = 2, PVT_DIR_LAMBERTIAN = 3, PVT_DIR_HG = 4,
       PVT_DIR_TABLE = 5 /* EXTENSION within v13: a tabulated direction (PvtSourceTables), pvt_scene_set_sources only */ };
typedef struct PvtEmitterTables {
    int32_t n_lights, n_spec;
    const int32_t* wl_type;
    const double* wl_value;         /* constant wavelength (nm) */
    const int32_t* wl_spec_start;   /* into spec_x / spec_cdf */
    const int32_t* wl_spec_n;
    const int32_t* pos_type;
    const double* pos_param;        /* (n_lights,3) half-extents / radius */
    const int32_t* dir_type;
    const double* dir_param;        /* theta_max or g */
    const double* light_to_world;   /* (n_lights,4,4) */
    const double* spec_x;           /* pooled inverse-CDF tables */
    const double* spec_cdf;
} PvtEmitterTables;

/* ---- tabulated sources (extension within v13, passed to pvt_scene_set_sources beside the emitter) -----------------
 * A light whose pos_type is PVT_POS_GRID names a position grid, light_grid[i] >= 0; a light whose dir_type is
 * PVT_DIR_TABLE names a direction table, light_table[i] >= 0; every other light has -1 there.  The emitter's pos_param
 * and dir_param of such a light are not read: the packer writes where the light's records lie into them.
 *
 * The position grid (the Python PositionGrid states the same): a non-negative weight per cell of a lattice in the
 * light's own frame, shape (nx, ny, nz), each >= 1, at most 2^22 cells.  An axis with grid_bounded = 0 has one cell,
 * the coordinate on it is exactly 0.0 and no draw is taken for it.
 *  1. The CDF has C_0 = 0.  C_{k+1} is the running sum of the weights in slot order (ix ny + iy) nz + iz, divided by
 *     the total.  The last entry is set to exactly 1.  (grid_cdf holds the cells + 1 entries of each grid.)
 *  2. Draw u_c.  The cell is the slot k with C_k <= u_c < C_{k+1}.  It is found by the bisection the phase tables use
 *     (cdf[m] <= u ? a = m : b = m), so a cell of zero weight is never chosen.
 *  3. For each bounded axis, in the order x, y, z, draw u_a.  h_a = (upper_a - lower_a) / n_a is one division (grid_h
 *     holds it).  The coordinate is lower_a + ((double)i_a + u_a) * h_a: an add, a multiply and an add, with no fused
 *     multiply-add.
 *  4. In the light's draw order, these draws stand where the built-in masks' position draws stand.  That is after the
 *     wavelength draw of a spectrum light and before the direction draws.
 *
 * The direction table: a table in the layout of PvtPhaseTables, sampled by steps 3 and 4 of its contract about the
 * light's +z.  The first row is used; u1 is drawn whenever the table has several rows; u2 gives the polar cosine, u3
 * the azimuth.  These draws stand where the built-in directions' draws stand.  Equal tables may be stored once.
 * A separate struct so that PvtEmitterTables keeps the length old callers pass. */
typedef struct PvtSourceTables {
    int32_t n_lights;               /* the emitter's n_lights */
    int32_t n_grids, n_tables;      /* position grids, direction tables */
    int32_t n_grid_cdf;             /* length of the grid CDF pool */
    int32_t n_table_wavelength, n_table_mu, n_table_cdf;   /* lengths of the tables' wavelength, mu and CDF pools */
    const int32_t* light_grid;      /* (n_lights) grid of each light, -1 = none */
    const int32_t* light_table;     /* (n_lights) direction table of each light, -1 = none */
    const int32_t* grid_shape;      /* (n_grids,3) cells per axis */
    const int32_t* grid_bounded;    /* (n_grids,3) 1 = bounded, 0 = a one-cell axis without bounds */
    const double* grid_lower;       /* (n_grids,3) lower bound, 0 on an axis without bounds */
    const double* grid_h;           /* (n_grids,3) cell width (upper - lower) / n, 1 on an axis without bounds */
    const int32_t* grid_cdf_start;  /* (n_grids) first CDF entry of each grid in `grid_cdf` (cells + 1 entries) */
    const double* grid_cdf;         /* pooled CDFs */
    const int32_t* table_nw;        /* (n_tables) rows (wavelengths) of each table, >= 1 */
    const int32_t* table_nmu;       /* (n_tables) mu points of each table, >= 2 */
    const int32_t* table_wl_start;  /* (n_tables) first wavelength of each table in `table_wavelength` */
    const int32_t* table_mu_start;  /* (n_tables) first point of each table in `table_mu` */
    const int32_t* table_cdf_start; /* (n_tables) first CDF entry of each table in `table_cdf` (nw x nmu, row-major) */
    const double* table_wavelength; /* pooled row wavelengths, nm, finite and strictly increasing per table */
    const double* table_mu;         /* pooled mu axes, each from exactly -1 to exactly 1 */
    const double* table_cdf;        /* pooled CDF rows, each from exactly 0 to exactly 1 */
} PvtSourceTables;

typedef struct PvtTraceParams {
    int64_t n_rays;         /* rays in this bundle                                   */
    uint64_t seed;          /* ray i traces with RNG stream seed + ray_offset + i    */
    uint64_t ray_offset;    /* global index of ray 0 (bundle streaming / GPU shard)  */
    uint64_t emit_seed;     /* device emission only                                  */
    int64_t record_every;   /* every k-th ray keeps a full history; 0 = none         */
    int32_t maxsteps;
    int32_t max_events;
    int32_t emit_method;    /* PVT_EMIT_*                                            */
    int32_t workgroups_per_cu; /* persistent workgroups launched per CU; 0 = default (4: one launch
                                * fills the chip).  Launches that overlap on several streams run best
                                * with fewer (2 with three in flight): each then holds fewer CU slots
                                * while it drains, and a workgroup amortises its drain over more photons */
    /* A stream of equal bundles in ONE launch (the reference's simulate_stream, api.py:249-264, hands
     * its kernel one bundle per call; a 50 000-photon bundle is far too little to occupy an MI355X).
     * With tally_bundle = m > 0 (tally mode only: record_every == 0) the n_rays rays are the
     * concatenation of bundles of m rays (the last may be shorter): ray i still uses the stream
     * seed + ray_offset + i — exactly the seeds of the streamed bundles — but the rays of bundle
     * j = i / m are tallied into set j of the tally arrays, set j starting tally_stride_i64 int64
     * elements (rec_distinct, rec_crossings, rec_bins alike) and tally_stride_f64 doubles (rec_sums)
     * after set j-1.  0 = the launch is one bundle. */
    int64_t tally_bundle;
    int64_t tally_stride_i64;
    int64_t tally_stride_f64;
    int64_t flags;          /* PVT_FLAG_* */
} PvtTraceParams;

/* PvtTraceParams.flags */
enum {
    /* pvt_trace_device: do NOT write the fill values into the rows of the event log that no event reached (for the
     * reference's defaults, 128 rows per ray of which a ray writes a dozen, that is most of the log).  Rows beyond
     * counts[j] of recorded ray j are then undefined; only counts[] is cleared.  For callers that read the
     * written rows only. */
    PVT_FLAG_NO_LOG_PREFILL = 1,
    /* A STREAM of tally bundles whose totals are wanted, not each bundle's own (record_every == 0, no tally sets):
     * the launch does not trace its last photons to completion.  A wave that finds no new ray parks its live
     * photons -- complete state: position, direction, wavelength, path, clock, RNG stream, step count, source,
     * first-crossing mask -- in a buffer of the scene that belongs to the HIP stream, and retires; the NEXT
     * launch on that stream (same scene, same maxsteps / emit_method; it adds to the tallies IT is given) hands
     * them to its lanes before its own rays.  Histories are unchanged bit for bit (a photon's draws depend on its
     * stream alone), integer tallies summed over the launches are identical; what disappears is the tail of
     * every launch, where a few long histories keep a few lanes busy (a fifth of all wave-iterations of a 10^6-
     * photon launch of the headline scene).  A launch WITHOUT the flag finishes everything, what it resumed
     * included; with n_rays == 0 it is the closing flush of a job.  pvt_scene_carry_pending() tells whether
     * photons are waiting.  The resuming launch must ask for the maxsteps / emit_method of the launch that parked
     * them (PVT_ERR_INVALID otherwise: the photons would silently change rules) and is never narrower than it (the
     * library widens its grid if need be); pvt_scene_carry_discard() drops parked photons of a job that was
     * abandoned.  The host-buffer entries (pvt_trace_bundle, pvt_trace_bundle_multi) ignore the flag: their scene
     * lives for one call.  (The reference has no counterpart: its bundles end when their slowest ray ends.) */
    PVT_FLAG_CARRY_OUT = 2
};

/* initial rays, world frame (exactly trace_bundle's three array arguments) */
typedef struct PvtRays {
    const double* position;   /* (n,3) */
    const double* direction;  /* (n,3) */
    const double* wavelength; /* (n)   */
} PvtRays;

/* recorder accumulators; the trace ADDS into them (caller zeroes) */
typedef struct PvtTallies {
    int64_t* rec_distinct;   /* (n_recorders)       */
    int64_t* rec_crossings;  /* (n_recorders)       */
    double* rec_sums;        /* (n_recorders,4,2)   */
    int64_t* rec_bins;       /* (total_bins), then the volume maps' slots (pvt_scene_map_slots) */
} PvtTallies;

/* event log: rows = ceil(n/record_every)*max_events; row of event k of
 * recorded ray j is j*max_events+k (same packing as _kernel.pyx:1035-1047).
 * pvt_trace_* pre-fills kind/position/... with 0 and the id columns with -1.
 * (The kernel itself writes PvtEventRecords, below; these columns are made from them by a
 * second, coalesced pass.) */
typedef struct PvtEventLog {
    int32_t* counts;         /* (n_recorded) */
    uint8_t* kind;
    int32_t* hit;
    int32_t* container;
    int32_t* adjacent;
    int32_t* component;
    int32_t* source;
    double* position;        /* (rows,3) */
    double* direction;       /* (rows,3) */
    double* normal;          /* (rows,3) */
    double* wavelength;
    double* travelled;
    double* duration;
} PvtEventLog;

/* event RECORDS: the form the kernel writes.  One event = one 128-byte row (16 x uint64, little endian):
 *   word 0  hit (int32, low half) | container (high half)     word 1  adjacent | component
 *   word 2  source | kind (low byte of the high half)         words 3-5 position, 6-8 direction,
 *   9-11 normal (zeros when the event has none), 12 wavelength, 13 travelled, 14 duration (doubles)
 *   word 15 the row index itself
 * Row of event k of recorded ray j = j*max_events + k, the reference's packing (_kernel.pyx:1035-1047) with
 * the thirteen columns of a row side by side: a lane that follows one ray then writes ONE full cache line
 * per event instead of thirteen scattered column elements (4.2 x less HBM write traffic, measured).  Rows
 * k >= counts[j] are never written and hold whatever the buffer held.  pvt_unpack_records_device turns
 * records into the column arrays of PvtEventLog. */
typedef struct PvtEventRecords {
    int32_t* counts;         /* (n_recorded) events written per recorded ray */
    uint64_t* rows;          /* (n_recorded * max_events, 16) */
} PvtEventRecords;

typedef struct PvtScene PvtScene;   /* opaque: tables resident in HBM on one GPU */

int pvt_abi_version(void);
const char* pvt_last_error(void);
int pvt_device_count(void);

/* Pack the tables and upload them once to `device`. */
int pvt_scene_create(const PvtSceneTables* tables, int device, PvtScene** out);
/* The same with refractive-index tables (NULL = none: then exactly pvt_scene_create). */
int pvt_scene_create_ex(const PvtSceneTables* tables, const PvtIndexTables* index_tables, int device, PvtScene** out);
/* The same with phase-function tables (NULL = none: then exactly pvt_scene_create_ex).  pvt_scene_create and
 * pvt_scene_create_ex refuse a component tagged PVT_PHASE_TABLE (PVT_ERR_INVALID). */
int pvt_scene_create_phase(const PvtSceneTables* tables, const PvtIndexTables* index_tables,
                           const PvtPhaseTables* phase_tables, int device, PvtScene** out);
/* The same with rough interfaces (NULL, n_nodes 0 or every alpha 0 = none: then exactly pvt_scene_create_phase). */
int pvt_scene_create_rough(const PvtSceneTables* tables, const PvtIndexTables* index_tables,
                           const PvtPhaseTables* phase_tables, const PvtSurfaceTables* surface_tables, int device,
                           PvtScene** out);
/* The same with concentration fields (NULL, n_nodes 0 or no node with a lattice = none: then exactly
 * pvt_scene_create_rough). */
int pvt_scene_create_field(const PvtSceneTables* tables, const PvtIndexTables* index_tables,
                           const PvtPhaseTables* phase_tables, const PvtSurfaceTables* surface_tables,
                           const PvtFieldTables* field_tables, int device, PvtScene** out);
/* The same with volume maps (NULL, n_nodes 0 or n_maps 0 = none: then exactly pvt_scene_create_field). */
int pvt_scene_create_maps(const PvtSceneTables* tables, const PvtIndexTables* index_tables,
                          const PvtPhaseTables* phase_tables, const PvtSurfaceTables* surface_tables,
                          const PvtFieldTables* field_tables, const PvtMapTables* map_tables, int device, PvtScene** out);
/* Slots of the scene's volume maps (PvtMapTables.map_slots; 0 without maps): PvtTallies.rec_bins of a launch on the
 * scene holds total_bins + this many elements (per tally set: tally_stride_i64 is at least that). */
int64_t pvt_scene_map_slots(const PvtScene* scene);
/* The same with captured recorders (NULL, n_recorders 0 or capture_rows 0 = none: then exactly pvt_scene_create_maps). */
int pvt_scene_create_capture(const PvtSceneTables* tables, const PvtIndexTables* index_tables,
                             const PvtPhaseTables* phase_tables, const PvtSurfaceTables* surface_tables,
                             const PvtFieldTables* field_tables, const PvtMapTables* map_tables,
                             const PvtCaptureTables* capture_tables, int device, PvtScene** out);
/* Rows of the scene's captures per tally set (PvtCaptureTables.capture_rows; 0 without captures). */
int64_t pvt_scene_capture_rows(const PvtScene* scene);
/* The same with absorbing coatings (NULL, n_coatings 0 or every A zero with no table = none: then exactly
 * pvt_scene_create_capture).  This is the one entry that knows the recorder selector PVT_RECX_DETECTED: the entries
 * before it refuse a recorder with it ("recorder selector out of range"), as they refused a selector 7 before it existed;
 * here such a recorder is accepted also where no coating absorbs, and then counts nothing.  By the same rule it is the
 * one entry that knows the histogram properties PVT_PROPX_* (the photon event counters): the entries before it refuse
 * them ("histogram property out of range"). */
int pvt_scene_create_absorb(const PvtSceneTables* tables, const PvtIndexTables* index_tables,
                            const PvtPhaseTables* phase_tables, const PvtSurfaceTables* surface_tables,
                            const PvtFieldTables* field_tables, const PvtMapTables* map_tables,
                            const PvtCaptureTables* capture_tables, const PvtCoatingAbsorbTables* absorb_tables, int device,
                            PvtScene** out);
/* The same, and the one entry that knows the histogram properties PVT_PROPX_ORIGIN_* (the launch origin): same arguments,
 * same scene for tables without them; pvt_scene_create_absorb and every entry before it refuse those ids ("histogram
 * property out of range"), as pvt_scene_create_absorb refused an id 10 before they existed. */
int pvt_scene_create_origin(const PvtSceneTables* tables, const PvtIndexTables* index_tables,
                            const PvtPhaseTables* phase_tables, const PvtSurfaceTables* surface_tables,
                            const PvtFieldTables* field_tables, const PvtMapTables* map_tables,
                            const PvtCaptureTables* capture_tables, const PvtCoatingAbsorbTables* absorb_tables, int device,
                            PvtScene** out);
/* The same with patterned coatings (PvtCoatingPatternTables; NULL, n_coatings 0 or no row with a pattern or an any-facet
 * flag = none: then exactly pvt_scene_create_origin).  Every entry before it knows no patterns. */
int pvt_scene_create_pattern(const PvtSceneTables* tables, const PvtIndexTables* index_tables,
                             const PvtPhaseTables* phase_tables, const PvtSurfaceTables* surface_tables,
                             const PvtFieldTables* field_tables, const PvtMapTables* map_tables,
                             const PvtCaptureTables* capture_tables, const PvtCoatingAbsorbTables* absorb_tables,
                             const PvtCoatingPatternTables* pattern_tables, int device, PvtScene** out);
/* The same with aligned components (PvtAlignTables; NULL, n_components 0 or no component with a record = none: then
 * exactly pvt_scene_create_pattern).  Every entry before it knows no alignment. */
int pvt_scene_create_aligned(const PvtSceneTables* tables, const PvtIndexTables* index_tables,
                             const PvtPhaseTables* phase_tables, const PvtSurfaceTables* surface_tables,
                             const PvtFieldTables* field_tables, const PvtMapTables* map_tables,
                             const PvtCaptureTables* capture_tables, const PvtCoatingAbsorbTables* absorb_tables,
                             const PvtCoatingPatternTables* pattern_tables, const PvtAlignTables* align_tables, int device,
                             PvtScene** out);
/* The same with convex polyhedra (PvtPolyhedronTables), and the one entry that knows geometry type PVT_GEOM_POLYHEDRON:
 * NULL, n_nodes 0 or a scene with no such node = exactly pvt_scene_create_aligned.  Every entry before it refuses the type
 * ("unknown geometry type"), as they did before it existed.  It is also the one entry that knows PVT_GEOM_CONICOID, which
 * needs no table: the same refusals hold for that type.  And the one entry that takes scattering coatings (a coating mode
 * word >= PVT_COAT_LOBE): every other entry refuses them ("coating mode out of range"). */
int pvt_scene_create_polyhedra(const PvtSceneTables* tables, const PvtIndexTables* index_tables,
                               const PvtPhaseTables* phase_tables, const PvtSurfaceTables* surface_tables,
                               const PvtFieldTables* field_tables, const PvtMapTables* map_tables,
                               const PvtCaptureTables* capture_tables, const PvtCoatingAbsorbTables* absorb_tables,
                               const PvtCoatingPatternTables* pattern_tables, const PvtAlignTables* align_tables,
                               const PvtPolyhedronTables* polyhedron_tables, int device, PvtScene** out);
/* Attach / replace the device-side emitter of a scene (optional).  It takes no source tables: a type word outside the
 * built-ins, PVT_POS_GRID and PVT_DIR_TABLE among them, is refused with PVT_ERR_INVALID ("emitter type out of range"),
 * and so the host-buffer entries refuse it (pvt_trace_bundle, pvt_trace_bundle_multi). */
int pvt_scene_set_emitter(PvtScene* scene, const PvtEmitterTables* emitter);
/* The same with tabulated sources (PvtSourceTables), and the one entry that knows PVT_POS_GRID and PVT_DIR_TABLE:
 * `sources` NULL = exactly pvt_scene_set_emitter.  The tables are validated first (pvt_sources_check). */
int pvt_scene_set_sources(PvtScene* scene, const PvtEmitterTables* emitter, const PvtSourceTables* sources);
/* The validation pvt_scene_set_sources runs, without a scene or a GPU: PVT_OK, or PVT_ERR_INVALID with the refusal in
 * pvt_last_error(). */
int pvt_sources_check(const PvtEmitterTables* emitter, const PvtSourceTables* sources);
void pvt_scene_destroy(PvtScene* scene);

/* Device-resident entry: every pointer in rays / tallies / log is a DEVICE
 * pointer owned by the caller (e.g. torch tensors) on the scene's GPU;
 * `stream` is a hipStream_t (NULL = default stream).  rays == NULL selects
 * device-side emission.  log may be NULL when record_every == 0.
 * Asynchronous: returns after enqueueing. */
int pvt_trace_device(PvtScene* scene, const PvtRays* rays, const PvtTraceParams* params,
                     const PvtTallies* tallies, const PvtEventLog* log, void* stream);
/* (With column arrays the kernel's 128-byte event records are staged in a buffer of the scene, one per stream that
 * asked for it, at most 1 GiB -- larger logs are traced over consecutive ray ranges, same results -- kept until
 * the scene is destroyed: device memory on top of the caller's 117 bytes per row.  pvt_trace_device_records has no
 * such buffer.) */

/* Same launch, the event log kept as RECORDS in caller-owned DEVICE memory (no staging, no unpack pass):
 * what a caller wants who reads only the rows that were written (the Python engine.simulate() does).
 * `records` may be NULL when record_every == 0. */
int pvt_trace_device_records(PvtScene* scene, const PvtRays* rays, const PvtTraceParams* params,
                             const PvtTallies* tallies, const PvtEventRecords* records, void* stream);

/* pvt_trace_device_records with the capture buffers of a scene made by pvt_scene_create_capture (`captures` NULL, or a
 * scene without captures: exactly pvt_trace_device_records -- the launch keeps no rows).  The other trace entries keep
 * no rows either; the host-buffer entries know no captures. */
int pvt_trace_device_capture(PvtScene* scene, const PvtRays* rays, const PvtTraceParams* params,
                             const PvtTallies* tallies, const PvtEventRecords* records, const PvtCaptures* captures,
                             void* stream);

/* 1 when photons parked by the last launch on `stream` (PVT_FLAG_CARRY_OUT) wait to be resumed, else 0. */
int pvt_scene_carry_pending(PvtScene* scene, void* stream);
/* Forget the photons parked on `stream` (a job abandoned half-way: an exception between two bundles, a consumer that
 * went away).  The next launch on the stream then starts from its own rays alone. */
int pvt_scene_carry_discard(PvtScene* scene, void* stream);
/* A scene that is put aside for later (a cache of resident scenes): frees the staging buffers of pvt_trace_device (up to
 * 1 GiB per stream that asked for column arrays) and forgets parked photons on every stream.  The tables stay. */
int pvt_scene_trim(PvtScene* scene);

/* Records -> column arrays (all DEVICE pointers), one coalesced pass; `prefill` != 0 also writes the
 * reference's fill values (0 / -1) into the rows no event reached, else those rows are left alone.
 * `out->counts` is not written (the counts are `records->counts`). */
int pvt_unpack_records_device(const PvtEventRecords* records, int64_t n_recorded, int32_t max_events,
                              const PvtEventLog* out, int prefill, void* stream);

/* Host-buffer entry — the literal replacement for _kernel.trace_bundle: all
 * pointers are HOST memory; uploads, traces, downloads, synchronises.
 * `kernel_ms` (nullable) receives the HIP-event time of the trace kernel. */
int pvt_trace_bundle(const PvtSceneTables* tables, const PvtEmitterTables* emitter,
                     const PvtRays* rays, const PvtTraceParams* params,
                     const PvtTallies* tallies, const PvtEventLog* log, int device,
                     double* kernel_ms);

/* (The rays are uploaded in chunks and a chunk is traced while the next one crosses PCIe; results do not depend on the
 * split.  The device block that held the rays and tallies -- up to 1 GiB, one per device -- is kept for the next
 * host-buffer call on that device; pvt_release_cached_memory() frees what is kept.  The reference's trace_bundle keeps
 * nothing between calls either way: _kernel.pyx:1035-1066 allocates per call.) */
void pvt_release_cached_memory(void);

/* In-process multi-GPU form of pvt_trace_bundle: the bundle is split over
 * `devices[0 .. n_devices)` by contiguous index range — shard g traces the global indices
 * pvt_shard_range(n_rays, g, n_devices, record_every) with ray_offset advanced accordingly, so every ray
 * keeps the RNG stream seed + ray_offset + global index and the result does not depend on the device
 * list.  One host thread, one resident scene and one stream per entry of `devices` (an id may appear
 * several times: its shards then share that GPU).  The tallies are summed on the devices (RCCL over
 * xGMI) when the entries are different GPUs, else on the host: integer tallies exactly, the f64 moment sums up to
 * the order of addition; each shard writes the rows of its own rays into the caller's event log (inner shard
 * boundaries are multiples of record_every, so the shards' logs together ARE the single-device log).
 * `kernel_ms` (nullable) receives the longest shard's kernel time.  The reference splits a bundle over
 * OpenMP threads instead (_kernel.pyx:1074-1095); there as here the output is independent of the split. */
int pvt_trace_bundle_multi(const PvtSceneTables* tables, const PvtEmitterTables* emitter,
                           const PvtRays* rays, const PvtTraceParams* params,
                           const PvtTallies* tallies, const PvtEventLog* log,
                           const int* devices, int n_devices, double* kernel_ms);

/* How the last pvt_trace_bundle_multi of THIS thread summed the shards' tallies: 0 none yet, 1 on the host,
 * 2 on the devices with RCCL (ncclCommInitAll over the device list, ncclReduce to the first shard; taken when every
 * entry of the list is a different GPU and librccl can be loaded; PVT_MULTI_REDUCE=host|rccl overrides). */
int pvt_last_multi_reduce(void);

/* [start, stop) of shard `shard` of `n_shards` over n_rays rays; inner boundaries are rounded down to
 * multiples of `align` (pass record_every; <= 1 means no alignment).  Pure host arithmetic. */
int pvt_shard_range(int64_t n_rays, int shard, int n_shards, int64_t align, int64_t* start, int64_t* stop);

/* Device emission only (fills caller-owned DEVICE arrays); used by tests. */
int pvt_emit_device(PvtScene* scene, const PvtTraceParams* params, double* position,
                    double* direction, double* wavelength, void* stream);

/* Self-test: y[i] = f(x[i]) evaluated ON THE DEVICE (host buffers in/out).
 * fn: 0 log, 1 sin, 2 cos, 3 asin, 4 acos, 5 sqrt, 6 1/x, 7 sin*cos via sincos,
 * 8 second xoshiro256+ uniform of stream (uint64)x, 9 x/(x+3), 10-13 known-divisor divisions,
 * 14/15 sin/cos(2 pi x) and 16 sqrt((1-x)(1+x)) (composed functions of pvt_math.h), 17-19 the short
 * 1/x, x/y and sqrt(x) sequences of the kernel (operands in their normal ranges).  Lets the tests prove the bit-reproducibility premise of
 * csrc/pvt_math.h on gfx950. */
int pvt_selftest_math(int fn, const double* x_host, double* y_host, int64_t n, int device);

/* Step counters of the scene since its creation (or the last reset), summed over every launch on every stream --
 * always on, two scalar adds per wave and trip of the photon loop:
 *   out[0] wave-iterations (trips in which a wave stepped its lanes)      out[1] lane-steps (live lanes summed over them)
 *   out[2] photons finished one step early by the fused exit             out[3] waves retired
 * out[1] + out[2] is the reference's loop count (`count`, _kernel.pyx:655) summed over the photons traced so far --
 * exactly, when no photon is parked between launches (PVT_FLAG_CARRY_OUT) at the time of the call; out[1] / (64 out[0])
 * is the fraction of lanes that held a live photon when a wave stepped.  The caller synchronises the streams it
 * launched on first (the copy only orders after the null stream); `reset` != 0 clears the counters afterwards. */
int pvt_scene_counters(PvtScene* scene, uint64_t* out, int reset);

/* The clocks the scene's launches ran at, read ON THE GPU (v12; no reference counterpart -- `elapsed` there is
 * time.perf_counter around the call, pvtrace/engine/api.py:232-245).  Every workgroup reads the constant 100 MHz clock and
 * the shader clock when it starts and when its last wave leaves:
 *   out[0] shader-clock cycles and out[1] 100 MHz ticks, both summed over the lives of all workgroups since the scene's
 *   creation or the last reset of pvt_scene_counters (which clears these too): 100 MHz x out[0] / out[1] is the shader
 *   clock the launches ran at, overlapping launches included.  Synchronise first, as for pvt_scene_counters. */
int pvt_scene_clock(PvtScene* scene, uint64_t* out);

/* GPU-side span of the LAST launch on `stream` (v12): out[0] = 100 MHz time at which its workgroup 0 started, out[1] = the
 * latest time at which one of its workgroups left; (out[1] - out[0]) x 10 ns is the launch's duration as the GPU saw it.
 * A pair of HIP events around the call also counts whatever the host does between recording them (a descheduled thread
 * reads as kernel time: profiles/r06_e2e_outlier.txt).  Synchronises the stream. */
int pvt_scene_launch_span(PvtScene* scene, void* stream, uint64_t* out);

/* Launch geometry actually used by the last trace on this scene (diagnostics). */
int pvt_scene_launch_info(PvtScene* scene, int32_t* grid, int32_t* block, int32_t* lds_bytes);

/* The kernel family the scene's launches run (diagnostics; additive under ABI 13).  PVT_VARIANT_LEAN: the scene was
 * proven plain when it was created -- unrotated boxes only (the root may be a sphere), per container at most two components,
 * each an absorber or an isotropic luminophore, spectra on even grids (not histograms), no coating, no index / reflectivity / phase
 * table, no rough node, field or map, at most 64 recorders none of which filters by source, no mesh, no node grid --
 * and its tables fit in LDS: its launches run a variant of the trace kernel compiled for exactly that (same arithmetic,
 * same draws, bit-identical histories).  Everything else runs the generic families: W4 (analytic shapes, node loop),
 * GRID (many nodes), ROUGH (rough nodes, fields, maps, captures, absorbing and patterned coatings, truncated cones, aligned components, convex polyhedra, conicoids), MESH.  The environment variable PVT_NO_LEAN, read when the scene
 * is created, sends a plain scene to the generic family too (parity tests, A/B runs). */
enum { PVT_VARIANT_LEAN = 0, PVT_VARIANT_W4 = 1, PVT_VARIANT_GRID = 2, PVT_VARIANT_ROUGH = 3, PVT_VARIANT_MESH = 4 };
/* ... of the last trace on this scene; before the first one, of a tally launch.  Returns PVT_VARIANT_*, < 0 on error. */
int pvt_scene_variant(PvtScene* scene);
/* Which entry point of that family the last trace on this scene ran (diagnostics; additive under ABI 13).
 * PVT_ENTRY_PARK: a tally launch of the lean family that parks its survivors for its successor on the stream
 * (PVT_FLAG_CARRY_OUT, and not too wide to park) runs `trace_kernel_lean_park`, the family's kernel compiled without the
 * drain rendezvous and the tail function, which such a launch cannot reach.  Every other launch: PVT_ENTRY_USUAL. */
enum { PVT_ENTRY_USUAL = 0, PVT_ENTRY_PARK = 1 };
int pvt_scene_entry(PvtScene* scene);
/* Whether the last trace on this scene ran a solo entry (diagnostics; additive under ABI 13): 1 or 0, < 0 on error.
 * A lean scene that is ONE unrotated box inside a root that is a box or a sphere strictly holding it, with no component in
 * the root and no recorder on it, is "solo".  Its tally launches -- not its history launches (record_every > 0), and no
 * launch of a scene where somebody observes exits -- run `trace_kernel_solo_park` / `trace_kernel_solo_fin`: the lean
 * kernels with the node stage of a step in closed form (same arithmetic, same draws, bit-identical histories).
 * pvt_scene_variant and pvt_scene_entry report such a launch as PVT_VARIANT_LEAN and PVT_ENTRY_PARK / PVT_ENTRY_USUAL as
 * before.  The environment variable PVT_NO_SOLO, read when the scene is created, switches the solo entries off. */
int pvt_scene_solo(PvtScene* scene);
/* Host-only (no GPU needed): *solo = 1 when the tables are proven solo in the sense above (PVT_NO_SOLO unset), else 0;
 * the call still returns PVT_OK then, and pvt_last_error() reads "not solo: " followed by the first clause the tables do
 * not meet. */
int pvt_scene_solo_check(const PvtSceneTables* tables, const PvtIndexTables* index_tables, const PvtPhaseTables* phase_tables,
                         const PvtSurfaceTables* surface_tables, const PvtFieldTables* field_tables,
                         const PvtMapTables* map_tables, int32_t* solo);
/* Host-only (no GPU needed): *lean = 0 when the tables are not proven plain in the sense above, 2 when they are and every
 * spectrum is a constant or an even grid bit for bit (the family's kernels without table searches), 1 when some grid is
 * even only up to rounding (np.linspace: the family's kernels that search) -- the proof alone, on the packed tables;
 * whether a launch then runs PVT_VARIANT_LEAN also needs the tables to fit in LDS.  When *lean is 0 the call still
 * returns PVT_OK, and pvt_last_error() reads "not lean: " followed by the first fact the proof asks for that the tables
 * do not meet -- among them "an index pair without a proven critical-angle threshold": the lean kernels decide total
 * reflection by a proven cosine threshold alone. */
int pvt_scene_lean_check(const PvtSceneTables* tables, const PvtIndexTables* index_tables, const PvtPhaseTables* phase_tables,
                         const PvtSurfaceTables* surface_tables, const PvtFieldTables* field_tables,
                         const PvtMapTables* map_tables, int32_t* lean);

/* Host-only check of the triangle BVH the library builds for mesh node `node` (no GPU needed):
 * every face appears in exactly one leaf, lies inside the boxes of its leaf and of all its
 * ancestors, the children of a record are a pair on one 64-byte line, a left child's skip link is its
 * sibling and a right child's its parent's; and the copy of the tree's top
 * levels that the trace kernel reads from LDS (cursors and links that name either array), made at five
 * sizes, walks the same records in the same order with the same successors after a hit and after a miss.
 * Returns PVT_OK and the node / leaf counts and the tree depth, or PVT_ERR_INVALID with pvt_last_error(). */
int pvt_mesh_bvh_check(const PvtSceneTables* tables, int32_t node, int32_t* n_bvh_nodes,
                       int32_t* n_leaves, int32_t* depth);

/* Host-only view of the NODE GRID the library builds for scenes of many nodes (no GPU needed).  The reference
 * intersects every node in every step (_kernel.pyx:666-680); for such scenes the trace kernel instead files every
 * node but the root under the cells of a uniform grid touched by its bounding box grown by a margin, and each
 * photon tests only the nodes filed under the cells its ray passes (results unchanged bit for bit).
 * dims[3] = cells per axis, all 0 when the scene gets no grid (few nodes, meshes, non-rigid poses; the plain node loop
 * then serves it); lo[3] / cell[3] = the grid's corner and cell edges, `guard` = the margin, `odd` = a cylinder is
 * filed (the walk's early exit is then more cautious).  `masks` (nullable) receives, per cell (x fastest), two 64-bit
 * words whose bit n says node n is filed there, up to `masks_cap` words. */
int pvt_node_grid_plan(const PvtSceneTables* tables, int32_t* dims, double* lo, double* cell, double* guard,
                       int32_t* odd, uint64_t* masks, int64_t masks_cap);

#ifdef __cplusplus
}
#endif
#endif /* PVTRACE_HIP_H */
