"""ctypes binding to libpvtrace_hip.so (the C ABI in include/pvtrace_hip.h).

This is the only place the Python host touches the native engine.  There is NO
CPU fallback: if the shared library is missing, or no GPU is visible, tracing
raises `EngineUnavailableError` — it never silently routes somewhere else.

`torch` is used purely as plumbing: device buffers are torch tensors (so they
can be all-reduced with torch.distributed over RCCL) and the kernel is enqueued
on torch's current HIP stream.  Pointers and sizes are all the library sees.
"""
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get(  # PVT_LIB: developer override (ablation builds); never a CPU path
    "PVT_LIB", os.path.join(os.path.dirname(_HERE), "csrc", "libpvtrace_hip.so"))

_p_i32 = C.POINTER(C.c_int32)
_p_f64 = C.POINTER(C.c_double)
_p_i64 = C.POINTER(C.c_int64)
_p_u8 = C.POINTER(C.c_uint8)


class EngineUnavailableError(RuntimeError):
    """The HIP engine cannot run here (library not built, or no MI355X visible)."""


# How a table struct is filled from a CompiledScene (`marshal`, below) is written once, next to its fields:
#   POINTERS  pointer field -> (the CompiledScene attribute it is read from, its numpy dtype);
#   COUNTS    count field -> how it is derived from the CompiledScene;
#   ABSENT    "the scene has none of this": the marshaller then answers None, which the library takes for "no such tables".
def _same_names(fields):
    """POINTERS of a struct whose pointer fields are named like the attributes they are read from."""
    return {name: (name, np.int32 if ctype is _p_i32 else np.float64) for name, ctype in fields if ctype in (_p_i32, _p_f64)}


class PvtSceneTables(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int32), ("root_id", C.c_int32), ("n_components", C.c_int32),
        ("n_abs", C.c_int32), ("n_ems", C.c_int32), ("n_recorders", C.c_int32),
        ("n_hists", C.c_int32), ("total_bins", C.c_int32), ("n_coatings", C.c_int32),
        ("n_coat_tables", C.c_int32),
        ("geom_type", _p_i32), ("geom_params", _p_f64), ("local_to_world", _p_f64),
        ("world_to_local", _p_f64), ("refractive_index", _p_f64), ("surface_type", _p_i32),
        ("comp_start", _p_i32), ("comp_count", _p_i32), ("coat_start", _p_i32),
        ("coat_count", _p_i32),
        ("comp_type", _p_i32), ("comp_qy", _p_f64), ("comp_tau_rad", _p_f64),
        ("comp_tau_nr", _p_f64), ("comp_phase_type", _p_i32), ("comp_phase_param", _p_f64),
        ("comp_abs_start", _p_i32), ("comp_abs_n", _p_i32), ("comp_ems_start", _p_i32),
        ("comp_ems_n", _p_i32),
        ("abs_x", _p_f64), ("abs_y", _p_f64), ("ems_x", _p_f64), ("ems_cdf", _p_f64),
        ("rec_node", _p_i32), ("rec_event", _p_i32), ("rec_has_facet", _p_i32),
        ("rec_facet", _p_f64), ("rec_atol", _p_f64), ("rec_hist_start", _p_i32),
        ("rec_hist_n", _p_i32),
        ("hist_prop_a", _p_i32), ("hist_prop_b", _p_i32), ("hist_na", _p_i32),
        ("hist_nb", _p_i32), ("hist_lo_a", _p_f64), ("hist_hi_a", _p_f64),
        ("hist_lo_b", _p_f64), ("hist_hi_b", _p_f64), ("hist_offset", _p_i32),
        ("coat_facet", _p_f64), ("coat_lo", _p_f64), ("coat_hi", _p_f64),
        ("coat_reflectivity", _p_f64), ("coat_reflect_mode", _p_i32),
        ("coat_transmit_mode", _p_i32),
        ("rec_source_mode", _p_i32), ("rec_source_id", _p_i32),
        ("comp_abs_hist", _p_i32), ("comp_ems_hist", _p_i32),
        ("n_mesh_vertices", C.c_int32), ("n_mesh_faces", C.c_int32),
        ("mesh_face_start", _p_i32), ("mesh_face_count", _p_i32), ("mesh_vertices", _p_f64),
        ("mesh_faces", _p_i32), ("mesh_normals", _p_f64),
        # coating reflectivity tables (read only when n_coat_tables > 0)
        ("coat_table", _p_i32),
        ("n_ctab_wavelength", C.c_int32), ("n_ctab_angle", C.c_int32), ("n_ctab_value", C.c_int32),
        ("reserved1", C.c_int32),
        ("ctab_nw", _p_i32), ("ctab_na", _p_i32), ("ctab_wl_start", _p_i32), ("ctab_angle_start", _p_i32),
        ("ctab_value_start", _p_i32), ("ctab_wavelength", _p_f64), ("ctab_angle", _p_f64), ("ctab_value", _p_f64),
    ]
    POINTERS = _same_names(_fields_)
    COUNTS = {
        "n_nodes": lambda c: c.geom_type.shape[0], "root_id": lambda c: c.root_id,
        "n_components": lambda c: c.comp_type.shape[0], "n_abs": lambda c: c.abs_x.shape[0],
        "n_ems": lambda c: c.ems_x.shape[0], "n_recorders": lambda c: c.rec_node.shape[0],
        "n_hists": lambda c: c.hist_prop_a.shape[0], "total_bins": lambda c: c.total_bins,
        "n_coatings": lambda c: getattr(c, "n_coatings", 0), "n_mesh_vertices": lambda c: getattr(c, "n_mesh_vertices", 0),
        "n_mesh_faces": lambda c: getattr(c, "n_mesh_faces", 0), "n_coat_tables": lambda c: getattr(c, "n_coat_tables", 0),
        "n_ctab_wavelength": lambda c: c.ctab_wavelength.shape[0] if getattr(c, "n_coat_tables", 0) else 0,
        "n_ctab_angle": lambda c: c.ctab_angle.shape[0] if getattr(c, "n_coat_tables", 0) else 0,
        "n_ctab_value": lambda c: c.ctab_value.shape[0] if getattr(c, "n_coat_tables", 0) else 0,
    }
    ABSENT = staticmethod(lambda c: False)

    @staticmethod
    def MISSING(st, field, dtype):
        """A table the object does not have at all: `coat_table` of a flattener without coating tables names no table,
        the tables of an engine without the coating extension are zeros."""
        if field == "coat_table":
            return np.full(max(st.n_coatings, 1), -1, dtype=dtype)
        return np.zeros(max(st.n_nodes, 1) * 3, dtype=dtype)


class PvtIndexTables(C.Structure):
    """Refractive-index tables n(wavelength) of a scene (include/pvtrace_hip.h; pvt_scene_create_ex); absent when the
    scene has no dispersive node."""
    _fields_ = [
        ("n_tables", C.c_int32), ("n_points", C.c_int32),
        ("node_table", _p_i32), ("table_n", _p_i32), ("table_start", _p_i32),
        ("wavelength", _p_f64), ("value", _p_f64),
    ]
    POINTERS = {"node_table": ("ri_table", np.int32), "table_n": ("rtab_n", np.int32), "table_start": ("rtab_start", np.int32),
                "wavelength": ("rtab_wavelength", np.float64), "value": ("rtab_value", np.float64)}
    COUNTS = {"n_tables": lambda c: c.n_ri_tables, "n_points": lambda c: c.rtab_wavelength.shape[0]}
    ABSENT = staticmethod(lambda c: int(getattr(c, "n_ri_tables", 0)) == 0)


class PvtPhaseTables(C.Structure):
    """Phase-function tables of a scene (include/pvtrace_hip.h; pvt_scene_create_phase); absent when no component has one."""
    _fields_ = [
        ("n_tables", C.c_int32), ("n_points", C.c_int32), ("n_wavelength", C.c_int32), ("n_cdf", C.c_int32),
        ("comp_table", _p_i32), ("table_nw", _p_i32), ("table_nmu", _p_i32),
        ("wl_start", _p_i32), ("mu_start", _p_i32), ("cdf_start", _p_i32),
        ("wavelength", _p_f64), ("mu", _p_f64), ("cdf", _p_f64),
    ]
    POINTERS = {"comp_table": ("comp_phase_table", np.int32), "table_nw": ("ptab_nw", np.int32),
                "table_nmu": ("ptab_nmu", np.int32), "wl_start": ("ptab_wl_start", np.int32),
                "mu_start": ("ptab_mu_start", np.int32), "cdf_start": ("ptab_cdf_start", np.int32),
                "wavelength": ("ptab_wavelength", np.float64), "mu": ("ptab_mu", np.float64), "cdf": ("ptab_cdf", np.float64)}
    COUNTS = {"n_tables": lambda c: c.n_phase_tables, "n_points": lambda c: c.ptab_mu.shape[0],
              "n_wavelength": lambda c: c.ptab_wavelength.shape[0], "n_cdf": lambda c: c.ptab_cdf.shape[0]}
    ABSENT = staticmethod(lambda c: int(getattr(c, "n_phase_tables", 0)) == 0)


class PvtSurfaceTables(C.Structure):
    """Rough interfaces of a scene (include/pvtrace_hip.h; pvt_scene_create_rough); absent when no node is rough."""
    _fields_ = [("n_nodes", C.c_int32), ("node_roughness", _p_f64)]
    POINTERS = {"node_roughness": ("surface_roughness", np.float64)}
    COUNTS = {"n_nodes": lambda c: np.shape(c.surface_roughness)[0]}
    ABSENT = staticmethod(lambda c: getattr(c, "surface_roughness", None) is None
                          or not np.any(np.asarray(c.surface_roughness) > 0.0))


class PvtFieldTables(C.Structure):
    """Concentration fields of a scene (include/pvtrace_hip.h; pvt_scene_create_field); absent when no node carries a
    lattice."""
    _fields_ = [
        ("n_nodes", C.c_int32), ("n_fields", C.c_int32),
        ("node_field", _p_i32), ("field_shape", _p_i32), ("field_lower", _p_f64), ("field_upper", _p_f64),
        ("n_components", C.c_int32), ("n_values", C.c_int32),
        ("comp_values", _p_i32), ("values_start", _p_i32), ("values_count", _p_i32),
        ("n_points", C.c_int32), ("reserved", C.c_int32),
        ("values", _p_f64),
    ]
    POINTERS = {"node_field": ("node_field", np.int32), "field_shape": ("field_shape", np.int32),
                "field_lower": ("field_lower", np.float64), "field_upper": ("field_upper", np.float64),
                "comp_values": ("comp_values", np.int32), "values_start": ("values_start", np.int32),
                "values_count": ("values_count", np.int32), "values": ("field_values", np.float64)}
    COUNTS = {"n_nodes": lambda c: len(c.node_field), "n_fields": lambda c: c.n_fields,
              "n_components": lambda c: len(c.comp_values), "n_values": lambda c: c.n_value_tables,
              "n_points": lambda c: len(c.field_values)}
    ABSENT = staticmethod(lambda c: getattr(c, "node_field", None) is None or not np.any(np.asarray(c.node_field) >= 0))


class PvtMapTables(C.Structure):
    """Volume maps of a scene (include/pvtrace_hip.h; pvt_scene_create_maps); absent when the scene has no map."""
    _fields_ = [
        ("n_nodes", C.c_int32), ("n_maps", C.c_int32),
        ("node_map_start", _p_i32), ("node_map_count", _p_i32), ("map_kind", _p_i32), ("map_component", _p_i32),
        ("map_shape", _p_i32), ("map_lower", _p_f64), ("map_h", _p_f64), ("map_nw", _p_i32),
        ("map_wl_start", _p_f64), ("map_wl_stop", _p_f64), ("map_offset", _p_i64),
        ("map_slots", C.c_int64),
    ]
    POINTERS = {**_same_names(_fields_), "map_offset": ("map_offset", np.int64)}
    COUNTS = {"n_nodes": lambda c: len(c.node_map_start), "n_maps": lambda c: c.n_maps, "map_slots": lambda c: c.map_slots}
    ABSENT = staticmethod(lambda c: int(getattr(c, "n_maps", 0)) == 0)


class PvtCaptureTables(C.Structure):
    """Captured recorders of a scene (include/pvtrace_hip.h; pvt_scene_create_capture); absent when no recorder is
    captured."""
    _fields_ = [
        ("n_recorders", C.c_int32),
        ("rec_capture_capacity", _p_i64), ("rec_capture_start", _p_i64),
        ("capture_rows", C.c_int64),
    ]
    POINTERS = {"rec_capture_capacity": ("rec_capture_capacity", np.int64), "rec_capture_start": ("rec_capture_start", np.int64)}
    COUNTS = {"n_recorders": lambda c: len(c.rec_capture_capacity), "capture_rows": lambda c: c.capture_rows}
    ABSENT = staticmethod(lambda c: int(getattr(c, "capture_rows", 0)) == 0)


class PvtCoatingAbsorbTables(C.Structure):
    """Absorptivities of a scene's coatings (include/pvtrace_hip.h; pvt_scene_create_absorb); absent when no coating has
    one."""
    _fields_ = [
        ("n_coatings", C.c_int32), ("n_tables", C.c_int32),
        ("coat_absorptivity", _p_f64), ("coat_table", _p_i32),
        ("n_wavelength", C.c_int32), ("n_angle", C.c_int32), ("n_value", C.c_int32), ("reserved", C.c_int32),
        ("table_nw", _p_i32), ("table_na", _p_i32), ("wl_start", _p_i32), ("angle_start", _p_i32), ("value_start", _p_i32),
        ("wavelength", _p_f64), ("angle", _p_f64), ("value", _p_f64),
    ]
    POINTERS = {"coat_absorptivity": ("coat_absorptivity", np.float64), "coat_table": ("coat_abs_table", np.int32),
                "table_nw": ("atab_nw", np.int32), "table_na": ("atab_na", np.int32), "wl_start": ("atab_wl_start", np.int32),
                "angle_start": ("atab_angle_start", np.int32), "value_start": ("atab_value_start", np.int32),
                "wavelength": ("atab_wavelength", np.float64), "angle": ("atab_angle", np.float64),
                "value": ("atab_value", np.float64)}
    COUNTS = {"n_coatings": lambda c: c.n_coatings, "n_tables": lambda c: c.n_abs_tables,
              "n_wavelength": lambda c: c.atab_wavelength.shape[0], "n_angle": lambda c: c.atab_angle.shape[0],
              "n_value": lambda c: c.atab_value.shape[0]}
    ABSENT = staticmethod(lambda c: not getattr(c, "has_absorbing_coatings", False))


class PvtCoatingPatternTables(C.Structure):
    """Where a scene's coatings cover: any-facet flags and mask lattices (include/pvtrace_hip.h; pvt_scene_create_pattern);
    absent when no coating has a pattern or facet=None."""
    _fields_ = [
        ("n_coatings", C.c_int32), ("n_patterns", C.c_int32),
        ("coat_any_facet", _p_i32), ("coat_pattern", _p_i32),
        ("shape", _p_i32), ("bounded", _p_i32), ("lower", _p_f64), ("h", _p_f64),
        ("mask_start", _p_i64), ("mask", _p_u8), ("n_mask", C.c_int64),
    ]
    POINTERS = {"coat_any_facet": ("coat_any_facet", np.int32), "coat_pattern": ("coat_pattern", np.int32),
                "shape": ("cpat_shape", np.int32), "bounded": ("cpat_bounded", np.int32), "lower": ("cpat_lower", np.float64),
                "h": ("cpat_h", np.float64), "mask_start": ("cpat_start", np.int64), "mask": ("cpat_mask", np.uint8)}
    COUNTS = {"n_coatings": lambda c: c.n_coatings, "n_patterns": lambda c: c.n_coat_patterns,
              "n_mask": lambda c: c.cpat_mask.shape[0]}
    ABSENT = staticmethod(lambda c: not getattr(c, "has_coating_patterns", False))


class PvtAlignTables(C.Structure):
    """Aligned components of a scene: directors in the root's frame, absorption orders and emission tables
    (include/pvtrace_hip.h; pvt_scene_create_aligned); absent when no component has an `Alignment`."""
    _fields_ = [
        ("n_components", C.c_int32), ("n_records", C.c_int32),
        ("comp_align", _p_i32), ("axis", _p_f64), ("abs_order", _p_f64), ("emit_table", _p_i32),
    ]
    POINTERS = {"comp_align": ("comp_align", np.int32), "axis": ("align_axis", np.float64),
                "abs_order": ("align_abs_order", np.float64), "emit_table": ("align_emit_table", np.int32)}
    COUNTS = {"n_components": lambda c: len(c.comp_align), "n_records": lambda c: c.n_align}
    ABSENT = staticmethod(lambda c: not getattr(c, "has_alignment", False))


class PvtPolyhedronTables(C.Structure):
    """Convex polyhedra of a scene: per node its run of plane rows (nx, ny, nz, h) in the pool (include/pvtrace_hip.h;
    pvt_scene_create_polyhedra); absent when no node is a `Polyhedron`."""
    _fields_ = [
        ("n_nodes", C.c_int32), ("node_plane_start", _p_i32), ("node_plane_count", _p_i32),
        ("n_planes", C.c_int32), ("planes", _p_f64),
    ]
    POINTERS = {"node_plane_start": ("poly_start", np.int32), "node_plane_count": ("poly_count", np.int32),
                "planes": ("poly_planes", np.float64)}
    COUNTS = {"n_nodes": lambda c: len(c.poly_start), "n_planes": lambda c: len(c.poly_planes)}
    ABSENT = staticmethod(lambda c: not getattr(c, "has_polyhedron", False))


# the extension structs, in the order the pvt_scene_create* entries take them behind the scene tables (each entry takes the
# first so many of them: CREATION_ENTRIES)
EXTENSION_TABLES = (PvtIndexTables, PvtPhaseTables, PvtSurfaceTables, PvtFieldTables, PvtMapTables, PvtCaptureTables,
                    PvtCoatingAbsorbTables, PvtCoatingPatternTables, PvtAlignTables, PvtPolyhedronTables)
CREATION_ENTRIES = {"pvt_scene_create": 0, "pvt_scene_create_ex": 1, "pvt_scene_create_phase": 2, "pvt_scene_create_rough": 3,
                    "pvt_scene_create_field": 4, "pvt_scene_create_maps": 5, "pvt_scene_create_capture": 6,
                    "pvt_scene_create_absorb": 7, "pvt_scene_create_origin": 7, "pvt_scene_create_pattern": 8,
                    "pvt_scene_create_aligned": 9}
# The newest entry, the one Python calls: pvt_scene_create_aligned and the tenth struct, PvtPolyhedronTables.  It stands
# beside CREATION_ENTRIES, not in it: that table lists the entries from before the convex polyhedron, which all refuse
# geometry type 5, and of which pvt_scene_create_aligned is the only one that can be handed alignment tables.
NEWEST_ENTRY = ("pvt_scene_create_polyhedra", 10)
LEAN_CHECK_TABLES = 5   # pvt_scene_lean_check takes the first five


class PvtCaptures(C.Structure):
    """Capture buffers of one launch (device pointers)."""
    _fields_ = [("rows", C.POINTER(C.c_uint64)), ("cursors", C.POINTER(C.c_int64))]


CAPTURE_ROW_WORDS = 12   # uint64 words of a captured row (PVT_CAPTURE_ROW_WORDS)


class PvtEmitterTables(C.Structure):
    _fields_ = [
        ("n_lights", C.c_int32), ("n_spec", C.c_int32),
        ("wl_type", _p_i32), ("wl_value", _p_f64), ("wl_spec_start", _p_i32),
        ("wl_spec_n", _p_i32), ("pos_type", _p_i32), ("pos_param", _p_f64),
        ("dir_type", _p_i32), ("dir_param", _p_f64), ("light_to_world", _p_f64),
        ("spec_x", _p_f64), ("spec_cdf", _p_f64),
    ]
    POINTERS = _same_names(_fields_)   # (read from an `emit.EmitterTables`)
    COUNTS = {"n_lights": lambda e: e.n_lights, "n_spec": lambda e: e.spec_x.shape[0]}
    ABSENT = staticmethod(lambda e: False)


class PvtSourceTables(C.Structure):
    """Tabulated sources of an emitter (include/pvtrace_hip.h; pvt_scene_set_sources): position grids and direction tables,
    read from an `emit.EmitterTables` (or any object with these fields); absent when no light names one."""
    _fields_ = [
        ("n_lights", C.c_int32), ("n_grids", C.c_int32), ("n_tables", C.c_int32), ("n_grid_cdf", C.c_int32),
        ("n_table_wavelength", C.c_int32), ("n_table_mu", C.c_int32), ("n_table_cdf", C.c_int32),
        ("light_grid", _p_i32), ("light_table", _p_i32), ("grid_shape", _p_i32), ("grid_bounded", _p_i32),
        ("grid_lower", _p_f64), ("grid_h", _p_f64), ("grid_cdf_start", _p_i32), ("grid_cdf", _p_f64),
        ("table_nw", _p_i32), ("table_nmu", _p_i32), ("table_wl_start", _p_i32), ("table_mu_start", _p_i32),
        ("table_cdf_start", _p_i32), ("table_wavelength", _p_f64), ("table_mu", _p_f64), ("table_cdf", _p_f64),
    ]
    POINTERS = _same_names(_fields_)
    COUNTS = {"n_lights": lambda e: e.n_lights, "n_grids": lambda e: e.n_grids, "n_tables": lambda e: e.n_tables,
              "n_grid_cdf": lambda e: np.size(e.grid_cdf), "n_table_wavelength": lambda e: np.size(e.table_wavelength),
              "n_table_mu": lambda e: np.size(e.table_mu), "n_table_cdf": lambda e: np.size(e.table_cdf)}
    ABSENT = staticmethod(lambda e: int(getattr(e, "n_grids", 0)) == 0 and int(getattr(e, "n_tables", 0)) == 0)


class PvtTraceParams(C.Structure):
    _fields_ = [
        ("n_rays", C.c_int64), ("seed", C.c_uint64), ("ray_offset", C.c_uint64),
        ("emit_seed", C.c_uint64), ("record_every", C.c_int64), ("maxsteps", C.c_int32),
        ("max_events", C.c_int32), ("emit_method", C.c_int32), ("workgroups_per_cu", C.c_int32),
        ("tally_bundle", C.c_int64), ("tally_stride_i64", C.c_int64), ("tally_stride_f64", C.c_int64),
        ("flags", C.c_int64),
    ]


class PvtRays(C.Structure):
    _fields_ = [("position", _p_f64), ("direction", _p_f64), ("wavelength", _p_f64)]


class PvtTallies(C.Structure):
    _fields_ = [
        ("rec_distinct", _p_i64), ("rec_crossings", _p_i64), ("rec_sums", _p_f64),
        ("rec_bins", _p_i64),
    ]


class PvtEventLog(C.Structure):
    _fields_ = [
        ("counts", _p_i32), ("kind", _p_u8), ("hit", _p_i32), ("container", _p_i32),
        ("adjacent", _p_i32), ("component", _p_i32), ("source", _p_i32),
        ("position", _p_f64), ("direction", _p_f64), ("normal", _p_f64),
        ("wavelength", _p_f64), ("travelled", _p_f64), ("duration", _p_f64),
    ]


class PvtEventRecords(C.Structure):
    _fields_ = [("counts", _p_i32), ("rows", C.POINTER(C.c_uint64))]


_CTYPE_OF = {
    np.dtype(np.int32): C.c_int32, np.dtype(np.float64): C.c_double,
    np.dtype(np.int64): C.c_int64, np.dtype(np.uint8): C.c_uint8,
}


def np_ptr(array):
    """ctypes pointer to a C-contiguous numpy array's data."""
    return array.ctypes.data_as(C.POINTER(_CTYPE_OF[array.dtype]))


def addr_ptr(address, ctype):
    """ctypes pointer from a raw (device) address."""
    return C.cast(C.c_void_p(int(address)), C.POINTER(ctype))


def marshal(struct_type, source):
    """`struct_type` over the arrays of `source` (a CompiledScene; an `emit.EmitterTables` for PvtEmitterTables), as the
    struct describes itself (POINTERS, COUNTS, ABSENT) -> (struct, keepalive), or (None, {}) when the source has none of it.
    `keepalive` holds, by C field name, the contiguous arrays the pointers refer to and must outlive every use of `struct`.
    The one place an attribute becomes a pointer."""
    if struct_type.ABSENT(source):
        return None, {}
    st, keep = struct_type(), {}
    for field, derive in struct_type.COUNTS.items():
        setattr(st, field, int(derive(source)))
    for field, (attribute, dtype) in struct_type.POINTERS.items():
        missing = getattr(struct_type, "MISSING", None)   # (the scene tables alone: see PvtSceneTables.MISSING)
        value = getattr(source, attribute) if missing is None else getattr(source, attribute, None)
        if value is None:
            value = missing(st, field, dtype)
        arr = np.ascontiguousarray(value, dtype=dtype)
        if arr.size == 0:
            arr = np.zeros(1, dtype=dtype)  # never hand out NULL for an empty table
        keep[field] = arr
        setattr(st, field, np_ptr(arr))
    return st, keep


def scene_tables_struct(compiled):
    """PvtSceneTables over the arrays of a CompiledScene -> (struct, keepalive)."""
    return marshal(PvtSceneTables, compiled)


def index_tables_struct(compiled):
    return marshal(PvtIndexTables, compiled)


def phase_tables_struct(compiled):
    return marshal(PvtPhaseTables, compiled)


def surface_tables_struct(compiled):
    return marshal(PvtSurfaceTables, compiled)


def field_tables_struct(compiled):
    return marshal(PvtFieldTables, compiled)


def map_tables_struct(compiled):
    return marshal(PvtMapTables, compiled)


def capture_tables_struct(compiled):
    return marshal(PvtCaptureTables, compiled)


def absorb_tables_struct(compiled):
    return marshal(PvtCoatingAbsorbTables, compiled)


def pattern_tables_struct(compiled):
    return marshal(PvtCoatingPatternTables, compiled)


def emitter_tables_struct(emitter):
    """PvtEmitterTables over an `emit.EmitterTables` object -> (struct, keepalive)."""
    return marshal(PvtEmitterTables, emitter)


def extension_tables(compiled, count=len(EXTENSION_TABLES)):
    """The first `count` extension structs of a CompiledScene -> (the arguments a creation entry takes for them, NULL for
    an absent one; what must outlive the call)."""
    made = [marshal(struct_type, compiled) for struct_type in EXTENSION_TABLES[:count]]
    return [None if st is None else C.byref(st) for st, _ in made], made


def trace_params(n_rays, seed, ray_offset, emit_seed, record_every, maxsteps, max_events,
                 emit_method, workgroups_per_cu=0, tally_bundle=0, tally_stride_i64=0, tally_stride_f64=0, flags=0):
    mask = (1 << 64) - 1
    return PvtTraceParams(
        int(n_rays), int(seed) & mask, int(ray_offset) & mask, int(emit_seed) & mask,
        int(record_every), int(maxsteps), int(max_events), int(emit_method), int(workgroups_per_cu),
        int(tally_bundle), int(tally_stride_i64), int(tally_stride_f64), int(flags),
    )


def num_recorded(n_rays, record_every):
    return (n_rays + record_every - 1) // record_every if record_every > 0 else 0


EVENT_LOG_COLUMNS = (
    # name, dtype, per-row width
    ("kind", np.uint8, 1), ("hit", np.int32, 1), ("container", np.int32, 1),
    ("adjacent", np.int32, 1), ("component", np.int32, 1), ("source", np.int32, 1),
    ("position", np.float64, 3), ("direction", np.float64, 3), ("normal", np.float64, 3),
    ("wavelength", np.float64, 1), ("travelled", np.float64, 1), ("duration", np.float64, 1),
)


RECORD_WORDS = 16   # uint64 words of one event record (include/pvtrace_hip.h PvtEventRecords)
_ID_COLUMNS = ("hit", "container", "adjacent", "component", "source")


def decode_records(rows):
    """(m, 16) int64 event records (host numpy) -> dict of the reference's columns for those m rows
    (layout: include/pvtrace_hip.h PvtEventRecords)."""
    rows = np.ascontiguousarray(rows).reshape(-1, RECORD_WORDS)
    i32 = rows.view(np.int32).reshape(-1, 2 * RECORD_WORDS)
    f64 = rows.view(np.float64).reshape(-1, RECORD_WORDS)
    return {
        "kind": i32[:, 5].astype(np.uint8), "hit": i32[:, 0].copy(), "container": i32[:, 1].copy(),
        "adjacent": i32[:, 2].copy(), "component": i32[:, 3].copy(), "source": i32[:, 4].copy(),
        "position": f64[:, 3:6].copy(), "direction": f64[:, 6:9].copy(), "normal": f64[:, 9:12].copy(),
        "wavelength": f64[:, 12].copy(), "travelled": f64[:, 13].copy(), "duration": f64[:, 14].copy(),
    }


def declare_signatures(lib, names):
    """Set argtypes/restype of the C-ABI entry points present in `lib`."""
    vp = C.c_void_p

    def scene_inputs(count):   # the scene tables and the first `count` extension structs
        return [C.POINTER(struct_type) for struct_type in (PvtSceneTables,) + EXTENSION_TABLES[:count]]

    sigs = {
        "pvt_abi_version": ([], C.c_int),
        "pvt_last_error": ([], C.c_char_p),
        "pvt_device_count": ([], C.c_int),
        "pvt_scene_map_slots": ([vp], C.c_int64),
        "pvt_scene_capture_rows": ([vp], C.c_int64),
        "pvt_trace_device_capture": ([vp, C.POINTER(PvtRays), C.POINTER(PvtTraceParams), C.POINTER(PvtTallies),
                                      C.POINTER(PvtEventRecords), C.POINTER(PvtCaptures), vp], C.c_int),
        "pvt_scene_set_emitter": ([vp, C.POINTER(PvtEmitterTables)], C.c_int),
        "pvt_scene_set_sources": ([vp, C.POINTER(PvtEmitterTables), C.POINTER(PvtSourceTables)], C.c_int),
        "pvt_sources_check": ([C.POINTER(PvtEmitterTables), C.POINTER(PvtSourceTables)], C.c_int),
        "pvt_scene_destroy": ([vp], None),
        "pvt_trace_device": (
            [vp, C.POINTER(PvtRays), C.POINTER(PvtTraceParams), C.POINTER(PvtTallies),
             C.POINTER(PvtEventLog), vp], C.c_int),
        "pvt_trace_device_records": (
            [vp, C.POINTER(PvtRays), C.POINTER(PvtTraceParams), C.POINTER(PvtTallies),
             C.POINTER(PvtEventRecords), vp], C.c_int),
        "pvt_scene_carry_pending": ([vp, vp], C.c_int),
        "pvt_scene_carry_discard": ([vp, vp], C.c_int),
        "pvt_scene_trim": ([vp], C.c_int),
        "pvt_last_multi_reduce": ([], C.c_int),
        "pvt_unpack_records_device": (
            [C.POINTER(PvtEventRecords), C.c_int64, C.c_int32, C.POINTER(PvtEventLog), C.c_int, vp], C.c_int),
        "pvt_trace_bundle": (
            [C.POINTER(PvtSceneTables), C.POINTER(PvtEmitterTables), C.POINTER(PvtRays),
             C.POINTER(PvtTraceParams), C.POINTER(PvtTallies), C.POINTER(PvtEventLog), C.c_int,
             C.POINTER(C.c_double)], C.c_int),
        "pvt_trace_bundle_multi": (
            [C.POINTER(PvtSceneTables), C.POINTER(PvtEmitterTables), C.POINTER(PvtRays),
             C.POINTER(PvtTraceParams), C.POINTER(PvtTallies), C.POINTER(PvtEventLog), C.POINTER(C.c_int),
             C.c_int, C.POINTER(C.c_double)], C.c_int),
        "pvt_release_cached_memory": ([], None),
        "pvt_shard_range": ([C.c_int64, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
        "pvt_emit_device": ([vp, C.POINTER(PvtTraceParams), vp, vp, vp, vp], C.c_int),
        "pvt_selftest_math": ([C.c_int, vp, vp, C.c_int64, C.c_int], C.c_int),
        "pvt_mesh_bvh_check": (
            [C.POINTER(PvtSceneTables), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
             C.POINTER(C.c_int32)], C.c_int),
        "pvt_scene_launch_info": (
            [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)], C.c_int),
        "pvt_scene_variant": ([vp], C.c_int),
        "pvt_scene_entry": ([vp], C.c_int),
        "pvt_scene_lean_check": (scene_inputs(LEAN_CHECK_TABLES) + [C.POINTER(C.c_int32)], C.c_int),
        "pvt_scene_solo": ([vp], C.c_int),
        "pvt_scene_solo_check": (scene_inputs(LEAN_CHECK_TABLES) + [C.POINTER(C.c_int32)], C.c_int),
        "pvt_scene_counters": ([vp, C.POINTER(C.c_uint64), C.c_int], C.c_int),
        "pvt_scene_clock": ([vp, C.POINTER(C.c_uint64)], C.c_int),
        "pvt_scene_launch_span": ([vp, vp, C.POINTER(C.c_uint64)], C.c_int),
        "pvt_node_grid_plan": (
            [C.POINTER(PvtSceneTables), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
             C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.c_int64], C.c_int),
    }
    for name, count in list(CREATION_ENTRIES.items()) + [NEWEST_ENTRY]:
        sigs[name] = (scene_inputs(count) + [C.c_int, C.POINTER(vp)], C.c_int)
    for name in names:
        argtypes, restype = sigs[name]
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    return sigs


ABI_SYMBOLS = (
    "pvt_abi_version", "pvt_last_error", "pvt_device_count", "pvt_scene_create",
    "pvt_scene_set_emitter", "pvt_scene_destroy", "pvt_trace_device", "pvt_trace_bundle",
    "pvt_emit_device", "pvt_selftest_math", "pvt_scene_launch_info", "pvt_mesh_bvh_check",
    "pvt_trace_bundle_multi", "pvt_shard_range", "pvt_trace_device_records", "pvt_unpack_records_device",
    "pvt_scene_carry_pending", "pvt_last_multi_reduce", "pvt_node_grid_plan", "pvt_scene_carry_discard", "pvt_scene_trim",
    "pvt_scene_counters", "pvt_scene_clock", "pvt_scene_launch_span", "pvt_release_cached_memory",
    "pvt_scene_create_ex", "pvt_scene_create_phase", "pvt_scene_create_rough", "pvt_scene_create_field",
    "pvt_scene_create_maps", "pvt_scene_map_slots", "pvt_scene_variant", "pvt_scene_lean_check",
    "pvt_scene_create_capture", "pvt_scene_capture_rows", "pvt_trace_device_capture", "pvt_scene_create_absorb",
    "pvt_scene_create_origin", "pvt_scene_create_pattern", "pvt_scene_create_aligned", "pvt_scene_entry",
    "pvt_scene_create_polyhedra", "pvt_scene_solo", "pvt_scene_solo_check", "pvt_scene_set_sources", "pvt_sources_check",
)
VARIANT_NAMES = ("lean", "w4", "grid", "rough", "mesh")   # include/pvtrace_hip.h PVT_VARIANT_*
# the family's entry point a launch ran (PVT_ENTRY_*): its usual kernel, or the lean family's parking one
ENTRY_NAMES = {"lean": ("trace_kernel_lean_w4", "trace_kernel_lean_park")}

_lib = None
ABI_VERSION = 13  # include/pvtrace_hip.h PVT_ABI_VERSION
FLAG_NO_LOG_PREFILL = 1   # PvtTraceParams.flags
FLAG_CARRY_OUT = 2        # park the photons still alive at the end of the launch for the next launch on the stream


def library_built():
    return os.path.exists(LIB_PATH)


def _preload_torch_hip_runtime():
    """One process must not hold two HIP/HSA runtimes.  PyTorch wheels bundle their own
    libamdhip64.so.7 (+ libhsa-runtime64) under torch/lib; our library's NEEDED entry has
    the same SONAME and a RUNPATH to /opt/rocm.  If ours loaded first, the system runtime
    would be mapped and torch's bundled HSA would later fail with "No HIP GPUs are
    available".  So when torch is installed, map ITS runtime first (without importing
    torch); the dynamic loader then resolves our NEEDED entry to that same copy, whatever
    the import order.  Without torch the RUNPATH copy is used."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if not os.path.exists(path):
        return None
    try:
        return C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError:
        return None


def load_library():
    """dlopen the engine (needs libamdhip64 from /opt/rocm, present on CPU boxes too)."""
    global _lib
    if _lib is None:
        if not library_built():
            raise EngineUnavailableError(
                f"{LIB_PATH} is not built; run `python -c 'import __graft_entry__ as g; g.build()'`"
                " (hipcc --offload-arch=gfx950)."
            )
        _preload_torch_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        declare_signatures(lib, ABI_SYMBOLS)
        if lib.pvt_abi_version() != ABI_VERSION:   # a stale .so would misread the table struct
            raise EngineUnavailableError(
                f"{LIB_PATH} implements ABI v{lib.pvt_abi_version()}, this package needs v{ABI_VERSION}; "
                "rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)."
            )
        _lib = lib
    return _lib


def check(code, what):
    if code == 0:
        return
    lib = load_library()
    detail = lib.pvt_last_error()
    detail = detail.decode() if detail else ""
    if code == -2:
        raise ValueError("Engine supports at most 128 geometry nodes.")
    if code == -1:
        raise ValueError(f"{what}: invalid argument ({detail})")
    raise EngineUnavailableError(f"{what} failed with code {code}: {detail}")


def device_count():
    return int(load_library().pvt_device_count())


def is_available():
    """True iff the HIP library is built AND at least one GPU is visible."""
    if not library_built():
        return False
    try:
        return device_count() > 0
    except OSError:
        return False


def shard_range(n_rays, shard, n_shards, align=1):
    """The library's own shard arithmetic (pvt_shard_range; pure host code, no GPU needed)."""
    lib = load_library()
    a, b = C.c_int64(), C.c_int64()
    check(lib.pvt_shard_range(int(n_rays), int(shard), int(n_shards), int(align), C.byref(a), C.byref(b)),
          "pvt_shard_range")
    return a.value, b.value


def selftest_math(fn, x, device=0):
    """y = f(x) evaluated on the GPU (see pvt_selftest_math in the header)."""
    lib = load_library()
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    check(lib.pvt_selftest_math(int(fn), x.ctypes.data, y.ctypes.data, x.size, int(device)),
          "pvt_selftest_math")
    return y


def mesh_bvh_check(compiled, node):
    """Build the BVH of mesh node `node` on the host and verify its invariants (no GPU needed)
    -> (bvh nodes, leaves, depth)."""
    lib = load_library()
    st, keep = scene_tables_struct(compiled)
    out = [C.c_int32(0) for _ in range(3)]
    check(lib.pvt_mesh_bvh_check(C.byref(st), int(node), *(C.byref(v) for v in out)), "pvt_mesh_bvh_check")
    del keep
    return tuple(int(v.value) for v in out)


def sources_check(emitter):
    """The packer's validation of an emitter and its tabulated sources (host only, no GPU needed; include/pvtrace_hip.h:
    pvt_sources_check) -> None when they are accepted, else the refusal's message.  `emitter`: an `emit.EmitterTables`
    or any object with its fields; without a grid or a table it is checked as pvt_scene_set_emitter checks it."""
    lib = load_library()
    st, keep = emitter_tables_struct(emitter)
    sources, keep_sources = marshal(PvtSourceTables, emitter)
    code = lib.pvt_sources_check(C.byref(st), None if sources is None else C.byref(sources))
    del keep, keep_sources
    return None if code == 0 else lib.pvt_last_error().decode()


def lean_check(compiled):
    """True when the library proves the scene plain from its packed tables (host only, no GPU needed;
    include/pvtrace_hip.h: pvt_scene_lean_check): its launches may run the lean kernel family."""
    return lean_kind(compiled) != 0


def lean_kind(compiled):
    """pvt_scene_lean_check's own answer: 0 = not plain, 1 = plain with a spectrum on a grid that is even only up to
    rounding (the family's kernels that search the tables), 2 = plain with every spectrum a constant or even bit for bit."""
    lib = load_library()
    st, keep = scene_tables_struct(compiled)
    others, alive = extension_tables(compiled, LEAN_CHECK_TABLES)
    lean = C.c_int32(0)
    check(lib.pvt_scene_lean_check(C.byref(st), *others, C.byref(lean)), "pvt_scene_lean_check")
    del keep, alive
    return int(lean.value)


def lean_refusal(compiled):
    """Why the library does not prove the scene plain: the first clause of the proof that its packed tables fail
    (pvt_scene_lean_check's message), or None for a lean scene.  Host only."""
    if lean_kind(compiled) != 0:
        return None
    return load_library().pvt_last_error().decode().removeprefix("not lean: ")


def solo_check(compiled):
    """True when the library proves the scene solo from its packed tables -- lean, and one unrotated box in a lazy root
    that holds nothing and carries no recorder (host only; include/pvtrace_hip.h: pvt_scene_solo_check): its tally
    launches may run the trace_kernel_solo entries.  False under PVT_NO_SOLO."""
    lib = load_library()
    st, keep = scene_tables_struct(compiled)
    others, alive = extension_tables(compiled, LEAN_CHECK_TABLES)
    solo = C.c_int32(0)
    check(lib.pvt_scene_solo_check(C.byref(st), *others, C.byref(solo)), "pvt_scene_solo_check")
    del keep, alive
    return bool(solo.value)


def solo_refusal(compiled):
    """The first clause of the solo proof that the scene's packed tables fail (pvt_scene_solo_check's message), or None
    for a solo scene.  Host only."""
    if solo_check(compiled):
        return None
    return load_library().pvt_last_error().decode().removeprefix("not solo: ")


def node_grid_plan(compiled):
    """The node grid the library files the nodes of a many-node scene under (host only, no GPU needed;
    include/pvtrace_hip.h: pvt_node_grid_plan) -> dict(dims, lo, cell, guard, odd, masks[cells, 2] uint64),
    or None when the scene is served by the plain node loop."""
    lib = load_library()
    st, keep = scene_tables_struct(compiled)
    dims = (C.c_int32 * 3)()
    lo, cell = (C.c_double * 3)(), (C.c_double * 3)()
    guard, odd = C.c_double(0.0), C.c_int32(0)
    check(lib.pvt_node_grid_plan(C.byref(st), dims, lo, cell, C.byref(guard), C.byref(odd), None, 0), "pvt_node_grid_plan")
    if dims[0] == 0:
        del keep
        return None
    cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    masks = np.zeros((cells, 2), dtype=np.uint64)
    check(lib.pvt_node_grid_plan(C.byref(st), dims, lo, cell, C.byref(guard), C.byref(odd),
                                 masks.ctypes.data_as(C.POINTER(C.c_uint64)), masks.size), "pvt_node_grid_plan")
    del keep
    return {"dims": tuple(int(v) for v in dims), "lo": np.array(list(lo)), "cell": np.array(list(cell)),
            "guard": float(guard.value), "odd": bool(odd.value), "masks": masks}


class DeviceScene:
    """Scene tables resident in HBM on one GPU (uploaded once, reused per bundle)."""

    def __init__(self, compiled, device=0, emitter=None):
        self.lib = load_library()
        if device_count() <= 0:
            raise EngineUnavailableError("No HIP device visible; the engine has no CPU path.")
        self.compiled = compiled
        self.device = int(device)
        st, keep = scene_tables_struct(compiled)
        others, alive = extension_tables(compiled, NEWEST_ENTRY[1])
        handle = C.c_void_p()
        # (the newest entry, the only one Python ever calls: the older ones do the same with NULL for the structs they lack)
        check(getattr(self.lib, NEWEST_ENTRY[0])(C.byref(st), *others, self.device, C.byref(handle)), NEWEST_ENTRY[0])
        del keep, alive
        self.handle = handle
        self.has_emitter = False
        # HIP stream handle -> weak reference to the BundlePipeline whose job lives on it (parked photons belong to a
        # job, and torch hands the same stream handles out again: see claim_stream)
        self._stream_owners = {}
        self._owners_lock = threading.Lock()
        if emitter is not None:
            self.set_emitter(emitter)

    def set_emitter(self, emitter):
        st, keep = emitter_tables_struct(emitter)
        sources, keep_sources = marshal(PvtSourceTables, emitter)
        if sources is None:
            check(self.lib.pvt_scene_set_emitter(self.handle, C.byref(st)), "pvt_scene_set_emitter")
        else:   # (the one entry that knows position grids and direction tables)
            check(self.lib.pvt_scene_set_sources(self.handle, C.byref(st), C.byref(sources)), "pvt_scene_set_sources")
        self.has_emitter = True

    def close(self):
        if getattr(self, "handle", None):
            self.lib.pvt_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counters(self, reset=False):
        """The scene's always-on step counters since creation / the last reset (pvt_scene_counters): wave-iterations,
        lane-steps, fused exits, waves retired, and what follows from them.  `lane_steps + fused_exits` is the
        reference's loop count (_kernel.pyx:655) summed over the photons traced.  Synchronises the device first."""
        import torch

        torch.cuda.synchronize(self.device)
        out = (C.c_uint64 * 4)()
        check(self.lib.pvt_scene_counters(self.handle, out, 1 if reset else 0), "pvt_scene_counters")
        it, ls, fused, waves = (int(v) for v in out)
        return {"wave_iterations": it, "lane_steps": ls, "fused_exits": fused, "waves": waves,
                "steps": ls + fused, "lane_utilisation": ls / (64.0 * it) if it else 0.0}

    def clock(self):
        """The clocks the scene's launches ran at since its creation / the last `counters(reset=True)`, read on the GPU
        (pvt_scene_clock): shader cycles and 100 MHz ticks summed over the workgroups' lives, and their ratio in MHz.
        Synchronises the device first."""
        import torch

        torch.cuda.synchronize(self.device)
        out = (C.c_uint64 * 2)()
        check(self.lib.pvt_scene_clock(self.handle, out), "pvt_scene_clock")
        cycles, ticks = int(out[0]), int(out[1])
        return {"shader_cycles": cycles, "ticks_100mhz": ticks, "shader_clock_mhz": 100.0 * cycles / ticks if ticks else 0.0}

    def launch_span_ms(self, stream=None):
        """GPU-side duration of the last launch on `stream` (a raw handle; default: torch's current stream), from the
        kernel's own 100 MHz stamps (pvt_scene_launch_span) -- unlike a pair of HIP events around `trace`, it cannot contain
        time the host spent between recording them.  Synchronises the stream."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        out = (C.c_uint64 * 2)()
        check(self.lib.pvt_scene_launch_span(self.handle, C.c_void_p(stream), out), "pvt_scene_launch_span")
        return (int(out[1]) - int(out[0])) * 1e-5

    def launch_info(self):
        g, b, l = C.c_int32(), C.c_int32(), C.c_int32()
        check(self.lib.pvt_scene_launch_info(self.handle, C.byref(g), C.byref(b), C.byref(l)),
              "pvt_scene_launch_info")
        variant = int(self.lib.pvt_scene_variant(self.handle))
        if variant < 0:
            check(variant, "pvt_scene_variant")
        info = {"grid": g.value, "block": b.value, "lds_bytes": l.value, "variant": VARIANT_NAMES[variant]}
        entry = int(self.lib.pvt_scene_entry(self.handle))
        if entry < 0:
            check(entry, "pvt_scene_entry")
        if VARIANT_NAMES[variant] in ENTRY_NAMES:   # (the families with more than one entry per kind of launch)
            info["entry"] = ENTRY_NAMES[VARIANT_NAMES[variant]][entry]
        return info

    def solo(self):
        """Whether the last launch on this scene ran a solo entry (pvt_scene_solo): a tally launch of a scene that is one
        box in a lazy root; `launch_info` goes on reporting the lean family and its park / usual entry for it."""
        solo = int(self.lib.pvt_scene_solo(self.handle))
        if solo < 0:
            check(solo, "pvt_scene_solo")
        return bool(solo)

    # -- device buffers (torch tensors) ----------------------------------
    def new_tallies(self, sets=1, captures=True):
        """Zeroed recorder accumulators on the GPU -> `TallySet` (tally_set.py owns their layout).  `sets` > 1: that many
        consecutive sets (the bundles of a stream traced by one launch, PvtTraceParams.tally_bundle).  A scene with captured
        recorders gets its capture rows as well: a buffer that no launch will append to is made with `captures=False`,
        and `sets` x `capture_rows` may not exceed MAX_CAPTURE_ROWS."""
        import torch

        from pvtrace_amd.engine.tally_set import TallySet

        return TallySet(self.compiled, torch.device("cuda", self.device), sets=sets, captures=captures)

    def new_event_log(self, n_rays, record_every, max_events):
        """Event-RECORD buffers for one bundle (PvtEventRecords): `counts` (recorded rays) and `rows`
        (recorded rays x max_events, 16) int64 -- one 128-byte row per event, uninitialised: only the
        rows k < counts[j] of recorded ray j are ever written (`decode_records`)."""
        import torch

        dev = torch.device("cuda", self.device)
        nrec = num_recorded(n_rays, record_every)
        rows = nrec * max_events
        return {"counts": torch.empty(max(nrec, 1), dtype=torch.int32, device=dev),
                "rows": torch.empty((max(rows, 1), RECORD_WORDS), dtype=torch.int64, device=dev)}

    def new_event_columns(self, n_rays, record_every, max_events):
        """The reference's thirteen column arrays on the device (PvtEventLog), for `unpack_records`."""
        import torch

        dev = torch.device("cuda", self.device)
        nrec = num_recorded(n_rays, record_every)
        rows = nrec * max_events
        log = {"counts": torch.empty(max(nrec, 1), dtype=torch.int32, device=dev)}
        tmap = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
        for name, dtype, width in EVENT_LOG_COLUMNS:
            log[name] = torch.empty(max(rows, 1) * width, dtype=tmap[dtype], device=dev)
        return log

    @staticmethod
    def _columns_struct(log):
        el = PvtEventLog()
        el.counts = addr_ptr(log["counts"].data_ptr(), C.c_int32)
        for name, dtype, _ in EVENT_LOG_COLUMNS:
            setattr(el, name, addr_ptr(log[name].data_ptr(), _CTYPE_OF[np.dtype(dtype)]))
        return el

    def unpack_records(self, records, columns, n_recorded, max_events, prefill=True, stream=None):
        """Records -> column arrays on the device (pvt_unpack_records_device)."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        rec = PvtEventRecords(addr_ptr(records["counts"].data_ptr(), C.c_int32),
                              addr_ptr(records["rows"].data_ptr(), C.c_uint64))
        el = self._columns_struct(columns)
        check(self.lib.pvt_unpack_records_device(C.byref(rec), int(n_recorded), int(max_events), C.byref(el),
                                                 1 if prefill else 0, C.c_void_p(stream)), "pvt_unpack_records_device")

    def trace(self, rays, n_rays, seed, tallies, log=None, ray_offset=0, emit_seed=0,
              record_every=0, maxsteps=1000, max_events=128, emit_method=0, stream=None,
              workgroups_per_cu=0, tally_bundle=0, log_prefill=True, carry_out=False):
        """Enqueue one bundle (`workgroups_per_cu`: see PvtTraceParams; 0 = the library default).
        `rays` is None (device emission) or a tuple of
        three float64 CUDA tensors (positions (n,3), directions (n,3), wavelengths (n)).
        `carry_out` (tally launches of a stream of bundles): PVT_FLAG_CARRY_OUT -- the photons still alive when the
        launch runs out of new rays are parked for the NEXT launch on this HIP stream instead of being traced to
        completion; finish a job with a launch without it (`n_rays` may be 0), see `carry_pending`."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if tally_bundle:
            need = -(-int(n_rays) // int(tally_bundle))
            if record_every > 0:
                raise ValueError("tally_bundle needs record_every == 0")
            if tallies.sets < need:
                raise ValueError(f"{need} tally sets needed, the buffers hold {tallies.sets}")
        params = trace_params(n_rays, seed, ray_offset, emit_seed, record_every, maxsteps,
                              max_events, emit_method, workgroups_per_cu, tally_bundle,
                              tallies.layout.stride_i64 if tally_bundle else 0,
                              tallies.layout.stride_f64 if tally_bundle else 0,
                              (0 if log_prefill else FLAG_NO_LOG_PREFILL) | (FLAG_CARRY_OUT if carry_out else 0))
        tl = tallies.struct
        rays_ref = None
        if rays is not None:
            pos, direc, wl = rays
            for t in (pos, direc, wl):
                if t.dtype != torch.float64 or not t.is_contiguous() or t.device.index != self.device:
                    raise ValueError("rays must be contiguous float64 tensors on the scene's GPU")
            rays_ref = C.byref(PvtRays(addr_ptr(pos.data_ptr(), C.c_double),
                                       addr_ptr(direc.data_ptr(), C.c_double),
                                       addr_ptr(wl.data_ptr(), C.c_double)))
        elif not self.has_emitter and n_rays > 0:
            raise ValueError("device emission requested but the scene has no emitter tables")
        if record_every > 0 and log is None:
            raise ValueError("record_every > 0 needs event-log buffers")
        if record_every > 0 and "rows" not in log:
            # column arrays (PvtEventLog) on the device: the library stages the records and unpacks them
            el = self._columns_struct(log)
            check(self.lib.pvt_trace_device(self.handle, rays_ref, C.byref(params), C.byref(tl),
                                            C.byref(el), C.c_void_p(stream)), "pvt_trace_device")
            return
        rec_ref = None
        if record_every > 0:
            rec_ref = C.byref(PvtEventRecords(addr_ptr(log["counts"].data_ptr(), C.c_int32),
                                              addr_ptr(log["rows"].data_ptr(), C.c_uint64)))
        # a set with captured recorders: the launch appends to its rows at their cursors (NULL: exactly pvt_trace_device_records)
        cap = tallies.capture_struct
        check(self.lib.pvt_trace_device_capture(self.handle, rays_ref, C.byref(params), C.byref(tl), rec_ref,
                                                None if cap is None else C.byref(cap), C.c_void_p(stream)),
              "pvt_trace_device_capture")

    def carry_pending(self, stream=None):
        """True when photons parked by the last launch on `stream` (`carry_out=True`) wait to be resumed."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        return bool(self.lib.pvt_scene_carry_pending(self.handle, C.c_void_p(stream)))

    def trim(self):
        """Before the scene is put aside for reuse: free staging buffers, forget parked photons (pvt_scene_trim).
        Refused while a live pipeline still owns one of the scene's streams: its parked photons would vanish."""
        live = self.stream_owners()
        if live:
            raise RuntimeError(f"{len(live)} BundlePipeline(s) still hold streams of this scene; close them first "
                               "(trimming would drop the photons their jobs have parked)")
        check(self.lib.pvt_scene_trim(self.handle), "pvt_scene_trim")

    # -- who a stream's parked photons belong to ------------------------------------------------------------------
    def stream_owners(self):
        """The live pipelines that own a stream of this scene."""
        with self._owners_lock:
            owners = {}
            for handle, ref in list(self._stream_owners.items()):
                owner = ref()
                if owner is None:
                    del self._stream_owners[handle]   # its job died with it
                else:
                    owners[id(owner)] = owner
            return list(owners.values())

    def claim_stream(self, owner, stream_handle):
        """`owner` (a BundlePipeline) starts a job on `stream_handle`.  torch hands out streams from a pool of ~32 per
        device, so the handle may be one an EARLIER pipeline used: if that pipeline is gone (closed, or dropped) whatever
        it left parked belongs to a dead job and is discarded; if it is still alive the two jobs would resume each
        other's photons, and the claim is refused."""
        import weakref

        with self._owners_lock:
            ref = self._stream_owners.get(stream_handle)
            other = ref() if ref is not None else None
            if other is not None and other is not owner:
                raise RuntimeError(
                    "this HIP stream already carries the job of another live BundlePipeline on the same scene (torch reuses "
                    "stream handles); close() that pipeline first, or give each pipeline a scene of its own")
            self._stream_owners[stream_handle] = weakref.ref(owner)
        if self.carry_pending(stream_handle):
            self.carry_discard(stream_handle)

    def release_stream(self, owner, stream_handle):
        with self._owners_lock:
            ref = self._stream_owners.get(stream_handle)
            if ref is not None and ref() in (owner, None):
                del self._stream_owners[stream_handle]

    def carry_discard(self, stream=None):
        """Forget the photons parked on `stream` (an abandoned job)."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        check(self.lib.pvt_scene_carry_discard(self.handle, C.c_void_p(stream)), "pvt_scene_carry_discard")

    def emit(self, n_rays, emit_seed, ray_offset=0, stream=None):
        """Device-side emission only -> (positions, directions, wavelengths) CUDA tensors."""
        import torch

        if not self.has_emitter:
            raise ValueError("scene has no emitter tables")
        dev = torch.device("cuda", self.device)
        pos = torch.empty((n_rays, 3), dtype=torch.float64, device=dev)
        direc = torch.empty((n_rays, 3), dtype=torch.float64, device=dev)
        wl = torch.empty(n_rays, dtype=torch.float64, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        params = trace_params(n_rays, 0, ray_offset, emit_seed, 0, 0, 0, 0)
        check(self.lib.pvt_emit_device(self.handle, C.byref(params), C.c_void_p(pos.data_ptr()),
                                       C.c_void_p(direc.data_ptr()), C.c_void_p(wl.data_ptr()),
                                       C.c_void_p(stream)), "pvt_emit_device")
        return pos, direc, wl
