"""Malformed scene tables, one broken field per case, and the refusal each must meet: the case lists of the GPU tests that
hand them to a pvt_scene_create* entry (tests/test_gpu_parity.py, test_gpu_dispersion.py, test_gpu_rough_surfaces.py,
test_gpu_concentration_fields.py, test_gpu_volume_maps.py) and of tests/test_table_refusals.py, which hands the same
cases to pvt_scene_lean_check -- the packer's host half, no GPU -- and expects the same answer.

Not every case can meet the same refusal there: LEAN_CHECK_CANNOT names those that cannot, each with its reason."""
import numpy as np

from pvtrace_amd.engine import native
from tests import scenes

INVALID, TOO_MANY_NODES = -1, -2


# -- the core tables (PvtSceneTables; tests/test_gpu_parity.py) ----------------------------------------------------------
def _coating_table_scene():
    from pvtrace_amd import (Box, CoatedSurfaceDelegate, Coating, Light, Luminophore, Material, Node, ReflectivityTable,
                             Scene, Surface, rectangular_mask)
    from pvtrace_amd.data import lumogen_f_red_305
    from tests import coating_table_scene as S

    table = ReflectivityTable(S.MIRROR_WAVELENGTH, S.MIRROR_VALUE, angle=S.MIRROR_ANGLE)
    scene, _ = S.build(Node, Scene, Box, Material, Surface, Light, rectangular_mask, lambda: S.PUMP_NM,
                       S.components(Luminophore, lumogen_f_red_305),
                       delegate=CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=table)]))
    return scene


def _cfg2():
    from benchmarks.configs import cfg2_lsc

    return cfg2_lsc()


def _set(st, keep, name, index, value):
    """Table `name` of the struct with element `index` replaced (a copy: the compiled scene is left alone)."""
    arr = keep[name].copy()
    arr[index] = value
    keep[name] = arr
    setattr(st, name, native.np_ptr(arr))


def _many_coating_tables(st, keep, c):
    """As many tables as make 2^27 doubles, every one of them the scene's own (same ranges of the pools)."""
    nt = (1 << 27) // int(c.ctab_nw[0] + c.ctab_na[0] + c.ctab_nw[0] * c.ctab_na[0]) + 1
    for name in ("ctab_nw", "ctab_na", "ctab_wl_start", "ctab_angle_start", "ctab_value_start"):
        keep[name] = np.full(nt, keep[name][0], dtype=np.int32)
        setattr(st, name, native.np_ptr(keep[name]))
    st.n_coat_tables = nt


SCENES = {"cfg2": _cfg2, "mesh_lsc": scenes.mesh_lsc, "coating_table": _coating_table_scene, "two_nodes": scenes.hello_world}
BROKEN_TABLES = [   # (scene, how one field is broken, return code, pvt_last_error)
    ("two_nodes", lambda st, k, c: setattr(st, "n_nodes", 0), INVALID, "scene has no nodes"),
    ("two_nodes", lambda st, k, c: setattr(st, "n_nodes", 129), TOO_MANY_NODES, "more than 128 geometry nodes"),
    ("cfg2", lambda st, k, c: setattr(st, "n_recorders", 257), INVALID, "more than 256 recorders"),
    ("two_nodes", lambda st, k, c: _set(st, k, "geom_type", 1, 4), INVALID, "unknown geometry type"),
    ("mesh_lsc", lambda st, k, c: setattr(st, "mesh_faces", None), INVALID, "mesh node without mesh tables"),
    ("mesh_lsc", lambda st, k, c: _set(st, k, "mesh_face_count", 1, c.n_mesh_faces + 1), INVALID,
     "mesh face range out of bounds"),
    ("mesh_lsc", lambda st, k, c: setattr(st, "n_mesh_faces", 1 << 27), INVALID, "more than 2^27 mesh faces in one scene"),
    ("mesh_lsc", lambda st, k, c: _set(st, k, "mesh_faces", 3 * c.mesh_face_start[1] + 2, c.n_mesh_vertices), INVALID,
     "mesh face indexes a missing vertex"),
    ("coating_table", lambda st, k, c: setattr(st, "ctab_angle", None), INVALID, "coating tables: missing arrays"),
    ("coating_table", lambda st, k, c: _set(st, k, "ctab_na", 0, st.n_ctab_angle + 1), INVALID,
     "coating tables: axis or value range out of bounds"),
    ("coating_table", lambda st, k, c: _set(st, k, "ctab_wavelength", 2, np.inf), INVALID,
     "coating tables: wavelengths must be finite and strictly increasing"),
    ("coating_table", lambda st, k, c: _set(st, k, "ctab_angle", 1, 0.0), INVALID,
     "coating tables: angles must be strictly increasing, in [0, 90] degrees"),
    ("coating_table", lambda st, k, c: _set(st, k, "ctab_value", 3, -0.5), INVALID, "coating tables: values must be in [0, 1]"),
    ("coating_table", _many_coating_tables, INVALID, "coating tables: more than 2^27 doubles"),
    ("coating_table", lambda st, k, c: _set(st, k, "coat_table", 0, 1), INVALID, "coating row names a missing table"),
    ("two_nodes", lambda st, k, c: _set(st, k, "refractive_index", 1, np.nan), INVALID,
     "refractive indices must be finite and positive"),
    ("cfg2", lambda st, k, c: _set(st, k, "comp_count", 1, 3), INVALID, "component range of a node out of bounds"),
    ("cfg2", lambda st, k, c: _set(st, k, "rec_node", 9, 2), INVALID, "recorder on a missing node"),
    # ranges the packer and the kernel follow that were not checked before
    ("two_nodes", lambda st, k, c: setattr(st, "root_id", 2), INVALID, "root node out of range"),
    ("cfg2", lambda st, k, c: _set(st, k, "comp_abs_n", 0, c.abs_x.shape[0] + 1), INVALID,
     "absorption spectrum range of a component out of bounds"),
    ("coating_table", lambda st, k, c: _set(st, k, "comp_ems_start", 0, 1), INVALID,
     "emission spectrum range of a component out of bounds"),
    ("coating_table", lambda st, k, c: _set(st, k, "coat_count", 1, 2), INVALID, "coating range of a node out of bounds"),
    ("cfg2", lambda st, k, c: _set(st, k, "rec_hist_start", 0, c.hist_prop_a.shape[0]), INVALID,
     "histogram range of a recorder out of bounds"),
    ("mesh_lsc", lambda st, k, c: _set(st, k, "rec_event", 0, 7), INVALID, "recorder selector out of range"),
    ("cfg2", lambda st, k, c: _set(st, k, "hist_offset", 5, c.total_bins), INVALID,
     "histogram bins out of range of total_bins"),
]

# The cases of BROKEN_TABLES (by message) that pvt_scene_lean_check cannot refuse as pvt_scene_create does.  Only three
# kinds of reason count: the refusal is one of create_scene's own guards (pvt_scene_lean_check has its own, which answers
# "bad argument"), it depends on the level of the entry (pvt_scene_lean_check works at the newest level, which knows the
# truncated cone and the `detected` selector), or it sits in a struct pvt_scene_lean_check does not take (the capture,
# absorb and pattern structs: their cases are in tests/test_gpu_ray_capture.py, test_gpu_absorbing_coatings.py and
# test_gpu_coating_patterns.py and never were in these lists).  tests/test_table_refusals.py runs every other case.
LEAN_CHECK_CANNOT = {
    "scene has no nodes": "create_scene's own guard on the node count; pvt_scene_lean_check's guard answers 'bad argument'",
    "more than 128 geometry nodes": "create_scene's own guard on the node count; pvt_scene_lean_check's guard answers "
                                    "'bad argument' with PVT_ERR_INVALID",
    "more than 256 recorders": "create_scene's own guard on the recorder count; pvt_scene_lean_check's guard answers "
                               "'bad argument'",
    "unknown geometry type": "the entry's level: geometry type 4 is PVT_GEOM_FRUSTUM, which pvt_scene_lean_check's level knows",
    "recorder selector out of range": "the entry's level: selector 7 is PVT_RECX_DETECTED, which pvt_scene_lean_check's "
                                      "level knows",
}


# -- refractive-index tables (PvtIndexTables; tests/test_gpu_dispersion.py) ----------------------------------------------
def index_scene():
    from pvtrace_amd import RefractiveIndexTable
    from tests import dispersion_scene as D

    return D.block_scene(RefractiveIndexTable(D.BLOCK_WAVELENGTH, D.BLOCK_VALUE))


def index_tables(compiled, edit):
    """PvtIndexTables over copies of the compiled scene's index tables, after `edit(struct, arrays)` -> (struct, arrays)."""
    arrays = {"node_table": compiled.ri_table.copy(), "table_n": compiled.rtab_n.copy(),
              "table_start": compiled.rtab_start.copy(), "wavelength": compiled.rtab_wavelength.copy(),
              "value": compiled.rtab_value.copy()}
    xt = native.PvtIndexTables()
    xt.n_tables, xt.n_points = int(compiled.n_ri_tables), int(compiled.rtab_wavelength.size)
    edit(xt, arrays)
    for name, arr in arrays.items():
        setattr(xt, name, native.np_ptr(arr) if arr is not None else None)
    return xt, arrays


def index_edit(**kw):
    def edit(xt, arrays):
        for key, value in kw.items():
            if key in arrays:
                if callable(value):
                    value(arrays[key])
                else:
                    arrays[key] = value
            else:
                setattr(xt, key, value)
    return edit


def _put(i, v):
    def f(a):
        a[i] = v
    return f


INDEX_BREAKS = {   # what is broken: (the edit, a part of pvt_last_error); the return code is INVALID
    "missing node_table": (index_edit(node_table=None), "index tables: missing arrays"),
    "missing value": (index_edit(value=None), "index tables: missing arrays"),
    "negative count": (index_edit(n_tables=-1), "index tables: missing arrays"),
    "node table too large": (index_edit(node_table=_put(1, 1)), "index tables: node names a missing table"),
    "node table below -1": (index_edit(node_table=_put(0, -2)), "index tables: node names a missing table"),
    "empty table": (index_edit(table_n=_put(0, 0)), "index tables: point range out of bounds"),
    "negative start": (index_edit(table_start=_put(0, -1)), "index tables: point range out of bounds"),
    "past the pools": (index_edit(n_points=2), "index tables: point range out of bounds"),
    "wavelengths not increasing": (index_edit(wavelength=_put(1, 400.0)), "index tables: wavelengths must be finite and strictly increasing"),
    "wavelength not finite": (index_edit(wavelength=_put(2, np.nan)), "index tables: wavelengths must be finite and strictly increasing"),
    "value zero": (index_edit(value=_put(0, 0.0)), "index tables: values must be finite and positive"),
    "value negative": (index_edit(value=_put(1, -1.5)), "index tables: values must be finite and positive"),
    "value infinite": (index_edit(value=_put(2, np.inf)), "index tables: values must be finite and positive"),
    "value huge": (index_edit(value=_put(2, 1e101)), "index tables: values must be finite and positive"),
}


# -- rough interfaces (PvtSurfaceTables; tests/test_gpu_rough_surfaces.py) -----------------------------------------------
BAD_ROUGHNESS = (-0.1, 1.5, float("nan"))   # the second node's GGX width: every one of them is refused


def rough_scene():
    from tests.test_rough_surfaces import rough_block_scene

    return rough_block_scene(0.2)


def surface_tables(second):
    """PvtSurfaceTables of a scene of two nodes: a smooth root and a node of GGX width `second` -> (struct, array)."""
    alpha = np.array([0.0, second])
    rt = native.PvtSurfaceTables()
    rt.n_nodes = 2
    rt.node_roughness = native.np_ptr(alpha)
    return rt, alpha


# -- concentration fields (PvtFieldTables; tests/test_gpu_concentration_fields.py) ---------------------------------------
FIELD_LO, FIELD_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def field_scene():
    """An index-matched 2 cm cube of two absorbers on one 1 x 1 x 2 lattice, in an n = 1 world."""
    from pvtrace_amd import Absorber, Box, ConcentrationGrid, Material, Node, Scene, Surface
    from pvtrace_amd.material import NullSurfaceDelegate

    grid = ConcentrationGrid(np.ones((1, 1, 2)), FIELD_LO, FIELD_HI)
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    Node(name="block", parent=world, geometry=Box((2.0, 2.0, 2.0), material=Material(
        refractive_index=1.0, surface=Surface(NullSurfaceDelegate()),
        components=[Absorber(1.0, concentration=grid), Absorber(0.5, concentration=grid)])))
    return Scene(world)


def field_tables(**change):
    """PvtFieldTables of field_scene() written out by hand, with the arrays of `change` replaced -> (struct, arrays)."""
    tabs = {"node_field": np.array([-1, 0], np.int32), "field_shape": np.array([[1, 1, 2]], np.int32),
            "field_lower": np.array([FIELD_LO], float), "field_upper": np.array([FIELD_HI], float),
            "comp_values": np.array([0, 0], np.int32), "values_start": np.array([0], np.int32),
            "values_count": np.array([2], np.int32), "values": np.array([1.0, 2.0])}
    tabs.update(change)
    ft = native.PvtFieldTables()
    ft.n_nodes, ft.n_fields = 2, 1
    ft.n_components, ft.n_values, ft.n_points = 2, 1, int(tabs["values"].size)
    held = {name: np.ascontiguousarray(tabs[name]) for name in (
        "node_field", "field_shape", "field_lower", "field_upper", "comp_values", "values_start", "values_count", "values")}
    for name, value in held.items():
        setattr(ft, name, native.np_ptr(value))
    return ft, held


FIELD_BREAKS = {   # every one is refused with a message of its own that names "field tables"
    "nan": dict(values=np.array([1.0, np.nan])),
    "negative": dict(values=np.array([1.0, -2.0])),
    "shape": dict(field_shape=np.array([[1, 0, 2]], np.int32)),
    "bounds": dict(field_upper=np.array([[1.0, -1.0, 1.0]])),
    "infinite bounds": dict(field_lower=np.array([[-np.inf, -1.0, -1.0]])),
    "lattice index": dict(node_field=np.array([-1, 3], np.int32)),
    "value index": dict(comp_values=np.array([0, 5], np.int32)),
    "no values": dict(comp_values=np.array([0, -1], np.int32)),
    "size": dict(values_count=np.array([1], np.int32)),
    "root": dict(node_field=np.array([0, 0], np.int32)),
    "run": dict(values_start=np.array([1], np.int32)),
}


# -- volume maps (PvtMapTables; tests/test_gpu_volume_maps.py) -----------------------------------------------------------
def map_scene():
    """An index-matched 2 cm cube of two absorbers in an n = 1 world."""
    from pvtrace_amd import Absorber, Box, Material, Node, Scene, Surface
    from pvtrace_amd.material import NullSurfaceDelegate

    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    Node(name="block", parent=world, geometry=Box((2.0, 2.0, 2.0), material=Material(
        refractive_index=1.0, surface=Surface(NullSurfaceDelegate()),
        components=[Absorber(1.0, name="a"), Absorber(0.5, name="b")])))
    return Scene(world)


MAP_SLOTS = 22   # of the two maps map_tables() describes


def map_tables(n_nodes=2, **change):
    """PvtMapTables of two maps on the block of map_scene(), with the fields of `change` replaced -> (struct, arrays)."""
    tabs = {"node_map_start": np.array([0, 0], np.int32), "node_map_count": np.array([0, 2], np.int32),
            "map_kind": np.array([3, 4], np.int32), "map_component": np.array([-1, 1], np.int32),
            "map_shape": np.array([[2, 2, 2], [1, 1, 3]], np.int32), "map_lower": np.array([[-1.0] * 3] * 2),
            "map_h": np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 0.5]]), "map_nw": np.array([0, 4], np.int32),
            "map_wl_start": np.array([0.0, 400.0]), "map_wl_stop": np.array([1.0, 800.0]),
            "map_offset": np.array([0, 9], np.int64), "map_slots": MAP_SLOTS}
    tabs.update(change)
    mt = native.PvtMapTables()
    mt.n_nodes, mt.n_maps, mt.map_slots = n_nodes, 2, int(tabs.pop("map_slots"))
    held = {k: np.ascontiguousarray(v) for k, v in tabs.items()}
    for name, value in held.items():
        setattr(mt, name, native.np_ptr(value))
    return mt, held


MAP_BREAKS = {   # every one is refused with a message of its own that names "map tables"
    "nodes": dict(n_nodes=3),
    "run": dict(node_map_count=np.array([0, 5], np.int32)),
    "tiling": dict(node_map_start=np.array([0, 1], np.int32), node_map_count=np.array([0, 1], np.int32)),
    "root": dict(node_map_start=np.array([0, 1], np.int32), node_map_count=np.array([1, 1], np.int32)),
    "kind": dict(map_kind=np.array([3, 2], np.int32)),
    "component": dict(map_component=np.array([-1, 7], np.int32)),
    "shape": dict(map_shape=np.array([[2, 0, 2], [1, 1, 3]], np.int32)),
    "lower": dict(map_lower=np.array([[-1.0, np.nan, -1.0], [-1.0] * 3])),
    "width": dict(map_h=np.array([[1.0, 1.0, 0.0], [2.0, 2.0, 0.5]])),
    "bins": dict(map_nw=np.array([0, -1], np.int32)),
    "infinite range": dict(map_wl_stop=np.array([1.0, np.inf])),
    "range": dict(map_wl_stop=np.array([1.0, 400.0])),
    "offset": dict(map_offset=np.array([0, 8], np.int64)),
    "total": dict(map_slots=23),
    "limit": dict(map_shape=np.array([[2, 2, 2], [4096, 4096, 8]], np.int32)),
}
