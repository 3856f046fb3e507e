"""Flatten a Scene into structure-of-arrays tables for the HIP tracer.

`CompiledScene` carries, field for field, what the reference's lowering
produces (pvtrace/engine/compiler.py:57-204: geometry / transform / material /
component / pooled-spectra / recorder / histogram tables, same dtypes, same
node order = pre-order over nodes that have a geometry, same error cases) so it
can be handed unchanged to the reference kernel — that is how the golden
fixtures are made — plus one extension the reference engine lacks: a per-node
table of declarative surface coatings (`coat_*`), which is what lets `LSC()`
(whose delegate the reference compiler rejects, compiler.py:237-247) and the
Coatings-notebook scene run on the device.

Everything here is host-side numpy executed once per `simulate` call; the
tables (a few KB) are packed and uploaded to HBM once by `native.DeviceScene`.
"""
import math
import numbers

import numpy as np

from pvtrace_amd.engine import native
from pvtrace_amd.engine.recorder import (
    ALL_EVENTS,
    EXTENSION_PROPERTIES,
    HISTOGRAM_PROPERTIES,
    MAP_EVENTS,
    MAX_CAPTURE_ROWS,
    MAX_MAP_SLOTS,
    ORIGIN_PROPERTIES,
    SOURCE_COMPONENT,
    SOURCE_COMPONENTS,
    SOURCE_LIGHTS,
    VOLUME_EVENTS,
    Heatmap,
    Recorder,
    VolumeMap,
)
from pvtrace_amd.geometry import Box, Conicoid, Cylinder, Frustum, Mesh, Polyhedron, Sphere, _polyhedron_analysis
from pvtrace_amd.material import (
    Absorber,
    Alignment,
    CoatedSurfaceDelegate,
    Coating,
    CoatingPattern,
    ConcentrationGrid,
    Cone,
    FresnelSurfaceDelegate,
    HenyeyGreenstein,
    Luminophore,
    NullSurfaceDelegate,
    PhaseFunctionTable,
    Reactor,
    ReflectivityTable,
    RefractiveIndexTable,
    ScatterLobe,
    Scatterer,
    isotropic,
)

MAX_NODES = 128       # device limit (reference _kernel.pyx:66, :929-930)
MAX_RECORDERS = 256   # per-photon distinct-ray bitmask width (compiler.py:23)
MAX_PATTERN_CELLS = 1 << 26   # cells of all coating patterns of a scene: 64 MiB of bytes, the order of MAX_MAP_SLOTS

GEOM_BOX, GEOM_SPHERE, GEOM_CYLINDER, GEOM_MESH = 0, 1, 2, 3
GEOM_FRUSTUM = 4   # EXTENSION: truncated cone (include/pvtrace_hip.h: PVT_GEOM_FRUSTUM)
GEOM_POLYHEDRON = 5   # EXTENSION: convex polyhedron, a table of planes (include/pvtrace_hip.h: PVT_GEOM_POLYHEDRON)
GEOM_CONICOID = 6   # EXTENSION: solid of revolution of a conic (include/pvtrace_hip.h: PVT_GEOM_CONICOID)
SURF_FRESNEL, SURF_NULL = 0, 1
COMP_ABSORBER, COMP_SCATTERER, COMP_LUMINOPHORE, COMP_REACTOR = 0, 1, 2, 3
PHASE_ISOTROPIC, PHASE_HENYEY_GREENSTEIN, PHASE_CONE = 0, 1, 2
PHASE_LAMBERTIAN = 3   # extension: the reference compiler rejects it (compiler.py:300-310); cli/parse.py:166-167 builds it
PHASE_TABLE = 4        # extension: a PhaseFunctionTable, sampled about the incoming direction (comp_phase_table)
COAT_LOBE = 16         # extension: a coat_reflect_mode / coat_transmit_mode word >= 16 is a ScatterLobe, COAT_LOBE + 4 table + axis
                       # (include/pvtrace_hip.h: PVT_COAT_LOBE); axis 0 normal, 1 specular, 2 refracted, 3 straight
EMIT_KT, EMIT_REDSHIFT, EMIT_FULL = 0, 1, 2
EMIT_METHODS = {"kT": EMIT_KT, "redshift": EMIT_REDSHIFT, "full": EMIT_FULL}

_F64 = np.float64
_I32 = np.int32


class UnsupportedSceneError(Exception):
    """The scene uses something the device engine cannot lower to tables."""


def _phase_of(node, component):
    """(tag, parameter) for a component's phase function."""
    import functools

    from pvtrace_amd import material as M

    phase = component.phase_function
    if phase is isotropic:
        return PHASE_ISOTROPIC, 0.0
    if isinstance(phase, HenyeyGreenstein):
        return PHASE_HENYEY_GREENSTEIN, float(phase.g)
    if isinstance(phase, Cone):
        return PHASE_CONE, float(phase.theta_max)
    if phase is M.lambertian:   # (reference material/utils.py:176-186; what `phase-function: {lambertian:}` parses to)
        return PHASE_LAMBERTIAN, 0.0
    if isinstance(phase, PhaseFunctionTable):   # (the table itself is pooled by _lower_component)
        return PHASE_TABLE, 0.0
    # functools.partial spellings of the same built-ins (not recognised by the
    # reference compiler, which raises for them)
    if isinstance(phase, functools.partial) and not phase.keywords:
        if phase.func is M.cone and len(phase.args) == 1:
            return PHASE_CONE, float(phase.args[0])
        if phase.func is M.henyey_greenstein and len(phase.args) == 1:
            return PHASE_HENYEY_GREENSTEIN, float(phase.args[0])
    raise UnsupportedSceneError(
        f"Node {node.name!r}: custom phase functions are not supported."
    )


class CompiledScene:
    """SoA tables describing `scene` (see module docstring)."""

    def __init__(self, scene):
        root = scene.root
        if root is None:
            raise UnsupportedSceneError("Scene has no geometry nodes.")
        nodes = [n for n in root.preorder() if n.geometry is not None]
        if not nodes:
            raise UnsupportedSceneError("Scene has no geometry nodes.")
        if root.geometry is None:
            raise UnsupportedSceneError("Root node must have a geometry.")

        count = len(nodes)
        self.scene = scene
        self.nodes = nodes
        self.node_names = [n.name for n in nodes]
        self.root_id = nodes.index(root)

        self.geom_type = np.zeros(count, dtype=_I32)
        self.geom_params = np.zeros((count, 4), dtype=_F64)
        self.local_to_world = np.zeros((count, 4, 4), dtype=_F64)
        self.world_to_local = np.zeros((count, 4, 4), dtype=_F64)
        self.refractive_index = np.zeros(count, dtype=_F64)
        self.surface_type = np.zeros(count, dtype=_I32)
        self.comp_start = np.zeros(count, dtype=_I32)
        self.comp_count = np.zeros(count, dtype=_I32)
        self.coat_start = np.zeros(count, dtype=_I32)
        self.coat_count = np.zeros(count, dtype=_I32)
        # GGX width alpha of each node's surface (FresnelSurfaceDelegate / CoatedSurfaceDelegate `roughness`): all zeros
        # unless some node is rough, and then passed to the library as PvtSurfaceTables
        self.surface_roughness = np.zeros(count, dtype=_F64)
        # Refractive-index tables n(wavelength) of the dispersive nodes (ri_table: -1 = the scalar index), pooled like
        # the coating tables: per table its length and where its wavelengths and values start in the pools.  The
        # scalar column of a dispersive node holds n at the table's first wavelength.
        self.ri_table = np.full(count, -1, dtype=_I32)
        rtab = {"index": {}, "n": [], "start": [], "wavelength": [], "value": []}
        # Phase-function tables of the components (comp_phase_table: -1 = a built-in phase function), pooled by
        # identity: per table its rows (wavelengths) and mu points, and where its wavelengths, mu axis and CDF rows
        # (row-major, n_wavelength x n_mu) start in the pools.
        self._ptab = {"index": {}, "nw": [], "nmu": [], "wl_start": [], "mu_start": [], "cdf_start": [],
                      "wavelength": [], "mu": [], "cdf": []}
        # Concentration fields (ConcentrationGrid): one lattice per node (node_field: -1 = none) with its shape and
        # bounds, and per component the value table it reads (comp_values: -1 = none), pooled by identity; a component
        # without a field in a node with one reads a table of ones of the lattice's size (pooled by shape).
        self.node_field = np.full(count, -1, dtype=_I32)
        fields = {"shape": [], "lower": [], "upper": [], "index": {}, "comp": [], "start": [], "count": [], "values": []}
        self.mesh_face_start = np.zeros(count, dtype=_I32)
        self.mesh_face_count = np.zeros(count, dtype=_I32)
        self._mesh_pool = {"vertices": [], "faces": [], "normals": [], "nv": 0, "nf": 0}
        # Convex polyhedra (Polyhedron): per node where its plane rows (nx, ny, nz, h) start in the pool and how many they
        # are (0: the node is no polyhedron).  Passed to the library as PvtPolyhedronTables, only by scenes that hold one.
        self.poly_start = np.zeros(count, dtype=_I32)
        self.poly_count = np.zeros(count, dtype=_I32)
        self._poly_pool = []

        pools = {"abs_x": [], "abs_y": [], "ems_x": [], "ems_cdf": []}
        comp_cols = {
            key: []
            for key in (
                "type", "qy", "tau_rad", "tau_nr", "phase_type", "phase_param", "phase_table",
                "abs_start", "abs_n", "ems_start", "ems_n", "abs_hist", "ems_hist",
            )
        }
        coat_rows = []
        self.component_names = []
        # Aligned components (Alignment): comp_align names a component's alignment record (-1: none); a record holds the
        # director in the ROOT's frame (align_axis, a unit vector), the absorption order and the single-row phase table of
        # f(mu; S_e) the emission samples about that axis (align_emit_table: its id among the phase tables, -1 = S_e is 0).
        # One record per (Alignment object, node).  Passed to the library as PvtAlignTables, only by scenes that use them.
        align = {"index": {}, "comp": [], "axis": [], "abs_order": [], "emit_table": []}

        for i, node in enumerate(nodes):
            geometry = node.geometry
            self._lower_geometry(i, geometry)
            self._lower_transform(i, node, root)

            material = geometry.material
            if material is None:
                raise UnsupportedSceneError(
                    f"Node {node.name!r} has geometry without a material."
                )
            self.ri_table[i] = self._lower_refractive_index(i, node, material.refractive_index, rtab)

            self.coat_start[i] = len(coat_rows)
            self.surface_type[i] = self._lower_surface(node, material, coat_rows)
            self.surface_roughness[i] = self._surface_roughness(node, material)
            self.coat_count[i] = len(coat_rows) - self.coat_start[i]

            self.comp_start[i] = len(comp_cols["type"])
            self._check_alignment(node, material, node is root)
            for component in material.components:
                self._lower_component(node, component, comp_cols, pools)
                self.component_names.append(component.name)
                align["comp"].append(self._lower_alignment(i, node, component, comp_cols, align))
            self.comp_count[i] = len(material.components)
            self.node_field[i] = self._lower_fields(node, material, node is root, fields)

        self.comp_align = np.array(align["comp"], dtype=_I32)
        self.n_align = len(align["abs_order"])
        self.align_axis = np.array(align["axis"], dtype=_F64).reshape(-1, 3)
        self.align_abs_order = np.array(align["abs_order"], dtype=_F64)
        self.align_emit_table = np.array(align["emit_table"], dtype=_I32)

        self.n_fields = len(fields["shape"])
        self.field_shape = np.array(fields["shape"], dtype=_I32).reshape(-1, 3)
        self.field_lower = np.array(fields["lower"], dtype=_F64).reshape(-1, 3)
        self.field_upper = np.array(fields["upper"], dtype=_F64).reshape(-1, 3)
        self.comp_values = np.array(fields["comp"], dtype=_I32)
        self.n_value_tables = len(fields["start"])
        self.values_start = np.array(fields["start"], dtype=_I32)
        self.values_count = np.array(fields["count"], dtype=_I32)
        self.field_values = (np.concatenate(fields["values"]) if fields["values"] else np.zeros(0, dtype=_F64))

        self.n_ri_tables = len(rtab["n"])
        self.rtab_n = np.array(rtab["n"], dtype=_I32)
        self.rtab_start = np.array(rtab["start"], dtype=_I32)
        self.rtab_wavelength = np.array(rtab["wavelength"], dtype=_F64)
        self.rtab_value = np.array(rtab["value"], dtype=_F64)

        self.comp_type = np.array(comp_cols["type"], dtype=_I32)
        self.comp_qy = np.array(comp_cols["qy"], dtype=_F64)
        self.comp_tau_rad = np.array(comp_cols["tau_rad"], dtype=_F64)
        self.comp_tau_nr = np.array(comp_cols["tau_nr"], dtype=_F64)
        self.comp_phase_type = np.array(comp_cols["phase_type"], dtype=_I32)
        self.comp_phase_param = np.array(comp_cols["phase_param"], dtype=_F64)
        self.comp_phase_table = np.array(comp_cols["phase_table"], dtype=_I32)
        # Scattering coatings (Coating(reflection=ScatterLobe(...)) / transmission=): their tables join the phase pool
        # behind the components', one entry per table object however many lobes or coatings share it, and the row's mode
        # word names table and axis (COAT_LOBE).  A scene without a lobe pools nothing and keeps the words 0 / 1.
        coat_modes = [(self._lower_coat_mode(r, coating.reflection, Coating.REFLECTION_MODES, ScatterLobe.REFLECTION_ABOUT, "reflection"),
                       self._lower_coat_mode(r, coating.transmission, Coating.TRANSMISSION_MODES, ScatterLobe.TRANSMISSION_ABOUT, "transmission"))
                      for r, coating in enumerate(coat_rows)]
        ptab = self._ptab
        self.n_phase_tables = len(ptab["nw"])
        self.ptab_nw = np.array(ptab["nw"], dtype=_I32)
        self.ptab_nmu = np.array(ptab["nmu"], dtype=_I32)
        self.ptab_wl_start = np.array(ptab["wl_start"], dtype=_I32)
        self.ptab_mu_start = np.array(ptab["mu_start"], dtype=_I32)
        self.ptab_cdf_start = np.array(ptab["cdf_start"], dtype=_I32)
        self.ptab_wavelength = np.array(ptab["wavelength"], dtype=_F64)
        self.ptab_mu = np.array(ptab["mu"], dtype=_F64)
        self.ptab_cdf = np.array(ptab["cdf"], dtype=_F64)
        del self._ptab
        self.comp_abs_start = np.array(comp_cols["abs_start"], dtype=_I32)
        self.comp_abs_n = np.array(comp_cols["abs_n"], dtype=_I32)
        self.comp_ems_start = np.array(comp_cols["ems_start"], dtype=_I32)
        self.comp_ems_n = np.array(comp_cols["ems_n"], dtype=_I32)
        self.comp_abs_hist = np.array(comp_cols["abs_hist"], dtype=_I32)
        self.comp_ems_hist = np.array(comp_cols["ems_hist"], dtype=_I32)

        self.abs_x = np.array(pools["abs_x"], dtype=_F64)
        self.abs_y = np.array(pools["abs_y"], dtype=_F64)
        self.ems_x = np.array(pools["ems_x"], dtype=_F64)
        self.ems_cdf = np.array(pools["ems_cdf"], dtype=_F64)

        # Coating table: one row per Coating, grouped per node.
        ncoat = len(coat_rows)
        self.coat_facet = np.zeros((max(ncoat, 1), 3), dtype=_F64)
        self.coat_lo = np.full((max(ncoat, 1), 3), -np.inf, dtype=_F64)
        self.coat_hi = np.full((max(ncoat, 1), 3), np.inf, dtype=_F64)
        self.coat_reflectivity = np.full(ncoat, -1.0, dtype=_F64)
        self.coat_reflect_mode = np.zeros(ncoat, dtype=_I32)
        self.coat_transmit_mode = np.zeros(ncoat, dtype=_I32)
        # Reflectivity tables R(wavelength, angle) of the coatings that have one (coat_table: -1 = none), pooled like
        # the spectra: per table its axis lengths and where its wavelengths, angles (degrees) and values (row-major,
        # n_angle x n_wavelength) start in the pools.  A table shared by several coatings is pooled once.
        self.coat_table = np.full(ncoat, -1, dtype=_I32)
        ctab = {"index": {}, "nw": [], "na": [], "wl_start": [], "angle_start": [], "value_start": [],
                "wavelength": [], "angle": [], "value": []}
        # Absorptivity A(wavelength, angle) of the coatings (Coating(absorptivity=...)): a scalar per coating (0: none) and
        # the table of those that have one (coat_abs_table: -1 = the scalar), pooled in `atab_*` pools of their own, laid
        # out like `ctab_*`.  All zeros / empty unless some coating has an absorptivity, and then passed to the library as
        # PvtCoatingAbsorbTables.
        self.coat_absorptivity = np.zeros(ncoat, dtype=_F64)
        self.coat_abs_table = np.full(ncoat, -1, dtype=_I32)
        atab = {"index": {}, "nw": [], "na": [], "wl_start": [], "angle_start": [], "value_start": [],
                "wavelength": [], "angle": [], "value": []}
        self.has_absorbing_coatings = False
        # Where a coating covers (Coating(pattern=..., facet=None)): coat_any_facet flags the rows whose normal test is
        # skipped (a flag of the row, its coat_facet stays zero and is ignored); coat_pattern names the row's mask lattice
        # (-1: none) in the `cpat_*` tables -- per pattern its shape, which axes are bounded, lower and cell widths (0 on an
        # unbounded axis) and where its uint8 mask starts in the pool `cpat_mask`.  One CoatingPattern object shared by
        # several coatings is stored once.  Passed to the library as PvtCoatingPatternTables, only by scenes that use them.
        self.coat_any_facet = np.zeros(ncoat, dtype=_I32)
        self.coat_pattern = np.full(ncoat, -1, dtype=_I32)
        cpat = {"index": {}, "shape": [], "bounded": [], "lower": [], "h": [], "start": [], "mask": [], "cells": 0}
        for r, coating in enumerate(coat_rows):
            self.coat_pattern[r] = self._pool_coating_pattern(r, getattr(coating, "pattern", None), cpat)
            if coating.facet is None:
                self.coat_any_facet[r] = 1
            absorptivity = getattr(coating, "absorptivity", None)
            if absorptivity is not None:
                self.has_absorbing_coatings = True
                if isinstance(absorptivity, ReflectivityTable):
                    self.coat_abs_table[r] = self._pool_coating_table(absorptivity, atab)
                else:
                    a = float(absorptivity)   # (assigned after construction, perhaps: checked again)
                    if not 0.0 <= a <= 1.0:
                        raise UnsupportedSceneError(f"Coating {r}: absorptivity must be in [0, 1], got {absorptivity!r}.")
                    self.coat_absorptivity[r] = a
            if coating.facet is not None:
                self.coat_facet[r] = coating.facet
            self.coat_lo[r] = [b[0] for b in coating.region]
            self.coat_hi[r] = [b[1] for b in coating.region]
            if isinstance(coating.reflectivity, ReflectivityTable):
                self.coat_table[r] = self._pool_coating_table(coating.reflectivity, ctab)
            elif coating.reflectivity is not None:
                self.coat_reflectivity[r] = coating.reflectivity
            self.coat_reflect_mode[r], self.coat_transmit_mode[r] = coat_modes[r]
        self.n_coatings = ncoat
        self.n_coat_tables = len(ctab["nw"])
        for key in ("nw", "na", "wl_start", "angle_start", "value_start"):
            setattr(self, f"ctab_{key}", np.array(ctab[key], dtype=_I32))
        for key in ("wavelength", "angle", "value"):
            setattr(self, f"ctab_{key}", np.array(ctab[key], dtype=_F64))
        self.n_abs_tables = len(atab["nw"])
        for key in ("nw", "na", "wl_start", "angle_start", "value_start"):
            setattr(self, f"atab_{key}", np.array(atab[key], dtype=_I32))
        for key in ("wavelength", "angle", "value"):
            setattr(self, f"atab_{key}", np.array(atab[key], dtype=_F64))

        self.n_coat_patterns = len(cpat["start"])
        self.cpat_shape = np.array(cpat["shape"], dtype=_I32).reshape(-1, 3)
        self.cpat_bounded = np.array(cpat["bounded"], dtype=_I32).reshape(-1, 3)
        self.cpat_lower = np.array(cpat["lower"], dtype=_F64).reshape(-1, 3)
        self.cpat_h = np.array(cpat["h"], dtype=_F64).reshape(-1, 3)
        self.cpat_start = np.array(cpat["start"], dtype=np.int64)
        self.cpat_mask = (cpat["mask"][0] if len(cpat["mask"]) == 1 else
                          np.concatenate(cpat["mask"]) if cpat["mask"] else np.zeros(0, dtype=np.uint8))

        pool = self._mesh_pool
        self.n_mesh_vertices, self.n_mesh_faces = pool["nv"], pool["nf"]
        self.mesh_vertices = (np.concatenate(pool["vertices"]) if pool["nv"] else np.zeros((0, 3), dtype=_F64))
        self.mesh_faces = (np.concatenate(pool["faces"]).astype(_I32) if pool["nf"] else np.zeros((0, 3), dtype=_I32))
        self.mesh_normals = (np.concatenate(pool["normals"]) if pool["nf"] else np.zeros((0, 3), dtype=_F64))
        del self._mesh_pool
        self.poly_planes = (np.ascontiguousarray(np.concatenate(self._poly_pool), dtype=_F64) if self._poly_pool
                            else np.zeros((0, 4), dtype=_F64))
        del self._poly_pool

        self._lower_recorders(nodes)
        self._lower_maps(root, nodes)

    # -- geometry & pose -------------------------------------------------
    def _lower_geometry(self, i, geometry):
        if isinstance(geometry, Box):
            self.geom_type[i] = GEOM_BOX
            self.geom_params[i, :3] = np.asarray(geometry._size, dtype=_F64)
        elif isinstance(geometry, Sphere):
            self.geom_type[i] = GEOM_SPHERE
            self.geom_params[i, 0] = float(geometry.radius)
        elif isinstance(geometry, Cylinder):
            self.geom_type[i] = GEOM_CYLINDER
            self.geom_params[i, 0] = float(geometry.length)
            self.geom_params[i, 1] = float(geometry.radius)
        elif isinstance(geometry, Frustum):
            # EXTENSION: the reference has no truncated cone; (length, radius_bottom, radius_top), checked again here
            # because the attributes may have been changed since construction
            problem = Frustum.parameter_problem(geometry.length, geometry.radius_bottom, geometry.radius_top)
            if problem:
                raise UnsupportedSceneError(problem)
            self.geom_type[i] = GEOM_FRUSTUM
            self.geom_params[i, 0] = float(geometry.length)
            self.geom_params[i, 1] = float(geometry.radius_bottom)
            self.geom_params[i, 2] = float(geometry.radius_top)
        elif isinstance(geometry, Conicoid):
            # EXTENSION: the reference has no such solid; (length, p0, p1, p2), checked again here because the attributes
            # may have been changed since construction
            problem = Conicoid.parameter_problem(geometry.length, geometry.profile)
            if problem:
                raise UnsupportedSceneError(problem)
            self.geom_type[i] = GEOM_CONICOID
            self.geom_params[i, 0] = float(geometry.length)
            self.geom_params[i, 1:4] = [float(v) for v in geometry.profile]
        elif isinstance(geometry, Polyhedron):
            # EXTENSION: the reference has no convex polyhedron; the stored rows are the shape, checked again here because
            # the attributes may have been changed since construction
            problem, rows, vertices, _, _ = _polyhedron_analysis(geometry.planes)
            if problem is None and np.any(np.abs(np.sqrt(np.sum(rows[:, :3] ** 2, axis=1)) - 1.0) > 1e-12):
                problem = "Polyhedron plane normals must be unit vectors."
            if problem:
                raise UnsupportedSceneError(problem)
            self.geom_type[i] = GEOM_POLYHEDRON
            self.geom_params[i, 0] = float(np.max(np.sqrt(np.sum(vertices * vertices, axis=1))))   # bounding radius
            self.poly_start[i] = sum(len(rows) for rows in self._poly_pool)
            self.poly_count[i] = len(rows)
            self._poly_pool.append(rows)
        elif isinstance(geometry, Mesh):
            # EXTENSION: the reference engine rejects meshes (compiler.py:220-223)
            pool = self._mesh_pool
            self.geom_type[i] = GEOM_MESH
            self.mesh_face_start[i] = pool["nf"]
            self.mesh_face_count[i] = len(geometry.faces)
            pool["vertices"].append(np.asarray(geometry.vertices, dtype=_F64))
            pool["faces"].append(np.asarray(geometry.faces, dtype=_I32) + pool["nv"])
            pool["normals"].append(np.asarray(geometry.face_normals, dtype=_F64))
            pool["nv"] += len(geometry.vertices)
            pool["nf"] += len(geometry.faces)
            lo, hi = geometry.vertices.min(axis=0), geometry.vertices.max(axis=0)
            self.geom_params[i, :3] = hi - lo          # informational: local AABB size
        else:
            raise UnsupportedSceneError(
                f"Geometry type {type(geometry).__name__} is not supported."
            )

    def _lower_transform(self, i, node, root):
        l2w = np.asarray(node.transformation_to(root), dtype=_F64)
        rot = l2w[:3, :3]
        if not np.allclose(rot @ rot.T, np.eye(3), atol=1e-9):
            raise UnsupportedSceneError(
                f"Node {node.name!r} transform is not rigid (has scale or shear)."
            )
        self.local_to_world[i] = l2w
        self.world_to_local[i] = np.linalg.inv(l2w)

    # -- surfaces --------------------------------------------------------
    def _lower_surface(self, node, material, coat_rows):
        delegate = material.surface.delegate
        if type(delegate) is FresnelSurfaceDelegate:
            return SURF_FRESNEL
        if type(delegate) is NullSurfaceDelegate:
            return SURF_NULL
        if isinstance(delegate, CoatedSurfaceDelegate):
            # `coatings` may be computed lazily from mutable state (the LSC
            # builder's delegates do that), so read it at flatten time.
            for coating in delegate.coatings:
                if not isinstance(coating, Coating):
                    raise UnsupportedSceneError(
                        f"Node {node.name!r}: coatings must be Coating objects."
                    )
                coat_rows.append(coating)
            return SURF_FRESNEL
        raise UnsupportedSceneError(
            f"Node {node.name!r} uses surface delegate "
            f"{type(delegate).__name__}; only FresnelSurfaceDelegate, "
            "NullSurfaceDelegate and CoatedSurfaceDelegate (declarative "
            "coatings) are supported."
        )

    @staticmethod
    def _pool_coating_pattern(row, pattern, cpat):
        """Id of a coating row's pattern in the `cpat_*` tables (-1: none), pooled by identity."""
        if pattern is None:
            return -1
        if not isinstance(pattern, CoatingPattern):
            raise UnsupportedSceneError(f"Coating {row}: pattern must be a CoatingPattern, got {type(pattern).__name__}.")
        if id(pattern) in cpat["index"]:
            return cpat["index"][id(pattern)][0]
        mask = np.ascontiguousarray(pattern.mask, dtype=np.uint8)
        if mask.ndim != 3 or min(mask.shape) < 1:
            raise UnsupportedSceneError(f"Coating {row}: the pattern's mask must have three axes of >= 1 cells, got {mask.shape}.")
        lower, h = [], []
        for a in range(3):   # (assigned after construction, perhaps: checked again)
            if not pattern.bounded[a]:
                if mask.shape[a] != 1:
                    raise UnsupportedSceneError(f"Coating {row}: pattern axis {a} is unbounded but has {mask.shape[a]} cells.")
                lower.append(0.0); h.append(0.0)
                continue
            lo, hi = float(pattern.lower[a]), float(pattern.upper[a])
            width = (hi - lo) / float(mask.shape[a])
            if not (math.isfinite(lo) and math.isfinite(hi) and math.isfinite(width) and width > 0.0):
                raise UnsupportedSceneError(
                    f"Coating {row}: pattern axis {a} needs finite bounds with lower < upper, got {pattern.lower[a]!r}, "
                    f"{pattern.upper[a]!r}.")
            lower.append(lo); h.append(width)
        if cpat["cells"] + mask.size > MAX_PATTERN_CELLS:
            raise UnsupportedSceneError(
                f"The scene's coating patterns hold more than {MAX_PATTERN_CELLS} cells (2^26), reached at coating {row}.")
        k = len(cpat["start"])
        cpat["index"][id(pattern)] = (k, pattern)   # (the object is kept: its id stays its own while the pool lives)
        cpat["shape"].append(list(mask.shape))
        cpat["bounded"].append([int(b) for b in pattern.bounded])
        cpat["lower"].append(lower)
        cpat["h"].append(h)
        cpat["start"].append(cpat["cells"])
        cpat["mask"].append(mask.reshape(-1))   # (bytes as they are: the kernel and the host both ask `!= 0`; no copy of a large mask)
        cpat["cells"] += mask.size
        return k

    @property
    def has_coating_patterns(self):
        """A coating with a pattern or with facet=None: the scene needs pvt_scene_create_pattern's tables."""
        return bool(np.any(self.coat_pattern >= 0) or np.any(self.coat_any_facet != 0))

    def _surface_roughness(self, node, material):
        delegate = material.surface.delegate
        if type(delegate) is NullSurfaceDelegate:
            return 0.0
        alpha = float(getattr(delegate, "roughness", 0.0))
        if not (math.isfinite(alpha) and 0.0 <= alpha <= 1.0):
            raise UnsupportedSceneError(f"Node {node.name!r}: surface roughness must satisfy 0 <= alpha <= 1, got {alpha!r}.")
        return alpha

    @property
    def has_frustum(self):
        return bool(np.any(self.geom_type == GEOM_FRUSTUM))

    @property
    def has_conicoid(self):
        return bool(np.any(self.geom_type == GEOM_CONICOID))

    @property
    def has_polyhedron(self):
        return bool(np.any(self.geom_type == GEOM_POLYHEDRON))

    @property
    def has_roughness(self):
        return bool(np.any(self.surface_roughness > 0.0))

    @staticmethod
    def _lower_fields(node, material, is_root, fields):
        components = list(material.components)
        grids = [getattr(c, "concentration", None) for c in components]
        present = [g for g in grids if g is not None]
        if not present:
            fields["comp"].extend([-1] * len(components))
            return -1
        if is_root:
            raise UnsupportedSceneError(
                f"Root node {node.name!r}: the scene's root cannot carry a concentration field (ConcentrationGrid).")
        lattice = present[0]
        for g in present[1:]:
            if not lattice.same_lattice(g):
                raise UnsupportedSceneError(
                    f"Node {node.name!r}: the concentration fields of one material must share their lattice (the same "
                    f"shape, lower and upper bit for bit); got {lattice.shape} {lattice.lower.tolist()}..{lattice.upper.tolist()} "
                    f"and {g.shape} {g.lower.tolist()}..{g.upper.tolist()}.")

        def pool(key, table):
            values = table.values if isinstance(table, ConcentrationGrid) else table
            if key not in fields["index"]:
                fields["index"][key] = (len(fields["start"]), table)   # (the grid itself keeps its id from being reused)
                if sum(fields["count"]) + values.size > 2 ** 31 - 1:
                    raise UnsupportedSceneError("The concentration fields hold more than 2^31 - 1 values.")
                fields["start"].append(sum(fields["count"]))
                fields["count"].append(int(values.size))
                fields["values"].append(np.ascontiguousarray(values, dtype=_F64).ravel())
            return fields["index"][key][0]

        for g in grids:
            if g is not None:
                fields["comp"].append(pool(("grid", id(g)), g))
            else:
                fields["comp"].append(pool(("ones", lattice.shape), np.ones(lattice.shape, dtype=_F64)))
        at = len(fields["shape"])
        fields["shape"].append(list(lattice.shape))
        fields["lower"].append(lattice.lower.tolist())
        fields["upper"].append(lattice.upper.tolist())
        return at

    @property
    def has_fields(self):
        return bool(np.any(self.node_field >= 0))

    def _lower_refractive_index(self, i, node, index, rtab):
        if isinstance(index, RefractiveIndexTable):
            key = id(index)
            if key not in rtab["index"]:
                rtab["index"][key] = (len(rtab["n"]), index)   # (the table itself keeps its id from being reused)
                rtab["n"].append(index.wavelength.size)
                rtab["start"].append(len(rtab["wavelength"]))
                rtab["wavelength"].extend(index.wavelength.tolist())
                rtab["value"].extend(index.values.tolist())
            self.refractive_index[i] = float(index.values[0])
            return rtab["index"][key][0]
        if not isinstance(index, numbers.Real):
            raise UnsupportedSceneError(
                f"Node {node.name!r}: refractive_index must be a number or a RefractiveIndexTable, "
                f"got {type(index).__name__}."
            )
        self.refractive_index[i] = float(index)
        return -1

    @staticmethod
    def _pool_coating_table(table, ctab):
        key = id(table)
        if key not in ctab["index"]:
            ctab["index"][key] = (len(ctab["nw"]), table)   # (the table itself keeps its id from being reused)
            ctab["nw"].append(table.wavelength.size)
            ctab["na"].append(table._angle_axis.size)
            ctab["wl_start"].append(len(ctab["wavelength"]))
            ctab["angle_start"].append(len(ctab["angle"]))
            ctab["value_start"].append(len(ctab["value"]))
            ctab["wavelength"].extend(table.wavelength.tolist())
            ctab["angle"].extend(table._angle_axis.tolist())
            ctab["value"].extend(table._grid.ravel().tolist())
        return ctab["index"][key][0]

    @staticmethod
    def _check_alignment(node, material, is_root):
        components = list(material.components)
        aligned = [c for c in components if getattr(c, "alignment", None) is not None]
        if not aligned:
            return
        if is_root:
            raise UnsupportedSceneError(
                f"Root node {node.name!r}: the scene's root cannot carry an aligned component (Alignment).")
        if any(getattr(c, "concentration", None) is not None for c in components):
            raise UnsupportedSceneError(
                f"Node {node.name!r}: alignment together with a concentration field (ConcentrationGrid) on a component of "
                "the same material is out of scope: the march would need the factors.")
        for c in aligned:
            a = c.alignment
            if not isinstance(a, Alignment):
                raise UnsupportedSceneError(f"Node {node.name!r}: alignment must be an Alignment, got {type(a).__name__}.")
            if a.emission_order != 0.0 and not isinstance(c, Luminophore):
                raise UnsupportedSceneError(
                    f"Node {node.name!r}: component {c.name!r} has emission_order != 0, which applies to a Luminophore only.")
            if a.emission_order != 0.0 and c.phase_function is not isotropic:
                raise UnsupportedSceneError(
                    f"Node {node.name!r}: component {c.name!r} has emission_order != 0 together with a phase function.")

    def _lower_alignment(self, i, node, component, cols, align):
        """Id of the component's alignment record (-1: none).  The director goes ONCE to the root's frame: with the rows
        R0, R1, R2 of the node's rotation to the root, n_w,i = (Ri,0 nx + Ri,1 ny) + Ri,2 nz, then divided by
        sqrt((x x + y y) + z z) of the result (rule 1 of the `Alignment` docstring).  An emission order != 0 turns the
        component's phase function into the pooled single-row table of f(mu; S_e), one table per order."""
        a = getattr(component, "alignment", None)
        if a is None:
            return -1
        if a.emission_order != 0.0:   # (the column `_lower_component` has just written: isotropic)
            cols["phase_type"][-1] = PHASE_TABLE
            cols["phase_table"][-1] = self._pool_phase_table(a.emission_table, key=("aligned", float(a.emission_order)))
        key = (id(a), i)
        if key not in align["index"]:
            rot = self.local_to_world[i][:3, :3]
            nx, ny, nz = (float(v) for v in a.director)
            w = [(float(rot[r, 0]) * nx + float(rot[r, 1]) * ny) + float(rot[r, 2]) * nz for r in range(3)]
            norm = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
            if not (math.isfinite(norm) and norm > 0.0):
                raise UnsupportedSceneError(f"Node {node.name!r}: the director of component {component.name!r} has no direction in the root's frame.")
            align["index"][key] = (len(align["abs_order"]), a)   # (the object keeps its id from being reused)
            align["axis"].append([v / norm for v in w])
            align["abs_order"].append(float(a.absorption_order))
            align["emit_table"].append(int(cols["phase_table"][-1]) if a.emission_order != 0.0 else -1)
        return align["index"][key][0]

    @property
    def has_alignment(self):
        """A component carries an `Alignment`: the scene needs pvt_scene_create_aligned's tables."""
        return bool(np.any(self.comp_align >= 0))

    def _lower_coat_mode(self, r, mode, names, about, slot):
        """The mode word of coating row `r`: a built-in's number, or COAT_LOBE + 4 table + axis of a ScatterLobe."""
        if isinstance(mode, ScatterLobe):
            if mode.about not in about or not isinstance(mode.table, PhaseFunctionTable):   # (assigned after construction, perhaps)
                raise UnsupportedSceneError(f"Coating {r}: a {slot} lobe must be a PhaseFunctionTable about one of {sorted(about)}.")
            word = COAT_LOBE + 4 * self._pool_phase_table(mode.table) + about[mode.about]
            if word > np.iinfo(_I32).max:
                raise UnsupportedSceneError(f"Coating {r}: too many phase tables for a {slot} lobe.")
            return word
        if mode not in names:
            raise UnsupportedSceneError(f"Coating {r}: {slot} must be one of {sorted(names)} or a ScatterLobe.")
        return names[mode]

    @property
    def has_coating_lobes(self):
        """A coating reflects or transmits into a `ScatterLobe`: the scene needs pvt_scene_create_polyhedra."""
        return bool(np.any(self.coat_reflect_mode >= COAT_LOBE) or np.any(self.coat_transmit_mode >= COAT_LOBE))

    def _pool_phase_table(self, table, key=None):
        ptab = self._ptab
        key = id(table) if key is None else key
        if key not in ptab["index"]:
            ptab["index"][key] = (len(ptab["nw"]), table)   # (the table itself keeps its id from being reused)
            nw, nmu = table.cdf.shape
            ptab["nw"].append(nw)
            ptab["nmu"].append(nmu)
            ptab["wl_start"].append(len(ptab["wavelength"]))
            ptab["mu_start"].append(len(ptab["mu"]))
            ptab["cdf_start"].append(len(ptab["cdf"]))
            # (a table without wavelengths has one row: its wavelength is never read, 0 stands in for it)
            ptab["wavelength"].extend([0.0] if table.wavelength is None else table.wavelength.tolist())
            ptab["mu"].extend(table.mu.tolist())
            ptab["cdf"].extend(table.cdf.ravel().tolist())
        return ptab["index"][key][0]

    # -- components ------------------------------------------------------
    def _lower_component(self, node, component, cols, pools):
        # Subclass order matters: Reactor < Absorber < Scatterer > Luminophore
        if isinstance(component, Reactor):
            ctype = COMP_REACTOR
        elif isinstance(component, Absorber):
            ctype = COMP_ABSORBER
        elif isinstance(component, Luminophore):
            ctype = COMP_LUMINOPHORE
        elif isinstance(component, Scatterer):
            ctype = COMP_SCATTERER
        else:
            raise UnsupportedSceneError(
                f"Component type {type(component).__name__} is not supported."
            )
        phase_type, phase_param = _phase_of(node, component)
        a_start, a_n = self._pool_spectrum(
            node, component._abs_dist, pools["abs_x"], pools["abs_y"]
        )
        e_start, e_n, e_hist = 0, 0, 0
        if ctype == COMP_LUMINOPHORE:
            dist = component._ems_dist
            e_hist = 1 if dist.hist else 0   # histogram-sampled emission (extension, see header)
            e_start = len(pools["ems_x"])
            pools["ems_x"].extend(np.asarray(dist._x, dtype=_F64).tolist())
            pools["ems_cdf"].extend(np.asarray(dist._cdf, dtype=_F64).tolist())
            e_n = len(pools["ems_x"]) - e_start

        cols["type"].append(ctype)
        cols["qy"].append(float(component.quantum_yield))
        cols["tau_rad"].append(float(component.tau_rad) if component.tau_rad else 0.0)
        cols["tau_nr"].append(float(component.tau_nr) if component.tau_nr else 0.0)
        cols["phase_type"].append(phase_type)
        cols["phase_param"].append(phase_param)
        cols["phase_table"].append(
            self._pool_phase_table(component.phase_function) if phase_type == PHASE_TABLE else -1)
        cols["abs_start"].append(a_start)
        cols["abs_n"].append(a_n)
        cols["ems_start"].append(e_start)
        cols["ems_n"].append(e_n)
        cols["abs_hist"].append(1 if (component._abs_dist.hist and component._abs_dist._x is not None) else 0)
        cols["ems_hist"].append(e_hist)

    def _pool_spectrum(self, node, dist, xs, ys):
        # hist=True spectra are pooled like interpolated ones; the per-component hist flag
        # switches the device lookup to the step-function rule (extension: the reference
        # compiler raises here, compiler.py:313-317)
        start = len(xs)
        if dist._x is None:
            # constant coefficient -> a one-point table
            xs.append(0.0)
            ys.append(float(dist._y))
            return start, 1
        xs.extend(np.asarray(dist._x, dtype=_F64).tolist())
        ys.extend(np.asarray(dist._y, dtype=_F64).tolist())
        return start, len(xs) - start

    # -- recorders -------------------------------------------------------
    def _lower_recorders(self, nodes):
        found = []
        for i, node in enumerate(nodes):
            for recorder in getattr(node, "recorders", []):
                if not isinstance(recorder, Recorder):
                    raise UnsupportedSceneError(
                        f"Node {node.name!r} recorders must be Recorder objects."
                    )
                if recorder.event in VOLUME_EVENTS and recorder.facet is not None:
                    raise UnsupportedSceneError(
                        f"Recorder {recorder.name!r}: facet filters only apply "
                        "to surface events."
                    )
                found.append((i, recorder))
        if len(found) > MAX_RECORDERS:
            raise UnsupportedSceneError(
                f"At most {MAX_RECORDERS} recorders are supported."
            )
        names = [rec.name for _, rec in found]
        if len(set(names)) != len(names):
            raise UnsupportedSceneError("Recorder names must be unique.")

        n = len(found)
        self.recorder_names = names
        self.recorder_specs = [rec for _, rec in found]
        self.rec_node = np.zeros(n, dtype=_I32)
        self.rec_event = np.zeros(n, dtype=_I32)
        self.rec_has_facet = np.zeros(n, dtype=_I32)
        self.rec_facet = np.zeros((max(n, 1), 3), dtype=_F64)
        self.rec_atol = np.zeros(n, dtype=_F64)
        self.rec_hist_start = np.zeros(n, dtype=_I32)
        self.rec_hist_n = np.zeros(n, dtype=_I32)
        self.rec_source_mode = np.zeros(n, dtype=_I32)
        self.rec_source_id = np.full(n, -1, dtype=_I32)

        hist = {k: [] for k in ("pa", "pb", "na", "nb", "loa", "hia", "lob", "hib", "off")}
        offset = 0
        for r, (node_index, recorder) in enumerate(found):
            self.rec_node[r] = node_index
            self.rec_event[r] = ALL_EVENTS[recorder.event]
            if recorder.facet is not None:
                self.rec_has_facet[r] = 1
                self.rec_facet[r] = recorder.facet
            self.rec_atol[r] = recorder.atol
            src = getattr(recorder, "source", None)
            if src is not None:
                if src == "lights":
                    self.rec_source_mode[r] = SOURCE_LIGHTS
                elif src == "components":
                    self.rec_source_mode[r] = SOURCE_COMPONENTS
                elif src in self.component_names:
                    if self.component_names.count(src) > 1:
                        # the filter is one component id; the reference's dataframe filter by name
                        # would match every component of that name
                        raise UnsupportedSceneError(
                            f"Recorder {recorder.name!r}: source {src!r} names "
                            f"{self.component_names.count(src)} components; give them distinct names."
                        )
                    self.rec_source_mode[r] = SOURCE_COMPONENT
                    self.rec_source_id[r] = self.component_names.index(src)
                else:
                    raise UnsupportedSceneError(
                        f"Recorder {recorder.name!r}: unknown source {src!r} (use 'lights', "
                        "'components' or a component name)."
                    )
            self.rec_hist_start[r] = len(hist["pa"])
            for spec in recorder.histograms:
                if isinstance(spec, Heatmap):
                    a, b = spec.a, spec.b
                    row = (HISTOGRAM_PROPERTIES[a.prop], HISTOGRAM_PROPERTIES[b.prop], a.bins, b.bins,
                           a.start, a.stop, b.start, b.stop)
                else:
                    row = (HISTOGRAM_PROPERTIES[spec.prop], -1, spec.bins, 1,
                           spec.start, spec.stop, 0.0, 1.0)
                for key, value in zip(("pa", "pb", "na", "nb", "loa", "hia", "lob", "hib"), row):
                    hist[key].append(value)
                hist["off"].append(offset)
                offset += row[2] * row[3]
            self.rec_hist_n[r] = len(recorder.histograms)

        self.hist_prop_a = np.array(hist["pa"], dtype=_I32)
        self.hist_prop_b = np.array(hist["pb"], dtype=_I32)
        self.hist_na = np.array(hist["na"], dtype=_I32)
        self.hist_nb = np.array(hist["nb"], dtype=_I32)
        self.hist_lo_a = np.array(hist["loa"], dtype=_F64)
        self.hist_hi_a = np.array(hist["hia"], dtype=_F64)
        self.hist_lo_b = np.array(hist["lob"], dtype=_F64)
        self.hist_hi_b = np.array(hist["hib"], dtype=_F64)
        self.hist_offset = np.array(hist["off"], dtype=_I32)
        self.total_bins = int(offset)

        # ray capture: rows each recorder may keep (0: not captured) and its first row, the captures packed one after the
        # other in recorder order (`capture_rows` rows per tally set)
        self.rec_capture_capacity = np.zeros(n, dtype=np.int64)
        self.rec_capture_start = np.zeros(n, dtype=np.int64)
        rows = 0
        for r, (_, recorder) in enumerate(found):
            capacity = getattr(recorder, "capture", None)
            self.rec_capture_start[r] = rows
            if capacity is None:
                continue
            if not isinstance(capacity, numbers.Integral) or isinstance(capacity, bool) or capacity <= 0:
                raise UnsupportedSceneError(
                    f"Recorder {recorder.name!r}: capture must be a positive integer number of rows, got {capacity!r}.")
            capacity = int(capacity)   # (a numpy integer assigned after construction)
            if rows + capacity > MAX_CAPTURE_ROWS:
                raise UnsupportedSceneError(
                    f"The scene's captures hold more than {MAX_CAPTURE_ROWS} rows (2^24, summed over its recorders), "
                    f"reached at Recorder {recorder.name!r}.")
            self.rec_capture_capacity[r] = capacity
            rows += capacity
        self.capture_rows = int(rows)

    @property
    def has_captures(self):
        return self.capture_rows > 0

    @property
    def has_counter_histograms(self):
        """A histogram axis is a photon event counter (`recorder.EXTENSION_PROPERTIES`)."""
        first, last = min(EXTENSION_PROPERTIES.values()), max(EXTENSION_PROPERTIES.values())
        return bool(np.any((self.hist_prop_a >= first) & (self.hist_prop_a <= last))
                    or np.any((self.hist_prop_b >= first) & (self.hist_prop_b <= last)))

    @property
    def origin_mask(self):
        """Which launch-origin properties (`recorder.ORIGIN_PROPERTIES`) some histogram axis reads: bit k for the k-th of
        origin_wavelength, origin_x, origin_y, origin_z; 0 = none."""
        first, mask = min(ORIGIN_PROPERTIES.values()), 0
        for k in range(len(ORIGIN_PROPERTIES)):
            if np.any(self.hist_prop_a == first + k) or np.any(self.hist_prop_b == first + k):
                mask |= 1 << k
        return mask

    # -- volume maps -----------------------------------------------------
    def _lower_maps(self, root, nodes):
        """VolumeMap specs -> per-node runs (node_map_start / node_map_count) and one record per map, in node order:
        the event kind (or the path-length kind), the component id (-1: any; always -1 for a path-length map), shape,
        lower, cell widths h = (upper - lower) / n, wavelength bins (0: no axis) and range, and the map's first slot in the maps' block, which follows the recorders' bins in the
        int64 tally buffer (`map_slots` slots in all; `total_bins` keeps the reference's meaning)."""
        for node in root.preorder():
            if node.geometry is None and getattr(node, "volume_maps", None):
                raise UnsupportedSceneError(
                    f"Node {node.name!r} has no geometry: a volume map tallies the events inside a node's volume.")
        count = len(nodes)
        self.node_map_start = np.zeros(count, dtype=_I32)
        self.node_map_count = np.zeros(count, dtype=_I32)
        self.map_specs, self.map_names = [], []
        cols = {k: [] for k in ("kind", "component", "shape", "lower", "h", "nw", "wl_start", "wl_stop", "offset")}
        slots = 0
        for i, node in enumerate(nodes):
            self.node_map_start[i] = len(self.map_specs)
            for spec in getattr(node, "volume_maps", None) or ():
                if not isinstance(spec, VolumeMap):
                    raise UnsupportedSceneError(f"Node {node.name!r} volume_maps must be VolumeMap objects.")
                if node is root:
                    raise UnsupportedSceneError(
                        f"Root node {node.name!r}: the scene's root cannot carry a volume map (VolumeMap {spec.name!r}).")
                if spec.event not in MAP_EVENTS:
                    raise UnsupportedSceneError(
                        f"VolumeMap {spec.name!r}: unknown event {spec.event!r}; use one of {sorted(MAP_EVENTS)}.")
                component = -1
                if spec.event == "pathlength" and spec.component is not None:
                    raise UnsupportedSceneError(
                        f"VolumeMap {spec.name!r}: a path-length map takes no component filter "
                        f"(component={spec.component!r}).")
                if spec.component is not None:
                    first, n = int(self.comp_start[i]), int(self.comp_count[i])
                    own = self.component_names[first:first + n]
                    if own.count(spec.component) != 1:
                        raise UnsupportedSceneError(
                            f"VolumeMap {spec.name!r}: unknown component {spec.component!r}; node {node.name!r} has "
                            f"{own} (the filter names exactly one of the node's own components).")
                    component = first + own.index(spec.component)
                if spec.name in self.map_names:
                    raise UnsupportedSceneError(f"Volume map names must be unique; {spec.name!r} is used twice.")
                if spec.name in self.recorder_names:
                    raise UnsupportedSceneError(
                        f"VolumeMap {spec.name!r}: a recorder has the same name; maps and recorders share one namespace.")
                h = spec.cell_widths
                if not all(math.isfinite(v) and v > 0.0 for v in h):
                    raise UnsupportedSceneError(f"VolumeMap {spec.name!r}: cell widths {h} must be finite and > 0.")
                if slots + spec.size > MAX_MAP_SLOTS:
                    raise UnsupportedSceneError(
                        f"The scene's volume maps hold more than {MAX_MAP_SLOTS} slots (2^26: cells x wavelength bins, plus "
                        f"one per map), reached at VolumeMap {spec.name!r}.")
                self.map_specs.append(spec)
                self.map_names.append(spec.name)
                cols["kind"].append(MAP_EVENTS[spec.event])
                cols["component"].append(component)
                cols["shape"].append(list(spec.shape))
                cols["lower"].append(list(spec.lower))
                cols["h"].append(list(h))
                cols["nw"].append(spec.wavelength_bins)
                cols["wl_start"].append(spec.wavelength.start if spec.wavelength is not None else 0.0)
                cols["wl_stop"].append(spec.wavelength.stop if spec.wavelength is not None else 1.0)
                cols["offset"].append(slots)
                slots += spec.size
            self.node_map_count[i] = len(self.map_specs) - self.node_map_start[i]
        self.n_maps = len(self.map_specs)
        self.map_kind = np.array(cols["kind"], dtype=_I32)
        self.map_component = np.array(cols["component"], dtype=_I32)
        self.map_shape = np.array(cols["shape"], dtype=_I32).reshape(-1, 3)
        self.map_lower = np.array(cols["lower"], dtype=_F64).reshape(-1, 3)
        self.map_h = np.array(cols["h"], dtype=_F64).reshape(-1, 3)
        self.map_nw = np.array(cols["nw"], dtype=_I32)
        self.map_wl_start = np.array(cols["wl_start"], dtype=_F64)
        self.map_wl_stop = np.array(cols["wl_stop"], dtype=_F64)
        self.map_offset = np.array(cols["offset"], dtype=np.int64)
        self.map_slots = int(slots)

    @property
    def has_maps(self):
        return self.n_maps > 0

    # -- introspection ----------------------------------------------------
    TABLE_FIELDS = (
        "geom_type", "geom_params", "local_to_world", "world_to_local",
        "refractive_index", "surface_type", "comp_start", "comp_count",
        "comp_type", "comp_qy", "comp_tau_rad", "comp_tau_nr",
        "comp_phase_type", "comp_phase_param", "comp_abs_start", "comp_abs_n",
        "comp_ems_start", "comp_ems_n", "comp_abs_hist", "comp_ems_hist", "abs_x", "abs_y", "ems_x", "ems_cdf",
        "rec_node", "rec_event", "rec_has_facet", "rec_facet", "rec_atol",
        "rec_hist_start", "rec_hist_n", "rec_source_mode", "rec_source_id", "hist_prop_a", "hist_prop_b", "hist_na",
        "hist_nb", "hist_lo_a", "hist_hi_a", "hist_lo_b", "hist_hi_b",
        "hist_offset",
        "coat_start", "coat_count", "coat_facet", "coat_lo", "coat_hi",
        "coat_reflectivity", "coat_reflect_mode", "coat_transmit_mode",
        "coat_table", "ctab_nw", "ctab_na", "ctab_wl_start", "ctab_angle_start", "ctab_value_start",
        "ctab_wavelength", "ctab_angle", "ctab_value",
        "mesh_face_start", "mesh_face_count", "mesh_vertices", "mesh_faces", "mesh_normals",
        "ri_table", "rtab_n", "rtab_start", "rtab_wavelength", "rtab_value",
        "comp_phase_table", "ptab_nw", "ptab_nmu", "ptab_wl_start", "ptab_mu_start", "ptab_cdf_start",
        "ptab_wavelength", "ptab_mu", "ptab_cdf",
        "surface_roughness",
        "node_field", "field_shape", "field_lower", "field_upper", "comp_values", "values_start", "values_count",
        "field_values",
    )

    # The tables of the later extensions are part of `tables()` only when the scene has the extension, so that a scene
    # without it lowers to the same tables, key for key, as before there was one: the volume maps', the captures', the
    # absorbing coatings' (a coating has an absorptivity), the coating patterns' (a coating has a pattern or
    # facet=None), the alignments' (a component has an Alignment) and the polyhedra's (a node is a Polyhedron).  Which attributes they are is what the binding reads for the extension's struct.
    MAP_TABLE_FIELDS, CAPTURE_TABLE_FIELDS, ABSORB_TABLE_FIELDS, PATTERN_TABLE_FIELDS, ALIGN_TABLE_FIELDS, POLYHEDRON_TABLE_FIELDS = (
        tuple(attribute for attribute, _ in struct_type.POINTERS.values())
        for struct_type in (native.PvtMapTables, native.PvtCaptureTables, native.PvtCoatingAbsorbTables,
                            native.PvtCoatingPatternTables, native.PvtAlignTables, native.PvtPolyhedronTables))

    def tables(self):
        """dict of every numeric table (for fixtures / debugging)."""
        out = {name: getattr(self, name) for name in self.TABLE_FIELDS}
        out["root_id"] = np.int32(self.root_id)
        out["total_bins"] = np.int32(self.total_bins)
        if self.has_maps:
            out.update({name: getattr(self, name) for name in self.MAP_TABLE_FIELDS})
            out["map_slots"] = np.int64(self.map_slots)
        if self.has_captures:
            out.update({name: getattr(self, name) for name in self.CAPTURE_TABLE_FIELDS})
            out["capture_rows"] = np.int64(self.capture_rows)
        if self.has_absorbing_coatings:
            out.update({name: getattr(self, name) for name in self.ABSORB_TABLE_FIELDS})
        if self.has_coating_patterns:
            out.update({name: getattr(self, name) for name in self.PATTERN_TABLE_FIELDS})
        if self.has_alignment:
            out.update({name: getattr(self, name) for name in self.ALIGN_TABLE_FIELDS})
        if self.has_polyhedron:
            out.update({name: getattr(self, name) for name in self.POLYHEDRON_TABLE_FIELDS})
        return out

    @property
    def has_coatings(self):
        return self.n_coatings > 0


def compile_scene(scene) -> CompiledScene:
    """Flatten `scene` into tables, or raise `UnsupportedSceneError`."""
    return CompiledScene(scene)
