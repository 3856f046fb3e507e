"""Recorder statistics recomputed on the host from photon histories.

The device accumulates recorders inside the trace kernel (tally block of
csrc/pvt_trace_kernel.h).  This module answers the same question — "what should every recorder
of this scene hold?" — from `(ray, event, metadata)` histories such as `EngineResult.histories()`,
with the semantics of the reference's pvtrace/engine/tally.py:26-156.  The tests use it to prove
the kernel's accumulators exact on sampled runs.

Organisation: every recorder becomes a `_Probe` bound to its node.  Probes are filed under the
event kind that can fire them, each history is streamed once through the probes of its events,
a probe keeps the property values of the FIRST qualifying event of each ray, and moments and
histograms are computed from those columns with numpy at the end.  The stream counts the EMIT, SCATTER
and REFLECT events of a history as it goes; a probe is offered an event with the counts of the events
BEFORE it (the photon as it arrives: the contract in `recorder.Histogram`), and with the ray of the
history's first row, the photon as launched (the `origin_*` properties).
"""
import math

import numpy as np

from pvtrace_amd.engine.recorder import MAP_PATHLENGTH, Heatmap
from pvtrace_amd.lattice import cell_inside, slot as lattice_slot, walk
from pvtrace_amd.light import Event

# recorder selector -> (history event, metadata keys that must all name the recorder's node)
_TRIGGERS = {
    "entering": (Event.TRANSMIT, ("hit", "adjacent")),
    "escaping": (Event.TRANSMIT, ("hit", "container")),
    "reflected": (Event.REFLECT, ("hit", "adjacent")),
    "lost": (Event.NONRADIATIVE, ("container",)),
    "reacted": (Event.REACT, ("container",)),
    "killed": (Event.KILL, ("container",)),
    "exit": (Event.EXIT, ("hit",)),
    "detected": (Event.DETECT, ("hit",)),   # absorbed by a coating of the node, from either side (extension)
}
_COLUMNS = ("wavelength", "angle", "duration", "pathlength", "x", "y", "z", "emissions", "scatterings", "reflections",
            "origin_wavelength", "origin_x", "origin_y", "origin_z")
# the photon's event counters (recorder.EXTENSION_PROPERTIES): history event -> its place among the three
_COUNTED = {Event.EMIT: 0, Event.SCATTER: 1, Event.REFLECT: 2}


class _Probe:
    """One recorder attached to one node."""

    def __init__(self, node, recorder, root, component_names):
        self.node, self.recorder, self.root = node, recorder, root
        self.event, self.keys = _TRIGGERS[recorder.event]
        self.component_names = component_names
        self.crossings = 0
        self.rows = []          # one row of _COLUMNS per distinct ray
        self.open = True        # no crossing of the current ray counted yet

    # -- selection ---------------------------------------------------------------------
    def _from_wanted_source(self, source):
        want = getattr(self.recorder, "source", None)
        if want is None:
            return True
        emitted_by_component = source in self.component_names
        if want == "lights":
            return not emitted_by_component
        if want == "components":
            return emitted_by_component
        return source == want

    def _local(self, position):
        return tuple(position) if self.node is self.root else self.root.point_to_node(position, self.node)

    def offer(self, ray, meta, incoming, counters=(0, 0, 0), origin=None):
        """Present one history event of this probe's kind; `incoming` is the ray as it arrived, `counters` the EMIT,
        SCATTER and REFLECT events of its history before this one, `origin` the ray of the history's FIRST row (the
        photon as launched; None: this ray) -- its wavelength and its position, in the root's frame as the log has it,
        are the `origin_*` columns."""
        name = self.node.name
        if any(meta.get(key) != name for key in self.keys) or not self._from_wanted_source(ray.source):
            return
        normal = meta.get("normal")
        if normal is None and self.event == Event.EXIT:
            normal = self.node.vector_to_node(self.node.geometry.normal(self._local(ray.position)), self.root)
        facet = self.recorder.facet
        if facet is not None:
            if normal is None or max(abs(f - c) for f, c in zip(facet, normal)) > self.recorder.atol:
                return
        self.crossings += 1
        if not self.open:
            return
        self.open = False
        angle = 0.0
        if normal is not None:
            along = ray.direction if self.event == Event.EXIT else incoming.direction
            angle = math.acos(min(abs(float(np.dot(along, normal))), 1.0))
        x, y, z = self._local(ray.position)
        first = ray if origin is None else origin
        self.rows.append((ray.wavelength, angle, ray.duration, ray.travelled, x, y, z) + tuple(counters)
                         + (first.wavelength,) + tuple(first.position))

    # -- reduction ---------------------------------------------------------------------
    @staticmethod
    def _bin_indices(values, axis):
        """C-style truncation of (v - lo) / (hi - lo) * n, -1 outside [0, n) (tally.py:81-83)."""
        index = ((values - axis.start) / (axis.stop - axis.start) * axis.bins).astype(np.int64)
        return np.where((index >= 0) & (index < axis.bins), index, -1)

    def result(self):
        from pvtrace_amd.engine.api import RecorderResult

        table = np.array(self.rows, dtype=np.float64).reshape(len(self.rows), len(_COLUMNS))
        column = {name: table[:, k] for k, name in enumerate(_COLUMNS)}
        moments = np.zeros((4, 2))
        for k, name in enumerate(_COLUMNS[:4]):
            moments[k] = column[name].sum(), (column[name] * column[name]).sum()
        bins = []
        for spec in self.recorder.histograms:
            if isinstance(spec, Heatmap):
                ia, ib = self._bin_indices(column[spec.a.prop], spec.a), self._bin_indices(column[spec.b.prop], spec.b)
                inside = (ia >= 0) & (ib >= 0)
                flat = ia[inside] * spec.b.bins + ib[inside]
                bins.append(np.bincount(flat, minlength=spec.a.bins * spec.b.bins).astype(np.int64))
            else:
                index = self._bin_indices(column[spec.prop], spec)
                bins.append(np.bincount(index[index >= 0], minlength=spec.bins).astype(np.int64))
        return RecorderResult(self.recorder, len(self.rows), self.crossings, moments, bins)


def tally_histories(scene, histories):
    """{recorder name: RecorderResult} from one history per ray."""
    root = scene.root
    nodes = list(root.preorder())
    component_names = {component.name for node in nodes
                       if node.geometry is not None and node.geometry.material is not None
                       for component in node.geometry.material.components}
    probes = [_Probe(node, recorder, root, component_names)
              for node in nodes for recorder in getattr(node, "recorders", [])]
    by_event = {}
    for probe in probes:
        by_event.setdefault(probe.event, []).append(probe)

    for history in histories:
        for probe in probes:
            probe.open = True
        incoming, counters, origin = None, [0, 0, 0], None
        for ray, event, meta in history:
            if origin is None:
                origin = ray   # the GENERATE row: the photon as launched
            for probe in by_event.get(event, ()):
                probe.offer(ray, meta or {}, incoming or ray, counters, origin)
            if event in _COUNTED:
                counters[_COUNTED[event]] += 1
            incoming = ray
    return {probe.recorder.name: probe.result() for probe in probes}


def capture_histories(scene, histories, ray_offset=0, indices=None):
    """{recorder name: CapturedRays} from one history per ray: the rays behind each captured recorder's `rays` count, built
    on the host with the matching rule of `tally_histories` (first match per ray, facet tolerance, source filter).  The
    row of a ray holds the values of the matching history event -- position, direction, wavelength, path, clock --, the
    photon's source as a component id of the compiled scene (-1: a light) and its event counters as it arrives.  History j is ray `ray_offset + j`, or
    `indices[j]`; the capacity is applied in ray order: the first `capacity` matching rays are kept.  The host path for
    `follow(backend="host")` users, and the referee of the kernel's captures.

    A history names a photon's source by the component's NAME, so the id is that of the first component of the name:
    where two components share a name the `source` column may differ from the kernel's, which knows the component
    itself.  The scene is flattened anew on every call (for the component ids); a referee's cost, not a hot path's."""
    from pvtrace_amd.engine.compiler import compile_scene
    from pvtrace_amd.engine.recorder import CapturedRays

    root = scene.root
    nodes = list(root.preorder())
    component_ids = {}
    for k, name in enumerate(compile_scene(scene).component_names):
        component_ids.setdefault(name, k)
    probes = [_Probe(node, recorder, root, set(component_ids))
              for node in nodes for recorder in getattr(node, "recorders", []) if getattr(recorder, "capture", None)]
    by_event = {}
    for probe in probes:
        by_event.setdefault(probe.event, []).append(probe)
    kept = {id(probe): [] for probe in probes}
    for j, history in enumerate(histories):
        index = int(indices[j]) if indices is not None else int(ray_offset) + j
        for probe in probes:
            probe.open = True
        incoming, counters = None, [0, 0, 0]
        for ray, event, meta in history:
            for probe in by_event.get(event, ()):
                before = len(probe.rows)
                probe.offer(ray, meta or {}, incoming or ray, counters)
                if len(probe.rows) > before:   # this ray's first match
                    kept[id(probe)].append((index, tuple(ray.position), tuple(ray.direction), float(ray.wavelength),
                                            float(ray.travelled), float(ray.duration), component_ids.get(ray.source, -1))
                                           + tuple(counters))
            if event in _COUNTED:
                counters[_COUNTED[event]] += 1
            incoming = ray
    out = {}
    for probe in probes:
        rows = sorted(kept[id(probe)], key=lambda row: row[0])
        matched, capacity = len(rows), probe.recorder.capture
        rows = rows[:capacity]
        out[probe.recorder.name] = CapturedRays(probe.recorder.name, capacity, matched, {
            "index": np.array([r[0] for r in rows], dtype=np.int64),
            "position": np.array([r[1] for r in rows], dtype=np.float64).reshape(len(rows), 3),
            "direction": np.array([r[2] for r in rows], dtype=np.float64).reshape(len(rows), 3),
            "wavelength": np.array([r[3] for r in rows], dtype=np.float64),
            "pathlength": np.array([r[4] for r in rows], dtype=np.float64),
            "duration": np.array([r[5] for r in rows], dtype=np.float64),
            "source": np.array([r[6] for r in rows], dtype=np.int32),
            "emissions": np.array([r[7] for r in rows], dtype=np.int32),
            "scatterings": np.array([r[8] for r in rows], dtype=np.int32),
            "reflections": np.array([r[9] for r in rows], dtype=np.int32)})
    return out


def path_segment_pieces(p, u, length, lower, h, shape):
    """The pieces of one segment in one lattice, by the path-length contract of the `VolumeMap` docstring (items 5-10), in
    pure Python floats and in the contract's operation order: `p`, `u` the local start and direction, `length` = L.
    Returns [((cx, cy, cz), units)] for every piece with units != 0, in walking order; a cell index of -1 or n is a slab
    outside the lattice."""
    if not (length > 0.0) or not (length < math.inf):
        return []
    units = ((cell, int((sout - s) * 1073741824.0 + 0.5)) for cell, s, sout in walk(p, u, length, lower, h, shape, slabs=True))
    return [(cell, k) for cell, k in units if k != 0]


def path_map_slots(compiled, histories):
    """(slots, pieces) of the compiled scene's path-length maps from one history per ray: two int64 arrays laid out as
    the maps' block (`CompiledScene.map_offset`), the units every slot holds and how many pieces put them there (what a
    comparison with another walk of the same histories may differ by, one unit each).  The event maps' slots stay 0."""
    slots = np.zeros(compiled.map_slots, dtype=np.int64)
    pieces = np.zeros(compiled.map_slots, dtype=np.int64)
    mapped = {compiled.node_names[i]: i for i in range(len(compiled.node_names)) if compiled.node_map_count[i] > 0}
    _path_maps(compiled, histories, mapped, slots, pieces)
    return slots, pieces


def _path_maps(compiled, histories, mapped, slots, pieces=None):
    """The path-length maps' part of `map_histories`: every segment of every history, walked into `slots`."""
    records = {}   # node index -> (world_to_local rows as Python floats, [(offset, shape, lower, h, nw, wl_start, wl_stop)])
    for i in mapped.values():
        first = int(compiled.node_map_start[i])
        maps = []
        for m in range(first, first + int(compiled.node_map_count[i])):
            if int(compiled.map_kind[m]) != MAP_PATHLENGTH:
                continue
            maps.append((int(compiled.map_offset[m]), tuple(int(n) for n in compiled.map_shape[m]),
                         tuple(float(v) for v in compiled.map_lower[m]), tuple(float(v) for v in compiled.map_h[m]),
                         int(compiled.map_nw[m]), float(compiled.map_wl_start[m]), float(compiled.map_wl_stop[m])))
        if maps:
            records[i] = ([[float(v) for v in row] for row in compiled.world_to_local[i][:3]], maps)
    if not records:
        return
    for history in histories:
        history = list(history)
        for (ray, _, _), (after, _, meta) in zip(history, history[1:]):
            record = records.get(mapped.get((meta or {}).get("container")))
            if record is None:
                continue
            length = float(after.travelled) - float(ray.travelled)
            if not (length > 0.0) or not (length < math.inf):
                continue
            w2l, maps = record
            x, y, z = (float(v) for v in ray.position)
            dx, dy, dz = (float(v) for v in ray.direction)
            p = [((w2l[a][0] * x + w2l[a][1] * y) + w2l[a][2] * z) + w2l[a][3] for a in range(3)]
            u = [(w2l[a][0] * dx + w2l[a][1] * dy) + w2l[a][2] * dz for a in range(3)]
            wl = float(ray.wavelength)
            for at, shape, lower, h, nw, wl_start, wl_stop in maps:
                nwc, iw, wl_in = max(nw, 1), 0, True
                if nw > 0:   # a Histogram's rule; out of range: the whole segment goes to `outside`
                    q = (wl - wl_start) / (wl_stop - wl_start) * float(nw)
                    wl_in = q > -1.0 and q < float(nw)
                    iw = int(q) if wl_in else 0
                outside = shape[0] * shape[1] * shape[2] * nwc
                for (cx, cy, cz), k in path_segment_pieces(p, u, length, lower, h, shape):
                    inside = wl_in and 0 <= cx < shape[0] and 0 <= cy < shape[1] and 0 <= cz < shape[2]
                    slot = at + (lattice_slot(shape, (cx, cy, cz)) * nwc + iw if inside else outside)
                    slots[slot] += k
                    if pieces is not None:
                        pieces[slot] += 1


def map_histories(scene, histories):
    """{map name: VolumeMapResult} from one history per ray: the scene's `VolumeMap`s binned on the host, in numpy, by
    the contract stated in the `VolumeMap` docstring -- every event of the map's kind whose container is the map's node,
    local point ((R0 x + R1 y) + R2 z) + t from the COMPILED scene's `world_to_local` rows (the tables the kernel reads,
    not a second composition of the node tree), `lattice.cell_inside` per axis, no clamping, one `outside` slot.  The host
    path for `follow(backend="host")` users, and the referee of the kernel's maps.

    Path-length maps (``event="pathlength"``) are walked by `path_segment_pieces`, in pure Python floats: a ray's segments
    are consecutive rows k, k + 1 of its history -- from row k's position along row k's direction, with row k's
    wavelength, for L = `travelled` of row k + 1 minus that of row k, in the node row k + 1 names as its `container`."""
    from pvtrace_amd.engine.api import maps_from_slots
    from pvtrace_amd.engine.compiler import compile_scene

    compiled = scene if hasattr(scene, "map_specs") else compile_scene(scene)
    if not compiled.has_maps:
        return {}
    kinds = sorted(set(int(k) for k in compiled.map_kind) - {MAP_PATHLENGTH})
    has_path = any(int(k) == MAP_PATHLENGTH for k in compiled.map_kind)
    if has_path:
        histories = list(histories)   # (walked a second time below)
    mapped = {compiled.node_names[i]: i for i in range(len(compiled.node_names)) if compiled.node_map_count[i] > 0}
    # the events a map can count, per node: kind, component name, world position, wavelength
    rows = {i: ([], [], [], []) for i in mapped.values()}
    for history in histories:
        for ray, event, meta in history:
            code = int(getattr(event, "value", event))
            if code not in kinds:
                continue
            i = mapped.get((meta or {}).get("container"))
            if i is None:
                continue
            kind, comp, pos, wl = rows[i]
            kind.append(code)
            comp.append(meta.get("component"))
            pos.append(tuple(float(v) for v in ray.position))
            wl.append(float(ray.wavelength))
    slots = np.zeros(compiled.map_slots, dtype=np.int64)
    if has_path:
        _path_maps(compiled, histories, mapped, slots)
    for i, (kind, comp, pos, wl) in rows.items():
        kind = np.array(kind, dtype=np.int64)
        x = np.array(pos, dtype=np.float64).reshape(len(pos), 3)
        wl = np.array(wl, dtype=np.float64)
        w2l = compiled.world_to_local[i]
        # (element-wise products and sums in the contract's order: no matrix product, whose summation order is BLAS's)
        local = [((w2l[a, 0] * x[:, 0] + w2l[a, 1] * x[:, 1]) + w2l[a, 2] * x[:, 2]) + w2l[a, 3] for a in range(3)]
        first = int(compiled.node_map_start[i])
        for m in range(first, first + int(compiled.node_map_count[i])):
            spec = compiled.map_specs[m]
            if int(compiled.map_kind[m]) == MAP_PATHLENGTH:
                continue
            match = kind == int(compiled.map_kind[m])
            if spec.component is not None:
                match &= np.array([c == spec.component for c in comp], dtype=bool)
            inside = np.ones(len(kind), dtype=bool)
            cell = np.zeros(len(kind), dtype=np.int64)
            with np.errstate(invalid="ignore"):
                for a in range(3):
                    n = int(compiled.map_shape[m, a])
                    ok, f = cell_inside(local[a], compiled.map_lower[m, a], compiled.map_h[m, a], n)
                    inside &= ok
                    cell = cell * n + np.where(ok, f, 0.0).astype(np.int64)
                nw = int(compiled.map_nw[m])
                if nw > 0:
                    lo, hi = compiled.map_wl_start[m], compiled.map_wl_stop[m]
                    q = (wl - lo) / (hi - lo) * float(nw)
                    ok = (q > -1.0) & (q < float(nw))   # (truncation, a Histogram's rule: bin 0 reaches down to -1 exclusive)
                    inside &= ok
                    cell = cell * nw + np.trunc(np.where(ok, q, 0.0)).astype(np.int64)
            size = spec.size
            index = np.where(inside, cell, size - 1)[match]
            at = int(compiled.map_offset[m])
            slots[at:at + size] += np.bincount(index, minlength=size).astype(np.int64)
    return maps_from_slots(compiled, slots)
