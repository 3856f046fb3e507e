"""Recorder (tally) specifications attached to scene nodes.

A recorder counts the rays that interact with its node in one particular way
and accumulates moments / histograms of their properties; memory scales with
the number of bins, never with the number of photons.  On the MI355X engine
the accumulators live in LDS per workgroup and are flushed with one atomic per
slot per workgroup, then summed across GPUs with a single RCCL all-reduce.

Numeric ids are part of the device ABI (include/pvtrace_hip.h) and equal the
reference's (pvtrace/engine/recorder.py:33-53; kernel side _kernel.pyx:166-172,
:482-498).
"""
import math

from pvtrace_amd.lattice import Lattice

# property id -> what the histogram axis measures.  x/y/z are in the frame of
# the node that owns the recorder.
PROPERTIES = {
    name: code
    for code, name in enumerate(
        ("wavelength", "angle", "duration", "pathlength", "x", "y", "z")
    )
}

# properties the reference does not have (its `PROPERTIES` above stays the reference's dict, exactly): the photon's event
# counters as it ARRIVES at the matching event -- the EMIT / SCATTER / REFLECT rows that strictly precede the matching row
# in the ray's history (include/pvtrace_hip.h, "photon event counters"; `Histogram` states the contract)
EXTENSION_PROPERTIES = {"emissions": 7, "scatterings": 8, "reflections": 9}
ALL_PROPERTIES = {**PROPERTIES, **EXTENSION_PROPERTIES}

# ... and the photon as it was LAUNCHED: the wavelength and the position of its GENERATE row, the position in the scene
# root's frame -- the frame lights emit in and the log stores (include/pvtrace_hip.h, "launch origin"; `Histogram` states
# the contract).  A dict of their own: the two above are pinned as they stand.  `HISTOGRAM_PROPERTIES` is every name a
# histogram axis may carry, what `Histogram` validates against and the flattener lowers from.
ORIGIN_PROPERTIES = {"origin_wavelength": 10, "origin_x": 11, "origin_y": 12, "origin_z": 13}
HISTOGRAM_PROPERTIES = {**ALL_PROPERTIES, **ORIGIN_PROPERTIES}

# selector id -> which interaction fires the recorder.
#   surface: entering (transmit in from outside), escaping (transmit out from
#            inside), reflected (bounced off the outside)
#   volume : lost (non-radiative absorption), reacted (Reactor), killed
#   root   : exit (left the scene through the root surface)
EVENTS = {
    name: code
    for code, name in enumerate(
        ("entering", "escaping", "reflected", "lost", "reacted", "killed", "exit")
    )
}

# selectors the reference does not have (its `EVENTS` above stays the reference's dict, exactly):
#   surface: detected (absorbed at the node's surface by a coating's absorptivity, from either side; include/pvtrace_hip.h
#            PVT_RECX_DETECTED)
EXTENSION_EVENTS = {"detected": 7}
ALL_EVENTS = {**EVENTS, **EXTENSION_EVENTS}

VOLUME_EVENTS = frozenset(("lost", "reacted", "killed"))

# optional source filter (EXTENSION; the reference's recorders have none, its CLI count
# queries filter by source instead, pvtrace/cli/db.py:61-83): which emitter the photon's
# current incarnation came from
SOURCE_ANY, SOURCE_LIGHTS, SOURCE_COMPONENTS, SOURCE_COMPONENT = 0, 1, 2, 3


# rows the captures of one scene may hold, summed over its recorders (include/pvtrace_hip.h PVT_MAX_CAPTURE_ROWS): 1.5 GiB
# of 96-byte rows per tally set on the device, and as much again while `download` gathers the written rows.  One buffer of
# rows exists per launch in flight (two per `Session`, one per `BundlePipeline`, one per stream of a pipeline with
# per-bundle all-reduces); a grouped launch of `simulate_stream` holds one set per bundle and groups no more bundles
# than keep sets x rows within this limit (`DeviceScene.new_tallies` refuses more)
MAX_CAPTURE_ROWS = 1 << 24


def _require(condition, message):
    if not condition:
        raise ValueError(message)


class Histogram:
    """Equal-width binning of one ray property: `bins` bins over [start, stop).

    Same constructor and attributes (`prop`, `start`, `stop`, `bins`) as the reference's
    Histogram (pvtrace/engine/recorder.py:56-72); the flattener turns it into one row of the
    `hist_*` tables.

    Besides the reference's properties `prop` may be one of `EXTENSION_PROPERTIES`, the photon's event counters.  The contract
    (include/pvtrace_hip.h, "photon event counters", states the same; the kernel and `engine.tally` both follow it):

    1. A photon carries three counters, all zero when a light emits it: `emissions`, `scatterings` and `reflections`, the
       rows of kind `Event.EMIT`, `Event.SCATTER` and `Event.REFLECT` in its history -- REFLECT at every node, from either
       side, whether Fresnel, total internal, coating, rough or Lambertian.
    2. At a matching event a counter's value is the number of such rows that STRICTLY PRECEDE the matching row in the ray's
       full history: the counters describe the photon as it arrives.  A `reflected` recorder sees 0 at a ray's first
       reflection.
    3. They are integers, binned as the doubles of the same value by the rule of every other property.
    4. They draw no random number: a scene that uses them traces the same histories and the same other tallies, bit for bit.
    5. They do not depend on launch geometry, carrying, tally-set grouping, the device list or which code finishes a photon.
    6. They add no moments: the eight sums of a recorder stay those of wavelength, angle, duration and pathlength.

    Or one of `ORIGIN_PROPERTIES`, the photon as it was launched: `origin_wavelength`, and `origin_x`, `origin_y`,
    `origin_z`.  The contract (include/pvtrace_hip.h, "launch origin", states the same):

    1. The four doubles are the wavelength and the position of the photon's GENERATE row, bit for bit: what the launch's
       ray arrays hold for it, or what device emission sampled.  They are fixed when the photon is claimed and never
       recomputed: re-emission, scattering and refraction leave them as they are.
    2. The position is in the scene ROOT's frame, the frame lights emit in and the event log stores -- deliberately NOT
       in the recorder node's frame, unlike `x`, `y`, `z`: the bins are then exact against the launch arrays, with no
       transform in between.  For an untransformed node the two frames agree.
    3. They are binned by the rule of every other property, at the recorder's first match.
    4. They draw no random number and change no other result: histories and every other tally stay bit for bit.
    5. They do not depend on how the job was launched: carried launches, tally sets, shards, the device list or which code
       finishes a photon.
    6. They add no moments and no capture columns, and no recorder filters by them."""

    __slots__ = ("prop", "start", "stop", "bins")

    def __init__(self, prop, start, stop, bins):
        _require(prop in HISTOGRAM_PROPERTIES, f"Unknown property {prop!r}; use one of {sorted(PROPERTIES)}")
        lo, hi, count = float(start), float(stop), int(bins)
        _require(hi > lo, "Histogram range requires stop > start.")
        _require(count >= 1, "Histogram requires at least one bin.")
        self.prop, self.start, self.stop, self.bins = prop, lo, hi, count

    @property
    def size(self):
        """Number of accumulator slots."""
        return self.bins

    def __repr__(self):
        return "Histogram(%r, %s, %s, %d)" % (self.prop, self.start, self.stop, self.bins)


class Heatmap:
    """Two properties binned jointly; each range is `(start, stop, bins)`.  Slot of a sample is
    `ia * b.bins + ib` (reference recorder.py:75-83, kernel _kernel.pyx:540-553)."""

    __slots__ = ("a", "b")

    def __init__(self, prop_a, prop_b, range_a, range_b):
        self.a, self.b = Histogram(prop_a, *range_a), Histogram(prop_b, *range_b)

    @property
    def size(self):
        return self.a.bins * self.b.bins

    def __repr__(self):
        return "Heatmap(%r, %r)" % (self.a, self.b)


class Recorder:
    """What to count at a node (reference recorder.py:86-117, plus `source`).

    name        key of the result in `EngineResult.recorders`
    event       one of `EVENTS`: "entering" / "escaping" / "reflected" at the node's surface,
                "lost" / "reacted" / "killed" inside it, "exit" on the root; or of `EXTENSION_EVENTS`: "detected",
                absorbed at the node's surface by a coating's absorptivity (`Coating(absorptivity=...)`), from either side
    facet       optional outward world normal a surface interaction must have (each component
                within `atol`) -- one recorder per face of a box, say
    histograms  `Histogram` / `Heatmap` specs filled by the first matching interaction of a ray
    source      None, "lights", "components" or a component name: only photons whose current
                incarnation was emitted there (extension; splits "solar" from "luminescent")
    capture     None, or a positive integer: keep up to that many of the rays behind `rays` as rows
                (`EngineResult.captures[name]`, a `CapturedRays`; extension)

    A ray is counted once per recorder (`rays`, moments, histograms) however often it
    matches; `crossings` counts every match.
    """

    def __init__(self, name, event="entering", facet=None, atol=1e-6, histograms=None,
                 source=None, capture=None):
        _require(event in EVENTS or event in EXTENSION_EVENTS, f"Unknown event {event!r}; use one of {sorted(EVENTS)}")
        specs = list(histograms or ())
        _require(all(isinstance(spec, (Histogram, Heatmap)) for spec in specs),
                 "histograms must contain Histogram or Heatmap objects.")
        self.name = name
        self.event = event
        self.facet = tuple(map(float, facet)) if facet is not None else None
        self.atol = float(atol)
        self.histograms = specs
        self.source = source
        if capture is not None:
            import numbers

            _require(isinstance(capture, numbers.Integral) and not isinstance(capture, bool),
                     f"Recorder {name!r}: capture must be a positive integer number of rows, got {capture!r}")
            _require(capture > 0, f"Recorder {name!r}: capture must be a positive number of rows, got {capture!r}")
            capture = int(capture)
        self.capture = capture

    @property
    def is_volume(self):
        return self.event in VOLUME_EVENTS

    def __repr__(self):
        return "Recorder(%r, event=%r)" % (self.name, self.event)


CAPTURE_COLUMNS = ("index", "position", "direction", "wavelength", "pathlength", "duration", "source",
                   "emissions", "scatterings", "reflections")
COUNTER_BITS = 20   # width of one counter in word 11 of a captured row: emissions | scatterings << 20 | reflections << 40


class CapturedRays:
    """The rays that fired a recorder with ``capture=capacity``: one row for each ray's FIRST match of the recorder, the
    event that increments `rays`, feeds the moments and fills the histograms.  Columns (numpy, sorted ascending by `index`):

    index       int64, the global ray index `ray_offset + i`; the ray's RNG stream is `seed + index`
    position    (n, 3) float64, bit for bit the `position` column of that event's row in the event log
    direction   (n, 3) float64, likewise (the direction the photon leaves the event with)
    wavelength, pathlength, duration   float64, the `wavelength`, `travelled` and `duration` columns of that row
    source      int32, the photon's current source: a component id (`CompiledScene.component_names`), -1 for a light
    emissions, scatterings, reflections   int32, the photon's event counters as it arrives at that event: the EMIT, SCATTER
                and REFLECT rows that strictly precede the event's row in the ray's history (`Histogram` states the
                contract).  Columns built from a dict without them are zeros.

    and `matched` (first matches, equal to `recorders[name].rays`), `dropped` = matched - len, `capacity`.

    The contract (include/pvtrace_hip.h, PvtCaptureTables, states the same; the kernel and
    `engine.tally.capture_histories` both follow it):

    1. When `dropped == 0` the row set is exact: sorted by index it does not depend on launch geometry, carrying,
       tally-set grouping or the device list.
    2. When the capacity is exceeded, later arrivals are dropped; every kept row is still a correct row and indices stay
       unique.
    3. Which rows survive an overflow is unspecified (the host path keeps the first in ray order; a GPU keeps the first
       to arrive).  With `simulate(devices=[...])` and in pipeline totals the capacity applies per shard / per buffer.
    4. `simulate` warns once per recorder that overflowed.
    """

    def __init__(self, name, capacity, matched, columns):
        import numpy as np

        self.name, self.capacity, self.matched = name, int(capacity), int(matched)
        index = np.asarray(columns["index"], dtype=np.int64)
        # (rows that come off the GPU are sorted already: nothing is copied then)
        order = slice(None) if np.all(index[1:] >= index[:-1]) else np.argsort(index, kind="stable")
        self.index = index[order]
        self.position = np.asarray(columns["position"], dtype=np.float64).reshape(-1, 3)[order]
        self.direction = np.asarray(columns["direction"], dtype=np.float64).reshape(-1, 3)[order]
        self.wavelength = np.asarray(columns["wavelength"], dtype=np.float64)[order]
        self.pathlength = np.asarray(columns["pathlength"], dtype=np.float64)[order]
        self.duration = np.asarray(columns["duration"], dtype=np.float64)[order]
        self.source = np.asarray(columns["source"], dtype=np.int32)[order]
        for counter in EXTENSION_PROPERTIES:
            values = columns.get(counter)
            setattr(self, counter, np.zeros(len(self.index), dtype=np.int32) if values is None
                    else np.asarray(values, dtype=np.int32)[order])

    def __len__(self):
        return len(self.index)

    @property
    def dropped(self):
        return self.matched - len(self)

    def columns(self):
        return {name: getattr(self, name) for name in CAPTURE_COLUMNS}

    @classmethod
    def from_rows(cls, name, capacity, matched, rows, index_shift=0):
        """From device rows, an (n, 12) uint64 / int64 array laid out as include/pvtrace_hip.h says."""
        import numpy as np

        rows = np.ascontiguousarray(rows).reshape(-1, 12)
        f64, i32 = rows.view(np.float64), rows.view(np.int32)
        packed, mask = rows[:, 11].view(np.int64), (1 << COUNTER_BITS) - 1
        return cls(name, capacity, matched, {
            "index": rows[:, 0].view(np.int64) + int(index_shift), "position": f64[:, 1:4], "direction": f64[:, 4:7],
            "wavelength": f64[:, 7], "pathlength": f64[:, 8], "duration": f64[:, 9], "source": i32[:, 20],
            "emissions": packed & mask, "scatterings": (packed >> COUNTER_BITS) & mask,
            "reflections": (packed >> (2 * COUNTER_BITS)) & mask})

    @classmethod
    def merged(cls, parts):
        """Captures of one recorder from consecutive shards, bundles or buffers -> one, concatenated and sorted."""
        import numpy as np

        first = parts[0]
        columns = {name: np.concatenate([getattr(p, name) for p in parts]) for name in CAPTURE_COLUMNS}
        return cls(first.name, first.capacity, sum(p.matched for p in parts), columns)

    def __repr__(self):
        return f"CapturedRays({self.name!r}, rows={len(self)}, matched={self.matched}, capacity={self.capacity})"


# volume-map selector -> the event-log kind it counts (include/pvtrace_hip.h PVT_EV_*; light.Event has the same values)
# ... and "pathlength", which is no event: the kind of a path-length map (include/pvtrace_hip.h PVT_MAP_PATHLENGTH, a
# value that is no PVT_EV_*)
MAP_PATHLENGTH = 100
MAP_EVENTS = {"absorbed": 3, "emitted": 6, "scattered": 5, "lost": 4, "reacted": 8, "pathlength": MAP_PATHLENGTH}
# the length, in the scene's length unit, that one count of a path-length map stands for (PVT_FLUENCE_UNIT)
FLUENCE_UNIT = 2.0 ** -30
# slots (cells x wavelength bins, plus one `outside` slot per map) the maps of one scene may hold: 512 MiB of int64
# counts per tally set (include/pvtrace_hip.h PVT_MAX_MAP_SLOTS)
MAX_MAP_SLOTS = 1 << 26


class VolumeMap:
    """Per-voxel integer tally of one kind of volume event inside a node: attach as ``node.volume_maps = [...]``,
    beside ``node.recorders``; the result is ``EngineResult.volume_maps[name]``, a `VolumeMapResult`.

    name        key of the result
    shape       (nx, ny, nz), each >= 1
    lower,upper the lattice's box in the NODE's own frame, finite, lower < upper on each axis (both required, as for a
                `ConcentrationGrid`; `VolumeMap.like(grid, name, ...)` copies a grid's lattice).  The root carries no map.
    event       "absorbed", "emitted", "scattered", "lost" or "reacted": the event-log kinds ABSORB, EMIT, SCATTER,
                NONRADIATIVE, REACT, restricted to events whose `container` is this node; or "pathlength": no event but
                the path photons travel in each voxel (below)
    component   None, or the name of one of the node's components: only events whose `component` column names it
                (refused together with "pathlength": a path belongs to no component)
    wavelength  None, or (start, stop, bins): a fourth axis binned by `Histogram`'s rule on the wavelength column of the
                event's row (the incoming wavelength for absorbed / lost / reacted / scattered, the new one for emitted)

    A map counts EVERY matching event (the `crossings` rule of a recorder, not its first-per-ray rule): deposition needs
    every event.  All slots are integers, so results are exact and independent of summation order, launch geometry,
    carrying and GPU count.  The contract (include/pvtrace_hip.h, PvtMapTables, states the same; the kernel and
    `engine.tally.map_histories` both follow it):

    1. The local point is p = R x + t, x the event's world position, bit for bit the `position` of its log row.
    2. R and t are the node's world->local rows as the flattener lowers them (`CompiledScene.world_to_local`).
    3. Each coordinate is evaluated as ((R[a][0] x + R[a][1] y) + R[a][2] z) + t[a], without FMA.
    4. Per axis h = (upper - lower) / n and i = floor((p - lower) / h).
    5. The event is inside when 0 <= i <= n - 1 on all three axes and the wavelength bin, if any, is in range:
       iw = trunc((w - start) / (stop - start) * bins), inside when 0 <= iw <= bins - 1.
    6. The slot is ((ix ny + iy) nz + iz) nw + iw.
    7. Every other matching event adds one to the map's single `outside` slot.
    8. No clamping: unlike a concentration field a map may be a region of interest smaller than its node, and clamping
       would pile the rest into its edge cells.
    9. Hence ``counts.sum() + outside`` is the number of matching events in the node.

    A PATH-LENGTH map (``event="pathlength"``) holds the path photons travel in each voxel, the track-length estimator of
    the fluence: multiplied by any absorption coefficient it is the local absorption rate of any species, present or not,
    and where alpha h << 1 its variance is far below that of the `absorbed` counts.  Lengths are accumulated as fixed-point
    integers, one count = `FLUENCE_UNIT` = 2^-30 of the scene's length unit, so the map is as exact and as independent of
    summation order, launch geometry, carrying and GPU count as the others.  A slot wraps at 2^63 units, about 8.6e9 length
    units; the `outside` slot of a small region of interest inside a large node is the first to get there.  The contract
    (include/pvtrace_hip.h, PvtMapTables, states the same; the kernel and `engine.tally.map_histories` follow it operation
    for operation, without FMA):

    1. A *segment* is one advance of a photon: from world position x along unit direction d for length L, while the
       photon's container is the map's node.  A segment with non-finite L, or L <= 0, adds nothing.
    2. Local start: p_a = ((R[a][0] x + R[a][1] y) + R[a][2] z) + t[a].
    3. Local direction: u_a = (R[a][0] dx + R[a][1] dy) + R[a][2] dz.
    4. R and t are the node's `world_to_local` rows.
    5. Per axis the planes are lower_a + i h_a for i = 0 ... n_a, written ``lower + float(i) * h``.  The cell index c_a
       runs over -1 ... n_a; -1 and n_a are the two half-infinite slabs outside the lattice.
    6. Start: c_a = clamp(floor((p_a - lower_a) / h_a), -1, n_a).  A NaN gives -1.
    7. step_a is the sign of u_a; 0 means the axis never crosses.
    8. The plane ahead is i = c_a + 1 for a positive step and i = c_a for a negative one; it exists when 0 <= i <= n_a, and
       its parameter is (lower_a + i h_a - p_a) / u_a.  Otherwise the parameter is +inf.
    9. The loop is that of a `ConcentrationGrid`'s march.  Start with s = 0.  In each pass tmin is the least of the three
       parameters; sout = max(min(tmin, L), s); the piece sout - s belongs to the current cell; stop when not (sout < L);
       otherwise cross ONE axis whose parameter equals tmin -- ties in the order X, then Y, then Z, the others follow at
       zero length -- and then s = sout.
    10. A piece of length l adds k = int(l * 2^30 + 0.5).  Nothing is added when k = 0.
    11. The piece goes to slot ((cx ny + cy) nz + cz) nw' + iw when every c_a is in 0 ... n_a - 1 and the wavelength bin
        is in range, otherwise to the map's single `outside` slot.
    12. With a wavelength axis iw is a `Histogram`'s bin of the wavelength the photon travels with; out of range means
        the whole segment goes to `outside`.
    13. No clamping: a map may be smaller than its node.
    14. Hence (sum of all slots) * `FLUENCE_UNIT` is the path length travelled inside the node, to within half a unit per
        piece.
    """

    def __init__(self, name, shape, lower, upper, event="absorbed", component=None, wavelength=None):
        _require(event in MAP_EVENTS, f"Unknown volume-map event {event!r}; use one of {sorted(MAP_EVENTS)}")
        self.lattice = Lattice(shape, lower, upper, f"VolumeMap {name!r}")
        if wavelength is not None:
            start, stop, bins = wavelength
            wavelength = Histogram("wavelength", start, stop, bins)
            _require(math.isfinite(wavelength.start) and math.isfinite(wavelength.stop),
                     f"VolumeMap {name!r}: the wavelength range must be finite")
        _require(event != "pathlength" or component is None,
                 f"VolumeMap {name!r}: a path-length map takes no component filter (component={component!r}): the path "
                 f"a photon travels belongs to no component")
        self.name, self.shape, self.lower, self.upper = name, self.lattice.shape, self.lattice.lower, self.lattice.upper
        self.event, self.component, self.wavelength = event, component, wavelength

    @classmethod
    def like(cls, grid, name, **kwargs):
        """A map on the lattice (shape, lower, upper) of a `ConcentrationGrid`, or of anything that exposes a `lattice`."""
        return cls(name, grid.lattice.shape, grid.lattice.lower, grid.lattice.upper, **kwargs)

    @property
    def cell_widths(self):
        """h = (upper - lower) / n per axis, the widths the binning divides by."""
        return self.lattice.h

    @property
    def wavelength_bins(self):
        return self.wavelength.bins if self.wavelength is not None else 0

    @property
    def size(self):
        """Number of slots, the `outside` slot included."""
        cells = self.shape[0] * self.shape[1] * self.shape[2] * max(self.wavelength_bins, 1)
        return cells + 1

    def __repr__(self):
        return "VolumeMap(%r, %r, event=%r)" % (self.name, self.shape, self.event)


class VolumeMapResult:
    """Counts of one `VolumeMap`: `counts` (int64, shape (nx, ny, nz) or (nx, ny, nz, nw)), `outside` (matching events
    of the node that fell outside the lattice or the wavelength range), `total` = counts.sum() + outside, and the
    lattice: `shape`, `lower`, `upper`, `cell_volume`.

    `unit` is what one count stands for: 1 for an event map, `FLUENCE_UNIT` for a path-length map, whose `counts` and
    `outside` are the raw, exact int64 units.  `pathlength` = counts * unit (float64, the path travelled in each cell in
    the scene's length unit) and `fluence` = pathlength / cell_volume: path length per volume, summed over the launch's
    photons -- dividing by the photon count is the caller's job."""

    def __init__(self, spec, slots):
        import numpy as np

        slots = np.asarray(slots, dtype=np.int64)
        if slots.shape != (spec.size,):
            raise ValueError(f"VolumeMap {spec.name!r} has {spec.size} slots, got {slots.shape}")
        self.spec = spec
        nw = spec.wavelength_bins
        self.counts = slots[:-1].reshape(spec.shape + ((nw,) if nw else ()))
        self.outside = int(slots[-1])

    @property
    def total(self):
        return int(self.counts.sum()) + self.outside

    @property
    def unit(self):
        return FLUENCE_UNIT if self.spec.event == "pathlength" else 1

    @property
    def pathlength(self):
        import numpy as np

        return self.counts * np.float64(self.unit)

    @property
    def fluence(self):
        return self.pathlength / self.cell_volume

    @property
    def shape(self):
        return self.spec.shape

    @property
    def lower(self):
        return self.spec.lower

    @property
    def upper(self):
        return self.spec.upper

    @property
    def cell_volume(self):
        h = self.spec.cell_widths
        return h[0] * h[1] * h[2]

    def __repr__(self):
        return f"VolumeMapResult({self.spec.name!r}, total={self.total}, outside={self.outside})"
