"""The four lattice features in ONE node, each on a lattice of its own: a concentration field on 3 x 2 x 2 cells, an
`absorbed` map on 2 x 3 x 1 cells smaller than the node, a `pathlength` map on 1 x 2 x 3 cells with other bounds, and a
patterned coating on the top face with a 4 x 4 x 1 mask and unbounded z.  The packer writes a field record, two map records and
a pattern record, and the kernel reads each at its own offsets (kFr*, kMr*, kPr*); the shapes differ so that one record's
words read through another record's offsets could not pass.

The referees are the host's rules (pvtrace_amd/lattice.py through `map_histories`, `path_map_slots`, `pattern_cell`) run on
the kernel's OWN histories: the event map's slots integer for integer, the path map's within one unit per piece of the
slot, every surface event at the top face DETECT exactly where the mask is set.  The flattener accepts the combination:
one scene, not two."""
import numpy as np
import pytest

from pvtrace_amd import (
    Absorber, Box, CoatedSurfaceDelegate, Coating, CoatingPattern, ConcentrationGrid, Event, Light, Material, Node, Scene,
    Surface, VolumeMap, isotropic, pattern_cell,
)
from pvtrace_amd.engine import Recorder, Session, map_histories
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.engine.tally import path_map_slots
from tests.capture_scenes import submit
from tests.pattern_scenes import local_points, third_mask

pytestmark = pytest.mark.gpu

N, SEED, MAX_EVENTS = 20_000, 7, 128
TOP = (0.0, 0.0, 1.0)
SHIFT = (1.0, -2.0, 0.5)
SURFACE = (Event.REFLECT.value, Event.TRANSMIT.value, Event.DETECT.value)


def scene_of_four_lattices():
    ix, iy, iz = np.indices((3, 2, 2))
    grid = ConcentrationGrid(0.25 + ((ix + 2 * iy + 3 * iz) % 4) * 0.5, (-5.0, -5.0, -1.0), (5.0, 5.0, 1.0))
    pattern = CoatingPattern(third_mask((4, 4, 1)), (-4.0, -3.5, None), (4.5, 4.0, None))      # smaller than the face
    detector = Coating(TOP, reflectivity=0.0, absorptivity=1.0, transmission="matched", pattern=pattern)
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    box = Node(name="box", parent=world, geometry=Box((10.0, 10.0, 2.0), material=Material(
        refractive_index=1.5, components=[Absorber(0.2, name="tint", concentration=grid)],
        surface=Surface(delegate=CoatedSurfaceDelegate([detector])))))
    box.rotate(0.3, (0.0, 1.0, 0.0))
    box.location = SHIFT
    box.volume_maps = [VolumeMap("dose", (2, 3, 1), (-2.0, -3.0, -0.5), (3.0, 2.0, 0.75), event="absorbed"),
                       VolumeMap("path", (1, 2, 3), (-4.0, -3.0, -0.75), (3.0, 6.5, 1.25), event="pathlength")]
    box.recorders = [Recorder("detected", event="detected"), Recorder("lost", event="lost")]
    world.recorders = [Recorder("exit", event="exit")]
    lamp = Node(name="lamp", parent=world, light=Light(direction=isotropic, name="lamp"))
    lamp.location = (SHIFT[0] + 0.4, SHIFT[1] + 0.3, SHIFT[2] - 0.1)
    return Scene(world), pattern


def test_field_event_map_path_map_and_pattern_in_one_node_each_follow_the_host_rule():
    scene, pattern = scene_of_four_lattices()
    pos, dirs, wl, _ = emit_bundle(scene, N, seed=3)
    with Session(scene, emission="host") as s:
        hist = submit(s, (pos, dirs, wl), SEED, record_every=1, max_events=MAX_EVENTS)
        assert int(np.asarray(hist.data["counts"]).max()) < MAX_EVENTS          # no history was cut
        columns = {k: np.asarray(hist.data[k]).copy() for k in ("counts", "kind", "hit", "position", "normal", "map_bins")}
        kernel = hist.volume_maps
        detected = hist.recorders["detected"].crossings
        compiled = hist.compiled
        histories = list(hist.histories())
    assert compiled.has_fields and compiled.has_coating_patterns and compiled.n_maps == 2
    box = compiled.node_names.index("box")

    # 1. the event map: integer for integer
    host = map_histories(compiled, histories)
    assert np.array_equal(kernel["dose"].counts, host["dose"].counts) and kernel["dose"].outside == host["dose"].outside
    assert kernel["dose"].counts.min() > 0 and kernel["dose"].outside > 0       # every cell was met, and the rest of the node

    # 2. the path map: within the pieces of each slot
    want, pieces = path_map_slots(compiled, histories)
    got = columns["map_bins"].astype(np.int64)
    at = int(compiled.map_offset[compiled.map_names.index("path")])
    size = kernel["path"].spec.size
    worst = int(np.abs(got - want)[at:at + size].max())
    print(f"path map: worst |GPU - host| {worst} units; pieces per slot up to {int(pieces.max())}")
    assert np.all(np.abs(got - want)[at:at + size] <= pieces[at:at + size])
    assert np.all(want[:at] == 0) and kernel["path"].counts.min() > 0 and kernel["path"].outside > 0

    # 3. the pattern: every surface event at the top face is DETECT exactly where the mask is set
    rows = np.flatnonzero((np.arange(MAX_EVENTS)[None, :] < columns["counts"][:, None]).reshape(-1))
    kind, hit = columns["kind"][rows], columns["hit"][rows]
    position, normal = columns["position"].reshape(-1, 3)[rows], columns["normal"].reshape(-1, 3)[rows]
    local_normal = normal @ np.asarray(compiled.world_to_local[box])[:3, :3].T
    top = np.isin(kind, SURFACE) & (hit == box) & np.all(np.abs(local_normal - np.asarray(TOP)) <= 1e-8 + 1e-5 * np.abs(np.asarray(TOP)) + 1e-12, axis=1)
    flat = pattern.mask.reshape(-1)
    covered = np.array([slot is not None and bool(flat[slot])
                        for slot in (pattern_cell(pattern, p) for p in local_points(scene, "box", position[top]))])
    assert np.array_equal(kind[top] == Event.DETECT.value, covered)
    assert not np.any(kind[~top] == Event.DETECT.value)
    assert covered.sum() > 200 and (~covered).sum() > 200 and int(covered.sum()) == detected
