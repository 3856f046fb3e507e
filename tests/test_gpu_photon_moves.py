"""A photon that changes lanes keeps every word of its state.  The trace kernel moves a live photon in three ways: through
the LDS exchange buffer when a draining workgroup repacks its survivors, through the same buffer into the tail function
that finishes a workgroup's last wave, and through a carry record from one launch of a stream to the next.  All three
go through one put and one get (trace_body's PVT_PHOTON_PUT / PVT_PHOTON_GET), whose word counts the host shares
(xbuf_words / carry_words).  Which way a photon went must not show in any output, so each cell traces the same 1 536 rays

  whole:    in one launch (the drain repacks, the tail function finishes);
  carried:  as three launches of 512 that park their live photons for the next, closed by a launch of no rays
            (tally cells only: a history launch refuses carrying);
  alone:    with 32 of the rays each in a launch of its own at its `ray_offset` -- one photon goes straight to the tail
            function's prologue -- and the rays between them in launches of a few dozen,

and compares every integer output exactly (first crossings, crossings, bins, map slots, captured rows sorted by index,
histories bit for bit) and the moment sums to the tolerance tests/test_gpu_carry.py holds them to.  The scene is the
edge-recorder slab with a dye of quantum yield 1: photons are re-emitted many times, so workgroups run dry with survivors.

The cells are those of {up to 64 recorders, more (the four-word first-crossing mask)} x {tally, history launch} x {plain
scene, one with captured recorders + a counter histogram + an origin histogram + a volume map} that no other test covers.
The two left out, up to 64 recorders x tally launch, are covered: plain by tests/test_gpu_carry.py (carried, against the
oracle) and tests/test_gpu_park_variant.py, extended by tests/test_gpu_history_counters.py and
tests/test_gpu_origin_properties.py (`..._carried_launches_streams_shards_and_a_ray_alone_...`: carried and alone).

Each cell's launch must also ask for the LDS it asked for before the word counts had one owner: LDS_BYTES is what
`launch_info()["lds_bytes"]` reported for the whole launch of each cell at commit 0657b57, on an MI355X."""
import numpy as np
import pytest

from pvtrace_amd import Absorber, Luminophore, VolumeMap
from pvtrace_amd.engine import Histogram, Recorder, compile_scene, native
from tests.capture_scenes import node
from tests.test_gpu_history_counters import EDGES, edge_slab, same_captures
from tests.test_gpu_origin_properties import spread_rays

pytestmark = pytest.mark.gpu

N, PART, LONE, SEED, MAX_EVENTS = 1536, 512, 32, 41, 128
INT_KEYS = ("rec_distinct", "rec_crossings", "rec_bins", "map_bins")
CELLS = {   # id: (more than 64 recorders, history launch, extended scene)
    "7rec-history-plain": (False, True, False), "7rec-history-extended": (False, True, True),
    "65rec-tally-plain": (True, False, False), "65rec-tally-extended": (True, False, True),
    "65rec-history-plain": (True, True, False), "65rec-history-extended": (True, True, True),
}
LDS_BYTES = {   # launch_info()["lds_bytes"] of each cell's whole launch at commit 0657b57
    "7rec-history-plain": 22096, "7rec-history-extended": 29232,
    "65rec-tally-plain": 31360, "65rec-tally-extended": 38496,
    "65rec-history-plain": 31936, "65rec-history-extended": 39072,
}
# (the exchange buffer IS there: a history launch's 72 slots are one word longer each, 576 bytes -- a launch that did without
# the buffer would ask for the same LDS with and without a history)
assert all(LDS_BYTES[f"65rec-history-{kind}"] - LDS_BYTES[f"65rec-tally-{kind}"] == 72 * 8 for kind in ("plain", "extended"))


def slab(many, extended):
    """The edge-recorder slab with a dye of 21-point spectra (quantum yield 1, absorption and emission overlapping): tables and
    bins small enough that the exchange buffer fits into LDS beside them in every cell, the 25-word slots of the last included."""
    extra = [Recorder(f"again-{k}", event="escaping", facet=list(EDGES.values())[k % 4]) for k in range(58)] if many else []
    scene = edge_slab(counters=False, extra=extra)
    body = node(scene, "LSC")
    x = np.linspace(400.0, 800.0, 21)
    body.geometry.material.components = [
        Luminophore(np.column_stack([x, 8.0 * np.exp(-((x - 540.0) / 70.0) ** 2)]),
                    emission=np.column_stack([x, np.exp(-((x - 600.0) / 40.0) ** 2)]), quantum_yield=1.0, name="dye"),
        Absorber(0.1, name="background")]
    if extended:
        body.volume_maps = [VolumeMap("dose", (4, 4, 2), (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5))]
        for rec in body.recorders + scene.root.recorders:
            rec.capture = N          # (a ray fires a recorder once: no row is ever dropped)
            rec.histograms = []
            if rec.name in ("edge-left", "lost"):
                rec.histograms = [Histogram("emissions", 0, 8, 8), Histogram("origin_wavelength", 400, 800, 20)]
    return scene


class Run:
    """The launches [a, b) of one way of tracing the rays, into one tally set -> every output on the host."""

    def __init__(self, dscene, compiled, rays, history):
        self.dscene, self.compiled, self.rays, self.history = dscene, compiled, rays, history
        self.tallies, self.logs = dscene.new_tallies(), []

    def launch(self, a, b, carry_out=False):
        log = self.dscene.new_event_log(b - a, 1, MAX_EVENTS) if self.history and b > a else None
        part = tuple(t[a:b] for t in self.rays) if b > a else None
        self.dscene.trace(part, b - a, SEED, self.tallies, log=log, ray_offset=a, record_every=1 if log else 0,
                          max_events=MAX_EVENTS, carry_out=carry_out)
        if log:
            self.logs.append((a, b, log))

    def outputs(self):
        import torch

        torch.cuda.synchronize()
        out = {k: np.array(v, copy=True) for k, v in self.tallies.host(0).items()}
        out["captures"] = self.tallies.captures(self.compiled)
        out["histories"] = {}
        for a, b, log in self.logs:
            counts = log["counts"][:b - a].cpu().numpy()
            rows = log["rows"][:(b - a) * MAX_EVENTS].cpu().numpy().reshape(b - a, MAX_EVENTS, native.RECORD_WORDS)
            for j in range(b - a):      # (the last word of a record is its row's number in its own launch's log: not the photon's)
                out["histories"][a + j] = rows[j, :counts[j], :native.RECORD_WORDS - 1].copy()
        return out


def same_outputs(got, want, what):
    for key in INT_KEYS:
        assert (key in got) == (key in want)
        if key in want:
            assert np.array_equal(got[key], want[key]), (what, key)
    assert np.allclose(got["rec_sums"], want["rec_sums"], rtol=1e-11), what
    same_captures(got["captures"], want["captures"])
    for i, rows in got["histories"].items():
        assert np.array_equal(rows, want["histories"][i]), (what, "history of ray", i)


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_a_photon_keeps_its_state_whichever_way_it_is_moved(cell):
    import torch

    many, history, extended = CELLS[cell]
    scene = slab(many, extended)
    compiled = compile_scene(scene)
    assert len(compiled.recorder_names) == (65 if many else 7)
    pos, dirs, wl = spread_rays(scene, None, N, width=4.0)
    dscene = native.DeviceScene(compiled, device=0)
    try:
        dev = torch.device("cuda", 0)
        rays = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pos, dirs, wl))
        whole = Run(dscene, compiled, rays, history)
        whole.launch(0, N)
        info = dscene.launch_info()
        want = whole.outputs()
        print(cell, "variant", info["variant"], "lds_bytes", info["lds_bytes"], "crossings", int(want["rec_crossings"].sum()),
              "longest history", max((len(r) for r in want["histories"].values()), default=0))
        assert info["lds_bytes"] == LDS_BYTES[cell], (cell, info)
        assert (info["variant"] == "rough") == extended
        assert ("map_bins" in want) == extended and (len(want["captures"]) > 0) == extended
        # the photons live many steps: where they are counted, re-emissions; where they are logged, long histories
        assert len(want["histories"]) == (N if history else 0)
        if extended:
            assert max(int(rows.emissions.max()) for rows in want["captures"].values() if len(rows)) >= 3
        if history:
            assert max(len(rows) for rows in want["histories"].values()) >= 16
        if not history:
            carried = Run(dscene, compiled, rays, history)
            for a in range(0, N, PART):
                carried.launch(a, a + PART, carry_out=True)
            torch.cuda.synchronize()
            assert dscene.carry_pending()             # something went through a carry record ...
            carried.launch(N, N)                      # ... and the launch of no rays finishes it
            same_outputs(carried.outputs(), want, (cell, "carried"))
            assert not dscene.carry_pending()
        alone = Run(dscene, compiled, rays, history)
        lone = sorted(set(int(i) for i in np.linspace(0, N - 1, LONE)))
        at = 0
        for i in lone:
            if i > at:
                alone.launch(at, i)
            alone.launch(i, i + 1)
            at = i + 1
        assert at == N and len(lone) == LONE
        same_outputs(alone.outputs(), want, (cell, "alone"))
    finally:
        dscene.close()
