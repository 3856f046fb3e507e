"""The lean family's parking entries (`trace_kernel_lean_park`): a tally launch that parks its survivors for its
successor on the stream (PVT_FLAG_CARRY_OUT) runs the family's kernel compiled without the drain rendezvous and the
tail function, which it cannot reach.  Which entry a launch runs must not show in a single photon's history: carried
streams of the headline scene are held to the CPU referee (same seeds, same global ray indices) and to the same job
without carrying, which never parks and runs `trace_kernel_lean_w4` with its tail."""
import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd.engine import BundlePipeline, compile_scene, native
from pvtrace_amd.engine.emit import EmitterTables, emit_bundle

pytestmark = pytest.mark.gpu
INT_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
SEED, MAXSTEPS = 12345, 1000
PARK, USUAL = "trace_kernel_lean_park", "trace_kernel_lean_w4"
STREAM = (20_000,) * 7       # test 1: the last three close their streams, the last one is the tail


class Headline:
    """cfg2 with 140 000 host-emitted rays on the device, and the referee's tallies of any leading part of them."""

    def __init__(self):
        import torch

        from benchmarks.configs import cfg2_lsc

        self.scene = cfg2_lsc()
        self.compiled = compile_scene(self.scene)
        self.host_rays = emit_bundle(self.scene, sum(STREAM), seed=1)[:3]
        self.rays = tuple(torch.from_numpy(a).to(torch.device("cuda", 0)) for a in self.host_rays)
        self._referee = {}

    def referee(self, n):
        """(tallies, loop count) of rays [0, n) -- computed once per n, never modified."""
        if n not in self._referee:
            pos, dirs, wl = (a[:n] for a in self.host_rays)
            cpu = O.trace_bundle(self.compiled, pos, dirs, wl, SEED, MAXSTEPS, 128, 0, 8, 0, math_mode=O.MATH_PORTABLE)
            self._referee[n] = (cpu, O.last_steps())
        return self._referee[n]


@pytest.fixture(scope="module")
def headline():
    return Headline()


def run_stream(dscene, rays, sizes, carry, depth=3, closing=None, tail=True, emit_seed=0):
    """The bundles `sizes` through a BundlePipeline -> (totals, [entry of each launch], [grid of each launch]).
    `closing`: how many bundles at the end close their streams (default: `depth`); `tail`: the last one is a tail."""
    closing = depth if closing is None else closing
    pipe = BundlePipeline(dscene, depth=depth, carry=carry)
    entries, grids, at = [], [], 0
    try:
        for k, m in enumerate(sizes):
            part = None if rays is None else tuple(t[at:at + m] for t in rays)
            pipe.submit(part, m, seed=SEED, ray_offset=at, emit_seed=emit_seed, maxsteps=MAXSTEPS, timed=False,
                        closing=k >= len(sizes) - closing, tail=tail and k == len(sizes) - 1)
            info = dscene.launch_info()
            assert info["variant"] == "lean"
            entries.append(info["entry"])
            grids.append(info["grid"])
            at += m
        totals = {k: np.asarray(v).copy() for k, v in pipe.totals_host().items()}
        last = dscene.launch_info()["entry"]    # (of the launch that finished what was parked, if there was one)
    finally:
        pipe.close()
    return totals, entries, grids, last


def assert_equal_tallies(got, want, what):
    for key in INT_KEYS:
        assert np.array_equal(got[key], want[key]), (what, key)
    assert np.allclose(got["rec_sums"], want["rec_sums"], rtol=1e-11, atol=0), what


def test_a_carried_stream_equals_the_referee_and_the_uncarried_job_and_counts_its_steps(headline):
    """Equality of the tallies, which entry each launch ran, and the kernel's own step counters, over one stream."""
    cpu, want_steps = headline.referee(sum(STREAM))
    dscene = native.DeviceScene(headline.compiled, device=0)
    try:
        dscene.counters(reset=True)
        carried, entries, _, _ = run_stream(dscene, headline.rays, STREAM, carry=True)
        c = dscene.counters(reset=True)
        plain, plain_entries, _, _ = run_stream(dscene, headline.rays, STREAM, carry=False)
        c_plain = dscene.counters(reset=True)
    finally:
        dscene.close()
    print("entries:", entries, plain_entries, "steps:", c["steps"], c_plain["steps"], want_steps)
    assert entries == [PARK] * 4 + [USUAL] * 3      # the parking launches ran the new entry, the closing ones the tail's
    assert plain_entries == [USUAL] * 7             # a job that never parks never runs it
    assert_equal_tallies(carried, cpu, "carried stream against the referee")
    assert_equal_tallies(carried, plain, "carried stream against the same job without carrying")
    assert cpu["rec_distinct"].sum() > 0
    assert c["lane_steps"] + c["fused_exits"] == want_steps, (c, want_steps)
    assert c_plain["lane_steps"] + c_plain["fused_exits"] == want_steps, (c_plain, want_steps)


def test_a_launch_too_wide_to_park_runs_the_entry_that_finishes_its_photons(headline):
    """bind_carry clears `carry_out` of a launch wider than carry_cap / 256 workgroups (4 per CU): the kernel is chosen
    after that, so such a launch gets `trace_kernel_lean_w4` and leaves nothing parked."""
    import torch

    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = num_cu * 6 * 256 + 4096
    rays = tuple(t.repeat((n + t.shape[0] - 1) // t.shape[0], *([1] * (t.dim() - 1)))[:n].contiguous() for t in headline.rays)
    dscene = native.DeviceScene(headline.compiled, device=0)
    try:
        tallies = dscene.new_tallies()
        dscene.trace(rays, n, SEED, tallies, carry_out=True, workgroups_per_cu=6)
        info = dscene.launch_info()
        torch.cuda.synchronize()
        assert info["grid"] > 4 * num_cu, info
        assert info["entry"] == USUAL and not dscene.carry_pending(), info
        # ... while the same rays at the usual width do park, through the new entry
        dscene.trace(rays, n, SEED, tallies, carry_out=True, workgroups_per_cu=4)
        info = dscene.launch_info()
        assert info["grid"] == 4 * num_cu and info["entry"] == PARK and dscene.carry_pending(), info
        dscene.trace(None, 0, 0, tallies)
        assert dscene.launch_info()["entry"] == USUAL
        # both launches traced the same rays with the same seeds: together they tally twice what one launch that
        # never heard of carrying does
        once = dscene.new_tallies()
        dscene.trace(rays, n, SEED, once)
        torch.cuda.synchronize()
        got, want = tallies.host(0), once.host(0)
        for key in INT_KEYS:
            assert np.array_equal(got[key], 2 * want[key]), key
        assert want["rec_distinct"].sum() > 0
    finally:
        dscene.close()


@pytest.mark.parametrize("m", [1, 63, 100])
def test_small_bundles(headline, m):
    """Bundles of one photon, of one short of a wave, and of fewer rays than one claim per wave (most waves park nothing)."""
    sizes = (m,) * 7
    cpu, _ = headline.referee(sum(sizes))
    dscene = native.DeviceScene(headline.compiled, device=0)
    try:
        carried, entries, _, _ = run_stream(dscene, headline.rays, sizes, carry=True)
        plain, plain_entries, _, _ = run_stream(dscene, headline.rays, sizes, carry=False)
    finally:
        dscene.close()
    assert entries == [PARK] * 4 + [USUAL] * 3 and plain_entries == [USUAL] * 7
    assert_equal_tallies(carried, cpu, f"bundles of {m} against the referee")
    assert_equal_tallies(carried, plain, f"bundles of {m} against the same job without carrying")


def test_a_middle_bundle_smaller_than_what_its_predecessor_parked(headline):
    """One stream: 20 000 photons park their survivors, the next bundle brings 10 rays -- `size_grid` widens it to the
    carried count, it resumes everything, parks again (the new entry both times), and the last bundle finishes the job."""
    sizes = (20_000, 10, 20_000)
    cpu, _ = headline.referee(sum(sizes))
    dscene = native.DeviceScene(headline.compiled, device=0)
    try:
        carried, entries, grids, _ = run_stream(dscene, headline.rays, sizes, carry=True, depth=1)
        plain, plain_entries, plain_grids, _ = run_stream(dscene, headline.rays, sizes, carry=False, depth=1)
    finally:
        dscene.close()
    assert entries == [PARK, PARK, USUAL] and plain_entries == [USUAL] * 3
    # (wide enough for one lane per photon its predecessor may have parked, plus its own ten rays)
    assert grids[1] >= grids[0] > 1 and plain_grids[1] == 1, (grids, plain_grids)
    assert_equal_tallies(carried, cpu, "narrow middle bundle against the referee")
    assert_equal_tallies(carried, plain, "narrow middle bundle against the same job without carrying")


def test_parked_photons_drained_by_reduce_totals_without_a_closing_bundle(headline):
    """No bundle closes its stream: every launch parks, and `reduce_totals()` -> `finish_parked` drains the three streams
    through the usual entry (launches without rays)."""
    sizes = (20_000,) * 4
    cpu, _ = headline.referee(sum(sizes))
    dscene = native.DeviceScene(headline.compiled, device=0)
    try:
        carried, entries, _, last = run_stream(dscene, headline.rays, sizes, carry=True, closing=0, tail=False)
    finally:
        dscene.close()
    assert entries == [PARK] * 4 and last == USUAL
    assert_equal_tallies(carried, cpu, "drained by reduce_totals against the referee")


def test_lds_of_the_headline_launch_fits_five_workgroups_per_cu(headline):
    import torch

    dscene = native.DeviceScene(headline.compiled, device=0)
    try:
        dscene.trace(tuple(t[:4096] for t in headline.rays), 4096, SEED, dscene.new_tallies(), carry_out=True)
        info = dscene.launch_info()
        dscene.trace(None, 0, 0, dscene.new_tallies())
        torch.cuda.synchronize()
    finally:
        dscene.close()
    assert info["entry"] == PARK and 0 < info["lds_bytes"] * 5 <= 160 * 1024, info


def test_the_emitter_entries_on_two_nodes():
    """tiles1 (world + one slab: lean, device emission): 4 bundles of 20 000 photons sampled on the device, against the
    referee on the very rays the device samples."""
    from benchmarks.configs import tiles_lsc

    scene = tiles_lsc(1)
    compiled = compile_scene(scene)
    sizes, emit_seed = (20_000,) * 4, 6
    dscene = native.DeviceScene(compiled, device=0, emitter=EmitterTables(scene))
    try:
        pos, dirs, wl = (t.cpu().numpy() for t in dscene.emit(sum(sizes), emit_seed))
        # (one stream: every parking launch after the first also resumes what its predecessor parked)
        carried, entries, _, _ = run_stream(dscene, None, sizes, carry=True, depth=1, emit_seed=emit_seed)
        plain, plain_entries, _, _ = run_stream(dscene, None, sizes, carry=False, depth=1, emit_seed=emit_seed)
    finally:
        dscene.close()
    cpu = O.trace_bundle(compiled, pos, dirs, wl, SEED, MAXSTEPS, 128, 0, 8, 0, math_mode=O.MATH_PORTABLE)
    assert entries == [PARK] * 3 + [USUAL] and plain_entries == [USUAL] * 4
    assert cpu["rec_distinct"].sum() > 0
    assert_equal_tallies(carried, cpu, "device emission against the referee")
    assert_equal_tallies(carried, plain, "device emission against the same job without carrying")
