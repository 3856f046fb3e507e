"""`TallyLayout` (pvtrace_amd/engine/tally_set.py): where the recorder accumulators of a tally set lie in the int64 and the
float64 buffer.  The slices below are written out by hand -- they are the referee, not the module under test -- from the
C ABI's contract (include/pvtrace_hip.h: PvtTallies, PvtTraceParams.tally_bundle)."""
import numpy as np
import pytest

from pvtrace_amd.engine import Recorder, compile_scene
from pvtrace_amd.engine.tally_set import TallyLayout
from tests import capture_scenes, scenes


def _bare_recorders():
    scene = scenes.lsc_equivalent(recorders=False)
    capture_scenes.node(scene, "LSC").recorders = scenes.face_recorders(hist=False)
    return scene


def _captured_block():
    scene = capture_scenes.rough_fielded_block()[0]
    capture_scenes.node(scene, "block").recorders = [Recorder("in", event="entering", capture=100),
                                                     Recorder("out", event="escaping"),
                                                     Recorder("lost", event="lost", capture=7)]
    return scene


SCENES = {
    "no recorder": scenes.fresnel_box,
    "recorders without histograms": _bare_recorders,
    "histograms": scenes.lsc_equivalent,
    "a heatmap": scenes.coated_slab,
    "histograms and a heatmap": scenes.kitchen_sink,
    "volume maps": lambda: capture_scenes.rough_fielded_block()[0],
    "captures and volume maps": _captured_block,
}


@pytest.fixture(scope="module", params=sorted(SCENES))
def compiled(request):
    return request.param, compile_scene(SCENES[request.param]())


def test_the_scenes_cover_every_shape_of_a_tally_set():
    made = {name: compile_scene(build()) for name, build in SCENES.items()}
    assert made["no recorder"].rec_node.shape[0] == 0 and made["no recorder"].total_bins == 0
    assert made["recorders without histograms"].rec_node.shape[0] == 10 and made["recorders without histograms"].total_bins == 0
    assert made["histograms"].total_bins == 480 and made["a heatmap"].total_bins == 400
    assert made["histograms and a heatmap"].total_bins > 0
    assert made["volume maps"].has_maps and made["volume maps"].rec_node.shape[0] == 0
    assert made["captures and volume maps"].has_maps and made["captures and volume maps"].capture_rows == 107
    assert [name for name in SCENES if made[name].has_maps] == ["volume maps", "captures and volume maps"]
    assert [name for name in SCENES if made[name].capture_rows] == ["captures and volume maps"]


@pytest.mark.parametrize("sets", [1, 3])
def test_split_returns_the_slices_of_the_abi(compiled, sets):
    name, c = compiled
    layout = TallyLayout(c)
    n_rec, n_bins = int(c.rec_node.shape[0]), int(c.total_bins)
    pad = max(n_rec, 1)
    slots = int(c.map_slots) if c.has_maps else 0
    assert (layout.n_rec, layout.pad, layout.n_bins, layout.map_slots) == (n_rec, pad, n_bins, slots)
    assert layout.stride_i64 == 2 * pad + max(n_bins + slots, 1) and layout.stride_f64 == pad * 8
    assert layout.capture_rows == int(c.capture_rows)
    if not c.has_maps:   # the strides `_kernel.trace_bundle_sets` has always passed to the library
        assert (layout.stride_i64, layout.stride_f64) == (2 * pad + max(n_bins, 1), pad * 8)
    S, F = layout.stride_i64, layout.stride_f64
    ints = np.arange(sets * S, dtype=np.int64)
    sums = np.arange(sets * F, dtype=np.float64)
    for j in range(sets):
        got = layout.split(ints[j * S:(j + 1) * S], sums[j * F:(j + 1) * F])
        want = {"rec_distinct": ints[j * S:j * S + n_rec],
                "rec_crossings": ints[j * S + pad:j * S + pad + n_rec],
                "rec_bins": ints[j * S + 2 * pad:j * S + 2 * pad + n_bins],
                "rec_sums": sums[j * F:j * F + n_rec * 8].reshape(n_rec, 4, 2)}
        if c.has_maps:
            want["map_bins"] = ints[j * S + 2 * pad + n_bins:j * S + 2 * pad + n_bins + slots]
        assert sorted(got) == sorted(want), name   # (`map_bins` is there exactly when the scene has maps)
        for key, value in want.items():
            assert got[key].shape == value.shape and got[key].dtype == value.dtype, (name, key)
            assert np.array_equal(got[key], value), (name, key)
            assert np.shares_memory(got[key], ints if value.dtype == np.int64 else sums) or value.size == 0, (name, key)
        assert got["rec_distinct"].shape == (n_rec,) and got["rec_bins"].shape == (n_bins,)
        assert got["rec_sums"].shape == (n_rec, 4, 2)


def test_split_slices_torch_tensors_the_same_way():
    import torch

    c = compile_scene(_captured_block())
    layout = TallyLayout(c)
    ints = np.arange(layout.stride_i64, dtype=np.int64)
    sums = np.arange(layout.stride_f64, dtype=np.float64)
    want = layout.split(ints, sums)
    got = layout.split(torch.from_numpy(ints), torch.from_numpy(sums))
    assert list(got) == list(want)
    for key, value in want.items():
        assert tuple(got[key].shape) == value.shape and np.array_equal(got[key].numpy(), value), key
        assert np.shares_memory(got[key].numpy(), value) or value.size == 0, key


def test_the_struct_points_at_the_same_blocks():
    c = compile_scene(scenes.lsc_equivalent())
    layout = TallyLayout(c)
    ints = np.arange(layout.stride_i64, dtype=np.int64)
    sums = np.arange(layout.stride_f64, dtype=np.float64)
    tl = layout.struct(ints.ctypes.data, sums.ctypes.data)
    parts = layout.split(ints, sums)
    assert tl.rec_distinct[0] == parts["rec_distinct"][0] and tl.rec_crossings[0] == parts["rec_crossings"][0]
    assert tl.rec_bins[0] == parts["rec_bins"][0] and tl.rec_sums[5] == 5.0


def test_a_tally_set_on_host_tensors_zeroes_adds_and_reads_set_by_set():
    """`TallySet` itself, on CPU tensors: the buffers' sizes, `host` of one set and of the first few, `add_`, and `zero_`
    with and without the capture cursors."""
    import torch

    from pvtrace_amd.engine.tally_set import TallySet

    c = compile_scene(_captured_block())
    cpu = torch.device("cpu")
    t, u = TallySet(c, cpu, sets=3), TallySet(c, cpu, sets=3, captures=False)
    S, F = t.layout.stride_i64, t.layout.stride_f64
    assert t.sets == 3 and t.ints.shape == (3 * S,) and t.sums.shape == (3 * F,)
    assert t.cap_rows.shape == (3 * 107, 12) and t.cap_cursor.shape == (3 * 3,) and t.capture_struct is not None
    assert u.cap_rows is None and u.cap_cursor is None and u.capture_struct is None
    assert not t.ints.any() and not t.sums.any() and not t.cap_cursor.any()
    u.ints += torch.arange(3 * S)
    u.sums += torch.arange(3 * F, dtype=torch.float64)
    t.add_(u)
    t.add_(u)
    one = t.host(2)
    assert np.array_equal(one["rec_distinct"], 2 * np.arange(2 * S, 2 * S + 3))
    assert np.array_equal(one["rec_sums"], 2.0 * np.arange(2 * F, 2 * F + 24).reshape(3, 4, 2))
    first_two = t.host(sets=2)
    assert len(first_two) == 2 and len(t.host()) == 3
    assert np.array_equal(first_two[1]["rec_crossings"], 2 * np.arange(S + 3, S + 6))
    assert np.array_equal(first_two[1]["map_bins"], 2 * np.arange(S + 6, 2 * S))
    t.cap_cursor += 5
    t.zero_(captures=False)
    assert not t.ints.any() and not t.sums.any() and t.cap_cursor.eq(5).all()
    t.ints += 1
    t.zero_(tallies=False)
    assert t.ints.eq(1).all() and not t.cap_cursor.any()
    t.cap_cursor += 5
    t.zero_()
    assert not t.ints.any() and not t.cap_cursor.any()
    u.zero_()   # (no cursors to forget)
    assert not u.ints.any() and not u.sums.any()
    with pytest.raises(ValueError, match="capture rows each exceed"):
        TallySet(c, cpu, sets=(1 << 24) // 107 + 1)
