"""The solo entries (trace_kernel_solo_park / trace_kernel_solo_fin: trace_body with SOLO) run the
tally launches of scenes the library has PROVEN solo from their packed tables (pvt_scene_pack.h: prove_solo): lean, and ONE
unrotated box inside a lazy root that holds no component and carries no recorder.  Here, without a GPU, through
pvt_scene_solo_check: which scenes the proof accepts, that each clause refuses a scene on its own and is named, and that
PVT_NO_SOLO is honoured."""
import numpy as np
import pytest

from benchmarks import configs
from pvtrace_amd import Absorber, Box, Material, Node
from pvtrace_amd.engine import Recorder, compile_scene, native
from tests import scenes
from tests.test_lean_variant import GLASS, plain


@pytest.fixture(autouse=True)
def built(monkeypatch):
    if not native.library_built():
        pytest.skip("library not built")
    monkeypatch.delenv("PVT_NO_SOLO", raising=False)
    monkeypatch.delenv("PVT_NO_FUSED_EXIT", raising=False)


def solo(scene):
    return native.solo_check(compile_scene(scene))


def refusal(scene):
    return native.solo_refusal(compile_scene(scene))


@pytest.mark.parametrize("name, build", [
    ("the headline: LSC((5, 5, 1)) + face_recorders()", configs.cfg2_lsc),
    ("tiles1", lambda: configs.tiles_lsc(1)),
    ("bench_slab", scenes.bench_slab),
    ("fresnel_box", scenes.fresnel_box),
    ("lsc_equivalent", scenes.lsc_equivalent),
    ("the plain slab of tests/test_lean_variant.py", plain),
])
def test_one_box_in_a_world_is_solo(name, build):
    assert solo(build()), name
    assert refusal(build()) is None, name


def test_two_boxes_are_not_solo():
    def more(world, slab):
        node = Node(name="extra", parent=world, geometry=Box((1.0, 1.0, 1.0), material=GLASS))
        node.location = (20.0, 0.0, 0.0)
    scene = plain(more=more)
    assert native.lean_check(compile_scene(scene))   # (lean all the same: the lean loop is where it stays)
    assert not solo(scene)
    assert "one node inside the root" in refusal(scene)
    assert not solo(scenes.touching_boxes())


def test_a_recorder_on_the_root_is_not_solo():
    def more(world, slab):
        world.recorders = [Recorder("entering the world", event="entering")]
    scene = plain(more=more)
    assert not solo(scene)
    assert refusal(scene) == "a recorder on the root"


def test_an_exit_recorder_on_the_root_is_not_solo():
    def more(world, slab):
        world.recorders = [Recorder("exit", event="exit")]
    scene = plain(more=more)
    assert not solo(scene)
    assert refusal(scene) == "a recorder on the root"


def test_an_absorber_in_the_world_is_not_solo():
    def more(world, slab):
        world.geometry.material = Material(refractive_index=1.0, components=[Absorber(0.01, name="haze")])
    scene = plain(more=more)
    assert native.lean_check(compile_scene(scene))
    assert not solo(scene)
    assert refusal(scene) == "a component in the root"


def test_a_scene_that_is_not_lean_is_not_solo():
    irregular = np.array([400.0, 450.0, 520.0, 600.0, 800.0])
    scene = plain(components=[Absorber(np.column_stack((irregular, 0.1 + 0.0 * irregular)), name="host")])
    assert not native.lean_check(compile_scene(scene))
    assert not solo(scene)
    assert refusal(scene) == "the scene is not lean"
    assert not solo(scenes.mesh_lsc())


def test_without_the_fused_exit_a_scene_is_not_solo(monkeypatch):
    monkeypatch.setenv("PVT_NO_FUSED_EXIT", "1")
    assert not solo(plain())
    assert "fused exit" in refusal(plain())


def test_the_switch_is_honoured(monkeypatch):
    assert solo(configs.cfg2_lsc())
    monkeypatch.setenv("PVT_NO_SOLO", "1")
    assert not solo(configs.cfg2_lsc())
    assert refusal(configs.cfg2_lsc()) == "PVT_NO_SOLO is set"
    assert native.lean_check(compile_scene(configs.cfg2_lsc()))   # (the lean family is not what the switch is about)


def test_the_new_entries_are_declared_and_bound():
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvtrace_hip.h")).read()
    for symbol in ("pvt_scene_solo", "pvt_scene_solo_check"):
        assert f"int {symbol}(" in header and symbol in native.ABI_SYMBOLS
        assert hasattr(native.load_library(), symbol)
