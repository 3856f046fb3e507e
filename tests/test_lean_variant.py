"""The lean kernel family (trace_kernel_lean_w4: trace_body with LEAN) runs scenes the library
has PROVEN plain from their packed tables (pvt_scene_pack.h: prove_lean).  Here, without a GPU: which scenes the proof
accepts, that each fact the variant holds as a constant disqualifies a scene on its own, and what the built lean
kernel costs in registers and code next to the generic headline variant."""
import functools

import numpy as np
import pytest

from benchmarks import configs
from pvtrace_amd import (
    Absorber, Box, Coating, CoatedSurfaceDelegate, Cylinder, Light, Luminophore, Material, Node, PhaseFunctionTable,
    ReflectivityTable, RefractiveIndexTable, Scatterer, Scene, Sphere, Surface, cone,
)
from pvtrace_amd.data import lumogen_f_red_305
from pvtrace_amd.engine import Recorder, compile_scene, native
from pvtrace_amd.material import Cone, HenyeyGreenstein
from tests import scenes
from tests.test_kernel_registers import CALL_FRAME, LIB

X = np.arange(400, 800)


def _dye(**kw):
    return Luminophore(coefficient=np.column_stack((X, lumogen_f_red_305.absorption(X) * 10.0)),
                       emission=np.column_stack((X, lumogen_f_red_305.emission(X))), quantum_yield=1.0,
                       name=kw.pop("name", "dye"), **kw)


def plain(components=None, index=1.5, surface=None, recorders=None, more=None):
    """A slab in a box world: lean as it stands; every argument is a way of making it something else."""
    world = Node(name="World", geometry=Box((500.0, 500.0, 100.0), material=Material(refractive_index=1.0)))
    components = [_dye(), Absorber(0.1, name="Background")] if components is None else components
    material = Material(refractive_index=index, components=components, **({} if surface is None else {"surface": surface}))
    slab = Node(name="LSC", parent=world, geometry=Box((5.0, 5.0, 1.0), material=material),
                recorders=scenes.face_recorders() if recorders is None else recorders)
    if more is not None:
        more(world, slab)
    light = Node(name="Light", parent=world, light=Light(direction=functools.partial(cone, np.radians(20)), name="Light"))
    light.location = (0.0, 0.0, 5.0)
    light.rotate(np.radians(180), (1, 0, 0))
    return Scene(world)


def lean(scene):
    if not native.library_built():
        pytest.skip("library not built")
    return native.lean_check(compile_scene(scene))


def lean_kind(scene):
    """0: not lean; 1: lean, some spectrum on a grid that is even only up to rounding (its kernels search the tables);
    2: lean, every spectrum a constant or even bit for bit (the kernels without searches: the headline's)."""
    if not native.library_built():
        pytest.skip("library not built")
    return native.lean_kind(compile_scene(scene))


@pytest.mark.parametrize("name, build", [
    ("LSC((5, 5, 1)) + face_recorders()", configs.cfg2_lsc),
    ("lsc_equivalent", scenes.lsc_equivalent),
    ("fresnel_box", scenes.fresnel_box),
    ("touching_boxes", scenes.touching_boxes),
    ("the plain slab of this file", plain),
])
def test_plain_scenes_are_lean(name, build):
    assert lean(build()), name
    assert lean_kind(build()) == 2, name   # (integer-spaced or constant spectra: none of them is searched)


def test_bench_slab_is_lean():
    """bench_slab's spectra are np.linspace(300, 1000, 200): an even grid, but only up to rounding -- the spacing 700/199
    is no double, so the packer's even_w proof rejects them (CD_ABS_W and CD_EMS_W are NaN) and their intervals have no
    one known divisor.  The scene is lean all the same, of the kind whose kernels search the tables (guide bracket and
    bisection, as the generic ones do; the step-table path alone is left out)."""
    assert lean(scenes.bench_slab())
    assert lean(scenes.bench_slab(recorders=True))
    assert lean_kind(scenes.bench_slab()) == 1


def _child(geometry, rotate=None):
    def more(world, slab):
        node = Node(name="extra", parent=world, geometry=geometry)
        node.location = (20.0, 0.0, 0.0)
        if rotate:
            node.rotate(*rotate)
    return more


GLASS = Material(refractive_index=1.5)
IRREGULAR = np.array([400.0, 450.0, 520.0, 600.0, 800.0])


def test_a_sphere_node_is_not_lean():
    assert not lean(plain(more=_child(Sphere(1.0, material=GLASS))))


def test_a_cylinder_node_is_not_lean():
    assert not lean(plain(more=_child(Cylinder(2.0, 0.5, material=GLASS))))


def test_a_rotated_box_is_not_lean():
    assert lean(plain(more=_child(Box((1.0, 1.0, 1.0), material=GLASS))))   # (the same child, unrotated: lean)
    assert not lean(plain(more=_child(Box((1.0, 1.0, 1.0), material=GLASS), rotate=(0.3, (0.0, 1.0, 0.0)))))


def test_a_coating_is_not_lean():
    mirror = Surface(delegate=CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=1.0)]))
    assert not lean(plain(surface=mirror))


def test_an_index_table_is_not_lean():
    assert not lean(plain(index=RefractiveIndexTable([400.0, 800.0], [1.4, 1.6])))


def test_a_reflectivity_table_is_not_lean():
    table = ReflectivityTable([300.0, 1000.0], [1.0, 0.0])
    assert not lean(plain(surface=Surface(delegate=CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=table)]))))


def test_a_phase_table_is_not_lean():
    table = PhaseFunctionTable([0.0, 60.0, 120.0, 180.0], [3.0, 1.0, 0.5, 0.2])
    assert not lean(plain(components=[_dye(phase_function=table)]))


def test_a_henyey_greenstein_component_is_not_lean():
    assert not lean(plain(components=[_dye(phase_function=HenyeyGreenstein(0.7))]))


def test_a_cone_component_is_not_lean():
    assert not lean(plain(components=[_dye(phase_function=Cone(0.5))]))


def test_a_scatterer_is_not_lean():
    assert not lean(plain(components=[_dye(), Scatterer(0.4, name="fog")]))


def test_three_components_in_one_container_are_not_lean():
    two = [_dye(), Absorber(0.1, name="a")]
    assert lean(plain(components=two))
    assert not lean(plain(components=two + [Absorber(0.2, name="b")]))


def test_a_spectrum_off_the_even_grid_is_not_lean():
    even_to_rounding = np.linspace(400.0, 800.0, 7)   # (spacing 400/6: no double -- lean, of the searching kind)
    assert lean_kind(plain(components=[Absorber(np.column_stack((even_to_rounding, 0.1 + 0.0 * even_to_rounding)), name="host")])) == 1
    nudged = even_to_rounding.copy()
    nudged[3] += 1e-6                                 # one abscissa a millionth of a nanometre off the grid
    assert not lean(plain(components=[Absorber(np.column_stack((nudged, 0.1 + 0.0 * nudged)), name="host")]))
    assert not lean(plain(components=[Absorber(np.column_stack((IRREGULAR, 0.1 + 0.0 * IRREGULAR)), name="host")]))
    uneven = Luminophore(coefficient=np.column_stack((X, lumogen_f_red_305.absorption(X) * 10.0)),
                         emission=np.column_stack((IRREGULAR, [0.0, 1.0, 3.0, 1.0, 0.0])), quantum_yield=1.0, name="dye")
    assert not lean(plain(components=[uneven]))


def test_a_recorder_with_a_source_filter_is_not_lean():
    recorders = scenes.face_recorders() + [Recorder("lamp light out", event="escaping", source="lights")]
    assert not lean(plain(recorders=recorders))


def test_more_than_64_recorders_are_not_lean():
    assert lean(plain(recorders=[Recorder(f"lost-{i}", event="lost") for i in range(64)]))
    assert not lean(plain(recorders=[Recorder(f"lost-{i}", event="lost") for i in range(65)]))


def test_a_mesh_is_not_lean():
    assert not lean(scenes.mesh_lsc())


def test_a_node_grid_is_not_lean():
    scene = configs.tiles_lsc(3)   # ten unrotated boxes of the headline's material: only the grid stands in the way
    if not native.library_built():
        pytest.skip("library not built")
    assert native.node_grid_plan(compile_scene(scene)) is not None
    assert not lean(scene)


def test_budgets_of_the_built_lean_kernel():
    import __graft_entry__ as entry

    kernels = entry.kernel_metadata(LIB)
    if not kernels:
        pytest.skip("library or LLVM binutils not present")
    family = {n: m for n, m in kernels.items() if "trace_kernel_lean_w4" in n}
    assert len(family) == 8                               # {tally, history} x {rays, emitter} x {spectra searched, all even}
    assert not any("trace_kernel_w4" in n for n in family)   # (what tests/test_kernel_registers.py counts stays what it was)
    lean_k = [m for n, m in family.items() if "lean_w4ILb0ELb0ELb1E" in n]   # tally, rays in, every spectrum even: the headline's
    searching = [m for n, m in family.items() if "lean_w4ILb0ELb0ELb0E" in n]
    assert len(searching) == 1 and lean_k[0]["text_bytes"] <= searching[0]["text_bytes"] <= 58 * 1024
    generic = [m for n, m in kernels.items() if "trace_kernel_w4ILb0ELi1ELi1ELb0E" in n]
    assert len(lean_k) == 1 and len(generic) == 1
    lean_k, generic = lean_k[0], generic[0]
    print("lean", lean_k, "generic", generic)
    assert lean_k["vgpr_count"] <= 128 and lean_k["vgpr_spill_count"] == 0
    assert lean_k["private_segment_fixed_size"] <= CALL_FRAME
    assert lean_k["text_bytes"] <= generic["text_bytes"]
    assert lean_k["sgpr_spill_count"] <= generic["sgpr_spill_count"]
    for name, m in family.items():   # four waves per SIMD, the history pair under the analytic variants' own allowance
        assert m["vgpr_count"] <= 128 and m["vgpr_spill_count"] <= (1 if "lean_w4ILb1E" in name else 0), (name, m)
