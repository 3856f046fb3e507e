"""Coating reflectivity tables R(wavelength, angle of incidence) without a GPU: the public `ReflectivityTable` and its
validation, the host delegate against a direct evaluation of the bilinear rule, the flattener's pooled tables, the
neutral state of the new tables in every other scene, the C struct's appended fields against the header, and
hand-traced rays through the per-ray host tracer."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from pvtrace_amd import (
    Box, CoatedSurfaceDelegate, Coating, Material, Node, Ray, ReflectivityTable, Scene, Surface,
)
from pvtrace_amd.engine import compile_scene
from tests import coating_table_scene as S
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvtrace_hip.h")

WL = np.array([400.0, 500.0, 550.0, 700.0, 900.0])
ANG = np.array([0.0, 15.0, 45.0, 70.0, 90.0])
VAL = np.random.default_rng(3).uniform(0.0, 1.0, size=(5, 5))


# -- API -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs, words", [
    (dict(wavelength=[500.0, 400.0], values=[0.1, 0.2]), "wavelength"),
    (dict(wavelength=[400.0, 400.0], values=[0.1, 0.2]), "wavelength"),
    (dict(wavelength=[400.0, np.nan], values=[0.1, 0.2]), "wavelength"),
    (dict(wavelength=[], values=[]), "wavelength"),
    (dict(wavelength=[[400.0, 500.0]], values=[0.1, 0.2]), "wavelength"),
    (dict(wavelength=[400.0, 500.0], values=[0.1, 0.2, 0.3]), "shape"),
    (dict(wavelength=[400.0, 500.0], values=[[0.1, 0.2]]), "shape"),
    (dict(wavelength=[400.0, 500.0], values=[0.1, 1.2]), "[0, 1]"),
    (dict(wavelength=[400.0, 500.0], values=[-0.1, 0.2]), "[0, 1]"),
    (dict(wavelength=[400.0, 500.0], values=[np.nan, 0.2]), "[0, 1]"),
    (dict(wavelength=[400.0, 500.0], values=[[0.1, 0.2]] * 2, angle=[10.0, 5.0]), "angle"),
    (dict(wavelength=[400.0, 500.0], values=[[0.1, 0.2]] * 2, angle=[10.0, 10.0]), "angle"),
    (dict(wavelength=[400.0, 500.0], values=[[0.1, 0.2]] * 2, angle=[-1.0, 10.0]), "[0, 90]"),
    (dict(wavelength=[400.0, 500.0], values=[[0.1, 0.2]] * 2, angle=[10.0, 91.0]), "[0, 90]"),
    (dict(wavelength=[400.0, 500.0], values=[0.1, 0.2], angle=[10.0, 20.0]), "shape"),
    (dict(wavelength=[400.0, 500.0], values=[[0.1, 0.2]] * 3, angle=[10.0, 20.0]), "shape"),
    (dict(wavelength=[400.0, 500.0], values=[[0.1, 0.2, 0.3]] * 2, angle=[10.0, 20.0]), "shape"),
])
def test_invalid_tables_raise_value_error(kwargs, words):
    with pytest.raises(ValueError) as info:
        ReflectivityTable(**kwargs)
    assert words in str(info.value)


def test_valid_tables_and_coatings():
    one = ReflectivityTable([400.0, 800.0], [0.2, 0.4])
    assert one.angle is None and one.values.shape == (2,)
    two = ReflectivityTable(WL, VAL, angle=ANG)
    assert two.values.shape == (5, 5) and np.array_equal(two.angle, ANG)
    single = ReflectivityTable([555.0], [[0.3], [0.6]], angle=[0.0, 90.0])   # one wavelength: R depends on the angle only
    assert single.at(300.0, 45.0) == 0.3 + 0.5 * (0.6 - 0.3)
    for mode in ("specular", "lambertian"):
        for transmission in ("fresnel", "matched"):
            c = Coating((0, 0, 1), reflectivity=two, reflection=mode, transmission=transmission)
            assert c.reflectivity is two
    with pytest.raises(ValueError):
        Coating((0, 0, 1), reflectivity=1.5)
    assert Coating((0, 0, 1), reflectivity=0.25).reflectivity == 0.25
    assert Coating((0, 0, 1)).reflectivity is None


def bilinear(wl_axis, ang_axis, values, wl, ang):
    """Direct evaluation: np.interp along the wavelength for every angle row, then along the angle."""
    rows = np.array([np.interp(wl, wl_axis, row) for row in values])
    return np.interp(ang, ang_axis, rows)


def test_table_evaluation_against_a_direct_bilinear_evaluation():
    table = ReflectivityTable(WL, VAL, angle=ANG)
    rng = np.random.default_rng(11)
    wls = np.concatenate([rng.uniform(300.0, 1000.0, 3000), WL, [250.0, 1200.0]])
    angs = np.concatenate([rng.uniform(0.0, 90.0, 3000), ANG, [0.0, 90.0]])
    for wl, ang in zip(wls, angs):
        assert abs(table.at(wl, ang) - bilinear(WL, ANG, VAL, wl, ang)) <= 1e-12
    for i, wl in enumerate(WL):           # grid nodes: exactly the stored value
        for j, ang in enumerate(ANG):
            assert table.at(wl, ang) == VAL[j, i]
    # clamped: beyond either end of the wavelength axis, the end column
    for j, ang in enumerate(ANG):
        assert table.at(100.0, ang) == VAL[j, 0] and table.at(5000.0, ang) == VAL[j, -1]
    # a table holding a constant evaluates to exactly that constant anywhere
    const = ReflectivityTable(WL, np.full((5, 5), 0.37), angle=ANG)
    assert all(const.at(wl, ang) == 0.37 for wl, ang in zip(wls, angs))
    # without an angle axis: no dependence on the angle
    flat = ReflectivityTable(WL, VAL[2])
    for wl in wls[:200]:
        assert flat.at(wl, 0.0) == flat.at(wl, 77.0)
        assert abs(flat.at(wl, 33.0) - np.interp(wl, WL, VAL[2])) <= 1e-12


def _slab_with(coatings, n=1.5):
    world = Node(name="world", geometry=Box((10.0, 10.0, 10.0), material=Material(refractive_index=1.0)))
    slab = Node(name="slab", parent=world, geometry=Box((2.0, 2.0, 1.0), material=Material(
        refractive_index=n, surface=Surface(delegate=CoatedSurfaceDelegate(coatings)))))
    return world, slab


def test_host_delegate_evaluates_the_table_at_the_rays_wavelength_and_incidence():
    table = ReflectivityTable(WL, VAL, angle=ANG)
    world, slab = _slab_with([Coating((0, 0, 1), reflectivity=table)])
    geometry = slab.geometry
    delegate = geometry.material.surface.delegate
    rng = np.random.default_rng(5)
    for wl, theta in zip(rng.uniform(300.0, 1000.0, 500), rng.uniform(0.0, 89.0, 500)):
        t = math.radians(theta)
        phi = rng.uniform(0.0, 2 * math.pi)
        d = (math.sin(t) * math.cos(phi), math.sin(t) * math.sin(phi), -math.cos(t))   # from the air, onto the top face
        ray = Ray(position=(0.1, -0.2, 0.5), direction=d, wavelength=float(wl))
        got = delegate.reflectivity(geometry.material.surface, ray, geometry, world, slab)
        assert abs(got - bilinear(WL, ANG, VAL, wl, theta)) <= 1e-9
        # from inside the glass the angle is measured on the glass side; beyond the critical angle it stays 1
        up = Ray(position=(0.1, -0.2, 0.5), direction=(d[0], d[1], -d[2]), wavelength=float(wl))
        got = delegate.reflectivity(geometry.material.surface, up, geometry, slab, world)
        want = 1.0 if theta > math.degrees(math.asin(1 / 1.5)) else bilinear(WL, ANG, VAL, wl, theta)
        assert abs(got - want) <= 1e-9
    # an index-matched coating has no critical angle: the table applies at every angle
    world, slab = _slab_with([Coating((0, 0, 1), reflectivity=table, transmission="matched")])
    t = math.radians(60.0)
    up = Ray(position=(0.0, 0.0, 0.5), direction=(math.sin(t), 0.0, math.cos(t)), wavelength=600.0)
    d = slab.geometry.material.surface.delegate
    assert abs(d.reflectivity(slab.geometry.material.surface, up, slab.geometry, slab, world) - bilinear(WL, ANG, VAL, 600.0, 60.0)) <= 1e-9


# -- flattener -------------------------------------------------------------------------------------------------------
def test_flattener_pools_the_tables_of_a_two_coating_scene():
    a = ReflectivityTable(WL, VAL, angle=ANG)
    b = ReflectivityTable([450.0, 650.0, 850.0], [0.9, 0.1, 0.5])
    coatings = [Coating((0, 0, 1), reflectivity=a), Coating((0, 0, -1), reflectivity=0.4),
                Coating((1, 0, 0), reflectivity=b, transmission="matched"), Coating((-1, 0, 0), reflectivity=a)]
    world, _ = _slab_with(coatings)
    c = compile_scene(Scene(world))
    assert c.n_coatings == 4 and c.n_coat_tables == 2
    assert c.coat_table.tolist() == [0, -1, 1, 0]
    assert c.coat_reflectivity.tolist() == [-1.0, 0.4, -1.0, -1.0]
    assert c.ctab_nw.tolist() == [5, 3] and c.ctab_na.tolist() == [5, 1]
    assert c.ctab_wl_start.tolist() == [0, 5] and c.ctab_angle_start.tolist() == [0, 5]
    assert c.ctab_value_start.tolist() == [0, 25]
    assert np.array_equal(c.ctab_wavelength, np.concatenate([WL, [450.0, 650.0, 850.0]]))
    assert np.array_equal(c.ctab_angle, np.concatenate([ANG, [0.0]]))
    assert np.array_equal(c.ctab_value, np.concatenate([VAL.ravel(), [0.9, 0.1, 0.5]]))
    for name in ("coat_table", "ctab_nw", "ctab_na", "ctab_wl_start", "ctab_angle_start", "ctab_value_start",
                 "ctab_wavelength", "ctab_angle", "ctab_value"):
        assert name in c.TABLE_FIELDS and name in c.tables()
    assert c.coat_table.dtype == np.int32 and c.ctab_nw.dtype == np.int32 and c.ctab_value.dtype == np.float64


@pytest.mark.parametrize("name", sorted(scenes.ALL_SCENES))
def test_scenes_without_tables_leave_the_new_tables_neutral(name):
    c = compile_scene(scenes.ALL_SCENES[name]())
    assert c.n_coat_tables == 0
    assert np.all(c.coat_table == -1) and c.coat_table.shape == (c.n_coatings,)
    for key in ("ctab_nw", "ctab_na", "ctab_wl_start", "ctab_angle_start", "ctab_value_start",
                "ctab_wavelength", "ctab_angle", "ctab_value"):
        assert getattr(c, key).size == 0, key


def test_lsc_scenes_with_scalar_coatings_leave_the_new_tables_neutral():
    from benchmarks import configs
    from pvtrace_amd import LSC

    cells = LSC((5.0, 5.0, 1.0))
    cells.add_solar_cell({"left", "right", "near", "far"})
    cells.add_back_surface_mirror()
    cells._make_scene()
    for scene in (configs.cfg5_coated_slab(), cells._scene):
        c = compile_scene(scene)
        assert c.n_coatings > 0 and np.all(c.coat_table == -1) and c.n_coat_tables == 0
        assert not any(np.any(np.asarray(c.tables()[k]) > 0) for k in c.tables() if k.startswith(("ctab_", "coat_table")))


# -- C ABI: the fields appended to PvtSceneTables ----------------------------------------------------------------------
def test_appended_ctypes_fields_match_the_header(tmp_path):
    from pvtrace_amd.engine import native as N

    fields = ["n_coat_tables", "mesh_normals", "coat_table", "n_ctab_wavelength", "n_ctab_angle", "n_ctab_value",
              "ctab_nw", "ctab_na", "ctab_wl_start", "ctab_angle_start", "ctab_value_start", "ctab_wavelength",
              "ctab_angle", "ctab_value"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("sizeof %zu\\n", sizeof(PvtSceneTables));']
    lines += [f'printf("{f} %zu\\n", offsetof(PvtSceneTables, {f}));' for f in fields]
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert C.sizeof(N.PvtSceneTables) == int(out.pop("sizeof"))
    for f, value in out.items():
        assert getattr(N.PvtSceneTables, f).offset == int(value), f
    # additive: the fields of the v13 struct keep their offsets, the new ones come after the last of them
    assert N.PvtSceneTables.n_coat_tables.offset == 9 * 4
    assert N.PvtSceneTables.coat_table.offset >= N.PvtSceneTables.mesh_normals.offset + C.sizeof(C.c_void_p)


def test_struct_of_a_scene_with_tables_carries_them():
    from pvtrace_amd.engine import native as N

    table = ReflectivityTable(WL, VAL, angle=ANG)
    world, _ = _slab_with([Coating((0, 0, 1), reflectivity=table), Coating((0, 0, -1), reflectivity=0.5)])
    c = compile_scene(Scene(world))
    st, keep = N.scene_tables_struct(c)
    assert st.n_coat_tables == 1 and st.n_ctab_wavelength == 5 and st.n_ctab_angle == 5 and st.n_ctab_value == 25
    assert [st.coat_table[i] for i in range(2)] == [0, -1]
    assert [st.ctab_value[i] for i in range(25)] == VAL.ravel().tolist()
    plain = compile_scene(scenes.coated_slab())
    st, keep = N.scene_tables_struct(plain)
    assert st.n_coat_tables == 0 and st.n_ctab_value == 0


# -- hand-traced rays through the per-ray host tracer ----------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(S.STEP_CASES)))
def test_step_tables_decide_hand_traced_rays_on_the_host(case):
    from pvtrace_amd.algorithm import photon_tracer

    make, theta, wl, reflected = S.STEP_CASES[case]
    scene = S.step_scene(make(ReflectivityTable))
    ray = S.step_ray(theta, wl)
    history = photon_tracer.follow(scene, ray, backend="host")
    kinds = [event.name for _, event in history]
    top = np.array([0.0, 0.0, S.STEP_SLAB[2] / 2])
    assert np.allclose(history[1][0].position, top, atol=1e-12)
    d = np.array(ray.direction)
    if reflected:
        assert kinds == ["GENERATE", "REFLECT", "EXIT"]
        assert np.allclose(history[1][0].direction, d * [1, 1, -1], atol=1e-12)   # specular, back up into the air
    else:
        assert kinds == ["GENERATE", "TRANSMIT", "TRANSMIT", "EXIT"]
        t = math.radians(theta)
        s = math.sin(t) / 1.5   # Snell into the glass
        assert np.allclose(history[1][0].direction, [s, 0.0, -math.sqrt(1 - s * s)], atol=1e-12)
        assert abs(history[2][0].position[2] + S.STEP_SLAB[2] / 2) < 1e-12   # out through the bottom, undeviated
        assert np.allclose(history[2][0].direction, history[1][0].direction, atol=1e-12)
