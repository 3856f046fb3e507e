"""The dispersive Lumogen slab of tests/golden/dispersion_tracer.npz, and the exaggerated-dispersion block of the
hand-traced rays, built from whichever classes are handed in.

The slab is the one of tests/coating_table_scene.py (a Lumogen F Red 305 slab pumped at 555 nm from above) without the
mirror, whose index depends on the wavelength: n(lambda) interpolated linearly in the table below, clamped at both ends.
The dispersion is exaggerated (0.3 across 400-800 nm, ten times that of PMMA) so that a fixture of some thousand rays
tells it apart from the scalar slab.  The generator (tests/golden/make_dispersion_fixture.py) builds it from the
REFERENCE's classes, with the dispersion as a `FresnelSurfaceDelegate` subclass; the tests build it from this project's
classes with `Material(refractive_index=RefractiveIndexTable(...))`.  The numbers below are the one description both use.
"""
import numpy as np

from tests import coating_table_scene as S

SLAB, WORLD, PUMP_NM, LAMP_HALF, LAMP_Z = S.SLAB, S.WORLD, S.PUMP_NM, S.LAMP_HALF, S.LAMP_Z
N_SCALAR = 1.5
DISP_WAVELENGTH = np.array([400.0, 500.0, 600.0, 700.0, 800.0])
DISP_VALUE = np.array([1.40, 1.46, 1.55, 1.63, 1.70])
outcome_class, CLASSES, components = S.outcome_class, S.CLASSES, S.components


def dispersive_index(wavelength):
    """n(lambda) of the table: np.interp clamps at both ends, as RefractiveIndexTable.at does."""
    return float(np.interp(wavelength, DISP_WAVELENGTH, DISP_VALUE))


def build(Node, Scene, Box, Material, Surface, Light, rectangular_mask, pump, slab_components, index=N_SCALAR, delegate=None):
    """(scene, slab node): the slab with refractive index `index` (a number or a table object) and surface delegate
    `delegate` (None = plain Fresnel)."""
    import functools

    world = Node(name="world (air)", geometry=Box((WORLD, WORLD, WORLD), material=Material(refractive_index=1.0)))
    surface = Surface() if delegate is None else Surface(delegate=delegate)
    slab = Node(name="slab", parent=world,
                geometry=Box(SLAB, material=Material(refractive_index=index, surface=surface, components=slab_components)))
    lamp = Node(name="Light", parent=world,
                light=Light(wavelength=pump, position=functools.partial(rectangular_mask, LAMP_HALF, LAMP_HALF),
                            name="Light"))
    lamp.location = (0.0, 0.0, LAMP_Z)
    lamp.rotate(np.radians(180.0), (1.0, 0.0, 0.0))
    return Scene(world), slab


# -- hand-traced rays: a clear block of strongly dispersive glass in air ---------------------------------------------
BLOCK = (4.0, 4.0, 1.0)
BLOCK_WAVELENGTH = [400.0, 600.0, 800.0]
BLOCK_VALUE = [1.40, 1.55, 1.70]


def block_scene(index):
    """A clear block (no absorber) of index `index` in air."""
    from pvtrace_amd import Box, Material, Node, Scene

    world = Node(name="world (air)", geometry=Box((20.0, 20.0, 20.0), material=Material(refractive_index=1.0)))
    Node(name="block", parent=world, geometry=Box(BLOCK, material=Material(refractive_index=index)))
    return Scene(world)
