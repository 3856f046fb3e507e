"""The selective-mirror slab of tests/golden/coating_table_tracer.npz, built from whichever classes are handed in.

A Lumogen F Red 305 slab whose top face carries a wavelength- and angle-selective mirror: a band-stop reflector that lets
the green pump through and sends the luminophore's red emission back into the slab, less so at oblique incidence.  The
generator (tests/golden/make_coating_table_fixture.py) builds it from the REFERENCE's material / light classes with the
mirror as a `FresnelSurfaceDelegate` subclass; the tests build it from this project's classes with the mirror as a
`Coating(reflectivity=ReflectivityTable(...))`.  The numbers below are the one description both use.
"""
import functools

import numpy as np

SLAB = (5.0, 5.0, 0.5)                 # cm
WORLD = 20.0
N_SLAB = 1.5
QUANTUM_YIELD = 0.9
PUMP_NM = 555.0
LAMP_HALF = 2.0                        # the lamp's rectangle: 4 x 4 cm, centred above the slab
LAMP_Z = 2.0
# the mirror's table: wavelengths (nm), angles of incidence (degrees), R (n_angle x n_wavelength)
MIRROR_WAVELENGTH = np.array([400.0, 560.0, 590.0, 610.0, 640.0, 700.0, 800.0])
MIRROR_ANGLE = np.array([0.0, 20.0, 40.0, 60.0, 90.0])
MIRROR_VALUE = np.outer([1.0, 0.95, 0.7, 0.35, 0.1], [0.02, 0.03, 0.2, 0.85, 0.97, 0.97, 0.9])
SPECTRUM_X = np.linspace(400.0, 800.0, 401)


def components(Luminophore, lumogen):
    x = SPECTRUM_X
    return [Luminophore(np.column_stack((x, lumogen.absorption(x) * 10.0)), emission=np.column_stack((x, lumogen.emission(x))),
                        quantum_yield=QUANTUM_YIELD, name="Lumogen F Red 305")]


def build(Node, Scene, Box, Material, Surface, Light, rectangular_mask, pump, slab_components, delegate=None):
    """(scene, slab node).  `pump`: the light's wavelength delegate (PUMP_NM); `delegate`: the slab's surface delegate
    (None = plain Fresnel)."""
    world = Node(name="world (air)", geometry=Box((WORLD, WORLD, WORLD), material=Material(refractive_index=1.0)))
    surface = Surface() if delegate is None else Surface(delegate=delegate)
    slab = Node(name="slab", parent=world,
                geometry=Box(SLAB, material=Material(refractive_index=N_SLAB, surface=surface, components=slab_components)))
    lamp = Node(name="Light", parent=world,
                light=Light(wavelength=pump, position=functools.partial(rectangular_mask, LAMP_HALF, LAMP_HALF),
                            name="Light"))
    lamp.location = (0.0, 0.0, LAMP_Z)
    lamp.rotate(np.radians(180.0), (1.0, 0.0, 0.0))
    return Scene(world), slab


def outcome_class(last_kind, where, tol=1e-6):
    """Per-ray outcome: 0 left through the top face (or bounced off it), 1 through the bottom face, 2 through an edge,
    3 lost (non-radiative absorption), 4 anything else.  `where`: the position of the last event before EXIT."""
    last_kind, where = np.asarray(last_kind), np.asarray(where)
    half = np.array(SLAB) / 2.0
    out = np.full(len(last_kind), 4, dtype=np.int64)
    exit_ = last_kind == 7
    top = exit_ & (np.abs(where[:, 2] - half[2]) < tol)
    bottom = exit_ & (np.abs(where[:, 2] + half[2]) < tol)
    edge = exit_ & ~top & ~bottom & ((np.abs(np.abs(where[:, 0]) - half[0]) < tol) | (np.abs(np.abs(where[:, 1]) - half[1]) < tol))
    out[top], out[bottom], out[edge] = 0, 1, 2
    out[last_kind == 4] = 3
    return out


CLASSES = ("top", "bottom", "edge", "lost", "other")


# -- hand-traced rays: step tables that make every decision certain (R is 0 or 1) ------------------------------------
def wavelength_step_table(ReflectivityTable):
    """R = 1 below 600 nm, 0 above (a 2 nm ramp between 599 and 601 nm), whatever the angle."""
    return ReflectivityTable([300.0, 599.0, 601.0, 1000.0], [1.0, 1.0, 0.0, 0.0])


def angle_step_table(ReflectivityTable):
    """R = 1 below 30 degrees of incidence, 0 above (a ramp between 29 and 31 degrees), whatever the wavelength."""
    return ReflectivityTable([300.0, 1000.0], [[1.0, 1.0], [1.0, 1.0], [0.0, 0.0], [0.0, 0.0]], angle=[0.0, 29.0, 31.0, 90.0])


STEP_SLAB = (2.0, 2.0, 1.0)


def step_scene(table):
    """A glass block (n = 1.5) in air whose top face carries `table` and whose other faces are index-matched and
    transparent (R = 0): a ray that comes down onto the top face either bounces straight back out of the world or goes
    through the block and out through the bottom -- no random decision anywhere."""
    from pvtrace_amd import Box, CoatedSurfaceDelegate, Coating, Material, Node, Scene, Surface

    clear = [Coating(f, reflectivity=0.0, transmission="matched")
             for f in ((0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0))]
    delegate = CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=table)] + clear)
    world = Node(name="world (air)", geometry=Box((10.0, 10.0, 10.0), material=Material(refractive_index=1.0)))
    Node(name="block", parent=world,
         geometry=Box(STEP_SLAB, material=Material(refractive_index=1.5, surface=Surface(delegate=delegate))))
    return Scene(world)


def step_ray(theta_deg, wavelength):
    """A ray in the xz plane that meets the top face at its centre at `theta_deg` from the normal."""
    from pvtrace_amd import Ray

    t = np.radians(theta_deg)
    d = (float(np.sin(t)), 0.0, -float(np.cos(t)))
    start = (-1.5 * d[0] / -d[2], 0.0, STEP_SLAB[2] / 2 + 1.5)
    return Ray(position=start, direction=d, wavelength=float(wavelength))


# (table builder, angle of incidence, wavelength, reflected at the top face?)
STEP_CASES = (
    (wavelength_step_table, 10.0, 550.0, True),
    (wavelength_step_table, 10.0, 650.0, False),
    (angle_step_table, 20.0, 555.0, True),
    (angle_step_table, 40.0, 555.0, False),
)
