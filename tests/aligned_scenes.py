"""Scenes and pencils of the aligned-luminophore tests (tests/test_aligned_luminophores.py, tests/test_gpu_aligned_luminophores.py):
one slab of index 1.0 in a world of index 1.0 -- a pencil keeps its direction, the chord through the slab is the path
length -- holding the components under test, optionally rotated; and the closed forms the samples are held to."""
import math

import numpy as np

from pvtrace_amd import Absorber, Alignment, Box, Light, Luminophore, Material, Node, Scene
from pvtrace_amd.material import ray_basis
from tests import laws as L

SLAB = (4.0, 4.0, 1.0)
MAGIC = math.degrees(math.acos(1.0 / math.sqrt(3.0)))   # 54.7356 degrees: P2 = 0
ANGLES = (0.0, MAGIC, 90.0)
TILT = (math.radians(30.0), (1.0, 0.0, 0.0))            # the rotated slab: 30 degrees about x
X = np.arange(400.0, 801.0)


def slab_scene(components, rotate=None, index=1.0):
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    slab = Node(name="slab", parent=world,
                geometry=Box(SLAB, material=Material(refractive_index=index, components=list(components))))
    if rotate is not None:
        slab.rotate(*rotate)
    lamp = Node(name="lamp", parent=world, light=Light(name="lamp"))
    lamp.location = (0.0, 0.0, -5.0)
    return Scene(world)


def rotation_of(rotate):
    return np.eye(3) if rotate is None else L.rotation(*rotate)


def pencil(theta_deg, n, rotate=None, wavelength=555.0):
    """n identical rays at `theta_deg` to the slab's normal (its local +z) -> ((pos, dirs, wl), chord length in the slab).
    Below 90 degrees the pencil comes from below and crosses the two large faces (chord 1 / cos); at 90 it runs along
    the slab's local +x through its mid-plane (chord: the slab's length).  Built in the slab's frame, turned with it."""
    t = math.radians(theta_deg)
    if theta_deg == 90.0:
        d, p, chord = np.array([1.0, 0.0, 0.0]), np.array([-6.0, 0.1, 0.05]), SLAB[0]
    else:
        d = np.array([math.sin(t), 0.0, math.cos(t)])
        p = np.array([-0.3, 0.1, 0.0]) - 4.0 * d
        chord = SLAB[2] / math.cos(t)
    R = rotation_of(rotate)
    d, p = R @ d, R @ p
    d = d / math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return (np.tile(p, (n, 1)), np.tile(d, (n, 1)), np.full(n, wavelength)), chord


def factor_along(direction, director_world, order):
    """f by the rule's own operations: mu = (dx nx + dy ny) + dz nz clamped, f = 1.0 - S (1.5 (mu mu) - 0.5)."""
    return float(Alignment.factor(Alignment.cosine(direction, director_world), order))


def absorbed_probability(alpha, f, chord):
    return -math.expm1(-alpha * f * chord)


def table_bin_masses(table, bins):
    """P(mu in bin) of what sampling `table` gives: its CDF is piecewise linear through (mu_j, C_j)."""
    edges = np.linspace(-1.0, 1.0, bins + 1)
    return np.diff(np.interp(edges, table.mu, table.cdf[0]))


def mu_and_azimuth(directions, axis):
    """(mu, phi) of unit vectors about the unit vector `axis`, phi in the basis `ray_basis(axis)`."""
    axis = np.asarray(axis, dtype=np.float64)
    e1, e2 = ray_basis(axis)
    d = np.asarray(directions, dtype=np.float64)
    return d @ axis, np.arctan2(d @ e2, d @ e1)


def absorber(alpha, director, order, name="dye"):
    return Absorber(float(alpha), name=name, alignment=Alignment(director, absorption_order=order))


def luminophore(alpha, director, s_a, s_e, name="dye", qy=1.0):
    alignment = None if director is None else Alignment(director, absorption_order=s_a, emission_order=s_e)
    return Luminophore(float(alpha), x=X, quantum_yield=qy, name=name, alignment=alignment)


def zero_aligned(scene, director=(1.0, 2.0, 2.0)):
    """`Alignment(director, 0.0, 0.0)` on every component of the scene (the root holds none) -> the scene."""
    for node in scene.root.preorder():
        if node.geometry is None or node is scene.root:
            continue
        for c in node.geometry.material.components:
            c.alignment = Alignment(director, 0.0, 0.0)
    return scene
