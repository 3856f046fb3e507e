"""Generator of tests/golden/dispersion_tracer.npz: the REFERENCE's own per-ray Python tracer
(`algorithm/photon_tracer.py` `follow`) on the dispersive Lumogen slab of tests/dispersion_scene.py.

The dispersion is written here as the reference lets users write it: a `FresnelSurfaceDelegate` subclass that
interpolates the slab's index at `ray.wavelength` (np.interp, clamped at the ends) and hands it, with the other side's
index, to the reference's own `fresnel_reflectivity` and `fresnel_refraction`, exactly as the reference's delegate does
with scalar indices.  Everything else -- material, luminophore, light, emission, the tracer -- is the reference's; the
scene graph and the Box are this project's, as in make_coating_table_fixture.py.  Rays: the reference's `emit_bundle`
under numpy seeds 2207 (dispersive) and 2208 (the same slab at the scalar index).

Kept per ray (numbers only): its outcome class (dispersion_scene.outcome_class) and its count of events of each kind.

    python tests/golden/make_dispersion_fixture.py [n_rays]
"""
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden  # noqa: E402,F401  (puts the repository root on sys.path)
from make_coating_table_fixture import reference_modules, trace  # noqa: E402
from make_golden import ref_module, save  # noqa: E402

RAYS = 6000


def dispersive_delegate_class(surface_mod, slab_index):
    """`slab_index(wavelength)`: the slab's index; every other node keeps its scalar one."""

    class DispersiveFresnel(surface_mod.FresnelSurfaceDelegate):
        def _indices(self, ray, container, adjacent):
            def n(node):
                return slab_index(ray.wavelength) if node.name == "slab" else node.geometry.material.refractive_index
            return n(container), n(adjacent)

        def _normal(self, ray, geometry):
            normal = geometry.normal(ray.position)
            if np.dot(normal, ray.direction) < 0.0:
                normal = surface_mod.flip(normal)
            return normal

        def reflectivity(self, surface, ray, geometry, container, adjacent):
            n1, n2 = self._indices(ray, container, adjacent)
            angle = surface_mod.angle_between(self._normal(ray, geometry), np.array(ray.direction))
            return float(surface_mod.fresnel_reflectivity(angle, n1, n2))

        def transmitted_direction(self, surface, ray, geometry, container, adjacent):
            n1, n2 = self._indices(ray, container, adjacent)
            return tuple(surface_mod.fresnel_refraction(ray.direction, self._normal(ray, geometry), n1, n2).tolist())

    return DispersiveFresnel


def make_dispersion_tracer(n=RAYS):
    from tests import dispersion_scene as D

    prod_scene, prod_geometry = reference_modules()
    surface = ref_module("pvtrace.material.surface")
    material = ref_module("pvtrace.material.material")
    component = ref_module("pvtrace.material.component")
    light = ref_module("pvtrace.light.light")
    emit = ref_module("pvtrace.engine.emit")
    tracer = ref_module("pvtrace.algorithm.photon_tracer")
    ray_cls = ref_module("pvtrace.light.ray").Ray
    event_cls = ref_module("pvtrace.light.event").Event
    lumogen = ref_module("pvtrace.data.lumogen_f_red_305")
    dispersive = dispersive_delegate_class(surface, D.dispersive_index)

    out = {}
    for name, delegate, seed in (("dispersive", dispersive(), 2207), ("scalar", None, 2208)):
        full, _ = D.build(prod_scene.Node, prod_scene.Scene, prod_geometry.Box, material.Material, surface.Surface, light.Light,
                          light.rectangular_mask, light.ConstantWavelengthMask(D.PUMP_NM),
                          D.components(component.Luminophore, lumogen), index=D.N_SCALAR, delegate=delegate)
        counts, last, where = trace(full, n, seed, emit, tracer, ray_cls, event_cls)
        outcome = D.outcome_class(last, where)
        out[f"{name}/outcome"] = outcome.astype(np.uint8)
        out[f"{name}/event_counts"] = counts
        print(f"   {name}: outcome fractions", dict(zip(D.CLASSES, np.round(np.bincount(outcome, minlength=5) / n, 4).tolist())),
              "mean events", np.round(counts.mean(axis=0), 3).tolist())
    save("dispersion_tracer.npz", **out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    make_dispersion_tracer(int(sys.argv[1]) if len(sys.argv) > 1 else RAYS)
