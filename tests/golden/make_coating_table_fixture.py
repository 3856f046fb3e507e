"""Generator of tests/golden/coating_table_tracer.npz: the REFERENCE's own per-ray Python tracer
(`algorithm/photon_tracer.py` `follow`) on the selective-mirror slab of tests/coating_table_scene.py.

The mirror is written here as the reference lets users write coatings: a `FresnelSurfaceDelegate` subclass whose
`reflectivity(surface, ray, geometry, container, adjacent)` reads `ray.wavelength` and the angle of incidence and
interpolates the table with numpy (in wavelength, then in angle, clamped at the ends), keeping the reflectivity of 1
beyond the critical angle.  Everything else -- material, luminophore, light, emission, the tracer -- is the reference's;
the scene graph and the Box are this project's, as in make_golden.make_cfg5_tracer (the reference's need anytree and
trimesh, neither of which is here).  Rays: the reference's `emit_bundle` under numpy seed 1207.

Kept per ray (numbers only): its outcome class (coating_table_scene.outcome_class: where it left the slab, or lost or
killed), made from the last event's kind and the position the reference's `LSC.simulate` would store as the exit ray.  The same run
without the mirror is stored too, so a test can show that it tells the two apart.

    python tests/golden/make_coating_table_fixture.py [n_rays]
"""
import os
import sys
import types

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden  # noqa: E402  (puts the repository root on sys.path)
from make_golden import REF, ref_module, save  # noqa: E402

RAYS = 10000


def reference_modules():
    """The module substitutions of make_golden.make_cfg5_tracer."""
    import pvtrace_amd.geometry as prod_geometry
    import pvtrace_amd.scene as prod_scene

    ref_module("pvtrace.data.lumogen_f_red_305")
    for sub in ("scene", "light", "material", "geometry", "algorithm", "common", "device", "engine"):
        if f"pvtrace.{sub}" not in sys.modules:
            pkg = types.ModuleType(f"pvtrace.{sub}")
            pkg.__path__ = [os.path.join(REF, sub)]
            sys.modules[f"pvtrace.{sub}"] = pkg
    sys.modules["pvtrace.scene.node"] = prod_scene
    sys.modules["pvtrace.scene.scene"] = prod_scene
    sys.modules["pvtrace.geometry.box"] = prod_geometry
    return prod_scene, prod_geometry


def selective_mirror_class(FresnelSurfaceDelegate, wavelength, angle, value):
    class SelectiveTopMirror(FresnelSurfaceDelegate):
        """Band-stop mirror on the top face (+z): R(wavelength, angle of incidence) from a table."""

        def reflectivity(self, surface, ray, geometry, container, adjacent):
            r = super(SelectiveTopMirror, self).reflectivity(surface, ray, geometry, container, adjacent)
            normal = np.asarray(geometry.normal(ray.position), dtype=float)
            if not np.allclose(normal, (0.0, 0.0, 1.0)) or r == 1.0:
                return r   # other faces, and total internal reflection, stay Fresnel
            cosang = abs(float(np.dot(normal, ray.direction)))
            theta = np.degrees(np.arccos(min(cosang, 1.0)))
            by_angle = [np.interp(ray.wavelength, wavelength, row) for row in value]
            return float(np.interp(theta, angle, by_angle))

    return SelectiveTopMirror


def trace(full, n, seed, emit, tracer, ray_cls, event_cls):
    view = types.SimpleNamespace(root=full.root, light_nodes=[m for m in full.root.levelorder() if getattr(m, "light", None) is not None])
    np.random.seed(seed)
    pos, direc, wl, _ = emit.emit_bundle(view, n)
    counts = np.zeros((n, 10), dtype=np.uint16)
    last = np.zeros(n, dtype=np.uint8)
    where = np.zeros((n, 3))
    for j in range(n):
        hist = tracer.follow(full, ray_cls(position=tuple(pos[j]), direction=tuple(direc[j]), wavelength=float(wl[j])))
        for _, event in hist:
            counts[j, event.value] += 1
        last[j] = hist[-1][1].value
        where[j] = hist[-2][0].position if hist[-1][1] == event_cls.EXIT else hist[-1][0].position
    return counts, last, where


def make_coating_table_tracer(n=RAYS):
    import coating_table_scene as S  # noqa: E402  (tests/ on the path below)

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
    mirror_cls = selective_mirror_class(surface.FresnelSurfaceDelegate, S.MIRROR_WAVELENGTH, S.MIRROR_ANGLE, S.MIRROR_VALUE)

    out = {}
    for name, delegate, seed in (("mirror", mirror_cls(), 1207), ("plain", None, 1208)):
        full, _ = S.build(prod_scene.Node, prod_scene.Scene, prod_geometry.Box, material.Material, surface.Surface, light.Light,
                          light.rectangular_mask, light.ConstantWavelengthMask(S.PUMP_NM),
                          S.components(component.Luminophore, lumogen), delegate=delegate)
        _, last, where = trace(full, n, seed, emit, tracer, ray_cls, event_cls)
        outcome = S.outcome_class(last, where)
        out[f"{name}/outcome"] = outcome.astype(np.uint8)
        print(f"   {name}: outcome fractions", dict(zip(S.CLASSES, np.round(np.bincount(outcome, minlength=5) / n, 4).tolist())))
    save("coating_table_tracer.npz", **out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    make_coating_table_tracer(int(sys.argv[1]) if len(sys.argv) > 1 else RAYS)
