"""Fixture generator for tests/test_reference_unit_tests.py (needs the reference tree, like make_golden.py).

    python tests/golden/make_ref_unit_cases.py

The reference's unit-test files for geometry utils, Material, Distribution, the Fresnel helpers and Transformable make
calls with fixed inputs and check what comes back.  This script makes the same calls on the reference's own modules
(imported where they lie, through the namespace stub of make_golden.py) and saves only the inputs and the answers, as
JSON, in ref_unit_cases.json.  Where a test of the reference draws a random number, a seeded one stands in for it.
`Material` is the one class whose module does not import without a third-party package (anytree): its case stores the
index it is built with, which is what the reference's test expects back."""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ref_module  # noqa: E402  (sets sys.dont_write_bytecode; the reference tree stays untouched)


def _list(x):
    return np.asarray(x, dtype=float).tolist()


def make():
    gu = ref_module("pvtrace.geometry.utils")
    mu = ref_module("pvtrace.material.utils")
    dist = ref_module("pvtrace.material.distribution")
    tr = ref_module("pvtrace.geometry.transformable")
    rng = np.random.default_rng(20240611)
    eps = float(gu.EPS_ZERO)
    out = {"EPS_ZERO": eps}

    zeros = [0.0, 0.9 * eps, -0.9 * eps, eps, -eps]
    out["close_to_zero"] = [[x, bool(gu.close_to_zero(x))] for x in zeros]
    a = float(rng.random())
    pairs = [(a, a + eps), (a, a - eps), (a, a + 0.9 * eps), (a, a - 0.9 * eps), (a, a)]
    out["floats_close"] = [[x, y, bool(gu.floats_close(x, y))] for x, y in pairs]

    v = (1.0, 1.0, 1.0)
    out["magnitude"] = [[list(v), float(gu.magnitude(v))]]
    out["norm"] = [[list(v), _list(gu.norm(v))]]
    angle_pairs = [((1.0, 0.0, 0.0), (1.0, 0.0, 0.0)), ((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
                   ((1.0, 1.0, 0.0), (1.0, 0.0, 0.0)), ((1.0, 1.0, 0.0), (-1.0, 0.0, 0.0))]
    out["angle_between"] = [[list(p), list(q), float(gu.angle_between(gu.norm(p), gu.norm(q)))] for p, q in angle_pairs]
    out["smallest_angle_between"] = [[list(p), list(q), float(gu.smallest_angle_between(gu.norm(p), gu.norm(q)))]
                                     for p, q in angle_pairs]

    rays = [((0.2, 0.2, -1.0), (0.0, 0.0, 1.0)), ((-2.0, 0.2, 0.0), (1.0, 0.2, -0.2)),
            ((-2.0, 0.2, 0.0), (1.0, 0.2, 0.2)), ((0.0, 0.0, -1.5), (0.0, 1.0, 1.0))]
    out["ray_z_cylinder"] = []
    for origin, direction in rays:
        points, _ = gu.ray_z_cylinder(1.0, 1.0, origin, gu.norm(direction))
        out["ray_z_cylinder"].append([1.0, 1.0, list(origin), list(direction), [_list(p) for p in points]])

    out["material_refractive_index"] = [[1.5, 1.5]]

    x = np.linspace(400, 1010, 2000)
    ems = mu.thermodynamic_emission(np.column_stack((x, mu.bandgap(x, 600, 1000))), T=300, mu=0.1)
    d = dist.Distribution(ems[:, 0], ems[:, 1])
    lo, hi = float(d.sample(0)), float(d.sample(1))
    out["distribution_emission"] = {"x": [400, 1010, 2000], "bandgap": [600, 1000], "T": 300, "mu": 0.1,
                                    "sample": [[0.0, lo], [1.0, hi]], "lookup": [[lo, float(d.lookup(lo))],
                                                                                 [hi, float(d.lookup(hi))]]}
    xs = np.arange(400.0, 801.0, 1.0)
    h = dist.Distribution(xs, mu.bandgap(xs, 600.0, 1.0), hist=True)
    probe = np.linspace(h.lookup(598.0), h.lookup(601.0), 10000)
    out["distribution_step"] = {"x": [400.0, 800.0, 1.0], "bandgap": [600.0, 1.0],
                                "sample": [[0.0, float(h.sample(0))], [1.0, float(h.sample(1))]],
                                "lookup": [[w, float(h.lookup(w))] for w in (400.0, 401.0, 800.0)],
                                "probe": [598.0, 601.0, 10000], "probe_values": sorted(set(_list(h.sample(probe))))}

    out["fresnel_reflectivity"] = [[0.0, 1.0, 1.5, float(mu.fresnel_reflectivity(0.0, 1.0, 1.5))]]
    out["specular_reflection"] = [[list(dv), list(nv), _list(mu.specular_reflection(dv, nv))]
                                  for dv, nv in (((0.0, 0.0, -1.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, -1.0), (0.0, 0.0, -1.0)))]
    out["fresnel_refraction"] = [[list(dv), list(nv), 1.0, 1.5, _list(mu.fresnel_refraction(dv, nv, 1.0, 1.5))]
                                 for dv, nv in (((0.0, 0.0, -1.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, -1.0), (0.0, 0.0, -1.0)))]

    pose = rng.random((4, 4))
    out["transformable"] = {"default_location": _list(tr.Transformable().location),
                            "location": [[1.0, 1.0, 1.0], _list(tr.Transformable(location=(1, 1, 1)).location)],
                            "pose": [_list(pose), _list(tr.Transformable.from_pose(pose).pose)]}

    path = os.path.join(HERE, "ref_unit_cases.json")
    with open(path, "w") as fp:
        json.dump(out, fp, indent=1)
        fp.write("\n")
    print(f"ref_unit_cases.json: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    make()
