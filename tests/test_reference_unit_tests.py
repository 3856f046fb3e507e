"""The reference's own unit tests of its geometry utils, Material, Distribution, Fresnel helpers and Transformable, as
known answers: tests/golden/make_ref_unit_cases.py made the calls those tests make on the reference's modules and kept the
inputs and the answers (tests/golden/ref_unit_cases.json).  Here the same calls go to this package under the reference's
module paths -- `pvtrace_amd.compat.install()` makes it answer to the name `pvtrace`, so `from pvtrace.geometry.utils
import ...`, `from pvtrace.material.utils import ...` resolve to the product's modules -- in a child process, so that the
alias does not leak into the rest of the session.  Comparisons are the reference tests' own: `==` for the boolean
helpers, np.isclose / np.allclose for the numbers.  (The reference's geometry / node / scene test files need third-party
packages, its engine, scene simulate and flux tests a GPU: those are mirrored call for call in
tests/test_gpu_engine_api.py instead.)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "golden", "ref_unit_cases.json")


def _answers():
    """This package's answers to every case of the fixture, through the reference's module paths -> JSON on stdout."""
    import pvtrace_amd.compat

    pvtrace_amd.compat.install()
    from pvtrace.geometry.transformable import Transformable
    from pvtrace.geometry.utils import (EPS_ZERO, angle_between, close_to_zero, floats_close, magnitude, norm,
                                        ray_z_cylinder, smallest_angle_between)
    from pvtrace.material.distribution import Distribution
    from pvtrace.material.material import Material
    from pvtrace.material.utils import (bandgap, fresnel_reflectivity, fresnel_refraction, specular_reflection,
                                        thermodynamic_emission)

    def f(x):
        return np.asarray(x, dtype=float).tolist()

    case = json.load(open(CASES))
    out = {"EPS_ZERO": float(EPS_ZERO)}
    out["close_to_zero"] = [bool(close_to_zero(x)) for x, _ in case["close_to_zero"]]
    out["floats_close"] = [bool(floats_close(a, b)) for a, b, _ in case["floats_close"]]
    out["magnitude"] = [float(magnitude(v)) for v, _ in case["magnitude"]]
    out["norm"] = [f(norm(v)) for v, _ in case["norm"]]
    out["angle_between"] = [float(angle_between(norm(p), norm(q))) for p, q, _ in case["angle_between"]]
    out["smallest_angle_between"] = [float(smallest_angle_between(norm(p), norm(q)))
                                     for p, q, _ in case["smallest_angle_between"]]
    out["ray_z_cylinder"] = [[f(p) for p in ray_z_cylinder(length, radius, origin, norm(direction))[0]]
                             for length, radius, origin, direction, _ in case["ray_z_cylinder"]]
    out["material_refractive_index"] = [float(Material(n).refractive_index) for n, _ in case["material_refractive_index"]]

    c = case["distribution_emission"]
    x = np.linspace(*c["x"])
    ems = thermodynamic_emission(np.column_stack((x, bandgap(x, *c["bandgap"]))), T=c["T"], mu=c["mu"])
    d = Distribution(ems[:, 0], ems[:, 1])
    out["distribution_emission"] = {"sample": [float(d.sample(p)) for p, _ in c["sample"]],
                                    "lookup": [float(d.lookup(w)) for w, _ in c["lookup"]]}
    c = case["distribution_step"]
    lo, hi, step = c["x"]
    xs = np.arange(lo, hi + step, step)
    h = Distribution(xs, bandgap(xs, *c["bandgap"]), hist=True)
    a, b, count = c["probe"]
    out["distribution_step"] = {"sample": [float(h.sample(p)) for p, _ in c["sample"]],
                                "lookup": [float(h.lookup(w)) for w, _ in c["lookup"]],
                                "probe_values": sorted(set(f(h.sample(np.linspace(h.lookup(a), h.lookup(b), count)))))}

    out["fresnel_reflectivity"] = [float(fresnel_reflectivity(t, n1, n2)) for t, n1, n2, _ in case["fresnel_reflectivity"]]
    out["specular_reflection"] = [f(specular_reflection(dv, nv)) for dv, nv, _ in case["specular_reflection"]]
    out["fresnel_refraction"] = [f(fresnel_refraction(dv, nv, n1, n2)) for dv, nv, n1, n2, _ in case["fresnel_refraction"]]
    c = case["transformable"]
    out["transformable"] = {"is_transformable": type(Transformable()) is Transformable,
                            "default_location": f(Transformable().location),
                            "location": f(Transformable(location=tuple(c["location"][0])).location),
                            "pose": f(Transformable.from_pose(np.array(c["pose"][0])).pose)}
    print(json.dumps(out))


def test_the_references_own_unit_tests_pass_against_this_package():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    done = subprocess.run([sys.executable, "-c", "import tests.test_reference_unit_tests as t; t._answers()"],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    got = json.loads(done.stdout.strip().splitlines()[-1])
    case = json.load(open(CASES))

    assert got["EPS_ZERO"] == case["EPS_ZERO"]
    assert got["close_to_zero"] == [want for _, want in case["close_to_zero"]]
    assert got["floats_close"] == [want for _, _, want in case["floats_close"]]
    assert np.allclose(got["magnitude"], [want for _, want in case["magnitude"]])
    assert np.allclose(got["norm"], [want for _, want in case["norm"]])
    for key in ("angle_between", "smallest_angle_between"):
        assert np.allclose(got[key], [want for _, _, want in case[key]]), key
    # exact 0 and pi for parallel and anti-parallel vectors, as the reference's test asks
    assert got["angle_between"][:2] == [case["angle_between"][0][2], case["angle_between"][1][2]] == [0.0, np.pi]
    for mine, (*_, want) in zip(got["ray_z_cylinder"], case["ray_z_cylinder"], strict=True):
        assert len(mine) == len(want) and all(np.allclose(a, b) for a, b in zip(mine, want)), (mine, want)
    assert got["material_refractive_index"] == [want for _, want in case["material_refractive_index"]]

    for key in ("distribution_emission", "distribution_step"):
        for what in ("sample", "lookup"):
            assert np.allclose(got[key][what], [want for _, want in case[key][what]]), (key, what)
    step = case["distribution_step"]
    assert len(got["distribution_step"]["probe_values"]) == len(step["probe_values"]) == 3
    assert np.allclose(got["distribution_step"]["probe_values"], step["probe_values"])
    assert got["distribution_step"]["lookup"][2] == 1.0   # the cumulative probability at the upper end
    p400, p401 = got["distribution_step"]["lookup"][:2]
    assert 0.0 <= p400 <= p401

    assert np.allclose(got["fresnel_reflectivity"], [want for *_, want in case["fresnel_reflectivity"]])
    assert np.allclose(got["fresnel_reflectivity"], 0.04)
    for key in ("specular_reflection", "fresnel_refraction"):
        assert np.allclose(got[key], [want for *_, want in case[key]]), key
    t = case["transformable"]
    assert got["transformable"]["is_transformable"]
    assert np.allclose(got["transformable"]["default_location"], t["default_location"])
    assert np.allclose(got["transformable"]["location"], t["location"][1])
    assert np.allclose(got["transformable"]["pose"], t["pose"][1])
