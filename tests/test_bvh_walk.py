"""The f32 cull of the kernel's BVH walk, restated on the host (oracle/bvh_walk.cpp) over the REAL tree of pvt_bvh.h, held to
the two things the design rests on:

  * NO CROSSING IS LOST: every face the f64 triangle test crosses lies in a leaf the walk reaches -- for the exact
    reference's crossings of every family of tests/mesh_cases.py, and for 2 * 10^5 further seeded rays per mesh whose
    crossings the referee's brute-force loop over the faces finds in doubles;
  * the header's own claim, "the padding is eight times the rounding": of the pad of every box on a crossing's path to the
    root at least 7/8 is left by the f32 arithmetic (least slack / pad >= 7/8), wherever the claim's premise holds -- the
    origin within 10^3 diagonals of the mesh.  From 10^6 diagonals only the first assertion is made.

Measured least slack / pad per mesh and family: docs/parity_chain.md, "Triangle meshes"."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import mesh_cases as MC

CLAIM = 7.0 / 8.0
N_RANDOM = 200_000


def _crossings_of(name, family, rays):
    """(ray, face, t) of the exact reference's crossings of the rays `rays` of a family, every face of a group with its own t."""
    refs = MC.references(name, family)
    rows = [(k, f, t) for k, j in enumerate(rays) if not refs[j].ambiguous
            for c in refs[j].crossings for f, (t, _) in c.faces.items()]
    if not rows:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)
    r, f, t = zip(*rows)
    return np.array(r, np.int32), np.array(f, np.int32), np.array(t)


def _split(name, family):
    """A family's rays by the claim's premise: (label, ray indices, premise holds)."""
    case = MC.mesh(name)
    o, _, _ = MC.rays(name, family)
    far = np.sqrt(np.sum((o - case.centre) ** 2, axis=1)) > 2.0e3 * case.diag
    parts = [(family, np.nonzero(~far)[0], True)]
    if far.any():
        parts.append((family + " from 10^6 diagonals", np.nonzero(far)[0], False))
    return parts


@pytest.mark.parametrize("family", MC.FAMILIES)
@pytest.mark.parametrize("name", MC.MESHES)
def test_the_walk_reaches_every_exact_crossing_with_seven_eighths_of_the_pad_to_spare(name, family):
    case = MC.mesh(name)
    o, d, _ = MC.rays(name, family)
    for label, rays, premise in _split(name, family):
        exact = O.bvh_walk_check(case.vertices, case.faces, o[rays], d[rays], crossings=_crossings_of(name, family, rays))
        brute = O.bvh_walk_check(case.vertices, case.faces, o[rays], d[rays])          # (the ambiguous rays as well)
        print(f"bvh-walk {name} {label}: {exact['checked']} exact crossings, least slack / pad = {exact['min_slack']:.4f} "
              f"(ray {rays[exact['at'][0]] if exact['at'][0] >= 0 else -1}, face {exact['at'][1]}, axis {exact['at'][2]}); brute force {brute['checked']} crossings, "
              f"{brute['min_slack']:.4f}; most leaves reached by a ray {brute['most_leaves']}")
        assert exact["lost"] == 0 and brute["lost"] == 0, (name, label, exact["first_lost"], brute["first_lost"])
        assert exact["checked"] > 0 or family == "P"
        if premise:
            assert min(exact["min_slack"], brute["min_slack"]) >= CLAIM, (name, label, exact, brute)


def random_rays(case, n, seed):
    """Origins from a hundredth of a diagonal to a thousand diagonals from the centre (log-uniform), aimed at points of the
    bounding box, at vertices (the corners of the tightest boxes) and, one ray in ten, along a coordinate plane."""
    rng = np.random.default_rng(seed)
    origins = case.centre + case.diag * (10.0 ** rng.uniform(-2.0, 3.0, (n, 1))) * MC._isotropic(rng, n)
    targets = rng.uniform(case.lo, case.hi, (n, 3))
    at_vertex = rng.random(n) < 0.3
    targets[at_vertex] = case.vertices[rng.integers(0, len(case.vertices), int(at_vertex.sum()))]
    d = targets - origins
    flat = np.nonzero(rng.random(n) < 0.1)[0]
    d[flat, rng.integers(0, 3, len(flat))] = 0.0
    origins[flat] = targets[flat] - d[flat]
    return origins, MC._unit(d)


@pytest.mark.parametrize("name", MC.MESHES)
def test_the_walk_loses_no_crossing_of_the_brute_force_loop_over_200000_rays(name):
    case = MC.mesh(name)
    o, d = random_rays(case, N_RANDOM, 77 + MC.MESHES.index(name))
    got = O.bvh_walk_check(case.vertices, case.faces, o, d)
    print(f"bvh-walk {name} random: {got['checked']} crossings of {N_RANDOM} rays, least slack / pad = {got['min_slack']:.4f} "
          f"(ray {got['at'][0]}, face {got['at'][1]}, axis {got['at'][2]}), {got['leaves'] / N_RANDOM:.1f} leaves a ray, most {got['most_leaves']}")
    assert got["checked"] > N_RANDOM // 4
    assert got["lost"] == 0, (name, got["first_lost"], o[got["first_lost"][0]].tolist(), d[got["first_lost"][0]].tolist())
    assert got["min_slack"] >= CLAIM, (name, got, o[got["at"][0]].tolist(), d[got["at"][0]].tolist())


def test_a_tree_as_deep_as_the_large_balls_loses_no_crossing():
    """`deep`, 81 920 faces: G and E rays against the brute-force loop (never through the exact reference)."""
    case = MC.mesh("deep")
    for family, n in MC.DEEP_RAYS.items():
        o, d, _ = MC.deep_rays(family)
        got = O.bvh_walk_check(case.vertices, case.faces, o, d)
        print(f"bvh-walk deep {family}: depth {got['depth']}, {got['checked']} crossings, least slack / pad = {got['min_slack']:.4f}")
        assert got["depth"] >= 17 and got["checked"] > n
        assert got["lost"] == 0, (family, got["first_lost"])
        near = np.sqrt(np.sum((o - case.centre) ** 2, axis=1)) <= 2.0e3 * case.diag
        part = O.bvh_walk_check(case.vertices, case.faces, o[near], d[near])
        assert part["min_slack"] >= CLAIM, (family, part)


def test_the_queue_of_deferred_leaves_is_refilled_many_times_on_the_small_ball():
    """What `scale` is for: a ray near the 1e-3 ball, whose triangles are of the pad's size, reaches dozens of leaves: the
    eight slots a lane notes leaves in before its triangles are tested fill four times and more in one walk."""
    case = MC.mesh("scale")
    o, d, _ = MC.rays("scale", "E")
    got = O.bvh_walk_check(case.vertices, case.faces, o, d)
    assert got["most_leaves"] >= 4 * 8, got
