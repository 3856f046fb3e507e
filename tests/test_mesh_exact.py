"""The host restatement of the triangle test (`mesh.ray_triangle_distances`) and the referee's (`oracle.mesh_hits`, the
`tri_hit` of oracle/pvt_oracle.c) held, ray by ray, to the EXACT reference of tests/mesh_cases.py: the same number of
crossings, every distance within the bound B derived there, every face the exact face or its neighbour across an interior
edge the ray passes within the bound of.  Before this file the three copies of the test were only compared with each other.

Measured worst |t - exact| / B per family: docs/parity_chain.md, "Triangle meshes"."""
import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd import mesh as M
from tests import mesh_cases as MC

CASES = [(name, family) for name in MC.MESHES for family in MC.FAMILIES]


def _host(case, o, d):
    return M.ray_triangle_distances(case.vertices, case.faces, o, d)


def _oracle(case, o, d):
    ts, faces = O.mesh_hits(case.vertices, case.faces, o, d)
    order = np.lexsort((faces, ts))
    return ts[order], faces[order]


@pytest.mark.parametrize("name,family", CASES)
def test_the_reference_alone_sets_aside_at_most_two_percent_of_a_family(name, family):
    refs = MC.references(name, family)
    assert 300 <= len(refs) <= 600
    aside = [r.ambiguous for r in refs if r.ambiguous]
    assert len(aside) <= MC.MAX_AMBIGUOUS * len(refs), (name, family, len(aside), aside[:3])
    assert any(r.crossings for r in refs)


def test_family_e_passes_within_1e_12_of_an_edges_size_of_an_edge():
    """From the reference alone: at least a quarter of the rays of family E run closer to an edge's line than 1e-12 of the
    edge's size (the displacements of 0, 1 and 2 ulp and of 1e-15 of the size do; the direction's own rounding is of that
    order)."""
    for name in MC.MESHES:
        case = MC.mesh(name)
        tri = case.vertices[case.faces]
        size = float(np.median(np.sqrt(np.sum((tri[:, 1] - tri[:, 0]) ** 2, axis=1))))
        refs = MC.references(name, "E")
        close = sum(1 for r in refs if r.edge_distance <= 1e-12 * size)
        assert close >= 0.25 * len(refs), (name, close, len(refs))


@pytest.mark.parametrize("which", ["host", "oracle"])
@pytest.mark.parametrize("name,family", CASES)
def test_every_crossing_is_the_exact_one_within_the_derived_bound(name, family, which):
    case = MC.mesh(name)
    o, d, _ = MC.rays(name, family)
    refs = MC.references(name, family)
    hits = _host if which == "host" else _oracle
    worst, judged = 0.0, 0
    for j, ref in enumerate(refs):
        if ref.ambiguous:
            continue
        ts, faces = hits(case, o[j], d[j])
        problem, ratio = MC.judge(case, ref, ts, faces)
        assert problem is None, (name, family, which, j, o[j].tolist(), d[j].tolist(), problem)
        worst = max(worst, ratio)
        judged += 1
    print(f"mesh-exact {which} {name} {family}: {judged} rays judged, worst |t - exact| / B = {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("name,family", CASES)
def test_closed_parts_are_crossed_an_even_number_of_times_from_outside_and_an_odd_number_from_inside(name, family):
    """Free of any decision of the reference's: an unambiguous ray from outside a closed part crosses it an even number of
    times, from inside an odd number -- counted by the exact reference, and the host's and the referee's lists must give
    the same counts, part by part."""
    case = MC.mesh(name)
    o, d, where = MC.rays(name, family)
    refs = MC.references(name, family)
    known = 0
    for j, ref in enumerate(refs):
        if ref.ambiguous:
            continue
        want = ref.counts(case)
        for hits in (_host, _oracle):
            _, faces = hits(case, o[j], d[j])
            got = np.bincount(case.part[faces], minlength=case.n_parts).tolist() if len(faces) else [0] * case.n_parts
            assert got == want, (name, family, j, got, want)
        if where[j] == -2:
            continue                     # (an origin inside the root box or on it: which side it is on is not known by construction)
        known += 1
        for part, count in enumerate(want):
            assert count % 2 == (1 if part == where[j] else 0), (name, family, j, part, count, int(where[j]))
    assert known > 0 or family == "P"
