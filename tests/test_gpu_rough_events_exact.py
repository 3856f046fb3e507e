"""The kernel's rough-surface event (`rough_event_call`, pvt_trace_kernel.h) against the exact reference of the
PvtSurfaceTables contract (tests/exact_events.py), one event at a time.

A host ray that meets a rough node first draws u_a, u_b and (when R > 0) u: the first three uniforms of its stream
`seed + index` -- neither the world nor the node absorbs, so no free path is drawn before.  The row after GENERATE holds
the event's kind, the new direction and the geometric normal the kernel handed to the sampler, so one step and three
draws are replayed, nothing else; the reference takes the LOGGED normal, and so does not depend on the intersection
arithmetic or on how a rotated node's normal was rounded.  The anchor tests fix the draw position on the same nodes
with alpha = 0, bit for bit against the referee's reflection and refraction; the rough cases (tests/exact_events.py:
generic rays on a box, a rotated box, a sphere, a cylinder, a 12-triangle mesh and a tile of a node-grid scene, alpha
from 1e-4 to 1, both orders of the indices, n1 = n2 and an index table; exact normal incidence, signed zeros, grazing
incidence, the critical angle and rays inside a coordinate plane) then hold the kind and the direction to the reference
within the derived bound.  The same rays hold the host sampler in tests/test_rough_events_exact.py.  The draw order
behind an index-matched interface, where the kernel's R is 0 or a rounding residue, is held on the SECOND event of the
nested case, replayed at both stream positions (tests/exact_events.py, "n1 = n2 and the draw u").

Measured on an MI355X (worst |direction - exact| / bound): 0.074 in the generic family, 0.085 in the edge family (the
critical angle at alpha = 1e-4); no ray of any case is ambiguous; behind the matched interface 811 of 1000 rays skipped
u and 189 drew it (docs/parity_chain.md, rough interfaces, which also lists the kernel faults tried)."""
import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd.engine import Session, compile_scene, native
from pvtrace_amd.material import rough_fresnel_reflectivity
from tests import exact_events as X
from tests.test_rough_events_exact import SEED, case_inputs

pytestmark = pytest.mark.gpu

GENERATE, REFLECT, TRANSMIT = 0, 1, 2


def events(scene, pos, dirs, wl, rows=(1,), variants=None):
    """The events `rows` after GENERATE of every ray (1: the first), of one launch: (kind, direction, normal) of each.
    `variants`: a list that receives the name of the kernel family the launch ran."""
    n, me = len(pos), max(rows) + 2   # (GENERATE, the events, and the KILL row that ends a full log)
    with Session(scene, emission="host") as session:
        result = session.collect(session.submit(n, SEED, host_rays=(pos, dirs, wl, ["r"] * n), record_every=1,
                                                max_events=me))
        data = {k: np.asarray(result.data[k]).copy() for k in ("counts", "kind", "direction", "normal")}
        if variants is not None:
            variants.append(session.dscene.launch_info()["variant"])
    assert np.all(data["counts"] >= max(rows) + 1)
    first = np.arange(n) * me
    assert np.all(data["kind"][first] == GENERATE)
    out = []
    for row in rows:
        kind = data["kind"][first + row]
        assert np.all(np.isin(kind, (REFLECT, TRANSMIT)))
        out.append((kind, data["direction"].reshape(-1, 3)[first + row], data["normal"].reshape(-1, 3)[first + row]))
    return out


def first_events(scene, pos, dirs, wl):
    return events(scene, pos, dirs, wl)[0]


ANCHORS = ["G-box-rotated-0.05", "G-sphere-0.3", "G-mesh-0.3", "G-tile-0.3", "G-box-rotated-index-table-0.3"]


@pytest.mark.parametrize("name", ANCHORS)
def test_anchor_a_smooth_node_decides_its_first_surface_event_with_the_first_draw(name):
    """alpha = 0: the event is REFLECT exactly when draw 0 of the stream is below the Fresnel R, and the new direction
    is the referee's specular reflection or refraction about the logged normal, bit for bit."""
    case = X.ROUGH_BY_NAME[name]
    scene, _, _, _, pos, dirs, wl, inside, n1, n2, draws = case_inputs(case, alpha=0.0)
    kind, direction, normal = first_events(scene, pos, dirs, wl)
    u = draws[:, 0]
    assert np.array_equal(np.sum(normal * dirs, axis=1) > 0.0, inside)
    seen = set()
    for i in range(case.n):
        c = abs(float(np.dot(normal[i], dirs[i])))
        R = rough_fresnel_reflectivity(c, float(n1[i]), float(n2[i]))       # (Hecht's formula about the normal itself)
        if abs(u[i] - R) > 1e-9:
            assert (kind[i] == REFLECT) == (u[i] < R), (name, i, u[i], R)
        if kind[i] == REFLECT:
            want = O.specular_reflect(dirs[i], normal[i])
        else:
            along = normal[i] if np.dot(normal[i], dirs[i]) >= 0.0 else -normal[i]
            want = O.fresnel_refract(dirs[i], along, float(n1[i]), float(n2[i]))
        assert np.array_equal(direction[i], want), (name, i, kind[i], direction[i], want)
        seen.add((int(kind[i]), bool(inside[i]), R == 1.0))
    # reflections and refractions from both sides, and total internal reflection from inside
    assert {(REFLECT, False, False), (TRANSMIT, False, False), (TRANSMIT, True, False), (REFLECT, True, True)} <= seen


@pytest.mark.parametrize("case", X.ROUGH_CASES, ids=[c.name for c in X.ROUGH_CASES])
def test_the_kernel_event_agrees_with_the_exact_reference_ray_by_ray(case):
    scene, _, _, _, pos, dirs, wl, inside, n1, n2, draws = case_inputs(case)
    kind, direction, normal = first_events(scene, pos, dirs, wl)
    assert np.array_equal(np.sum(normal * dirs, axis=1) > 0.0, inside)       # (every ray met the node it was aimed at)
    refs = X.rough_refs(case, dirs, normal, n1, n2, draws, X.TRIG_KERNEL)
    X.check_rough_conditions(case, refs)
    X.judge_rough(case, refs, [(kind[i] == REFLECT, direction[i]) for i in range(case.n)], "kernel")


def test_the_tile_case_runs_the_node_grid_walk_of_the_rough_family():
    """G-tile-0.3 is there for `trace_kernel_rough_grid`: choose_variant (pvt_trace.hip) takes it for a scene of the
    extension family whose nodes are filed in a node grid (plan_node_grid: at least 8 nodes, rigid boxes, spheres or
    cylinders only) and whose tables are staged in LDS -- 37 plain boxes are a few hundred bytes of tables."""
    case = X.ROUGH_BY_NAME["G-tile-0.3"]
    scene, _, compiled, _, pos, dirs, wl, _, _, _, _ = case_inputs(case)
    assert len(compiled.node_names) == 37 and native.node_grid_plan(compiled) is not None
    variants = []
    events(scene, pos[:8], dirs[:8], wl[:8], variants=variants)
    assert variants == ["rough"]
    # (and the other generic scenes are not: one or two nodes in a world)
    for name in ("G-box-0.3", "G-nested-matched-0.3"):
        assert native.node_grid_plan(compile_scene(X.ROUGH_BY_NAME[name].scene()[0])) is None


def test_a_matched_rough_interface_moves_the_later_draws_only_where_its_residue_of_r_is_above_zero():
    """The draw order of items 4 and 7 BEHIND an index-matched rough interface (tests/exact_events.py, "n1 = n2 and the
    draw u").  Every ray of G-nested-matched-0.3 crosses the matched outer box (event 1: TRANSMIT, the direction kept
    to a rounding) and then meets the rough glass box inside it (event 2).  Event 2 is replayed from the log -- the
    direction of row 1, the normal of row 2, (n1, n2) = (1, 1.5) -- with u_a, u_b, u at stream positions 2, 3, 4 (event 1
    drew no u) and at 3, 4, 5 (it drew one); each ray must agree with exactly one replay and both must occur.
    Measured on an MI355X: 811 rays at the first position, 189 at the second."""
    case = X.ROUGH_BY_NAME["G-nested-matched-0.3"]
    scene, _, _, _, pos, dirs, wl, inside, _, _, _ = case_inputs(case)
    (kind1, direction1, _), (kind2, direction2, normal2) = events(scene, pos, dirs, wl, rows=(1, 2))
    assert not inside.any() and np.all(kind1 == TRANSMIT)
    assert np.all(np.sum(normal2 * direction1, axis=1) < 0.0)                # (event 2: entering the inner box)
    stream = np.array([O.uniforms(SEED + i, 6) for i in range(case.n)])
    n1, n2 = np.ones(case.n), np.full(case.n, X.N_GLASS)
    refs = [X.rough_refs(case, direction1, normal2, n1, n2, stream[:, k:k + 3], X.TRIG_KERNEL) for k in (2, 3)]
    for r in refs:   # (the replays themselves are well conditioned: the conditions of a generic case, but its kinds)
        assert sum(x.ambiguous for x in r) * 100 <= case.n
        assert sum(x.bound(x.reflect) < 1e-12 for x in r) * 100 >= 99 * case.n
    X.judge_draw_order(case, refs[0], refs[1], [(kind2[i] == REFLECT, direction2[i]) for i in range(case.n)], "kernel")
