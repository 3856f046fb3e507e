"""Scenes and the step-by-step judge shared by tests/test_mesh_exact.py (through the referee, no GPU) and
tests/test_gpu_mesh_exact.py (the kernel): one mesh of tests/mesh_cases.py, in its own frame, inside an analytic world sphere.

With the mesh's refractive index equal to the world's and no components a photon passes undeviated and draws nothing; with
`record_every=1` its history lists the crossings along its line, one surface row each, and every crossing is found by a fresh
intersection from the previous, LOGGED, position -- an origin on the surface, which is what `t > kEps` is for."""
import functools

import numpy as np

from pvtrace_amd import Light, Material, Mesh, Node, Scene, Sphere
from pvtrace_amd.engine import compile_scene
from tests import mesh_cases as MC

U = MC.U
GENERATE, TRANSMIT, REFLECT, EXIT = 0, 2, 1, 7
MAX_EVENTS = 20
WORLD, MESH = 0, 1            # node ids, in the order the scene is compiled


@functools.lru_cache(maxsize=None)
def scene(name, index=1.0):
    case = MC.mesh(name)
    world = Node(name="world", geometry=Sphere(MC.WORLD_RADIUS, material=Material(refractive_index=1.0)))
    geometry = Mesh((case.vertices, case.faces), material=Material(refractive_index=index), recenter=False)
    assert np.array_equal(geometry.vertices, case.vertices) and np.array_equal(geometry.faces, case.faces)
    Node(name="mesh", parent=world, geometry=geometry)
    Node(name="lamp", parent=world, light=Light(name="lamp"))
    sc = Scene(world)
    return sc, compile_scene(sc), geometry


def trace(tracer, name, family, index=1.0, rays=None, threads=1, **kw):
    """One launch of a family through `tracer` (the kernel's or the referee's trace_bundle)."""
    _, compiled, _ = scene(name, index)
    o, d, _ = MC.rays(name, family) if rays is None else rays
    wl = np.full(len(o), 555.0)
    return tracer(compiled, o, d, wl, 11, 1000, MAX_EVENTS, 0, threads, 1, **kw)


def judge_history(case, normals, data, j):
    """Every step of ray j's history judged from the preceding row AS LOGGED: the exact reference, started at that row's
    position and direction, gives the nearest crossing beyond kEps; the next row must be a surface row of the mesh whose
    `travelled` difference lies within B of it, whose position lies within the bound that follows from B and the advance
    p + d * t, and whose normal is the stored normal of the exact face (or of a face of its group).  When the reference says
    no crossing remains the next row is the world's exit and the last.

    Bounds beyond B: travelled' = travelled + t rounds once (u |travelled'|) and the difference taken here once more;
    p'_a = p_a + d_a * t rounds the product and the sum, and so does the evaluation of the reference point here:
    |p'_a - (p_a + d_a t*)| <= |d_a| B + 4u (|p_a| + |d_a t*|).

    -> (problem or None, steps judged, worst ratio of a travelled difference to its bound, set aside: why or None)"""
    n = int(data["counts"][j])
    rows = slice(j * MAX_EVENTS, j * MAX_EVENTS + n)
    kind, hit = data["kind"][rows], data["hit"][rows]
    pos, dirs, nrm, trav = data["position"][rows], data["direction"][rows], data["normal"][rows], data["travelled"][rows]
    if n < 1 or kind[0] != GENERATE:
        return "no GENERATE row", 0, 0.0, None
    worst, steps = 0.0, 0
    for k in range(n):
        if k == n - 1 and kind[k] == EXIT and hit[k] == WORLD:
            break
        ref = MC.exact(case, pos[k], dirs[k])
        if ref.ambiguous:
            return None, steps, worst, ref.ambiguous
        if not ref.crossings:
            if k == n - 1 and kind[k] != EXIT:
                return f"row {k}: the history ends without the world's exit", steps, worst, None
            if k < n - 1 and not (kind[k + 1] == EXIT and hit[k + 1] == WORLD and k + 1 == n - 1):
                return f"row {k + 1}: kind {kind[k + 1]} on node {hit[k + 1]} where no crossing remains (an invented crossing)", steps, worst, None
            return None, steps, worst, None
        if k == n - 1:
            return f"row {k}: the history ends with {len(ref.crossings)} crossings ahead (a lost crossing)", steps, worst, None
        first = ref.crossings[0]
        reach = max(t + b for t, b in first.faces.values())
        allowed = {}
        for c in ref.crossings:
            if min(t - b for t, b in c.faces.values()) <= reach:      # (crossings the bounds cannot order: either may come first)
                allowed.update(c.faces)
        if not (kind[k + 1] == TRANSMIT and hit[k + 1] == MESH):
            return f"row {k + 1}: kind {kind[k + 1]} on node {hit[k + 1]}, the exact reference crosses face(s) {sorted(first.faces)} at {first.t!r}", steps, worst, None
        faces = [f for f in allowed if np.array_equal(normals[f], nrm[k + 1])]
        if not faces:
            return f"row {k + 1}: normal {nrm[k + 1].tolist()} is the stored normal of none of the faces {sorted(allowed)}", steps, worst, None
        step = trav[k + 1] - trav[k]
        ok = False
        for f in faces:
            t, b = allowed[f]
            bt = b + 2.0 * U * abs(trav[k + 1])
            bp = np.abs(dirs[k]) * b + 4.0 * U * (np.abs(pos[k]) + np.abs(dirs[k] * t))
            if abs(step - t) <= bt and np.all(np.abs(pos[k + 1] - (pos[k] + dirs[k] * t)) <= bp):
                ok = True
                worst = max(worst, abs(step - t) / bt)
                break
        if not ok:
            t, b = allowed[faces[0]]
            return (f"row {k + 1}: advanced by {step!r} to {pos[k + 1].tolist()}, the exact reference crosses face {faces[0]} at {t!r} "
                    f"(bound {b!r})"), steps, worst, None
        steps += 1
    return None, steps, worst, None


def judge_family(case, normals, data, n_rays):
    """-> (problems [(ray, text)], steps judged, worst ratio, rays set aside)"""
    problems, steps, worst, aside = [], 0, 0.0, 0
    for j in range(n_rays):
        problem, s, w, why = judge_history(case, normals, data, j)
        steps += s
        worst = max(worst, w)
        aside += why is not None
        if problem:
            problems.append((j, problem))
    return problems, steps, worst, aside
