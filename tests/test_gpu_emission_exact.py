"""The kernel's emitter (`emit_one`: compiled into `emit_kernel`, `emit_chunk` and `emit_chunk_park`) and its built-in
phase turns at the scatter site of the trace loop against the float64 restatement of the rule (tests/exact_emission.py),
bit for bit and ray for ray.  The restatement itself is held to the exact rule within derived bounds on the CPU
(tests/test_emission_exact.py), so equality with it places every device value within those bounds as well.

  * `DeviceScene.emit` on every case of the table, with 1 024 rays and with 1 000 (a partial last block);
  * the GENERATE rows of history launches of a plain scene, a scene with more than 64 recorders and an extension-family
    scene (`emit_chunk`), a launch at ray_offset 2^40 + 3 and a ray traced alone;
  * a carried stream that parks on a lean scene (`emit_chunk_park`).  The parking kernel writes no log, and a captured
    recorder or an origin histogram moves a scene to the extension family, which never parks: that copy is held through
    its integer tallies, which must equal the referee's on the restatement's rays;
  * the scatter site: Henyey-Greenstein 0.9, -0.6 and 1e-11, a cone, the isotropic default and the Lambertian tag on a
    Scatterer, Henyey-Greenstein emission of a luminophore; unrotated, in a rotated node, on a tile of the node grid and
    beside a mesh.  The draws' positions are anchored bit for bit by the isotropic twin of each scene
    (tests/test_gpu_phase_turn_exact.py has the method);
  * the hunt: 2^20 emitted rays and 2^18 first scatters at g = 1e-11, where about one cosine in 10^5 leaves [-1, 1]
    before the clamp: every direction finite, of unit length, equal to the clamped restatement.

Measured on an MI355X: every comparison above is an equality; worst |direction - exact| / bound at the scatter site
0.444 (the cone); clamped rays of the hunts: 14 emitted, 3 scattered (docs/parity_chain.md, device emission)."""
import functools
import math

import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd import (
    Box, FresnelSurfaceDelegate, Luminophore, Material, Mesh, Node, Scatterer, Scene, Surface, lambertian,
)
from pvtrace_amd.material import Cone, HenyeyGreenstein
from pvtrace_amd.engine import Recorder, compile_scene, native
from tests import exact_emission as X
from tests.test_gpu_phase_turn_exact import ALPHA, EMIT, GENERATE, ME, SCATTER, isotropic, turn_events
from tests.test_phase_turn_exact import FIRST_PHASE_DRAW, SEED

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _bundle(case, n=None):
    if not hasattr(case, "_kernel"):
        case._kernel = X.kernel_bundle(case.tables, case.n, case.emit_seed, case.ray_offset)
    pos, dirs, wl = case._kernel[:3]
    return (pos, dirs, wl) if n is None else (pos[:n], dirs[:n], wl[:n])


def block_scene(phase=None, component="scatterer", container="box"):
    """A block of n = 1 holding one component of coefficient ALPHA and quantum yield 1 -> (scene, size of the block, its
    rotation or None).  container: "box" 2 x 2 x 2, "rotated" (the same, turned), "wide" (65 recorders), "mesh" (a mesh
    stands beside the box), "grid" (the middle tile of a 6 x 6 array: the node grid), "rough" (a glass block with a rough
    Fresnel surface: the extension family)."""
    from tests.law_cases import EMS_X, EMS_Y
    kw = {} if phase is None else dict(phase_function=phase)
    if component == "luminophore":
        comp = Luminophore(ALPHA, emission=np.column_stack((EMS_X, EMS_Y)), quantum_yield=1.0, name="dye", **kw)
    else:
        comp = Scatterer(ALPHA, quantum_yield=1.0, name="mist", **kw)
    material = Material(refractive_index=1.0, components=[comp])
    if container == "rough":
        material = Material(refractive_index=1.5, components=[comp], surface=Surface(FresnelSurfaceDelegate(roughness=0.3)))
    if container == "grid":
        from benchmarks.configs import tiles_lsc
        scene = tiles_lsc(6, recorders="all")
        tile = next(n for n in scene.root.children if n.name == "tile-3-3")
        tile.geometry = Box((5.0, 5.0, 1.0), material=material)
        return scene, (5.0, 5.0, 1.0), None, np.asarray(tile.location, dtype=np.float64)
    world = Node(name="world", geometry=Box((64.0, 64.0, 64.0), material=Material(refractive_index=1.0)))
    block = Node(name="block", parent=world, geometry=Box((2.0, 2.0, 2.0), material=material))
    turn = None
    if container == "rotated":
        block.rotate(*X_ROT)
        turn = X.rotation(*X_ROT)
    if container == "wide":
        block.recorders = [Recorder(f"r{i}", event="entering") for i in range(65)]
    if container == "mesh":
        beside = Node(name="beside", parent=world, geometry=Mesh.box((1.0, 1.0, 1.0), material=Material(refractive_index=1.5)))
        beside.location = (6.0, 0.0, 0.0)
    return Scene(world), (2.0, 2.0, 2.0), turn, np.zeros(3)


X_ROT = (0.7, (0.3, -1.0, 0.6))


def inside_rays(n, size, turn, centre, seed=3):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.45, 0.45, (n, 3)) * np.asarray(size)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    if turn is not None:
        pos = pos @ turn.T
    return np.ascontiguousarray(pos + centre), np.ascontiguousarray(v), np.full(n, 555.0)


def trace_draws(n, k):
    return X.stream_array(np.array([X.trace_key(SEED, 0, i) for i in range(n)], dtype=np.uint64), k)


# ------------------------------------------------------------------------------------------------ emit_kernel
@pytest.fixture(scope="module")
def bare():
    world = Node(name="world", geometry=Box((64.0, 64.0, 64.0), material=Material(refractive_index=1.0)))
    Node(name="block", parent=world, geometry=Box((2.0, 2.0, 2.0), material=Material(refractive_index=1.5)))
    return compile_scene(Scene(world))


@pytest.mark.parametrize("n", [1024, 1000])
@pytest.mark.parametrize("case", X.CASES, ids=[c.name for c in X.CASES])
def test_device_emission_equals_the_restatement(bare, case, n):
    want = _bundle(case, n)
    dscene = native.DeviceScene(bare, device=0, emitter=case.tables)
    try:
        got = tuple(t.cpu().numpy() for t in dscene.emit(n, case.emit_seed, ray_offset=case.ray_offset))
    finally:
        dscene.close()
    for g, w, what in zip(got, want, ("position", "direction", "wavelength")):
        assert np.array_equal(g, w), (case.name, what, int((g != w).sum()))


# ------------------------------------------------------------------------------------------------ emit_chunk
def generate_rows(scene, tables, n, emit_seed, ray_offset):
    """The GENERATE rows of a history launch with device emission -> (position, direction, wavelength, launch info)."""
    import torch

    compiled = compile_scene(scene)
    dscene = native.DeviceScene(compiled, device=0, emitter=tables)
    try:
        log = dscene.new_event_columns(n, 1, ME)
        dscene.trace(None, n, SEED, dscene.new_tallies(), log=log, ray_offset=ray_offset, emit_seed=emit_seed,
                     record_every=1, maxsteps=200, max_events=ME)
        torch.cuda.synchronize()
        info = dscene.launch_info()
        counts, kind = log["counts"].cpu().numpy(), log["kind"].cpu().numpy()
        first = np.arange(n) * ME
        assert np.all(counts[:n] >= 1) and np.all(kind[first] == GENERATE)
        return (log["position"].cpu().numpy().reshape(-1, 3)[first], log["direction"].cpu().numpy().reshape(-1, 3)[first],
                log["wavelength"].cpu().numpy()[first], info)
    finally:
        dscene.close()


LAUNCHES = {
    # scene, the family its history launch must run, case
    "plain": (lambda: block_scene()[0], ("lean", "w4"), "R-seven-lights"),
    "wide": (lambda: block_scene(container="wide")[0], ("w4",), "R-seven-lights"),
    "extension": (lambda: block_scene(container="rough")[0], ("rough",), "R-seven-lights"),
    "mesh-offset-2^40": (lambda: block_scene(container="mesh")[0], ("mesh",), "R-offset-2^40"),
    "grid-seed-wraps": (lambda: block_scene(container="grid")[0], ("grid",), "R-seed-wraps"),
}


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_generate_rows_of_a_history_launch_equal_the_restatement(name):
    build, families, case_name = LAUNCHES[name]
    case = X.BY_NAME[case_name]
    n = 1000
    pos, dirs, wl, info = generate_rows(build(), case.tables, n, case.emit_seed, case.ray_offset)
    assert info["variant"] in families, info
    want = _bundle(case, n)
    assert np.array_equal(wl, want[2]) and np.array_equal(pos, want[0]) and np.array_equal(dirs, want[1])


def test_a_ray_traced_alone_is_emitted_like_any_other():
    case = X.BY_NAME["R-seven-lights"]
    want = _bundle(case)
    for i in (0, 3, 777):      # lights 6, 2 and 6 + 777 mod 7
        pos, dirs, wl, _ = generate_rows(block_scene()[0], case.tables, 1, case.emit_seed, case.ray_offset + i)
        assert np.array_equal(pos[0], want[0][i]) and np.array_equal(dirs[0], want[1][i]) and wl[0] == want[2][i]


# ------------------------------------------------------------------------------------------------ emit_chunk_park
def test_a_parking_stream_tallies_the_restatements_rays():
    from benchmarks.configs import tiles_lsc
    from tests.test_gpu_park_variant import MAXSTEPS, PARK, SEED as PARK_SEED, USUAL, assert_equal_tallies, run_stream

    # the seven lights moved above the tile, shining down on it: most rays meet the slab
    lights = []
    for light in X.SEVEN:
        light = dict(light)
        m = np.eye(4)
        m[:3, :3] = X.rotation(math.pi, (1.0, 0.0, 0.0)) @ X.rotation(0.2, (0.3, 1.0, 0.1))
        m[:3, 3] = (0.1, -0.2, 4.0)
        light["pose"] = m
        lights.append(light)
    tables = X.Tables(lights)
    scene = tiles_lsc(1)
    compiled = compile_scene(scene)
    sizes, emit_seed, offset = (2048,) * 4, 2 ** 64 - 3000, 0
    pos, dirs, wl, _, _ = X.kernel_bundle(tables, sum(sizes), emit_seed, offset)
    dscene = native.DeviceScene(compiled, device=0, emitter=tables)
    try:
        carried, entries, _, _ = run_stream(dscene, None, sizes, carry=True, depth=1, emit_seed=emit_seed)
    finally:
        dscene.close()
    cpu = O.trace_bundle(compiled, pos, dirs, wl, PARK_SEED, MAXSTEPS, 128, 0, 8, 0, math_mode=O.MATH_PORTABLE)
    assert entries == [PARK] * 3 + [USUAL]
    assert cpu["rec_distinct"].sum() > 1000
    assert_equal_tallies(carried, cpu, "a parking stream against the referee on the restatement's rays")


# ------------------------------------------------------------------------------------------------ the scatter site
PHASES = {
    "hg-0.9": (lambda: HenyeyGreenstein(0.9), X.DIR_HG, 0.9),
    "hg--0.6": (lambda: HenyeyGreenstein(-0.6), X.DIR_HG, -0.6),
    "hg-1e-11": (lambda: HenyeyGreenstein(1e-11), X.DIR_HG, 1e-11),
    "cone-0.6": (lambda: Cone(0.6), X.DIR_CONE, 0.6),
    "isotropic": (lambda: None, X.DIR_ISOTROPIC, 0.0),
    "lambertian": (lambda: lambertian, X.DIR_CONE, 1.5707963267948966),    # the packer lowers the tag to this cone
}
SITES = [(c, p, "scatterer") for c, ps in (("box", sorted(PHASES)), ("rotated", ("hg-0.9", "cone-0.6")),
                                           ("grid", ("hg-0.9", "cone-0.6")), ("mesh", ("hg--0.6", "lambertian")),
                                           ("wide", ("hg-0.9",))) for p in ps] + [("box", "hg-0.9", "luminophore")]
N_SITE = 1000


@functools.lru_cache(maxsize=None)
def anchor(container, component):
    """The isotropic twin of a site: which rays are absorbed first, bit-for-bit proof of the draws' positions, and the
    wavelength that follows the turn."""
    scene, size, turn, centre = block_scene(None, component, container)
    pos, dirs, wl = inside_rays(N_SITE, size, turn, centre)
    absorbed, kind, direction, wavelength, travelled = turn_events(scene, pos, dirs, wl)
    draws = trace_draws(N_SITE, FIRST_PHASE_DRAW + 2)
    assert absorbed.sum() * 10 >= 4 * N_SITE
    assert np.all(kind[absorbed] == (EMIT if component == "luminophore" else SCATTER))
    depth = -O.math("log", 1.0 - draws[:, 0]) / ALPHA
    assert np.array_equal(travelled[absorbed], depth[absorbed])
    want = isotropic(draws[:, FIRST_PHASE_DRAW], draws[:, FIRST_PHASE_DRAW + 1])
    assert np.array_equal(direction[absorbed], want[absorbed])       # in the WORLD frame, whatever the node's rotation
    return absorbed, wavelength, draws


@pytest.mark.parametrize("container,phase,component", SITES, ids=["-".join(s) for s in SITES])
def test_the_scatter_site_turns_as_the_restatement(container, phase, component):
    make, kind, param = PHASES[phase]
    absorbed0, wavelength0, draws = anchor(container, component)
    scene, size, turn, centre = block_scene(make(), component, container)
    pos, dirs, wl = inside_rays(N_SITE, size, turn, centre)
    launch = {}
    absorbed, rows, direction, wavelength, _ = turn_events(scene, pos, dirs, wl, launch=launch)
    want_family = {"grid": ("grid",), "mesh": ("mesh",), "wide": ("w4",)}.get(container, ("lean", "w4"))
    assert launch["variant"] in want_family, launch
    assert np.array_equal(absorbed, absorbed0)                       # the same draws up to the turn
    assert np.all(rows[absorbed] == (EMIT if component == "luminophore" else SCATTER))
    k = FIRST_PHASE_DRAW
    worst = 0.0
    for i in np.flatnonzero(absorbed):
        u = (draws[i, k], draws[i, k + 1])
        want, _ = X.kernel_turn(kind, param, u)
        assert tuple(direction[i]) == want, (i, u)
        if i % 4 == 0:      # the exact rule's bound, on a quarter of the rays (every one is EQUAL to the restatement)
            exact, bound, _ = X.exact_turn(kind, param, u)
            for a in range(3):
                err = abs(float(X._mp(X.F(float(direction[i, a]))) - exact[a]))
                worst = max(worst, err / bound[a] if err else 0.0)
    print(f"{container} {phase} {component}: worst |direction - exact| / bound = {worst:.3f}")
    assert worst <= 1.0
    # every built-in turn takes two draws, so what follows -- a luminophore's wavelength -- is the isotropic twin's
    assert np.array_equal(wavelength[absorbed], wavelength0[absorbed])
    if component == "luminophore":
        assert np.any(wavelength[absorbed] != 555.0)


# ------------------------------------------------------------------------------------------------ the hunt
HUNT_G = 1e-11
HUNT_EMIT_SEED = 2          # chosen on the CPU: the restatement names rays beyond the clamp at these seeds (asserted)


def test_hunt_emission_at_a_vanishing_asymmetry(bare):
    n = 2 ** 20
    tables = X.Tables([dict(dir=(X.DIR_HG, HUNT_G))])
    u = X.stream_array(X.emit_keys(HUNT_EMIT_SEED, 0, n), 2)
    want, raw = X.hg_turns(HUNT_G, u[:, 0], u[:, 1])
    beyond = np.flatnonzero(np.abs(raw) > 1.0)
    print("emitted rays whose cosine leaves [-1, 1] before the clamp:", len(beyond))
    assert len(beyond) >= 5
    dscene = native.DeviceScene(bare, device=0, emitter=tables)
    try:
        pos, dirs, wl = (t.cpu().numpy() for t in dscene.emit(n, HUNT_EMIT_SEED))
    finally:
        dscene.close()
    assert np.all(np.isfinite(dirs))
    assert np.max(np.abs((dirs * dirs).sum(axis=1) - 1.0)) <= 8.0 * U
    assert np.array_equal(dirs[beyond], want[beyond]) and np.all(np.abs(dirs[beyond, 2]) == 1.0)
    assert np.array_equal(dirs, want) and not pos.any() and np.all(wl == 555.0)
    for i in beyond[:3]:     # ... and the scalar restatement on the named rays
        assert list(dirs[i]) == X.kernel_emit(tables, HUNT_EMIT_SEED, int(i))[1]


def test_hunt_first_scatters_at_a_vanishing_asymmetry():
    n = 2 ** 18
    scene, size, turn, centre = block_scene(HenyeyGreenstein(HUNT_G))
    pos, dirs, wl = inside_rays(n, size, turn, centre, seed=8)
    with np.errstate(over="ignore"):
        keys = np.uint64(SEED) + np.arange(n, dtype=np.uint64)
    draws = X.stream_array(keys, FIRST_PHASE_DRAW + 2)
    want, raw = X.hg_turns(HUNT_G, draws[:, FIRST_PHASE_DRAW], draws[:, FIRST_PHASE_DRAW + 1])
    absorbed, rows, direction, _, travelled = turn_events(scene, pos, dirs, wl)
    assert np.array_equal(travelled[absorbed], (-O.math("log", 1.0 - draws[:, 0]) / ALPHA)[absorbed])
    beyond = np.flatnonzero((np.abs(raw) > 1.0) & absorbed)
    print("first scatters whose cosine leaves [-1, 1] before the clamp:", len(beyond))
    assert len(beyond) >= 2
    got = direction[absorbed]
    assert np.all(rows[absorbed] == SCATTER) and np.all(np.isfinite(got))
    assert np.max(np.abs((got * got).sum(axis=1) - 1.0)) <= 8.0 * U
    assert np.array_equal(direction[beyond], want[beyond])
    assert np.array_equal(got, want[absorbed])
