"""The CPU referee with refractive-index and coating reflectivity tables, anchored to the reference before it judges
the GPU (tests/test_gpu_table_parity.py).

The referee traces the two slabs behind the reference-tracer fixtures -- the dispersive Lumogen slab
(tests/golden/dispersion_tracer.npz) and the slab under a wavelength- and angle-selective mirror
(tests/golden/coating_table_tracer.npz) -- and must land within 5 standard errors (Welch) of the reference's own Python
tracer on every outcome share and (dispersion) mean event count, and far from the fixture's scalar / mirrorless run: the
same checks the GPU tests apply.  The step tables of the hand-traced rays decide every ray exactly as the host tracer
does.  Without a GPU."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd import (
    Box, CoatedSurfaceDelegate, Coating, Light, Luminophore, Material, Node, ReflectivityTable, RefractiveIndexTable,
    Scene, Surface, rectangular_mask,
)
from pvtrace_amd.data import lumogen_f_red_305
from pvtrace_amd.engine import compile_scene
from pvtrace_amd.engine.emit import emit_bundle
from pvtrace_amd.light import ConstantWavelengthMask
from tests import coating_table_scene as S
from tests import dispersion_scene as D
from tests.util import load_golden

THREADS = max(1, min(os.cpu_count() or 1, 8))
MAX_EVENTS = 2100


def welch(a, b):
    """|mean(a) - mean(b)| in standard errors (Welch)."""
    se = np.sqrt(a.var(axis=0, ddof=1) / len(a) + b.var(axis=0, ddof=1) / len(b))
    diff = np.abs(a.mean(axis=0) - b.mean(axis=0))
    return np.where(se > 0, diff / np.where(se > 0, se, 1.0), np.where(diff > 0, np.inf, 0.0))


def oracle_outcomes(scene, n, seed):
    """Per-ray outcome classes and event counts of `scene` traced by the referee (host emission, full histories)."""
    compiled = compile_scene(scene)
    pos, dirs, wl, _ = emit_bundle(scene, n, seed=seed)
    data = O.trace_bundle(compiled, pos, dirs, wl, seed + 1, 1000, MAX_EVENTS, 0, THREADS, 1, math_mode=O.MATH_PORTABLE)
    counts_per_ray = data["counts"].astype(np.int64)
    assert counts_per_ray.max() < MAX_EVENTS
    kind = data["kind"].reshape(n, MAX_EVENTS)
    position = data["position"].reshape(n, MAX_EVENTS, 3)
    rows = np.arange(n)
    last = kind[rows, counts_per_ray - 1].astype(np.int64)
    where = np.where((last == 7)[:, None], position[rows, np.maximum(counts_per_ray - 2, 0)],
                     position[rows, counts_per_ray - 1])
    mask = np.arange(MAX_EVENTS)[None, :] < counts_per_ray[:, None]
    counts = np.stack([np.sum((kind == k) & mask, axis=1) for k in range(10)], axis=1).astype(float)
    return D.outcome_class(last, where), counts, compiled


def test_dispersive_slab_against_the_references_python_tracer():
    g = load_golden("dispersion_tracer.npz")
    scene, _ = D.build(Node, Scene, Box, Material, Surface, Light, rectangular_mask, ConstantWavelengthMask(D.PUMP_NM),
                       D.components(Luminophore, lumogen_f_red_305),
                       index=RefractiveIndexTable(D.DISP_WAVELENGTH, D.DISP_VALUE))
    outcome, counts, compiled = oracle_outcomes(scene, 12000, 31)
    assert compiled.n_ri_tables == 1
    one_hot = np.eye(5)[outcome][:, :4]    # exit-facet shares: top, bottom, edge, lost
    ref = {k: (np.eye(5)[g[f"{k}/outcome"].astype(int)][:, :4], g[f"{k}/event_counts"].astype(float))
           for k in ("dispersive", "scalar")}
    z_share = welch(one_hot, ref["dispersive"][0])
    assert np.all(z_share < 5.0), dict(zip(D.CLASSES, z_share))
    z_events = welch(counts, ref["dispersive"][1])
    assert np.all(z_events < 5.0), z_events
    # power: the dispersive referee run is far from the reference's scalar run
    z_power = np.concatenate([welch(one_hot, ref["scalar"][0]), welch(counts, ref["scalar"][1])])
    assert z_power.max() > 5.0, z_power


def test_selective_mirror_against_the_references_python_tracer():
    g = load_golden("coating_table_tracer.npz")
    table = ReflectivityTable(S.MIRROR_WAVELENGTH, S.MIRROR_VALUE, angle=S.MIRROR_ANGLE)
    runs = {}
    for key, delegate in (("mirror", CoatedSurfaceDelegate([Coating((0, 0, 1), reflectivity=table)])), ("plain", None)):
        scene, _ = S.build(Node, Scene, Box, Material, Surface, Light, rectangular_mask, ConstantWavelengthMask(S.PUMP_NM),
                           S.components(Luminophore, lumogen_f_red_305), delegate=delegate)
        outcome, _, compiled = oracle_outcomes(scene, 20000, 13)
        assert compiled.n_coat_tables == (1 if key == "mirror" else 0)
        runs[key] = np.eye(5)[outcome][:, :4]
    ref = {k: np.eye(5)[g[f"{k}/outcome"].astype(int)][:, :4] for k in ("mirror", "plain")}
    z_mirror = welch(runs["mirror"], ref["mirror"])
    assert np.all(z_mirror < 5.0), dict(zip(S.CLASSES, z_mirror))
    z_plain = welch(runs["plain"], ref["plain"])
    assert np.all(z_plain < 5.0), dict(zip(S.CLASSES, z_plain))
    # power: the referee's mirror run is far from the reference's mirrorless run, and the other way round
    assert welch(runs["mirror"], ref["plain"]).max() > 5.0
    assert welch(runs["plain"], ref["mirror"]).max() > 5.0


@pytest.mark.parametrize("case", range(len(S.STEP_CASES)))
def test_step_tables_decide_hand_traced_rays_on_the_referee(case):
    """tests/test_gpu_coating_tables.py::test_step_tables_* on the referee: the same events as the host tracer, and
    every column of the log equal to that of the block whose top face has the scalar R the step gives."""
    from pvtrace_amd.algorithm import photon_tracer

    make, theta, wl, reflected = S.STEP_CASES[case]
    scene = S.step_scene(make(ReflectivityTable))
    host = photon_tracer.follow(scene, S.step_ray(theta, wl), backend="host")
    assert [e.name for _, e in host] == (["GENERATE", "REFLECT", "EXIT"] if reflected else ["GENERATE", "TRANSMIT", "TRANSMIT", "EXIT"])
    ray = S.step_ray(theta, wl)
    args = (np.array([ray.position]), np.array([ray.direction]), np.array([wl]), 3, 1000, 16, 0, 1, 1)
    got = O.trace_bundle(compile_scene(scene), *args, math_mode=O.MATH_PORTABLE)
    want = O.trace_bundle(compile_scene(S.step_scene(1.0 if reflected else 0.0)), *args, math_mode=O.MATH_PORTABLE)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    k = int(got["counts"][0])
    assert [int(v) for v in got["kind"][:k]] == [int(e.value) for _, e in host]
    for row, (r, _) in enumerate(host):
        assert np.allclose(got["position"][row], r.position, rtol=0, atol=1e-12)
        assert np.allclose(got["direction"][row], r.direction, rtol=0, atol=1e-12)
