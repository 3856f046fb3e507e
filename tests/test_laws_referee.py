"""The CPU referee (oracle/pvt_oracle.c, portable arithmetic -- the GPU's bits) held to closed-form laws.

The parity tests pin the HIP kernel to the referee bit for bit, but for the features the reference's kernel cannot
run (coating and index tables, scalar and Lambertian coatings, hist=True spectra, the Lambertian phase tag, source
filters, per-ray-stream emission) the referee is the project's own restatement of the rules: a misreading shared by
both would pass every parity test.  These cases hold the referee's samples to laws written independently of it
(tests/laws.py, from the scene's own tables); tests/test_gpu_laws.py runs the same cases on the GPU at 2.5-10 times
the photons (here 4e5 for laws read from event-log rows, 1e6 from recorders).  Each case's docstring
(tests/law_cases.py) gives its n and the smallest effect it resolves.
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd.engine import compile_scene
from pvtrace_amd.engine.emit import EmitterTables
from tests import law_cases as C

THREADS = max(1, min(8, os.cpu_count() or 1))


class Referee:
    """Traces through the referee in MATH_PORTABLE mode; pencils are replicated rays."""
    n_hist = 400_000
    n_tally = 1_000_000

    def trace_pencil(self, scene, start, direction, wavelength, n, seed, record_every, max_events=4, maxsteps=1000,
                     emit_method=2):
        compiled = compile_scene(scene)
        pos = np.tile(np.asarray(start, float), (n, 1))
        dirs = np.tile(np.asarray(direction, float), (n, 1))
        data = O.trace_bundle(compiled, pos, dirs, np.full(n, float(wavelength)), seed, maxsteps, max_events,
                              emit_method, THREADS, record_every, math_mode=O.MATH_PORTABLE)
        return data, compiled

    def trace_emitted(self, scene, n, seed, emit_seed, maxsteps=1000, emit_method=2):
        """Tally mode on rays of the per-ray-stream emitter."""
        compiled = compile_scene(scene)
        pos, dirs, wl = self.emit(scene, n, emit_seed)
        data = O.trace_bundle(compiled, pos, dirs, wl, seed, maxsteps, 4, emit_method, THREADS, 0,
                              math_mode=O.MATH_PORTABLE)
        return data, compiled

    def emit(self, scene, n, emit_seed):
        return O.emit(EmitterTables(scene), n, emit_seed=emit_seed)


B = Referee()


@pytest.mark.parametrize("key", sorted(C.FRESNEL_OUTSIDE))
def test_fresnel_from_outside(key):
    C.fresnel_outside(B, key)


@pytest.mark.parametrize("key", sorted(C.FRESNEL_INSIDE))
def test_fresnel_from_inside(key):
    C.fresnel_inside(B, key)


@pytest.mark.parametrize("key", sorted(C.DISPERSION_WL))
def test_fresnel_at_tabulated_index(key):
    C.fresnel_dispersive(B, key)


@pytest.mark.parametrize("key", sorted(C.COAT_OUTSIDE))
def test_coating_table_from_outside(key):
    C.coating_table_outside(B, key)


@pytest.mark.parametrize("key", ["arriving", "tir-fresnel", "tir-matched"])
def test_coating_table_from_inside(key):
    C.coating_table_inside(B, key)


def test_lambertian_coating():
    C.lambertian_coating(B)


@pytest.mark.parametrize("hist", [False, True], ids=["linear", "hist"])
@pytest.mark.parametrize("key", sorted(C.BEER_WL))
def test_beer_lambert_at_tabulated_coefficients(key, hist):
    C.beer_lambert_spectra(B, key, hist)


@pytest.mark.parametrize("key", sorted(C.BEER_CONST))
def test_beer_lambert_limits(key):
    C.beer_lambert_limits(B, key)


@pytest.mark.parametrize("key", sorted(C.PHASES))
def test_phase_function(key):
    C.phase_function(B, key)


@pytest.mark.parametrize("key", sorted(C.REEMISSION))
def test_reemission(key):
    C.reemission(B, key)


@pytest.mark.parametrize("name", sorted(C.LIGHTS))
def test_emitter(name):
    C.device_emission(B, name)


def test_recorder_identities():
    C.recorder_identities(B)
