"""The HIP engine held to closed-form laws: the cases of tests/test_laws_referee.py (tests/law_cases.py) on the GPU,
with 1e6 photons for the laws read from event-log rows and 1e7 for those read from recorders and histograms (the LDS
tally path at scale).  Everything goes through the device-resident `Session` entry that `engine.simulate` uses: host
rays for the pencils, the device emission kernel for the emitter cases.  A 1e7-photon tally is traced as five
launches of 2e6 with consecutive ray offsets (one stream of photons) and their tallies summed, so no host array holds
more than 2e6 rays.
"""
import numpy as np
import pytest

from pvtrace_amd.engine import Session
from tests import law_cases as C

pytestmark = pytest.mark.gpu

EMIT = {0: "kT", 1: "redshift", 2: "full"}
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_sums", "rec_bins")
CHUNK = 2_000_000


class Gpu:
    n_hist = 1_000_000
    n_tally = 10_000_000

    def trace_pencil(self, scene, start, direction, wavelength, n, seed, record_every, max_events=4, maxsteps=1000,
                     emit_method=2):
        chunk = n if record_every > 0 else min(n, CHUNK)
        pos = np.tile(np.asarray(start, float), (chunk, 1))
        dirs = np.tile(np.asarray(direction, float), (chunk, 1))
        wl = np.full(chunk, float(wavelength))
        total = None
        with Session(scene, emission="host") as session:
            for offset in range(0, n, chunk):
                m = min(chunk, n - offset)
                rays = (pos[:m], dirs[:m], wl[:m], ["pencil"] * m)
                result = session.collect(session.submit(m, seed, maxsteps=maxsteps, max_events=max_events,
                                                        emit_method=EMIT[emit_method], record_every=record_every,
                                                        ray_offset=offset, host_rays=rays))
                if record_every > 0:
                    keys = ("counts", "kind", "position", "direction", "wavelength", "duration")
                    return {k: np.asarray(result.data[k]) for k in keys}, session.compiled
                part = {k: np.asarray(result.data[k]).copy() for k in TALLY_KEYS}
                total = part if total is None else {k: total[k] + part[k] for k in TALLY_KEYS}
            return total, session.compiled

    def trace_emitted(self, scene, n, seed, emit_seed, maxsteps=1000, emit_method=2):
        total = None
        with Session(scene, emission="device") as session:
            for offset in range(0, n, CHUNK):
                m = min(CHUNK, n - offset)
                result = session.collect(session.submit(m, seed, maxsteps=maxsteps, max_events=4,
                                                        emit_method=EMIT[emit_method], record_every=0,
                                                        emit_seed=emit_seed, ray_offset=offset))
                part = {k: np.asarray(result.data[k]).copy() for k in TALLY_KEYS}
                total = part if total is None else {k: total[k] + part[k] for k in TALLY_KEYS}
            return total, session.compiled

    def emit(self, scene, n, emit_seed):
        """The GENERATE rows of device-emitted rays (max_events 2: GENERATE, KILL)."""
        with Session(scene, emission="device") as session:
            result = session.collect(session.submit(n, 0, max_events=2, record_every=1, emit_seed=emit_seed))
            kind = np.asarray(result.data["kind"])[0::2]
            assert np.all(kind == C.GENERATE)
            return (np.asarray(result.data["position"])[0::2], np.asarray(result.data["direction"])[0::2],
                    np.asarray(result.data["wavelength"])[0::2])


B = Gpu()


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
def test_device_emission(name):
    C.device_emission(B, name)


def test_recorder_identities():
    C.recorder_identities(B)
