"""Cost of a tabulated phase function (PhaseFunctionTable): photons/s of a scattering slab (the headline's 5 x 5 x 1 cm
slab of benchmarks/configs.py cfg2_lsc, its dye replaced by a Scatterer of 2 cm^-1, quantum yield 1, with the face
recorders) three ways -- the built-in isotropic phase function, a 2-point constant table (the same law drawn through
the table branch, other draws) and an 1801-angle x 20-wavelength Mie-like table (Henyey-Greenstein rows, g from 0.2
to 0.9 over 400-800 nm: 288 KB of CDF rows, too large for LDS, so the scene's spectra move to global memory) -- at
10^7 photons, tallies only, "fenced" (one `engine.simulate` call, timed to its return).  A short history run counts
the scatter events per photon of each scene, which turns the difference in time into a cost per scatter event.

    python benchmarks/phase_table.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: photons/s per scene, scatter events per photon, and the extra device time per scatter event
against the built-in isotropic phase function (ps of the whole GPU's throughput: 1 / rate difference / scatters).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import PhaseFunctionTable, Scatterer, isotropic   # noqa: E402
from pvtrace_amd import engine   # noqa: E402
from benchmarks import configs   # noqa: E402

SCATTER = 5


def mie_like():
    angle = np.linspace(0.0, 180.0, 1801)
    g = np.linspace(0.2, 0.9, 20)[:, None]
    mu = np.cos(np.radians(angle))[None, :]
    return PhaseFunctionTable(angle, (1.0 - g * g) / (1.0 + g * g - 2.0 * g * mu) ** 1.5,
                              wavelength=np.linspace(400.0, 800.0, 20))


def slab(phase):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    body.geometry.material.components = [Scatterer(2.0, quantum_yield=1.0, phase_function=phase, name="haze")]
    return scene


def fenced(scene, n, seed):
    tic = time.perf_counter()
    engine.simulate(scene, n, seed=seed, record_every=0)
    return time.perf_counter() - tic


def scatters_per_photon(scene, n=20000):
    r = engine.simulate(scene, n, seed=3, record_every=1, max_events=256)
    return float(np.count_nonzero(np.asarray(r.data["kind"]) == SCATTER)) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not engine.is_available():
        print("HIP engine not built or no GPU visible; run: python -c 'import __graft_entry__ as g; g.build()'")
        return 1
    scenes = {"isotropic": slab(isotropic), "constant_table": slab(PhaseFunctionTable([0.0, 180.0], [1.0, 1.0])),
              "mie_1801x20": slab(mie_like())}
    for scene in scenes.values():
        engine.simulate(scene, 100000, seed=1, record_every=0)   # load, upload, warm
    best = {name: float("inf") for name in scenes}
    for r in range(args.repeats):   # alternate the scenes, keep each one's best
        for name, scene in scenes.items():
            best[name] = min(best[name], fenced(scene, args.photons, 7 + r))
    out = {"photons": args.photons}
    for name in scenes:
        out[f"fenced_{name}_photons_per_s"] = args.photons / best[name]
    events = {name: scatters_per_photon(scene) for name, scene in scenes.items()}
    for name in scenes:
        out[f"{name}_scatters_per_photon"] = events[name]
    base = best["isotropic"] / args.photons
    for name in ("constant_table", "mie_1801x20"):
        out[f"ratio_{name}_over_isotropic"] = best["isotropic"] / best[name]
        # (the constant table follows the isotropic law: the same number of scatters, so the difference is the
        # table's own cost; the Mie-like table scatters forward and its photons take other paths)
        out[f"{name}_extra_ps_per_scatter"] = (best[name] / args.photons - base) / events[name] * 1e12
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
