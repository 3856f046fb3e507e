"""Cost of the convex polyhedron (`pvtrace_amd.Polyhedron`, a table of planes traced analytically by the extension kernel
variants): photons/s of the headline's dyed PMMA body (benchmarks/configs.py cfg2_lsc: its world, lamp, material and face
recorders) at 10^7 photons, tallies only, with the body as

  (a) the 5 x 5 x 1 cm `Box`, on the extension variants (a `reacted` volume map of 1 x 1 x 1: the slab has no Reactor, so
      the map counts nothing -- the way benchmarks/history_counters.py case (b) forces them);
  (b) the same slab as `Polyhedron.box`, six planes: (b)/(a) is the price of the plane loop against the slab test;
  (c) the same slab as `Mesh.box`, twelve triangles under a BVH: (b)/(c) is what the shape saves over a mesh;
  (d) a hexagonal prism of equal area and height, eight planes;
  (e) a 62-sided prism of equal area and height, 64 planes, the cap: (e)/(d) over the 56 planes between them is the cost
      of a plane.

Every case keeps ONE `Session` open -- the scene is lowered, packed and uploaded once -- and is timed launch for launch:
`launch` is the wall time of submit + collect of one launch, `kernel` the GPU's own time of that launch (`kernel_ms`).  A whole
`engine.simulate` call lowers the scene again (for a polyhedron: the plane table's analysis, cached by its bytes after the first
time) and may pack and upload it again; what that costs is reported apart, per case, as `host_ms`: `lower_first` (the first
`compile_scene`, analysis included), `lower_again` (every later one) and `simulate_call` (a whole call on a lowered-before scene,
minus its kernel time).

    python benchmarks/polyhedron.py [--photons N] [--repeats R]     # on a machine with an MI355X

Prints one JSON line: per case the median, minimum and maximum photons/s over the windows, by `launch` and by `kernel` (the
cases alternate, one warm launch each first), the kernel variant each ran, the host costs, and from the KERNEL medians the
ratios (b)/(a), (b)/(c) and (e)/(d) and the picoseconds per photon and plane that (e) against (d), and (b) against (a), imply.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pvtrace_amd import Mesh, Polyhedron, VolumeMap, engine   # noqa: E402
from pvtrace_amd.engine import Session, compile_scene   # noqa: E402
from benchmarks import configs   # noqa: E402

LOWER, UPPER = (-2.5, -2.5, -0.5), (2.5, 2.5, 0.5)
SIZE, AREA, HEIGHT = (5.0, 5.0, 1.0), 25.0, 1.0
CASES = ("a_box_extension", "b_polyhedron_box", "c_mesh_box", "d_hexagonal_prism", "e_prism_62_sides")


def circumradius(sides):
    """Of the regular polygon of `sides` corners and area AREA: A = n R^2 sin(2 pi / n) / 2."""
    return math.sqrt(2.0 * AREA / (sides * math.sin(2.0 * math.pi / sides)))


def body_scene(name):
    scene = configs.cfg2_lsc()
    body = next(n for n in scene.root.children if n.name == "LSC")
    material = body.geometry.material
    if name == "a_box_extension":
        body.volume_maps = [VolumeMap("reacted", (1, 1, 1), LOWER, UPPER, event="reacted")]
    elif name == "b_polyhedron_box":
        body.geometry = Polyhedron.box(SIZE, material=material)
    elif name == "c_mesh_box":
        body.geometry = Mesh.box(SIZE, material=material)
    elif name == "d_hexagonal_prism":
        body.geometry = Polyhedron.regular_prism(6, circumradius(6), HEIGHT, material=material)
    elif name == "e_prism_62_sides":
        body.geometry = Polyhedron.regular_prism(62, circumradius(62), HEIGHT, material=material)
    return scene


def stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of the cases")
    args = ap.parse_args()
    cases = tuple(name for name in CASES if name in args.cases.split(","))
    if not engine.is_available():
        print("HIP engine not built or no GPU visible; run: python -c 'import __graft_entry__ as g; g.build()'")
        return 1
    out = {"photons": args.photons, "windows": args.repeats}
    scenes, host = {}, {}
    for name in cases:
        scenes[name] = body_scene(name)
        tic = time.perf_counter()
        compile_scene(scenes[name])
        first = time.perf_counter() - tic
        tic = time.perf_counter()
        compile_scene(scenes[name])
        host[name] = {"lower_first": 1e3 * first, "lower_again": 1e3 * (time.perf_counter() - tic)}
    sessions = {name: Session(scene) for name, scene in scenes.items()}
    try:
        def launch(name, seed):
            s = sessions[name]
            tic = time.perf_counter()
            result = s.collect(s.submit(args.photons, seed, record_every=0, emit_seed=seed + 1))
            return time.perf_counter() - tic, 1e-3 * result.kernel_ms

        for name in sessions:
            launch(name, 1)   # load, upload, warm the clocks
        wall, kernel = {name: [] for name in sessions}, {name: [] for name in sessions}
        for r in range(args.repeats):   # alternate the cases
            for name in sessions:
                w, k = launch(name, 7 + r)
                wall[name].append(args.photons / w)
                kernel[name].append(args.photons / k)
        for name, s in sessions.items():
            out[f"{name}_photons_per_s"] = {"launch": stats(wall[name]), "kernel": stats(kernel[name]),
                                            "variant": s.dscene.launch_info()["variant"]}
    finally:
        for s in sessions.values():
            s.close()
    for name, scene in scenes.items():   # a whole call, the way a user's script pays it
        calls = []
        for r in range(3):
            tic = time.perf_counter()
            result = engine.simulate(scene, args.photons, seed=7 + r, record_every=0)
            calls.append(1e3 * (time.perf_counter() - tic) - result.kernel_ms)
        host[name]["simulate_call"] = statistics.median(calls)
    out["host_ms"] = host
    median = {name: out[f"{name}_photons_per_s"]["kernel"]["median"] for name in scenes}
    for top, bottom in (("b_polyhedron_box", "a_box_extension"), ("b_polyhedron_box", "c_mesh_box"),
                        ("e_prism_62_sides", "d_hexagonal_prism")):
        if top in scenes and bottom in scenes:
            out[f"{top}_over_{bottom}"] = median[top] / median[bottom]
    # the time of one photon is 1 / (photons/s); a photon meets the body's planes once per step, so this is per photon and
    # plane of the table, summed over the photon's steps
    if "e_prism_62_sides" in scenes and "d_hexagonal_prism" in scenes:
        out["ps_per_photon_and_plane_e_against_d"] = (1e12 / median["e_prism_62_sides"] - 1e12 / median["d_hexagonal_prism"]) / 56.0
    if "b_polyhedron_box" in scenes and "a_box_extension" in scenes:
        out["ps_per_photon_and_plane_b_against_a"] = (1e12 / median["b_polyhedron_box"] - 1e12 / median["a_box_extension"]) / 6.0
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
