"""Helpers of the ray-capture tests (tests/test_gpu_ray_capture.py): finding a node, launching host rays on a `Session`,
the launch that keeps every ray's history beside the same rays tallied only, and the rough, fielded, mapped block."""
import numpy as np

from pvtrace_amd import (
    Box, ConcentrationGrid, FresnelSurfaceDelegate, Luminophore, Material, Node, Scene, Surface, VolumeMap,
)
from pvtrace_amd.engine import Session
from pvtrace_amd.engine.emit import emit_bundle
from tests import laws as L


def node(scene, name):
    return next(n for n in scene.root.preorder() if n.name == name)


def submit(session, rays, seed, **kw):
    pos, dirs, wl = rays
    return session.collect(session.submit(len(wl), seed, host_rays=(pos, dirs, wl, ["r"] * len(wl)), **kw))


def history_launch(scene, rays, n=8192, seed=7, max_events=512):
    """ONE launch that keeps every ray's history -> (result, the same rays and seed tallied only).  `rays`: host rays
    (position, direction, wavelength), None (the scene's lights, sampled on the host) or "device" (device emission)."""
    if isinstance(rays, str):
        with Session(scene, emission="device") as s:
            hist = s.collect(s.submit(n, seed, record_every=1, max_events=max_events, emit_seed=31))
            tally = s.collect(s.submit(n, seed, record_every=0, emit_seed=31))
    else:
        if rays is None:
            pos, dirs, wl, _ = emit_bundle(scene, n, seed=3)
            rays = (pos, dirs, wl)
        with Session(scene, emission="host") as s:
            hist = submit(s, rays, seed, record_every=1, max_events=max_events)
            tally = submit(s, rays, seed, record_every=0)
    # no history was cut: neither by max_events nor by maxsteps
    assert int(np.asarray(hist.data["counts"]).max()) < max_events
    return hist, tally


def rough_fielded_block(n=8192):
    """A rotated glass block with a rough Fresnel surface, a luminophore on a 3 x 2 x 4 concentration field and three volume
    maps on the field's lattice, under a pencil beam -> (scene, rays)."""
    ix, iy, iz = np.indices((3, 2, 4))
    grid = ConcentrationGrid(0.2 + ((ix + 2 * iy + iz) % 3), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    x = np.linspace(400.0, 800.0, 41)
    lum = Luminophore(np.column_stack([x, 1.5 * np.exp(-((x - 520.0) / 80.0) ** 2)]),
                      emission=np.column_stack([x, np.exp(-((x - 560.0) / 50.0) ** 2)]), quantum_yield=0.95,
                      concentration=grid, name="lum")
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    body = Node(name="block", parent=world, geometry=Box((2.0, 2.0, 2.0), material=Material(
        refractive_index=1.5, surface=Surface(FresnelSurfaceDelegate(roughness=0.3)), components=[lum])))
    body.rotate(0.5, (1.0, 1.0, 0.0))
    body.volume_maps = [VolumeMap.like(grid, "dose", wavelength=(400.0, 800.0, 8)),
                        VolumeMap.like(grid, "glow", event="emitted"), VolumeMap.like(grid, "heat", event="lost")]
    R = L.rotation(0.5, (1.0, 1.0, 0.0))
    start, direction = R @ np.array([0.2, -0.1, -4.0]), R @ np.array([0.0, 0.0, 1.0])
    return Scene(world), (np.tile(start, (n, 1)), np.tile(direction, (n, 1)), np.full(n, 480.0))
