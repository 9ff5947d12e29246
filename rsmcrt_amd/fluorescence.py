"""Two-step fluorescence (Raman, autofluorescence) on one resident scene: an excitation run whose
absorb tally, weighted by a yield per layer, becomes the volume source of an emission run.

The reference's route to this is the approximation of its tools/CalcRamanDectEff.py: the absorb
grid times an escape function launched from voxel centres. Here the emission photons start inside
the voxels, in proportion to what was absorbed there (scene.volume_source,
Engine.set_volume_source), and are transported like any others. A convenience over the public
calls of Engine; no native code of its own."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import abi
from .scene import volume_source

Fluorescence = namedtuple("Fluorescence", "excitation emission weights per_excitation_photon")


def voxel_centres(grid) -> np.ndarray:
    """The centres of the grid's voxels, (nx * ny * nz, 3), x fastest as the tallies are."""
    cx, cy, cz = [(np.arange(n) + 0.5) * (2.0 * m / n) - m
                  for n, m in ((grid.nx, grid.xmax), (grid.ny, grid.ymax), (grid.nz, grid.zmax))]
    return np.stack(np.meshgrid(cz, cy, cx, indexing="ij")[::-1], axis=-1).reshape(-1, 3)


def emission_weights(absorb, layers, yield_by_layer) -> np.ndarray:
    """w = absorb * yield_by_layer[layer], voxel by voxel. `layers` holds the layer of each voxel
    centre as Engine.classify gives it (1-based; 0: in no SDF, which yields nothing);
    `yield_by_layer` is a mapping {layer: yield} (absent layers yield 0) or a sequence indexed by
    layer - 1. Returns an array of absorb's shape."""
    a = np.asarray(absorb, dtype=np.float64)
    lay = np.asarray(layers).reshape(-1)
    if lay.size != a.size:
        raise ValueError(f"{lay.size} layers for {a.size} voxels")
    n = int(lay.max()) if lay.size else 0
    table = np.zeros(n + 1)
    if hasattr(yield_by_layer, "items"):
        for k, v in yield_by_layer.items():
            if 1 <= int(k) <= n:
                table[int(k)] = float(v)
    else:
        y = [float(v) for v in yield_by_layer]
        table[1:1 + min(n, len(y))] = y[:n]
    if np.any(table < 0.0) or not np.all(np.isfinite(table)):
        raise ValueError("yields must be finite and >= 0")
    return (a.reshape(-1) * table[lay]).reshape(a.shape)


def fluorescence(engine, source, n_ex, n_em, yield_by_layer, emission_props=None, seed=123456789,
                 flags=abi.FLAG_PATHLENGTH, spectrum=None) -> Fluorescence:
    """Run `n_ex` excitation photons from `source`, then `n_em` emission photons from the volume
    source w = absorb * yield_by_layer[layer of the voxel centre] (emission_weights).

    `emission_props`, {top_index: (mus, mua, hgg, n)}, are the optical properties at the emission
    wavelength: they are applied with set_optprops for the emission run, and the excitation values
    (get_optprops) are put back afterwards, also when the run raises. The emission run uses the
    seed `seed + 1`; `spectrum` is the emission source's (scene.volume_source).

    Returns (excitation Result, emission Result, w of shape (nz, ny, nx), per_excitation_photon):
    emission tallies times per_excitation_photon = sum(w) / (n_ex * n_em) are per excitation
    photon, absorb being the absorbed weight of all n_ex photons. The scene keeps the table."""
    ex = engine.run(source, int(n_ex), seed=seed, flags=flags)
    layers, _ = engine.classify(voxel_centres(engine.grid))
    w = emission_weights(ex.absorb, layers, yield_by_layer)
    engine.set_volume_source(w)
    saved = {}
    try:
        for top, props in (emission_props or {}).items():
            saved[int(top)] = engine.get_optprops(int(top))[1:]
            engine.set_optprops(int(top), *[float(v) for v in props])
        em = engine.run(volume_source(spectrum), int(n_em), seed=seed + 1, flags=flags)
    finally:
        for top, props in saved.items():
            engine.set_optprops(top, *props)
    return Fluorescence(ex, em, w, float(w.sum()) / (float(n_ex) * float(n_em)))
