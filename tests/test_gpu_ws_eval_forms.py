"""The two forms of the photon waves' EVAL in ws_kernel (ws.h WsTraits, transport.h eval_sdfs PAIRS).

The plain instantiation of a power-of-two grid (grid mode 2) takes consecutive top-level spheres
and boxes two at a time; every other instantiation (another grid mode, the XF one) takes the tops
one by one. Both perform the same operations, so every case is the oracle's as
tests/test_gpu_parity.py compares them: counters, photon records, absorb and emission bit for
bit, jmean at rtol 1e-12. The top lists cover each order of a pair, a leftover after a pair, and
a top that cannot pair between two that can. 4,000 photons each; lean_launches > 0 shows that
ws_kernel ran.

SMCRT_DEBUG_EVAL_LOOP=1 (tests only) makes a pair-form kernel take the tops one by one; its
outputs are those of the pair form bit for bit, jmean included up to the order of its sums.
"""
import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, builders, scene
from rsmcrt_amd.engine import Engine
from rsmcrt_amd.scene import Scene, box, cylinder, mono, sphere, torus
from tests.test_gpu_parity import SEED, compare

pytestmark = pytest.mark.gpu

N = 4000
_SCAT = mono(10.0, 0.1, 0.9, 1.0)   # M1's medium
_SCAT2 = mono(4.0, 0.5, 0.5, 1.0)
_CLEAR = mono(0.0, 0.0, 0.0, 1.0)

LISTS = {
    "sphere+box": lambda: builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 1.0),  # M1's
    "box+sphere": lambda: Scene([box((1.0, 1.0, 1.0), _SCAT, 1), sphere(2.0, _CLEAR, 2)]),
    "sphere+sphere": lambda: Scene([sphere(0.6, _SCAT, 1), sphere(2.0, _CLEAR, 2)]),
    "box+box": lambda: builders.setup_box(10.0, 0.1, 0.9, 1.0, (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)),
    "one-top": lambda: Scene([box((2.0, 2.0, 2.0), _SCAT2, 1)]),
    # a pair and a leftover
    "three-tops": lambda: Scene([sphere(0.5, _SCAT, 1), box((1.4, 1.4, 1.4), _SCAT2, 2), box((2.0, 2.0, 2.0), _CLEAR, 3)]),
    # a top that cannot pair between two that can
    "torus-between": lambda: Scene([sphere(0.4, _SCAT, 1), torus(0.7, 0.15, _SCAT2, 2), box((2.0, 2.0, 2.0), _CLEAR, 3)]),
    "cylinder-between": lambda: Scene([box((0.6, 0.6, 0.6), _SCAT, 1),
                                       cylinder((0.0, 0.0, -0.8), (0.0, 0.0, 0.8), 0.7, _SCAT2, 2),
                                       box((2.0, 2.0, 2.0), _CLEAR, 3)]),
}
_ORACLE = {}


def _oracle(name, sc, g, flags=abi.FLAG_PATHLENGTH):
    if name not in _ORACLE:
        _ORACLE[name] = O.run(sc, g, scene.point_source(), N, seed=SEED, flags=flags, records=True)
    return _ORACLE[name]


def _run(sc, g, flags=abi.FLAG_PATHLENGTH):
    with Engine(sc, g) as eng:
        eng.kernel_times()
        res = eng.run(scene.point_source(), N, seed=SEED, flags=flags, records=True)
        eng.check()
        kt = eng.kernel_times()
    assert kt["lean_launches"] > 0 and kt["lean_hazards"] == 0, kt
    return res


@pytest.mark.parametrize("tops", list(LISTS))
def test_pair_form_top_lists(tops):
    """32^3 over a 2^3 box: grid mode 2, the plain instantiation, the pair form."""
    sc, g = LISTS[tops](), scene.grid(32, 32, 32, 1, 1, 1)
    cpu = _oracle(tops, sc, g)
    compare(_run(sc, g), cpu)
    assert cpu.counter("sdf_evals") > 0 and cpu.counter("grid_updates") > N
    assert cpu.counter("faults") == 0


def test_loop_form_other_grid_mode():
    """The sphere + box list on 24^3: the spacing is no power of two, so the loop form runs."""
    sc, g = LISTS["sphere+box"](), scene.grid(24, 24, 24, 1, 1, 1)
    compare(_run(sc, g), _oracle("sphere+box@24", sc, g))


def test_loop_form_fresnel_sphere():
    """An n = 1.33 sphere at 32^3: the XF instantiation (Fresnel events), the loop form."""
    sc, g = builders.setup_sphere(10.0, 0.1, 0.9, 1.33, 1.0), scene.grid(32, 32, 32, 1, 1, 1)
    cpu = _oracle("fresnel", sc, g)
    compare(_run(sc, g), cpu)
    assert cpu.counter("fresnel") > 0


def test_forced_loop_gives_the_pair_forms_outputs(monkeypatch):
    """32^3 sphere + box with SMCRT_DEBUG_EVAL_LOOP=1: the same kernel, no pairs taken."""
    sc, g = LISTS["sphere+box"](), scene.grid(32, 32, 32, 1, 1, 1)
    pairs = _run(sc, g)
    monkeypatch.setenv("SMCRT_DEBUG_EVAL_LOOP", "1")
    loop = _run(sc, g)
    compare(loop, pairs)
    compare(loop, _oracle("sphere+box", sc, g))
    for f in pairs.records.dtype.names:
        assert np.array_equal(loop.records[f], pairs.records[f]), f
