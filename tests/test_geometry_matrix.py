"""tests/geom_cases.py without a GPU: the table is complete, every case gets the plan it
states (and so the EVAL path it is there for), its inputs do their job on the oracle, and the
culling grid's per-cell certificate holds at sampled points.

The culled EVAL (transport.h eval_culled) trusts host code (cull.cpp): a query in cell c that
found min|ds| < T = max(h, lb[c]) (1 - 1e-12) over the listed and the always-evaluated tops
skips every other top, and stops its list walk at the first entry whose elb exceeds the
min|ds| it holds. A bound that is slightly too generous changes a result only where an unlisted
top would have mattered, which a few thousand photons against the oracle can miss; here the
claim itself is checked, with no tolerance: the values are the oracle's (the device's bit for
bit, tests/test_gpu_parity.py) and h and T are computed with the kernel's expressions.
"""
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, builders, scene
from rsmcrt_amd.scene import Scene, box, capsule, cylinder, invert, model, segment, sphere, torus, translate
from tests import geom_cases, planprobe
from tests.geom_cases import MEDIUM, SUBJECT, place, reflected
from tests.test_gpu_parity import SEED, _culling_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CULL_MODEL, CULL_TRANSLATE, CULL_SPHERE, CULL_CAPSULE = 1 << 31, 1 << 30, 1 << 29, 1 << 28  # cull.h
CULL_TOP_MASK = CULL_CAPSULE - 1
IDS = [c.id for c in geom_cases.CASES]

_oracle_runs = {}


def oracle(case):
    """The oracle's run of a case; cases that differ only in knobs share it, and nothing
    modifies it (tests/test_gpu_geometry.py uses the same runs)."""
    if case.oracle_key not in _oracle_runs:
        _oracle_runs[case.oracle_key] = O.run(case.scene(), case.scene_grid(), case.source(), case.n, seed=SEED,
                                              flags=case.flags, records=True)
    return _oracle_runs[case.oracle_key]


def check_inputs(case, cpu):
    """What a case needs of its inputs to test what it is there for: conditions on the oracle's
    run alone. Outside the far-march group no photon ends in a fault; the wall-hugging photons
    of that group may (tests/test_gpu_parity.py::test_far_glance_wall_photons)."""
    assert cpu.counter("photons") == case.n
    if case.group != "far":
        assert cpu.counter("faults") == 0
    assert cpu.counter("fresnel") >= case.fresnel and cpu.counter("reflections") >= case.reflections, \
        (cpu.counter("fresnel"), cpu.counter("reflections"))


def test_table_is_complete():
    assert geom_cases.check_table() == {"primitive": 40, "culled-entry": 9, "csg": 16, "modifier": 21, "pairs": 8,
                                        "far": 10}


@pytest.mark.parametrize("case", geom_cases.CASES, ids=IDS)
def test_plan_routing(case):
    """The plan fields that select the EVAL path: a changed threshold (the cooperative EVAL's 8
    tops, the table's 64, the culling grid's 16 tops and 8 boundable ones) fails here instead of
    leaving a path without its GPU case."""
    p = planprobe.plan(case.scene(), case.scene_grid(), env=case.env)
    assert p["status"] == abi.OK, p["error"]
    assert geom_cases.plan_fields(p) == case.plan


@pytest.mark.parametrize("case", geom_cases.CASES, ids=IDS)
def test_inputs_do_their_job(case):
    check_inputs(case, oracle(case))


# ---- the culling grid ----
def entries(H):
    """Per list entry: its cell, top, flags word and node word."""
    cell = np.repeat(np.arange(len(H["off"]) - 1), np.diff(H["off"].astype(np.int64)))
    return cell, (H["list"][:, 0] & CULL_TOP_MASK).astype(np.int64), H["list"][:, 0], H["list"][:, 1]


def translate_only(nd):
    return [nd.transform[k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10)] == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def check_structure(sc, H):
    """Everything about the grid that needs no SDF value: the lists' order, that no top is lost,
    and each entry's flag and node words."""
    n_top, ncell = sc.n_top, len(H["lb"])
    assert H["enabled"] and ncell == int(np.prod(H["n"])) and len(H["off"]) == ncell + 1
    assert H["off"][0] == 0 and H["off"][-1] == len(H["elb"]) == len(H["list"])
    cell, top, word, node = entries(H)
    # a cell's elb values are non-decreasing (the early stop of the list walk needs it)
    same = cell[1:] == cell[:-1]
    assert np.all(H["elb"][1:][same] >= H["elb"][:-1][same]) and np.all(H["elb"] >= 0.0)
    # every top: in `always`, or in every cell either listed or counted in lb (a cell with an
    # unlisted top has a finite lb; 1e300 stands for "none left out")
    always = set(int(t) for t in H["always"])
    listed = np.zeros((ncell, n_top), dtype=bool)
    listed[cell, top] = True
    assert len(top) == listed.sum(), "a top twice in one list"
    assert not listed[:, sorted(always)].any()
    cullable = [t for t in range(n_top) if t not in always]
    assert np.array_equal(listed[:, cullable].all(axis=1), H["lb"] == 1e300)
    assert np.all(H["lb"] >= 0.0)
    for t in cullable:
        assert listed[:, t].any(), t  # (its own box meets some cell)
    # the flags and the node word (cull.h)
    for t in range(n_top):
        nd = sc.nodes[sc.top[t]]
        w, nw = word[top == t], node[top == t]
        is_model, tr = nd.kind == abi.SDF_MODEL, translate_only(nd)
        want = (t | (CULL_MODEL if is_model else 0) | (CULL_TRANSLATE if tr and not is_model else 0) |
                (CULL_SPHERE if tr and nd.kind == abi.SDF_SPHERE else 0) |
                (CULL_CAPSULE if tr and nd.kind == abi.SDF_CAPSULE else 0))
        assert np.all(w == want), (t, hex(want))
        assert np.all(nw == (0 if is_model else sc.top[t])), t
    return listed, always


def sample_points(H, rng):
    """Every cell (at most 4000) or 3000 of them: its 8 corners and 6 face centres pulled in by
    1e-9 of the edge, and 16 uniform interior points."""
    nx, ny, nz = H["n"]
    ncell = nx * ny * nz
    cells = np.arange(ncell) if ncell <= 4000 else np.sort(rng.choice(ncell, 3000, replace=False))
    e = 1e-9
    frac = [(a, b, c) for a in (e, 1 - e) for b in (e, 1 - e) for c in (e, 1 - e)]
    for axis in range(3):
        for v in (e, 1 - e):
            f = [0.5, 0.5, 0.5]
            f[axis] = v
            frac.append(tuple(f))
    frac = np.concatenate([np.broadcast_to(np.array(frac), (len(cells), 14, 3)), rng.random((len(cells), 16, 3))], axis=1)
    idx = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], axis=1).astype(np.float64)
    clo = np.array(H["lo"]) + idx * H["cell"]  # (cull.cpp: lo + (double)ix * cs)
    return (clo[:, None, :] + frac * H["cell"]).reshape(-1, 3)


def kernel_threshold(H, pts):
    """eval_culled's cell, h and T for each point (transport.h, "const double fx = ..." and
    "every unlisted top has ds >= ..."), and which points it takes at all: the others go to a
    full EVAL."""
    lo, cell, n = np.array(H["lo"]), H["cell"], np.array(H["n"])
    inv_cell = 1.0 / cell  # (smcrt.hip upload_cull)
    f = (pts - lo) * inv_cell
    ok = np.all((f >= 0.0) & (f < n.astype(np.float64)), axis=1)
    pts, f = pts[ok], f[ok]
    i = f.astype(np.int32).astype(np.int64)
    c = i[:, 0] + n[0] * (i[:, 1] + n[1] * i[:, 2])
    corner = lo + i.astype(np.float64) * cell
    h = np.minimum(np.minimum(np.minimum(pts[:, 0] - corner[:, 0], corner[:, 0] + cell - pts[:, 0]),
                              np.minimum(pts[:, 1] - corner[:, 1], corner[:, 1] + cell - pts[:, 1])),
                   np.minimum(pts[:, 2] - corner[:, 2], corner[:, 2] + cell - pts[:, 2]))
    h = np.maximum(h, 0.0)
    T = np.maximum(h, H["lb"][c]) * (1.0 - 1e-12)
    return pts, c, T


def check_certificate(sc, g, env=None, seed=1):
    """The certificate of the culling grid of `sc`, with no tolerance. Returns the smallest slack
    ds - T of an unlisted top and the number of points."""
    H = planprobe.cull(sc, g, env)
    listed, always = check_structure(sc, H)
    pts, c, T = kernel_threshold(H, sample_points(H, np.random.default_rng(seed)))
    assert len(pts) >= 3000 * 30 * 0.9 or len(pts) >= len(H["lb"]) * 30 * 0.9
    cell, top, _, _ = entries(H)
    elb = np.zeros(listed.shape)
    elb[cell, top] = H["elb"].astype(np.float64)
    slack = np.inf
    for t in range(sc.n_top):
        if t in always:
            continue
        ds = O.sdf_eval(sc, pts, which=t)
        out = ~listed[c, t]
        # an unlisted top cannot matter to a query that passed m < T
        bad = out & ~(ds >= T)
        assert not bad.any(), (t, pts[bad][:3], ds[bad][:3], T[bad][:3])
        if out.any():
            slack = min(slack, float((ds[out] - T[out]).min()))
        # a listed entry's elb bounds its top over the whole cell (elb == 0: no claim, the box
        # meets the cell and ds may be negative)
        e = elb[c, t]
        bad = (e > 0.0) & ~(ds >= e)
        assert not bad.any(), (t, pts[bad][:3], ds[bad][:3], e[bad][:3])
    return slack, len(pts)


def tight_scene():
    """Made for tight bounds: rotated boxes, rotated tori, capped cylinders, segments, a
    reflected box, a smooth union of four children with k larger than they are, and a
    subtraction and an intersection model, in the medium box (29 tops)."""
    L = geom_cases.lattice()
    sdfs = []
    lay = lambda: len(sdfs) + 1  # noqa: E731
    for i in range(6):
        sdfs.append(box((0.2, 0.1, 0.16), SUBJECT, lay(), place(L[i], i, True)))
    for i in range(6, 12):
        sdfs.append(torus(0.09, 0.03, SUBJECT, lay(), place(L[i], i, True)))
    for i in range(12, 18):
        sdfs.append(cylinder((-0.08, -0.02, 0.0), (0.08, 0.03, 0.05), 0.04, SUBJECT, lay(), place(L[i], i, i % 2 == 1)))
    for i in range(18, 24):
        sdfs.append(segment((-0.05, 0.0, 0.0), (0.05, 0.02, 0.03), SUBJECT, lay(), place(L[i], i, i % 2 == 1)))
    sdfs.append(box((0.2, 0.1, 0.16), SUBJECT, lay(), reflected(L[24], 24)))
    c = L[25]
    t = lambda dx, dy: invert(translate((c[0] + dx, c[1] + dy, c[2])))  # noqa: E731
    sdfs.append(model([sphere(0.04, SUBJECT, lay(), t(-0.06, 0.0)), sphere(0.05, SUBJECT, lay(), t(0.06, 0.0)),
                       box((0.06, 0.06, 0.06), SUBJECT, lay(), t(0.0, 0.07)),
                       capsule((c[0], c[1] - 0.09, c[2]), (c[0] + 0.02, c[1] - 0.05, c[2]), 0.03, SUBJECT, lay())],
                      abi.OP_SMOOTH_UNION, 0.12))
    sdfs.append(geom_cases.csg(abi.OP_SUBTRACTION, 0.12, lay(), L[26], 26, True))
    sdfs.append(geom_cases.csg(abi.OP_INTERSECTION, 0.12, lay(), (0.25, 0.25, 0.25), 27, True))
    sdfs.append(box((2.0, 2.0, 2.0), MEDIUM, lay()))
    return Scene(sdfs)


def _certificate_scenes():
    g32 = scene.grid(32, 32, 32, 1, 1, 1)
    out, seen = [], set()
    for c in geom_cases.CASES:
        if c.plan["cull"] and c.scene_key not in seen:
            seen.add(c.scene_key)
            out.append(pytest.param(c.make_scene, c.scene_grid(), id=c.id))
    out.append(pytest.param(_culling_scene, g32, id="culling-scene"))
    out.append(pytest.param(lambda: builders.setup_sphere_scene(builders.random_sphere_list(40)), g32, id="40-spheres"))
    out.append(pytest.param(lambda: builders.synthetic_vessels(80), scene.grid(64, 64, 64, 0.16, 0.09, 0.13), id="vessels-80"))
    out.append(pytest.param(tight_scene, g32, id="tight"))
    return out


@pytest.mark.parametrize("make_scene,g", _certificate_scenes())
def test_cull_grid_certificate(make_scene, g):
    """cull.cpp's grid for every culled scene of the table, tests/test_gpu_parity.py's culling
    scene and 40 spheres, an 81-top capsule net and a scene made for tight bounds: at 30 points
    in each of 3000 cells (or all) every top that is neither listed nor always evaluated has
    ds >= T, every listed entry has ds >= elb, and the lists are ordered, complete and flagged
    as eval_culled reads them. The smallest slack ds - T is printed (DESIGN.md §3.3c has them)."""
    sc = make_scene()
    slack, n = check_certificate(sc, g)
    print(f"cull certificate: {sc.n_top} tops, {n} points, smallest slack {slack:.3g}")
    assert slack >= 0.0


def _walk_groups(words):
    """eval_culled's straight-line groups over one cell's list with the LDS table: 4
    translate-only spheres, else 2 translate-only capsules, until neither fits. Returns the groups
    taken and the number of entries left to the entry loop."""
    k, groups = 0, []
    while True:
        if k + 3 < len(words) and all(w & CULL_SPHERE for w in words[k:k + 4]):
            groups.append(4)
            k += 4
        elif k + 1 < len(words) and all(w & CULL_CAPSULE for w in words[k:k + 2]):
            groups.append(2)
            k += 2
        else:
            return groups, len(words) - k


def test_culled_cases_reach_their_entries():
    """The culled cases' lists hold what the cases are there for: the subjects of the
    always-evaluated cases are in the always list and those of every other case are listed (a
    model with CULL_MODEL); the all-translate scenes have cells that start with a full group;
    the mixed scene has at least 100 cells each whose lists leave 2 (the 8 nearest) and 1 and 3
    (SMCRT_CULL_K=7: the 7 nearest) entries after a group of 4 spheres, cells where a capsule pair follows or precedes other kinds, and reflected tops are bounded."""
    for case in geom_cases.CASES:
        if not case.plan["cull"] or "SMCRT_COOP_TAB" in case.env:  # (the table does not change the grid)
            continue
        sc = case.scene()
        H = planprobe.cull(sc, case.scene_grid(), case.env)
        cell, top, word, _ = entries(H)
        subj = geom_cases.subject_tops(case, sc)
        always = set(int(t) for t in H["always"])
        if case.subject[0] != "mixed":
            assert subj, case.id
        if case.always:
            assert set(subj) <= always, case.id
        else:
            assert not set(subj) & always and set(subj) <= set(top.tolist()), case.id
        if case.group == "csg":
            assert all(np.all(word[top == t] & CULL_MODEL) for t in subj), case.id
        lists = np.split(word.astype(np.int64), H["off"][1:-1].astype(np.int64))
        walks = [_walk_groups(w.tolist()) for w in lists]
        if "groups" in case.subject:
            size = 4 if case.subject[0] == abi.SDF_SPHERE else 2
            assert sum(1 for gr, _ in walks if gr and gr[0] == size) > len(walks) // 2, case.id
        if case.subject[0] == "mixed":
            left = {n: sum(1 for gr, rest in walks if 4 in gr and rest == n) for n in (1, 2, 3)}
            want = (1, 3) if case.env.get("SMCRT_CULL_K") == "7" else (2,)
            assert all(left[n] >= 100 for n in want), left  # (cells enough for the photons to meet)
            assert any(2 in gr and 4 in gr for gr, _ in walks)          # capsule pairs and sphere groups in one list
            assert any(not gr and rest >= 8 for gr, rest in walks)      # a list that starts with another kind
        if case.subject[0] == "reflection":
            assert len(subj) == 12  # (each reflected top is listed, not always evaluated: above)


def test_design_geometry_table_cites_the_cases():
    """DESIGN.md §3.3c names, for each kind, op and modifier on each EVAL path, the test id
    that runs it: every case of the table is cited there by its id, and nothing else is."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        doc = f.read()
    start = doc.index("### 3.3c")
    section = doc[start:doc.index("\n### ", start + 1)]
    missing = [c.id for c in geom_cases.CASES if f"`test_case[{c.id}]`" not in section]
    assert not missing, missing
    cited = set(re.findall(r"`test_case\[([A-Za-z0-9-]+)\]`", section))
    assert cited <= set(geom_cases.BY_ID), sorted(cited - set(geom_cases.BY_ID))
