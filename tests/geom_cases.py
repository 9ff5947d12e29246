"""The cases that drive every SDF kind, CSG op and modifier through every path that evaluates
the SDF array: plain data and helpers shared by tests/test_geometry_matrix.py (the plan each case
must get, what its inputs must do on the oracle, and the culling grid's certificate, all
without a GPU) and tests/test_gpu_geometry.py (the run against the oracle).

Five device paths evaluate the SDF array:
  lean    ws_kernel's serial fold, eval_sdfs without PAIRS (ws.h)
  serial  transport_kernel's serial fold, eval_sdfs<.., PAIRS> (SMCRT_LEAN=0; NEST for modifiers)
  table   the cooperative EVAL from the LDS table, 8 to 64 primitive tops (sdf_prim_s<64>)
  global  the cooperative EVAL from device memory (a model or modifier among the tops)
  culled  eval_culled / eval_culled_coop over the culling grid's lists (16 tops or more)
plan_scene picks one from the number and the kinds of the tops; a case states the plan fields it
must get. `check_table` asserts that every SDF_* kind and OP_* of rsmcrt_amd/abi.py is the
subject of a case on each path listed for it, so a kind added to the ABI without a case fails a
CPU test.

Every scene: a 32^3 grid of half-extent 1, subject tops with (mus, mua, g, n) = (10, 0.3, 0.6,
1.4) in a 2x2x2 medium box with (1, 0.02, 0.3, 1.0), so every subject surface is a Fresnel
interface (calcNormal's taps and the capture EVALs run), and a uniform source that shoots down
from z = 0.999 over the whole top face. Copies sit on a jittered 3x3x3 lattice of pitch 0.5;
every second copy gets a rigid rotation, the others a pure translation.
"""
from dataclasses import dataclass, field
from functools import lru_cache, partial

import numpy as np

from rsmcrt_amd import abi, scene
from rsmcrt_amd.scene import (Scene, bend, box, capsule, cone, cylinder, displacement_sine, egg, elongate, extrude,
                              invert, model, mono, onion, plane, revolution, rotate_x, rotate_z, segment, sphere, torus,
                              translate, triprism, twist)

GRID = (32, 32, 32, 1.0)
SUBJECT = mono(10.0, 0.3, 0.6, 1.4)
MEDIUM = mono(1.0, 0.02, 0.3, 1.0)
PLAN_FIELDS = ("lean_candidate", "coop", "ctab", "cull", "nested", "fm")
PATHS = ("lean", "serial", "table", "global", "culled")
SIZE_ONE, SIZE_MANY = 0.3, 0.12  # a lone copy; a copy on the lattice

PRIMITIVES = {abi.SDF_SPHERE: "sphere", abi.SDF_BOX: "box", abi.SDF_TORUS: "torus", abi.SDF_CYLINDER: "cylinder",
              abi.SDF_TRIPRISM: "triprism", abi.SDF_SEGMENT: "segment", abi.SDF_CAPSULE: "capsule",
              abi.SDF_CONE: "cone", abi.SDF_EGG: "egg", abi.SDF_PLANE: "plane"}
CULLABLE = (abi.SDF_SPHERE, abi.SDF_BOX, abi.SDF_TORUS, abi.SDF_CYLINDER, abi.SDF_SEGMENT, abi.SDF_CAPSULE)  # cull.cpp prim_bound
OPS = {abi.OP_UNION: "union", abi.OP_SMOOTH_UNION: "smooth", abi.OP_SUBTRACTION: "subtraction",
       abi.OP_INTERSECTION: "intersection"}
MODIFIERS = {abi.SDF_REVOLUTION: "revolution", abi.SDF_EXTRUDE: "extrude", abi.SDF_ONION: "onion",
             abi.SDF_TWIST: "twist", abi.SDF_BEND: "bend", abi.SDF_ELONGATE: "elongate",
             abi.SDF_DISPLACEMENT: "displacement"}


# ---- placement ----
def _mm(a, b):
    return (np.array(a) @ np.array(b)).tolist()


@lru_cache(maxsize=None)
def lattice():
    """27 centres: a 3x3x3 lattice of pitch 0.5 jittered by up to 0.04 per axis, in a fixed
    shuffled order (the first n are the centres of an n-copy scene)."""
    rng = np.random.Generator(np.random.Philox(20250607))
    pts = [(0.5 * i, 0.5 * j, 0.5 * k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    order = rng.permutation(len(pts))
    return tuple(tuple(float(pts[o][a] + rng.uniform(-0.04, 0.04)) for a in range(3)) for o in order)


def place(c, i, rigid):
    """The transform of copy i at centre c: a pure translation, or a rotation about z and x first."""
    if not rigid:
        return invert(translate(c))
    return invert(_mm(_mm(rotate_z(17.0 + 23.0 * i), rotate_x(31.0 + 11.0 * i)), translate(c)))


REFLECT_X = [[-1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]]


def reflected(c, i):
    """A reflection (det = -1, which cull.cpp prim_bound accepts as rigid) and a rotation."""
    return invert(_mm(_mm(REFLECT_X, rotate_z(29.0 + 13.0 * i)), translate(c)))


# ---- subjects: kind, size s, layer, transform -> an SDF centred on its local origin ----
def prim(kind, s, layer, t, opt=SUBJECT):
    if kind == abi.SDF_SPHERE:
        return sphere(s, opt, layer, t)
    if kind == abi.SDF_BOX:
        return box((1.6 * s, 1.2 * s, 2.0 * s), opt, layer, t)
    if kind == abi.SDF_TORUS:
        return torus(0.8 * s, 0.3 * s, opt, layer, t)
    if kind == abi.SDF_CYLINDER:
        return cylinder((-0.7 * s, -0.2 * s, 0.0), (0.7 * s, 0.3 * s, 0.2 * s), 0.6 * s, opt, layer, t)
    if kind == abi.SDF_TRIPRISM:
        return triprism(1.2 * s, 0.8 * s, opt, layer, t)
    if kind == abi.SDF_SEGMENT:  # (its radius is the formula's literal 0.1)
        return segment((-0.5 * s, 0.0, -0.1 * s), (0.5 * s, 0.2 * s, 0.1 * s), opt, layer, t)
    if kind == abi.SDF_CAPSULE:
        return capsule((-0.6 * s, -0.1 * s, 0.0), (0.6 * s, 0.3 * s, 0.2 * s), 0.6 * s, opt, layer, t)
    if kind == abi.SDF_CONE:
        return cone((0.0, 0.0, -0.8 * s), (0.1 * s, 0.0, 0.8 * s), 0.7 * s, 0.3 * s, opt, layer, t)
    if kind == abi.SDF_EGG:  # (the proportions of setup_egg: 2, 1.5, 1.4)
        return egg(s, 0.75 * s, 0.7 * s, opt, layer, t)
    raise ValueError(kind)


def the_plane(c, layer):
    """z < -0.7 or so: the half-space below a horizontal plane, by translation."""
    return plane((0.0, 0.0, 1.0), SUBJECT, layer, invert(translate((c[0], c[1], -0.7 + 0.1 * c[2]))))


def csg(op, s, layer, c, i, rigid):
    """Three children of mixed kinds around c, so that the left fold's order matters for
    subtraction and smooth union. Smooth union: k is larger than the children. Subtraction
    (max(-max(-a, b), c)): the first operand is the largest; the result is the last child
    without what the second cuts out of the first's complement. Intersection: all three overlap."""
    t = lambda dx, j: place((c[0] + dx * s, c[1], c[2]), i + j, rigid)  # noqa: E731
    if op == abi.OP_SUBTRACTION:
        kids = [sphere(1.1 * s, SUBJECT, layer, t(0.0, 0)), box((1.2 * s, 1.2 * s, 1.2 * s), SUBJECT, layer, t(0.5, 1)),
                capsule((-0.9 * s, -0.2 * s, 0.0), (0.9 * s, 0.3 * s, 0.1 * s), 0.5 * s, SUBJECT, layer, t(0.2, 2))]
    elif op == abi.OP_INTERSECTION:
        kids = [sphere(1.0 * s, SUBJECT, layer, t(0.0, 0)), box((1.4 * s, 1.8 * s, 1.2 * s), SUBJECT, layer, t(0.3, 1)),
                capsule((-0.9 * s, -0.2 * s, 0.0), (0.9 * s, 0.3 * s, 0.1 * s), 0.6 * s, SUBJECT, layer, t(0.1, 2))]
    else:
        kids = [sphere(0.6 * s, SUBJECT, layer, t(-0.6, 0)), box((0.8 * s, 1.0 * s, 0.6 * s), SUBJECT, layer, t(0.5, 1)),
                capsule((-0.2 * s, -0.6 * s, 0.0), (0.3 * s, 0.7 * s, 0.2 * s), 0.3 * s, SUBJECT, layer, t(0.0, 2))]
    return model(kids, op, 1.5 * s if op == abi.OP_SMOOTH_UNION else 0.0)


def modifier(kind, s, layer, c, i, rigid):
    """The modifier around a box or a capsule (neither has a symmetry the modifier could hide).
    Modifiers have no transform of their own: revolution takes its centre as a parameter;
    extrude clips to |z| < h and elongate mirrors about the scene's origin; twist and bend turn
    the point about the z axis before the child sees it."""
    t = place(c, i, rigid)
    bx = box((1.6 * s, 1.2 * s, 2.0 * s), SUBJECT, layer, t)
    cp = capsule((-0.6 * s, -0.1 * s, 0.0), (0.6 * s, 0.3 * s, 0.2 * s), 0.6 * s, SUBJECT, layer, t)
    if kind == abi.SDF_REVOLUTION:  # (the profile in the modifier's own plane: no transform)
        return revolution(capsule((-0.3 * s, -0.2 * s, 0.0), (0.4 * s, 0.5 * s, 0.0), 0.3 * s, SUBJECT, layer), 0.5 * s, center=c)
    if kind == abi.SDF_EXTRUDE:
        return extrude(bx, 0.55)
    if kind == abi.SDF_ONION:
        return onion(bx, 0.15 * s)
    if kind == abi.SDF_TWIST:
        return twist(bx, 0.8)
    if kind == abi.SDF_BEND:
        return bend(cp, 0.6)
    if kind == abi.SDF_ELONGATE:
        return elongate(cp, (0.3 * s, 0.0, 0.2 * s))
    if kind == abi.SDF_DISPLACEMENT:
        return displacement_sine(bx, 0.1 * s, (9.0, 7.0, 5.0))
    raise ValueError(kind)


def medium(layer):
    return box((2.0, 2.0, 2.0), MEDIUM, layer)


def _filler(n):
    """n spheres on the lattice, alternately translated and rotated: the boundable tops that
    switch the culled EVAL on for subjects it always evaluates."""
    return [sphere(0.1, SUBJECT, i + 1, place(lattice()[i], i, i % 2 == 1)) for i in range(n)]


# ---- scenes (each a function of plain arguments, so that a case names it by a key) ----
def prim_scene(kind, copies, all_translate=False, transform="rigid"):
    """`copies` of a primitive kind plus the medium box. The plane: one plane and copies - 1
    spheres (stacked half-spaces reflect the photons between them without end)."""
    s = SIZE_ONE if copies == 1 else SIZE_MANY
    sdfs = []
    for i in range(copies):
        c = lattice()[i] if copies > 1 else (0.1, -0.05, 0.2)
        rigid = (i % 2 == 1) and not all_translate
        if kind == abi.SDF_PLANE:
            sdfs.append(the_plane(c, i + 1) if i == 0 else sphere(0.1, SUBJECT, i + 1, place(c, i, rigid)))
        elif transform == "reflect" and i % 2 == 1:
            sdfs.append(prim(kind, s, i + 1, reflected(c, i)))
        else:
            sdfs.append(prim(kind, s, i + 1, place(c, i, rigid)))
    sdfs.append(medium(len(sdfs) + 1))
    return Scene(sdfs)


def always_scene(kind):
    """24 spheres, then 3 copies of a kind the culling grid cannot bound (1 for the plane)."""
    sdfs = _filler(24)
    for i in range(24, 25 if kind == abi.SDF_PLANE else 27):
        c = lattice()[i]
        sdfs.append(the_plane(c, i + 1) if kind == abi.SDF_PLANE else prim(kind, SIZE_MANY, i + 1, place(c, i, i % 2 == 1)))
    sdfs.append(medium(len(sdfs) + 1))
    return Scene(sdfs)


def scaled_scene():
    """24 spheres and one more under a uniform scale of 2 (not rigid: always evaluated)."""
    sdfs = _filler(24)
    c = lattice()[24]
    sdfs.append(sphere(0.25, SUBJECT, 25, transform=[[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 2.0, 0],
                                                      [-2.0 * c[0], -2.0 * c[1], -2.0 * c[2], 1.0]]))
    sdfs.append(medium(26))
    return Scene(sdfs)


def mixed_scene():
    """Translate-only spheres (towards -x) and capsules (towards +x), the culled EVAL's
    straight-line groups, among rotated boxes, tori and cylinders, so that the cell lists
    interleave them: lists of the 8 nearest leave 2 entries after a group of 4 spheres and a
    capsule pair, and 4 after the group alone; of the 7 nearest (SMCRT_CULL_K=7) 1 and 3."""
    rng = np.random.Generator(np.random.Philox(77))
    kinds = [abi.SDF_SPHERE] * 14 + [abi.SDF_CAPSULE] * 8 + [abi.SDF_BOX, abi.SDF_TORUS, abi.SDF_CYLINDER] * 2
    sdfs = []
    for i, kind in enumerate(kinds):
        c = [float(v) for v in rng.uniform(-0.75, 0.75, 3)]
        if kind == abi.SDF_SPHERE:
            c[0] = float(rng.uniform(-0.75, 0.15))
        if kind == abi.SDF_CAPSULE:
            c[0] = float(rng.uniform(-0.05, 0.75))
        sdfs.append(prim(kind, 0.07, i + 1, place(tuple(c), i, kind not in (abi.SDF_SPHERE, abi.SDF_CAPSULE))))
    sdfs.append(medium(len(sdfs) + 1))
    return Scene(sdfs)


def csg_scene(op, copies):
    s = SIZE_ONE if copies == 1 else SIZE_MANY
    sdfs = [csg(op, s, i + 1, lattice()[i] if copies > 1 else (0.1, -0.05, 0.2), i, i % 2 == 1) for i in range(copies)]
    sdfs.append(medium(len(sdfs) + 1))
    return Scene(sdfs)


def modifier_scene(kind, copies):
    """1 or 12 copies and the medium box, or (copies == 3) 24 spheres first: a modifier has no
    bound, so the culled EVAL needs them."""
    s = SIZE_ONE if copies == 1 else SIZE_MANY
    sdfs = _filler(24) if copies == 3 else []
    first = len(sdfs)
    for i in range(first, first + copies):
        c = lattice()[i] if copies > 1 else (0.1, -0.05, 0.2)
        sdfs.append(modifier(kind, s, i + 1, c, i, i % 2 == 1))
    sdfs.append(medium(len(sdfs) + 1))
    return Scene(sdfs)


PAIR_SCENES = {
    # tokens: s/b sphere/box, T/R translated/rotated, M the medium box (a translate-only box),
    # model (a union of three), cyl; eval_sdfs pairs tops greedily from the first (pairs_of)
    "sb": ("sT", "bT", "sT", "bR", "sR", "M"),
    "sb-bb": ("sR", "bR", "bT", "bT", "bT", "bR", "M"),
    "bb-bs": ("bR", "bT", "bR", "bR", "bT", "sT", "M"),
    "bs": ("bT", "sR", "bR", "sT", "bR", "sR", "M"),
    "ss": ("sT", "sT", "sT", "sR", "sR", "sT", "M"),
    "odd": ("M", "sR", "sR", "sR", "sT"),
    "model": ("sT", "bR", "model", "bR", "sT", "M"),
    "cyl": ("sT", "cyl", "bR", "M"),
}


def pair_scene(name):
    sdfs = []
    for i, tok in enumerate(PAIR_SCENES[name]):
        c, lay = lattice()[i], i + 1
        if tok == "M":
            sdfs.append(medium(lay))
        elif tok == "model":
            sdfs.append(csg(abi.OP_UNION, 0.2, lay, c, i, False))
        elif tok == "cyl":
            sdfs.append(prim(abi.SDF_CYLINDER, 0.2, lay, place(c, i, True)))
        else:
            sdfs.append(prim(abi.SDF_SPHERE if tok[0] == "s" else abi.SDF_BOX, 0.2, lay, place(c, i, tok[1] == "R")))
    return Scene(sdfs)


def pairs_of(sc):
    """eval_sdfs<.., PAIRS>'s greedy pairing (transport.h) restated on a scene: the list of
    (kind, kind, translate_only, translate_only) it evaluates as pairs, and the tops it leaves."""
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    tops = [sc.nodes[i] for i in sc.top]
    tr = [[nd.transform[k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10)] == ident for nd in tops]
    pairs, single, i = [], [], 0
    while i < len(tops):
        a = tops[i]
        if (i + 1 < len(tops) and a.kind in (abi.SDF_SPHERE, abi.SDF_BOX)
                and tops[i + 1].kind in (abi.SDF_SPHERE, abi.SDF_BOX)):
            pairs.append((a.kind, tops[i + 1].kind, tr[i], tr[i + 1], i))
            i += 2
        else:
            single.append((a.kind, i))
            i += 1
    return pairs, single


def far_scene(kind):
    """12 translate-only far tops and the medium box: the wall photons' near top is the box."""
    sdfs = [prim(kind, SIZE_MANY, i + 1, place(lattice()[i], i, False)) for i in range(12)]
    sdfs.append(medium(13))
    return Scene(sdfs)


def far_sphere_scene():
    """No box at all: 12 small translate-only spheres inside a medium sphere of radius 0.95, so
    that the near top of a photon that skims the medium's surface is a sphere
    (far_march<GM, SMCRT_SDF_SPHERE>)."""
    sdfs = [sphere(0.08, SUBJECT, i + 1, place(tuple(0.8 * v for v in lattice()[i]), i, False)) for i in range(12)]
    sdfs.append(sphere(0.95, MEDIUM, 13))
    return Scene(sdfs)


# ---- sources ----
def face_source():
    return scene.uniform_source((-1.0, -1.0, 0.999), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, -1.0))


def wall_source():
    """Within 1e-2 of the x = -1 wall, straight down it (test_far_field_march's, 10 x farther)."""
    return scene.uniform_source((-1.0, -1.0, 0.9999999), (1e-2, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, -1.0))


def skim_source():
    """1e-3 inside the medium sphere's surface at its top, moving tangentially."""
    return scene.uniform_source((-1e-3, -1e-3, 0.949), (2e-3, 0.0, 0.0), (0.0, 2e-3, 0.0), (1.0, 0.0, 0.0))


# ---- the table ----
@dataclass(frozen=True)
class Case:
    id: str
    group: str        # "primitive", "culled-entry", "csg", "modifier", "pairs" or "far"
    path: str         # one of PATHS
    subject: tuple    # the SDF_* kinds, ("op", OP_*) or tags the case is there for
    make_scene: object
    scene_key: tuple  # names the scene: cases with the same key, source and n share an oracle run
    n: int
    plan: dict        # the PLAN_FIELDS the probe must report
    lean: bool        # the run launches ws_kernel
    env: dict = field(default_factory=dict)
    make_source: object = face_source
    fresnel: int = 200        # the oracle's run has at least this many Fresnel events ...
    reflections: int = 50     # ... and reflections
    far: str = ""             # far group: "on" (far_steps > 0) or "off" (SMCRT_FAR_MARCH=0: far_steps == 0)
    always: bool = False      # culled: the subject tops are in the grid's always list
    flags: int = abi.FLAG_PATHLENGTH

    def scene(self):
        return self.make_scene()

    def source(self):
        return self.make_source()

    def scene_grid(self):
        nx, ny, nz, ext = GRID
        return scene.grid(nx, ny, nz, ext, ext, ext)

    @property
    def oracle_key(self):
        return (self.scene_key, self.make_source.__name__, self.n, self.flags)


def _plan(lean_candidate, coop, ctab, cull, nested=0, fm=0):
    return dict(zip(PLAN_FIELDS, (lean_candidate, coop, ctab, cull, nested, fm)))


ONE = dict(n=4000, fresnel=50, reflections=10)  # a lone subject
MANY = dict(n=1500, fresnel=200, reflections=50)
NO_LEAN = {"SMCRT_LEAN": "0"}


def _primitives():
    out = []
    for kind, name in PRIMITIVES.items():
        one = partial(prim_scene, kind, 1)
        out.append(Case(f"{name}-lean", "primitive", "lean", (kind,), one, ("prim", kind, 1), plan=_plan(1, 0, 0, 0),
                        lean=True, **ONE))
        out.append(Case(f"{name}-serial", "primitive", "serial", (kind,), one, ("prim", kind, 1), plan=_plan(0, 0, 0, 0),
                        lean=False, env=NO_LEAN, **ONE))
        # (rotated copies: no far-field march, fm_err == 0)
        out.append(Case(f"{name}-table", "primitive", "table", (kind,), partial(prim_scene, kind, 12), ("prim", kind, 12),
                        plan=_plan(0, 1, 1, 0), lean=False, **MANY))
        if kind in CULLABLE:
            out.append(Case(f"{name}-culled", "primitive", "culled", (kind,), partial(prim_scene, kind, 24),
                            ("prim", kind, 24), plan=_plan(0, 1, 1, 1), lean=False, **MANY))
        else:
            out.append(Case(f"{name}-culled", "primitive", "culled", (kind,), partial(always_scene, kind),
                            ("always", kind), plan=_plan(0, 1, 1, 1), lean=False, always=True, **MANY))
    return out


def _culled_entries():
    out = []
    for kind in (abi.SDF_SPHERE, abi.SDF_CAPSULE):
        name = PRIMITIVES[kind]
        # every copy translate-only: the groups of 4 spheres / 2 capsules, from the LDS table
        # and (SMCRT_COOP_TAB=0) from the nodes; such scenes get the far-field march too
        for tab in (1, 0):
            out.append(Case(f"culled-{name}-groups-{'table' if tab else 'nodes'}", "culled-entry", "culled",
                            (kind, "groups"), partial(prim_scene, kind, 24, True), ("prim-T", kind, 24),
                            plan=_plan(0, 1, tab, 1, fm=1), lean=False, env={} if tab else {"SMCRT_COOP_TAB": "0"}, **MANY))
    for tab in (1, 0):
        out.append(Case(f"culled-mixed-{'table' if tab else 'nodes'}", "culled-entry", "culled", ("mixed",), mixed_scene,
                        ("mixed",), plan=_plan(0, 1, tab, 1), lean=False, env={} if tab else {"SMCRT_COOP_TAB": "0"}, **MANY))
    out.append(Case("culled-mixed-k7", "culled-entry", "culled", ("mixed",), mixed_scene, ("mixed",),
                    plan=_plan(0, 1, 1, 1), lean=False, env={"SMCRT_CULL_K": "7"}, **MANY))
    out.append(Case("culled-reflected", "culled-entry", "culled", ("reflection",),
                    partial(prim_scene, abi.SDF_CYLINDER, 24, False, "reflect"), ("reflect",), plan=_plan(0, 1, 1, 1),
                    lean=False, **MANY))
    out.append(Case("culled-scaled", "culled-entry", "culled", ("scaled",), scaled_scene, ("scaled",),
                    plan=_plan(0, 1, 1, 1), lean=False, always=True, **MANY))
    return out


def _csg():
    out = []
    for op, name in OPS.items():
        one = partial(csg_scene, op, 1)
        out.append(Case(f"csg-{name}-lean", "csg", "lean", (("op", op),), one, ("csg", op, 1), plan=_plan(1, 0, 0, 0),
                        lean=True, **ONE))
        out.append(Case(f"csg-{name}-serial", "csg", "serial", (("op", op),), one, ("csg", op, 1), plan=_plan(0, 0, 0, 0),
                        lean=False, env=NO_LEAN, **ONE))
        out.append(Case(f"csg-{name}-global", "csg", "global", (("op", op),), partial(csg_scene, op, 11), ("csg", op, 11),
                        plan=_plan(0, 1, 0, 0), lean=False, **MANY))
        out.append(Case(f"csg-{name}-culled", "csg", "culled", (("op", op),), partial(csg_scene, op, 23), ("csg", op, 23),
                        plan=_plan(0, 1, 0, 1), lean=False, **MANY))
    return out


def _modifiers():
    out = []
    for kind, name in MODIFIERS.items():
        out.append(Case(f"mod-{name}-serial", "modifier", "serial", (kind,), partial(modifier_scene, kind, 1),
                        ("mod", kind, 1), plan=_plan(0, 0, 0, 0, nested=1), lean=False, **ONE))
        out.append(Case(f"mod-{name}-global", "modifier", "global", (kind,), partial(modifier_scene, kind, 11),
                        ("mod", kind, 11), plan=_plan(0, 1, 0, 0, nested=1), lean=False, **MANY))
        out.append(Case(f"mod-{name}-culled", "modifier", "culled", (kind,), partial(modifier_scene, kind, 3),
                        ("mod", kind, 3), plan=_plan(0, 1, 0, 1, nested=1), lean=False, always=True, **MANY))
    return out


def _pairs():
    return [Case(f"pairs-{name}", "pairs", "serial", ("pairs",), partial(pair_scene, name), ("pairs", name),
                 plan=_plan(0, 0, 0, 0), lean=False, env=NO_LEAN, **MANY) for name in PAIR_SCENES]


def _far():
    out = []
    for kind in (abi.SDF_TORUS, abi.SDF_SEGMENT, abi.SDF_CAPSULE, abi.SDF_BOX):
        for far in ("on", "off"):
            out.append(Case(f"far-{PRIMITIVES[kind]}-{far}", "far", "table", (kind, "far"), partial(far_scene, kind),
                            ("far", kind), n=100, plan=_plan(0, 1, 1, 0, fm=int(far == "on")), lean=False,
                            env={} if far == "on" else {"SMCRT_FAR_MARCH": "0"}, make_source=wall_source, fresnel=0,
                            reflections=0, far=far))
    for far in ("on", "off"):
        out.append(Case(f"far-near-sphere-{far}", "far", "table", (abi.SDF_SPHERE, "far-near-sphere"), far_sphere_scene,
                        ("far-sphere",), n=100, plan=_plan(0, 1, 1, 0, fm=int(far == "on")), lean=False,
                        env={} if far == "on" else {"SMCRT_FAR_MARCH": "0"}, make_source=skim_source, fresnel=0,
                        reflections=0, far=far))
    return out


CASES = _primitives() + _culled_entries() + _csg() + _modifiers() + _pairs() + _far()
BY_ID = {c.id: c for c in CASES}


def group(name):
    return [c for c in CASES if c.group == name]


def plan_fields(p):
    """The PLAN_FIELDS of a probed plan (tests/planprobe.py)."""
    return {"lean_candidate": p["lean_candidate"], "coop": int(p["coop_lanes"] > 0), "ctab": p["ctab"], "cull": p["cull"],
            "nested": p["nested"], "fm": int(p["fm_err"] > 0.0)}


def subject_tops(case, sc):
    """The 0-based tops a case is there for: those whose node is of the subject kind (a model
    for an op), the scaled sphere, or the reflected tops."""
    out = []
    for i, t in enumerate(sc.top):
        nd = sc.nodes[t]
        if nd.n == MEDIUM.n:  # (the medium box)
            continue
        for s in case.subject:
            if isinstance(s, tuple) and nd.kind == abi.SDF_MODEL and nd.op == s[1]:
                out.append(i)
            elif s == "scaled" and nd.transform[0] == 2.0:
                out.append(i)
            elif s == "reflection" and np.linalg.det(np.array(nd.transform[:]).reshape(4, 4)[:3, :3]) < 0.0:
                out.append(i)
            elif s == nd.kind and not (nd.kind == abi.SDF_SPHERE and case.always):
                out.append(i)
    return out


def abi_values(prefix):
    return {v for k, v in vars(abi).items() if k.startswith(prefix) and isinstance(v, int)}


def check_table():
    """The table covers what it claims: every SDF_* kind of the ABI (1 to 18) and every OP_* is
    the subject of a case on each path listed for it; the culled-entry variants, the pairs in
    all four orders and four transform combinations with their neighbours, and the far-march
    scenes are there; every case states all its plan fields."""
    assert len(BY_ID) == len(CASES), "duplicate case ids"
    kinds, ops = abi_values("SDF_"), abi_values("OP_")
    assert kinds == set(range(1, 19)) and ops == set(OPS), (kinds, ops)
    assert set(PRIMITIVES) | set(MODIFIERS) | {abi.SDF_MODEL} == kinds
    covered = {(s, c.path) for c in CASES if c.group in ("primitive", "csg", "modifier") for s in c.subject}
    want = ({(k, p) for k in PRIMITIVES for p in ("lean", "serial", "table", "culled")} |
            {(("op", o), p) for o in ops for p in ("lean", "serial", "global", "culled")} |
            {(k, p) for k in MODIFIERS for p in ("serial", "global", "culled")})
    assert covered == want, (sorted(map(str, want - covered)), sorted(map(str, covered - want)))
    assert len(group("primitive")) == 40 and len(group("csg")) == 16 and len(group("modifier")) == 21
    ce = group("culled-entry")
    assert sorted((c.subject, c.plan["ctab"]) for c in ce if "groups" in c.subject) == \
        [((k, "groups"), t) for k in (abi.SDF_SPHERE, abi.SDF_CAPSULE) for t in (0, 1)]
    assert {c.subject[0] for c in ce} >= {"mixed", "reflection", "scaled"}
    # the pair branches: both kinds in every order, every translate-only combination of each
    pairs, notes = set(), set()
    for c in group("pairs"):
        sc = c.scene()
        assert sc.n_top < 8 and c.env == NO_LEAN, c.id
        ps, single = pairs_of(sc)
        pairs |= {p[:4] for p in ps}
        last = len(sc.top) - 1
        for kind, i in single:
            if kind == abi.SDF_SPHERE and i == last and ps and ps[-1][4] == i - 2:
                notes.add("odd sphere after a pair")
            if kind == abi.SDF_CYLINDER and i > 0 and sc.nodes[sc.top[i - 1]].kind == abi.SDF_SPHERE:
                notes.add("sphere, cylinder falls through")
            if kind == abi.SDF_MODEL:
                if any(p[4] == i - 2 for p in ps):
                    notes.add("pair before a model")
                if any(p[4] == i + 1 for p in ps):
                    notes.add("pair after a model")
    sb = (abi.SDF_SPHERE, abi.SDF_BOX)
    assert pairs == {(a, b, t1, t2) for a in sb for b in sb for t1 in (True, False) for t2 in (True, False)}, pairs
    assert notes == {"odd sphere after a pair", "sphere, cylinder falls through", "pair before a model",
                     "pair after a model"}, notes
    far = group("far")
    assert {c.subject[0] for c in far if c.far == "on"} >= {abi.SDF_TORUS, abi.SDF_SEGMENT, abi.SDF_CAPSULE, abi.SDF_BOX}
    assert sorted(c.far for c in far) == ["off"] * (len(far) // 2) + ["on"] * (len(far) // 2)
    for c in far:
        assert c.plan["fm"] == int(c.far == "on") and c.n == 100, c.id
    for c in CASES:
        assert tuple(c.plan) == PLAN_FIELDS and c.path in PATHS, c.id
        assert c.lean == (c.path == "lean") == bool(c.plan["lean_candidate"]), c.id
    return {g: len(group(g)) for g in ("primitive", "culled-entry", "csg", "modifier", "pairs", "far")}
