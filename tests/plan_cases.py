"""The cases that drive every transport-kernel instantiation, every jmean deposit regime and
the axis-length edges: plain data and helpers shared by tests/test_sceneplan.py (the plan each
case must get, without a GPU) and tests/test_gpu_instantiations.py (the run against the oracle).

The engine compiles transport_kernel<lds_faces, grid_mode, xsrc, coop> 21 times and
ws_kernel<lds_faces, grid_mode, xf, slots> 24 times (kinst.hip, kernel_ptrs.h); plan_scene
(sceneplan.cpp) and the launch rules of sceneplan.h pick one of them and one of the deposit
regimes from the grid, the scene, the knobs and the run. A case states the plan fields it must
get and the kernel it must therefore run; `kernel_of` restates the engine's choice from a
probed plan, and `check_table` asserts that the matrix is exactly the 45 instantiations, so a
dropped case fails the suite instead of shrinking it.
"""
from dataclasses import dataclass, field

from rsmcrt_amd import abi, builders, scene

PLAN_FIELDS = ("lds_faces", "grid_mode", "lean_candidate", "ws_slots", "coop", "xf", "n_tiles", "bucketed",
               "hist_tiles")
TILE_VOXELS = 1 << 14  # deposit.h TILE_SHIFT


# ---- building blocks ----
def sphere():  # one HG sphere, no index step: the plain ws_kernel
    return builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 1.0)


def fresnel_sphere():  # n = 1.33 in n = 1: plan.fresnel, the XF ws_kernel
    return builders.setup_sphere(10.0, 0.1, 0.9, 1.33, 1.0)


def fresnel_sphere_small():
    """The Fresnel sphere scaled by 1/25 (radius 0.04, the same optical depths). The grids of grid
    mode 0 span (-0.05, 0.05)^3, which the unit sphere contains: no photon would meet its surface
    and the XF kernels would run without one Fresnel event."""
    return builders.setup_sphere(250.0, 2.5, 0.9, 1.33, 0.04)


def coop_spheres():  # ten tops: coop_lanes == 2 and the cooperative EVAL's table
    return builders.setup_sphere_scene(builders.random_sphere_list(9))


def weak_sphere():  # long free paths: a face source reaches every tile of a large grid
    return builders.setup_sphere(0.5, 0.01, 0.9, 1.0, 1.0)


def circular():  # the general emitter of test_gpu_parity._xsrc_cases()
    return scene.circular_source((0.1, -0.2, 0.3), (1.0, 2.0, 2.0), 0.5)


def circular_small():
    """The same disc scaled by 1/20. The grids of grid mode 0 span (-0.05, 0.05)^3, so the disc
    of `circular` (centre 0.37 from the origin, radius 0.5) starts every photon outside them
    and none enters the medium; this one lies inside the grid."""
    return scene.circular_source((0.005, -0.01, 0.015), (1.0, 2.0, 2.0), 0.025)


def point_off_face():
    """The 48-voxel grid of half-extent 0.05 has a face of every axis at the origin, and its
    computed position, 24 * 0.1 / 48, is one ulp above 0.05: photons that start there are in cell
    25 but below its lower face, and 1756 of 2000 end at their first step (wall_dist's negative
    distance, the reference's error stop). This origin is inside a cell."""
    return scene.point_source((0.001, 0.002, 0.003))


def face_source():  # test_sphere_scene's: the whole top face, straight down
    return scene.uniform_source((-1.0, -1.0, 0.9999999), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, -1.0))


# (lds_faces, grid_mode) -> nx, ny, nz, half-extent. Faces and props stay in LDS up to
# MAX_FACE_BYTES = 40960: (nx+ny+nz+4)*8 + 32*n_top; 5200 + 8 + 4 faces are 41696 B.
# Grid mode 2: every 2*max and every n a power of two; 1: every 2*max only; 0: neither.
GRIDS = {
    (1, 2): (32, 32, 32, 1.0), (1, 1): (48, 48, 48, 1.0), (1, 0): (48, 48, 48, 0.05),
    (0, 2): (8192, 2, 2, 1.0), (0, 1): (5200, 4, 4, 1.0), (0, 0): (5200, 4, 4, 0.05),
}


@dataclass(frozen=True)
class Case:
    id: str
    group: str      # "matrix", "small-n", "deposit", "axis-bound" or "tiny"
    make_scene: object
    grid: tuple     # nx, ny, nz, half-extent of every axis
    make_source: object
    n: int
    plan: dict      # the PLAN_FIELDS the probe must report
    lean: bool      # the run launches ws_kernel
    kernel: tuple   # ("ws_kernel", lds_faces, grid_mode, xf, slots) | ("transport_kernel", lds_faces, grid_mode, xsrc, coop)
    env: dict = field(default_factory=dict)
    flags: int = abi.FLAG_PATHLENGTH
    regime: str = "buckets"  # "buckets", "sorted-fused", "sorted-bin_hist" or "atomics"
    axis: int = -1           # axis-bound cases: the long axis

    def scene(self):
        return self.make_scene()

    def source(self):
        return self.make_source()

    def scene_grid(self):
        nx, ny, nz, ext = self.grid
        return scene.grid(nx, ny, nz, ext, ext, ext)

    @property
    def xsrc(self):
        return self.source().kind not in (abi.SRC_POINT, abi.SRC_PENCIL, abi.SRC_UNIFORM)


def tiles_of(grid):
    nx, ny, nz, _ = grid
    return (nx * ny * nz + TILE_VOXELS - 1) // TILE_VOXELS


def _plan(lds, gm, lean_candidate, slots, coop, xf, n_tiles, bucketed=1, hist_tiles=0):
    return dict(zip(PLAN_FIELDS, (lds, gm, lean_candidate, slots, coop, xf, n_tiles, bucketed, hist_tiles)))


def _matrix():
    out = []
    # ws_kernel<F, G, xf, slots>: 2 * 3 * 2 * 2
    for (f, g), grid in GRIDS.items():
        point = point_off_face if (f, g) == (1, 0) else scene.point_source
        for xf in (0, 1):
            for slots in (3, 2):
                sc = (fresnel_sphere_small if g == 0 else fresnel_sphere) if xf else sphere
                out.append(Case(f"ws-F{f}-G{g}-xf{xf}-s{slots}", "matrix", sc, grid, point, 2000,
                                _plan(f, g, 1, slots, 0, xf, tiles_of(grid)), True, ("ws_kernel", f, g, xf, slots),
                                env={"SMCRT_WS_SLOTS": "2"} if slots == 2 else {}))
    # transport_kernel<F, G, xsrc, coop>: 2 * 3 * 3, and xsrc && coop with faces in device memory only
    for (f, g), grid in GRIDS.items():
        for xsrc, coop in ((0, 0), (1, 0), (0, 1)):
            point = point_off_face if (f, g) == (1, 0) else scene.point_source
            src = (circular_small if g == 0 else circular) if xsrc else point
            out.append(Case(f"tr-F{f}-G{g}-x{xsrc}-c{coop}", "matrix", coop_spheres if coop else sphere, grid, src, 2000,
                            _plan(f, g, 0, 3, coop, coop, tiles_of(grid)), False, ("transport_kernel", f, g, xsrc, coop),
                            env={} if coop else {"SMCRT_LEAN": "0"}))
    # the plan stages the faces of these grids in LDS; transport_kernel_ptr takes the only
    # xsrc && coop form there is, with faces in device memory
    for g in (2, 1, 0):
        grid = GRIDS[(1, g)]
        out.append(Case(f"tr-F0-G{g}-x1-c1", "matrix", coop_spheres, grid, circular_small if g == 0 else circular, 2000,
                        _plan(1, g, 0, 3, 1, 1, tiles_of(grid)), False, ("transport_kernel", 0, g, 1, 1)))
    return out


def _small_n():
    """One lane, and one lane past a wave, in ws_kernel<false, 2, false, 3> and its
    transport_kernel twin."""
    grid = GRIDS[(0, 2)]
    out = []
    for n in (1, 65):
        out.append(Case(f"ws-F0-G2-xf0-s3-n{n}", "small-n", sphere, grid, scene.point_source, n,
                        _plan(0, 2, 1, 3, 0, 0, tiles_of(grid)), True, ("ws_kernel", 0, 2, 0, 3)))
        out.append(Case(f"tr-F0-G2-x0-c0-n{n}", "small-n", sphere, grid, scene.point_source, n,
                        _plan(0, 2, 0, 3, 0, 0, tiles_of(grid)), False, ("transport_kernel", 0, 2, 0, 0),
                        env={"SMCRT_LEAN": "0"}))
    return out


def _deposit():
    """The four jmean deposit regimes by tile count (sceneplan.cpp, deposit.h), each at the tile
    counts where the next one takes over. 20000 photons from the whole top face through the
    weak sphere touch every tile of each grid (the tests assert it on the oracle's jmean)."""
    def case(name, grid, plan, lean, kernel, regime, env=None):
        return Case("dep-" + name, "deposit", weak_sphere, grid, face_source, 20000, plan, lean, kernel, env=env or {},
                    regime=regime)
    return [
        # 1024 = MAX_DIRECT_TILES: the last bucketed size (8 KiB of bucket words per block)
        case("buckets-1024", (256, 256, 256, 1.0), _plan(1, 2, 1, 3, 0, 0, 1024), True, ("ws_kernel", 1, 2, 0, 3), "buckets"),
        # one past it: sorted records, counted by bin_hist (past MAX_FUSED_HIST_TILES = 512)
        case("sorted-1056", (264, 256, 256, 1.0), _plan(1, 1, 0, 3, 0, 0, 1056, 0), False, ("transport_kernel", 1, 1, 0, 0),
             "sorted-bin_hist"),
        # sorted by request, one tile past the fused histogram
        case("sorted-513", (513, 128, 128, 1.0), _plan(1, 1, 0, 3, 0, 0, 513, 0), False, ("transport_kernel", 1, 1, 0, 0),
             "sorted-bin_hist", env={"SMCRT_DEPOSIT": "sorted"}),
        # 4096 = MAX_TILES: the last binned size
        case("sorted-4096", (512, 512, 256, 1.0), _plan(1, 2, 0, 2, 0, 0, 4096, 0), False, ("transport_kernel", 1, 2, 0, 0),
             "sorted-bin_hist"),
        # past it: n_tiles == 0, no fold state, fp64 atomics
        case("atomics-4112", (512, 512, 257, 1.0), _plan(1, 1, 0, 3, 0, 0, 0, 0), False, ("transport_kernel", 1, 1, 0, 0),
             "atomics"),
    ]


LEAN_AXIS_LIMIT = (1 << 20) - 2  # sceneplan.cpp: the lean path packs cell indices of axes below this


def _axis_bounds():
    """Each axis at LEAN_AXIS_LIMIT - 1 (the longest lean axis: the packed cell index uses its
    top bit) and at LEAN_AXIS_LIMIT (transport_kernel). Neither length is a power of two (grid
    mode 1), the faces (8 MiB) stay in device memory, and 4 * 2^20 voxels are 256 tiles."""
    out = []
    for axis, name in enumerate("xyz"):
        for n_axis in (LEAN_AXIS_LIMIT - 1, LEAN_AXIS_LIMIT):
            dims = [2, 2, 2]
            dims[axis] = n_axis
            lean = n_axis < LEAN_AXIS_LIMIT
            out.append(Case(f"axis-{name}-{'below' if lean else 'at'}-limit", "axis-bound", sphere, (*dims, 1.0),
                            scene.point_source, 16, _plan(0, 1, int(lean), 3, 0, 0, 256), lean,
                            ("ws_kernel", 0, 1, 0, 3) if lean else ("transport_kernel", 0, 1, 0, 0), axis=axis))
    return out


def _tiny():
    """Axes of 1, 2 and 3 voxels (zface has nz + 2 entries, the other axes n + 1), on the lean
    path and with SMCRT_LEAN=0."""
    out = []
    for dims in ((1, 1, 1), (1, 7, 3), (3, 1, 2), (2, 2, 1)):
        gm = 2 if all(d & (d - 1) == 0 for d in dims) else 1
        name = "x".join(map(str, dims))
        out.append(Case(f"tiny-{name}-lean", "tiny", sphere, (*dims, 1.0), scene.point_source, 2000,
                        _plan(1, gm, 1, 3, 0, 0, 1), True, ("ws_kernel", 1, gm, 0, 3)))
        out.append(Case(f"tiny-{name}-transport", "tiny", sphere, (*dims, 1.0), scene.point_source, 2000,
                        _plan(1, gm, 0, 3, 0, 0, 1), False, ("transport_kernel", 1, gm, 0, 0), env={"SMCRT_LEAN": "0"}))
    return out


CASES = _matrix() + _small_n() + _deposit() + _axis_bounds() + _tiny()
BY_ID = {c.id: c for c in CASES}

# every compiled instantiation (kinst.hip)
WS_KERNELS = {("ws_kernel", f, g, xf, s) for f in (0, 1) for g in (0, 1, 2) for xf in (0, 1) for s in (2, 3)}
TRANSPORT_KERNELS = {("transport_kernel", f, g, x, c) for f in (0, 1) for g in (0, 1, 2) for x in (0, 1) for c in (0, 1)
                     if not (f and x and c)}
REGIMES = ("buckets", "sorted-fused", "sorted-bin_hist", "atomics")


def group(name):
    return [c for c in CASES if c.group == name]


def plan_fields(p, dets=()):
    """The PLAN_FIELDS of a probed plan (tests/planprobe.py)."""
    out = {k: p[k] for k in PLAN_FIELDS if k in p}
    out["coop"] = int(p["coop_lanes"] > 0)
    out["xf"] = int(bool(p["fresnel"]) or len(dets) > 0)  # smcrt.hip: the lane scratch, ws_kernel's XF
    return out


def regime_of(p):
    """The deposit regime of a path-length run without survival bias (sceneplan.h launch_binned)."""
    if p["n_tiles"] == 0 or p["force_atomic"]:
        return "atomics"
    if p["bucketed"]:
        return "buckets"
    return "sorted-fused" if p["hist_tiles"] else "sorted-bin_hist"


def kernel_of(p, xsrc, flags=abi.FLAG_PATHLENGTH, dets=()):
    """The instantiation the engine launches for a probed plan: sceneplan.h launch_lean, then
    kernel_ptrs.h ws_kernel_ptr / transport_kernel_ptr as smcrt.hip calls them. (The lane-scratch
    allocation can still veto the lean path; the GPU test reads lean_launches for that.)"""
    f = plan_fields(p, dets)
    plain = bool(flags & abi.FLAG_PATHLENGTH) and not flags & abi.FLAG_SURVIVAL_BIAS
    lean = bool(f["lean_candidate"]) and not xsrc and plain and regime_of(p) == "buckets"
    if lean:
        return ("ws_kernel", f["lds_faces"], f["grid_mode"], f["xf"], f["ws_slots"])
    lds = 0 if (xsrc and f["coop"]) else f["lds_faces"]
    return ("transport_kernel", lds, f["grid_mode"], int(xsrc), f["coop"])


CTAB_BYTES = 21 * 64 * 8  # transport.h CTAB_DOUBLES doubles: the cooperative EVAL's primitive table
# (name, flags, lean_ok, paths_on, phasor_on, n_screens): the run states whose choice
# tests/test_sceneplan.py compares with the probe's
RUN_STATES = (
    ("plain", abi.FLAG_PATHLENGTH, 1, 0, 0, 0),
    ("survival-bias", abi.FLAG_PATHLENGTH | abi.FLAG_SURVIVAL_BIAS, 1, 0, 0, 0),
    ("test-kernel", abi.FLAG_PATHLENGTH | abi.FLAG_TEST_KERNEL, 1, 0, 0, 0),
    ("paths-on", abi.FLAG_PATHLENGTH | abi.FLAG_TRACK_PATHS, 1, 1, 0, 0),
    ("paths-unset", abi.FLAG_PATHLENGTH | abi.FLAG_TRACK_PATHS, 1, 0, 0, 0),
    ("phasor-on", abi.FLAG_PATHLENGTH | abi.FLAG_PHASOR, 1, 0, 1, 0),
    ("phasor-unset", abi.FLAG_PATHLENGTH | abi.FLAG_PHASOR, 1, 0, 0, 0),
    ("phasor-screens", abi.FLAG_PATHLENGTH | abi.FLAG_PHASOR, 1, 0, 1, 2),
    ("phasor-unset-screens", abi.FLAG_PATHLENGTH | abi.FLAG_PHASOR, 1, 0, 0, 2),
    ("no-lean", abi.FLAG_PATHLENGTH, 0, 0, 0, 0),
)


def run_state_of(flags, paths_on, phasor_on, n_screens):
    """(hist, phas, scr) of a launch of transport_kernel: the path recorder when
    the run asks for paths and tracking is configured, else the phasor tally when the run asks for
    it and it is configured (never both), and the screens' LDS row when that tally has screens."""
    hist = bool(flags & abi.FLAG_TRACK_PATHS) and bool(paths_on)
    phas = bool(flags & abi.FLAG_PHASOR) and bool(phasor_on) and not hist
    return hist, phas, phas and n_screens > 0


def dep_bytes_of(p):
    """A block's deposit state in LDS (deposit.h): a 64-bit bucket word per tile, or a tile
    histogram per wave."""
    return 4 * (2 * p["n_tiles"] if p["bucketed"] else 4 * p["hist_tiles"])


def choice_of(p, xsrc, flags=abi.FLAG_PATHLENGTH, dets=(), lean_ok=True, paths_on=False, phasor_on=False, n_screens=0,
              kind="sdf", env=None):
    """The whole launch choice for a probed plan, in the keys of planprobe.choices: `kernel_of`,
    then hist / phas / scr, ws_kernel's TK and in-voxel coordinates, the dynamic LDS bytes, and
    `grid`: launches with equal values share a persistent grid. Written from DESIGN.md §4 and the
    launch sites smcrt.hip had before sceneplan.h launch_choice, not from that function."""
    c = dict.fromkeys(("xsrc", "lds_faces", "coop", "hist", "phas", "xf", "slots", "iv", "tk", "scr"), 0)
    c.update(gm=p["grid_mode"], block="256")
    if kind in ("voxel", "mesh"):  # voxel_kernel<gm, xsrc>, mesh_kernel<gm, xsrc>: media + faces, then the deposit words
        c.update(family=kind + "_kernel", xsrc=int(xsrc), lds=p["face_bytes"] + dep_bytes_of(p))
        c["grid"] = (c["family"], c["xsrc"])
        return c
    k = kernel_of(p, xsrc, flags, dets)
    tracked = flags & (abi.FLAG_TRACK_PATHS | abi.FLAG_PHASOR)  # ws_kernel has neither
    if k[0] == "ws_kernel" and lean_ok and not tracked:
        knob = (env or {}).get("SMCRT_WS_INVOXEL")  # on by default in the plain instantiation only
        iv = int(not k[3]) if knob is None else int(knob != "0")
        c.update(family="ws_kernel", lds_faces=k[1], xf=k[3], slots=k[4], iv=iv, tk=int(bool(flags & abi.FLAG_TEST_KERNEL)),
                 block="ws", lds=(p["face_bytes"] if p["lds_faces"] else 0) + 8 * p["n_tiles"])
        c["grid"] = ("ws_kernel",)  # (TK or not: same block, LDS and register cap)
        return c
    f = plan_fields(p, dets)
    hist, phas, scr = run_state_of(flags, paths_on, phasor_on, n_screens)
    faces = bool(f["lds_faces"]) and not (xsrc and f["coop"]) and not hist and not phas
    rows = 4 if scr else 3 if len(dets) else 0  # start points: 256 doubles a row
    c.update(family="transport_kernel", xsrc=int(xsrc), lds_faces=int(faces), coop=f["coop"], hist=int(hist), phas=int(phas),
             scr=int(scr), lds=(p["face_bytes"] if faces else 0) + rows * 256 * 8 + dep_bytes_of(p) +
             (CTAB_BYTES if p["ctab"] and f["coop"] else 0))
    c["grid"] = ("transport_kernel", c["xsrc"], c["hist"], c["phas"], c["scr"])
    return c


def check_table():
    """The table covers what it claims: each of the 24 + 21 instantiations exactly once in the
    matrix, the deposit regimes at their five boundary sizes, six axis-bound and eight tiny
    cases, every case with all plan fields and a lean flag that matches its kernel."""
    assert len(BY_ID) == len(CASES), "duplicate case ids"
    m = [c.kernel for c in group("matrix")]
    assert len(m) == len(set(m)) == 45, len(m)
    assert {k for k in m if k[0] == "ws_kernel"} == WS_KERNELS and len(WS_KERNELS) == 24
    assert {k for k in m if k[0] == "transport_kernel"} == TRANSPORT_KERNELS and len(TRANSPORT_KERNELS) == 21
    dep = group("deposit")
    assert [tiles_of(c.grid) for c in dep] == [1024, 1056, 513, 4096, 4112]
    assert [c.regime for c in dep] == ["buckets", "sorted-bin_hist", "sorted-bin_hist", "sorted-bin_hist", "atomics"]
    ab = group("axis-bound")
    assert sorted((c.axis, c.grid[c.axis], c.lean) for c in ab) == \
        [(a, n, n < LEAN_AXIS_LIMIT) for a in range(3) for n in (LEAN_AXIS_LIMIT - 1, LEAN_AXIS_LIMIT)]
    tiny = group("tiny")
    assert len(tiny) == 8 and sorted({c.grid[:3] for c in tiny}) == [(1, 1, 1), (1, 7, 3), (2, 2, 1), (3, 1, 2)]
    assert all(sum(c.lean for c in tiny if c.grid == g) == 1 for g in {c.grid for c in tiny})
    assert sorted((c.kernel[0], c.n) for c in group("small-n")) == \
        [("transport_kernel", 1), ("transport_kernel", 65), ("ws_kernel", 1), ("ws_kernel", 65)]
    for c in CASES:
        assert tuple(c.plan) == PLAN_FIELDS, c.id
        assert c.lean == (c.kernel[0] == "ws_kernel"), c.id
        assert c.regime in REGIMES, c.id
    return {"ws_kernel": 24, "transport_kernel": 21, "deposit": len(dep), "axis-bound": len(ab), "tiny": len(tiny)}
