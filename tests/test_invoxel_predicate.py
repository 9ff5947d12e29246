"""The in-voxel predicate (rsmcrt_amd/csrc/invoxel.h) against a literal restatement of
update_grids' first crossing, on the CPU: tests/invoxel_probe.cpp, a stand-alone program built
with g++ -O2 -ffp-contract=off (no HIP, no libsmcrt.so).

ws_kernel's photon waves deposit a segment themselves when the predicate says it ends inside
its start voxel (ws.h), so a true answer for a segment the reference would walk further, or
stop on with an error, would change the tallies. False is always safe.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "invoxel_probe.cpp")
SEED = 123456789


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("invoxel") / "invoxel_probe")
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-o", exe, SRC], check=True)
    out = subprocess.run([exe, str(SEED), "1000000", "1000000"], check=True, capture_output=True, text=True)
    print(out.stdout)
    print(out.stderr)
    return {k: int(v) for k, v in (line.split("=", 1) for line in out.stdout.splitlines() if "=" in line)}


def test_soundness(probe):
    """Zero violations over 10^6 seeded random cases and 5 * 10^5 adversarial ones: starts on a
    face and 1-4 ulps either side of it, len within 4 ulps of each exact quotient, len = 0, NaN
    and infinite inputs, direction components 0, +-2^-500, +-2^-501 and denormal, on grids with
    power-of-two, other (48, 67 cells) and anisotropic (0.16 x 0.09 x 0.13) spacings. NaNs, tiny
    direction components, numerators against the direction and lengths outside [0, 100000) all
    come out false."""
    assert probe["random_cases"] >= 1_000_000 and probe["adversarial_cases"] >= 500_000
    assert probe["random_accepted"] > probe["random_cases"] // 4  # (the cases do exercise true answers)
    assert probe["adversarial_accepted"] > 10_000
    assert probe["random_violations"] == 0 and probe["adversarial_violations"] == 0
    assert probe["complete_violations"] == 0
    assert probe["nan_true"] == 0 and probe["tiny_dir_true"] == 0
    assert probe["neg_num_true"] == 0 and probe["bad_len_true"] == 0


def test_completeness_not_below_far_form(probe):
    """On segments drawn like M1's (128^3 over 2 x 2 x 2, starts uniform in a voxel, len
    log-uniform in [1e-8, 0.05]) the predicate accepts no smaller share of the true one-crossing
    segments than far.h's form (refined reciprocal, 2^-40 margin) on the same cases."""
    single = probe["complete_single"]
    assert single > 0
    share, share_far = probe["complete_accepted"] / single, probe["complete_accepted_far"] / single
    print(f"accepted share of true one-crossing segments: {share:.9f} (far.h's form: {share_far:.9f}); "
          f"accepted by far.h's form only: {probe['complete_far_only']}")
    assert share >= share_far
