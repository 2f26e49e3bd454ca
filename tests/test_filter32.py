"""k_sspp_c2f's FP32-filtered scan (sspp_amd/csrc/sspp_filter.h): FP32 may only settle what the
FP64 narrowphase settles the same way.  The host build of the filter runs against the FP64
functions the kernel falls back to (pair_near, sat_box_box, col_plane_box) on random box-box
and plane-box configurations placed 1e-8..1e-1 m (per metre of extent) from touching, through the
kernel's input pipeline (a 4-term spline evaluation of position and quaternion from control
points, doubles vs their float copies; v_rsq_f32's 1-ulp error emulated): every certain FP32
decision must equal FP64's in both argument orders, and FP32's error must stay inside eps.

The configurations come from named strata, which together span the envelope f32_eps certifies:
  base    (filter32/check_filter.cpp) partners in [-1, 1]^3, half extents <= 0.6 m, the moving box
          at its mover's root, planes untilted at z = 0: S <= 1.7, eps = 2e-4
and in filter32/check_envelope.cpp, with eps = the library's f32_eps of the pair's own table,
  far     root coordinates up to +-7.99 m, partners up to +-16 m, S up to 8
  large   half extents of metres on either box, S spread over (1, 8]
  offset  the moving box a geom up to 2 m off its root with its own rotation (SSPF_LOAD_GEOM /
          SSPF_GEOM_ROT's matvec3f / matmul3f against geom_pose)
  movers  the partner a geom of a second mover (the omover >= 0 composition)
  plane   tilted planes, the GPU scenes' ramp among them, their origin up to 16 m per axis from
          the contact
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc")
def test_filter_never_contradicts_fp64(tmp_path):
    exe = str(tmp_path / "check_filter")
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    subprocess.check_call([hipcc, "-std=c++17", "-O2", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "sspp_amd", "csrc"),
                           os.path.join(HERE, "filter32", "check_filter.cpp"), "-o", exe])
    r = subprocess.run([exe, "300000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches 0" in r.stdout
    m = re.search(r"tested (\d+) certain-hit (\d+) certain-no (\d+)", r.stdout)
    tested, hit, no = (int(x) for x in m.groups())
    assert tested > 250000 and hit > 20000 and no > 20000  # both certificates exercised
    err = float(re.search(r"per metre of scale ([0-9.e+-]+)", r.stdout).group(1))
    assert err < 2e-4 / 50, r.stdout  # FP32's error is far inside the certified margin


STRATA = ("far", "large", "offset", "movers", "plane")
PER_STRATUM = 30000
EPS_PER_METRE = 2e-4      # sspp_kern.h: kF32EpsPerMetre
BUDGET_PER_METRE = 6e-5   # DESIGN.md §5's stated FP32 error per metre of S


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc")
def test_filter_over_the_certified_envelope(tmp_path):
    """Per stratum: no certain FP32 decision contradicts FP64; FP32's largest error on a decision
    quantity per metre of max(1, S) is below eps's 2e-4 (else the certificate is unsound) and is
    printed next to DESIGN.md's 6e-5 budget; at least 5 % of the tested configurations end as a
    certain HIT and 5 % as a certain NO (a stratum that is all "ambiguous" proves nothing)."""
    exe = str(tmp_path / "check_envelope")
    hipcc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "sspp_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "filter32", "check_envelope.cpp"), "-o", exe])
    r = subprocess.run([exe, str(PER_STRATUM)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] == "stratum":
            seen[w[1]] = dict(zip(w[2::2], w[3::2]))
    assert tuple(seen) == STRATA
    for name, f in seen.items():
        tested, hit, no = int(f["tested"]), int(f["certain-hit"]), int(f["certain-no"])
        err = float(f["error-per-metre"])
        print("%-7s tested %d hit %.1f%% no %.1f%% error %.2e of eps %.0e (budget %.0e: %s)" % (
            name, tested, 100.0 * hit / tested, 100.0 * no / tested, err, EPS_PER_METRE, BUDGET_PER_METRE,
            "inside" if err <= BUDGET_PER_METRE else "EXCEEDED"))
        assert int(f["mismatches"]) == 0, line
        assert err < EPS_PER_METRE, (name, err)
        assert tested >= 0.8 * PER_STRATUM, (name, tested)
        assert hit >= 0.05 * tested and no >= 0.05 * tested, (name, tested, hit, no)
    # each stratum reached the part of the envelope it is named for
    assert float(seen["far"]["largest-root"]) > 7.9 and float(seen["far"]["largest-partner"]) > 15.0
    assert float(seen["far"]["largest-S"]) > 7.5 and float(seen["large"]["largest-S"]) > 7.5
    assert float(seen["plane"]["largest-partner"]) > 15.0
