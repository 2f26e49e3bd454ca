"""The kernels' dynamic LDS layouts (sspp_amd/csrc/sspp_lds.h): k_sspp_c2f, its split epilogue,
k_sspp_census and k_tsp_pp / k_tsp_pp2 take their pointers from one layout each, and the host its
launch's byte count.  The host program sweeps the layouts' parameters (regions disjoint, inside
`bytes`, aligned; the FP32 copies at the doubles' offsets; phase 3's reuse of the hull boxes) and
pins the byte counts of the formulas the layouts replaced."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_lds_layouts(tmp_path):
    exe = str(tmp_path / "check_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "sspp_amd", "csrc"),
                           os.path.join(HERE, "lds_layout", "check_layout.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"layouts checked (\d+) failures (\d+)", r.stdout)
    assert int(m.group(1)) == 2 * 7 * 13 * 2 * 4 * 2 * 6 and int(m.group(2)) == 0, r.stdout
