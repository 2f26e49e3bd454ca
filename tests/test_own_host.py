"""The owning types of the host code's GPU resources (sspp_amd/csrc/sspp_own.h), without a GPU and
without the HIP runtime: tests/own/check_own.cpp defines the HIP entry points the header uses on top
of malloc (live counts, a call log, "fail the k-th creating call", abort on a free of an unknown
pointer) and runs under AddressSanitizer and UBSan as a stand-alone program.

What it checks: reserve() grows only; a creation sequence shaped like sspp_job_set_queries (two
device buffers, the pinned staging, its event) and one shaped like the k_tsp_pp2 records (three
device buffers, the last zeroed), each failed at every creating call in turn, returns SSPP_E_NOMEM
(SSPP_E_HIP for the event), leaves every member whole or empty, succeeds at the next attempt without
allocating anything twice, and leaves nothing alive after its scope; moves empty their source, move
assignment frees the target's buffer, self-assignment is harmless; release() leaves nothing to free;
a buffer moved into the retired list is freed once, when the list dies; Staging.wait() makes no HIP
call without a pending copy and one with, and its destructor synchronises the event before the
pinned memory is freed.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

CASES = ["reserve", "set_queries sweep", "records sweep", "moves", "release and retired", "staging"]


def test_owning_types_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "the host build needs g++"
    exe = str(tmp_path / "check_own")
    subprocess.check_call([gxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g",
                           "-I" + os.path.join(ROOT, "sspp_amd", "csrc"),
                           os.path.join(HERE, "own", "check_own.cpp"), "-o", exe])
    r = subprocess.run([exe], text=True, timeout=60, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.splitlines() == [c + " ok" for c in CASES]
