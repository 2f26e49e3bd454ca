"""A job's pair tables on the host (sspp_kern.h: PairTable, table_set, launch_table), without a GPU:
tests/pairtable/check_pairtable.cpp builds scene records by hand and prints what the host derives.

Every expected value below is worked out from the rules, not from the code:
  * np = the table's pairs; og = 1 when every pair has the same moving geom (also for an empty
    table); cb = the OR over the pairs of 1 (cylinder-box, either way round), 2 (a capsule on
    either side), 4 (cylinder-cylinder), with types 3 capsule, 5 cylinder, 6 box;
  * feps = 2e-4 * max(1, the largest rbound + orbound + margin) for geoms at their mover's root, and
    0 for an empty table, more than 64 pairs, an extent above 8 m or a moving geom with rbound <= 0.
The moving geoms: 0 box (rbound 0.5), 1 cylinder (0.25), 2 capsule (0.125), 3 box (rbound 0).
The pairs (moving geom, partner type, orbound, margin):
  box_cyl (0, 5, 0.5, 0)   cyl_cyl (1, 5, 1.0, 0.25)   cap_box (2, 6, 0.25, 0)
  box_box (0, 6, 2.0, 0.5)   small (1, 6, 0.25, 0)   cyl_box (1, 6, 1.5, 0.25)
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"

TABLES = [
    # mixed: bits 1 | 4 | 2 | 0; geoms 0, 1, 2, 0; extents 1.0, 1.5, 0.375, 3.0
    (4, 7, 0, 2e-4 * 3.0),
    # one geom: box_box twice; extent 0.5 + 2.0 + 0.5 = 3.0
    (2, 0, 1, 2e-4 * 3.0),
    # two geoms: box_cyl (bit 1, geom 0, extent 1.0), cyl_box (bit 1, geom 1, extent 0.25 + 1.5 + 0.25 = 2.0)
    (2, 1, 0, 2e-4 * 2.0),
    # small: cylinder-box, extent 0.25 + 0.25 = 0.5 -> the 1 m floor
    (1, 1, 1, 2e-4 * 1.0),
    # empty, with and without a scene
    (0, 0, 1, 0.0),
    (0, 0, 1, 0.0),
    # 65 times box_box
    (65, 0, 1, 0.0),
    # box_box and (0, 6, 7.75, 0): extent 0.5 + 7.75 = 8.25 > 8
    (2, 0, 1, 0.0),
    # box_box and a pair of geom 3 (rbound 0): two geoms
    (2, 0, 0, 0.0),
]


def test_pair_table_flags_margin_and_launch_selection(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "the host build needs hipcc"
    exe = str(tmp_path / "check_pairtable")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "sspp_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "pairtable", "check_pairtable.cpp"), "-o", exe])
    lines = subprocess.check_output([exe], text=True, timeout=60).splitlines()
    assert len(lines) == len(TABLES) + 3
    for line, want in zip(lines, TABLES):
        np_, cb, og, feps = line.split()
        assert (int(np_), int(cb), int(og), float(feps)) == want, (line, want)
    # the table of a launch, as an index (0 full, 1 sampled, 2 query set), for (caller splines,
    # query launch) = (no, no), (no, yes), (yes, no), (yes, yes): sampled candidates scan the
    # sampled table, caller splines the full one, a query launch its set's whatever else is set
    assert lines[len(TABLES)].split() == ["1", "2", "0", "2"]
    # a table without a device copy leaves the launch the scene's own pairs {box_cyl, cyl_cyl}
    # (2 pairs, bits 1 | 4, geoms 0 and 1) and the scene's device table; one with a copy gives its
    # own {box_box} (1 pair, no bits, one geom) and that copy
    assert lines[len(TABLES) + 1].split() == ["2", "5", "0", "0"]
    assert lines[len(TABLES) + 2].split() == ["1", "0", "1", "1"]
