"""object_slam_amd/csrc/stage_layout.h, the layout of the staging blocks of the host-pointer entry points, as a stand-alone host program (no GPU)."""
import os
import subprocess


def test_stage_layout_unit_checks(tmp_path):
    """tests/stage_layout_check.cc under AddressSanitizer and UBSan: offsets on 256-byte boundaries, fields disjoint and in declaration order, empty fields
    without room, total = sum of the rounded sizes, the sim3 block of 3 problems / 70 correspondences pinned by hand, and the put / get round trip."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "stage_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(here, "stage_layout_check.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
