"""object_slam_amd/csrc/window_search_host.h, the host arithmetic the windowed projection searches share, as a stand-alone host program (no GPU)."""
import os
import subprocess


def test_window_search_host_checks(tmp_path):
    """tests/window_search_check.cc: the code and the precedence of every shared refusal of a call and of a problem record, the accepted boundary values (an
    offset exactly at n_rows - n, n = 0, INT_MAX offsets that must not overflow), Fuse's record check without the kp_out terms, and the camera block (invW /
    invH, the zero fill of scale[nlevels ..])."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "window_search_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(here, "window_search_check.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
