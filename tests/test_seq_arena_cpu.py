"""CPU: tests/seq_arena_check.cc — the per-sequence map arenas (csrc/seq_arena.h) and the one-block observation lists of csrc/slam_map.h: list
operations across every capacity boundary, block reuse, chunks returned to the pool on a map reset, and a seeded differential run of add_observation /
erase_observation / set_bad_point / replace_point against a std::vector restatement (host C++, stand-alone program, no GPU, no oracle)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DOSLAM_ARENA_PASSTHROUGH"]],
                         ids=["arena", "sanitized_passthrough"])
def test_seq_arena_check(tmp_path, flags):
    exe = str(tmp_path / "seq_arena_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(HERE, "seq_arena_check.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "seq_arena_check ok" in out.stdout, out.stdout + out.stderr
