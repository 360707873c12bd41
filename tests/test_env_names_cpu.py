"""The environment names the library reads are the ones INTEGRATION.md lists ("Environment names the library reads"): a name added to the sources without a row,
or a row whose name nothing reads any more, fails here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_getenv_names_equal_the_table_of_integration_md():
    read = set()
    for d in ("object_slam_amd/csrc", "include"):
        for path in glob.glob(os.path.join(ROOT, d, "*")):
            with open(path, errors="replace") as f:
                read |= set(re.findall(r'getenv\(\s*"(OSLAM_[A-Z0-9_]*)"', f.read()))
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        section = f.read().split("### Environment names the library reads", 1)[1]
    listed = [m.group(1) for m in re.finditer(r"^\| `(OSLAM_[A-Z0-9_]*)` \|", section, re.M)]
    assert len(listed) == len(set(listed)), sorted(n for n in listed if listed.count(n) > 1)
    assert read and read == set(listed), (sorted(read - set(listed)), sorted(set(listed) - read))
