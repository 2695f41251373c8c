"""The host files of csrc/host/ and the list of them in csrc/voxcarve.hip: the Makefile takes whatever lies in host/ as a
dependency, so a stale or forgotten file there would ride along unnoticed."""
import os
import re

import fixtures_util as fx

HIP = os.path.join(fx.ROOT, "voxel-based-3d-reconstruction_amd", "csrc")


def _host_files():
    return sorted(f for f in os.listdir(os.path.join(HIP, "host")) if not f.startswith("."))


def test_every_host_file_is_included_exactly_once():
    top = open(os.path.join(HIP, "voxcarve.hip")).read()
    included = re.findall(r'^#include "host/([^"]+)"', top, re.M)
    assert sorted(included) == _host_files()          # (a file named twice, or one that is missing on either side, differs here)
    assert all(re.fullmatch(r"\w+\.h", f) for f in included)


def test_no_host_file_includes_anything():
    for f in _host_files():
        src = open(os.path.join(HIP, "host", f)).read()
        assert not re.search(r"^\s*#\s*include\b", src, re.M), f
