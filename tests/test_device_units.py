"""The device layer is several translation units (turtle_amd/csrc/*.hip, the Makefile's DEV_SRC), and a
shared library links with a launcher missing: the failure would show at the first call only.  So every
function that internal.h declares for the device layer is a symbol the built library defines, and every
unit in the directory is one the Makefile builds."""
import ctypes
import glob
import os
import re

import turtle_amd as TA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "turtle_amd", "csrc")


def declared_device_functions():
    text = open(os.path.join(CSRC, "internal.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(tamd_(?:k|dev|scratch)_\w+)\s*\(", text))
    names -= {"tamd_dev_pool_stats"}  # (exists under -DTRACE_POOL_STATS only)
    return sorted(names)


def test_every_device_function_is_defined():
    names = declared_device_functions()
    # (the launchers of every unit are among them, and the thread runtime's calls)
    for n in ("tamd_k_trace", "tamd_k_elevation", "tamd_k_resample", "tamd_k_horizon", "tamd_k_advance",
              "tamd_dev_init", "tamd_scratch_reset"):
        assert n in names, n
    assert len(names) >= 58  # (what internal.h declares today: the parser has not gone blind)
    L = ctypes.CDLL(TA.library_path())
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, f"declared in internal.h, defined by no unit: {missing}"


def test_every_unit_is_built():
    make = open(os.path.join(CSRC, "Makefile")).read()
    built = re.search(r"^DEV_SRC\s*:=\s*(.*)$", make, flags=re.M).group(1).split()
    there = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(there) >= 2
    assert sorted(built) == there
