"""The declared staging of the batch calls (csrc/stage.c; host.h) on the CPU: stage.c linked against a
host-memory stub of the eight device calls it uses (tests/c/stage_stub.c), under AddressSanitizer and
UBSan.  The stub's arena refuses to grow once a piece is out, as the device layer's does, and counts
every call."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "turtle_amd", "csrc")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """scenario -> {counter: value}, from one run of the stub's scenarios"""
    exe = os.path.join(str(tmp_path_factory.mktemp("stage")), "stage_stub")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "c", "stage_stub.c"), os.path.join(CSRC, "stage.c"),
                           "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    out = {}
    for line in run.stdout.splitlines():
        name, *fields = line.split()
        out[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return out


def test_device_space_is_used_in_place(runs):
    """IN / OUT / INOUT / NULL arrays: nothing copied, nothing waited for, the user's own pointers"""
    r = runs["device"]
    assert r["bad"] == 0 and r["same"] == 1
    assert r["h2d"] + r["d2h"] + r["to_device"] + r["to_host"] == 0
    assert r["syncs"] == 0


@pytest.mark.parametrize("name", ["host_small", "host_edge", "host_empty"])
def test_small_host_call_goes_packed(runs, name):
    """inputs arrive, outputs return (bad == 0: the stub's kernel and the caller saw the right bytes; a
    NULL array stayed NULL), in ONE copy towards the host and ONE wait; the three non-NULL IN / INOUT
    arrays went in by queued copies.  host_edge: the last size the formula sends this way."""
    r = runs[name]
    assert r["bad"] == 0 and r["same"] == 0 and r["packed"] == 1
    assert r["to_host"] == 1 and r["d2h"] == 0 and r["syncs"] == 1
    assert r["to_device"] == 3 and r["h2d"] == 0
    assert r["refused"] == 0


@pytest.mark.parametrize("name", ["host_large", "host_edge1"])
def test_large_host_call_copies_array_by_array(runs, name):
    """the same data, one copy per array: three in (IN, INOUT, INOUT), three back (INOUT, OUT, INOUT);
    the NULL arrays are neither copied nor brought back.  host_edge1: one byte per array past the
    packed size."""
    r = runs[name]
    assert r["bad"] == 0 and r["same"] == 0 and r["packed"] == 0
    assert r["h2d"] == 3 and r["d2h"] == 3
    assert r["to_device"] + r["to_host"] == 0
    assert r["refused"] == 0


def test_most_arrays_of_one_byte_fit_the_arena(runs):
    """every piece takes 256 bytes of the arena whatever its size: the request is the sum of the
    pieces (the stub's arena has no slack), so none is refused; and one declaration past the bound
    fails at the open, before anything is copied"""
    r = runs["many"]
    assert r["bad"] == 0 and r["refused"] == 0
    assert r["arena"] == 256 * r["arrays"]
    assert r["to_host"] == 1 and r["syncs"] == 1
    assert r["over_fails"] == 1


def test_a_table_is_staged_in_either_space(runs):
    """a blob of the library's own (a map's one-grid view) is in the arena in DEVICE space too, where
    the user's arrays stay in place and the close still waits, before the arena is reused"""
    d, h = runs["table_device"], runs["table_host"]
    assert d["bad"] == 0 and d["same"] == 1
    assert d["h2d"] == 1 and d["d2h"] + d["to_device"] + d["to_host"] == 0 and d["syncs"] == 1
    assert h["bad"] == 0 and h["same"] == 0
    assert h["to_device"] == 2 and h["to_host"] == 1 and h["syncs"] == 1 and h["h2d"] + h["d2h"] == 0
