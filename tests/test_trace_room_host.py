"""The layout of a stepper's scratch block (csrc/trace_room.h) on the CPU: a stand-alone program
(tests/c/trace_room_stub.c) prints every region for a list of batch sizes, under AddressSanitizer and
UBSan; the header also has to compile as C++, which is how device.hip reads it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "turtle_amd", "csrc")
STUB = os.path.join(ROOT, "tests", "c", "trace_room_stub.c")

SIZES = [1, 63, 64, 65, 257, 4097, 100003, 12500000, 2147483646]
INT, DOUBLE, MIB = 4, 8, 1 << 20

# what each region is used for needs, in bytes, for a call of n rays
NEEDS = {
    "parked": lambda n: n * INT,             # the hand-over list; the sorts' first id buffer
    "cross_ray": lambda n: n * INT,          # L1 from the front, L2 from the far end: n in all
    "cross_other": lambda n: n * INT,
    "own_n_steps": lambda n: n * INT,
    "ids_alt": lambda n: n * INT,
    "keys": lambda n: n * 2,                 # a byte a ray (the hand-over), up to two (the spatial order)
    "keys_alt": lambda n: n * 2,
    "sort_temp": lambda n: 32 * MIB,         # TAMD_TRACE_SORT_TEMP
    "pos_s": lambda n: 3 * n * DOUBLE,
    "dir_s": lambda n: 3 * n * DOUBLE,
    "length_s": lambda n: n * DOUBLE,
    "index_s": lambda n: 2 * n * INT,
    "n_steps_s": lambda n: n * INT,
    "order": lambda n: n * INT,
    "tentative": lambda n: n * DOUBLE,
    "cross_ds": lambda n: n * DOUBLE,
    "own_length": lambda n: n * DOUBLE,
    "ds_mark": lambda n: n * DOUBLE,
}


def parent_bytes(n):
    """what tamd_stepper_scratch allocated before the layout had a header: 7 n ints, a pad, the sort's
    room and 72 bytes a ray, rounded up to 256, and 4 n doubles behind"""
    ints = (n * 7 * INT + 256 + 32 * MIB + n * 72 + 255) // 256 * 256
    return ints + n * 4 * DOUBLE


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """n -> {region: offset, ..., "bytes": total}"""
    exe = os.path.join(str(tmp_path_factory.mktemp("room")), "trace_room_stub")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-I" + CSRC, STUB, "-o", exe])
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I" + CSRC, STUB])
    run = subprocess.run([exe] + [str(n) for n in SIZES], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    out = {}
    for line in run.stdout.splitlines():
        fields = {k: int(v) for k, v in (f.split("=") for f in line.split())}
        n = fields.pop("n")
        out[n] = fields
    assert sorted(out) == SIZES
    return out


def test_every_region_is_named_here(layouts):
    for n, room in layouts.items():
        assert set(room) == set(NEEDS) | {"bytes"}, n


@pytest.mark.parametrize("n", SIZES)
def test_regions_are_aligned_disjoint_and_large_enough(layouts, n):
    """every region starts on a 256-byte boundary, holds what its use needs up to where the next
    one starts (or the block ends), and none overlaps another"""
    room = dict(layouts[n])
    total = room.pop("bytes")
    spans = sorted((at, at + NEEDS[name](n), name) for name, at in room.items())
    for at, end, name in spans:
        assert at % 256 == 0, name
        assert 0 <= at and end <= total, name
    for (_, end, name), (at, _, after) in zip(spans, spans[1:]):
        assert end <= at, (name, after)


def test_a_larger_batch_s_block_serves_a_smaller_one(layouts):
    totals = [layouts[n]["bytes"] for n in SIZES]
    assert totals == sorted(totals)


@pytest.mark.parametrize("n", SIZES)
def test_no_more_than_a_pad_per_region_over_the_old_block(layouts, n):
    assert layouts[n]["bytes"] <= parent_bytes(n) + 256 * len(NEEDS)
