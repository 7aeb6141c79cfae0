"""A stepper's scratch block is laid out for the rays of the CALL (csrc/trace_room.h), whatever it
was allocated for: one stepper traces 4097 rays, then 257, then 1, then 4097 again -- the block of
the first call serves the others -- with every optional region of the block in use (the ray pool,
the ordered hand-over, the rays in spatial order forced on), and each result must equal, bit for
bit, the same batch on a fresh stepper with the three knobs at 0.  One map and a 2 x 2 stack; each
side in a child process (the library reads its knobs once)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (4097, 257, 1, 4097)
ARRAYS = ("position", "index", "length", "n_steps")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("trace_room")
    children = []
    for mode, knob in (("shared", "1"), ("fresh", "0")):   # (side by side: two processes on the GPU)
        out = os.path.join(tmp, f"{mode}.npz")
        env = dict(os.environ, TURTLE_AMD_POOL=knob, TURTLE_AMD_SORT_KEY=knob, TURTLE_AMD_SPATIAL=knob)
        children.append((mode, out, subprocess.Popen(
            [sys.executable, os.path.join(HERE, "room_probe.py"), mode, out, os.path.join(tmp, f"work_{mode}"),
             ",".join(str(n) for n in SIZES)], env=env)))
    results = {}
    for mode, out, child in children:
        assert child.wait(timeout=300) == 0, mode
        with np.load(out) as z:
            results[mode] = {k: z[k].copy() for k in z.files}
    return results


@pytest.mark.parametrize("tag", ["map", "stack"])
def test_a_block_larger_than_the_call_changes_no_bit(runs, tag):
    for call, n in enumerate(SIZES):
        for key in ARRAYS:
            got, ref = runs["shared"][f"{tag}_{call}_{key}"], runs["fresh"][f"{tag}_{call}_{key}"]
            assert got.shape[0] == n and got.shape == ref.shape, (call, n, key)
            assert np.array_equal(got, ref), (call, n, key)
    # (the batch goes through the lists: rays beyond the hand-over's 32 steps)
    assert runs["fresh"][f"{tag}_0_n_steps"].max() > 32


@pytest.mark.parametrize("tag", ["map", "stack"])
def test_a_call_that_asks_for_neither_length_nor_n_steps(runs, tag):
    """the passes then keep both in the block's own arrays: the same positions and media as the call
    that asked for both (the 257 rays, on the block of 4097)"""
    for key in ("position", "index"):
        assert np.array_equal(runs["shared"][f"{tag}_bare_{key}"], runs["shared"][f"{tag}_1_{key}"]), key
