"""The hand-over list ordered by the library's own counting sort (TURTLE_AMD_SORT_OWN=1, the rule)
or by hipCUB's radix sort (=0): the rays reach the lined pass in the same order of keys, ties
apart, and no result depends on that order -- every output array of a trace of 4097 and of 100 003
rays is the same, bit for bit, over one map and over a 2 x 2 stack.  Each side in a child process
(the library reads its knobs once): tests/room_probe.py, a stepper a batch."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (4097, 100_003)
ARRAYS = ("position", "index", "length", "n_steps")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sort_own")
    children = []
    for knob in ("0", "1"):                      # (side by side: two processes on the GPU)
        out = os.path.join(tmp, f"own_{knob}.npz")
        env = dict(os.environ, TURTLE_AMD_SORT_OWN=knob)
        children.append((knob, out, subprocess.Popen(
            [sys.executable, os.path.join(HERE, "room_probe.py"), "fresh", out, os.path.join(tmp, f"work_{knob}"),
             ",".join(str(n) for n in SIZES)], env=env)))
    results = {}
    for knob, out, child in children:
        assert child.wait(timeout=300) == 0, knob
        with np.load(out) as z:
            results[knob] = {k: z[k].copy() for k in z.files}
    return results


@pytest.mark.parametrize("tag", ["map", "stack"])
@pytest.mark.parametrize("call", range(len(SIZES)))
def test_either_sort_changes_no_bit(runs, tag, call):
    for key in ARRAYS:
        own, cub = runs["1"][f"{tag}_{call}_{key}"], runs["0"][f"{tag}_{call}_{key}"]
        assert own.shape[0] == SIZES[call] and own.shape == cub.shape, key
        assert np.array_equal(own, cub), key
    # (the batch goes through the hand-over: rays beyond its 32 steps)
    assert runs["1"][f"{tag}_{call}_n_steps"].max() > 32
