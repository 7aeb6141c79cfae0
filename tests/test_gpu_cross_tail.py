"""The crossings under the tail (device.hip, CrossTail): the lined pass lists a
trace's crossings in two parts and its own waves locate the first while the batch's longest rays go
on; k_cross takes what is left.  Which kernel locates a crossing changes no bit of it and adds the
same to the device's totals: every case here runs with TURTLE_AMD_CROSS_TAIL=0 (one list, all of it
k_cross's) and =1, each in a child process (the library reads its knobs once), through one map and
through a one-tile stack, and every output array and trace_stats() must be EQUAL."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ARRAYS = ("position", "index", "length", "n_steps")
SIZES = (1, 63, 64, 65, 4097)
# what a child process traces, per setting of the other knobs that choose the lined pass's instance
# and where its results go: the block's ray pool (the pooled kernel), the rays in the order of
# where they start (results through RayOut)
CONFIGS = {
    "default": (dict(), ["probe"] + [f"n{n}" for n in SIZES] + ["steep", "capped"]),
    "pool": (dict(TURTLE_AMD_POOL="1"), ["probe"]),
    "spatial": (dict(TURTLE_AMD_SPATIAL="1"), ["probe"]),
}
_pairs = {}


def _pair(tmp_path_factory, config):
    """(knob at 0, knob at 1) for one configuration: computed once, read by every test"""
    if config not in _pairs:
        env, names = CONFIGS[config]
        tmp = tmp_path_factory.mktemp(f"cross_tail_{config}")
        children = []
        for knob in ("0", "1"):   # (side by side: two processes on the GPU)
            out = os.path.join(tmp, f"tail{knob}.npz")
            children.append((out, subprocess.Popen(
                [sys.executable, os.path.join(HERE, "cross_tail_probe.py"), out,
                 os.path.join(tmp, f"work{knob}"), ",".join(names)],
                env=dict(os.environ, TURTLE_AMD_CROSS_TAIL=knob, **env))))
        results = []
        for out, child in children:
            assert child.wait(timeout=300) == 0
            with np.load(out) as z:
                results.append({k: z[k].copy() for k in z.files})
        for r in results:
            for a in r.values():
                a.setflags(write=False)
        _pairs[config] = tuple(results)
    return _pairs[config]


def _same(off, on, name):
    for tag in ("map", "stack"):
        for key in ARRAYS + ("stats",):
            a, b = off[f"{name}_{tag}_{key}"], on[f"{name}_{tag}_{key}"]
            assert a.shape == b.shape and np.array_equal(a, b), (name, tag, key)
        # (the totals are those of the batch: nothing counted twice, nothing left out)
        rays, steps, _, _ = (int(x) for x in on[f"{name}_{tag}_stats"])
        assert rays == on[f"{name}_{tag}_n_steps"].size
        assert steps == int(on[f"{name}_{tag}_n_steps"].sum())


@pytest.mark.parametrize("config", list(CONFIGS))
def test_probe_batch(tmp_path_factory, config):
    """creep_probe.py's batch, 40 000 shallow rays over a 1201^2 tile: crossings on both lists,
    rays of thousands of steps that end long after the first list is final.  Also with the block's
    ray pool forced on (the pooled kernel keeps one list: k_cross must then take all of it, told to
    look for two) and with the rays in the order of where they start (the results go to the caller's
    arrays through RayOut)."""
    off, on = _pair(tmp_path_factory, config)
    assert off["probe_map_n_steps"].max() > 2000 and off["probe_stack_n_steps"].max() > 2000
    _same(off, on, "probe")


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes_around_a_ticket(tmp_path_factory, n):
    """One ray, one short of a ticket of 64 entries, a ticket, one more, and 4 097: no multiple of
    the ticket and far below the grid, so most waves find the queue dry with nothing in hand."""
    off, on = _pair(tmp_path_factory, "default")
    assert off[f"n{n}_map_n_steps"].size == n
    _same(off, on, f"n{n}")


def test_batch_that_ends_in_phase_a(tmp_path_factory):
    """Rays at -60 degrees: all of them cross within phase A's closed-form steps, the lined pass
    starts with an empty queue and the whole list is located by its waves."""
    off, on = _pair(tmp_path_factory, "default")
    for tag in ("map", "stack"):
        assert off[f"steep_{tag}_n_steps"].max() < 32         # the hand-over's step count
        assert (off[f"steep_{tag}_index"][:, 0] == 0).all()   # every ray hit the ground
    _same(off, on, "steep")


def test_batch_without_a_crossing(tmp_path_factory):
    """Every ray stops at max_steps = 40, past the hand-over and before any boundary: both lists
    stay empty and the tickets take nothing."""
    off, on = _pair(tmp_path_factory, "default")
    for tag in ("map", "stack"):
        assert (off[f"capped_{tag}_n_steps"] == 40).all()
        assert int(off[f"capped_{tag}_stats"][3]) == off[f"capped_{tag}_n_steps"].size
    _same(off, on, "capped")
