"""The flat first pass (device.hip, k_first): where run_trace's rule allows, a fast
trace over one map or one stack takes its first 32 closed-form steps in a flat kernel, a ray a lane,
instead of in the persistent k_trace.  Which kernel takes them changes no bit of any result and adds
the same to the device's totals: every batch here is traced with TURTLE_AMD_FIRST_PASS=0 (k_trace
everywhere) and =1, each in a child process (the library reads its knobs once), and every output
array and every field of trace_stats() must be EQUAL -- with the rays in the caller's order and in
the library's own (TURTLE_AMD_SPATIAL: results through RayOut), with the hand-over sorted and not
(TURTLE_AMD_SORT_KEY), with step caps far away, in the lined pass (40), just past the hand-over (33)
and at or below it (32, 20: the fallback), and for a second call that resumes the first one's rays."""
import os
import subprocess
import sys

import numpy as np
import pytest

import first_pass_probe as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = {f"spatial{s}_sortkey{k}": dict(TURTLE_AMD_SPATIAL=str(s), TURTLE_AMD_SORT_KEY=str(k))
           for s in (0, 1) for k in (0, 1)}
_pairs = {}


def _pair(tmp_path_factory, config):
    """(knob at 0, knob at 1) for one configuration: computed once, read by every test"""
    if config not in _pairs:
        tmp = tmp_path_factory.mktemp(f"first_pass_{config}")
        children = []
        for knob in ("0", "1"):   # (side by side: two processes on the GPU)
            out = os.path.join(tmp, f"first{knob}.npz")
            children.append((out, subprocess.Popen(
                [sys.executable, os.path.join(HERE, "first_pass_probe.py"), out,
                 os.path.join(tmp, f"work{knob}")],
                env=dict(os.environ, TURTLE_AMD_FIRST_PASS=knob, **CONFIGS[config]))))
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


@pytest.mark.parametrize("config", list(CONFIGS))
def test_the_kinds_of_ray_are_there(tmp_path_factory, config):
    """What the batches are mixed for, asserted on the knob-off result: rays that a crossing ends
    before the hand-over, rays that start outside the data, rays of thousands of steps, and --
    under a cap -- capped ones.  Equality below then says something."""
    off, _ = _pair(tmp_path_factory, config)
    n = P.SIZES[-1]
    kind = P.kind_of(n)
    for tag in ("map", "stack"):
        steps, medium = off[f"{tag}_n{n}_m100000_n_steps"], off[f"{tag}_n{n}_m100000_index"][:, 0]
        steep, rim, outside = (kind == P.KINDS.index(k) for k in ("steep", "rim", "outside"))
        counts = dict(
            steep_hit_before_32=int((steep & (medium == 0) & (steps > 0) & (steps < 32)).sum()),
            rim_left_before_32=int((rim & (medium == -1) & (steps > 0) & (steps < 32)).sum()),
            outside_at_origin=int(((medium == -1) & (steps == 0)).sum()),
            beyond_2000=int((steps > 2000).sum()))
        print(config, tag, counts, "max steps", int(steps.max()))
        assert counts["steep_hit_before_32"] > 0
        assert counts["rim_left_before_32"] > 0
        assert counts["outside_at_origin"] == int(outside.sum()) > 0
        assert counts["beyond_2000"] > 0
        for ms in (40, 33, 32, 20):
            key = f"{tag}_n{n}_m{ms}"
            capped = int(off[f"{key}_stats"][3])
            print(config, key, "capped", capped)
            # (a crossing located at its ms-th step is no capped ray)
            assert 0 < capped <= int((off[f"{key}_n_steps"] == ms).sum())


@pytest.mark.parametrize("max_steps", P.MAX_STEPS)
@pytest.mark.parametrize("n", P.SIZES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_first_pass_changes_no_bit(tmp_path_factory, config, n, max_steps):
    off, on = _pair(tmp_path_factory, config)
    for tag in ("map", "stack"):
        for call in ("", "_resumed"):
            key = f"{tag}_n{n}_m{max_steps}{call}"
            for name in P.ARRAYS + ("stats",):
                a, b = off[f"{key}_{name}"], on[f"{key}_{name}"]
                assert a.shape == b.shape and np.array_equal(a, b), (key, name)
            assert on[f"{key}_n_steps"].size == n
        # (the totals are those of the batch: nothing counted twice, nothing left out)
        key = f"{tag}_n{n}_m{max_steps}"
        rays, steps, _, _ = (int(x) for x in on[f"{key}_stats"])
        assert rays == n
        assert steps == int(on[f"{key}_n_steps"].sum())
