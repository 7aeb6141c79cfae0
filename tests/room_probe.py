"""Helper of test_gpu_trace_room.py: batches of several sizes through one map and through a 2 x 2
stack, either all on ONE stepper per geometry ("shared": its scratch block is then larger than the
later calls) or each on a stepper of its own ("fresh").  Run as a child process, because the
library reads its knobs once.  The rays are those of scripts/exp_odd_sizes.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import turtle_amd as TA                      # noqa: E402
from turtle_amd import synth                 # noqa: E402

ARRAYS = ("position", "index", "length", "n_steps")


def main(mode, out_path, workdir, sizes):
    out = {}
    for tag in ("map", "stack"):
        if tag == "map":
            terrain = TA.Map.load(synth.write_hgt(os.path.join(workdir, "map"), 45, 3, 1201))
            box = ((45.0, 46.0), (3.0, 4.0))
        else:
            for la, lo in ((45, 3), (45, 4), (46, 3), (46, 4)):
                synth.write_hgt(os.path.join(workdir, "stack"), la, lo, 1201)
            terrain = TA.Stack(os.path.join(workdir, "stack"), 0)
            box = ((45.0, 47.0), (3.0, 5.0))

        def stepper():
            st = TA.Stepper()
            (st.add_map if tag == "map" else st.add_stack)(terrain, 0.0)
            return st

        shared = stepper() if mode == "shared" else None
        for call, n in enumerate(sizes):
            st = shared if shared is not None else stepper()
            lat, lon, az, el = synth.uniform_rays(n, box[0], box[1], seed=n, el_range=(-6.0, -0.3))
            pos, _ = st.position(lat, lon, 400.0)
            d = TA.ecef_from_horizontal(lat, lon, az, el)
            t = st.trace(pos.copy(), d)
            for k in ARRAYS:
                out[f"{tag}_{call}_{k}"] = np.asarray(t[k])
            if shared is not None and call == 1:
                # neither length nor n_steps asked for: the passes keep them in the stepper's own arrays
                t = st.trace(pos.copy(), d, want=())
                assert t["length"] is None and t["n_steps"] is None
                for k in ("position", "index"):
                    out[f"{tag}_bare_{k}"] = np.asarray(t[k])
            if shared is None:
                st.destroy()
        if shared is not None:
            shared.destroy()
        terrain.destroy()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3], [int(a) for a in sys.argv[4].split(",")])
