"""Helper of test_gpu_composite.test_hand_over_step_moves_no_result: traces composite_cases'
"layers" / "graze" batch in both arithmetics and stores the results.  Run as a child process,
because the library reads TURTLE_AMD_PARK once."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import turtle_amd as TA                      # noqa: E402

import composite_cases as CO                 # noqa: E402


def main(out_path, workdir):
    geo = CO.amd_geometry("layers", workdir)
    pos, d, _ = CO.graze("layers")
    out = {}
    for math in ("fast", "strict"):
        TA.set_math(math)
        t = geo["stepper"].trace(pos.copy(), d, max_steps=CO.GRAZE_MAX_STEPS)
        for k in ("position", "index", "length", "n_steps"):
            out[f"{math}_{k}"] = np.asarray(t[k])
    TA.set_math("fast")
    CO.destroy(geo)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
