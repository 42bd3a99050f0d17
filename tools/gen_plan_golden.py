"""Write tests/golden/plan_parent.npz: what `kpdi_plan_describe` of the library built in this tree answers over the grid
of tests/test_planner.py (MS x SHARES, the forms and keep_n of GOLDEN_SETS, k_kept = 3600) - every scalar field of
`kpdi_plan` and every launch descriptor.  Test infrastructure, host arithmetic only:

    python tools/gen_plan_golden.py

It was run on the commit BEFORE plan::sweep_plan replaced the three assemblies of a plan; test_planner.py holds every
later library to it.  Run it again only when a pull request changes what the planner decides on purpose."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_planner as tp  # noqa: E402
from kikuchipy_amd import _lib  # noqa: E402


def main():
    out = {"made_by": np.array(f"kpdi_plan_describe of {_lib.version()}"), "scalar_names": np.array(tp.SCALARS),
           "launch_names": np.array(tp.LAUNCH_FIELDS), "ms": np.array(tp.MS), "shares": np.array(tp.SHARES)}
    for form, keep_n in tp.GOLDEN_SETS:
        out[f"scalars__{form}__{keep_n}"], out[f"launches__{form}__{keep_n}"] = tp.plan_table(form, keep_n)
    np.savez_compressed(tp.GOLDEN, **out)
    print("wrote", tp.GOLDEN, os.path.getsize(tp.GOLDEN), "bytes;", out["made_by"])


if __name__ == "__main__":
    main()
