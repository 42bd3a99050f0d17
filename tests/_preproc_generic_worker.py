"""Worker of tests/test_gpu_preproc_kernels.py: the cases of _preproc_cases.GENERIC on GPU 0 with the generic correlation
loop in place of the unrolled forms.  The launcher reads $KPDI_PRE_GENERIC once per process, so the setting gets a fresh
process; the outputs go, one after the other and flattened, into the .npy named on the command line:

    KPDI_PRE_GENERIC=1 python tests/_preproc_generic_worker.py out.npy
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def run(ctx, c, patterns, bg):
    """The recorded steps of case `c` on `patterns`, then the read-back that runs them: one launch per kernel."""
    from kikuchipy_amd import _lib

    op = {"subtract": _lib.OP_SUBTRACT, "divide": _lib.OP_DIVIDE}[c.op]
    ctx.set_problem(c.shape[0], c.shape[1], None, _lib.METRIC_NCC, 1)
    ctx.set_experimental(patterns)
    record(ctx, c, bg, op)
    return ctx.get_experimental()


def record(ctx, c, bg, op):
    from kikuchipy_amd import _lib

    if c.static:
        ctx.remove_static_background(np.asarray(bg).astype(np.float32), op, c.scale_bg)
    if c.dynamic:
        ctx.remove_dynamic_background(op, {"frequency": _lib.DOMAIN_FREQUENCY, "spatial": _lib.DOMAIN_SPATIAL}[c.domain],
                                      c.std, c.truncate)


def main(path):
    assert os.environ.get("KPDI_PRE_GENERIC"), "the worker is the KPDI_PRE_GENERIC side of the comparison"
    for d in (ROOT, HERE):
        if d not in sys.path:
            sys.path.insert(0, d)
    import _preproc_cases as C
    from kikuchipy_amd import _lib

    out = []
    with _lib.Context(0) as ctx:
        for c in C.GENERIC:
            out.append(run(ctx, c, *C.inputs(c)).ravel())
    np.save(path, np.concatenate(out))


if __name__ == "__main__":
    main(sys.argv[1])
