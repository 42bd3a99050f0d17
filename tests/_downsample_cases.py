"""Cases of the downsampling / dynamic-background fixture (tests/golden/downsample.npz, made by
tools/gen_downsample_golden.py): the inputs, rebuilt at test time from the existing fixtures and the seeded stacks of
tests/_iq_inputs.py, and what each one runs.  A fixture key is `ds__<input>__f<factor>__<dtype_out>` or
`bg__<input>__<case>__<dtype_out>`, with `same` for dtype_out=None."""

import os

import numpy as np

import _intensity_cases
import _iq_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = _intensity_cases.DTYPES
BASE = {"uint8": "uint8", "int8": "uint8", "uint16": "uint16", "int16": "uint16", "float32": "float32",
        "float64": "float32"}
SYNTH = {(120, 96): 4100, (64, 48): 4200}  # shape -> seed base


def special(dtype):
    """Four 16 x 16 float patterns: ordinary, one NaN pixel, constant, one +inf pixel."""
    y, x = np.mgrid[:16, :16]
    base = ((3 * y + 5 * x) % 23).astype(np.float64) * 7.25 - 40
    s = np.stack([base, base, np.full_like(base, 3.5), base])
    s[1, 4, 5] = np.nan
    s[3, 7, 3] = np.inf
    return s.astype(dtype)


def inputs():
    """name -> stack (n, sy, sx)."""
    out = {}
    pre = np.load(os.path.join(GOLDEN, "preproc.npz"))
    ni = pre["ni"]
    out["ni"] = ni.reshape((-1,) + ni.shape[-2:])
    dummy = np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]
    dummy = dummy.reshape((-1,) + dummy.shape[-2:])
    for dtype in DTYPES:
        out[f"dummy__{dtype}"] = _intensity_cases.as_dtype(dummy, dtype)
        out[f"degenerate__{dtype}"] = _intensity_cases.degenerate(dtype)
        for shape, seed in SYNTH.items():
            s = _iq_inputs.stack(shape, BASE[dtype], seed + DTYPES.index(dtype))
            out[f"rand{shape[0]}x{shape[1]}__{dtype}"] = _intensity_cases.as_dtype(s, dtype)
    for dtype in ("float32", "float64"):
        out[f"special__{dtype}"] = special(dtype)
    return out


CROSS_DTYPES = ("uint8", "int16", "float32")  # inputs that are binned into every other dtype
DS_STORED = 2  # patterns of a seeded stack stored per case (the fixture stays under 1 MB); other inputs: all


def stored(name):
    return DS_STORED if name.startswith("rand") else None


def downsample_cases():
    """(input name, factor, dtype_out or None) of every stored result."""
    cases = []
    for f in (2, 3, 4, 5, 6):
        cases.append(("ni", f, None))
    for d in DTYPES:
        cases.append(("ni", 2, d))
        cases.append(("ni", 5, d))
        cases.append((f"dummy__{d}", 3, None))
        for f in (2, 3, 4, 6, 8):
            cases.append((f"rand120x96__{d}", f, None))
        for f in (2, 4, 8, 16):
            cases.append((f"rand64x48__{d}", f, None))
        if d in CROSS_DTYPES:
            for d2 in DTYPES:
                if d2 != d:
                    cases.append((f"rand64x48__{d}", 2, d2))
        for f in (2, 4):
            cases.append((f"degenerate__{d}", f, None))
            cases.append((f"degenerate__{d}", f, "float32"))
    for d in ("float32", "float64"):
        for d2 in DTYPES:
            cases.append((f"special__{d}", 2, d2))
        cases.append((f"special__{d}", 4, None))
    return cases


BACKGROUND = {
    "frequency": {"filter_domain": "frequency"},
    "frequency_2_3": {"filter_domain": "frequency", "std": 2, "truncate": 3},
    "spatial": {"filter_domain": "spatial"},
    "spatial_2_3": {"filter_domain": "spatial", "std": 2, "truncate": 3},
}
BG_STORED = 1  # patterns stored per case (the fixture stays under 1 MB)
# Integer results in the frequency domain are held to "at most 1 level on at most 1e-3 of the values" against the
# reference's float32 FFT, whose own round-off (about 6e-5 on values near 100, 0.015 on uint16 values near 40 000)
# decides on which side of an integer a value lands.  The generator measures the float64 restatement against the
# reference (`bgdist__*`): the seeded uint16 / int16 stacks differ on 6.5e-4 to 2.7e-3 of their values, which leaves
# no room under the cap or exceeds it, so they run in the spatial domain only; every frequency case kept here differs
# on at most 8.2e-5 of its values.
FREQUENCY_DROPPED = ("uint16", "int16")


def background_cases():
    """(input name, case name, dtype_out or None)."""
    cases = []
    for c, kw in BACKGROUND.items():
        freq = kw["filter_domain"] == "frequency"
        cases.append(("ni", c, None))
        for d in ("int16", "uint16", "float32", "float64"):
            cases.append(("ni", c, d))
        for d in DTYPES:
            if not (freq and d in FREQUENCY_DROPPED):
                cases.append((f"rand64x48__{d}", c, None))
        for d in ("uint8", "float32"):
            cases.append((f"rand120x96__{d}", c, None))
        cases.append(("rand64x48__float32", c, "int16"))
        cases.append(("rand64x48__uint8", c, "float32"))
    return cases


def key(kind, name, what, dtype_out):
    what = f"f{what}" if kind == "ds" else what
    return f"{kind}__{name}__{what}__{dtype_out or 'same'}"
