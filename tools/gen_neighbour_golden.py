"""Write tests/golden/neighbours.npz by RUNNING THE REFERENCE ITSELF: its pattern/chunk.py
`_average_neighbour_patterns` (the NumPy evaluation, `.py_func`, which is what the shim runs) and its
signals/util/_map_helper.py `_get_neighbour_dot_product_matrices` / `_get_average_dot_product_map`, loaded unmodified
through oracle/ref_shim.py.  Test infrastructure; run it where the reference's sources are:

    /opt/conda/bin/python3.9 -W ignore tools/gen_neighbour_golden.py

Only data goes in: the windows (made by the reference's `Window`), the window sums, expected arrays, the numbers of the
reference's own tests (`known__*`) and `made_by`; the inputs are golden arrays and synthetic maps rebuilt at test time
(tests/_neighbour_cases.py).  The few set-up lines of the `EBSD` methods that need HyperSpy are written out here:
`window.reshape(shape + (1,))` for a 1-D window on a 2-D map and `window_sums = correlate(ones(nav_shape, int), window,
mode="constant")`, with SciPy's own correlate.

Averaging: every case of _neighbour_cases.AVERAGE_CASES.  For the non-integer window the share of pixels on which the
restatement (tests/_neighbour_restate.py) differs from the reference is recorded as `gauss__restate_share`.
Dot products: every case of DOT_CASES x FLAGS: the float64 evaluation (`g64`: the ADP path with dtype_out=float64; for
the matrices the reference's own `_map_helper(..., dtype_out=np.float64, output=<float64 array>)`) and the reference's
float32 results, which are asserted to meet the bound |f32 - g64| <= 1e-5 s that the GPU is held to.
"""

import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _neighbour_cases as cases  # noqa: E402
import _neighbour_restate as R  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

# the numbers of the reference's tests (tests/test_signals/test_ebsd.py:1522-1615, :2187-2340)
KNOWN_AVERAGE = {
    ("dummy", "default"): [
        255, 109, 218, 218, 36, 236, 255, 36, 0, 143, 111, 255, 159, 0, 207, 159, 63, 175, 135, 119, 34, 119, 0, 255, 153,
        119, 102, 182, 24, 255, 121, 109, 85, 133, 0, 12, 255, 107, 228, 80, 40, 107, 161, 147, 0, 204, 0, 51, 51, 51, 229,
        25, 76, 255, 194, 105, 255, 135, 149, 60, 105, 119, 0, 204, 102, 255, 89, 127, 0, 12, 140, 127, 255, 185, 0, 69, 162,
        46, 0, 208, 0],
    ("dummy", "rect23"): [
        255, 223, 223, 255, 0, 223, 255, 63, 0, 109, 145, 145, 200, 0, 255, 163, 54, 127, 119, 136, 153, 170, 0, 255, 153,
        136, 221, 212, 42, 255, 127, 0, 141, 184, 14, 28, 210, 45, 180, 135, 0, 255, 210, 15, 30, 200, 109, 182, 109, 0, 255,
        182, 145, 182, 150, 34, 255, 57, 81, 0, 57, 69, 11, 255, 38, 191, 63, 114, 38, 51, 89, 0, 255, 117, 137, 19, 117, 0,
        0, 176, 58],
    ("dummy", "gauss"): [
        218, 46, 255, 139, 0, 150, 194, 3, 11, 211, 63, 196, 145, 0, 255, 211, 33, 55, 175, 105, 155, 110, 0, 255, 169, 135,
        177, 184, 72, 255, 112, 59, 62, 115, 55, 0, 255, 51, 225, 107, 21, 122, 85, 47, 0, 255, 129, 152, 77, 0, 169, 48, 187,
        170, 153, 36, 255, 63, 86, 0, 57, 69, 4, 254, 45, 206, 58, 115, 16, 33, 98, 0, 255, 121, 117, 32, 121, 14, 0, 174,
        66],
    ("dummy", "w3"): [
        233, 106, 212, 233, 170, 233, 255, 21, 0, 191, 95, 255, 95, 0, 111, 143, 127, 159, 98, 117, 0, 117, 117, 255, 137,
        117, 117, 239, 95, 255, 223, 191, 175, 207, 31, 0, 155, 127, 255, 56, 0, 14, 70, 155, 85, 175, 111, 0, 143, 127, 255,
        95, 127, 191, 231, 0, 255, 162, 139, 139, 162, 23, 0, 135, 135, 255, 60, 105, 0, 60, 165, 105, 255, 127, 0, 127, 163,
        182, 109, 145, 109],
    ("dummy1d", "w3"): [
        255, 223, 223, 255, 0, 223, 255, 63, 0, 109, 145, 145, 200, 0, 255, 163, 54, 127, 119, 136, 153, 170, 0, 255, 153,
        136, 221],
}
KNOWN_ADP = {
    ("ni1d", "w3", True, True): [0.997470, 0.997457, 0.99744],
    ("ni", "default", True, True): [[0.995679, 0.996117, 0.997220], [0.996363, 0.996561, 0.997252],
                                    [0.995731, 0.996134, 0.997048]],
    ("ni", "rect33", True, True): [[0.995135, 0.995891, 0.997144], [0.995425, 0.996032, 0.997245],
                                   [0.995160, 0.995959, 0.997019]],
    ("ni", "default", False, True): [[0.999663, 0.999699, 0.999785], [0.999717, 0.999733, 0.999786],
                                     [0.999666, 0.999698, 0.999769]],
    ("ni", "default", True, False): [[6402544, 6398041.5, 6434939.5], [6411949.5, 6409170, 6464348],
                                     [6451061, 6456555.5, 6489456]],
}


def main():
    import scipy
    from scipy.ndimage import correlate

    ref = ref_shim.load_reference_projection()
    chunk = ref_shim._load("kikuchipy.pattern.chunk", "pattern/chunk.py")
    helper = ref_shim._load("kikuchipy.signals.util._map_helper", "signals/util/_map_helper.py")
    Window = ref["window"].Window

    def window(spec):
        spec = dict(spec)
        if isinstance(spec.get("window"), np.ndarray):
            return Window(spec["window"])
        return Window(window=spec.pop("window"), shape=spec.pop("window_shape", spec.pop("shape", None)), **spec)

    out = {"made_by": np.array(f"python {platform.python_version()}, scipy {scipy.__version__}, numpy {np.__version__}")}

    # ---- averaging
    share = {}
    for name, spec in cases.WINDOWS.items():
        out[f"win__{name}"] = np.asarray(window(spec), dtype=np.float64)
    for inp, win in cases.AVERAGE_CASES:
        data = cases.inputs(inp)
        nav = data.shape[:-2]
        w = np.asarray(out[f"win__{win}"])
        if len(nav) > w.ndim:
            w = w.reshape(w.shape + (1,))  # signals/ebsd.py:1024-1025
        sums = correlate(np.ones(nav, dtype=int), weights=w, mode="constant")  # signals/ebsd.py:1029-1033
        omin, omax = R.DTYPE_RANGE[data.dtype.type]
        got = chunk._average_neighbour_patterns(data, sums.reshape(sums.shape + (1, 1)), w.reshape(w.shape + (1, 1)),
                                                data.dtype, omin, omax)
        key = cases.avg_key(inp, win)
        assert got.dtype == data.dtype and got.shape == data.shape
        out[key] = got
        out[key + "__window_sums"] = sums.astype(np.int64)
        ours = R.average(data, out[f"win__{win}"])
        assert np.array_equal(R.window_sums(R.as_map(data, w)[1], *R.as_map(data, w)[0].shape[:2]).reshape(nav), sums), key
        if win in cases.INTEGER_WINDOWS:
            assert np.array_equal(ours, got), f"{key}: the restatement is not the reference"
        else:
            d = np.abs(ours.astype(np.int64) - got.astype(np.int64))
            assert d.max() <= 1, key
            share[key] = float((d != 0).mean())
        if (inp, win) in KNOWN_AVERAGE:
            known = np.array(KNOWN_AVERAGE[(inp, win)], dtype=np.uint8).reshape(data.shape)
            d = np.abs(known.astype(int) - got.astype(int)).max()
            assert d <= 1, (key, d)  # the reference's answers come from its fastmath build
            out["known__" + key] = known
        print(key, got.dtype, share.get(key, ""), flush=True)
    out["gauss__restate_share"] = np.array(max(share.values()))
    for k, v in share.items():
        out[k + "__restate_share"] = np.array(v)

    # ---- dot products
    worst = 0.0
    for inp, fpn in cases.DOT_CASES:
        data = cases.inputs(inp)
        nav = data.shape[:-2]
        spec = cases.FOOTPRINTS[fpn]
        if spec is None:
            w = Window(window="circular", shape=(3, 3)[:len(nav)])
        elif isinstance(spec, np.ndarray):
            w = Window(spec)
        else:
            w = window(spec)
        out[f"fp__{inp}__{fpn}"] = np.asarray(w) != 0
        sig_size = int(np.prod(data.shape[-2:]))
        for zm, nm in cases.FLAGS:
            key = cases.dot_key(inp, fpn, zm, nm)
            m32 = helper._get_neighbour_dot_product_matrices(data, w, 2, sig_size, zm, nm, np.dtype("float32"))
            a32 = helper._get_average_dot_product_map(data, w, 2, sig_size, zm, nm, np.dtype("float32"))
            a64 = helper._get_average_dot_product_map(data, w, 2, sig_size, zm, nm, np.dtype("float64"))
            # the matrices in float64: the reference's own helper with a float64 output array
            boolean_window, truthy, center = helper._setup_window_indices(window=w)
            m64 = np.full((int(np.prod(nav)), w.size), np.nan, dtype=np.float64)
            helper._map_helper(data, helper._neighbour_dot_products, window=boolean_window, nav_shape=nav,
                               dtype_out=np.float64, sig_size=sig_size, center_index=center,
                               flat_window_truthy_indices=truthy, zero_mean=zm, normalize=nm, output=m64)
            m64 = m64.reshape(nav + w.shape)
            assert m32.dtype == np.float32 and a32.dtype == np.float32 and a64.dtype == np.float64
            s_mat, s_map = cases.dot_scale(m64, nm)
            assert np.array_equal(np.isnan(m32), np.isnan(m64)) and np.array_equal(np.isnan(a32), np.isnan(a64)), key
            with np.errstate(invalid="ignore", divide="ignore"):
                e_mat = np.nanmax(np.where(s_mat > 0, np.abs(m32 - m64) / s_mat, np.abs(m32 - m64)))
                e_map = np.nanmax(np.where(s_map > 0, np.abs(a32 - a64) / s_map, np.abs(a32 - a64)))
            worst = max(worst, e_mat, e_map)
            assert e_mat <= cases.DOT_RTOL and e_map <= cases.DOT_RTOL, (key, e_mat, e_map)
            out[key + "__mat64"], out[key + "__adp64"], out[key + "__adp32"] = m64, a64, a32
            if (inp, fpn, zm, nm) in KNOWN_ADP:
                known = np.array(KNOWN_ADP[(inp, fpn, zm, nm)], dtype=np.float64)
                assert np.allclose(a32, known, atol=1e-5 * (1 if nm else float(s_map.max()))), key
                out["known__" + key] = known
            print(key, f"f32 vs f64: {e_mat:.3g} {e_map:.3g}", flush=True)
    out["dot__ref_f32_worst"] = np.array(worst)
    path = os.path.join(GOLDEN, "neighbours.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", out["made_by"], "gauss share", out["gauss__restate_share"])


if __name__ == "__main__":
    main()
