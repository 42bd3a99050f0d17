"""The tutorial's chain on one GPU, host-backed and resident; writes one JSON file (`--out`, default
profiles/resident_chain.json) and prints it.

The chain, at the tutorial's size (a 75 x 55 map of 60 x 60 uint8 patterns, a dictionary of `--dictionary` float32
patterns): remove_static_background -> remove_dynamic_background -> isig[5:55, 10:50] -> average_neighbour_patterns ->
get_image_quality -> dictionary_indexing (signal mask + navigation mask) -> get_image_quality.  Wall times per step,
host clock, best of `--reps` warm runs (the first run is the warm-up); a resident step ends at a device synchronise.
`h2d_mb`: what went over the host link during the whole chain (`Context.counters()["h2d_bytes"]`; downloads are not
counted there).  `select_kernel`: kpdi_select_patterns alone on the resident set, per kernel path of csrc/select_plan.h,
HIP events around the launch (profiling level 1), best of `--reps`, with the bytes it reads + writes.

Every GPU step (`--step host | resident | select`) runs in a process of its own under a time limit; the first one that
fails or runs out of time ends the measurement."""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAV, SIG = (55, 75), (60, 60)
STEPS = ("static", "dynamic", "isig", "average", "image_quality", "dictionary_indexing", "image_quality_2")


def inputs(n_dictionary):
    import kikuchipy_amd as kpa
    from kikuchipy_amd.signals import DictionaryXmap

    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, NAV + SIG, dtype=np.uint8)
    bg = rng.integers(1, 256, SIG, dtype=np.uint8)
    q = rng.standard_normal((n_dictionary, 4))
    dic = kpa.EBSD(rng.random((n_dictionary, 40, 50), dtype=np.float32),
                   xmap=DictionaryXmap(q / np.linalg.norm(q, axis=1)[:, None]))
    nav_mask = np.zeros(NAV, dtype=bool)
    nav_mask[:5] = True
    y, x = np.mgrid[:40, :50]
    sig_mask = (y - 19.5) ** 2 + (x - 24.5) ** 2 > 24.5 ** 2
    return data, bg, dic, nav_mask, sig_mask


def run_chain(resident, reps, n_dictionary):
    import kikuchipy_amd as kpa

    data, bg, dic, nav_mask, sig_mask = inputs(n_dictionary)
    runs, h2d = [], 0.0
    for _ in range(reps + 1):
        s = kpa.EBSD(data.copy(), static_background=bg, device=0)
        t0 = time.perf_counter()
        if resident:
            s.to_device()
        upload = time.perf_counter() - t0
        times, signals = {"to_device": upload}, [s]

        def timed(name, fn):
            t = time.perf_counter()
            out = fn()
            for sig in signals:
                if sig.is_resident:
                    sig.context.synchronize()
            times[name] = time.perf_counter() - t
            return out

        timed("static", lambda: s.remove_static_background())
        timed("dynamic", lambda: s.remove_dynamic_background())
        s2 = timed("isig", lambda: s.isig[5:55, 10:50])
        signals.append(s2)
        timed("average", lambda: s2.average_neighbour_patterns())
        timed("image_quality", lambda: s2.get_image_quality())
        timed("dictionary_indexing", lambda: s2.dictionary_indexing(dic, keep_n=20, navigation_mask=nav_mask,
                                                                    signal_mask=sig_mask, verbose=False))
        timed("image_quality_2", lambda: s2.get_image_quality())
        t = time.perf_counter()
        final = np.asarray(s2.data)
        times["data"] = time.perf_counter() - t
        times["chain"] = sum(times[k] for k in STEPS)
        h2d = sum(sig.context.counters()["h2d_bytes"] for sig in signals)
        runs.append(times)
        for sig in signals:
            sig._discard() if sig.is_resident else sig.close()
    best = {k: round(min(r[k] for r in runs[1:]) * 1e3, 3) for k in runs[0]}
    return {"ms": best, "h2d_mb": round(h2d / 1e6, 3), "patterns_mb": round(data.nbytes / 1e6, 3),
            "checksum": int(final.astype(np.int64).sum())}


def run_select(reps):
    from kikuchipy_amd import _lib

    rng = np.random.default_rng(0)
    m = NAV[0] * NAV[1]
    data = rng.integers(0, 256, (m,) + SIG, dtype=np.uint8)
    cases = {"whole (identity copy)": (None, None), "rows (isig[5:55, 10:50])": ((10, 1, 40), (5, 1, 50)),
             "strided (isig[::2, ::2])": ((0, 2, 30), (0, 2, 30))}
    out = {}
    with _lib.Context(0) as src, _lib.Context(0) as dst:
        src.set_problem(SIG[0], SIG[1], None, _lib.METRIC_NCC, 1)
        src.set_experimental(data)
        dst.set_profiling(1)
        for name, (rows, cols) in cases.items():
            ms = []
            for _ in range(reps + 1):
                before = dst.counters()["preproc_ms"]
                src.select_patterns(None, rows, cols, into=dst)
                ms.append(dst.counters()["preproc_ms"] - before)
            nr, nc = (SIG[0] if rows is None else rows[2]), (SIG[1] if cols is None else cols[2])
            moved = 2 * m * nr * nc
            best = min(ms[1:])
            out[name] = {"kernel_us": round(best * 1e3, 2), "bytes_read_and_written": moved,
                         "tb_per_s": round(moved / (best * 1e-3) / 1e12, 3) if best > 0 else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dictionary", type=int, default=20000)
    ap.add_argument("--step", choices=("host", "resident", "select"), default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_chain.json"))
    args = ap.parse_args()
    if args.step:
        res = run_select(args.reps) if args.step == "select" else run_chain(args.step == "resident", args.reps, args.dictionary)
        print("RESULT " + json.dumps(res))
        return
    from kikuchipy_amd import _lib

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    out = {"tool": "measure_resident_chain", "version": _lib.version(), "map": list(NAV), "patterns": list(SIG) + ["uint8"],
           "dictionary": [args.dictionary, 40, 50, "float32"], "reps": args.reps}
    for step, key in (("host", "host_backed"), ("resident", "resident"), ("select", "select_kernel")):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps),
                            "--dictionary", str(args.dictionary)], capture_output=True, text=True, timeout=args.limit)
        if p.returncode != 0:
            raise SystemExit(f"step {step} ended with status {p.returncode}:\n{p.stderr[-2000:]}")
        out[key] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["host_backed"]["checksum"] == out["resident"]["checksum"], "the two chains end in different patterns"
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
