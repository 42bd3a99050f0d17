"""The cases of tests/test_gpu_preproc_kernels.py: background removal through every kernel form of csrc/preproc.hip,
compared bit for bit with tests/_preproc_restate.py.  Every case names the kernel form it must reach; `form()` restates
the launcher's rules and tests/test_host_preproc.py holds each case to its form and the restated rules to the source, so
that a changed threshold fails on the CPU instead of silently moving a case to another kernel."""

import itertools
from collections import namedtuple

import numpy as np

from _downsample_restate import DTYPE_RANGE

# ---- the launcher's rules (csrc/preproc.hip; the quoted text is what tests/test_host_preproc.py looks for there) -------
PP_THREADS = 256
LAUNCHER_RULES = (
    # fused_lds_bytes: the pattern + the transposed intermediate with an odd row pitch, float32
    "const size_t npix4 = ((size_t)sy * sx + 3) & ~(size_t)3;",
    "return (npix4 + (size_t)sx * (sy | 1)) * 4;",
    # fused_threads
    "return fused_lds_bytes(sy, sx) > 80 * 1024 ? 1024 : PP_THREADS;",
    # preprocess_fits_fused
    "return fused_lds_bytes(sy, sx) <= 150 * 1024 &&",
    # launch_pre_t: the NT selection of the fused kernel ...
    "const int nt = (!l.do_dynamic || generic_only) ? 0 : (l.ntaps == 30 ? 30 : (l.ntaps == 60 ? 60 : 0));",
    "auto kernel = threads == 1024 ? (nt == 60 ? KPDI_PRE_PICK(60, 1024) : KPDI_PRE_PICK(0, 1024))",
    ": (nt == 30 ? KPDI_PRE_PICK(30, PP_THREADS) : KPDI_PRE_PICK(0, PP_THREADS));",
    # ... and of the streaming kernels
    "if (l.ntaps == 60 && !getenv(\"KPDI_PRE_GENERIC\"))",
    "const int grid = (int)std::min<int64_t>(n, 512);",
    "constexpr int PP_THREADS = PREP_THREADS;",
)


def fused_lds_bytes(sy, sx):
    npix4 = (sy * sx + 3) & ~3
    return (npix4 + sx * (sy | 1)) * 4


def fused_threads(sy, sx):
    return 1024 if fused_lds_bytes(sy, sx) > 80 * 1024 else PP_THREADS


def fits_fused(sy, sx):
    return fused_lds_bytes(sy, sx) <= 150 * 1024


def window(c):
    """(ntaps, reflect) of a case's dynamic step: gaussian_taps of csrc/pattern_ops.hip."""
    std = c.std if c.std > 0 else c.shape[1] / 8.0
    if c.domain == "frequency":
        return int(c.truncate * std), False
    return 2 * int(c.truncate * std + 0.5) + 1, True


def form(c, generic=False):
    """The kernels a case runs, from the launcher's rules: a tuple of names.  `generic`: with KPDI_PRE_GENERIC set."""
    sy, sx = c.shape
    ntaps, reflect = window(c) if c.dynamic else (0, False)
    boundary = "reflect" if reflect else "edge"
    if fits_fused(sy, sx):
        threads = fused_threads(sy, sx)
        nt = 0
        if c.dynamic and not generic:
            nt = ntaps if (threads, ntaps) in ((PP_THREADS, 30), (1024, 60)) else 0
        return (f"fused/{threads}/NT{nt}" + (f"/{boundary}" if c.dynamic else ""),)
    out = ()
    if c.static:
        out += ("static_stream",)
    if c.dynamic:
        out += (f"dynamic_stream/NT{60 if ntaps == 60 and not generic else 0}/{boundary}",)
    return out


def stream_grid(n):
    return min(n, 512)


# ---- the case table -------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name shape dtype static dynamic op scale_bg domain std truncate n form")


def case(name, shape, want, dtype=np.uint8, static=False, dynamic=True, op="subtract", scale_bg=False,
         domain="frequency", std=0.0, truncate=4.0, n=3):
    return Case(name, shape, np.dtype(dtype), static, dynamic, op, scale_bg, domain, std, truncate, n, want)


# shape / window cases: the smallest shapes that reach each form (dynamic only, subtract; VARIANTS below repeats them)
WINDOWS = [
    case("60x60", (60, 60), ("fused/256/NT30/edge",)),
    case("47x61-odd", (47, 61), ("fused/256/NT30/edge",)),                      # odd pixel count, 47 % 16 != 0
    case("20x20-std7.5", (20, 20), ("fused/256/NT30/edge",), std=7.5),          # 30 taps on 20 pixels, unrolled
    case("24x20-10taps", (24, 20), ("fused/256/NT0/edge",)),
    case("24x20-11taps", (24, 20), ("fused/256/NT0/edge",), std=2.75),          # the other parity of the centre
    case("24x20-2taps", (24, 20), ("fused/256/NT0/edge",), std=0.5),
    case("24x20-1tap", (24, 20), ("fused/256/NT0/edge",), std=0.25),            # identity window: y constant, 0 / 0
    case("60x120-60taps", (60, 120), ("fused/256/NT0/edge",)),                  # 60 taps, 256 threads: generic loop
    # (uint16: the edge taps of SciPy's window, 5e-5 and 2e-5 of the sum, move no uint8 grey level - a dropped one would pass)
    case("24x20-spatial", (24, 20), ("fused/256/NT0/reflect",), dtype=np.uint16, domain="spatial"),          # r = 10
    case("12x9-spatial-r32", (12, 9), ("fused/256/NT0/reflect",), dtype=np.uint16, domain="spatial", std=8.0),  # beyond two periods
    case("86x120", (86, 120), ("fused/1024/NT60/edge",)),
    case("104x100-50taps", (104, 100), ("fused/1024/NT0/edge",)),
    case("139x138-last-fused", (139, 138), ("fused/1024/NT0/edge",)),           # odd quad count: scalar loads
    case("140x138-first-stream", (140, 138), ("dynamic_stream/NT0/edge",)),
    case("162x120-stream60", (162, 120), ("dynamic_stream/NT60/edge",)),        # never run before these tests
    case("141x140-stream70", (141, 140), ("dynamic_stream/NT0/edge",)),
]
STATIC_STREAM = case("162x120-static", (162, 120), ("static_stream",), static=True, dynamic=False)


def variants(c):
    """Both operations x (static only, dynamic only, both) x scale_bg where there is a static step."""
    out = []
    for op, (st, dy) in itertools.product(("subtract", "divide"), ((True, False), (False, True), (True, True))):
        for sc in ((False, True) if st else (False,)):
            steps = ("static" if st else "") + ("+" if st and dy else "") + ("dynamic" if dy else "")
            v = c._replace(name=f"{c.name}-{steps}-{op}" + ("-scale" if sc else ""), static=st, dynamic=dy, op=op, scale_bg=sc)
            out.append(v._replace(form=form(v)))
    return out


def _all_variants():
    seen, out = set(), []
    for c in WINDOWS:
        for v in variants(c):
            # static only does not see the window: once per shape
            key = (v.shape, v.op, v.scale_bg) if not v.dynamic else v.name
            if key not in seen:
                seen.add(key)
                out.append(v)
    return out


VARIANTS = _all_variants()

DTYPES = (np.uint8, np.int8, np.uint16, np.int16, np.float32, np.float64)
# every dtype: both operations and both domains at (24, 20), once more at (60, 60) default, after a static step
DTYPE_CASES = [
    case(f"{np.dtype(dt).name}-24x20-{op}-{dom}", (24, 20), ("fused/256/NT0/" + ("edge" if dom == "frequency" else "reflect"),),
         dtype=dt, static=True, op=op, domain=dom)
    for dt in DTYPES for op in ("subtract", "divide") for dom in ("frequency", "spatial")
] + [case(f"{np.dtype(dt).name}-60x60", (60, 60), ("fused/256/NT30/edge",), dtype=dt, static=True) for dt in DTYPES]

# the persistent loop of dynamic_stream_kernel: 516 patterns on a grid of 512, pattern j = pattern j % 3
PERSISTENT = case("162x120-persistent", (162, 120), ("dynamic_stream/NT60/edge",), n=516)
PERSISTENT_BASE = 3

# what the child process of the unrolled-against-generic test runs with KPDI_PRE_GENERIC=1
GENERIC = [c for c in WINDOWS if c.name in ("60x60", "47x61-odd", "20x20-std7.5", "86x120", "162x120-stream60")]

ALIGNMENT = [case("u8-60x60-offset", (60, 60), ("fused/256/NT30/edge",), static=True),
             case("u16-60x60-offset", (60, 60), ("fused/256/NT30/edge",), dtype=np.uint16, static=True)]

ALL_EXACT = WINDOWS + [STATIC_STREAM] + VARIANTS + DTYPE_CASES + [PERSISTENT] + ALIGNMENT


def inputs(c, n=None):
    """(patterns (n, sy, sx), static background (sy, sx)) of a case: seeded by its shape, dtype and operation, with
    values over the whole range of the dtype - strictly positive where something divides."""
    n = c.n if n is None else n
    seed = [c.shape[0], c.shape[1], DTYPES.index(c.dtype.type), c.op == "divide"]
    rng = np.random.default_rng(seed)
    lo, hi = DTYPE_RANGE[c.dtype.type]
    positive = c.op == "divide"
    if c.dtype.kind == "f":
        def draw(shape):
            v = rng.random(shape) * 999.0 + 1.0 if positive else rng.random(shape) * 2000.0 - 1000.0
            return v.astype(c.dtype)
    else:
        def draw(shape):
            return rng.integers(1 if positive else lo, hi + 1, shape).astype(c.dtype)
    return draw((n,) + c.shape), draw(c.shape)


def restate_kwargs(c):
    return dict(static=c.static, dynamic=c.dynamic, operation=c.op, scale_bg=c.scale_bg, filter_domain=c.domain,
                std=c.std, truncate=c.truncate)


# ---- degenerate patterns --------------------------------------------------------------------------------------------
Degenerate = namedtuple("Degenerate", "name dtype static dynamic op scale_bg domain plant")
# plant(patterns, bg) edits pattern 1 of 3 (and the background) in place; patterns 0 and 2 stay healthy
PIX = (5, 7)


def _dead_pixel(p, bg):
    p[1][PIX] = 0
    bg[PIX] = 0


def _zero_background(p, bg):
    bg[PIX] = 0


def _equals_background(p, bg):
    p[1] = bg


def _constant_background(p, bg):
    bg[...] = 9


def _constant_pattern(p, bg):
    p[1] = 100


def _one(value):
    def plant(p, bg):
        p[1][PIX] = value
    return plant


def _deg(name, dtype, plant, static=False, dynamic=False, op="subtract", scale_bg=False, domain="frequency"):
    return Degenerate(name, np.dtype(dtype), static, dynamic, op, scale_bg, domain, plant)


DEGENERATES = [
    _deg("dead-pixel-divide", np.uint8, _dead_pixel, static=True, op="divide"),            # 0 / 0: all 0
    _deg("x-over-0", np.uint8, _zero_background, static=True, op="divide"),                # inf: range inf, all 0
    _deg("x-over-0-int16", np.int16, _zero_background, static=True, op="divide"),          # finite pixels: omin; inf: 0
    _deg("equals-background", np.uint8, _equals_background, static=True),                  # constant y: 0 / 0
    _deg("constant-background-scaled", np.uint8, _constant_background, static=True, scale_bg=True),
    _deg("constant-frequency", np.uint8, _constant_pattern, dynamic=True),
    _deg("constant-spatial", np.uint8, _constant_pattern, dynamic=True, domain="spatial"),
    _deg("constant-spatial-divide-f32", np.float32, _constant_pattern, dynamic=True, op="divide", domain="spatial"),
    _deg("nan-f32-frequency", np.float32, _one(np.nan), dynamic=True),
    _deg("nan-f32-spatial", np.float32, _one(np.nan), dynamic=True, domain="spatial"),
    _deg("nan-f32-static", np.float32, _one(np.nan), static=True, scale_bg=True),
    _deg("nan-f64-frequency", np.float64, _one(np.nan), dynamic=True, op="divide"),
    _deg("nan-f64-static+dynamic", np.float64, _one(np.nan), static=True, dynamic=True),
    _deg("inf-f32-frequency", np.float32, _one(np.inf), dynamic=True),
    _deg("inf-f32-spatial", np.float32, _one(np.inf), dynamic=True, domain="spatial", op="divide"),
    _deg("inf-f64-frequency", np.float64, _one(np.inf), dynamic=True),
    _deg("inf-f64-static", np.float64, _one(np.inf), static=True),
]
DEGENERATE_SHAPES = {"fused": (24, 20), "stream": (140, 138)}


def degenerate_case(d, where):
    shape = DEGENERATE_SHAPES[where]
    c = case(f"{d.name}-{where}", shape, None, dtype=d.dtype, static=d.static, dynamic=d.dynamic, op=d.op,
             scale_bg=d.scale_bg, domain=d.domain)
    return c._replace(form=form(c))


def degenerate_inputs(d, where):
    p, bg = inputs(degenerate_case(d, where))
    p, bg = p.copy(), bg.copy()
    d.plant(p, bg)
    return p, bg
