"""A context owns its events and streams (csrc/context.h: Event, Stream): closing it right after any of the lazily
created ones has come into being - with its work still queued, nothing synchronised, no counters read - leaves the
process as it found it.  What "as it found it" is measured by: the plain sweep of test_gpu_api.py's smallest case (the
dummy signal against itself) in a fresh context gives, bit for bit, the lists of a process that did nothing before, and
cycles of create / use / close do not eat device memory.

(A buffer left by a timed-out communicator self-test, freed by kpdi_destroy as well: not staged here - it takes a
communicator and a collective that hangs.)"""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden
from kikuchipy_amd import _lib

pytestmark = pytest.mark.gpu

SIDE, M, N, KEEP = 8, 64, 600, 5
# more row blocks of 256 patterns than the chip has compute units: no launch covers them all
M_SEVERAL_LAUNCHES = 257 * 256 + 40


def plain_sweep():
    """test_gpu_api.py's smallest case through one fresh context: (scores, indices)."""
    dummy = load_golden("di_dummy.npz")["dummy"].reshape(9, 3, 3)
    with _lib.Context(0) as c:
        c.set_problem(3, 3, None, _lib.METRIC_NCC, 9)
        c.set_experimental(dummy)
        c.push_dictionary_chunk(dummy, 0)
        return c.finalize(9)


@pytest.fixture(scope="module")
def untouched(tmp_path_factory):
    """The plain sweep in a process that did nothing before."""
    out = str(tmp_path_factory.mktemp("untouched") / "lists.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    g = np.load(out)
    return g["scores"], g["indices"]


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2026)
    return rng.integers(0, 256, (M, SIDE, SIDE), dtype=np.uint8), rng.random((N, SIDE, SIDE), dtype=np.float32)


def ready(c, exp, compute=_lib.COMPUTE_F32):
    c.set_problem(SIDE, SIDE, None, _lib.METRIC_NCC, KEEP, compute)
    c.set_experimental(exp)


# Each path leaves one group of lazily created resources behind, work still queued on them where the path allows it.
# The switches are the library's own (csrc/plan.h), read by set_problem: KPDI_UPLOAD_TILES cuts a host chunk into pieces
# of that many tiles of 128 patterns, KPDI_NO_COALESCE has a pushed chunk swept at once instead of waiting for company.

def pieces_of_a_host_chunk(c, env, exp, dic):
    """The copy stream, stage_filled[] and stage_free[]: 600 patterns as pieces of 256, 256 and 88."""
    env.setenv("KPDI_UPLOAD_TILES", "2")
    ready(c, exp)
    c.push_dictionary_chunk(dic, 0)


def chunk_left_pending(c, env, exp, dic):
    """pending.filled and pending.consumed[]: one small chunk swept by a finalize, the next one left waiting."""
    ready(c, exp)
    c.push_dictionary_chunk(dic[:300], 0)
    c.finalize(KEEP)
    c.push_dictionary_chunk(dic[300:], 300)


def result_not_collected(c, env, exp, dic):
    """The result stream, result_done and a slot's `ready`: finalize_async without finalize_wait."""
    ready(c, exp)
    c.push_dictionary_chunk(dic, 0)
    c.finalize_async(KEEP)


def float64_chunk_not_certified(c, env, exp, dic):
    """pend64.ready: the certification read-back of the one chunk swept in float64 is never looked at."""
    env.setenv("KPDI_NO_COALESCE", "1")
    ready(c, exp, _lib.COMPUTE_F64)
    c.push_dictionary_chunk(dic, 0)


def rotations_staged(c, env, exp, dic):
    """rot_stage[].copied: a chunk simulated on the device from rotations that went through the page-locked ring."""
    from oracle import kpdi_oracle as ko

    rng = np.random.default_rng(7)
    pc = (0.42, 0.78, 0.5)
    c.set_master_pattern(*rng.random((2, 41, 41)).astype(np.float32))
    c.set_detector(ko.gnomonic_bounds((SIDE, SIDE), pc), pc[2], SIDE, SIDE, ko.sample_to_detector_matrix(70.0, 0, 0, 0).T)
    c.set_direction_cosines(ko.detector_direction_cosines((SIDE, SIDE), pc))
    ready(c, exp)
    quat = rng.standard_normal((N, 4))
    c.push_rotations_chunk(quat / np.linalg.norm(quat, axis=1)[:, None], 0)


def sweep_of_several_launches(c, env, exp, dic):
    """stream2, ev_fork and ev_join: an experimental set no single launch covers."""
    assert _lib.plan_describe(M_SEVERAL_LAUNCHES, N, SIDE * SIDE, KEEP).launches > 1
    env.setenv("KPDI_NO_COALESCE", "1")
    c.set_problem(SIDE, SIDE, None, _lib.METRIC_NCC, KEEP)
    c.set_experimental(np.resize(exp, (M_SEVERAL_LAUNCHES, SIDE, SIDE)))
    c.push_dictionary_chunk(dic, 0)


def timed_pairs_not_drained(c, env, exp, dic):
    """Timed event pairs in every list a sweep fills (ev_fixed among them), the counters never read."""
    env.setenv("KPDI_NO_COALESCE", "1")
    c.set_profiling(1)
    ready(c, exp)
    c.push_dictionary_chunk(dic, 0)


PATHS = [pieces_of_a_host_chunk, chunk_left_pending, result_not_collected, float64_chunk_not_certified, rotations_staged,
         sweep_of_several_launches, timed_pairs_not_drained]


@pytest.mark.parametrize("path", PATHS, ids=lambda f: f.__name__)
def test_close_right_after_a_resource_came_into_being(path, data, untouched, monkeypatch):
    c = _lib.Context(0)
    try:
        with monkeypatch.context() as env:  # (the plain sweep below runs without the path's switches)
            path(c, env, *data)
    finally:
        c.close()  # no synchronize(), no counters()
    scores, indices = plain_sweep()
    assert scores.tobytes() == untouched[0].tobytes() and np.array_equal(indices, untouched[1])


def free_device_memory():
    """hipMemGetInfo's free bytes, asked of the HIP runtime libkpdi.so runs on.  (The call torch.cuda.mem_get_info wraps;
    torch itself brings a HIP runtime of its own, which finds no device in a process where the library's has the GPU open.)"""
    _lib.load()
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64" in line)
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert ctypes.CDLL(path).hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_create_use_close_does_not_accumulate(data):
    """Ten contexts, each with one profiled sweep whose counters nobody reads: device memory free after the last is not
    below what was free after the first (which absorbs the runtime's one-time allocations)."""
    exp, dic = data
    free = [free_device_memory()]
    for _ in range(10):
        with _lib.Context(0) as c:
            c.set_problem(SIDE, SIDE, None, _lib.METRIC_NCC, KEEP)
            c.set_experimental(exp)
            c.set_profiling(1)
            c.push_dictionary_chunk(dic, 0)
            c.finalize(KEEP)
        free.append(free_device_memory())
    print("free device memory, before and after each cycle:", free)
    assert free[-1] >= free[1], free


if __name__ == "__main__":  # the `untouched` fixture's process
    s, i = plain_sweep()
    np.savez(sys.argv[1], scores=s, indices=i)
