"""Guards on the GENERATED code of the unbounded float32 match kernel (csrc/match32.hip) and of the template it was cut
from (csrc/match16.hip).  No GPU needed: hipcc cross-compiles, with the flags of tools/check_mfma_loops.py.

match32_kernel runs the MFMA step twice: one instance for whole tiles, one for the partial units of a launch's last
round.  What the whole-tile instance is there for can be read off its assembly - between the first and the last MFMA
of a step nothing branches, nothing goes through scratch, and the load counter is waited for once, where the source
says so: in front of the step's barrier.  match16.hip must not have moved: its 22 instantiations still give the rows of
profiles/match16_refactor_codegen.txt."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "kikuchipy_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists(HIPCC)), reason="needs hipcc")

BEGIN, END = "kpdi32 whole step begin", "kpdi32 whole step end"


def compile_kernels(source, tmp):
    """{kernel symbol: (body lines, metadata dict)} of one translation unit."""
    out = os.path.join(str(tmp), source.replace(".hip", ".s"))
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
                    "--cuda-device-only", os.path.join(CSRC, source), "-o", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lines = open(out).read().splitlines()
    bodies, name = {}, None
    for line in lines:
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            bodies[name] = []
        elif name:
            bodies[name].append(line)
    # the metadata: one entry per kernel under amdhsa.kernels, each opened by "  - ." and holding its keys at depth 4
    meta, entry = {}, None
    for line in lines + ["  - .end: 0"]:
        if re.match(r"^  - \.", line):
            if entry and entry.get("name") in bodies:
                meta[entry["name"]] = entry
            entry = {}
        m = re.match(r"^  (?:- |  )\.(\w+):\s+(\S+)\s*$", line)
        if m and entry is not None:
            entry[m.group(1)] = m.group(2)
    return {k: (bodies[k], meta.get(k, {})) for k in bodies if any("v_mfma" in l for l in bodies[k])}


def instructions(lines):
    """The instructions among `lines`: no comments, labels, directives or inline-asm brackets."""
    out = []
    for l in lines:
        t = l.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            out.append(t)
    return out


def mfma_span(lines):
    idx = [i for i, l in enumerate(lines) if "v_mfma" in l]
    return lines[idx[0]:idx[-1] + 1]


@pytest.fixture(scope="module")
def match32(tmp_path_factory):
    return compile_kernels("match32.hip", tmp_path_factory.mktemp("match32"))


@pytest.mark.parametrize("keep", [1, 8, 20, 32])
def test_whole_tile_step_has_no_branch_no_scratch_and_one_load_wait(match32, keep):
    names = [k for k in match32 if f"match32_kernelILi{keep}E" in k]
    assert len(names) == 1, sorted(match32)
    body = match32[names[0]][0]
    b = [i for i, l in enumerate(body) if BEGIN in l]
    e = [i for i, l in enumerate(body) if END in l]
    assert len(b) == 1 and len(e) == 1 and b[0] < e[0], (b, e)
    whole = body[b[0]:e[0]]
    rest = body[:b[0]] + body[e[0]:]
    n_whole = sum("v_mfma" in l for l in whole)
    # 3 k-steps x 4 elements x 16 accumulators in each instance of the step, and no MFMA anywhere else
    assert n_whole == 192 and sum("v_mfma" in l for l in rest) == 192
    span = instructions(mfma_span(whole))
    print(f"keep_n {keep}: {len(span)} instructions between the first and the last MFMA of the whole-tile step")
    assert not [t for t in span if re.match(r"s_(c?branch|setpc|call|swappc)", t)]
    assert not [t for t in span if "scratch_" in t]
    waits = [i for i, t in enumerate(span) if t.startswith("s_waitcnt") and "vmcnt" in t]
    barriers = [i for i, t in enumerate(span) if t.startswith("s_barrier")]
    assert len(waits) == 1 and len(barriers) == 1, [span[i] for i in waits + barriers]
    assert span[waits[0]].replace(" ", "") == "s_waitcntvmcnt(0)"
    # ... followed by the barrier: only waits in between, no MFMA and no memory instruction
    assert waits[0] < barriers[0] and all(t.startswith("s_waitcnt") for t in span[waits[0]:barriers[0]])
    # no accumulator and no fragment leaves its registers in either instance: nothing through scratch, no AGPR copy
    tail_in_one_piece = all("v_mfma" not in l for l in body[:b[0]]) or all("v_mfma" not in l for l in body[e[0]:])
    assert tail_in_one_piece, "the partial-unit step's MFMAs lie on both sides of the whole-tile step"
    for part in (whole, body[:b[0]] if any("v_mfma" in l for l in body[:b[0]]) else body[e[0]:]):
        inside = instructions(mfma_span(part))
        assert not [t for t in inside if "scratch_" in t or t.startswith("v_accvgpr")]


COLUMNS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
           "sgpr_spill_count", "group_segment_fixed_size")


def recorded_rows():
    """The right-hand table of profiles/match16_refactor_codegen.txt: {(KMAX, BOUNDED, WAVES, F32): 8 numbers}."""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "match16_refactor_codegen.txt")):
        m = re.match(r"^<\s*(\d+),\s*(\d),\s*(\d),\s*(\d)>(.*)\|(.*)$", line)
        if m:
            rows[tuple(int(m.group(i)) for i in range(1, 5))] = [int(v) for v in m.group(6).split()[:8]]
    return rows


def test_match16_still_generates_the_recorded_22_rows(tmp_path):
    want = recorded_rows()
    assert len(want) == 22
    got = {}
    for name, (body, meta) in compile_kernels("match16.hip", tmp_path).items():
        m = re.search(r"match16_kernelILi(\d+)ELb([01])ELi(\d)ELb([01])E", name)
        assert m, name
        span = len(instructions(mfma_span(body))) - 1  # (the record counts from behind the first MFMA to the last)
        got[tuple(int(v) for v in m.groups())] = [int(meta[c]) for c in COLUMNS] + [span]
    assert sorted(got) == sorted(want)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
