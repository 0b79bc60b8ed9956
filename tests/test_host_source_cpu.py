"""Source invariants of the host layer of libdsea (read from the sources: no build, no GPU).  One HIP error path: the
slot behind dsea_last_hip_error() is written by one function, and every hipGetLastError() of the two host files goes
through it or is discarded on purpose.  One CG polling loop, and one predicate for the fused Lanczos tail."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "dominantsparseeigenad_amd", "csrc")
HOST_FILES = ("dsea_capi.hip", "dsea_partitioned.hip")


def sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    return {os.path.basename(p): open(p).read() for p in paths}


def test_the_last_hip_error_is_recorded_by_one_function():
    src = sources()
    assert all(name in src for name in HOST_FILES)
    slot = re.search(r"int dsea_last_hip_error\(void\)\s*\{\s*return (\w+);", src["dsea_capi.hip"]).group(1)
    # assignments to the slot (its declaration, `int slot = 0;`, is not one)
    writes = [(name, m.start()) for name, text in src.items()
              for m in re.finditer(r"(?<!int )\b%s\s*=(?!=)" % slot, text)]
    assert len(writes) == 1, writes
    name, at = writes[0]
    setter = re.search(r"\nint (\w+)\(hipError_t \w+\) \{.*?\n\}", src[name], re.S)
    assert setter and setter.start() < at < setter.end(), "%s is written outside its setter" % slot
    assert setter.group(1) == "hip_fail"


def test_every_hip_last_error_goes_through_the_setter_or_is_discarded():
    src = sources()
    for name in HOST_FILES:
        text = src[name]
        calls = [m.start() for m in re.finditer(r"hipGetLastError\(\)", text)]
        allowed = [m.start() + len(m.group(1)) for m in re.finditer(r"(\(void\)|hip_fail\()hipGetLastError\(\)", text)]
        assert sorted(calls) == sorted(allowed), "%s: a hipGetLastError() that neither records nor discards" % name


def test_one_cg_polling_loop():
    hits = {name: text.count("< poll_every ?") for name, text in sources().items()}
    assert sum(hits.values()) == 1, {k: v for k, v in hits.items() if v}


def test_one_fused_tail_predicate():
    defs = [(name, m.group(0)) for name, text in sources().items()
            for m in re.finditer(r"\bbool\s+has_fused_tail\s*[(=]", text)]
    assert len(defs) == 1 and defs[0][1].endswith("("), defs
