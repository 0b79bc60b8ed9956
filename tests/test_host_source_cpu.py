"""Source invariants of the host layer of libdsea (read from the sources: no build, no GPU).  One HIP error path: the
slot behind dsea_last_hip_error() is written by one function, and every hipGetLastError() of the two host files goes
through it or is discarded on purpose.  One CG polling loop, and one predicate for the fused Lanczos tail.  The launchers: one
dispatch rule per kernel family and each grid rule once."""
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


# ---- the launch wrappers: every run-time choice of an instantiation and every grid rule is written once ---------------

LAUNCHERS = "// host-side launch wrappers"   # dsea_kernels.hip: the kernels above this line, their launchers below


def code(text):
    """The text without its // comments (which may name a kernel family without launching it)."""
    return re.sub(r"//[^\n]*", "", text)


def function_spans(text):
    """(name, start, end) of the host functions defined at namespace level: a header line without indentation that ends
    in `{`, up to the first line that is a bare `}`."""
    spans = []
    for m in re.finditer(r"^(?:template <[^\n]*>\n)?(?:static |inline )*[\w:<>*&]+\s+(\w+)\([^;{}]*\)\s*\{\n", text, re.M):
        spans.append((m.group(1), m.start(), text.index("\n}\n", m.end())))
    return spans


def enclosing_functions(text, needle):
    spans = function_spans(text)
    found = []
    for m in re.finditer(re.escape(needle), text):
        owners = [name for name, a, b in spans if a <= m.start() < b]
        found.append(owners[-1] if owners else None)
    return found


def test_each_template_ladder_is_spelled_once():
    src = sources()
    rpl = {name: len(re.findall(r"<\s*2,\s*4,\s*8,\s*16\s*>", text)) for name, text in src.items()}
    split = {name: len(re.findall(r"<\s*4,\s*8,\s*16\s*>", text)) for name, text in src.items()}
    assert sum(rpl.values()) == 1, rpl
    assert sum(split.values()) == 1, split
    # and no member of these kernel families is picked by a literal anywhere else (a `case 4: k_rdots<4, ...>` ladder)
    families = r"\b(k_rdots|k_rdots_split|k_axpy_norm|k_axpy_norm_split|k_ritz_block|k_ritz_block_split)<\(?\s*\d"
    literal = [(name, m.group(0)) for name, text in src.items() for m in re.finditer(families, text)]
    assert not literal, literal
    for macro in ("LAUNCH_RPL", "KLAUNCH"):
        assert not any(macro in text for text in src.values()), macro


def test_each_streaming_kernel_family_has_one_launch_expression():
    src = {name: code(text) for name, text in sources().items()}
    for family in ("k_rdots<", "k_axpy_norm<", "k_rdots_split<", "k_axpy_norm_split<"):
        hits = {name: text.count(family) for name, text in src.items() if family in text}
        assert hits == {"dsea_kernels.hip": 1}, (family, hits)
    for family in ("k_spmv_sell<", "k_spmv_tfim<"):
        assert [name for name, text in src.items() if family in text] == ["dsea_kernels.hip"]
        owners = set(enclosing_functions(src["dsea_kernels.hip"], family))
        assert len(owners) == 1 and None not in owners, (family, owners)


def test_each_grid_rule_is_stated_once():
    """In host code: the SELL kernels' own slice map (device code above the launchers) divides by the same four slices
    per block and is not a launcher's grid."""
    src = sources()
    assert src["dsea_kernels.hip"].count(LAUNCHERS) == 1
    src["dsea_kernels.hip"] = src["dsea_kernels.hip"].split(LAUNCHERS)[1]
    for rule in ("nslices + 3) / 4", "<= 2048 ? 4"):
        hits = {name: text.count(rule) for name, text in src.items() if rule in text}
        assert hits == {"dsea_kernels.hip": 1}, (rule, hits)


def test_the_fused_launcher_asks_the_fused_tail_predicate():
    text = sources()["dsea_kernels.hip"]
    assert "launch_tfim_fused" in enclosing_functions(text, "has_fused_tail(")
