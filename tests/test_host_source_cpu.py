"""Source invariants of the host layer of libdsea (read from the sources: no build, no GPU).  One HIP error path: the
slot behind dsea_last_hip_error() is written by one function, and every hipGetLastError() of the two host files goes
through it or is discarded on purpose.  One CG polling loop, and one predicate for the fused Lanczos tail.  The launchers: one
dispatch rule per kernel family and each grid rule once.  The kernels: each defined in one file and launched from that file.  The ladder maps:
one host rule set for both families and one site walk in the sector file."""
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
# (over all of csrc/: no assertion names the file a kernel family lives in)


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


def device_spans(text):
    """(name, start, end) of the kernels and device functions, found the same way."""
    spans = []
    for m in re.finditer(r"^(?:template <[^\n]*>\n)?__(?:global|device)__ [^;{}]*?(\w+)\([^;{}]*\)\s*\{\n", text, re.M):
        spans.append((m.group(1), m.start(), text.index("\n}\n", m.end())))
    return spans


def host_code(text):
    """code(text) with the bodies of its kernels and device functions cut out."""
    text = code(text)
    for _, a, b in reversed(device_spans(text)):
        text = text[:a] + text[b:]
    return text


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
        assert list(hits.values()) == [1], (family, hits)   # one expression, in one file
    for family in ("k_spmv_sell<", "k_spmv_tfim<"):
        files = [name for name, text in src.items() if family in text]
        assert len(files) == 1, (family, files)
        owners = set(enclosing_functions(src[files[0]], family))
        assert len(owners) == 1 and None not in owners, (family, owners)


def test_each_grid_rule_is_stated_once():
    """In host code: the SELL kernels' own slice map (k_spmv_sell, sell_slice_of) divides by the same four slices per
    block and is not a launcher's grid -- kernels and device functions are left out by their spans."""
    src = sources()
    for rule in ("nslices + 3) / 4", "<= 2048 ? 4"):
        hits = {name: host_code(text).count(rule) for name, text in src.items()}
        assert sorted(hits.values())[-2:] == [0, 1], (rule, {k: v for k, v in hits.items() if v})
    # (and the exclusion is what it says: the device code does use the first rule)
    assert sum(code(text).count("nslices + 3) / 4") for text in src.values()) > 1


def test_the_fused_launcher_asks_the_fused_tail_predicate():
    owners = [f for text in sources().values() for f in enclosing_functions(text, "has_fused_tail(")]
    assert "launch_tfim_fused" in owners, owners


def test_each_kernel_is_defined_in_one_file_and_launched_from_that_file():
    """A kernel copied into a second file, or launched from a file that does not define it, fails here."""
    src = {name: code(text) for name, text in sources().items() if name.endswith(".hip")}
    defined = {}
    for name, text in src.items():
        for m in re.finditer(r"__global__[^;{}]*?\bvoid\s+(k_\w+)\s*\(", text):
            defined.setdefault(m.group(1), []).append(name)
    assert len(defined) > 50, len(defined)   # (the pattern still finds them)
    twice = {k: v for k, v in defined.items() if len(v) > 1}
    assert not twice, twice
    # a launch site: a klaunch( or hipLaunchKernelGGL( / hipExtLaunchKernelGGL( call, up to the `;` that ends it (a lambda
    # handed a kernel, `go(k_x<...>)`, sits in the launcher that holds the klaunch and is looked for by name below)
    strays = []
    for name, text in src.items():
        for m in re.finditer(r"\b(?:klaunch|hip(?:Ext)?LaunchKernelGGL)\s*\([^;]*;", text):
            for k in re.findall(r"\bk_\w+", m.group(0)):
                if defined.get(k) != [name]:
                    strays.append((name, k))
        for k in set(re.findall(r"\bk_\w+", text)):
            if k in defined and defined[k] != [name]:
                strays.append((name, k))
    assert not strays, strays


# ---- the ladder maps (docs/design/38-ladder-parts.md): one host rule set for both families, one site walk per file ------
LADDER_FILES = ("dsea_ladder.hip", "dsea_hubbard_ladder.hip")


def enclosing_one_liner(text, needle):
    """the name of the one-line function `... name(...) { ... needle ... }` that holds the needle"""
    line = [ln for ln in code(text).splitlines() if needle in ln]
    assert len(line) == 1, line
    return re.match(r"(?:static |inline )*[\w:<>*&]+\s+(\w+)\(", line[0]).group(1)


def test_the_ladder_grid_cap_range_is_tested_once():
    hits = {name: len(re.findall(r"grid_log2\s*(?:>=|<)\s*6\b", code(text))) for name, text in sources().items()}
    assert sum(hits.values()) == 1, {k: v for k, v in hits.items() if v}
    assert enclosing_one_liner(sources()["dsea_internal.h"], "grid_log2 >= 6") == "ladder_grid_ok"


def test_the_ladder_partial_count_is_stated_once():
    """The scratch of the site forms and of the column dots: blocks of 256 rows, capped by DSEA_MAX_TFIM_BLOCKS, times the
    terms.  Neither ladder file nor the C entries repeat it."""
    src = sources()
    files = LADDER_FILES + ("dsea_capi.hip", "dsea_internal.h")
    rules = []
    for name in files:
        text = code(src[name])
        for fn, a, b in function_spans(text):
            if "+ 255) / 256" in text[a:b] and "DSEA_MAX_TFIM_BLOCKS" in text[a:b]:
                rules.append((name, fn))
    assert rules == [("dsea_internal.h", "ladder_partials")], rules
    for name in LADDER_FILES + ("dsea_capi.hip",):
        assert "DSEA_MAX_TFIM_BLOCKS" not in code(src[name]), name
    # one grid rule too: the cap 2^grid_log2 is applied in one function, and no ladder file divides rows by 256 itself
    shifts = [(name, fn) for name in files for fn in enclosing_functions(code(src[name]), "<< (grid_log2")]
    assert shifts == [("dsea_internal.h", "ladder_blocks")], shifts
    for name in LADDER_FILES:
        assert "/ 256" not in host_code(src[name]), name


def test_each_single_vector_ladder_kernel_has_one_launch_expression():
    src = {name: code(text) for name, text in sources().items()}
    for family in ("k_sector_ladder<", "k_sector_ladder_forms<", "k_hubbard_ladder<", "k_hubbard_ladder_forms<"):
        hits = {name: text.count(family) for name, text in src.items() if family in text}
        assert list(hits.values()) == [1], (family, hits)
    # and the Hubbard (species, step) pair is picked through dispatch_int, not through a hand-written chain
    text = src["dsea_hubbard_ladder.hip"]
    spans = {name: text[a:b] for name, a, b in function_spans(text)}
    assert spans["hubbard_ladder_dispatch"].count("dispatch_int<") == 2 and "integral_constant" not in text


def test_the_sector_ladder_has_one_site_walk():
    """The chunk is a template argument and the block helpers are the only helpers: no macro chunk, no second set of
    functions, no sign helper beside block_signed -- in either ladder file."""
    src = sources()
    text = src["dsea_ladder.hip"]
    assert "DSEA_LADDER_CHUNK" not in text
    assert not re.findall(r"\bladder_block_\w*", text)
    helpers = [name for name, _, _ in device_spans(code(text)) if name.startswith("ladder_")]
    assert sorted(helpers) == ["ladder_group", "ladder_qualifies", "ladder_ranks", "ladder_row", "ladder_sites"], helpers
    assert len(re.findall(r"\bint ladder_chunk\(\)", text)) == 1
    # what remains twice: the diagonal row of Z(c), in ladder_row and spelled out in k_sector_ladder at STEP = 0, whose shared
    # form missed the speed bar of the design note (38.6).  Every walk of the sites goes through ladder_sites, from ladder_row
    # and from the forms kernel.
    spans = {re.search(r"\b(?!__launch_bounds__)(\w+)\(", code(text)[a:b]).group(1): code(text)[a:b]    # (a kernel by its own name)
             for _, a, b in device_spans(code(text))}
    assert len(spans) == 5 + 5, sorted(spans)      # five helpers, five kernels
    assert sorted(name for name, body in spans.items() if "diag +=" in body) == ["k_sector_ladder", "ladder_row"]
    assert sorted(name for name, body in spans.items() if "ladder_sites<" in body) == ["k_sector_ladder_forms", "ladder_row"]
    assert sorted(name for name, body in spans.items() if "ladder_group<" in body) == ["ladder_sites"]
    for name in LADDER_FILES:
        assert not re.findall(r"\bh?ladder_signed\b", src[name]) and "block_signed(" in src[name], name
