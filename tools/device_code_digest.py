#!/usr/bin/env python3
"""Per-kernel digest of libdsea's device code (CPU only: compiles, runs nothing).

For every file in the Makefile's SRCS: compile the device side alone with the Makefile's own CXXFLAGS, disassemble it,
split the listing at the symbol headers, drop the trailing `// address: encoding` comment of every line and the padding
behind a symbol's last instruction (s_nop / zero bytes up to the next symbol's alignment or the end of the section: it
depends on which symbol follows, not on the kernel), and print
    sha256  instruction-count  mangled-name
per symbol, sorted by name, under a `# file` header.  Two trees whose outputs are equal run the same instructions in
every kernel -- whatever the order of the instantiations inside the ELF, which launch-site edits may change.  --flat
prints the lines of all files as one sorted list without the headers (and refuses a symbol that two files define): the
form to compare when kernels move between files.

    python tools/device_code_digest.py [--csrc DIR] [-j N] [-o OUT] [--flat] [FILE.hip ...]
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "dominantsparseeigenad_amd", "csrc")
HEADER = re.compile(r"^[0-9a-f]+ <(.+)>:\s*$")
PADDING = ("s_nop 0", "s_code_end", "...")


def makefile_vars(csrc):
    """The Makefile's simple assignments, with $(NAME) references expanded."""
    raw = {}
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"^(\w+)\s*[?:]?=\s*(.*?)\s*$", line)
        if m:
            raw[m.group(1)] = os.environ.get(m.group(1), m.group(2)) if "?=" in line else m.group(2)

    def expand(text):
        return re.sub(r"\$\((\w+)\)", lambda m: expand(raw.get(m.group(1), "")), text)

    return {k: expand(v) for k, v in raw.items()}


def objdump_for(hipcc):
    for cand in (os.path.join(os.path.dirname(hipcc), "..", "lib", "llvm", "bin", "llvm-objdump"),
                 os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "llvm-objdump")):
        if os.path.exists(cand):
            return cand
    return shutil.which("llvm-objdump") or sys.exit("llvm-objdump not found")


def digest_file(csrc, mk, objdump, name, tmp):
    elf = os.path.join(tmp, name + ".elf")
    subprocess.run([mk["HIPCC"]] + shlex.split(mk["CXXFLAGS"]) +
                   ["--cuda-device-only", "--no-gpu-bundle-output", "-c", name, "-o", elf], cwd=csrc, check=True)
    listing = subprocess.run([objdump, "-d", elf], check=True, capture_output=True, text=True).stdout
    symbols, current = {}, None
    for line in listing.splitlines():
        m = HEADER.match(line)
        if m:
            current = symbols.setdefault(m.group(1), [])
        elif current is not None and line.strip():
            current.append(line.split("//")[0].strip())
    for body in symbols.values():
        while body and body[-1] in PADDING:
            body.pop()
    return ["%s  %6d  %s" % (hashlib.sha256("\n".join(body).encode()).hexdigest(), len(body), sym)
            for sym, body in sorted(symbols.items())]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--csrc", default=CSRC, help="directory with the Makefile and the sources")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1), help="parallel compiles (at most 16)")
    ap.add_argument("-o", default=None, help="write here instead of stdout")
    ap.add_argument("--flat", action="store_true", help="one sorted list of all files' symbols, no `# file` headers")
    ap.add_argument("files", nargs="*", help="a subset of SRCS (default: all)")
    args = ap.parse_args()
    csrc = os.path.abspath(args.csrc)
    mk = makefile_vars(csrc)
    srcs = mk["SRCS"].split()
    unknown = [f for f in args.files if f not in srcs]
    if unknown:
        sys.exit("not in the Makefile's SRCS: %s" % " ".join(unknown))
    files = args.files or srcs
    objdump = objdump_for(mk["HIPCC"])
    with tempfile.TemporaryDirectory() as tmp, \
            concurrent.futures.ThreadPoolExecutor(max(1, min(16, args.j))) as pool:
        jobs = [pool.submit(digest_file, csrc, mk, objdump, f, tmp) for f in files]
        out = []
        for f, job in zip(files, jobs):
            out += ["# " + f] + job.result()
    if args.flat:
        out = sorted(line for line in out if not line.startswith("# "))
        names = [line.split()[-1] for line in out]
        if len(set(names)) != len(names):
            sys.exit("defined in two files: %s" % " ".join(sorted({s for s in names if names.count(s) > 1})))
    text = "\n".join(out) + "\n"
    if args.o:
        with open(args.o, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
