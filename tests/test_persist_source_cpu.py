"""Source invariants of the persistent single-launch kernels (read from the sources: no build, no GPU).  Their workgroups
wait on each other inside one launch, which is safe only if every wait is bounded and every workgroup is resident: the
first is the property of the bounded waits of dsea_device.h, the second of the one residency gate of the launchers."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "dominantsparseeigenad_amd", "csrc")


def sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    return {os.path.basename(p): open(p).read() for p in paths}


def test_every_poll_of_a_peer_goes_through_a_bounded_wait():
    src = sources()
    assert "dsea_device.h" in src and len(src) > 5
    for name, text in src.items():
        if name == "dsea_device.h":
            continue
        for word in ("__builtin_amdgcn_s_sleep", "granule_try_get", "granule_epoch"):
            assert word not in text, "%s: %s outside dsea_device.h -- poll through its bounded waits" % (name, word)
    # and in there every sleep is followed by the wall-clock test that ends the wait
    dev = src["dsea_device.h"]
    sleeps = dev.count("__builtin_amdgcn_s_sleep")
    assert sleeps >= 1
    assert len(re.findall(r"__builtin_amdgcn_s_sleep\(1\);\s*if \(wall_clock64\(\) - t0 > budget\) (return false|break);",
                          dev)) == sleeps


def test_one_residency_gate_asks_for_the_compute_units():
    hits = {name: text.count("hipDeviceAttributeMultiprocessorCount") for name, text in sources().items()}
    assert sum(hits.values()) == 1, {k: v for k, v in hits.items() if v}
