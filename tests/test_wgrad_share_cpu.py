"""CPU: the share scheme of the five weight-gradient kernel families is written once (dmvsnet_amd/csrc/wgrad_share.h).

The un-map of the xcd_grid order, the 2^22 tile limit, the partials' summation loop, the tile decode, the check between the two launches
and the plan code each occur exactly once across the six headers -- in the shared one -- so a sixth family cannot grow a copy unseen.
The shared header defines no kernel (the per-header kernel-set assertions and the profiling tooling keep every kernel's name where it
was) and every family header includes it.  scripts/wgrad_share_check.cpp walks the functions themselves on the host.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmvsnet_amd", "csrc")
SHARED = "wgrad_share.h"
FAMILIES = ("conv3d_wgrad.h", "conv3d_wgrad_s2.h", "conv3d_wgrad_c2.h", "conv2d_k5s2_bwd.h", "conv2d_wgrad_fpn.h")
PATTERNS = ("(blockIdx.x & 7) * per", "1L << 22", "sum += ws[", "tile % a.nx", "hipGetLastError(); e != hipSuccess", "* 512 + (int)xcd_grid")
# the same constructs whatever their operands are called: the un-map (its formula is quoted once in the shared header's text and
# written once in place()), the tile decode, the share's range
CODE_FORMS = ((r"& 7\) \* per", 2), (r"\w+ % \w+\.nx\b", 2), (r"\* \w+\.ntiles / \w+\.S\b", 1))


def read(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_share_scheme_is_written_once():
    src = {name: read(name) for name in (SHARED,) + FAMILIES}
    for pat in PATTERNS:
        counts = {name: text.count(pat) for name, text in src.items()}
        assert sum(counts.values()) == 1 and counts[SHARED] == 1, (pat, counts)
    for rx, want in CODE_FORMS:
        counts = {name: len(re.findall(rx, text)) for name, text in src.items()}
        assert counts[SHARED] == want and sum(counts.values()) == want, (rx, counts)
    assert not re.findall(r"__global__", src[SHARED])
    for name in FAMILIES:
        assert '#include "%s"' % SHARED in src[name], name
    assert '#include "conv3d_wgrad_s2.h"' in src["conv2d_k5s2_bwd.h"]   # K3k uses K3h's tile chain and partial store
    assert SHARED in open(os.path.join(CSRC, "Makefile")).read()
    check = open(os.path.join(ROOT, "scripts", "wgrad_share_check.cpp")).read()
    assert "-fsanitize=address,undefined" in check and all("wshare::%s(" % f in check for f in ("place", "first_tile", "decode"))
