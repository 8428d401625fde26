"""CPU: the host side of the differentiable convolutions is written once (dmvsnet_amd/ops.py, conv.py, featurenet.py).

* The frame of the five weight-gradient wrappers, the exactly-once check of the gather indices, the gather's appended zero slot and
  the autograd Function each occur exactly once across the three files, so a sixth family cannot grow a copy unseen.  Of ops.py only
  the section of the differentiable convolutions is read (from "training: shared by" up to K5): the BatchNorm wrappers after it keep
  a workspace refusal of their own.
* Every gather index the five ``pack_index_*`` functions return, for every shape of every family, equals the derivation restated
  here -- ``iota + 1`` through ``ops.pack_mfma`` / ``ops.pack_direct``, minus one, zeros to the slot n; the two permutation families
  never select that slot; the gather through the index is the host packer's output bit for bit; repeated calls return one object.
"""
import math
import os
import re

import pytest
import torch

from dmvsnet_amd import conv, featurenet, ops
from dmvsnet_amd.ops import CONV2D_K1, CONV2D_K5S2, CONV_S1, CONV_S2, DECONV_S2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(name):
    return open(os.path.join(ROOT, "dmvsnet_amd", name)).read()


def _sources():
    text = _read("ops.py")
    a = text.index("# ------------------------------------------------------------------------------------------ training: shared by")
    b = text.index("# ------------------------------------------------------------------------------------------ K5 (training: BatchNorm")
    assert 0 < a < b
    for fn in ("def pack_index_mfma(", "def conv3d_wgrad(", "def conv2d_wgrad_fpn(", "def gather_packed(", "def _workspace("):
        assert a < text.index(fn) < b, fn   # the section is the one that holds them
    return {"ops.py": text[a:b], "conv.py": _read("conv.py"), "featurenet.py": _read("featurenet.py")}


ONCE = ("accumulate needs the buffer to add to", "bincount(", "workspace too small")
ONCE_FORMS = (r"torch\.cat\(\(\w+, \w+\.new_zeros\(1\)\)\)", r"new_zeros\(1\)")


def test_the_frame_is_written_once():
    src = _sources()
    for pat in ONCE:
        counts = {name: text.count(pat) for name, text in src.items()}
        assert sum(counts.values()) == 1 and counts["ops.py"] == 1, (pat, counts)
    for rx in ONCE_FORMS:
        counts = {name: len(re.findall(rx, text)) for name, text in src.items()}
        assert sum(counts.values()) == 1 and counts["ops.py"] == 1, (rx, counts)
    fns = {name: re.findall(r"class .*\(torch\.autograd\.Function\)", text) for name, text in src.items()}
    assert fns == {"ops.py": [], "conv.py": ["class _ConvFn(torch.autograd.Function)"], "featurenet.py": []}
    assert not hasattr(featurenet, "_FeatureConvFn")
    assert featurenet._ConvFn is conv._ConvFn


# ------------------------------------------------------------------------------------------ the gather indices
def _tf(w):
    return w.transpose(0, 1).flip(*range(2, w.dim())).contiguous()


def _fourth_channel(w):
    return torch.cat((w, torch.zeros_like(w[:, :1])), 1).contiguous()


def _cases():
    """id -> (the pack_index_* call, the weight's shape, arrange, pack, permutation family)"""
    out = {}
    for C in conv.CHANNELS:
        for kd in (1, 3):
            for tf in (False, True):
                out[f"k3g_{C}_kd{kd}_{'t' if tf else 'f'}"] = (
                    lambda C=C, kd=kd, tf=tf, **kw: ops.pack_index_mfma(C, kd, tf, **kw), (C, C, kd, 3, 3), _tf if tf else None,
                    lambda w, C=C, kd=kd: ops.pack_mfma(w, C, C, CONV_S1, kd), True)
    for cin, cout in ops.WGRAD_C2_SHAPES:
        for tf in (False, True):
            out[f"k2g_{cin}to{cout}_{'t' if tf else 'f'}"] = (
                lambda cin=cin, cout=cout, tf=tf, **kw: ops.pack_index_direct(cin, cout, tf, **kw), (cout, cin, 3, 3, 3), _tf if tf else None,
                lambda w: ops.pack_direct(w, False), True)
    for nd, pairs in conv.CHANNELS_S2.items():
        kd = 3 if nd == 3 else 1
        for fine, coarse in pairs:
            for mode, cin, cout in ((CONV_S2, fine, coarse), (DECONV_S2, coarse, fine)):
                out[f"k3h_{cin}to{cout}_m{mode}_kd{kd}"] = (
                    lambda cin=cin, cout=cout, mode=mode, kd=kd, **kw: ops.pack_index_mfma_s2(cin, cout, mode, kd, **kw),
                    (coarse, fine, kd, 3, 3), None, lambda w, cin=cin, cout=cout, mode=mode, kd=kd: ops.pack_mfma(w, cin, cout, mode, kd), False)
    for cin, cout in ops.WGRAD_K5S2_SHAPES:
        out[f"k3k_{cin}to{cout}"] = (lambda cin=cin, cout=cout, **kw: ops.pack_index_mfma_k5s2(cin, cout, **kw), (cout, cin, 5, 5), None,
                                     lambda w, cin=cin, cout=cout: ops.pack_mfma(w, cin, cout, CONV2D_K5S2, 1), False)
    for cin, cout, k in ops.FPN_SHAPES:
        mode = CONV_S1 if k == 3 else CONV2D_K1
        for tf in (False, True):
            if tf and cin == 3:
                continue   # conv0.0 has no data gradient
            lin, lout = (cout, cin) if tf else (max(cin, 4), cout)
            out[f"k3f_{cin}to{cout}k{k}_{'t' if tf else 'f'}"] = (
                lambda cin=cin, cout=cout, k=k, tf=tf, **kw: ops.pack_index_mfma_fpn(cin, cout, k, tf, **kw), (cout, cin, k, k),
                _tf if tf else (_fourth_channel if cin == 3 else None),
                lambda w, lin=lin, lout=lout, mode=mode: ops.pack_mfma(w, lin, lout, mode, 1), False)
    return out


CASES = _cases()


def test_the_cases_are_every_shape_of_every_family():
    n = {f: sum(1 for k in CASES if k.startswith(f)) for f in ("k3g", "k2g", "k3h", "k3k", "k3f")}
    assert n == {"k3g": 12, "k2g": 4, "k3h": 8, "k3k": 2, "k3f": 11}


@pytest.mark.parametrize("name", list(CASES))
def test_pack_index_is_the_restated_derivation(name):
    index_of, shape, arrange, pack, permutation = CASES[name]
    n = math.prod(shape)
    assert n + 1 < 1 << 24   # iota + 1 is exact in fp32
    iota = (torch.arange(n, dtype=torch.float32) + 1.0).reshape(shape)
    want = pack(iota if arrange is None else arrange(iota)).reshape(-1).to(torch.int64) - 1
    want[want < 0] = n
    index = index_of()
    assert index.dtype == torch.int64 and index.device.type == "cpu" and index.shape == want.shape
    assert torch.equal(index, want)
    assert torch.equal(torch.bincount(index, minlength=n + 1)[:n], torch.ones(n, dtype=torch.int64))   # every element exactly once
    if permutation:
        assert int(index.max()) < n and index.numel() == n   # usable as w.reshape(-1)[index], no appended slot
    assert index_of() is index and index_of(device="cpu") is index
    # the gather through it is the host packer's output, bit for bit
    w = torch.randn(shape, generator=torch.Generator().manual_seed(n))
    packed = pack(w if arrange is None else arrange(w)).reshape(-1)
    assert torch.equal(ops.gather_packed(w, index, not permutation).view(torch.int32), packed.view(torch.int32))
    if permutation:
        assert torch.equal(w.reshape(-1)[index].view(torch.int32), packed.view(torch.int32))
