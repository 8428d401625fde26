"""CPU (-m "not gpu"): what ops.conv3d and the other timed conv launches dispatch, without a GPU.  A fake library records every
kernel launch with its integer arguments and returns scripted codes; host-only queries (plans, weight lengths, packers, error
strings) go to the real library.  Pinned per case: the C entry called and its flags, the launch_log families, the timer
records, and that no timer event leaks.  Also pinned: which kernel forms MVSNet.prepare packs for every layer."""
import pytest
import torch

from dmvsnet_amd import MVSNet, _lib, ops, synth
from dmvsnet_amd.ops import CONV_S1, CONV_S2, DECONV_S2, IN_VIEWS, OUT_Q4, RELU

EUNS = _lib.EUNSUPPORTED
HOST_ONLY = ("_plan", "_weight_floats")


class _FakeLib:
    def __init__(self, real, codes):
        self.real, self.codes, self.calls = real, dict(codes), []

    def __getattr__(self, name):
        if name.endswith(HOST_ONLY) or name.startswith(("dmvs_pack_", "dmvs_error_string")):
            return getattr(self.real, name)

        def launch(*args):
            self.calls.append((name, tuple(a for a in args if type(a) is int)))
            return self.codes.get(name, 0)
        return launch


class _Ev:
    def record(self):
        pass


class _Timer(ops.KernelTimer):
    def __init__(self):
        super().__init__()
        self.made = []

    def _event(self):
        if self._pool:
            return self._pool.pop()
        self.made.append(_Ev())
        return self.made[-1]

    def held(self):
        """Every event this timer made is in a record or back in the pool."""
        return sorted(map(id, [r[1] for r in self.records] + [r[2] for r in self.records] + self._pool)) == sorted(map(id, self.made))


@pytest.fixture
def fake(monkeypatch):
    real = _lib.load()
    state = {}

    def install(codes=()):
        lib = _FakeLib(real, codes)
        monkeypatch.setattr(ops._lib, "load", lambda: lib)
        state["lib"] = lib
        return lib

    monkeypatch.setattr(ops, "_req", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "timer", _Timer())
    monkeypatch.setattr(ops, "launch_log", [])
    for k in ("use_c8", "use_c8_fused", "use_wino", "use_coarse", "use_zmarch", "use_prob_fused"):
        monkeypatch.setattr(ops, k, True)
    monkeypatch.setattr(ops, "split_probe", 0)
    monkeypatch.setattr(ops, "WINO_MIN_BLOCKS", 0)
    monkeypatch.setattr(ops, "ZMARCH_MIN_DEPTH", 8)
    install()
    return install


def _records():
    t = ops.timer
    return [(r[0], lab, r[3], r[4], r[5]) for r, lab in zip(t.records, t.labels)]


def _no_leak():
    assert ops.timer.held()


_W = torch.zeros(1)


def _layer(name, mode, kd, cin, cout, direct=True, relu=True, **forms):
    L = ops.ConvLayer(name, mode, kd, cin, cout, _W if direct else None, forms.pop("w_mfma", _W), _W, _W, relu)
    for k, v in forms.items():
        setattr(L, k, v)
    return L


CONV2 = _layer("r.conv2", CONV_S1, 3, 16, 16, w_wino=_W, w_zmarch=_W)
CONV4 = _layer("r.conv4", CONV_S1, 3, 32, 32, w_wino=_W, w_coarse=_W)
CONV0X2 = _layer("r.conv0x2", CONV_S1, 3, 2, 16, w_wino=_W)
CONV1 = _layer("r.conv1", CONV_S2, 3, 8, 16, w_split=_W)
CONV7 = _layer("r.conv7", DECONV_S2, 3, 64, 32)
PROB = _layer("r.prob", CONV_S1, 3, 8, 2, relu=False, w_mfma=None)
FC00 = _layer("feature.conv0.0", CONV_S1, 1, 4, 8, direct=False, w_c8=_W)
FC01 = _layer("feature.conv0.1", CONV_S1, 1, 8, 8, direct=False, w_c8=_W)
OUT2 = _layer("feature.out2", CONV_S1, 1, 32, 16, direct=False, relu=False, w_wino=_W)


def _k3(L, D, H, W, xdiv=None, cin=None):
    """Timer record of a form launch: FLOPs in the direct form; executed = FLOPs / xdiv (conv0: 8/6 of that, padded k-groups)."""
    cin = L.cin if cin is None else cin
    fl = 2.0 * 9 * L.kdepth * cin * L.cout * D * H * W
    xf = fl if xdiv is None else fl / xdiv * (8.0 / 6.0 if cin == 2 else 1.0)
    return fl, 4.0 * (cin + L.cout) * D * H * W, xf


def _tail(L, D, H, W, skip=False):
    Do, Ho, Wo = L.out_shape(D, H, W)
    vox = D * H * W if L.mode == DECONV_S2 else Do * Ho * Wo
    fl = 2.0 * 9 * L.kdepth * L.cin * L.cout * vox
    return fl, 4.0 * (L.cin * D * H * W + L.cout * Do * Ho * Wo * (2 if skip else 1)), fl


def _form_args(L, D, H, W, flags, cin=None):
    return ((cin or L.cin), L.cout, D, H, W, L.kdepth, flags)


# (id, layer, kwargs of conv3d, module switches, scripted codes, D, W,
#  expected launches [(entry, int args)], expected timer record (family, label, flops, bytes, exec) | exception)
H = 8
CASES = [
    ("k3z", CONV2, {}, {}, {}, 8, 16,
     [("dmvs_conv3d_zmarch", _form_args(CONV2, 8, H, 16, RELU))], ("conv3d_mfma", "r.conv2") + _k3(CONV2, 8, H, 16, 2.25)),
    ("k3z_shallow_to_k3w", CONV2, {}, {}, {}, 4, 16,
     [("dmvs_conv3d_wino", _form_args(CONV2, 4, H, 16, RELU))], ("conv3d_mfma", "r.conv2") + _k3(CONV2, 4, H, 16, 2.25)),
    ("k3z_min_depth_knob", CONV2, {}, {"ZMARCH_MIN_DEPTH": 4}, {}, 4, 16,
     [("dmvs_conv3d_zmarch", _form_args(CONV2, 4, H, 16, RELU))], ("conv3d_mfma", "r.conv2") + _k3(CONV2, 4, H, 16, 2.25)),
    ("k3z_declines_to_k3w", CONV2, {}, {}, {"dmvs_conv3d_zmarch": EUNS}, 8, 16,
     [("dmvs_conv3d_zmarch", _form_args(CONV2, 8, H, 16, RELU)), ("dmvs_conv3d_wino", _form_args(CONV2, 8, H, 16, RELU))],
     ("conv3d_mfma", "r.conv2") + _k3(CONV2, 8, H, 16, 2.25)),
    ("k3z_and_k3w_decline_to_k3", CONV2, {"family": "fam"}, {}, {"dmvs_conv3d_zmarch": EUNS, "dmvs_conv3d_wino": EUNS}, 8, 16,
     [("dmvs_conv3d_zmarch", _form_args(CONV2, 8, H, 16, RELU)), ("dmvs_conv3d_wino", _form_args(CONV2, 8, H, 16, RELU)),
      ("dmvs_conv3d_mfma", (16, 16, 8, H, 16, CONV_S1, 3, RELU))], ("fam", "r.conv2") + _tail(CONV2, 8, H, 16)),
    ("k3z_off_w_not_4", CONV2, {}, {}, {}, 8, 18,     # the Winograd plan is negative for W % 4 != 0: auto skips K3w
     [("dmvs_conv3d_zmarch", _form_args(CONV2, 8, H, 18, RELU))], ("conv3d_mfma", "r.conv2") + _k3(CONV2, 8, H, 18, 2.25)),
    ("w_not_4_declined_to_k3", CONV2, {}, {}, {"dmvs_conv3d_zmarch": EUNS}, 8, 18,
     [("dmvs_conv3d_zmarch", _form_args(CONV2, 8, H, 18, RELU)), ("dmvs_conv3d_mfma", (16, 16, 8, H, 18, CONV_S1, 3, RELU))],
     ("conv3d_mfma", "r.conv2") + _tail(CONV2, 8, H, 18)),
    ("use_zmarch_off", CONV2, {}, {"use_zmarch": False}, {}, 8, 16,
     [("dmvs_conv3d_wino", _form_args(CONV2, 8, H, 16, RELU))], ("conv3d_mfma", "r.conv2") + _k3(CONV2, 8, H, 16, 2.25)),
    ("use_wino_off", CONV2, {}, {"use_wino": False}, {}, 8, 16,
     [("dmvs_conv3d_mfma", (16, 16, 8, H, 16, CONV_S1, 3, RELU))], ("conv3d_mfma", "r.conv2") + _tail(CONV2, 8, H, 16)),
    ("wino_min_blocks", CONV2, {}, {"WINO_MIN_BLOCKS": 1 << 30, "use_zmarch": False}, {}, 8, 16,
     [("dmvs_conv3d_mfma", (16, 16, 8, H, 16, CONV_S1, 3, RELU))], ("conv3d_mfma", "r.conv2") + _tail(CONV2, 8, H, 16)),
    ("direct", CONV2, {"backend": "direct"}, {}, {}, 8, 16,
     [("dmvs_conv3d_direct", (16, 16, 8, H, 16, CONV_S1, 3, RELU))], ("conv3d_direct", "r.conv2") + _tail(CONV2, 8, H, 16)),
    ("forced_mfma", CONV2, {"backend": "mfma"}, {}, {}, 8, 16,
     [("dmvs_conv3d_mfma", (16, 16, 8, H, 16, CONV_S1, 3, RELU))], ("conv3d_mfma", "r.conv2") + _tail(CONV2, 8, H, 16)),
    ("forced_zmarch_shallow", CONV2, {"backend": "zmarch"}, {"use_zmarch": False}, {}, 2, 16,
     [("dmvs_conv3d_zmarch", _form_args(CONV2, 2, H, 16, RELU))], ("conv3d_mfma", "r.conv2") + _k3(CONV2, 2, H, 16, 2.25)),
    ("forced_zmarch_declined", CONV2, {"backend": "zmarch"}, {}, {"dmvs_conv3d_zmarch": EUNS}, 8, 16,
     [("dmvs_conv3d_zmarch", _form_args(CONV2, 8, H, 16, RELU))], _lib.DmvsError),
    ("forced_zmarch_no_weights", CONV4, {"backend": "zmarch"}, {}, {}, 8, 16, [], _lib.DmvsError),
    ("forced_wino_w_not_4", CONV2, {"backend": "wino"}, {}, {}, 8, 18,
     [("dmvs_conv3d_wino", _form_args(CONV2, 8, H, 18, RELU))], ("conv3d_mfma", "r.conv2") + _k3(CONV2, 8, H, 18, 2.25)),
    ("forced_wino_declined", CONV2, {"backend": "wino"}, {}, {"dmvs_conv3d_wino": EUNS}, 8, 16,
     [("dmvs_conv3d_wino", _form_args(CONV2, 8, H, 16, RELU))], _lib.DmvsError),
    ("einval_raises", CONV2, {}, {}, {"dmvs_conv3d_zmarch": _lib.EINVAL}, 8, 16,
     [("dmvs_conv3d_zmarch", _form_args(CONV2, 8, H, 16, RELU))], _lib.DmvsError),
    ("k3r", CONV4, {}, {}, {}, 4, 16,
     [("dmvs_conv3d_coarse", _form_args(CONV4, 4, H, 16, RELU))], ("conv3d_mfma", "r.conv4") + _k3(CONV4, 4, H, 16, 2.25)),
    ("k3r_declines_to_k3w", CONV4, {}, {}, {"dmvs_conv3d_coarse": EUNS}, 4, 16,
     [("dmvs_conv3d_coarse", _form_args(CONV4, 4, H, 16, RELU)), ("dmvs_conv3d_wino", _form_args(CONV4, 4, H, 16, RELU))],
     ("conv3d_mfma", "r.conv4") + _k3(CONV4, 4, H, 16, 2.25)),
    ("use_coarse_off", CONV4, {}, {"use_coarse": False}, {}, 4, 16,
     [("dmvs_conv3d_wino", _form_args(CONV4, 4, H, 16, RELU))], ("conv3d_mfma", "r.conv4") + _k3(CONV4, 4, H, 16, 2.25)),
    ("k3r_needs_use_wino", CONV4, {}, {"use_wino": False}, {}, 4, 16,
     [("dmvs_conv3d_mfma", (32, 32, 4, H, 16, CONV_S1, 3, RELU))], ("conv3d_mfma", "r.conv4") + _tail(CONV4, 4, H, 16)),
    ("forced_coarse", CONV4, {"backend": "coarse"}, {"use_coarse": False}, {}, 4, 18,
     [("dmvs_conv3d_coarse", _form_args(CONV4, 4, H, 18, RELU))], ("conv3d_mfma", "r.conv4") + _k3(CONV4, 4, H, 18, 2.25)),
    ("forced_coarse_with_skip", CONV4, {"backend": "coarse", "skip": True}, {}, {}, 4, 16, [], _lib.DmvsError),
    ("k3w_conv0", CONV0X2, {}, {}, {}, 8, 16,
     [("dmvs_conv3d_wino", _form_args(CONV0X2, 8, H, 16, RELU))], ("conv3d_mfma", "r.conv0x2") + _k3(CONV0X2, 8, H, 16, 2.25)),
    ("skip_goes_to_k3", CONV2, {"skip": True}, {}, {}, 8, 16,
     [("dmvs_conv3d_mfma", (16, 16, 8, H, 16, CONV_S1, 3, RELU))], ("conv3d_mfma", "r.conv2") + _tail(CONV2, 8, H, 16, True)),
    ("deconv_skip_up", CONV7, {"skip": True}, {}, {}, 2, 8,
     [("dmvs_conv3d_mfma", (64, 32, 2, H, 8, DECONV_S2, 3, RELU))], ("conv3d_mfma", "r.conv7") + _tail(CONV7, 2, H, 8, True)),
    ("prob_auto_is_k2", PROB, {}, {}, {}, 8, 16,
     [("dmvs_conv3d_direct", (8, 2, 8, H, 16, CONV_S1, 3, 0))], ("prob_head", "r.prob") + _tail(PROB, 8, H, 16)),
    ("prob_forced_mfma", PROB, {"backend": "mfma"}, {}, {}, 8, 16, [], _lib.DmvsError),
    ("k3w_q4", OUT2, {"out_q4": True, "family": "feature_mfma"}, {}, {}, 3, 16,
     [("dmvs_conv3d_wino", _form_args(OUT2, 3, H, 16, OUT_Q4))], ("feature_mfma", "feature.out2") + _k3(OUT2, 3, H, 16, 2.25)),
    ("k3w_q4_declined", OUT2, {"out_q4": True}, {}, {"dmvs_conv3d_wino": EUNS}, 3, 16,
     [("dmvs_conv3d_wino", _form_args(OUT2, 3, H, 16, OUT_Q4)), ("dmvs_conv3d_mfma", (32, 16, 3, H, 16, CONV_S1, 1, OUT_Q4))],
     ("conv3d_mfma", "feature.out2") + _tail(OUT2, 3, H, 16)),
    ("k3s", FC01, {}, {}, {}, 3, 16,
     [("dmvs_conv2d_c8", (8, 3, H, 16, RELU))], ("conv3d_mfma", "feature.conv0.1") + _k3(FC01, 3, H, 16)),
    ("k3s_views", FC00, {"in_views": True, "family": "feature_mfma"}, {}, {}, 3, 16,
     [("dmvs_conv2d_c8", (3, 3, H, 16, RELU | IN_VIEWS))], ("feature_mfma", "feature.conv0.0") + _k3(FC00, 3, H, 16, cin=3)),
    ("k3s_declines_to_k3", FC00, {"in_views": True}, {}, {"dmvs_conv2d_c8": EUNS}, 3, 16,
     [("dmvs_conv2d_c8", (3, 3, H, 16, RELU | IN_VIEWS)), ("dmvs_conv3d_mfma", (4, 8, 3, H, 16, CONV_S1, 1, RELU | IN_VIEWS))],
     ("conv3d_mfma", "feature.conv0.0") + _tail(FC00, 3, H, 16)),
    ("use_c8_off", FC01, {}, {"use_c8": False}, {}, 3, 16,
     [("dmvs_conv3d_mfma", (8, 8, 3, H, 16, CONV_S1, 1, RELU))], ("conv3d_mfma", "feature.conv0.1") + _tail(FC01, 3, H, 16)),
    ("k3s_q4_goes_to_k3", FC01, {"out_q4": True}, {}, {}, 3, 16,
     [("dmvs_conv3d_mfma", (8, 8, 3, H, 16, CONV_S1, 1, RELU | OUT_Q4))], ("conv3d_mfma", "feature.conv0.1") + _tail(FC01, 3, H, 16)),
    ("forced_c8_declined", FC01, {"backend": "c8"}, {}, {"dmvs_conv2d_c8": EUNS}, 3, 16,
     [("dmvs_conv2d_c8", (8, 3, H, 16, RELU))], _lib.DmvsError),
    ("forced_c8_no_weights", CONV2, {"backend": "c8"}, {}, {}, 8, 16, [], _lib.DmvsError),
    ("split_probe", CONV1, {}, {"split_probe": 3}, {}, 8, 16,
     [("dmvs_conv3d_split_probe", (8, H, 16, 3, RELU))], ("conv3d_mfma", "r.conv1", 2.0 * 27 * 8 * 16 * 4 * 4 * 8,
                                                       4.0 * (8 * 8 * H * 16 + 16 * 4 * 4 * 8), 2.0 * 27 * 8 * 16 * 4 * 4 * 8)),
    ("split_probe_not_with_skip", CONV1, {"skip": True}, {"split_probe": 6}, {}, 8, 16,
     [("dmvs_conv3d_mfma", (8, 16, 8, H, 16, CONV_S2, 3, RELU))], ("conv3d_mfma", "r.conv1") + _tail(CONV1, 8, H, 16, True)),
    ("forced_split6", CONV1, {"backend": "split6"}, {}, {}, 8, 16,
     [("dmvs_conv3d_split_probe", (8, H, 16, 6, RELU))], ("conv3d_mfma", "r.conv1", 2.0 * 27 * 8 * 16 * 4 * 4 * 8,
                                                       4.0 * (8 * 8 * H * 16 + 16 * 4 * 4 * 8), 2.0 * 27 * 8 * 16 * 4 * 4 * 8)),
    ("forced_split_no_weights", CONV2, {"backend": "split3"}, {}, {}, 8, 16, [], _lib.DmvsError),
    # deliberate changes: a forced backend runs its own kernel or raises (on the parent these fell through to another kernel)
    ("forced_c8_with_skip", FC01, {"backend": "c8", "skip": True}, {}, {}, 3, 16, [], _lib.DmvsError),
    ("forced_c8_with_q4", FC01, {"backend": "c8", "out_q4": True}, {}, {}, 3, 16, [], _lib.DmvsError),
    ("forced_wino_with_skip", CONV2, {"backend": "wino", "skip": True}, {}, {}, 8, 16, [], _lib.DmvsError),
    ("forced_split_with_skip", CONV1, {"backend": "split6", "skip": True}, {}, {}, 8, 16, [], _lib.DmvsError),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv3d_dispatch(fake, monkeypatch, case):
    _, L, kw, switches, codes, D, W, launches, want = case
    for k, v in switches.items():
        monkeypatch.setattr(ops, k, v)
    lib = fake(codes)
    kw = dict(kw)
    in_views = kw.get("in_views", False)
    x = torch.zeros((D, 3, H, W) if in_views else (L.cin, D, H, W))
    if kw.get("skip"):
        Do, Ho, Wo = L.out_shape(D, H, W)
        kw["skip"] = torch.zeros((L.cout, Do, Ho, Wo))
    if isinstance(want, type):
        with pytest.raises(want):
            ops.conv3d(x, L, **kw)
        assert lib.calls == launches and ops.launch_log == [] and ops.timer.records == []
        return
    y = ops.conv3d(x, L, **kw)
    Do, Ho, Wo = L.out_shape(D, H, W)
    assert tuple(y.shape) == ((2, Do, L.cout // 8, Ho, Wo, 4) if kw.get("out_q4") else (L.cout, Do, Ho, Wo))
    assert lib.calls == launches
    assert ops.launch_log == [want[0]]
    assert _records() == [want]
    _no_leak()


def test_featurenet_conv0(fake, monkeypatch):
    imgs = torch.zeros(3, 3, H, 16)
    y = ops.featurenet_conv0(imgs, FC00, FC01, family="feature_mfma")
    assert tuple(y.shape) == (8, 3, H, 16)
    assert ops._lib.load().calls == [("dmvs_featurenet_conv0", (3, H, 16))]
    assert ops.launch_log == ["feature_mfma"]
    assert _records() == [("feature_mfma", "feature.conv0.fused", 2.0 * 9 * 11 * 8 * 3 * H * 16, 4.0 * 11 * 3 * H * 16,
                           2.0 * 9 * 11 * 8 * 3 * H * 16)]
    lib = fake({"dmvs_featurenet_conv0": EUNS})
    assert ops.featurenet_conv0(imgs, FC00, FC01) is None
    assert lib.calls == [("dmvs_featurenet_conv0", (3, H, 16))] and len(ops.launch_log) == 1
    _no_leak()
    monkeypatch.setattr(ops, "use_c8_fused", False)
    assert ops.featurenet_conv0(imgs, FC00, FC01) is None and len(lib.calls) == 1


def test_conv3d_fpn(fake):
    L = _layer("feature.out3", CONV_S1, 1, 32, 16, direct=False, relu=False, w_wino=_W, w_wino_fpn=_W)
    lat, td = torch.zeros(8, 3, H, 16), torch.zeros(32, 3, H // 2, 8)
    y = ops.conv3d_fpn(lat, td, L, out_q4=True, family="feature_mfma")
    assert tuple(y.shape) == (2, 3, 2, H, 16, 4)
    assert ops._lib.load().calls == [("dmvs_conv3d_wino_fpn2", (3, H, 16, OUT_Q4))]
    vox = 3 * H * 16
    assert ops.launch_log == ["feature_mfma"]
    assert _records() == [("feature_mfma", "feature.out3.fpn", 2.0 * vox * (9 * 32 * 16 + 8 * 32),
                           4.0 * (8 * vox + 32 * vox / 4 + 16 * vox), vox * 120 * 2048 / 64.0)]
    lib = fake({"dmvs_conv3d_wino_fpn2": EUNS})
    assert ops.conv3d_fpn(lat, td, L) is None
    assert lib.calls == [("dmvs_conv3d_wino_fpn2", (3, H, 16, 0))] and len(ops.launch_log) == 1
    _no_leak()


@pytest.mark.parametrize("affine", [False, True])
def test_prob_regress(fake, affine):
    D = 8
    x, out, itv = torch.zeros(8, D, H, 16), torch.zeros(2, H, 16), torch.zeros(())
    hyp = ops.AffinePlanes(torch.zeros(H, 16), itv, D) if affine else torch.zeros(D, H, 16)
    assert ops.prob_regress(x, PROB, hyp, itv, 5.0, out) is True
    assert ops._lib.load().calls == [("dmvs_prob_regress", (8, D, H, 16))]
    hb = H * 16 if affine else D * H * 16
    assert ops.launch_log == ["prob_head"]
    assert _records() == [("prob_head", "r.prob", 2.0 * 27 * 8 * 2 * D * H * 16, 4.0 * (8 * D * H * 16 + hb + 2 * H * 16),
                           2.0 * 27 * 8 * 2 * D * H * 16)]
    lib = fake({"dmvs_prob_regress": EUNS})
    assert ops.prob_regress(x, PROB, hyp, itv, 5.0, out) is False
    assert len(lib.calls) == 1 and len(ops.launch_log) == 1
    _no_leak()


def test_conv3d_split(fake):
    y = ops.conv3d_split(torch.zeros(8, 6, H, 14), CONV1, 3)
    assert tuple(y.shape) == (16, 3, H // 2, 7)
    assert ops._lib.load().calls == [("dmvs_conv3d_split_probe", (6, H, 14, 3, RELU))]
    fl = 2.0 * 27 * 8 * 16 * 3 * 4 * 7
    assert _records() == [("conv3d_mfma", "r.conv1", fl, 4.0 * (8 * 6 * H * 14 + 16 * 3 * 4 * 7), fl)]
    with pytest.raises(_lib.DmvsError):
        ops.conv3d_split(torch.zeros(8, 6, H, 14), CONV2, 3)
    _no_leak()


@pytest.fixture(scope="module")
def packed():
    cfg = synth.CONFIGS["c1"]
    net = MVSNet(cfg["ndepths"], cfg["ratios"], verbose=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
    net.prepare(torch.device("cpu"))
    return net


def _fields(L):
    return {k[2:] for k in vars(L) if k.startswith("w_") and getattr(L, k) is not None}


def test_prepare_packs_these_forms(packed):
    reg = {"conv1": {"direct", "mfma", "split"},
           "conv2": {"direct", "mfma", "wino", "zmarch"}, "conv4": {"direct", "mfma", "wino", "coarse"},
           "conv6": {"direct", "mfma", "wino", "coarse"}, "conv2@d1": {"mfma", "wino"},
           "conv4@d1": {"mfma", "wino", "coarse"}, "conv6@d1": {"mfma", "wino", "coarse"}, "prob": {"direct"}}
    reg.update({n: {"direct", "mfma"} for n in ("conv3", "conv5", "conv7", "conv9", "conv11")})
    ref = {n: f for n, f in reg.items() if n != "conv6@d1"}   # the refine nets' conv5 - conv7 are 2D layers already
    for cr in list(packed.cost_regularization) + list(packed.cost_regularization_refine):
        conv0, small, huge = cr._packed
        assert _fields(conv0) == {"direct", "mfma", "wino"} and conv0.name.endswith(".conv0x2")
        for L in (small, huge):
            assert {n: _fields(l) for n, l in L.items()} == (ref if cr.refine else reg)
            for n, l in L.items():
                assert l.name.endswith("." + n)
    feat = {n: {"mfma"} for n in ("conv1.0", "conv2.0", "out1", "inner1", "inner2")}
    feat.update({n: {"mfma", "c8"} for n in ("conv0.0", "conv0.1")})
    feat.update({n: {"mfma", "wino"} for n in ("conv1.1", "conv1.2", "conv2.1", "conv2.2", "out2")})
    feat["out3"] = {"mfma", "wino", "wino_fpn"}
    assert {n: _fields(l) for n, l in packed.feature._packed.items()} == feat


@pytest.mark.parametrize("backend", ["auto", "direct", "mfma"])
def test_branch_backends(fake, packed, backend):
    """One U-Net branch of a 3D pass (D = 8): every layer runs under each backend the network offers (conv_backend)."""
    lib = fake()
    _, small, _ = packed.cost_regularization[0]._packed
    out = torch.zeros(2, 8, 16, 16)
    assert packed.cost_regularization[0]._branch(torch.zeros(8, 8, 16, 16), small, out, backend) is True
    k3 = {"direct": "dmvs_conv3d_direct"}.get(backend, "dmvs_conv3d_mfma")
    forms = {"conv2": "dmvs_conv3d_wino", "conv4": "dmvs_conv3d_coarse", "conv6": "dmvs_conv3d_coarse"}
    want = [forms.get(n, k3) if backend == "auto" else k3
            for n in ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11")]
    assert [c[0] for c in lib.calls] == want + ["dmvs_conv3d_direct"]
    assert ops.launch_log[-1] == "prob_head" and len(ops.launch_log) == 10
    _no_leak()
