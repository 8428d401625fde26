"""N6 (validation mode) on the MI355X: ``mvs_loss`` / the metrics against the reference's recorded values, the kernel against
the CPU restatement (validate_ref) at every size and mask shape, and ``run_validate`` against the restatement applied to the
product's own forward outputs.  Comparisons are against the goldens or the restatement; the only run-against-run checks are
the ones that are about exactly that (two runs give the same bits; the feature cache changes no bit).

Integer outputs (n, n_cells, n_valid, the three threshold counts) are compared EXACTLY: both sides do the same single fp32
subtract / abs / compare on identical inputs, so no input condition is needed."""
import numpy as np
import pytest
import torch

import validate_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN_REL = ref.GOLDEN_REL     # kernel vs the reference's recorded value: 4 x the measured gap restatement vs reference
KERNEL_REL = ref.KERNEL_REL     # kernel vs restatement, total
TERM_ULPS = ref.TERM_ULPS       # kernel vs restatement, each fp32 mean


def ulps(a, b):
    """Distance in representable fp32 numbers between two finite same-sign floats."""
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def cuda(tree):
    if isinstance(tree, dict):
        return {k: cuda(v) for k, v in tree.items()}
    return tree.cuda() if isinstance(tree, torch.Tensor) else tree


@pytest.fixture(scope="module")
def loss_golden(golden):
    return golden("validate_loss.npz")


@pytest.mark.parametrize("name", list(ref.CASES))
def test_loss_and_metrics_match_the_reference(loss_golden, name):
    from dmvsnet_amd import AbsDepthError_metrics, Thres_metrics, mvs_loss
    case = ref.loss_case(name)
    assert ref.case_digest(case) == str(loss_golden[name + ".digest"])
    dev = cuda(case)
    kw = {} if case["dlossw"] is None else {"dlossw": list(case["dlossw"])}
    loss = mvs_loss(dev["inputs"], dev["depth_gt"], dev["mask"], "regression", **kw)
    assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32
    last = "stage{}".format(len(case["inputs"]))
    gt, mask = dev["depth_gt"][last], dev["mask"][last] > 0.5
    met = [AbsDepthError_metrics(dev["depth"], gt, mask).item()] + [Thres_metrics(dev["depth"], gt, mask, t).item() for t in (2, 4, 8)]
    want, want_met = float(loss_golden[name + ".loss"]), loss_golden[name + ".metrics"]
    print(f"{name}: loss {loss.item()!r} reference {want!r}; metrics {met} reference {want_met.tolist()}")
    if np.isnan(want):
        assert np.isnan(loss.item()) and met == [0.0, 0.0, 0.0, 0.0]
    else:
        assert abs(loss.item() - want) <= GOLDEN_REL * abs(want)
    assert [np.float32(m) for m in met[1:]] == list(want_met[1:])
    assert abs(met[0] - float(want_met[0])) <= GOLDEN_REL * abs(float(want_met[0]))
    # the float mask (valid > 0.5) and the bool mask are the same thing
    assert AbsDepthError_metrics(dev["depth"], gt, dev["mask"][last]).item() == met[0]


def planes(B, h, w, seed, noise=(0.3, 3.0), kinds=("holes", "holes"), poisoned=False):
    per = []
    for b in range(B):
        gt, main, refine, depth = ref.synth_planes(h, w, seed, noise[b % 2], f"gpu.{b}")
        m = ref.ragged_mask(h, w, seed + b, kinds[b % 2])
        if poisoned:
            ref.poison((gt, main, refine, depth), m, seed + b)
        else:
            for a in (gt, main, refine, depth):
                a[..., m <= 0.5] += np.float32(1000.0)   # whatever sits under the mask must not matter
        per.append((gt, main, refine, depth, m))
    return [torch.from_numpy(np.stack([p[i] for p in per])) for i in range(5)]


def check_against_restatement(out, gt, main, refine, depth, mask, weight):
    terms = out["terms"].cpu().numpy()
    counts = out["counts"].cpu().numpy()
    total = np.float32(0.0)
    for s, dsp in enumerate((main, refine)):
        want, n, n_cells = ref.stage_terms(dsp, gt, mask, weight)
        assert (int(counts[0]), int(counts[1])) == (n, n_cells)
        for k, name in enumerate(ref.TERMS):
            d = ulps(terms[s, k], want[name].item())
            print(f"  set {s} {name}: {terms[s, k]!r} restatement {want[name].item()!r} ({d} ulp)")
            assert d <= TERM_ULPS, (s, name)
        total = total + np.float32(ref.stage_contribution(want).item())
    got = out["total"].item()
    print(f"  total {got!r} restatement {float(total)!r} rel {abs(got - float(total)) / float(total):.3e}")
    assert abs(got - float(total)) <= KERNEL_REL * float(total)
    sums, want_sums = out["image_sums"].cpu().numpy(), ref.metric_sums(depth, gt, mask)
    assert np.array_equal(sums[:, 1:], want_sums[:, 1:])                       # n_valid and the three counts: exact
    assert np.allclose(sums[:, 0], want_sums[:, 0], rtol=1e-12, atol=0)        # fp64 sums of the same fp32 errors
    met, want_met = out["metrics"].cpu().numpy(), ref.metrics_ref(depth, gt, mask)
    assert np.array_equal(met[1:], want_met[1:]) and ulps(met[0], want_met[0]) <= max(1, gt.shape[0])


# widths that are not a multiple of 64 (40, 400) or of the 63-column wave tile, heights that are not a multiple of the 32-row
# workgroup (296), batches; the masks have holes on the tile / strip borders and in the last row / column (ref.ragged_mask)
SIZES = [(1, 32, 40), (2, 128, 160), (1, 296, 400), (2, 512, 640), (1, 1184, 1600)]


@pytest.mark.parametrize("B,h,w", SIZES)
def test_kernel_matches_the_restatement(B, h, w):
    from dmvsnet_amd.validate import dual_depth_loss_stage
    gt, main, refine, depth, mask = planes(B, h, w, seed=3)
    border = mask[0].numpy() <= 0.5
    assert border[h - 1].any() and border[:, w - 1].any() and (w < 63 or border[:, 62].any()) and border[7].any()
    out = dual_depth_loss_stage(main.cuda(), refine.cuda(), gt.cuda(), mask.cuda(), weight=0.7, depth=depth.cuda())
    check_against_restatement(out, gt, main, refine, depth, mask, 0.7)
    # the loss-only and the metrics-only kernels give the same numbers as the combined one
    only = dual_depth_loss_stage(main.cuda(), refine.cuda(), gt.cuda(), mask.cuda(), weight=0.7)
    assert torch.equal(only["terms"], out["terms"]) and torch.equal(only["counts"], out["counts"])
    only = dual_depth_loss_stage(None, None, gt.cuda(), mask.cuda(), depth=depth.cuda())
    assert torch.equal(only["image_sums"], out["image_sums"]) and torch.equal(only["metrics"], out["metrics"])


def test_nonfinite_values_under_the_mask_change_nothing():
    from dmvsnet_amd.validate import dual_depth_loss_stage
    B, h, w = 2, 128, 160
    clean = planes(B, h, w, seed=5)
    dirty = planes(B, h, w, seed=5, poisoned=True)
    for c, d in zip(clean[:4], dirty[:4]):
        assert not torch.isfinite(d).all() and torch.isfinite(c).all()
    gt, main, refine, depth, mask = dirty
    out = dual_depth_loss_stage(main.cuda(), refine.cuda(), gt.cuda(), mask.cuda(), weight=2.0, depth=depth.cuda())
    assert all(torch.isfinite(v.double()).all() for v in out.values())
    cgt, cmain, crefine, cdepth, cmask = clean
    check_against_restatement(out, cgt, cmain, crefine, cdepth, cmask, 2.0)    # the restatement never saw the NaNs
    same = dual_depth_loss_stage(cmain.cuda(), crefine.cuda(), cgt.cuda(), cmask.cuda(), weight=2.0, depth=cdepth.cuda())
    for k in out:
        assert torch.equal(out[k], same[k]), k                                  # every output unchanged, bit for bit


def test_empty_mask():
    from dmvsnet_amd.validate import dual_depth_loss_stage
    gt, main, refine, depth, mask = planes(2, 32, 40, seed=9, kinds=("empty", "empty"))
    out = dual_depth_loss_stage(main.cuda(), refine.cuda(), gt.cuda(), mask.cuda(), depth=depth.cuda())
    assert torch.isnan(out["total"]).all() and torch.isnan(out["terms"]).all()
    assert out["counts"].tolist() == [0, 0]
    assert out["metrics"].tolist() == [0.0, 0.0, 0.0, 0.0] and not out["image_sums"].any()
    # a mask whose valid pixels never form a 2x2 cell: the per-pixel terms are finite, the centre terms NaN (a mean of nothing)
    mask[:] = 0
    mask[:, ::2, ::2] = 1
    out = dual_depth_loss_stage(main.cuda(), refine.cuda(), gt.cuda(), mask.cuda())
    t = out["terms"].cpu()
    assert out["counts"].tolist() == [2 * 16 * 20, 0] and torch.isfinite(t[:, :4]).all() and torch.isnan(t[:, 4:]).all()
    assert torch.isnan(out["total"]).all()


def test_two_runs_are_bit_identical():
    from dmvsnet_amd.validate import dual_depth_loss_stage
    gt, main, refine, depth, mask = [t.cuda() for t in planes(2, 512, 640, seed=13)]
    a = dual_depth_loss_stage(main, refine, gt, mask, weight=0.5, depth=depth)
    b = dual_depth_loss_stage(main, refine, gt, mask, weight=0.5, depth=depth)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # adding into a running total is the reference's `total_loss +=`
    acc = dual_depth_loss_stage(main, refine, gt, mask, weight=0.5, total=a["total"].clone())
    t = a["terms"].cpu().numpy()
    want = np.float32(a["total"].item())
    for s in range(2):
        m = t[s]
        want = want + (((np.float32(2) * m[0] + np.float32(2) * m[1]) + m[2]) + m[3] + (((m[4] + m[5]) + m[6]) + m[7]))
    assert acc["total"].item() == float(want)


# ------------------------------------------------------------------------------------------ run_validate
class Recording:
    """The network as run_validate sees it, keeping a host copy of what every forward returned."""

    def __init__(self, net):
        self.net, self.outputs = net, []

    def __getattr__(self, name):
        return getattr(self.net, name)

    def _keep(self, out):
        self.outputs.append({k: ({kk: vv.cpu() for kk, vv in v.items() if kk.startswith("depth_sub_plus")} if isinstance(v, dict)
                                 else v.cpu()) for k, v in out.items() if k == "depth" or "stage" in k})
        return out

    def __call__(self, *a):
        return self._keep(self.net(*a))

    def forward_features(self, *a):
        return self._keep(self.net.forward_features(*a))


@pytest.fixture(scope="module")
def val_run(tmp_path_factory):
    from dmvsnet_amd import MVSNet, synth
    from dmvsnet_amd.validate import DTUValDataset
    root = str(tmp_path_factory.mktemp("val_scene"))
    info = synth.synth_val_scene(root, seed=0)
    net = MVSNet([16, 8, 8], [3, 2, 1], verbose=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
    net = net.to("cuda:0")
    net.return_prob_volume = False       # the loss does not read it
    ds = DTUValDataset(root, info["listfile"], "val", 3, lights=info["lights"])
    return root, info, net, ds


DLOSSW = (0.5, 1.0, 2.0)


def restated_rows(rec_outputs, ds, batch_size):
    """The five scalars of every batch from the recorded forward outputs (one per forward call) by the restatement."""
    rows, idx = [], 0
    per_call = rec_outputs[0]["depth"].shape[0]
    for b0 in range(0, len(ds), batch_size):
        ids = list(range(b0, min(b0 + batch_size, len(ds))))
        samples = [ds.__getitem__(i, with_images=False) for i in ids]
        outs = rec_outputs[idx:idx - (-len(ids) // per_call)]
        idx += len(outs)
        keys = [k for k in outs[0] if "stage" in k]
        inputs = {k: {n: torch.cat([o[k][n] for o in outs]) for n in ("depth_sub_plus", "depth_sub_plus_refine")} for k in keys}
        gts = {k: torch.from_numpy(np.stack([s["depth"][k] for s in samples])) for k in keys}
        masks = {k: torch.from_numpy(np.stack([s["mask"][k] for s in samples])) for k in keys}
        depth = torch.cat([o["depth"] for o in outs])
        loss = ref.mvs_loss_ref(inputs, gts, masks, DLOSSW).item()
        rows.append([loss] + [float(v) for v in ref.metrics_ref(depth, gts[keys[-1]], masks[keys[-1]])])
    return rows


def check_rows(got_rows, want_rows):
    assert len(got_rows) == len(want_rows)
    for g, w in zip(got_rows, want_rows):
        print(f"  batch: {g} restatement {w}")
        assert abs(g[0] - w[0]) <= KERNEL_REL * abs(w[0])
        assert ulps(g[1], w[1]) <= 2 and g[2:] == w[2:]


@pytest.mark.parametrize("batch_size", [1, 2])
def test_run_validate_matches_the_restatement(val_run, batch_size):
    from dmvsnet_amd import run_validate
    from dmvsnet_amd.validate import SCALARS
    root, info, net, ds = val_run
    rec, rows, stats = Recording(net), [], {}
    got = run_validate(rec, root, info["listfile"], nviews=3, dlossw=DLOSSW, batch_size=batch_size, lights=info["lights"],
                       stats=stats, batch_scalars=rows)
    n_batches = -(-len(ds) // batch_size)
    assert stats["maps"] == len(ds) == 6 and stats["batches"] == n_batches == len(rec.outputs)
    assert {"decode", "h2d", "forward", "loss"} <= set(stats["phases_s"]) and stats["wall_s"] > 0
    want_rows = restated_rows(rec.outputs, ds, batch_size)
    check_rows(rows, want_rows)
    want = ref.average_meter(want_rows)
    assert list(got) == list(SCALARS)
    assert got == ref.average_meter(rows)                      # the host average of the rows that came back, in batch order
    for k in SCALARS:
        assert abs(got[k] - want[k]) <= KERNEL_REL * abs(want[k]), k
    assert all(np.isfinite(v) for v in got.values()) and got["loss"] > 0


def test_run_validate_feature_cache_changes_no_bit(val_run):
    from dmvsnet_amd import run_validate
    root, info, net, ds = val_run
    plain, cached, stats = [], [], {}
    a = run_validate(net, root, info["listfile"], nviews=3, dlossw=DLOSSW, lights=info["lights"], batch_scalars=plain)
    rec = Recording(net)
    b = run_validate(rec, root, info["listfile"], nviews=3, dlossw=DLOSSW, lights=info["lights"], batch_scalars=cached,
                     feature_cache=True, stats=stats)
    check_rows(cached, restated_rows(rec.outputs, ds, 1))      # against the restatement first
    assert cached == plain and a == b                          # ... and bit-identical to the default path
    assert stats["encodes"] == stats["images"] == info["views"] * info["lights"]
    assert stats["hits"] + stats["misses"] == 3 * len(ds) and stats["evictions"] == 0
    assert {"decode", "h2d_ingest", "encode", "forward", "loss"} <= set(stats["phases_s"])
    c = run_validate(net, root, info["listfile"], nviews=3, dlossw=DLOSSW, lights=info["lights"], batch_size=2, feature_cache=True)
    d = run_validate(net, root, info["listfile"], nviews=3, dlossw=DLOSSW, lights=info["lights"], batch_size=2)
    assert c == d
