"""Float64 torch restatement of the cost aggregation (CostAgg.forward over homo_warping, networks/mvsnet.py:111-153 and
networks/module.py:212-251) and its gradients: the common yardstick of tests/test_costagg_grad_{cpu,gpu}.py.

The fp32 oracle (oracle/dmvs_oracle.py) builds its pixel grid in float32 and fails on float64 inputs, so it cannot serve as
the high-precision side.  Here EVERYTHING is float64 -- projections, inverse, grid, sampling, products, sums -- on the fp32
inputs cast up, so that the distance of an fp32 implementation to this file is that implementation's whole rounding error
(projection, coordinates, interpolation, summation order).  The distance of the fp32 oracle / reference to it is ``e_oracle``,
the unit in which the product's distance is bounded.  The grid is built under no_grad like the reference's
(module.py:222-243): gradients reach the feature maps only.

Also the synthetic cases shared by the golden generator (tests/golden/make_golden_costagg_grad.py) and the tests.
"""
import numpy as np
import torch
import torch.nn.functional as F

from dmvsnet_amd import synth


def cost_agg_f64(features, proj_matrices, depth_values):
    """features: V tensors [B,C,H,W]; proj_matrices [B,V,2,4,4]; depth_values [B,D,H,W] (any float dtype; computed in float64).
    -> [B,2,D,H,W] float64."""
    feats = [f.double() for f in features]
    proj = proj_matrices.detach().double()
    depth = depth_values.detach().double()
    ref = feats[0]
    B, C, H, W = ref.shape
    D = depth.shape[1]
    total = 0
    with torch.no_grad():
        def compose(pair):   # K[:3,:3] @ E[:3,:4] into a copy of E (mvsnet.py:133-136)
            P = pair[:, 0].clone()
            P[:, :3, :4] = pair[:, 1, :3, :3] @ pair[:, 0, :3, :4]
            return P
        ref_inv = torch.inverse(compose(proj[:, 0]))
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=ref.device),
                                torch.arange(W, dtype=torch.float64, device=ref.device), indexing="ij")
        xyz = torch.stack((xx.reshape(-1), yy.reshape(-1), torch.ones(H * W, dtype=torch.float64, device=ref.device)))
    for v in range(1, len(feats)):
        with torch.no_grad():
            P = compose(proj[:, v]) @ ref_inv
            rot, trans = P[:, :3, :3], P[:, :3, 3]
            pts = (rot @ xyz.unsqueeze(0).expand(B, 3, H * W)).unsqueeze(2) * depth.reshape(B, 1, D, H * W) + trans.view(B, 3, 1, 1)
            z = pts[:, 2]
            z = torch.where(z == 0, z + 1e-5, z)   # module.py:237
            gx = pts[:, 0] / z / ((W - 1) / 2) - 1
            gy = pts[:, 1] / z / ((H - 1) / 2) - 1
            grid = torch.stack((gx, gy), dim=3).view(B, D * H, W, 2)
        warped = F.grid_sample(feats[v], grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(B, C, D, H, W)
        total = total + (warped.view(B, C // 2, 2, D, H, W) * ref.view(B, C // 2, 2, 1, H, W)).mean(1)
    return total


def grads_f64(features, proj_matrices, depth_values, gsim):
    """-> (sim float64, [dL/dfeature_v float64]) for L = <gsim, sim>."""
    leaves = [f.detach().double().requires_grad_(True) for f in features]
    sim = cost_agg_f64(leaves, proj_matrices, depth_values)
    grads = torch.autograd.grad(sim, leaves, gsim.double())
    return sim.detach(), list(grads)


def grads_of(fn, features, proj_matrices, depth_values, gsim):
    """The same through any fp32 implementation ``fn(features, proj, depth) -> sim`` under autograd."""
    leaves = [f.detach().clone().requires_grad_(True) for f in features]
    sim = fn(leaves, proj_matrices, depth_values)
    grads = torch.autograd.grad(sim, leaves, gsim)
    return sim.detach(), list(grads)


def outside_share(proj_matrices, depth_values):
    """Share of the (view, plane, pixel) samples with at least one bilinear tap outside the image (float64 coordinates)."""
    proj = proj_matrices.double()
    depth = depth_values.double()
    B, D, H, W = depth.shape

    def compose(pair):
        P = pair[:, 0].clone()
        P[:, :3, :4] = pair[:, 1, :3, :3] @ pair[:, 0, :3, :4]
        return P
    ref_inv = torch.inverse(compose(proj[:, 0]))
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    xyz = torch.stack((xx.reshape(-1), yy.reshape(-1), torch.ones(H * W, dtype=torch.float64))).to(depth.device)
    out = n = 0
    for v in range(1, proj.shape[1]):
        P = compose(proj[:, v]) @ ref_inv
        pts = (P[:, :3, :3] @ xyz.unsqueeze(0).expand(B, 3, H * W)).unsqueeze(2) * depth.reshape(B, 1, D, H * W) + P[:, :3, 3].view(B, 3, 1, 1)
        ix, iy = pts[:, 0] / pts[:, 2], pts[:, 1] / pts[:, 2]
        x0, y0 = torch.floor(ix), torch.floor(iy)
        inside = (x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1)
        out += (~inside).sum().item()
        n += inside.numel()
    return out / n


# ---------------------------------------------------------------------------------------------- synthetic cases
def turned_cameras(H, W, V):
    """synth cameras whose LAST source view sits INSIDE the sampled volume, at mid depth range, turned by 0.3 rad about the
    vertical axis: the near hypothesis planes lie behind it (z < 0: samples mirrored through its centre), the far ones in
    front; about 1 % of its samples land inside the image from behind, the rest outside.  All legal inputs."""
    cams = synth.synth_cameras(H * 4, W * 4, V)["stage1"].clone()
    a = 0.3
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    centre = np.array([10.0, 0.0, 605.0])   # camera centre in the reference frame
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ centre
    cams[0, V - 1, 0] = torch.from_numpy(E.astype(np.float32))
    return cams


def make_case(C, V, D, H, W, seed, B=1, turned=False, feature_scale=1.0):
    """Deterministic inputs of one case: features (V x [B,C,H,W]), cameras [B,V,2,4,4], hypotheses [B,D,H,W] and an upstream
    gradient [B,2,D,H,W]."""
    g = np.random.Generator(np.random.PCG64(seed))

    def rnd(*shape, scale=1.0):
        return torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(scale))
    feats = [rnd(B, C, H, W, scale=feature_scale) for _ in range(V)]
    cams = (turned_cameras(H, W, V) if turned else synth.synth_cameras(H * 4, W * 4, V)["stage1"]).repeat(B, 1, 1, 1, 1)
    step = 240.0 / D
    depth = 500.0 + step * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1) + rnd(B, D, H, W, scale=5.0)
    gsim = rnd(B, 2, D, H, W)
    return feats, cams, depth, gsim


# name -> make_case arguments of the golden cases (tests/golden/op_costagg_grad.npz)
GOLDEN_CASES = {
    "c8_v3_d4": dict(C=8, V=3, D=4, H=8, W=12, seed=11),
    "c16_v3_d8": dict(C=16, V=3, D=8, H=10, W=14, seed=12),
    "c32_v3_d4": dict(C=32, V=3, D=4, H=8, W=12, seed=13),
    "c8_v7_d8": dict(C=8, V=7, D=8, H=12, W=16, seed=14),
    "c16_v7_d4": dict(C=16, V=7, D=4, H=8, W=12, seed=15),
    "c8_v4_d8_turned": dict(C=8, V=4, D=8, H=12, W=16, seed=16, turned=True),
}

# larger synthetic cases of the GPU parity test (not stored: both sides are computed in the test's process)
LARGE_CASES = {
    "c32_v3_d48_128x160": dict(C=32, V=3, D=48, H=128, W=160, seed=21),
    "c8_v7_d8_256x320": dict(C=8, V=7, D=8, H=256, W=320, seed=22),
    "c16_v3_d8_b2_61x83": dict(C=16, V=3, D=8, H=61, W=83, seed=23, B=2),
}
