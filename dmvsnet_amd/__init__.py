"""dmvsnet_amd -- MI355X-native (gfx950) implementation of DMVSNet's cost-volume hot path.

Public surface mirrors the reference's network interface for this path
(/root/reference/networks/mvsnet.py): ``MVSNet(ndepths, depth_interval_ratio, ...)`` with
``forward(imgs, proj_matrices, depth_values) -> dict``.  The compute path is the hand-written HIP
library behind include/dmvs.h; there is no CPU or PyTorch fallback.
"""
from .mvsnet import CostAgg, CostRegNet, DepthNet, FeatureNet, MVSNet, ViewFeatures, shard_source_views  # noqa: F401

from .costagg import DiffCostAgg, cost_agg  # noqa: F401  (differentiable cost aggregation: K1 + its backward)

from . import head  # noqa: F401  (differentiable dual-depth head: K4 + K4b, and the dual-depth loss N6 + N6b)
from .head import DiffDepthNet, diff_mvs_loss  # noqa: F401

from . import conv  # noqa: F401  (differentiable convs: K3 forward / data gradient, K3g / K3h weight gradient)
from .conv import DiffConv2d, DiffConv3d, DiffConvTranspose2d, DiffConvTranspose3d  # noqa: F401

from . import bn  # noqa: F401  (differentiable BatchNorm + ReLU: K5 forward / backward, and the four U-Net blocks on it)
from .bn import (DiffBatchNormReLU2d, DiffBatchNormReLU3d, DiffConvBlock2d, DiffConvBlock3d, DiffDeconvBlock2d,  # noqa: F401
                 DiffDeconvBlock3d, DiffSyncBatchNormReLU2d, DiffSyncBatchNormReLU3d, convert_sync_batchnorm)

from . import regnet  # noqa: F401  (the four regularisation networks on the differentiable layers; conv0 / prob: K2 + K2g)
from .regnet import DiffCostRegNet, DiffCostRegNetPart, DiffCostRegNetPartRefine, DiffCostRegNetRefine  # noqa: F401

from . import featurenet  # noqa: F401  (the differentiable FeatureNet: K3 + K3f for its rectangular layers, the whole network)
from .featurenet import DiffFeatureConv2d, DiffFeatureConvBlock2d, DiffFeatureNet  # noqa: F401

from . import train  # noqa: F401  (the training model: the parts above assembled into the reference's MVSNet, and one training step)
from .train import DiffMVSNet, train_step  # noqa: F401

from . import eval_io  # noqa: F401  (PFM / cam I/O, eval dataset, Model.test step 1)
from . import fusion   # noqa: F401  (geometric-consistency fusion filter, PLY)
from . import cloud_eval  # noqa: F401  (DTU accuracy / completeness of a fused cloud)
from .cloud_eval import evaluate_dtu, max_dist_cp, point_compare, reduce_points, scan_stats  # noqa: F401
from . import validate  # noqa: F401  (Model.validate: dual-depth loss and depth metrics on ground truth)
from .validate import AbsDepthError_metrics, DTUValDataset, Thres_metrics, mvs_loss, run_validate  # noqa: F401

__all__ = ["MVSNet", "CostAgg", "CostRegNet", "DepthNet", "FeatureNet", "ViewFeatures", "shard_source_views", "eval_io", "fusion",
           "cloud_eval", "reduce_points", "max_dist_cp", "point_compare", "scan_stats", "evaluate_dtu", "validate", "mvs_loss",
           "AbsDepthError_metrics", "Thres_metrics", "DTUValDataset", "run_validate", "DiffCostAgg", "cost_agg", "head", "DiffDepthNet",
           "diff_mvs_loss", "conv", "DiffConv3d", "DiffConv2d", "DiffConvTranspose3d",
           "DiffConvTranspose2d", "bn", "DiffBatchNormReLU3d", "DiffBatchNormReLU2d", "DiffSyncBatchNormReLU3d",
           "DiffSyncBatchNormReLU2d", "convert_sync_batchnorm", "DiffConvBlock3d", "DiffDeconvBlock3d",
           "DiffConvBlock2d", "DiffDeconvBlock2d", "regnet", "DiffCostRegNetPart", "DiffCostRegNetPartRefine", "DiffCostRegNet",
           "DiffCostRegNetRefine", "featurenet", "DiffFeatureConv2d", "DiffFeatureConvBlock2d", "DiffFeatureNet", "train",
           "DiffMVSNet", "train_step"]
