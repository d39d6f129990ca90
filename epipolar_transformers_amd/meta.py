"""The Meta fusion layer (modeling/layers/meta.py:9-57), the learned-fusion baseline of the `metaHG*` backbones: per (reference,
source) pair a 256 x 256 weight made from the pair's fundamental matrix by two small linear layers, applied to the source map as a
1x1 convolution, plus a shared 1x1 convolution:

    ret_n = (W_n + W_share) . other_n + b_share        W_n = fc1(relu(fc0(F_n))).view(C, C)

The embedding (`camera.fundamental_matrices`: float32 on the host, the reference's ops in the reference's order) and the two linear
layers are stock torch; the data pass -- the reference's Python loop of N conv2d calls, the shared convolution and the adds, with
the hourglass caller's `ret + feat` (ProHG.py:219-220,239) folded in -- is ONE HIP GEMM with a weight per pair (`ops.meta_fuse`:
et_meta_pack / et_meta_gemm, backward et_meta_gemm on the transposed packs and et_meta_wgrad).

Parameter names as in the reference (`fc0`, `fc1`, `share`), so a reference checkpoint loads; its `self.bias` is a plain zero tensor,
neither a parameter nor in the state dict, and is left out.
"""
from __future__ import annotations

import torch
from torch import nn
import torch.nn.functional as F

from . import camera, ops


class Meta(nn.Module):
    embedding_size = 9
    hidden_size = 100

    def __init__(self, in_channels):
        super().__init__()
        if in_channels != 256:
            raise ValueError("the Meta fusion layer's kernels are written for the 256-channel head: KEYPOINT.NFEATS must be 256, "
                             "got %d" % in_channels)
        self.shape = [in_channels, in_channels, 1, 1]
        self.fc0 = nn.Linear(self.embedding_size, self.hidden_size)
        self.fc1 = nn.Linear(self.hidden_size, in_channels * in_channels)
        self.share = nn.Conv2d(in_channels, in_channels, 1)
        self._fundamental = camera.PairAlgebraCache(algebra=camera.fundamental_matrices)

    def forward(self, KRT, other_KRT, input, feat=None, fundamental=None):
        """KRT, other_KRT: (N,3,4); input: the source maps (N,C,H,W); feat: the reference maps the caller adds (`ret + feat`), fused
        into the same pass; fundamental: (N,3,3) in place of `camera.fundamental_matrices(KRT, other_KRT)`.  Returns (N,C,H,W)."""
        N, C, H, W = input.shape
        if fundamental is None:
            fundamental = self._fundamental.get(KRT, other_KRT, input.device)
        emb = fundamental.reshape(-1, self.embedding_size).to(device=input.device, dtype=input.dtype)
        if emb.shape[0] != N:
            raise ValueError("%d fundamental matrices for %d maps" % (emb.shape[0], N))
        weight = self.fc1(F.relu(self.fc0(emb))).view(N, C, C)
        rows = lambda t: t.permute(0, 2, 3, 1).contiguous()          # (a view when the map is channels_last)
        x = ops.meta_fuse(rows(input), weight, self.share.weight, self.share.bias, None if feat is None else rows(feat))
        return x.permute(0, 3, 1, 2)

    def __repr__(self):
        return self.__class__.__name__ + "(size=" + str(self.shape) + ")"
