"""Model level of the path: the `multiview_keypoint` branch of the reference's
`Modelbuilder` (modeling/model.py:29-58 construction, :210-247 forward, :281-302 triangulation) built MI355X-first.

What changes against the reference:
  * N1 -- the trunk runs ONCE per view.  The reference runs the whole pose ResNet twice per (reference, source) pair:
    `self.backbone(other_img)` for the source features (model.py:244) and `self.reference(img, ...)` for the fused
    pass (model.py:246), although in a multi-view batch every view's pre-fusion feature (resnet.py:406,437) is needed
    exactly once.  `forward_views` computes the trunk + deconvolution head of all views in one channels_last pass and
    hands the fused layer `feats` and `feats[source_index]` (exact in eval mode; in training it changes only which
    samples share a BN batch).  MERGE late -- the headline mode; early / both fuse layer1 features with the source's
    DECONVOLUTION features (resnet.py:390-396), which needs the unfused pass first, so they keep two passes.
  * N3 -- test-time lifting stays on the GPU: batched float64 SVD-DLT (`triangulate.py`) instead of the per-joint
    pymvg loop on the CPU (vision/triangulation.py:400-441), no device-to-host copy of the detections; with
    KEYPOINT.TRIANGULATION epipolar / epipolar_dlt the reference's `triangulate_epipolar` (:234-348), which consumes the
    layer's corr_pos, as one HIP kernel (`ops.triangulate_epipolar`); with KEYPOINT.TRIANGULATION rpsm and the batch's `rpsm`
    dict the recursive pictorial structure model (modeling/pictorial_cuda.py:222-254) on the heat maps, all frames at once
    (`ops.rpsm`); with EPIPOLAR_AMD.LIFT_KERNELS, pymvg / naive / refine (:425-441, 99-154, 162-232) as one HIP launch
    (`ops.triangulate_views`) instead of the torch DLT.
  * `EPIPOLAR.MULTITEST` (model.py:213-239): every other view in turn as the source, per joint the detection with
    the highest score -- here all (reference, source) combinations go through ONE launch of the fused layer.
  * `BACKBONE.SYNC_BN` converts through `parallel.convert_sync_batchnorm` (model.py:56-58).

The batch-dict keys are the reference's (model.py:166-207).  Training returns the reference's loss dict (`loss`: the
JointsMSELoss of modeling/metrics/metrics2d.py, renamed from `stage_loss0` as model.py:482-484 does for a single entry)
so a training loop written against Modelbuilder keeps working for this task."""
from __future__ import annotations

import torch
from torch import nn

from . import backbones, ops
from .config import get_cfg
from .triangulate import mpjpe, triangulate_dlt


# DATASETS.H36M.MAPPING (model.py:268-274): the 17 H36M joints among the 20 channels of the heads trained with it
H36M_MAPPING = (0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 12, 14, 15, 16, 17, 18, 19)


def ring_sources(num_frames: int, num_views: int, device=None) -> torch.Tensor:
    """Index of the source view of every view of a frame-major (frames * views) batch: view v+1 of the same frame
    (the pairing of the synthetic rig; H36M uses `neighbor_cameras`, vision/multiview.py:59-83 -- pass that instead)."""
    return torch.arange(num_frames * num_views, device=device).view(num_frames, num_views).roll(-1, 1).reshape(-1)


class JointsMSELoss(nn.Module):
    """modeling/metrics/metrics2d.py:18-41 JointsMSELoss: per joint the mean squared error of the visibility-weighted
    heat maps (nn.MSELoss(reduction='mean') over batch x pixels), summed over the joints and -- unless
    cfg.KEYPOINT.LOSS_PER_JOINT -- divided by their number.  (No factor 1/2: pinned by tests/golden/model_r18.npz.)"""

    def __init__(self, per_joint: bool = False):
        super().__init__()
        self.per_joint = per_joint

    def forward(self, output, target, target_weight):
        n, j = output.shape[:2]
        pred = output.reshape(n, j, -1)
        gt = target.reshape(n, j, -1)
        w = target_weight.reshape(n, j, 1)
        loss = ((pred * w - gt * w) ** 2).mean(dim=(0, 2)).sum()
        return loss if self.per_joint else loss / j


class MultiViewPoseModel(nn.Module):
    def __init__(self, cfg=None, sharded=None):
        """sharded: a `parallel.ViewShardExchange` -- this process then owns the images of ITS cameras only (one camera
        per GPU at world size = views) and the source features come through the exchange (`forward_views_sharded`);
        what the reference does with nn.DataParallel inside one process (model.py:44,246-247)."""
        super().__init__()
        self.sharded = sharded
        self.cfg = cfg = cfg if cfg is not None else get_cfg()
        assert "epipolarpose" in cfg.BACKBONE.BODY, "MultiViewPoseModel is the multiview_keypoint task of Modelbuilder"
        self.reference = backbones.build_backbone(cfg)                     # model.py:34
        self.backbone = self.reference if cfg.EPIPOLAR.SHARE_WEIGHTS else backbones.build_backbone(cfg)   # :48-57
        if cfg.BACKBONE.SYNC_BN:                                           # :56-58
            from .parallel import convert_sync_batchnorm

            convert_sync_batchnorm(self)
        self.criterion = JointsMSELoss(bool(getattr(cfg.KEYPOINT, "LOSS_PER_JOINT", False)))
        from .config import amd_knob

        if amd_knob(cfg, "LOSS_KERNELS", False):
            self.loss_kind()                                               # an unknown KEYPOINT.LOSS fails here, not at the first step

    # ------------------------------------------------------------------------------------------ N1
    def forward_views(self, img: torch.Tensor, KRT: torch.Tensor, source_index: torch.Tensor,
                      camera=None, other_camera=None):
        """All views of a batch at once.  img (M,3,Hi,Wi), KRT (M,3,4), source_index (M,) = row of the source view of
        every row.  Returns the backbone's 8-tuple (resnet.py:437) with the trunk run once per view."""
        net = self.reference
        other_KRT = KRT[source_index.to(KRT.device)]            # KRT on the host: pass a host index to avoid a sync
        from .config import amd_knob

        by_index = bool(amd_knob(self.cfg, "PAIR_INDEX", False))
        if self.cfg.EPIPOLAR.MERGE != "late" or self.backbone is not self.reference:
            with torch.set_grad_enabled(torch.is_grad_enabled() and bool(self.cfg.EPIPOLAR.OTHER_GRAD)):
                feats = self.backbone(img)[0]                               # model.py:241-244
            if by_index and self.cfg.EPIPOLAR.MERGE == "late":
                # (the source stack as it is + the index: the layer reads map source_index[n] for row n, no gathered copy)
                return net(img, [feats, other_KRT, None, KRT, camera, other_camera, None, source_index])
            return net(img, [feats[source_index], other_KRT, None, KRT, camera, other_camera, None])
        feature = net.trunk(img)                                            # once per view
        # (PAIR_INDEX: the layer names its source maps by index into the trunk's stack -- no gathered copy, made or saved for the backward)
        other, ix = (feature, {"src_index": source_index}) if by_index else (feature[source_index], {})
        if not self.cfg.EPIPOLAR.OTHER_GRAD:
            other = other.detach()
        x, corr_pos, depth, sample_locs = net._fuse(feature, net.epipolar_sampler, other, KRT, other_KRT, camera, other_camera, **ix)
        heatmap = net.final_layer(x)
        locs, scos = backbones.find_peaks(heatmap, self.cfg.KEYPOINT.SIGMA, self.cfg.BACKBONE.DOWNSAMPLE, grad=backbones.peak_grad(self.cfg))
        return feature, [heatmap], locs, scos, corr_pos, depth, sample_locs, None

    def forward_views_sharded(self, img: torch.Tensor, KRT: torch.Tensor, other_KRT: torch.Tensor, camera=None,
                              other_camera=None, num_chunks: int = 1):
        """The view-sharded partition as a model path, forward AND backward.  img (M,3,Hi,Wi): the images
        of this rank's cameras, camera-major (all frames of camera a, then of camera b, ..: `ViewShardExchange`'s pair
        order); KRT / other_KRT (M,3,4): their projection matrices and those of their source views (the ring neighbour,
        owned by another rank).  The trunk runs on the own images only; the source feature maps arrive through ONE
        all-gather (`parallel.sharded_sources`, channels-last memory as the trunk leaves it; ONE all-to-all with
        EPIPOLAR_AMD.SHARD_P2P: each map only to the rank that samples it), its backward returns
        d(source maps) to their owners with ONE all-to-all; the weight gradients of the shared network are summed by the
        caller (`parallel.allreduce_gradients` or DDP).  Returns the backbone's 8-tuple."""
        from .config import amd_knob
        from .parallel import sharded_sources

        if self.sharded is None:
            raise RuntimeError("MultiViewPoseModel was built without a ViewShardExchange (sharded=...)")
        if self.cfg.EPIPOLAR.MERGE != "late" or self.backbone is not self.reference:
            raise NotImplementedError("the view-sharded path covers MERGE late with SHARE_WEIGHTS (every configs/epipolar/*.yaml)")
        net = self.reference
        feature = net.trunk(img)                                            # own cameras only
        nhwc = feature.permute(0, 2, 3, 1).contiguous()                     # (a view when the trunk ran channels_last)
        other = sharded_sources(nhwc, self.sharded, num_chunks, p2p=bool(amd_knob(self.cfg, "SHARD_P2P", False))).permute(0, 3, 1, 2)
        if not self.cfg.EPIPOLAR.OTHER_GRAD:
            other = other.detach()
        x, corr_pos, depth, sample_locs = net._fuse(feature, net.epipolar_sampler, other, KRT, other_KRT, camera, other_camera)
        heatmap = net.final_layer(x)
        locs, scos = backbones.find_peaks(heatmap, self.cfg.KEYPOINT.SIGMA, self.cfg.BACKBONE.DOWNSAMPLE, grad=backbones.peak_grad(self.cfg))
        return feature, [heatmap], locs, scos, corr_pos, depth, sample_locs, None

    def forward_multitest(self, img: torch.Tensor, KRT: torch.Tensor, num_views: int):
        """EPIPOLAR.MULTITEST (model.py:213-239): every other view of the frame as the source in turn; per joint the
        location with the highest score.  img (F*V, ...) frame-major.  One trunk pass per network (two without
        SHARE_WEIGHTS: the sources come from `self.backbone`), ONE fused-layer launch over all F*V*(V-1)
        (reference, source) pairs."""
        net = self.reference
        m = img.shape[0]
        feature = net.trunk(img)
        # the source features come from `self.backbone` (model.py:219): the same network only with SHARE_WEIGHTS
        source = feature if self.backbone is net else self.backbone(img)[0]
        x = self._multitest_layer(feature, source, KRT, num_views)
        heat = net.final_layer(x)
        locs, scos = backbones.find_peaks(heat, self.cfg.KEYPOINT.SIGMA, self.cfg.BACKBONE.DOWNSAMPLE)
        locs = locs.view(num_views - 1, m, -1, 2)
        scos = scos.view(num_views - 1, m, -1)
        best, which = scos.max(0)                                           # model.py:233-236
        locs = torch.gather(locs, 0, which[None, ..., None].expand(-1, -1, -1, 2)).squeeze(0)
        return locs, best

    def _multitest_layer(self, feature, source, KRT, num_views: int):
        """forward_multitest's layer call: x (F*V*(V-1), C, H, W) of every (reference, source) pair, shift-major, from the
        stacks `feature` / `source` (F*V maps each, frame-major).  With EPIPOLAR_AMD.PAIR_INDEX the pairs are named by index
        into the two stacks; otherwise both operands are gathered first (2 x F*V*(V-1) maps)."""
        from .config import amd_knob

        net = self.reference
        m = feature.shape[0]
        frames = m // num_views
        by_index = bool(amd_knob(self.cfg, "PAIR_INDEX", False))
        base = torch.arange(m, device="cpu" if by_index else feature.device).view(frames, num_views)
        ref_idx, src_idx = [], []
        for shift in range(1, num_views):
            ref_idx.append(base.reshape(-1))
            src_idx.append(base.roll(-shift, 1).reshape(-1))
        ref_idx, src_idx = torch.cat(ref_idx), torch.cat(src_idx)
        Kc = KRT.to("cpu")
        camera = other_camera = None
        if self.cfg.EPIPOLAR.PRIOR or self.cfg.EPIPOLAR.SIMILARITY == "prior":
            # the learned per-camera-pair tables (epipolar.py:73-80,288-301) are keyed by the camera ids of the data set:
            # view v of a frame-major batch is cfg.DATASETS.CAMERAS[v] (multiview_h36m.py:225-252)
            ids = list(self.cfg.DATASETS.CAMERAS)
            assert len(ids) >= num_views, "EPIPOLAR.PRIOR needs DATASETS.CAMERAS to name every view"
            camera = [ids[int(i) % num_views] for i in ref_idx.tolist()]
            other_camera = [ids[int(i) % num_views] for i in src_idx.tolist()]
        if by_index:
            return net._fuse(feature, net.epipolar_sampler, source, Kc[ref_idx], Kc[src_idx], camera, other_camera,
                             ref_index=ref_idx, src_index=src_idx)[0]
        return net._fuse(feature[ref_idx], net.epipolar_sampler, source[src_idx], Kc[ref_idx.cpu()], Kc[src_idx.cpu()],
                         camera, other_camera)[0]

    # ------------------------------------------------------------------------------------------ N3
    def lift(self, batch_locs: torch.Tensor, batch_scos: torch.Tensor, KRT: torch.Tensor, num_views: int,
             corr_pos: torch.Tensor = None, other_KRT: torch.Tensor = None, *, rpsm: dict = None,
             heatmaps: torch.Tensor = None):
        """(F*V, J, 2) detections -> (F, J, 3) world points, on the device the detections live on, by the method
        cfg.KEYPOINT.TRIANGULATION names (model.py:295-311):
          epipolar / epipolar_dlt   triangulate_epipolar (vision/triangulation.py:234-348) as one HIP kernel
                                    (ops.triangulate_epipolar); needs the layer's corr_pos (F*V,H,W,2) and the projections of
                                    the source views other_KRT (F*V,3,4), with KEYPOINT.CONF_THRES / RANSAC_THRES;
          rpsm                      with the batch's `rpsm` dict (forward's docstring): the recursive pictorial structure model
                                    (modeling/pictorial_cuda.py:222-254) as HIP kernels (ops.rpsm) on the heat maps
                                    (F*V,J,H,W), with PICT_STRUCT.* and limb compatibility as a distance band instead of
                                    PICT_STRUCT.PAIRWISE_FILE; without the dict it takes the next row;
          anything else             the thresholded linear DLT of triangulate.py (the reference's `pymvg`); `naive` / `refine`
                                    take this path too -- unless EPIPOLAR_AMD.LIFT_KERNELS is set.  Then pymvg / naive /
                                    refine (:425-441, 99-154, 162-232) run as HIP kernels (ops.triangulate_views, which states
                                    how the random pairs of naive / refine are enumerated) from the detections, scores and
                                    projections alone, so all three also work with EPIPOLAR.MULTITEST; rpsm without its dict
                                    is pymvg, and an unknown name is a ValueError.
        Gradient: with EPIPOLAR_AMD.PEAK_GRAD the detections arrive attached to the heat maps (ops.heatmap_peaks(with_grad=True)),
        and every DLT lifting differentiates in them, so a loss on the lifted points reaches the network: the default route (the
        float64 torch DLT of triangulate.py, torch.linalg.svd) through torch's autograd, the HIP liftings pymvg / naive / refine
        (ops.triangulate_views) and epipolar / epipolar_dlt (ops.triangulate_epipolar) through one HIP kernel
        (et_triangulate_bwd), called with with_grad=True exactly when PEAK_GRAD is set.  It is the gradient of the DLT the
        forward settled on -- the selected views, the winning pair, the inliers, or the one view with its correspondence -- in
        the detections that DLT used; the selection, the scores, the projections and corr_pos are constants.  ops.rpsm returns
        no gradient: a grid search has none."""
        cfg = self.cfg
        grad = {"with_grad": True} if backbones.peak_grad(cfg) else {}     # (PEAK_GRAD off: exactly the calls without the keyword)
        m, j, _ = batch_locs.shape
        f = m // num_views
        scale = float(cfg.DATASETS.IMAGE_RESIZE) * float(cfg.DATASETS.PREDICT_RESIZE)
        pts = (batch_locs * scale).view(f, num_views, j, 2)
        method = getattr(cfg.KEYPOINT, "TRIANGULATION", "naive")
        if method in ("epipolar", "epipolar_dlt"):
            if corr_pos is None or other_KRT is None:
                raise ValueError("KEYPOINT.TRIANGULATION %s needs the layer's corr_pos and the source views' projections; "
                                 "EPIPOLAR.MULTITEST keeps neither (every other view is the source in turn): use pymvg with it"
                                 % method)
            dev = batch_locs.device
            planes = lambda t: t.to(dev, torch.float32).reshape(f, num_views, 3, 4).contiguous()
            return ops.triangulate_epipolar(
                pts.contiguous(), batch_scos.reshape(f, num_views, j).contiguous(), planes(KRT), planes(other_KRT),
                corr_pos.reshape(f, num_views, *corr_pos.shape[-3:]).contiguous(), downsample=float(cfg.BACKBONE.DOWNSAMPLE),
                resize=scale, conf_thres=float(getattr(cfg.KEYPOINT, "CONF_THRES", 0.05)),
                ransac_thres=float(getattr(cfg.KEYPOINT, "RANSAC_THRES", 3)), dlt=method == "epipolar_dlt", **grad)
        if method == "rpsm" and rpsm is not None:
            if heatmaps is None:
                raise ValueError("KEYPOINT.TRIANGULATION rpsm scores the heat maps, and EPIPOLAR.MULTITEST keeps none (every other "
                                 "view is the source in turn): use pymvg with it")
            from . import pictorial
            from .config import amd_knob

            dev, ps = heatmaps.device, cfg.PICT_STRUCT
            image_size = tuple(cfg.DATASETS.IMAGE_SIZE)
            f32 = lambda t, *shape: torch.as_tensor(t).to(dev, torch.float32).reshape(*shape).contiguous()
            limbs = lambda t: None if t is None else f32(t, *((-1, j - 1) if torch.as_tensor(t).dim() > 1 else (j - 1,)))
            return ops.rpsm(
                heatmaps.detach().to(torch.float32).reshape(f, num_views, *heatmaps.shape[-3:]).contiguous(),
                f32(rpsm["cameras"], f, num_views, 3, 4),
                pictorial.crop_transform(f32(rpsm["crop_center"], f, num_views, 2), f32(rpsm["crop_scale"], f, num_views, -1),
                                         image_size).contiguous(),
                f32(rpsm["center"], f, 3), limbs(rpsm["limb_length"]), first_limb_length=limbs(rpsm.get("first_limb_length")),
                parent=rpsm.get("parent"), image_size=image_size, grid_size=float(ps.GRID_SIZE), first_nbins=int(ps.FIRST_NBINS),
                recur_nbins=int(ps.RECUR_NBINS), recur_depth=int(ps.RECUR_DEPTH), tolerance=float(ps.LIMB_LENGTH_TOLERANCE),
                align_corners=bool(amd_knob(cfg, "ALIGN_CORNERS", False)))
        from .config import amd_knob

        if amd_knob(cfg, "LIFT_KERNELS", False):
            if method == "rpsm":
                method = "pymvg"
            if method not in ops.VIEW_METHODS:
                raise ValueError("KEYPOINT.TRIANGULATION %r is none of %s" % (
                    method, ", ".join(["epipolar", "epipolar_dlt", "rpsm"] + list(ops.VIEW_METHODS))))
            dev = batch_locs.device
            return ops.triangulate_views(
                pts.contiguous(), batch_scos.reshape(f, num_views, j).contiguous(),
                KRT.to(dev, torch.float32).reshape(f, num_views, 3, 4).contiguous(), method=method,
                conf_thres=float(getattr(cfg.KEYPOINT, "CONF_THRES", 0.05)),
                ransac_thres=float(getattr(cfg.KEYPOINT, "RANSAC_THRES", 3)), **grad)
        return triangulate_dlt(pts, KRT.to(batch_locs.device).view(f, num_views, 3, 4), batch_scos.view(f, num_views, j),
                               conf_thres=float(getattr(cfg.KEYPOINT, "CONF_THRES", 0.05)))

    # ------------------------------------------------------------------------------------------ test-time 2-D metrics
    def metrics_2d(self, inputs: dict, heat, target_heat, batch_locs, visibility, metric_dict: dict, out: dict):
        """The `cfg.TEST.PCK` block of Modelbuilder.forward (model.py:372-404; PCK defaults to True) on the device, into
        `metric_dict` / `out`: JDR of the predicted against the target heat maps (ops.eval_jdr; not under EPIPOLAR.MULTITEST, which
        keeps no maps) and, with the batch's `points-2d`, calculate_err -- the reference's DOTEST branch, its default -- on the
        detections (ops.eval_pck): PCK@<th> for cfg.TEST.THRESHOLDS, err_joints / total_joints for cfg.TEST.MAX_TH.  The values
        are device tensors; nothing is copied to the host."""
        test = self.cfg.get("TEST") if hasattr(self.cfg, "get") else None
        if not getattr(test, "PCK", True):
            return
        if heat is not None and target_heat is not None:
            dev = heat[0].device
            _, acc = ops.eval_jdr(heat[0].detach().to(torch.float32).contiguous(), target_heat.to(dev, torch.float32).contiguous())
            metric_dict["JDR"], out["jdr_per_joint"] = acc[0], acc[1:]
        if inputs.get("points-2d") is not None:
            thresholds = tuple(getattr(test, "THRESHOLDS", (1, 2, 5, 10, 20, 30, 40, 50, 60, 80, 100)))
            locs = batch_locs.detach().to(torch.float32).contiguous()
            gt = inputs["points-2d"][..., :2].to(locs.device, torch.float64).contiguous()
            pck, out["err_joints"], out["total_joints"] = ops.eval_pck(locs, gt, vis=visibility, thresholds=thresholds,
                                                                       max_threshold=getattr(test, "MAX_TH", 20))
            for i, th in enumerate(thresholds):
                metric_dict["PCK@" + str(th)] = pck[i]

    # ------------------------------------------------------------------------------------------ training loss
    def loss_kind(self) -> str:
        """KEYPOINT.LOSS (model.py:59-71): joint when absent, smoothmse or mse; anything else is a ValueError."""
        kind = getattr(self.cfg.KEYPOINT, "LOSS", "joint")
        if kind not in ops.LOSS_KINDS:
            raise ValueError("KEYPOINT.LOSS %r is none of %s" % (kind, ", ".join(ops.LOSS_KINDS)))
        return kind

    def kernel_losses(self, inputs: dict, heat, loss_dict: dict):
        """The training loss of Modelbuilder.forward (model.py:249-258) through ops.heatmap_loss, into `loss_dict`: the criterion
        KEYPOINT.LOSS names -- joint and smoothmse on heat[0] as `stage_loss0`, weighted by `visibility` (M,J) or (M,J,1); mse as
        compute_stage_loss does, `stage_loss{i}` for every map of `heat`, visibility ignored (the reference's non-H36M call: its
        H36M branch raises under mse).  The target is the batch's `heatmap`; without it `points-2d` (M,J,>=2), from which the
        kernels make Heatmapcreator's target on the fly with KEYPOINT.SIGMA, BACKBONE.DOWNSAMPLE and the predicted map's own
        size; without both there is no loss."""
        kind = self.loss_kind()
        target, points = inputs.get("heatmap"), inputs.get("points-2d")
        if target is None and points is None:
            return
        dev = heat[0].device
        how = {}
        if target is not None:
            target = target.to(dev, torch.float32).contiguous()
        else:
            how = dict(points=points[..., :2].to(dev, torch.float64).contiguous(), sigma=float(self.cfg.KEYPOINT.SIGMA),
                       downsample=float(self.cfg.BACKBONE.DOWNSAMPLE))
        vis = inputs.get("visibility")
        if kind == "mse" or vis is None:
            vis = None
        else:
            vis = vis.to(dev, torch.float32).reshape(heat[0].shape[:2]).contiguous()
        per_joint = bool(getattr(self.cfg.KEYPOINT, "LOSS_PER_JOINT", False))
        for i, maps in enumerate(heat if kind == "mse" else heat[:1]):
            loss_dict["stage_loss%d" % i] = ops.heatmap_loss(maps.to(torch.float32), target, vis, kind=kind, per_joint=per_joint, **how)

    # ------------------------------------------------------------------------------------------ Modelbuilder.forward
    def forward(self, inputs: dict, is_train: bool = True):
        """The multiview_keypoint branch of Modelbuilder.forward (model.py:160-302).  `inputs` holds the reference's
        keys: img, KRT, and either `other_index` (rows of the source views inside `img`: the de-duplicated path) or
        `other_img` + `other_KRT` (the reference's two-pass form); optional heatmap / visibility (loss) and points-3d
        (MPJPE); optional `rpsm`, what KEYPOINT.TRIANGULATION rpsm needs (model.py:312-334): a dict of `cameras` (F*V,3,4: origK @ RT),
        `crop_center` (F*V,2), `crop_scale` (F*V,2) or (F*V,), `center` (F,3), `limb_length` (F,J-1) or (J-1,) and optionally
        `first_limb_length`, `parent` -- the reference takes centre and limb lengths from the first frame's ground truth, here
        the caller supplies them per frame.  Returns (loss_dict, metric_dict) in training, (loss_dict, metric_dict, out) otherwise, as the reference does
        (model.py:478-493).

        EPIPOLAR_AMD.EVAL_METRICS (default off: everything above is all there is) adds, in evaluation, the rest of the reference's
        test-time branch, computed on the device with no copy to the host:
          * DATASETS.H36M.MAPPING (model.py:268-274), when the key is present and true (absent counts as false): the predicted heat
            maps, the target `heatmap`, the detections, their scores and `visibility` are reduced to the 17 channels H36M_MAPPING
            before the lift and before any metric; a head with other than 20 channels is a ValueError.  The reference also tests
            `'h36m' in cfg.OUTPUT_DIR`, its switch between data sets; this model IS the H36M task, so that test is dropped.
          * metric_dict["EPEmean_global"] and out["epe_per_joint"] (F,J) from ops.eval_epe (EPEmean, model.py:339-346), given a lift
            and `points-3d`; `unit` = inputs.get("unit") or 1, a host number; the clamp is cfg.TEST.EPEMEAN_MAX_DIST (150 when
            absent); visibility is that of each frame's first view, like `points-3d`.  "MPJPE" stays.  The reference drops the
            key when the value is NaN (:345), a test that needs the value on the host: here the key is always written and a NaN
            stays a NaN.
          * unless cfg.TEST.PCK is false (absent counts as true, the reference's default): `metrics_2d` -- "JDR" and
            out["jdr_per_joint"] given a target `heatmap`, "PCK@<th>", out["err_joints"] and out["total_joints"] given `points-2d`
            (M,J,>=2; the J joints that remain after the mapping).
        The per-action and per-joint-name keys (MPJPE@<action>, JDR@<name>) need the data set's name tables and are not written.

        EPIPOLAR_AMD.LOSS_KERNELS (default off: training computes the torch JointsMSELoss above from `heatmap`) takes the training
        loss from the HIP kernels instead (`kernel_losses`): KEYPOINT.LOSS joint | smoothmse | mse is read, and a batch without
        `heatmap` but with `points-2d` gets its target made on the device, never stored."""
        cfg = self.cfg
        img = inputs["img"]
        KRT = inputs["KRT"].to(torch.float32)                               # model.py:183-185
        camera, other_camera = inputs.get("camera"), inputs.get("other_camera")
        views = int(inputs.get("num_views", len(cfg.DATASETS.CAMERAS) or 4))
        if cfg.EPIPOLAR.MULTITEST and not is_train:
            with torch.no_grad():
                batch_locs, batch_scos = self.forward_multitest(img, KRT, views)
            heat = corr_pos = depths = other_KRT = None
        else:
            if self.sharded is not None and "other_img" not in inputs and "other_index" not in inputs:
                other_KRT = inputs["other_KRT"].to(torch.float32)
                res = self.forward_views_sharded(img, KRT, other_KRT, camera, other_camera, int(inputs.get("exchange_chunks", 1)))
            elif "other_index" in inputs:
                other_KRT = KRT[inputs["other_index"].to(KRT.device)]
                res = self.forward_views(img, KRT, inputs["other_index"], camera, other_camera)
            else:
                other_KRT = inputs["other_KRT"].to(torch.float32)
                with torch.set_grad_enabled(torch.is_grad_enabled() and bool(cfg.EPIPOLAR.OTHER_GRAD)):
                    other_features = self.backbone(inputs["other_img"])[0]                           # model.py:244
                res = self.reference(img, [other_features, other_KRT, None, KRT, camera, other_camera, inputs["other_img"]])  # model.py:246
            _, heat, batch_locs, batch_scos, corr_pos, depths, _, _ = res
        loss_dict, metric_dict, out = {}, {}, {}
        from .config import amd_knob

        evaluate = not is_train and bool(amd_knob(cfg, "EVAL_METRICS", False))
        target_heat, visibility = inputs.get("heatmap"), inputs.get("visibility")
        if evaluate:
            m = batch_locs.shape[0]
            if visibility is not None:
                visibility = visibility.to(batch_locs.device, torch.float32).reshape(m, -1)            # model.py:181
            h36m = cfg.DATASETS.get("H36M") if hasattr(cfg.DATASETS, "get") else None
            if h36m is not None and h36m.get("MAPPING", False):                                          # model.py:268-274
                if batch_locs.shape[1] != 20:
                    raise ValueError("DATASETS.H36M.MAPPING takes the 17 H36M joints out of a 20-channel head; this head has %d "
                                     "channels" % batch_locs.shape[1])
                keep = torch.tensor(H36M_MAPPING, device=batch_locs.device)
                take = lambda t: None if t is None else t.index_select(1, keep.to(t.device))
                if heat is not None:
                    heat = [take(heat[0])] + list(heat[1:])
                target_heat, batch_locs, batch_scos, visibility = take(target_heat), take(batch_locs), take(batch_scos), take(visibility)
        if is_train and amd_knob(cfg, "LOSS_KERNELS", False):
            self.kernel_losses(inputs, heat, loss_dict)
        elif is_train and inputs.get("heatmap") is not None:
            vis = inputs.get("visibility")
            vis = torch.ones(heat[0].shape[:2], device=heat[0].device) if vis is None else vis.to(torch.float32)
            loss_dict["stage_loss0"] = self.criterion(heat[0], inputs["heatmap"].to(torch.float32), vis)   # model.py:253
        # the reference's keys (model.py:362-373: heatmap_pred, corr_pos, depth, batch_locs, score_pred) + two aliases
        out.update(heatmap_pred=heat[-1] if heat is not None else None, corr_pos=corr_pos, depth=depths,
                   batch_locs=batch_locs, score_pred=batch_scos, batch_scos=batch_scos,
                   heatmaps=heat[0] if heat is not None else None)
        if not is_train and cfg.VIS.MULTIVIEW:
            pred = self.lift(batch_locs, batch_scos, KRT, views, corr_pos, other_KRT, rpsm=inputs.get("rpsm"),
                             heatmaps=heat[0] if heat is not None else None)
            out["points-3d"] = pred
            if inputs.get("points-3d") is not None:
                gt = inputs["points-3d"].to(pred.device).view(-1, views, pred.shape[1], 3)[:, 0]
                metric_dict["MPJPE"] = mpjpe(pred, gt)                      # metrics3d.py:5-46
                if evaluate:                                                # model.py:339-346
                    test = cfg.get("TEST") if hasattr(cfg, "get") else None
                    vis = None if visibility is None else visibility.view(-1, views, visibility.shape[1])[:, 0].contiguous()
                    metric_dict["EPEmean_global"], out["epe_per_joint"] = ops.eval_epe(
                        pred.to(torch.float64).contiguous(), gt.to(torch.float64).contiguous(), vis=vis,
                        unit=float(inputs.get("unit") or 1), max_dist=float(getattr(test, "EPEMEAN_MAX_DIST", 150)))
        if evaluate:
            self.metrics_2d(inputs, heat, target_heat, batch_locs, visibility, metric_dict, out)
        # model.py:478-493: several losses are summed into 'loss', a single one is RENAMED to 'loss'; training returns
        # (loss_dict, metric_dict), evaluation (loss_dict, metric_dict, out) with the empty entries of `out` dropped
        if len(loss_dict) > 1:
            loss_dict["loss"] = sum(loss_dict.values())
        elif len(loss_dict) == 1:
            loss_dict["loss"] = loss_dict.popitem()[1]
        if is_train:
            return loss_dict, metric_dict
        return loss_dict, metric_dict, {k: v for k, v in out.items() if v is not None}
