"""``SGCDet`` detector shell: the three calls of the reference that form the hot path.

Reference: mmdet3d_plugin/models/detectors/SGCDet.py:61-129.  The 2D backbone (mmdet's ResNet -- not in the reference tree) is
NOT built by the constructor: its config is accepted and kept, and ``attach_backbone()`` builds it on request
(plugin/resnet.py); with it attached, ``build_volume`` / ``simple_test`` / ``forward_train`` take the reference's ``batch``
dict from images on.  ``depth_head``
(``DepthNet_Fusion``, row f-2 of SURVEY.md section 8) IS built when configured: ``build_volume_from_fpn`` runs it on the
finest FPN map + the images (SGCDet.py:71-85) and hands its depth distribution to the path -- in inference on the GPU its
2-D CNNs run on the library's MFMA kernels and the distribution is channels-last in memory (plugin/depth_net.py), which
``depth_pyramid`` keeps zero-copy.  The path itself starts
from FPN maps ``x[l] = [1,N,C,H_l,W_l]`` and the depth distribution ``[1,N,D,H_0,W_0]``:

    volume, valid, occ = voxel_head(x, img_metas[0], mlvl_dpt_dists)      # SGCDet.py:87
    feats = neck_3d(volume)                                               # :96
    outs  = bbox_head(feats); bbox_head.get_bboxes(*outs, valid.float(), img_metas)  # :123-124
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..mmcv_lite import DETECTORS, build_backbone, build_head, build_neck


@DETECTORS.register_module()
class SGCDet(nn.Module):
    def __init__(self, backbone=None, neck=None, depth_head=None, neck_3d=None, bbox_head=None, n_voxels=None,
                 voxel_size=None, voxel_head=None, head_2d=None, train_cfg=None, test_cfg=None,
                 use_gt_dpt=False, depth_loss=False, occ_loss=False, lighting_augmentation=False):
        super().__init__()
        self.upstream_cfg = dict(backbone=backbone, neck=neck, depth_head=depth_head, head_2d=head_2d)
        # the image FPN (row f-1): built when the config names the plain FPN; the backbone stays a config entry until
        # ``attach_backbone()`` is called
        self.backbone = None
        self.neck = build_neck(neck) if isinstance(neck, dict) and neck.get("type") == "FPN" else None
        self.depth_head = build_head(depth_head) if depth_head is not None else None
        self.use_gt_dpt, self.depth_loss = use_gt_dpt, depth_loss
        self.neck_3d = build_neck(neck_3d)
        bbox_head = dict(bbox_head)
        bbox_head.update(train_cfg=train_cfg, test_cfg=test_cfg)
        self.bbox_head = build_head(bbox_head)
        self.bbox_head.voxel_size = voxel_size
        self.voxel_head = build_head(voxel_head) if voxel_head is not None else None
        self.n_voxels = n_voxels
        self.voxel_size = voxel_size
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.occ_loss = occ_loss

    # ---- the 2-D backbone: opt-in, images -> the maps the FPN reads (row f-0) --------------------------------------------
    def attach_backbone(self, cfg=None):
        """Build ``self.backbone`` from ``cfg`` (or from the ``backbone`` entry the constructor kept) and register it as a
        submodule: ``state_dict()`` then carries the reference's ``backbone.*`` keys (a released checkpoint loads whole) and
        ``optim.build_optimizer`` finds its 0.1 x lr group.  The constructor does not do this: a detector fed from feature
        maps carries no backbone.  Returns ``self``."""
        cfg = cfg if cfg is not None else self.upstream_cfg.get("backbone")
        if cfg is None:
            raise RuntimeError("SGCDet.attach_backbone: no backbone config was given and the detector was built without one")
        self.backbone = build_backbone(cfg)
        return self

    def _need_backbone(self, who):
        if self.backbone is None:
            raise RuntimeError(f"SGCDet.{who}: no backbone is attached -- call attach_backbone() first, or feed feature maps "
                               "(simple_test_from_features, build_volume_from_fpn, forward_train_from_fpn)")
        if self.upstream_cfg.get("head_2d") is not None:
            raise NotImplementedError("SGCDet: head_2d is not built (the SGCDet configs set none)")

    def extract_img_feat(self, img):
        """img [B, N, 3, H, W] -> FPN maps [[B, N, C, H_l, W_l], ...] (SGCDet.py:62-69).  The reference's voxel head is batch 1 by
        assertion and its step is one scene per rank; here a batch is B scenes on one device: the image side sees
        B * N images, the voxel head runs scene by scene, neck_3d and the head on the batch."""
        self._need_backbone("extract_img_feat")
        return self.image_features(self.backbone(img.reshape([-1] + list(img.shape)[2:])), batch=img.shape[0])

    def build_volume(self, batch):
        """SGCDet.build_volume (SGCDet.py:61-94): ``batch`` = dict(img [B,N,3,H,W], img_metas, depth_maps for ``use_gt_dpt``)
        -> (volume, valid, features_2d = None, dpt_dist, occ)."""
        self._need_backbone("build_volume")
        x = self.extract_img_feat(batch["img"])
        volume, valid, dpt_dist, occ = self.build_volume_from_fpn(x, batch["img"], batch["img_metas"], batch.get("depth_maps"))
        return volume, valid, None, dpt_dist, occ

    def simple_test(self, batch):
        """SGCDet.simple_test (SGCDet.py:119-129): images -> ``bbox3d2result`` dicts."""
        self._need_backbone("simple_test")
        x = self.extract_img_feat(batch["img"])
        dpt_dist = self.depth_distribution(x, batch["img"], batch["img_metas"], batch.get("depth_maps"))
        return self.simple_test_from_features(x, batch["img_metas"], dpt_dist, as_results=True)

    def forward_test(self, batch):
        return self.simple_test(batch)

    def forward_train(self, batch):
        """SGCDet.forward_train (SGCDet.py:98-114): the losses of a batch from images on.  The backbone trains on the HIP
        kernels when its norms are frozen (plugin/resnet.py ``_forward_hip_train``), so the step's weight planes are repacked
        here, before it runs."""
        self._need_backbone("forward_train")
        if self.training and torch.is_grad_enabled():
            from ..functions import train_weight_planes
            train_weight_planes().begin_step()
            self._step_begun = True                    # build_volume_from_features does not begin the step a second time
        try:
            x = self.extract_img_feat(batch["img"])
            return self.forward_train_from_fpn(x, batch["img"], batch["img_metas"], batch["gt_bboxes_3d"], batch["gt_labels_3d"],
                                               batch.get("depth_maps"))
        finally:
            self._step_begun = False

    def image_features(self, backbone_feats, batch=1):
        """Backbone maps [[B*N, C_l, H_l, W_l], ...] -> [[B, N, C, H, W], ...] as SGCDet.py:67-69.  In eval mode on
        the GPU the FPN's convolutions emit channels-last memory (plugin/fpn.py), which the view transformation reads in
        place; the reshape keeps that memory format (per scene: ``f[b:b+1]`` of a batch is the B = 1 tensor of scene b)."""
        if self.neck is None:
            raise RuntimeError("SGCDet.image_features: the config has no FPN neck")
        if batch == 1:
            return [f.unsqueeze(0) for f in self.neck(backbone_feats)]
        return [f.unflatten(0, (batch, -1)) for f in self.neck(backbone_feats)]

    @staticmethod
    def depth_pyramid(dpt_dist):
        """nearest x1/2, x1/4 copies of the depth distribution (SGCDet.py:83-85)."""
        if dpt_dist.dim() == 5 and dpt_dist.shape[0] == 1 and dpt_dist[0].is_contiguous(memory_format=torch.channels_last) \
                and not dpt_dist[0].is_contiguous():
            # channels-last producer: the 2-D nearest resize picks the same elements and keeps
            # the memory format, so the coarse levels stay zero-copy for the gathers too
            return [dpt_dist,
                    F.interpolate(dpt_dist[0], scale_factor=0.5, mode="nearest").unsqueeze(0),
                    F.interpolate(dpt_dist[0], scale_factor=0.25, mode="nearest").unsqueeze(0)]
        if dpt_dist.is_cuda and not torch.is_grad_enabled() and dpt_dist.dim() == 5:
            # nearest x1/2, x1/4 == every 2nd / 4th pixel (src index = floor(dst * 2)): strided VIEWS of the full-resolution
            # map; the per-level crop + transpose kernel reads them in place (sgc_nchw_to_nhwc_crop, `step`)
            H, W = dpt_dist.shape[-2:]
            return [dpt_dist, dpt_dist[..., ::2, ::2][..., :H // 2, :W // 2], dpt_dist[..., ::4, ::4][..., :H // 4, :W // 4]]
        return [dpt_dist,
                F.interpolate(dpt_dist, scale_factor=(1, 0.5, 0.5), mode="nearest"),
                F.interpolate(dpt_dist, scale_factor=(1, 0.25, 0.25), mode="nearest")]

    def depth_distribution(self, x, img, img_metas, depth_maps=None, stride=4):
        """SGCDet.build_volume's depth branch (SGCDet.py:71-82): x = FPN maps [B,N,C,H_l,W_l], img [B,N,3,4H,4W] ->
        dpt_dist [B,N,D,H_0,W_0] from ``depth_head`` (or from the ground-truth depth maps with ``use_gt_dpt``)."""
        if self.depth_head is None:
            raise RuntimeError("SGCDet was built without a depth_head config")
        if self.use_gt_dpt:
            b, n, _, h, w = x[0].shape
            return self.depth_head.get_downsampled_gt_depth(depth_maps).view(b, n, h, w, -1).permute(0, 1, 4, 2, 3)
        xs = x[0].detach() if self.depth_loss else x[0]
        return self.depth_head(xs=xs, imgs=img, img_metas=img_metas, stride=stride)

    def build_volume_from_fpn(self, x, img, img_metas, depth_maps=None):
        """FPN maps + images -> (volume, valid, dpt_dist, occ): the reference's build_volume from the FPN output on."""
        dpt_dist = self.depth_distribution(x, img, img_metas, depth_maps)
        volume, valid, occ = self.build_volume_from_features(x, img_metas, dpt_dist)
        return volume, valid, dpt_dist, occ

    def build_volume_from_features(self, x, img_metas, dpt_dist):
        if self.training and torch.is_grad_enabled() and not getattr(self, "_step_begun", False):
            # a training step begins: every weight plane the HIP training Functions have registered is repacked in ONE launch
            from ..functions import train_weight_planes
            train_weight_planes().begin_step()
        B = x[0].shape[0]
        if B == 1:
            volume, valid, occ = self.voxel_head(x, img_metas[0], self.depth_pyramid(dpt_dist))
        else:
            if len(img_metas) != B or dpt_dist.shape[0] != B:
                raise RuntimeError(f"SGCDet: {B} scenes of feature maps, {len(img_metas)} img_metas, {dpt_dist.shape[0]} depth distributions")
            # the voxel head is batch 1 (AdaptiveSparseHead.py:45, DenseHead.py:60): scene by scene, stacked
            per = [self.voxel_head([f[b:b + 1] for f in x], img_metas[b], self.depth_pyramid(dpt_dist[b:b + 1])) for b in range(B)]
            volume = torch.cat([p[0] for p in per])
            valid = None if any(p[1] is None for p in per) else torch.cat([p[1] for p in per])
            occ = None if any(p[2] is None for p in per) else torch.cat([p[2] for p in per])
        if valid is None:
            _, _, vh, vw, vz = volume.shape
            valid = torch.ones([volume.shape[0], 1, vh, vw, vz], device=volume.device)
        return volume, valid, occ

    def extract_feat(self, volumes):
        return self.neck_3d(volumes)

    # ---- hipGraph replay of the static-shape tail (neck + head: ~30 launches, fixed shapes) -----------
    use_graph = True

    # opt-in: output-masked decoder tail (north star: "sparse 3D convolution over the occupancy-masked voxels").  The head
    # tensors are then only defined where the head's valid pyramid is 1 -- exactly where get_bboxes consumes them
    # (imvoxel_head_v2.py:258,301); decoded boxes are identical to the dense path (tests/test_gpu_modules.py).
    masked_tail = False

    def _tail_masks(self, valid):
        """(neck masks, head masks) from the finest valid [1,1,X,Y,Z] int64: head scale s needs valid@s; out_block_0 needs
        the 3x3x3 dilation of valid@0 (the head conv reads one voxel around every valid one), up_block_1's conv one more."""
        from .. import ext
        ops = ext.ops()
        grid = tuple(valid.shape[-3:])
        flat = valid.reshape(-1)
        head = [ops.valid_pyramid(flat, grid, 2 ** s) for s in range(self.bbox_head.n_scales)]
        d1 = ops.mask_dilate3(head[0], grid)
        d2 = ops.mask_dilate3(d1, grid)
        return (d2, d1), head

    def _neck_head_eager(self, volume, valid=None):
        if valid is not None and self.masked_tail and not self.training and volume.is_cuda:
            neck_masks, head_masks = self._tail_masks(valid)
            outs = self.bbox_head(self.neck_3d(volume, neck_masks), head_masks)
        else:
            outs = self.bbox_head(self.extract_feat(volume))
        return tuple(list(o) for o in outs)

    def _neck_head(self, volume):
        """neck_3d + bbox_head.  In eval / no-grad on the GPU the launch sequence is captured once into a
        hipGraph per input shape and replayed (one host call instead of ~30 kernel launches plus their
        Python orchestration).  Outputs then live in the graph's static buffers: they are overwritten by the
        next call, so consume (or clone) them before calling again."""
        if (not self.use_graph) or self.training or torch.is_grad_enabled() or not volume.is_cuda:
            return self._neck_head_eager(volume)
        from .conv_plan import CONV_MODE, module_fingerprint
        # one graph (and one set of static buffers) per stream: scenes in flight on different streams
        # must not share replay buffers
        key = (tuple(volume.shape), tuple(volume.stride()), CONV_MODE, module_fingerprint(self.neck_3d),
               module_fingerprint(self.bbox_head), torch.cuda.current_stream().cuda_stream)
        cache = self.__dict__.setdefault("_graph_cache", {})
        entry = cache.get(key)
        if entry is None:
            if len(cache) >= 16:
                # evict the oldest graph -- only after the device is idle: destroying a graph hands its private
                # memory pool back to the allocator, which must not happen while a replay is still running
                torch.cuda.synchronize()
                cache.pop(next(iter(cache)))
            static_in = torch.empty_strided(volume.shape, volume.stride(), dtype=volume.dtype, device=volume.device)
            static_in.copy_(volume)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                 # warm-up outside capture (plans, attributes, allocator)
                self._neck_head_eager(static_in)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                outs = self._neck_head_eager(static_in)
            entry = cache[key] = (graph, static_in, outs)
        graph, static_in, outs = entry
        static_in.copy_(volume)
        graph.replay()
        return outs

    # ---- whole-scene hipGraph: voxel head + neck + head as ONE replay, no host read-backs ------------------
    scene_graph = False      # opt-in: outputs live in the graph's static buffers until the next replay on it
    scene_graph_capacity = 8 # graphs that alias their input buffers; callers beyond that share input-copying graphs

    def _scene_graph_key(self, x, img_metas, dpt_dist, aliased):
        from .conv_plan import CONV_MODE, module_fingerprint
        meta = img_metas[0]
        n_views = len(meta["lidar2img"]["extrinsic"])
        tensors = list(x) + [dpt_dist]
        return (tuple((t.data_ptr() if aliased else 0, tuple(t.shape), tuple(t.stride()), t.dtype) for t in tensors),
                tuple(meta["img_shape"][:2]), tuple(meta["ori_shape"][:2]), n_views, CONV_MODE,
                module_fingerprint(self.voxel_head), module_fingerprint(self.neck_3d), module_fingerprint(self.bbox_head),
                torch.cuda.current_stream().cuda_stream)

    def _capture_scene_graph(self, x, img_metas, dpt_dist):
        from .voxformer import scene_constants_host
        const_host = scene_constants_host(img_metas[0]).pin_memory()
        const_dev = const_host.to(dpt_dist.device, non_blocking=True)
        meta = dict(img_metas[0])
        meta["_sgc_scene_const"] = const_dev
        meta["_sgc_static"] = True

        def body():
            volume, valid, occ = self.build_volume_from_features(x, [meta], dpt_dist)
            outs = self._neck_head_eager(volume, valid)
            return dict(volume=volume, valid=valid, occ=occ, centerness=outs[0], bbox_pred=outs[1], cls_score=outs[2])

        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):              # warm-up outside capture (plans, attributes, allocator)
            body()
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            result = body()
        entry = dict(graph=graph, const_host=const_host, const_dev=const_dev, result=result,
                     copied=torch.cuda.Event(), inputs=None)
        entry["copied"].record()
        return entry

    def _forward_scene_graph(self, x, img_metas, dpt_dist):
        """The launch sequence of a scene does not depend on its content once the pair / voxel counts stay on the
        device (``static_counts``): it is captured once and replayed -- one host call per scene instead of ~150
        launches, three read-backs and their Python orchestration (2.2 ms of host time per scene, more than the
        kernels need once two scenes overlap).  The only per-scene host work is the 3x4 projection matrices of
        ``img_meta`` (one pinned 1.9 KB copy).

        Inputs: the graph reads the feature / depth maps IN PLACE, keyed by their addresses -- a producer that
        reuses its output buffers always hits.  Up to ``scene_graph_capacity`` such graphs are kept; a caller that
        keeps arriving with new addresses is served by ONE more graph per (shapes, stream) that owns a private copy
        of the inputs (a device-to-device copy per scene, 0.1 ms on config 2) instead of a capture per scene."""
        from .voxformer import scene_constants_host
        cache = self.__dict__.setdefault("_scene_graph_cache", {})
        key = self._scene_graph_key(x, img_metas, dpt_dist, aliased=True)
        entry = cache.get(key)
        if entry is None:
            n_aliased = sum(1 for e in cache.values() if e["inputs"] is None)
            if n_aliased < self.scene_graph_capacity:
                entry = cache[key] = self._capture_scene_graph(x, img_metas, dpt_dist)
            else:
                key = self._scene_graph_key(x, img_metas, dpt_dist, aliased=False)
                entry = cache.get(key)
                if entry is None:
                    own = [torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device) for t in list(x) + [dpt_dist]]
                    for dst, src in zip(own, list(x) + [dpt_dist]):
                        dst.copy_(src)
                    entry = cache[key] = self._capture_scene_graph(own[:-1], img_metas, own[-1])
                    entry["inputs"] = own
        if entry["inputs"] is not None:
            for dst, src in zip(entry["inputs"], list(x) + [dpt_dist]):
                dst.copy_(src)
        entry["copied"].synchronize()                  # the previous upload has left the pinned staging buffer
        entry["const_host"].copy_(scene_constants_host(img_metas[0]))
        entry["const_dev"].copy_(entry["const_host"], non_blocking=True)
        entry["copied"].record()
        entry["graph"].replay()
        return entry["result"]

    def forward_features(self, x, img_metas, dpt_dist):
        """FPN maps + depth distribution -> head tensors (the timed hot path).  A batch in eval / no-grad is this call scene by scene,
        stacked: bit-identical to B separate calls (graphs, masks and the Winograd form stay as they are)."""
        if x[0].shape[0] > 1 and not self.training and not torch.is_grad_enabled():
            per = []
            for b in range(x[0].shape[0]):
                r = self.forward_features([f[b:b + 1] for f in x], img_metas[b:b + 1], dpt_dist[b:b + 1])
                # graph replays hand out their static buffers: the next scene overwrites them
                per.append({k: ([t.clone() for t in v] if isinstance(v, (list, tuple)) else None if v is None else v.clone()) for k, v in r.items()})
            out = {k: None if per[0][k] is None else torch.cat([p[k] for p in per]) for k in ("volume", "valid", "occ")}
            for k in ("centerness", "bbox_pred", "cls_score"):
                out[k] = [torch.cat([p[k][i] for p in per]) for i in range(len(per[0][k]))]
            return out
        if (self.scene_graph and not self.training and not torch.is_grad_enabled() and dpt_dist.is_cuda
                and self.voxel_head is not None):
            return self._forward_scene_graph(x, img_metas, dpt_dist)
        volume, valid, occ = self.build_volume_from_features(x, img_metas, dpt_dist)
        outs = self._neck_head_eager(volume, valid) if self.masked_tail else self._neck_head(volume)
        return dict(volume=volume, valid=valid, occ=occ, centerness=outs[0], bbox_pred=outs[1], cls_score=outs[2])

    def forward_train_from_features(self, x, img_metas, dpt_dist, gt_bboxes_3d, gt_labels_3d):
        """SGCDet.forward_train (SGCDet.py:98-114) from the FPN maps on: detection losses of the head and, with
        ``occ_loss=True``, the occupancy loss of the voxel head against the head's own ``geo_occ`` targets (the 2D
        head / depth-loss branches belong to the out-of-scope producers)."""
        volume, valid, occ = self.build_volume_from_features(x, img_metas, dpt_dist)
        feats = self.neck_3d(volume)
        losses, sem_occ, geo_occ = self.bbox_head.forward_train(feats, valid.float(), img_metas, gt_bboxes_3d, gt_labels_3d)
        if self.occ_loss:
            losses.update(self.voxel_head.occ_loss(occ, sem_occ, geo_occ))
        return losses

    def forward_train_from_fpn(self, x, img, img_metas, gt_bboxes_3d, gt_labels_3d, depth_maps=None):
        """SGCDet.forward_train (SGCDet.py:98-114) from the FPN maps and the images on, depth head included: the depth
        distribution of ``depth_head`` (SGCDet.py:75-82: ``x[0]`` is detached only with ``depth_loss``; ``use_gt_dpt``
        takes the ground-truth bins instead), ``loss_dpt`` from ``DepthNet_Fusion.loss`` when ``depth_loss=True``
        (:108-109), then exactly ``forward_train_from_features``.  x = FPN maps [B,N,C,H_l,W_l], img [B,N,3,4H,4W],
        depth_maps [B,N,4H,4W] (needed with ``use_gt_dpt`` or ``depth_loss``)."""
        if (self.use_gt_dpt or self.depth_loss) and depth_maps is None:
            raise RuntimeError("SGCDet.forward_train_from_fpn: use_gt_dpt / depth_loss need depth_maps")
        dpt_dist = self.depth_distribution(x, img, img_metas, depth_maps)
        losses = self.forward_train_from_features(x, img_metas, dpt_dist, gt_bboxes_3d, gt_labels_3d)
        if self.depth_loss:
            losses.update(self.depth_head.loss(depth_maps, dpt_dist))
        return losses

    def simple_test_from_features(self, x, img_metas, dpt_dist, as_results=False):
        """SGCDet.simple_test (SGCDet.py:119-129) from the FPN maps on.  ``as_results=True`` returns the reference's
        ``bbox3d2result`` dicts (mmdet3d core/bbox/transforms.py:50-77: ``boxes_3d`` / ``scores_3d`` / ``labels_3d`` on
        the CPU), the format ``dataset.evaluate`` / ``indoor_eval`` consume."""
        r = self.forward_features(x, img_metas, dpt_dist)
        dets = self.bbox_head.get_bboxes(r["centerness"], r["bbox_pred"], r["cls_score"], r["valid"].float(), img_metas)
        if not as_results:
            return dets
        return [dict(boxes_3d=b.to("cpu"), scores_3d=s.cpu(), labels_3d=l.cpu()) for b, s, l in dets]
