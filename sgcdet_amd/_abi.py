"""ctypes description of the C ABI declared in ``include/sgcdet_amd.h``.

One table drives every binding of that header: the product library
(``sgcdet_amd/csrc/libsgcdet_amd.so``, HIP/gfx950) and -- from the test side
only -- the CPU oracle that exports the same symbols.  The training-only entry
points of ``include/sgcdet_amd_train.h`` have a table of their own
(``TRAIN_SIGNATURES`` / ``TRAIN_INTROSPECTION``), bound only when ``Library`` is
asked for it (the product library; the oracle has no twin of them); the image-side
convolutions of ``include/sgcdet_amd_image.h`` likewise (``IMAGE_SIGNATURES`` /
``IMAGE_INTROSPECTION``); ``include/sgcdet_amd_depth_train.h`` (``DEPTH_TRAIN_SIGNATURES`` /
``DEPTH_TRAIN_INTROSPECTION``), ``include/sgcdet_amd_level_train.h`` (``LEVEL_TRAIN_SIGNATURES`` /
``LEVEL_TRAIN_INTROSPECTION``) and ``include/sgcdet_amd_scene_batch.h`` (``SCENE_BATCH_SIGNATURES`` /
``SCENE_BATCH_INTROSPECTION``) and ``include/sgcdet_amd_syncbn.h`` (``SYNCBN_SIGNATURES`` / ``SYNCBN_INTROSPECTION``) are bound
together with the training tables.  Nothing
here touches torch; pointers are plain integers (``tensor.data_ptr()``).
"""
import ctypes as C

_p = C.c_void_p
_i = C.c_int
_f = C.c_float
_d = C.c_double

# name -> argtypes (restype is int for all but the introspection / query calls)
SIGNATURES = {
    "sgc_depth_score_forward": [_p, _p, _p, _p, _p] + [_i] * 7 + [_p],
    "sgc_wms_forward": [_p, _p, _p, _p, _p, _p, _p] + [_i] * 7 + [_p],
    "sgc_wms_backward": [_p] * 11 + [_i] * 7 + [_p],
    "sgc_depth_score_backward": [_p] * 7 + [_i] * 7 + [_p],
    "sgc_dfa3d_forward": [_p] * 8 + [_i] * 9 + [_p],
    "sgc_dfa3d_backward": [_p] * 11 + [_i] * 9 + [_p],
    "sgc_dfa3d_forward_items": [_p] * 9 + [_i] * 9 + [_p],
    "sgc_dfa3d_backward_items": [_p] * 12 + [_i] * 9 + [_p],
    "sgc_dfa3d_backward_binned": [_p] * 11 + [_i] * 13 + [_p],
    "sgc_project_points": [_p] * 6 + [_i, _i, _f, _f, _f, _f, _p],
    "sgc_compact_pairs": [_p, _i, _i] + [_p] * 9 + [_p],
    "sgc_pairs_geometry_sample": [_p] * 7 + [_i] * 9 + [_p],
    "sgc_pairs_geometry_linear_bf16x3": [_p] * 11 + [_i] * 10 + [_p],
    "sgc_pairs_deform_gather": [_p] * 9 + [_i] * 12 + [_p],
    "sgc_depth_pairs": [_p, _p] + [_i] * 5 + [_p],
    "sgc_bin_pairs": [_p] * 9 + [_i] * 7 + [_p],
    "sgc_pairs_deform_gather_tiled": [_p, _i] + [_p] * 6 + [_i] * 15 + [_p],
    "sgc_linear_rows_headmajor_bf16x3": [_p] * 5 + [_i] * 6 + [_p],
    "sgc_tile_window": [_i] * 12 + [C.POINTER(C.c_int)] * 5,
    "sgc_view_mean": [_p] * 4 + [_i] * 3 + [_p, _i] + [_p],
    "sgc_view_attend": [_p] * 5 + [_i] * 4 + [_p, _i] + [_p],
    "sgc_view_attend_backward": [_p] * 8 + [_i] * 5 + [_p],
    "sgc_view_attend_pq": [_p] * 5 + [_i] * 4 + [_p, _i] + [_p],
    "sgc_scatter_rows": [_p] * 4 + [_p, _i, _i, _p],
    "sgc_nchw_to_nhwc_crop": [_p, _p] + [_i] * 7 + [_p],
    "sgc_nhwc_to_nchw_pad": [_p, _p] + [_i] * 6 + [_p],
    "sgc_conv3d_cl_f32": [_p] * 6 + [_i] * 9 + [_p, C.c_int64] + [_p],
    "sgc_conv3d_cl_bf16x3": [_p] * 7 + [_i] * 9 + [_p, C.c_int64] + [_p],
    "sgc_conv3d_cl_bf16x3_masked": [_p] * 8 + [_i] * 6 + [_p, C.c_int64] + [_p],
    "sgc_conv3d_cl_bf16x3_act": [_p] * 8 + [_i] * 8 + [_p, _p, C.c_int64] + [_p],
    "sgc_conv3d_winograd_z_bf16x3": [_p] * 7 + [_i] * 6 + [_p, C.c_int64] + [_p],
    "sgc_conv2d_nhwc_bf16x3": [_p] * 7 + [_i] * 7 + [_p],
    "sgc_conv3d_wgrad_bf16x3": [_p] * 3 + [_i] * 7 + [_p, C.c_int64] + [_p],
    "sgc_mask_dilate3": [_p, _p, _i, _i, _i, _p],
    "sgc_valid_pyramid": [_p, _p, _i, _i, _i, _i, _p],
    "sgc_linear_rows_bf16x3": [_p] * 6 + [_i] * 3 + [_p],
    "sgc_linear_rows_zrow_bf16x3": [_p] * 6 + [_i] * 3 + [_p],
    "sgc_linear_rows_blockdiag_bf16x3": [_p] * 6 + [_i] * 4 + [_p],
    "sgc_level_tail": [_p] * 7 + [_f] + [_p] * 8 + [_f] + [_p] + [_i] * 3 + [_p],
    "sgc_topk_select": [_p, _i, _i, _p, _p, _p, _p],
    "sgc_topk_select_ws": [_p, _i, _i, _p, _p, _p, _p, C.c_int64, _p],
    "sgc_layer_norm_rows": [_p, _p, _p, _f, _p, _p, _i, _i, _p],
    "sgc_bn_rows_forward": [_p] * 5 + [_f, _f] + [_p] * 4 + [C.c_int64, _i, _i, _p],
    "sgc_bn_rows_backward": [_p] * 9 + [C.c_int64, _i, _i, _p],
    "sgc_bn_rows_act_forward": [_p] * 5 + [_f, _f] + [_p, _i] + [_p] * 4 + [C.c_int64, _i, _i, _p],
    "sgc_bn_rows_act_backward": [_p] * 11 + [C.c_int64, _i, _i, _p],
    "sgc_aligned_nms3d": [_p] * 3 + [_f] + [_p] * 3 + [_i] + [_p],
    "sgc_nms_rotated_bev": [_p] * 3 + [_f] + [_p] * 3 + [_i, _i] + [_p],
    "sgc_box_iou_rotated": [_p] * 3 + [_i, _i] + [_p],
    "sgc_assign_targets": [_p] * 4 + [_i] * 4 + [_p] * 5 + [_i, _i] + [_p],
    "sgc_plane_sweep_corr": [_p] * 5 + [_i] * 6 + [_p],
    "sgc_upsample2x_occ": [_p] * 5 + [_i] * 4 + [_p],
    "sgc_upsample2x_backward": [_p, _p] + [_i] * 4 + [_p],
    "sgc_scatter_add_rows": [_p] * 3 + [_i, _i, _p],
    "sgc_set_tuning": [C.c_char_p, _i],
    "sgc_set_conv_products": [_i],
    "sgc_pack_conv_weight": [_p] * 3 + [_i] * 7 + [_p],
    "sgc_unpack_conv_wgrad": [_p] * 2 + [_i] * 7 + [_p],
    "sgc_pack_conv_weight_batch": [_p] + [_i] * 3 + [_p],
}

INTROSPECTION = {
    "sgc_abi_version": (C.c_int, []),
    "sgc_last_error": (C.c_char_p, []),
    "sgc_backend": (C.c_char_p, []),
    "sgc_conv3d_workspace_floats": (C.c_int64, [_i] * 9),
    "sgc_conv3d_wgrad_workspace_floats": (C.c_int64, [_i] * 7),
    "sgc_bn_rows_workspace_floats": (C.c_int64, [_i] * 2),
    "sgc_topk_select_workspace_bytes": (C.c_int64, [_i]),
    "sgc_level_tail_supported": (C.c_int, [_i] * 2),
    "sgc_view_attend_pq_supported": (C.c_int, [_i] * 3),
    "sgc_conv3d_winograd_z_supported": (C.c_int, [_i] * 5),
    "sgc_pack_conv_weight_blocks": (C.c_int, [_i] * 4),
    "sgc_conv3d_winograd_z_workspace_floats": (C.c_int64, [_i] * 5),
    "sgc_get_conv_products": (C.c_int, []),
    "sgc_bin_pairs_workspace_bytes": (C.c_int64, [_i] * 7),
    "sgc_dfa3d_backward_binned_lds_bytes": (C.c_int64, [_i] * 8),
    "sgc_pairs_geometry_linear_supported": (C.c_int, [_i] * 4),
    "sgc_linear_rows_blockdiag_supported": (C.c_int, [_i] * 3),
    "sgc_pairs_geometry_linear_workspace_bytes": (C.c_int64, [_i]),
}

# include/sgcdet_amd_train.h: training-only entry points (no CPU-oracle twin)
TRAIN_SIGNATURES = {
    "sgc_plane_sweep_corr_backward": [_p] * 7 + [C.c_int64] + [_i] * 6 + [_p],
    "sgc_grad_sqnorm_batch": [_p, _i, _i, _p, _p, _p],
    "sgc_adamw_step_batch": [_p, _i, _i, _p, _i, _p, _f, _p],        # groups: HOST array of sgc_optim_group
    "sgc_head_loss_forward": [_p, _i] + [_p] * 4 + [_i] * 4 + [_d] * 5 + [_p] * 5 + [C.c_int64, _p],      # levels: HOST array of sgc_head_loss_level
    "sgc_head_loss_finalize": [_p, C.c_int64, _p, _i, _p] + [_d] * 3 + [_p] * 3,                         # level_points: HOST int64 array
    "sgc_head_loss_scale_grads": [_p, _p, _p] + [_i] * 3 + [_p] * 5,
    "sgc_conv2d_wgrad_bf16x3": [_p] * 3 + [_i] * 7 + [_p, C.c_int64] + [_p],
    "sgc_frozen_norm_act_backward": [_p] * 5 + [C.c_int64, _i, _i] + [_p],
    "sgc_upsample_nearest_add_nhwc": [_p] * 3 + [_i] * 6 + [_p],
    "sgc_upsample_nearest_add_backward_nhwc": [_p] * 2 + [_i] * 6 + [_p],
    "sgc_rows_colsum": [_p, _p, C.c_int64, _i, _p, C.c_int64] + [_p],
    "sgc_conv2d_stem7_wgrad_bf16x3": [_p] * 3 + [_i] * 3 + [_p, C.c_int64] + [_p],
}

TRAIN_INTROSPECTION = {
    "sgc_plane_sweep_corr_backward_workspace_bytes": (C.c_int64, [_i] * 5),
    "sgc_grad_sqnorm_batch_workspace_bytes": (C.c_int64, [_i]),
    "sgc_head_loss_workspace_bytes": (C.c_int64, [_i] * 2),
    "sgc_conv2d_wgrad_workspace_floats": (C.c_int64, [_i] * 7),
    "sgc_rows_colsum_workspace_floats": (C.c_int64, [C.c_int64, _i]),
    "sgc_conv2d_stem7_wgrad_workspace_floats": (C.c_int64, [_i] * 3),
}

# include/sgcdet_amd_depth_train.h: the padded live BatchNorm and the softmax backward of the depth net's U-Nets and depth_reg in
# training (no CPU-oracle twin; bound with the training tables)
DEPTH_TRAIN_SIGNATURES = {
    "sgc_bn_rows_padded_forward": [_p] * 5 + [_f, _f] + [_p, _i] + [_p] * 4 + [C.c_int64, _i, _i, _i, _p],
    "sgc_bn_rows_padded_backward": [_p] * 11 + [_i, _p, C.c_int64, _i, _i, _i, _p],
    "sgc_softmax_rows_backward": [_p] * 3 + [C.c_int64] + [_i] * 4 + [_p],
}

DEPTH_TRAIN_INTROSPECTION = {}      # the padded norm sizes its workspace with sgc_bn_rows_workspace_floats (INTROSPECTION)

# include/sgcdet_amd_level_train.h: the backward halves of a view-transform level in training -- LayerNorm, sampling locations /
# attention weights, mean over views (no CPU-oracle twin; bound with the training tables)
LEVEL_TRAIN_SIGNATURES = {
    "sgc_layer_norm_rows_backward": [_p, _p, _f] + [_p] * 5 + [C.c_int64, _i, _i, _p],
    "sgc_sampling_locations_forward": [_p] * 5 + [_i] * 5 + [_p],
    "sgc_sampling_locations_backward": [_p] * 5 + [_i] * 5 + [_p],
    "sgc_view_mean_backward": [_p] * 4 + [_i] * 5 + [_p],
}

LEVEL_TRAIN_INTROSPECTION = {
    "sgc_layer_norm_rows_backward_workspace_floats": (C.c_int64, [_i] * 2),
}

# include/sgcdet_amd_scene_batch.h: the 3-D convolution passes on a batch of scenes in one launch (training on scene batches; bound
# with the training tables).  With scenes = 1 they ARE sgc_conv3d_cl_bf16x3 / sgc_conv3d_wgrad_bf16x3, which call them.
SCENE_BATCH_SIGNATURES = {
    "sgc_conv3d_cl_bf16x3_batched": [_p] * 7 + [_i] * 10 + [_p, C.c_int64] + [_p],
    "sgc_conv3d_wgrad_bf16x3_batched": [_p] * 3 + [_i] * 8 + [_p, C.c_int64] + [_p],
}

SCENE_BATCH_INTROSPECTION = {
    "sgc_conv3d_batched_workspace_floats": (C.c_int64, [_i] * 10),
    "sgc_conv3d_wgrad_batched_workspace_floats": (C.c_int64, [_i] * 8),
}

# include/sgcdet_amd_syncbn.h: the BatchNorm passes over rows cut at the collective of SyncBatchNorm -- local statistics / global
# apply, local sums / global apply (no CPU-oracle twin; bound with the training tables)
SYNCBN_SIGNATURES = {
    "sgc_bn_rows_sync_stats": [_p] * 3 + [C.c_int64, _i, _i, _p],
    "sgc_bn_rows_sync_apply": [_p, _p, _i] + [_p] * 4 + [_f, _f] + [_p, _i] + [_p] * 4 + [_i, _i, _p],
    "sgc_bn_rows_sync_backward_sums": [_p] * 7 + [C.c_int64, _i, _i, _p],
    "sgc_bn_rows_sync_backward_apply": [_p] * 10 + [_i, _i, _p],
}

SYNCBN_INTROSPECTION = {}      # the workspace is sized with sgc_bn_rows_workspace_floats (INTROSPECTION)
SYNCBN_MAX_WORLD = 1024        # == SGC_SYNCBN_MAX_WORLD
SYNCBN_MAX_COUNT = 1 << 24     # counts travel as fp32: rows per rank and world * rows stay below it

# include/sgcdet_amd_image.h: the 2-D convolutions of the image-side CNNs (no CPU-oracle twin)
IMAGE_SIGNATURES = {
    "sgc_conv2d_nhwc_ex_bf16x3": [_p] * 7 + [_i] * 13 + [_p],
    "sgc_conv2d_nhwc_strided_bf16x3": [_p] * 7 + [_i] * 13 + [_p],
    "sgc_maxpool2d_nhwc": [_p, _p] + [_i] * 4 + [_p],
    "sgc_conv2d_stem7_bf16x3": [_p] * 6 + [_i] * 4 + [_p],
    "sgc_nchw_to_nhwc_padc": [_p, _p] + [_i] * 5 + [_p],
}

IMAGE_INTROSPECTION = {
    "sgc_conv2d_nhwc_ex_supported": (C.c_int, [_i] * 12),
    "sgc_conv2d_nhwc_strided_supported": (C.c_int, [_i] * 12),
}

CONV2D_RELU, CONV2D_RELU_AFTER_ADD = 1, 2      # SGC_CONV2D_* flags of include/sgcdet_amd_image.h


class OptimGroup(C.Structure):
    """``sgc_optim_group`` of include/sgcdet_amd_train.h: the hyper-parameters of one parameter group, as Python floats."""
    _fields_ = [("lr", C.c_double), ("weight_decay", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


OPTIM_ITEM_BYTES = 64     # sizeof(sgc_optim_item); TensorOps.optim_item_list packs it as "<4Qq4i2f"
HEAD_LOSS_LEVEL_BYTES = 64     # sizeof(sgc_head_loss_level); TensorOps.head_loss packs it as "<4Qq6i"
HEAD_LOSS_MAX_SCALES = 4       # SGC_HEAD_LOSS_MAX_SCALES

ABI_VERSION = 4      # == SGC_ABI_VERSION of include/sgcdet_amd.h (tests/test_abi_cpu.py compares the two)


class SgcError(RuntimeError):
    """Raised when an entry point returns a negative status."""


class Library:
    """A loaded shared object exporting the sgcdet_amd C ABI."""

    def __init__(self, path, train=False, image=False):
        """``train`` / ``image``: also bind (and require) the entry points of include/sgcdet_amd_train.h and
        include/sgcdet_amd_depth_train.h, include/sgcdet_amd_level_train.h, include/sgcdet_amd_scene_batch.h,
        include/sgcdet_amd_syncbn.h / of
        include/sgcdet_amd_image.h."""
        self.path = str(path)
        self._dll = C.CDLL(self.path)
        missing = []
        signatures = {**SIGNATURES, **(TRAIN_SIGNATURES if train else {}), **(DEPTH_TRAIN_SIGNATURES if train else {}),
                      **(LEVEL_TRAIN_SIGNATURES if train else {}), **(SCENE_BATCH_SIGNATURES if train else {}),
                      **(SYNCBN_SIGNATURES if train else {}),
                      **(IMAGE_SIGNATURES if image else {})}
        introspection = {**INTROSPECTION, **(TRAIN_INTROSPECTION if train else {}), **(DEPTH_TRAIN_INTROSPECTION if train else {}),
                         **(LEVEL_TRAIN_INTROSPECTION if train else {}), **(SCENE_BATCH_INTROSPECTION if train else {}),
                         **(SYNCBN_INTROSPECTION if train else {}),
                         **(IMAGE_INTROSPECTION if image else {})}
        for name, argtypes in signatures.items():
            try:
                fn = getattr(self._dll, name)
            except AttributeError:
                missing.append(name)
                continue
            fn.argtypes = argtypes
            fn.restype = C.c_int
        for name, (res, argtypes) in introspection.items():
            try:
                fn = getattr(self._dll, name)
            except AttributeError:
                missing.append(name)
                continue
            fn.argtypes = argtypes
            fn.restype = res
        if missing:
            raise ImportError(f"{self.path} does not export: {', '.join(missing)}")
        if self._dll.sgc_abi_version() != ABI_VERSION:
            raise ImportError(
                f"{self.path}: ABI version {self._dll.sgc_abi_version()} != {ABI_VERSION}")

    @property
    def backend(self):
        return self._dll.sgc_backend().decode()

    def last_error(self):
        return self._dll.sgc_last_error().decode()

    def call(self, name, *args):
        rc = getattr(self._dll, name)(*args)
        if rc != 0:
            raise SgcError(f"{name} failed with status {rc}: {self.last_error()}")
        return rc
