"""ctypes binding of libmmnn_sts.so (include/mmnn_sts.h).  The product path has NO fallback: if the library is
missing or a call fails, an exception is raised."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int32, c_int64, c_uint64, c_void_p

import torch  # before the library: it loads libamdhip64 with the SONAME the extension needs

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMNN_LIB_PATH") or os.path.join(_HERE, "libmmnn_sts.so")   # override: developer builds only
_lib = None


class DenseNetConfig(Structure):
    _fields_ = [
        ("in_channels", c_int32), ("init_features", c_int32), ("growth_rate", c_int32), ("bn_size", c_int32),
        ("num_blocks", c_int32), ("block_config", c_int32 * 8), ("eps", c_float), ("momentum", c_float),
        ("dropout_prob", c_float),
    ]


class Conv3dDesc(Structure):
    _fields_ = [("n", c_int32), ("c_in", c_int32), ("d", c_int32), ("h", c_int32), ("w", c_int32), ("c_out", c_int32),
                ("kernel", c_int32 * 3), ("stride", c_int32 * 3), ("padding", c_int32 * 3)]


MLP_MAX_LAYERS = 8
_FP = POINTER(c_float)


class MlpDesc(Structure):
    _fields_ = [
        ("n", c_int32), ("num_layers", c_int32), ("in_dim", c_int32 * MLP_MAX_LAYERS), ("out_dim", c_int32 * MLP_MAX_LAYERS),
        ("relu_first", c_int32 * MLP_MAX_LAYERS), ("dropout_prob", c_float), ("eps", c_float), ("momentum", c_float),
        ("seed", c_uint64), ("training", c_int32), ("first_layer_id", c_int32),
    ]


MULTI_MAX = 64
CE_TARGET_INDEX, CE_TARGET_PROB = 0, 1
CE_REDUCTIONS = {"none": 0, "sum": 1, "mean": 2}
# byte offsets inside the lr range-test state (include/mmnn_sts.h, mmnn_lr_range_*)
LRS_LIVE, LRS_STOP_ITER, LRS_ITERS_DONE, LRS_BEST, LRS_HIST = 4, 8, 12, 24, 40
DT_F64, DT_F32, DT_I64, DT_I32, DT_U8 = 0, 1, 2, 3, 4


class TensorRef(Structure):
    """mmnn_tensor_ref: one small tensor of a multi-tensor launch (mmnn_sgd_step_multi / mmnn_multi_copy)."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("count", c_int64), ("flat_offset", c_int64), ("first_step", c_int32),
                ("reserved", c_int32)]


class GradcamDesc(Structure):
    _fields_ = [("c_total", c_int32), ("growth", c_int32), ("d", c_int32), ("h", c_int32), ("w", c_int32), ("classes", c_int32),
                ("features", c_int32), ("head_ld", c_int32), ("out_d", c_int32), ("out_h", c_int32), ("out_w", c_int32), ("eps", c_float)]


GC_HEAD_DENSENET, GC_HEAD_SIGMOID = 0, 1
GC_LABEL_SUM, GC_LABEL_BEST = -1, -2


class GradcamUnimodalDesc(Structure):
    """mmnn_gradcam_unimodal_desc (include/mmnn_sts.h)."""
    _fields_ = [("n", c_int32), ("channels", c_int32), ("d", c_int32), ("h", c_int32), ("w", c_int32), ("out_d", c_int32),
                ("out_h", c_int32), ("out_w", c_int32), ("classes", c_int32), ("label", c_int32), ("act_ns", c_int64), ("mask_ns", c_int64)]


class GradcamHead(Structure):
    """mmnn_gradcam_head: the layers between the captured Conv3d and the outputs."""
    _fields_ = [("kind", c_int32), ("features", c_int32), ("w_feat_ld", c_int32), ("chan_off", c_int32), ("w_out", c_void_p),
                ("w_feat", c_void_p), ("gamma", c_void_p), ("running_var", c_void_p), ("outputs", c_void_p), ("eps", c_float)]


class MlpParams(Structure):
    _fields_ = [(k, c_void_p * MLP_MAX_LAYERS) for k in (
        "weight", "bias", "gamma", "beta", "running_mean", "running_var", "grad_weight", "grad_bias", "grad_gamma", "grad_beta",
        "num_batches_tracked")]


TF_MAX_TAPS = 13


class TransformDesc(Structure):
    """mmnn_transform_desc (include/mmnn_sts.h)."""
    _fields_ = [("n", c_int32), ("c", c_int32), ("d", c_int32), ("h", c_int32), ("w", c_int32), ("out_d", c_int32), ("out_h", c_int32),
                ("out_w", c_int32), ("stages", c_int32), ("norm_mean", c_float), ("norm_std", c_float)]


class TransformParams(Structure):
    """mmnn_transform_params: one sample's draws, with the Gaussian taps and zoom geometry already derived."""
    _fields_ = [("fire", c_int32), ("flip_axis", c_int32), ("theta", ctypes.c_double), ("noise_seed", c_uint64),
                ("zoom_m", c_int32 * 3), ("zoom_off", c_int32 * 3), ("shift", c_float), ("gamma", c_float), ("alpha", c_float),
                ("noise_std", c_float), ("hist_fl", c_float * 10), ("smooth_r", c_int32 * 3), ("sharp1_r", c_int32 * 3),
                ("sharp2_r", c_int32 * 3), ("smooth_k", (c_float * TF_MAX_TAPS) * 3), ("sharp1_k", (c_float * TF_MAX_TAPS) * 3),
                ("sharp2_k", (c_float * TF_MAX_TAPS) * 3)]


class IngestDesc(Structure):
    """mmnn_ingest_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("scan_type", c_int32), ("mask_type", c_int32), ("scan_slope", c_float),
                ("scan_inter", c_float), ("mask_slope", c_float), ("mask_inter", c_float)]


class ResampleMaskDesc(Structure):
    """mmnn_resample_mask_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("mx", c_int32), ("my", c_int32), ("mz", c_int32), ("mask_type", c_int32),
                ("mask_slope", c_float), ("mask_inter", c_float), ("index_map", ctypes.c_double * 12), ("threshold", ctypes.c_double)]


MAPS_TO_SCAN_MAX_MAPS = 16


class MapsToScanDesc(Structure):
    """mmnn_maps_to_scan_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("n_maps", c_int32)]


class DecodeSlicesDesc(Structure):
    """mmnn_decode_slices_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("bits_allocated", c_int32), ("bits_stored", c_int32), ("high_bit", c_int32),
                ("is_signed", c_int32), ("out_type", c_int32)]


RLE_CHUNK = 4096                             # MMNN_RLE_CHUNK


class RleDesc(Structure):
    """mmnn_rle_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("bits_allocated", c_int32), ("payload_bytes", c_int64)]


JPEGLL_CHUNK = 1024                          # MMNN_JPEGLL_CHUNK
JPEGLL_FRAME_BYTES = 56                      # mmnn_jpegll_frame: int64 offset, length, int32 precision, 16 BITS, 17 HUFFVAL, 3 reserved


class JpegllDesc(Structure):
    """mmnn_jpegll_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("bits_allocated", c_int32), ("payload_bytes", c_int64)]


RASTERIZE_CHUNK_EDGES = 1024                 # MMNN_RASTERIZE_CHUNK_EDGES


class RasterizeDesc(Structure):
    """mmnn_rasterize_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("n_contours", c_int32), ("n_points", c_int64)]


class UnpackFramesDesc(Structure):
    """mmnn_unpack_frames_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("n_frames", c_int32), ("n_refs", c_int32), ("one", c_int32)]


GATHER_MAX_ROWS = 256                        # MMNN_GATHER_MAX_ROWS
OCCLUSION_MAX_OUTPUTS = 16                   # MMNN_OCCLUSION_MAX_OUTPUTS
CHANNEL_MEANS_PARTS = 64                     # MMNN_CHANNEL_MEANS_PARTS


class OcclusionDesc(Structure):
    """mmnn_occlusion_desc (include/mmnn_sts.h)."""
    _fields_ = [("c", c_int32), ("d", c_int32), ("h", c_int32), ("w", c_int32), ("win", c_int32 * 3), ("stride", c_int32 * 3)]


RADIOMICS_DIRECTIONS, RADIOMICS_FIRSTORDER, RADIOMICS_GLCM, RADIOMICS_MAX_BINS = 13, 17, 23, 1024
RADIOMICS_RESULT_INT64, RADIOMICS_RESULT_BYTES = 20, (20 + 10 + 17 + 23) * 8      # mmnn_radiomics_result: 20 int64, then 50 doubles
RADIOMICS_GLRLM, RADIOMICS_GLDM, RADIOMICS_NGTDM, RADIOMICS_NEIGHBOURS = 16, 14, 5, 27
RADIOMICS_TEXTURE_BYTES = (16 + 14 + 5) * 8                                       # mmnn_radiomics_texture_result: 35 doubles
RADIOMICS_GLSZM = 16
RADIOMICS_ZONES_BYTES = (6 + 16) * 8                                              # mmnn_radiomics_zones_result: 6 int64, then 16 doubles
RADIOMICS_MESH_BYTES = (3 + 1 + 4) * 8                                            # mmnn_radiomics_mesh_result: 3 int64, then 5 doubles
RADIOMICS_MESH_CONFIGS, RADIOMICS_MESH_TRI_ROW = 256, 16


class RadiomicsDesc(Structure):
    """mmnn_radiomics_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("scan_type", c_int32), ("mask_type", c_int32),
                ("scan_slope", ctypes.c_double), ("scan_inter", ctypes.c_double), ("mask_slope", ctypes.c_double),
                ("mask_inter", ctypes.c_double), ("bin_width", ctypes.c_double), ("max_bins", c_int32)]


LOG_FILTER_MAX_RADIUS = 88                   # MMNN_LOG_FILTER_MAX_RADIUS


class LogFilterDesc(Structure):
    """mmnn_log_filter_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("scan_type", c_int32), ("scan_slope", ctypes.c_double),
                ("scan_inter", ctypes.c_double), ("radius", c_int32 * 3), ("weight", ctypes.c_double * 3)]


RESAMPLE_HORIZON = 40                        # MMNN_RESAMPLE_HORIZON
NORMALIZE_RESULT_BYTES = 32                  # mmnn_normalize_result: int64 n, double mean, sd, int64 nonfinite


class NormalizeDesc(Structure):
    """mmnn_normalize_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("scan_type", c_int32), ("scan_slope", ctypes.c_double),
                ("scan_inter", ctypes.c_double), ("scale", ctypes.c_double), ("outliers", ctypes.c_double)]


class ResampleEntry(Structure):
    """mmnn_resample_entry (include/mmnn_sts.h): 56 bytes."""
    _fields_ = [("w", ctypes.c_double * 4), ("i", c_int32 * 4), ("nearest", c_int32), ("inside", c_int32)]


class ResampleDesc(Structure):
    """mmnn_resample_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("mx", c_int32), ("my", c_int32), ("mz", c_int32), ("scan_type", c_int32),
                ("mask_type", c_int32), ("scan_slope", ctypes.c_double), ("scan_inter", ctypes.c_double), ("mask_slope", ctypes.c_double),
                ("mask_inter", ctypes.c_double), ("pole", ctypes.c_double), ("pole_gain", ctypes.c_double), ("gain", ctypes.c_double),
                ("pole_power", ctypes.c_double * RESAMPLE_HORIZON)]


MARGIN_MAX_REACH = 128                       # MMNN_MARGIN_MAX_REACH
MARGIN_DILATE, MARGIN_SHELL = 0, 1           # MMNN_MARGIN_DILATE, MMNN_MARGIN_SHELL


class MaskMarginDesc(Structure):
    """mmnn_mask_margin_desc (include/mmnn_sts.h)."""
    _fields_ = [("x", c_int32), ("y", c_int32), ("z", c_int32), ("mask_type", c_int32), ("mask_slope", ctypes.c_double),
                ("mask_inter", ctypes.c_double), ("spacing", ctypes.c_double * 3), ("radius", ctypes.c_double), ("mode", c_int32)]


def _signatures():
    """Every prototype of include/mmnn_sts.h as {symbol: (restype, argtypes)}, from one table per return type (tests/test_host_cpu.py
    holds them against the header)."""
    V, I, U, F, Q, D, S, P = c_void_p, c_int32, c_uint64, c_float, c_int64, ctypes.c_double, c_char_p, POINTER
    status = {                               # int32 status: 0, or 1 (ValueError) / another (RuntimeError) with mmnn_last_error set
        "mmnn_densenet_out_shape": [V] + [P(I)] * 4,
        "mmnn_densenet_forward": [V, V, V, V, V, V, I, U, V],
        "mmnn_densenet_backward": [V, V, V, V, V, V, I, U, V],
        "mmnn_densenet_backward_range": [V, V, V, V, V, V, I, U, I, I, V],
        "mmnn_densenet_block_param_range": [V, I, P(Q), P(Q)],
        "mmnn_densenet_relu_mask": [V, V, V, I, I, I, V, V],
        "mmnn_gap_linear_forward": [I, I, I, I, V, V, V, V, V, F, U, I, V],
        "mmnn_gap_linear_backward": [I, I, I, I, V, V, V, V, V, V, V, F, U, I, I, V],
        "mmnn_mlp_forward": [P(MlpDesc), P(MlpParams), V, V, V, V],
        "mmnn_mlp_backward": [P(MlpDesc), P(MlpParams), V, V, V, V, V, I, V],
        "mmnn_fusion_heads_forward": [I, I, I, I] + [V] * 9 + [V],
        "mmnn_fusion_heads_backward": [I, I, I, I] + [V] * 14 + [I, V],
        "mmnn_linear_forward": [I, I, I, V, V, V, V, V],
        "mmnn_linear_backward": [I, I, I, V, V, V, V, V, V, I, V],
        "mmnn_cox_blend_loss": [I, I, I, V, V, V, V, V, V, V, V, V],
        "mmnn_cox_blend_loss_typed": [I, I, I, V, V, I, V, I, V, V, V, V, V, V],
        "mmnn_cox_blend_backward": [I, I, I, V, V, V, V, V, V],
        "mmnn_sgd_step": [V, V, V, Q, F, F, F, I, I, V],
        "mmnn_sgd_step_multi": [P(TensorRef), I, V, F, F, F, I, V],
        "mmnn_multi_copy": [P(TensorRef), I, V, I, V],
        "mmnn_sgd_step_dev": [V, V, V, Q, V, V, F, F, I, I, V],
        "mmnn_sgd_step_multi_dev": [P(TensorRef), I, V, V, V, F, F, I, V],
        "mmnn_cross_entropy": [I, I, V, V, I, Q, I, V, V, V],
        "mmnn_cross_entropy_backward": [I, I, I, V, V, V, V],
        "mmnn_lr_range_init": [V, I, V],
        "mmnn_lr_range_accumulate": [V, V, F, I, V],
        "mmnn_lr_range_update": [V, I, D, D, D, V],
        "mmnn_gradcam": [P(GradcamDesc), V, V, V, V, V, V, V, V, V, V, V],
        "mmnn_gradcam_unimodal": [P(GradcamUnimodalDesc), P(GradcamHead), V, V, V, V, V, V, Q, V],
        "mmnn_bce_logits": [Q, I, V, V, V, V, V, V],
        "mmnn_conv3d_out_shape": [P(Conv3dDesc), P(I), P(I), P(I)],
        "mmnn_conv3d_forward": [P(Conv3dDesc), V, V, V, V],
        "mmnn_conv3d_backward_data": [P(Conv3dDesc), V, V, V, V],
        "mmnn_conv3d_backward_weight": [P(Conv3dDesc), V, V, V, V, I, V],
        "mmnn_bn3d_forward": [I, I, Q, V, V, V, V, V, F, F, I, I, V, F, U, V, V, V, V],
        "mmnn_bn3d_backward": [I, I, Q, V, V, V, V, V, I, I, F, U, V, V, V, V, V, V],
        "mmnn_gap_fc_sigmoid_forward": [I, I, Q, I, V, V, V, V, V, V],
        "mmnn_gap_fc_sigmoid_backward": [I, I, Q, I, V, V, V, V, V, V, V, V],
        "mmnn_densenet_set_timer": [V, I, I],
        "mmnn_densenet_read_timer": [V, P(D), P(Q)],
        "mmnn_densenet_read_timer_class": [V, I, I, P(D), P(Q)],
        "mmnn_densenet_set_option": [V, S, Q],
        "mmnn_densenet_set_batch_counters": [V, V, I],
        "mmnn_measure_mfma_clock": [P(D), V, V],
        "mmnn_transform_volumes": [P(TransformDesc), P(TransformParams), V, V, V, Q, V],
        "mmnn_ingest_volume": [P(IngestDesc), V, V, V, V, V, V],
        "mmnn_ingest_volume_sized": [P(IngestDesc), I, V, V, V, V, V, V],
        "mmnn_resample_mask": [P(ResampleMaskDesc), V, V, V],
        "mmnn_maps_to_scan": [P(MapsToScanDesc), V, V, V, V, V],
        "mmnn_maps_to_scan_sized": [P(MapsToScanDesc), I, V, V, V, V, V],
        "mmnn_decode_slices": [P(DecodeSlicesDesc), V, V, V, V],
        "mmnn_rle_expand": [P(RleDesc), V, V, V, V, V, V],
        "mmnn_jpegll_decode": [P(JpegllDesc), V, V, V, V, V, V],
        "mmnn_rasterize_contours": [P(RasterizeDesc), V, V, V, V, V],
        "mmnn_unpack_frames": [P(UnpackFramesDesc), V, V, V, V, V],
        "mmnn_gather_rows": [V, Q, Q, P(I), I, V, V],
        "mmnn_occlude_windows": [P(OcclusionDesc), V, V, I, I, V, V],
        "mmnn_occlusion_map": [P(OcclusionDesc), I, V, V, V, V],
        "mmnn_channel_means": [V, I, Q, V, V, V],
        "mmnn_radiomics": [P(RadiomicsDesc)] + [V] * 7,
        "mmnn_radiomics_texture": [P(RadiomicsDesc)] + [V] * 9,
        "mmnn_radiomics_zones": [P(RadiomicsDesc)] + [V] * 8,
        "mmnn_radiomics_mesh": [P(RadiomicsDesc), V, V, P(D)] + [V] * 4,
        "mmnn_radiomics_mesh_table": [V, V, V],
        "mmnn_log_filter": [P(LogFilterDesc), V, V, V, V, V],
        "mmnn_normalize_scan": [P(NormalizeDesc), V, V, V, V, V],
        "mmnn_resample_pair": [P(ResampleDesc)] + [V] * 8,
        "mmnn_mask_margin_reach": [P(D), D, P(I)],
        "mmnn_mask_margin": [P(MaskMarginDesc), V, V, V, V, V],
    }
    counts = {                               # int64 size, count or offset; negative: refused, with mmnn_last_error set
        "mmnn_densenet_param_count": [V],
        "mmnn_densenet_runstat_count": [V],
        "mmnn_densenet_workspace_bytes": [V],
        "mmnn_densenet_ws_offset": [V, S, I, I],
        "mmnn_conv3d_wgrad_workspace_bytes": [P(Conv3dDesc)],
        "mmnn_gradcam_unimodal_workspace_bytes": [P(GradcamUnimodalDesc)],
        "mmnn_transform_workspace_bytes": [P(TransformDesc)],
        "mmnn_ingest_workspace_bytes": [I, I, I],
        "mmnn_maps_to_scan_workspace_bytes": [I, I, I],
        "mmnn_rle_workspace_bytes": [I, I, I, I],
        "mmnn_jpegll_workspace_bytes": [I, I, I, I],
        "mmnn_occlusion_window_count": [P(OcclusionDesc), P(I)],
        "mmnn_radiomics_workspace_bytes": [I, I, I, I],
        "mmnn_radiomics_texture_workspace_bytes": [I, I, I, I],
        "mmnn_radiomics_zones_workspace_bytes": [I, I, I, I],
        "mmnn_radiomics_mesh_workspace_bytes": [I, I, I, I],
        "mmnn_log_filter_workspace_bytes": [I, I, I],
        "mmnn_normalize_scan_workspace_bytes": [I, I, I],
        "mmnn_resample_pair_workspace_bytes": [I] * 6,
        "mmnn_mask_margin_workspace_bytes": [I, I, I],
        "mmnn_lr_range_state_bytes": [I],
        "mmnn_mlp_saved_floats": [P(MlpDesc)],
    }
    sigs = {                                 # neither of the two: (restype, argtypes)
        "mmnn_version": (I, []),
        "mmnn_last_error": (S, []),
        "mmnn_densenet_plan_create": (V, [P(DenseNetConfig), I, I, I, I]),
        "mmnn_densenet_plan_destroy": (None, [V]),
    }
    sigs.update((name, (I, args)) for name, args in status.items())
    sigs.update((name, (Q, args)) for name, args in counts.items())
    return sigs


def lib():
    """Load the shared library once (torch is imported first, above, so that its HIP runtime is the one bound)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -m mmnn_sts_amd.build` (hipcc, gfx950). "
            "mmnn_sts_amd has no CPU / eager fallback.")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, args) in _signatures().items():
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = args
    _lib = L
    return L


def check(status: int, what: str) -> None:
    """C status -> Python exception (1: ValueError, otherwise RuntimeError), SURVEY 8(b) error contract."""
    if status == 0:
        return
    msg = lib().mmnn_last_error().decode("utf-8", "replace")
    if status == 1:
        raise ValueError(f"{what}: {msg}")
    raise RuntimeError(f"{what}: {msg} (status {status})")


def last_error() -> str:
    return lib().mmnn_last_error().decode("utf-8", "replace")


def call(symbol: str, *args) -> None:
    """Call a status-returning function; a nonzero status raises through `check` under the symbol's name."""
    status = getattr(lib(), symbol)(*args)
    if status:
        check(status, symbol)


def enqueue(symbol: str, *args, device=None) -> None:
    """`call` with the current stream appended as the last argument: the current device's, or, under a guard, that of `device`."""
    if device is None:
        return call(symbol, *args, torch.cuda.current_stream().cuda_stream)
    with torch.cuda.device(device):
        call(symbol, *args, torch.cuda.current_stream().cuda_stream)


def count(symbol: str, *args) -> int:
    """Call an int64 size / count / offset function; a negative result raises ValueError with the library's message."""
    n = getattr(lib(), symbol)(*args)
    if n < 0:
        raise ValueError(f"{symbol}: {last_error()}")
    return int(n)


def device_buffer(t, shape_or_count, dtype, device, who: str):
    """`t`, checked to be what `who` can write on `device`: contiguous, of `dtype`, with exactly that shape (a tuple) or that many
    elements (an int); a new tensor when None."""
    if t is None:
        return torch.empty(shape_or_count, dtype=dtype, device=device)
    fits = tuple(t.shape) == shape_or_count if isinstance(shape_or_count, tuple) else t.numel() == shape_or_count
    if not (fits and t.device == device and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"{who}: out must be {shape_or_count} contiguous {dtype} on {device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    return t


def workspace(t, nbytes: int, device, who: str):
    """`t`, checked to hold at least `nbytes` contiguous bytes on `device`; a new uint8 tensor when None."""
    if t is None:
        return torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    have = t.numel() * t.element_size()
    if t.device != device or not t.is_contiguous() or have < nbytes:
        raise ValueError(f"{who}: workspace of {have} bytes on {t.device}{'' if t.is_contiguous() else ' (not contiguous)'}, "
                         f"{nbytes} needed on {device}")
    return t
