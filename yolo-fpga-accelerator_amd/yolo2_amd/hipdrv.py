"""ctypes binding of libyolo2_hip.so (include/yolo2_hip.h).

This is host plumbing only: every compute call goes through the C ABI into the hand-written
HIP kernels.  There is no CPU fallback: if the library is missing or no GPU is present the
calls raise.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import net

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# YOLO2_HIP_LIB: another build of the same library (A/B runs of compile-time kernel variants, tools/ab.sh)
LIB_PATH = os.environ.get("YOLO2_HIP_LIB") or os.path.join(PKG_DIR, "libyolo2_hip.so")
HOST_LIB_PATH = os.path.join(PKG_DIR, "libyolo2_host.so")   # the host restatements (no GPU code)

YOLO2_SUCCESS, YOLO2_ERROR, YOLO2_TIMEOUT, YOLO2_INIT_ERROR, YOLO2_MMAP_ERROR, YOLO2_DMA_ERROR = 0, -1, -2, -3, -4, -5

EXPORTS = [
    "yolo2_accel_init", "yolo2_accel_cleanup", "yolo2_hip_select_device", "yolo2_hip_device_count",
    "yolo2_hip_last_error", "yolo2_set_q_values", "yolo2_is_busy", "yolo2_is_done", "yolo2_wait_for_completion",
    "yolo2_execute_conv_layer", "yolo2_execute_maxpool_layer", "yolo2_execute_conv_layer_f32",
    "memory_allocate_ddr", "memory_free_ddr", "memory_allocate_weights", "memory_allocate_bias",
    "memory_allocate_inference_buffer", "memory_get_phys_addr", "memory_flush_cache", "memory_invalidate_cache",
    "yolo2_hip_alloc", "yolo2_hip_free", "yolo2_hip_memcpy_h2d", "yolo2_hip_memcpy_d2h", "yolo2_hip_memset",
    "yolo2_hip_create", "yolo2_hip_destroy", "yolo2_hip_load_weights_int16", "yolo2_hip_load_weights_int16_dev",
    "yolo2_hip_layer_path", "yolo2_hip_set_batch", "yolo2_hip_run_batch_int16", "yolo2_hip_run_batch_int16_host",
    "yolo2_hip_debug_layer_output", "yolo2_hip_set_profiling", "yolo2_hip_layer_times_ms",
    "yolo2_hip_conv_launch_info", "yolo2_strip_int16_layer_pad", "yolo2_weight_len", "yolo2_bias_len",
    "yolo2_hip_num_layers", "yolo2_hip_layer_desc", "yolo2_hip_layer_routes", "yolo2_hip_debug_layer_wiring",
    "yolo2_hip_layer_path_counts", "yolo2_hip_run_frames_int16", "yolo2_hip_num_lanes", "yolo2_hip_load_weights_fp32", "yolo2_hip_run_batch_fp16", "yolo2_hip_run_batch_fp16_host",
    "yolo2_hip_letterbox_u8", "yolo2_hip_run_images_u8_host", "yolo2_hip_last_layer_path", "yolo2_hip_run_frame_fp32_host", "yolo2_hip_num_lanes_fp16",
    "yolo2_hip_layer_pool_fused", "yolo2_get_status", "yolo2_read_reg", "yolo2_write_reg", "yolo2_hip_driver_calls",
    "dma_buffer_init", "dma_buffer_cleanup", "dma_buffer_alloc", "dma_buffer_free", "dma_buffer_sync_for_device",
    "dma_buffer_sync_for_cpu", "dma_buffer_get_phys",
    "yolo2_hip_run_batch_fp32", "yolo2_hip_run_batch_fp32_host", "yolo2_hip_load_weights_fp32_dev", "yolo2_hip_postprocess_int16", "yolo2_hip_postprocess_f32",
    "yolo2_hip_postprocess_int16_app", "yolo2_hip_postprocess_f32_app",
    "yolo2_hip_shard_range", "yolo2_hip_multi_create", "yolo2_hip_multi_destroy", "yolo2_hip_multi_num_devices",
    "yolo2_hip_multi_uses_rccl", "yolo2_hip_multi_ctx", "yolo2_hip_multi_load_weights_int16", "yolo2_hip_multi_load_weights_fp32",
    "yolo2_hip_multi_run_frames_int16", "yolo2_hip_multi_run_images_u8_host", "yolo2_hip_rccl_unique_id",
    "yolo2_hip_rccl_init_rank", "yolo2_hip_rccl_finalize", "yolo2_hip_load_weights_int16_bcast", "yolo2_hip_load_weights_fp32_bcast",
    "yolo2_hip_rccl_info", "yolo2_hip_multi_rccl_info", "yolo2_hip_ctx_device", "yolo2_hip_alloc_on",
    "yolo2_hip_fp16_layer_kernel", "yolo2_hip_f16_store_check", "yolo2_hip_f16_plan_describe",
    "yolo2_hip_run_images_u8_dets", "yolo2_hip_multi_run_images_u8_dets", "yolo2_hip_set_fp16_lanes", "yolo2_hip_conv_plan_string", "yolo2_hip_plan_source",
    "yolo2_hip_set_option", "yolo2_hip_options_string", "yolo2_hip_set_plan_cache", "yolo2_hip_plan_cache_info", "yolo2_hip_plan_cache_check",
    "yolo2_hip_i16_plan_check", "yolo2_hip_ks_scratch_bytes", "yolo2_hip_i16_edge_map", "yolo2_hip_last_layer_edge",
    "yolo2_hip_run_batch_f32tol", "yolo2_hip_run_batch_f32tol_host", "yolo2_hip_f32tol_layer_kernel", "yolo2_hip_num_lanes_f32tol",
    "yolo2_hip_debug_f16_tensor", "yolo2_hip_debug_live_bytes",
    "yolo2_hip_run_images_u8_f16_host", "yolo2_hip_run_images_u8_dets_f16", "yolo2_hip_multi_run_images_u8_dets_f16",
    "yolo2_hip_images_layer0_kernel",
    "yolo2_hip_letterbox_pix", "yolo2_hip_run_images_pix_host", "yolo2_hip_run_images_pix_dets", "yolo2_hip_run_images_pix_f16_host",
    "yolo2_hip_run_images_pix_dets_f16", "yolo2_hip_multi_run_images_pix_host", "yolo2_hip_multi_run_images_pix_dets",
    "yolo2_hip_multi_run_images_pix_dets_f16",
    "yolo2_hip_absmax_f32", "yolo2_hip_calib_reset", "yolo2_hip_calib_frames", "yolo2_hip_calib_images_pix_host", "yolo2_hip_calib_stats",
    "yolo2_hip_calib_q_tables", "yolo2_hip_calib_q_from_stats", "yolo2_hip_quantize_weights_int16",
    "yolo2_hip_annotate_pix", "yolo2_hip_annotate_images_pix_host", "yolo2_hip_multi_annotate_images_pix_host",
    "yolo2_hip_jpeg_bound", "yolo2_hip_jpeg_encode_rgb24", "yolo2_hip_annotate_images_pix_jpeg_host",
    "yolo2_hip_multi_annotate_images_pix_jpeg_host",
    "yolo2_hip_loop_images_pix", "yolo2_hip_multi_loop_images_pix", "yolo2_hip_loop_last_info", "yolo2_hip_draw_items_dev",
    "yolo2_hip_draw_item_size",
    "yolo2_hip_calib_q8_from_stats", "yolo2_hip_calib_q8_tables", "yolo2_hip_quantize_weights_int8", "yolo2_hip_load_weights_int8",
    "yolo2_hip_run_batch_int8", "yolo2_hip_run_batch_int8_host", "yolo2_hip_debug_i8_tensor", "yolo2_execute_conv_layer_int8",
    "yolo2_hip_run_images_pix_int8_host", "yolo2_hip_run_images_pix_dets_int8", "yolo2_hip_images_front_kernel_int8",
    "yolo2_hip_jpeg_probe", "yolo2_hip_jpeg_reason_name", "yolo2_hip_decode_jpeg_host", "yolo2_hip_decode_jpeg_ref",
    "yolo2_hip_run_images_jpeg_dets", "yolo2_hip_jpeg_last_info", "yolo2_hip_decode_jpeg_split_ref", "yolo2_hip_jpeg_split_info",
    "yolo2_hip_loop_images_jpeg", "yolo2_hip_multi_loop_images_jpeg", "yolo2_hip_multi_run_images_jpeg_dets",
]

# include/yolo2_hip.h YOLO2_PIX_*: the pixfmt argument of the _pix entries ("yuyv": packed YUYV 4:2:2, arrays uint8 [h][w][2])
PIXFMTS = {"grey8": 1, "rgb24": 3, "yuyv": 0x56595559}
# ... and the video formats, planar YUV 4:2:0: arrays uint8 [h * 3 / 2][w] - the Y plane's h rows, then h / 2 rows of chroma bytes.
# A table of their own: PIXFMTS stays the camera formats' (tests pin it); every pixfmt= parameter takes a name of either.
PIXFMTS_420 = {"nv12": 0x3231564E, "i420": 0x32315559}
PLANAR_420 = tuple(PIXFMTS_420)
# ... and packed RGB as most callers hold it: "bgr24" (OpenCV) arrays uint8 [h][w][3] of B G R; "rgba32" / "bgra32" (GUI toolkits, screen
# capture) arrays uint8 [h][w][4] of R G B X / B G R X, the fourth byte never used.  A third table, for the same reason.
PIXFMTS_PACKED = {"bgr24": 0x33524742, "rgba32": 0x34324241, "bgra32": 0x34325241}
PACKED_RGB = tuple(PIXFMTS_PACKED)
LOOP_OUT_RGB24, LOOP_OUT_JPEG, LOOP_OUT_BGR24 = 0, 1, 0x33524742   # include/yolo2_hip.h YOLO2_LOOP_OUT_*
LOOP_OUT_NV12, LOOP_OUT_I420 = 0x3231564E, 0x32315559                # ... the annotated frame as planar YUV 4:2:0


def pix_code(pixfmt: str) -> int:
    """the YOLO2_PIX_* value of a pixfmt name"""
    if pixfmt in PIXFMTS:
        return PIXFMTS[pixfmt]
    if pixfmt in PIXFMTS_420:
        return PIXFMTS_420[pixfmt]
    if pixfmt in PIXFMTS_PACKED:
        return PIXFMTS_PACKED[pixfmt]
    raise ValueError(f"pixfmt must be None or one of {tuple(PIXFMTS) + PLANAR_420 + PACKED_RGB}, not {pixfmt!r}")


def _pix_code(pixfmt, imgs) -> int:
    """the entries' pixfmt argument for a list of contiguous uint8 arrays, whose shapes must be that format's"""
    code = pix_code(pixfmt)
    last = {"grey8": None, "rgb24": 3, "yuyv": 2, "nv12": None, "i420": None, "bgr24": 3, "rgba32": 4, "bgra32": 4}[pixfmt]
    for im in imgs:
        if pixfmt in PLANAR_420 and (im.ndim != 2 or im.shape[0] % 3):
            raise ValueError(f"a {pixfmt} image is uint8 [h * 3 / 2][w] with h even (rows a multiple of 3), not {im.shape}")
        if (im.ndim != 2 if last is None else im.ndim != 3 or im.shape[2] != last):
            raise ValueError(f"a {pixfmt} image is uint8 [h][w]{'' if last is None else f'[{last}]'}, not {im.shape}")
    return code


def _pix_hw(pixfmt, shape):
    """(h, w) of the picture an array of that shape holds: a planar 4:2:0 array has h * 3 / 2 rows"""
    return (shape[0] * 2 // 3 if pixfmt in PLANAR_420 else shape[0]), shape[1]


_hip = None      # the HIP runtime itself, for _stream_sync only


def _stream_sync(stream: int):
    """hipStreamSynchronize on a caller's stream (the wrappers below copy results back with blocking copies on the null stream, which
    do not order behind a non-blocking stream)"""
    global _hip
    if _hip is None:
        for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
            try:
                _hip = C.CDLL(name)
                break
            except OSError:
                continue
        else:
            raise Yolo2HipError("libamdhip64.so not found: cannot synchronise a caller's stream")
        _hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    rc = _hip.hipStreamSynchronize(C.c_void_p(stream))
    if rc:
        raise Yolo2HipError(f"hipStreamSynchronize failed with HIP error {rc}")


def letterbox_pix(image: np.ndarray, pixfmt: str, net_w: int = 416, net_h: int = 416, stream: int = 0) -> np.ndarray:
    """letterbox_u8 with a pixel format (yolo2_hip_letterbox_pix): "grey8" [h][w], "rgb24" [h][w][3], "yuyv" [h][w][2] (packed
    YUYV 4:2:2) "nv12" / "i420" [h * 3 / 2][w] (planar YUV 4:2:0) or "bgr24" [h][w][3] / "rgba32" / "bgra32" [h][w][4] (packed RGB), converted per fetched pixel on the GPU -> float [3][net_h][net_w] frame."""
    return letterbox_u8(image, net_w, net_h, pixfmt=pixfmt, stream=stream)


def letterbox_u8(image_hwc: np.ndarray, net_w: int = 416, net_h: int = 416, pixfmt=None, stream: int = 0) -> np.ndarray:
    """uint8 [h][w][3] (or [h][w]) host image -> float [3][net_h][net_w] frame, letterboxed on the GPU; the kernel is enqueued on
    `stream` (a hipStream_t as an integer, 0 = the null stream)."""
    im = np.ascontiguousarray(image_hwc, dtype=np.uint8)
    ch = 1 if im.ndim == 2 else im.shape[2]
    code = None if pixfmt is None else _pix_code(pixfmt, [im])
    L = lib()
    src, dst = C.c_uint64(0), C.c_uint64(0)
    out = np.empty((3, net_h, net_w), dtype=np.float32)
    check(L.yolo2_hip_alloc(im.nbytes, C.byref(src)), "alloc")
    check(L.yolo2_hip_alloc(out.nbytes, C.byref(dst)), "alloc")
    try:
        check(L.yolo2_hip_memcpy_h2d(src, im.ctypes.data_as(C.c_void_p), im.nbytes), "h2d")
        if code is None:
            check(L.yolo2_hip_letterbox_u8(src, im.shape[1], im.shape[0], ch, dst, net_w, net_h, C.c_void_p(stream)), "yolo2_hip_letterbox_u8")
        else:
            check(L.yolo2_hip_letterbox_pix(src, im.shape[1], _pix_hw(pixfmt, im.shape)[0], code, dst, net_w, net_h, C.c_void_p(stream)), "yolo2_hip_letterbox_pix")
        if stream:
            _stream_sync(stream)
        check(L.yolo2_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), dst, out.nbytes), "d2h")
    finally:
        L.yolo2_hip_free(src)
        L.yolo2_hip_free(dst)
    return out


class Yolo2HipError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(PKG_DIR, "csrc", f) for f in os.listdir(os.path.join(PKG_DIR, "csrc"))]
    srcs.append(os.path.join(os.path.dirname(PKG_DIR), "include", "yolo2_hip.h"))
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        subprocess.run(["make", "-s", "-C", PKG_DIR], check=True)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Yolo2HipError(f"{LIB_PATH} is missing: build it with `make -C {PKG_DIR}` "
                            "(the GPU path has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    u64, i32, u32, vp = C.c_uint64, C.c_int, C.c_uint32, C.c_void_p
    L.yolo2_hip_last_error.restype = C.c_char_p
    L.yolo2_execute_conv_layer.argtypes = [u64] * 4 + [i32] * 23 + [u32]
    L.yolo2_execute_maxpool_layer.argtypes = [u64] * 2 + [i32] * 14 + [u32]
    L.yolo2_execute_conv_layer_f32.argtypes = [u64] * 4 + [i32] * 10 + [u32]
    L.yolo2_hip_alloc.argtypes = [C.c_size_t, C.POINTER(u64)]
    L.yolo2_hip_free.argtypes = [u64]
    L.yolo2_hip_memcpy_h2d.argtypes = [u64, vp, C.c_size_t]
    L.yolo2_hip_memcpy_d2h.argtypes = [vp, u64, C.c_size_t]
    L.yolo2_hip_memset.argtypes = [u64, i32, C.c_size_t]
    L.yolo2_hip_create.argtypes = [i32, C.POINTER(vp)]
    L.yolo2_hip_destroy.argtypes = [vp]
    L.yolo2_hip_load_weights_int16.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, i32, vp, i32, vp, i32]
    L.yolo2_hip_load_weights_int16_dev.argtypes = [vp, u64, C.c_size_t, u64, C.c_size_t, vp, i32, vp, i32, vp, i32]
    L.yolo2_hip_layer_path.argtypes = [vp, i32]
    L.yolo2_hip_num_lanes.argtypes = [vp]
    L.yolo2_hip_layer_pool_fused.argtypes = [vp, i32]
    L.yolo2_hip_run_frames_int16.argtypes = [vp, vp, i32, i32, vp, C.POINTER(i32)]
    L.yolo2_hip_layer_path_counts.argtypes = [vp, i32, C.POINTER(i32)]
    L.yolo2_hip_set_batch.argtypes = [vp, i32]
    L.yolo2_hip_run_batch_int16.argtypes = [vp, u64, i32, u64, C.POINTER(i32), vp]
    L.yolo2_hip_run_batch_int16_host.argtypes = [vp, vp, i32, vp, C.POINTER(i32)]
    L.yolo2_hip_debug_layer_output.argtypes = [vp, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.yolo2_hip_set_profiling.argtypes = [vp, i32]
    L.yolo2_hip_layer_times_ms.argtypes = [vp, vp]
    L.yolo2_hip_conv_launch_info.argtypes = [vp, i32] + [C.POINTER(i32)] * 5
    L.yolo2_strip_int16_layer_pad.argtypes = [vp, C.c_size_t, vp, i32, vp]
    L.yolo2_strip_int16_layer_pad.restype = C.c_long
    L.yolo2_hip_load_weights_fp32.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
    L.yolo2_hip_run_batch_fp16.argtypes = [vp, u64, i32, u64, vp]
    L.yolo2_hip_run_batch_fp16_host.argtypes = [vp, vp, i32, vp]
    L.yolo2_hip_run_frame_fp32_host.argtypes = [vp, vp, vp]
    L.yolo2_hip_run_batch_fp32.argtypes = [vp, u64, i32, u64, vp]
    L.yolo2_hip_run_batch_fp32_host.argtypes = [vp, vp, i32, vp]
    L.yolo2_hip_letterbox_u8.argtypes = [u64, i32, i32, i32, u64, i32, i32, vp]
    L.yolo2_hip_run_images_u8_host.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, C.POINTER(i32)]
    L.memory_get_phys_addr.restype = u64
    pi32 = C.POINTER(i32)
    L.yolo2_hip_load_weights_fp32_dev.argtypes = [vp, u64, C.c_size_t, u64, C.c_size_t]
    L.yolo2_hip_postprocess_int16.argtypes = [vp, u64, i32, i32, vp, vp, C.c_float, C.c_float, vp, i32, vp, vp, vp, vp, vp]
    L.yolo2_hip_postprocess_f32.argtypes = [vp, u64, i32, vp, vp, C.c_float, C.c_float, vp, i32, vp, vp, vp, vp, vp]
    L.yolo2_hip_postprocess_int16_app.argtypes = L.yolo2_hip_postprocess_int16.argtypes
    L.yolo2_hip_postprocess_f32_app.argtypes = L.yolo2_hip_postprocess_f32.argtypes
    L.yolo2_hip_shard_range.argtypes = [i32, i32, i32, pi32, pi32]
    # (an older build loaded through YOLO2_HIP_LIB for an A/B run may lack the newer entries: their signatures are set when present)
    def sig(name, argtypes, restype=None):
        f = getattr(L, name, None)
        if f is not None:
            f.argtypes = argtypes
            if restype is not None:
                f.restype = restype
    sig("yolo2_hip_set_option", [vp, C.c_char_p, C.c_char_p])
    sig("yolo2_hip_options_string", [vp, C.c_char_p, i32])
    sig("yolo2_hip_set_plan_cache", [vp, C.c_char_p])
    sig("yolo2_hip_plan_cache_info", [vp, C.POINTER(u64), pi32, pi32, pi32])
    sig("yolo2_hip_plan_cache_check", [C.c_char_p, u64, pi32])
    sig("yolo2_hip_i16_plan_check", [i32, i32, i32, C.c_size_t])
    sig("yolo2_hip_f16_plan_describe", [C.c_char_p, i32, i32, C.c_char_p, i32], i32)
    sig("yolo2_hip_i16_edge_map", [i32, i32, i32, i32, vp, vp, vp, vp])
    sig("yolo2_hip_last_layer_edge", [], i32)
    sig("yolo2_hip_run_batch_f32tol", [vp, u64, i32, u64, vp])
    sig("yolo2_hip_run_batch_f32tol_host", [vp, vp, i32, vp])
    sig("yolo2_hip_f32tol_layer_kernel", [vp, i32], C.c_char_p)
    sig("yolo2_hip_num_lanes_f32tol", [vp])
    sig("yolo2_hip_ks_scratch_bytes", [vp], C.c_size_t)
    sig("yolo2_hip_debug_f16_tensor", [vp, i32, i32, i32, i32, vp, C.c_size_t, pi32])
    sig("yolo2_hip_debug_live_bytes", [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)])
    sig("yolo2_hip_run_images_u8_f16_host", [vp, i32, vp, vp, vp, i32, i32, i32, vp])
    sig("yolo2_hip_run_images_u8_dets_f16", [vp, i32, vp, vp, vp, i32, i32, i32, C.c_float, C.c_float, i32, vp, i32, vp])
    sig("yolo2_hip_multi_run_images_u8_dets_f16", [vp, i32, vp, vp, vp, i32, i32, i32, C.c_float, C.c_float, i32, vp, i32, vp])
    sig("yolo2_hip_images_layer0_kernel", [vp, i32], C.c_char_p)
    L.yolo2_hip_multi_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.yolo2_hip_multi_destroy.argtypes = [vp]
    L.yolo2_hip_multi_num_devices.argtypes = [vp]
    L.yolo2_hip_multi_uses_rccl.argtypes = [vp]
    L.yolo2_hip_multi_ctx.argtypes = [vp, i32]
    L.yolo2_hip_multi_ctx.restype = vp
    L.yolo2_hip_multi_load_weights_int16.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, i32, vp, i32, vp, i32]
    L.yolo2_hip_multi_load_weights_fp32.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
    L.yolo2_hip_multi_run_frames_int16.argtypes = [vp, vp, i32, i32, vp, pi32]
    L.yolo2_hip_multi_run_images_u8_host.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, pi32]
    L.yolo2_hip_rccl_unique_id.argtypes = [vp]
    L.yolo2_hip_rccl_init_rank.argtypes = [vp, i32, vp, i32, i32]
    L.yolo2_hip_rccl_finalize.argtypes = [vp]
    L.yolo2_hip_load_weights_int16_bcast.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, i32, vp, i32, vp, i32, i32]
    L.yolo2_hip_load_weights_fp32_bcast.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32]
    L.yolo2_hip_run_images_u8_dets.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_float, C.c_float, i32, vp, i32, vp, C.POINTER(i32)]
    L.yolo2_hip_multi_run_images_u8_dets.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_float, C.c_float, i32, vp, i32, vp, C.POINTER(i32)]
    L.yolo2_hip_set_fp16_lanes.argtypes = [vp, i32]
    L.yolo2_hip_conv_plan_string.argtypes = [vp, i32, C.c_char_p, i32]
    L.yolo2_hip_plan_source.argtypes = [vp]
    L.yolo2_hip_rccl_info.argtypes = [vp, vp]
    L.yolo2_hip_multi_rccl_info.argtypes = [vp, vp]
    L.yolo2_hip_ctx_device.argtypes = [vp]
    L.yolo2_hip_alloc_on.argtypes = [vp, C.c_size_t, C.POINTER(u64)]
    L.yolo2_hip_fp16_layer_kernel.argtypes = [vp, i32]
    L.yolo2_hip_fp16_layer_kernel.restype = C.c_char_p
    L.yolo2_hip_f16_store_check.argtypes = [i32] * 12
    L.yolo2_get_status.restype = u32
    L.yolo2_read_reg.restype = u32
    L.yolo2_read_reg.argtypes = [u32]
    L.yolo2_write_reg.argtypes = [u32, u32]
    L.yolo2_hip_driver_calls.restype = C.c_long
    L.yolo2_set_q_values.argtypes = [i32] * 4
    L.dma_buffer_alloc.argtypes = [C.c_size_t, vp]
    L.dma_buffer_free.argtypes = [vp]
    L.dma_buffer_get_phys.restype = u64
    L.dma_buffer_get_phys.argtypes = [vp, C.c_size_t]
    L.dma_buffer_sync_for_device.argtypes = [vp, C.c_size_t, C.c_size_t]
    L.dma_buffer_sync_for_cpu.argtypes = [vp, C.c_size_t, C.c_size_t]
    L.memory_get_phys_addr.argtypes = [vp]
    # the images entries with a pixel format: the u8 entries' argument lists, pixfmt in place of channels
    sig("yolo2_hip_letterbox_pix", L.yolo2_hip_letterbox_u8.argtypes)
    for name in ("run_images_pix_host", "multi_run_images_pix_host"):
        sig("yolo2_hip_" + name, L.yolo2_hip_run_images_u8_host.argtypes)
    for name in ("run_images_pix_dets", "multi_run_images_pix_dets"):
        sig("yolo2_hip_" + name, L.yolo2_hip_run_images_u8_dets.argtypes)
    sig("yolo2_hip_run_images_pix_f16_host", L.yolo2_hip_run_images_u8_f16_host.argtypes)
    for name in ("run_images_pix_dets_f16", "multi_run_images_pix_dets_f16"):
        sig("yolo2_hip_" + name, L.yolo2_hip_run_images_u8_dets_f16.argtypes)
    # calibration (include/yolo2_hip.h "calibration")
    sig("yolo2_hip_absmax_f32", [u64, C.c_size_t, C.POINTER(C.c_float), C.POINTER(u32), vp])
    sig("yolo2_hip_calib_reset", [vp])
    sig("yolo2_hip_calib_frames", [vp, u64, i32, vp])
    sig("yolo2_hip_calib_images_pix_host", [vp, vp, vp, vp, i32, i32, i32])
    sig("yolo2_hip_calib_stats", [vp, vp, vp, vp, C.POINTER(C.c_long)])
    sig("yolo2_hip_calib_q_tables", [vp, C.c_float, vp, vp, vp])
    sig("yolo2_hip_calib_q_from_stats", [vp, vp, vp, C.c_float, vp, vp, vp])
    sig("yolo2_hip_quantize_weights_int16", [vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_long)])
    # annotated frames (include/yolo2_hip.h "annotated frames")
    sig("yolo2_hip_annotate_pix", [u64, i32, i32, i32, vp, i32, C.c_float, vp, i32, u64, C.POINTER(i32), vp])
    for name in ("annotate_images_pix_host", "multi_annotate_images_pix_host"):
        sig("yolo2_hip_" + name, [vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, C.c_float, vp, i32, vp, vp])
    # annotated frames as JPEG (include/yolo2_hip.h "annotated frames as JPEG")
    sig("yolo2_hip_jpeg_bound", [i32, i32], C.c_size_t)
    sig("yolo2_hip_jpeg_encode_rgb24", [u64, i32, i32, i32, u64, C.c_size_t, C.POINTER(C.c_size_t), vp])
    for name in ("annotate_images_pix_jpeg_host", "multi_annotate_images_pix_jpeg_host"):
        sig("yolo2_hip_" + name, [vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, C.c_float, vp, i32, i32, vp, vp, vp, vp])
    # the camera loop as one call (include/yolo2_hip.h "the camera loop as one call")
    for name in ("loop_images_pix", "multi_loop_images_pix"):
        sig("yolo2_hip_" + name, [vp, i32, vp, vp, vp, i32, i32, i32, C.c_float, C.c_float, i32, vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp])
    sig("yolo2_hip_loop_last_info", [vp, vp])
    sig("yolo2_hip_draw_item_size", [], C.c_size_t)
    sig("yolo2_hip_draw_items_dev", [vp, u64, u64, i32, i32, vp, vp, C.c_float, vp, i32, vp, vp, vp])
    # the int8 pass (include/yolo2_hip.h "int8 pass")
    sig("yolo2_hip_calib_q8_from_stats", [vp, C.c_float, vp])
    sig("yolo2_hip_calib_q8_tables", [vp, C.c_float, vp])
    sig("yolo2_hip_quantize_weights_int8", [vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp])
    sig("yolo2_hip_load_weights_int8", [vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp])
    sig("yolo2_hip_run_batch_int8", [vp, u64, i32, u64, vp])
    sig("yolo2_hip_run_batch_int8_host", [vp, vp, i32, vp])
    sig("yolo2_hip_debug_i8_tensor", [vp, i32, i32, vp, C.c_size_t, pi32])
    sig("yolo2_execute_conv_layer_int8", [u64] * 4 + [vp] + [i32] * 10 + [u32])
    sig("yolo2_hip_run_images_pix_int8_host", L.yolo2_hip_run_images_pix_host.argtypes[:-1])       # (no final_q)
    sig("yolo2_hip_run_images_pix_dets_int8", L.yolo2_hip_run_images_pix_dets.argtypes[:-1])
    sig("yolo2_hip_images_front_kernel_int8", [vp], C.c_char_p)
    # JPEG streams decoded on the GPU (include/yolo2_hip.h)
    sig("yolo2_hip_jpeg_probe", [vp, C.c_size_t, vp])
    sig("yolo2_hip_jpeg_reason_name", [i32], C.c_char_p)
    sig("yolo2_hip_decode_jpeg_host", [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp])
    sig("yolo2_hip_decode_jpeg_ref", [vp, C.c_size_t, vp, C.c_size_t, pi32, pi32, pi32])
    sig("yolo2_hip_jpeg_last_info", [vp, vp])
    sig("yolo2_hip_decode_jpeg_split_ref", [vp, C.c_size_t, C.c_int, vp, C.c_size_t, pi32, pi32, pi32, vp])
    sig("yolo2_hip_jpeg_split_info", [vp, vp])
    for name in ("run_images_jpeg_dets", "multi_run_images_jpeg_dets"):
        sig("yolo2_hip_" + name, [vp, i32, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, i32, vp, i32, vp, pi32, vp])
    # the camera loop from JPEG streams: the records entry's list up to final_q, then the loop's from labels on, then status
    for name in ("loop_images_jpeg", "multi_loop_images_jpeg"):
        sig("yolo2_hip_" + name, [vp, i32, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, i32, vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp])
    _lib = L
    return L


def check(rc: int, what: str = ""):
    if rc != YOLO2_SUCCESS:
        raise Yolo2HipError(f"{what} failed with status {rc}: {lib().yolo2_hip_last_error().decode()}")


def f16_plan_describe(options: str, split: int, batch: int) -> str:
    """The fp16 (split=0) / fp32-tolerance (split=1) launch table for a plan batch as text, one line per step; no GPU needed."""
    n = lib().yolo2_hip_f16_plan_describe(options.encode(), split, batch, None, 0)
    if n < 0:
        check(n, "yolo2_hip_f16_plan_describe")
    buf = C.create_string_buffer(n + 1)
    assert lib().yolo2_hip_f16_plan_describe(options.encode(), split, batch, buf, n + 1) == n
    return buf.value.decode()


# ------------------------------------------------------------------ tier 1 helpers (tests)

class DevBuf:
    """HBM buffer holding a numpy array (the analogue of a udmabuf + its physical address)."""

    def __init__(self, arr: np.ndarray = None, nbytes: int = None, fill: int = 0):
        self.nbytes = arr.nbytes if arr is not None else nbytes
        a = C.c_uint64(0)
        check(lib().yolo2_hip_alloc(max(self.nbytes, 16), C.byref(a)), "yolo2_hip_alloc")
        self.addr = a.value
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            check(lib().yolo2_hip_memcpy_h2d(self.addr, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "h2d")
        else:
            check(lib().yolo2_hip_memset(self.addr, fill, self.nbytes), "memset")

    def get(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        check(lib().yolo2_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.addr, out.nbytes), "d2h")
        return out

    def free(self):
        if self.addr:
            lib().yolo2_hip_free(self.addr)
            self.addr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def w8(w):
    return (w + 7) // 8 * 8


def conv_layer_i16(x, w_reorg, bias, C_, N, K, stride, W, H, pad, leaky, Qw, Qa_in, Qa_out, Qb, fill=0):
    """Calls yolo2_execute_conv_layer the way linux_app/src/yolo2_inference.c:371-381 does."""
    OW = (W - K + 2 * pad) // stride + 1
    OH = (H - K + 2 * pad) // stride + 1
    TR = min(min((27 - K) // stride + 1, 13), OH)
    TC = min(min((27 - K) // stride + 1, 13), OW)
    TM, TN = min(N, 32), min(C_, 4)
    mLoops = -(-N // TM)
    bx, bw, bb = DevBuf(x), DevBuf(w_reorg), DevBuf(bias)
    out0 = np.full((N, OH, w8(OW)), fill, dtype=np.int16)
    by = DevBuf(out0)
    rc = lib().yolo2_execute_conv_layer(bx.addr, by.addr, bw.addr, bb.addr, C_, N, K, stride, W, H, OW, OH, pad,
                                        int(leaky), 0, TM, TN, TR, TC, (mLoops + 1) * TM, mLoops * TM,
                                        (mLoops + 1) * TM, 0, Qw, Qa_in, Qa_out, Qb, 60000)
    check(rc, "yolo2_execute_conv_layer")
    y = by.get(np.int16, (N, OH, w8(OW)))
    for b in (bx, bw, bb, by):
        b.free()
    return y


def conv_layer_f32(x, w_reorg, bias, C_, N, K, stride, W, H, pad, leaky):
    OW = (W - K + 2 * pad) // stride + 1
    OH = (H - K + 2 * pad) // stride + 1
    bx, bw, bb = DevBuf(x), DevBuf(w_reorg), DevBuf(bias)
    by = DevBuf(np.zeros((N, OH, w8(OW)), dtype=np.float32))
    check(lib().yolo2_execute_conv_layer_f32(bx.addr, by.addr, bw.addr, bb.addr, C_, N, K, stride, W, H, OW, OH,
                                             pad, int(leaky), 60000), "yolo2_execute_conv_layer_f32")
    y = by.get(np.float32, (N, OH, w8(OW)))
    for b in (bx, bw, bb, by):
        b.free()
    return y


def conv_layer_i8(x, w8, bias32, weight_q, q_in, q_out, leaky, out_float=False, guard=128):
    """yolo2_execute_conv_layer_int8: one stride-1 "same" conv through the int8 MFMA kernel.  x int8 [B][C][H][W], w8 int8
    [N][C][K][K] (K 1 or 3), bias32 int32 [N], weight_q int32 [N] -> int8 [B][N][H][W], or float32 by layer 30's rule (out_float).
    The output buffer sits between two `guard`-byte regions of 0xA5; they are returned for the caller to look at:
    (y, guard_before, guard_after)."""
    x = np.ascontiguousarray(x, dtype=np.int8)
    w = np.ascontiguousarray(w8, dtype=np.int8)
    b = np.ascontiguousarray(bias32, dtype=np.int32)
    qw = np.ascontiguousarray(weight_q, dtype=np.int32)
    B, C_, H, W = x.shape
    N, K = w.shape[0], w.shape[2]
    if w.shape != (N, C_, K, K) or b.shape != (N,) or qw.shape != (N,) or guard % 4:
        raise ValueError("conv_layer_i8: x [B][C][H][W], w8 [N][C][K][K], bias32 [N], weight_q [N]")
    dt = np.float32 if out_float else np.int8
    nbytes = B * N * H * W * np.dtype(dt).itemsize
    pad = -nbytes % 4
    bx, bw, bb = DevBuf(x), DevBuf(w), DevBuf(b)
    by = DevBuf(nbytes=guard + nbytes + pad + guard, fill=0xA5)
    try:
        check(lib().yolo2_execute_conv_layer_int8(bx.addr, by.addr + guard, bw.addr, bb.addr, qw.ctypes.data_as(C.c_void_p), C_, N, K, W, H, B,
                                                  int(q_in), int(q_out), int(bool(leaky)), int(bool(out_float)), 60000),
              "yolo2_execute_conv_layer_int8")
        raw = by.get(np.uint8, (guard + nbytes + pad + guard,))
    finally:
        for d in (bx, bw, bb, by):
            d.free()
    y = raw[guard:guard + nbytes].view(dt).reshape(B, N, H, W).copy()
    return y, raw[:guard].copy(), raw[guard + nbytes:].copy()


def maxpool_layer_i16(x, C_, W, H, K=2, stride=2):
    OW, OH = W // stride, H // stride
    TR = min((27 - K) // stride + 1, 13, OH)
    TC = min((27 - K) // stride + 1, 13, OW)
    TM = min(4, C_)
    mLoops = -(-C_ // TM)
    bx = DevBuf(x)
    by = DevBuf(np.zeros((C_, OH, w8(OW)), dtype=np.int16))
    check(lib().yolo2_execute_maxpool_layer(bx.addr, by.addr, C_, K, stride, W, H, OW, OH, 1, TM, TR, TC,
                                            (mLoops + 2) * TM, mLoops * TM, (mLoops + 1) * TM, 60000),
          "yolo2_execute_maxpool_layer")
    y = by.get(np.int16, (C_, OH, w8(OW)))
    bx.free(); by.free()
    return y


# ------------------------------------------------------------------ tier 2: whole network

class Yolo2Hip:
    """One accelerator context on one GPU (yolo2_hip_ctx)."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p(0)
        check(lib().yolo2_hip_create(device, C.byref(self._h)), "yolo2_hip_create")
        self.device = device
        self.final_q = None

    def close(self):
        if self._h:
            lib().yolo2_hip_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weights(self, weights_i16, bias_i16, weight_q, bias_q, act_q):
        w = np.ascontiguousarray(weights_i16, dtype=np.int16)
        b = np.ascontiguousarray(bias_i16, dtype=np.int16)
        wq, bq, aq = (np.ascontiguousarray(a, dtype=np.int32) for a in (weight_q, bias_q, act_q))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().yolo2_hip_load_weights_int16(self._h, vp(w), w.size, vp(b), b.size, vp(wq), wq.size,
                                                 vp(bq), bq.size, vp(aq), aq.size), "yolo2_hip_load_weights_int16")

    def load_weights_dev(self, w_ptr, n_w, b_ptr, n_b, weight_q, bias_q, act_q):
        wq, bq, aq = (np.ascontiguousarray(a, dtype=np.int32) for a in (weight_q, bias_q, act_q))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().yolo2_hip_load_weights_int16_dev(self._h, w_ptr, n_w, b_ptr, n_b, vp(wq), wq.size, vp(bq),
                                                     bq.size, vp(aq), aq.size), "yolo2_hip_load_weights_int16_dev")

    def load_model(self, model):
        if isinstance(model, CalibratedModelI8):
            return self.load_weights_int8(model.w8, model.bias32, model.weight_q, model.act_q)
        self.load_weights(model.weights_i16(), model.bias_i16(), model.weight_q, model.bias_q, model.act_q)

    def layer_paths(self):
        return [lib().yolo2_hip_layer_path(self._h, o) for o in range(len(net.CONVS))]

    def layer_path_counts(self):
        out = []
        for o in range(len(net.CONVS)):
            v = (C.c_int * 5)()
            check(lib().yolo2_hip_layer_path_counts(self._h, o, v), "yolo2_hip_layer_path_counts")
            out.append(list(v))
        return out

    def set_batch(self, batch: int):
        check(lib().yolo2_hip_set_batch(self._h, batch), "yolo2_hip_set_batch")

    def run_batch_ptr(self, frames_ptr: int, batch: int, region_ptr: int, stream: int = 0) -> int:
        """Device pointers in/out; enqueues on `stream` and returns without synchronising."""
        q = C.c_int(0)
        check(lib().yolo2_hip_run_batch_int16(self._h, frames_ptr, batch, region_ptr, C.byref(q),
                                              C.c_void_p(stream)), "yolo2_hip_run_batch_int16")
        self.final_q = q.value
        return q.value

    def run_batch_host(self, frames: np.ndarray):
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        B = frames.shape[0]
        region = np.empty((B, 425, 13, 13), dtype=np.int16)
        q = C.c_int(0)
        check(lib().yolo2_hip_run_batch_int16_host(self._h, frames.ctypes.data_as(C.c_void_p), B,
                                                   region.ctypes.data_as(C.c_void_p), C.byref(q)),
              "yolo2_hip_run_batch_int16_host")
        self.final_q = q.value
        return region, q.value

    def run_images_host(self, images, batch: int = 64, pixfmt=None):
        """images: list of uint8 arrays [h][w][3] (or [h][w] grey) of arbitrary sizes -> region tensors.
        Bytes cross PCIe, letterboxing runs on the GPU (yolo2_hip_run_images_u8_host).  pixfmt "grey8" / "rgb24" / "yuyv" (arrays
        [h][w][2]) / "nv12" / "i420" (arrays [h * 3 / 2][w]) / "bgr24" ([h][w][3]) / "rgba32" / "bgra32" ([h][w][4]) names the format instead (yolo2_hip_run_images_pix_host); None infers grey / RGB from the shape."""
        n, ptrs, ws, hs, fmt, _keep = _image_args(images, pixfmt)
        region = np.empty((n, 425, 13, 13), dtype=np.int16)
        q = C.c_int(0)
        fn = lib().yolo2_hip_run_images_u8_host if pixfmt is None else lib().yolo2_hip_run_images_pix_host
        check(fn(self._h, ptrs, ws, hs, fmt, n, batch, region.ctypes.data_as(C.c_void_p), C.byref(q)),
              "yolo2_hip_run_images_u8_host" if pixfmt is None else "yolo2_hip_run_images_pix_host")
        self.final_q = q.value
        return region, q.value

    def loop_images(self, images, pixfmt=None, precision: str = "int16", tail: str = "core", thresh: float = 0.24, nms: float = 0.45,
                    labels=None, jpeg_quality=None, batch: int = 64, cap: int = 845, out_order: str = "rgb"):
        """the camera loop as one call: records and annotated frames from one upload (module-level loop_images)"""
        return loop_images(self._h, images, pixfmt=pixfmt, precision=precision, tail=tail, thresh=thresh, nms=nms, labels=labels,
                           jpeg_quality=jpeg_quality, batch=batch, cap=cap, out_order=out_order)

    def jpeg_decode(self, streams, batch: int = 64, strict: bool = True):
        """see jpeg_decode"""
        return jpeg_decode(self._h, streams, batch=batch, strict=strict)

    def run_jpegs_dets(self, streams, precision: str = "int16", tail: str = "core", batch: int = 64, thresh: float = 0.24, nms: float = 0.45,
                       cap: int = 845, best_class: bool = True, strict: bool = True):
        """see run_jpegs_dets"""
        return run_jpegs_dets(self._h, streams, batch, thresh, nms, cap=cap, best_class=best_class, precision=precision, tail=tail, strict=strict)

    def loop_jpegs(self, streams, precision: str = "int16", tail: str = "core", thresh: float = 0.24, nms: float = 0.45, labels=None,
                   jpeg_quality=None, batch: int = 64, cap: int = 845, strict: bool = True, out_order: str = "rgb"):
        """the camera loop as one call from JPEG streams (module-level loop_jpegs)"""
        return loop_jpegs(self._h, streams, precision=precision, tail=tail, thresh=thresh, nms=nms, labels=labels, jpeg_quality=jpeg_quality,
                          batch=batch, cap=cap, strict=strict, out_order=out_order)

    def loop_last_info(self) -> dict:
        return loop_last_info(self._h)

    def annotate_images(self, images, dets, counts, batch: int, thresh: float, labels=None, pixfmt=None, jpeg_quality=None):
        """the images with their detection records painted in, as the reference's camera loop does (module-level annotate_images);
        with jpeg_quality, as the JPEG streams its MJPEG streamer sends (a list of bytes)"""
        return annotate_images(self._h, images, dets, counts, batch, thresh, labels=labels, pixfmt=pixfmt, jpeg_quality=jpeg_quality)

    # ---- fp16 MFMA path
    def load_weights_fp32(self, weights_f32, bias_f32):
        w = np.ascontiguousarray(weights_f32, dtype=np.float32)
        b = np.ascontiguousarray(bias_f32, dtype=np.float32)
        check(lib().yolo2_hip_load_weights_fp32(self._h, w.ctypes.data_as(C.c_void_p), w.size,
                                                b.ctypes.data_as(C.c_void_p), b.size), "yolo2_hip_load_weights_fp32")

    def run_frame_fp32_host(self, frame: np.ndarray) -> np.ndarray:
        """One frame through the exact fp32 network (reference arithmetic); needs load_weights_fp32."""
        f = np.ascontiguousarray(frame, dtype=np.float32).reshape(3, 416, 416)
        region = np.empty((425, 13, 13), dtype=np.float32)
        check(lib().yolo2_hip_run_frame_fp32_host(self._h, f.ctypes.data_as(C.c_void_p), region.ctypes.data_as(C.c_void_p)),
              "yolo2_hip_run_frame_fp32_host")
        return region

    def run_batch_fp32_ptr(self, frames_ptr: int, batch: int, region_ptr: int, stream: int = 0):
        check(lib().yolo2_hip_run_batch_fp32(self._h, frames_ptr, batch, region_ptr, C.c_void_p(stream)), "yolo2_hip_run_batch_fp32")

    def run_batch_fp32_host(self, frames: np.ndarray) -> np.ndarray:
        """The tiled exact fp32 pass (bit-identical to the reference's fp32 path) on a batch of host frames."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        B = frames.shape[0]
        region = np.empty((B, 425, 13, 13), dtype=np.float32)
        check(lib().yolo2_hip_run_batch_fp32_host(self._h, frames.ctypes.data_as(C.c_void_p), B, region.ctypes.data_as(C.c_void_p)),
              "yolo2_hip_run_batch_fp32_host")
        return region

    def run_batch_fp16_ptr(self, frames_ptr: int, batch: int, region_ptr: int, stream: int = 0):
        check(lib().yolo2_hip_run_batch_fp16(self._h, frames_ptr, batch, region_ptr, C.c_void_p(stream)),
              "yolo2_hip_run_batch_fp16")

    def run_batch_fp16_host(self, frames: np.ndarray) -> np.ndarray:
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        B = frames.shape[0]
        region = np.empty((B, 425, 13, 13), dtype=np.float32)
        check(lib().yolo2_hip_run_batch_fp16_host(self._h, frames.ctypes.data_as(C.c_void_p), B,
                                                  region.ctypes.data_as(C.c_void_p)), "yolo2_hip_run_batch_fp16_host")
        return region

    def run_frames(self, frames: np.ndarray, batch: int):
        """Streaming entry: any number of host frames, chunks of `batch`, copies overlapped with compute."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n = frames.shape[0]
        region = np.empty((n, 425, 13, 13), dtype=np.int16)
        q = C.c_int(0)
        check(lib().yolo2_hip_run_frames_int16(self._h, frames.ctypes.data_as(C.c_void_p), n, batch,
                                               region.ctypes.data_as(C.c_void_p), C.byref(q)), "yolo2_hip_run_frames_int16")
        return region, q.value

    def debug_layer_output(self, layer_idx: int, frame: int = 0) -> np.ndarray:
        if layer_idx < 0:      # the quantised network input
            shape = (3, 416, 416)
        else:
            l = net.LAYERS[layer_idx]
            shape = (l.out_c, l.out_h, w8(l.out_w))
        out = np.empty(shape, dtype=np.int16)
        n = C.c_size_t(0)
        check(lib().yolo2_hip_debug_layer_output(self._h, layer_idx, frame, out.ctypes.data_as(C.c_void_p),
                                                 out.size, C.byref(n)), "yolo2_hip_debug_layer_output")
        assert n.value == out.size
        return out

    def num_lanes(self) -> int:
        return lib().yolo2_hip_num_lanes(self._h)

    def pool_fused_layers(self):
        """Conv layers that run fused with the max pool after them (their full-resolution tensor is not written)."""
        return [i for i in range(32) if lib().yolo2_hip_layer_pool_fused(self._h, i)]

    def set_profiling(self, on: bool):
        check(lib().yolo2_hip_set_profiling(self._h, int(on)), "yolo2_hip_set_profiling")

    def layer_times_ms(self) -> np.ndarray:
        ms = np.zeros(32, dtype=np.float32)
        check(lib().yolo2_hip_layer_times_ms(self._h, ms.ctypes.data_as(C.c_void_p)), "yolo2_hip_layer_times_ms")
        return ms

    # ---- split-fp16 ("fp32 fast"): fp32 accuracy on the matrix cores
    def run_batch_f32tol_host(self, frames: np.ndarray) -> np.ndarray:
        f = np.ascontiguousarray(frames, dtype=np.float32)
        batch = f.shape[0]
        region = np.empty((batch, 425, 13, 13), dtype=np.float32)
        check(lib().yolo2_hip_run_batch_f32tol_host(self._h, f.ctypes.data_as(C.c_void_p), batch, region.ctypes.data_as(C.c_void_p)),
              "yolo2_hip_run_batch_f32tol_host")
        return region

    def run_images_f16_host(self, images, batch: int, split: bool = False, pixfmt=None) -> np.ndarray:
        """images (uint8 [h][w][3] or [h][w] grey, any sizes) -> float32 region tensors [n][425][13][13] through the fp16 pass
        (split=True: the fp32-tolerance pass); layers 0+1 read the image bytes on the GPU (yolo2_hip_run_images_u8_f16_host).
        pixfmt as in run_images_host (yolo2_hip_run_images_pix_f16_host)."""
        n, ptrs, ws, hs, fmt, _keep = _image_args(images, pixfmt)
        region = np.empty((n, 425, 13, 13), dtype=np.float32)
        fn = lib().yolo2_hip_run_images_u8_f16_host if pixfmt is None else lib().yolo2_hip_run_images_pix_f16_host
        check(fn(self._h, int(bool(split)), ptrs, ws, hs, fmt, n, batch, region.ctypes.data_as(C.c_void_p)),
              "yolo2_hip_run_images_u8_f16_host" if pixfmt is None else "yolo2_hip_run_images_pix_f16_host")
        return region

    def images_layer0_kernel(self, split: bool = False) -> str:
        """What the last images call of the fp16 (split=False) / fp32-tolerance pass ran for layers 0+1 ("" before the first)."""
        return lib().yolo2_hip_images_layer0_kernel(self._h, int(bool(split))).decode()

    def run_batch_f32tol_ptr(self, frames_ptr: int, batch: int, region_ptr: int, stream: int = 0):
        check(lib().yolo2_hip_run_batch_f32tol(self._h, frames_ptr, batch, region_ptr, C.c_void_p(stream)), "yolo2_hip_run_batch_f32tol")

    def f32tol_layer_kernel(self, layer_idx: int) -> str:
        return lib().yolo2_hip_f32tol_layer_kernel(self._h, layer_idx).decode()

    def num_lanes_f32tol(self) -> int:
        return int(lib().yolo2_hip_num_lanes_f32tol(self._h))

    F16_GEOM = ("C", "Cp", "H", "W", "Wp", "items", "part_stride", "ch_off")

    def debug_f16_tensor(self, layer_idx: int, frame: int = 0, split: bool = False, which: int = 0):
        """Raw items of layer `layer_idx`'s fp16 (split=False) or split-fp16 tensor from the last run: (uint16 [items][Cp], geometry
        dict).  which: 0 the frame's (H+1)(W+1) items, 1 the lead items, 2 the tail items of the lane holding the frame."""
        g = (C.c_int * 8)()
        check(lib().yolo2_hip_debug_f16_tensor(self._h, int(split), layer_idx, frame, which, None, 0, g), "yolo2_hip_debug_f16_tensor")
        geom = dict(zip(self.F16_GEOM, list(g)))
        out = np.empty((geom["items"], geom["Cp"]), dtype=np.uint16)
        check(lib().yolo2_hip_debug_f16_tensor(self._h, int(split), layer_idx, frame, which, out.ctypes.data_as(C.c_void_p), out.size, g),
              "yolo2_hip_debug_f16_tensor")
        return out, geom

    def set_fp16_lanes(self, lanes: int):
        check(lib().yolo2_hip_set_fp16_lanes(self._h, lanes), "yolo2_hip_set_fp16_lanes")

    def num_lanes_fp16(self) -> int:
        return int(lib().yolo2_hip_num_lanes_fp16(self._h))

    def plan_source(self) -> str:
        return {0: "none", 1: "plan table", 2: "autotuned in this process", 3: "static defaults", 4: "forced by a test hook",
                5: "weight cache"}[int(lib().yolo2_hip_plan_source(self._h))]

    def set_option(self, name: str, value=None):
        """One named option of the context (include/yolo2_hip.h "options"); None restores the default."""
        check(lib().yolo2_hip_set_option(self._h, name.encode(), None if value is None else str(value).encode()), f"yolo2_hip_set_option({name})")

    def options(self) -> str:
        if not hasattr(lib(), "yolo2_hip_options_string"):
            return "(library without option sets)"
        buf = C.create_string_buffer(1024)
        check(lib().yolo2_hip_options_string(self._h, buf, 1024), "yolo2_hip_options_string")
        return buf.value.decode()

    def ks_scratch_bytes(self) -> int:
        return int(lib().yolo2_hip_ks_scratch_bytes(self._h))

    def set_plan_cache(self, path):
        check(lib().yolo2_hip_set_plan_cache(self._h, None if path is None else str(path).encode()), "yolo2_hip_set_plan_cache")

    def plan_cache_info(self):
        h, used, n, nb = C.c_uint64(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().yolo2_hip_plan_cache_info(self._h, C.byref(h), C.byref(used), C.byref(n), C.byref(nb)), "yolo2_hip_plan_cache_info")
        return {"hash": h.value, "bounds_from_file": bool(used.value), "lines": n.value, "batches": nb.value}

    def conv_plan(self, ord_: int) -> str:
        buf = C.create_string_buffer(256)
        check(lib().yolo2_hip_conv_plan_string(self._h, ord_, buf, 256), "yolo2_hip_conv_plan_string")
        return buf.value.decode()

    def conv_launch_info(self, ord_: int):
        v = [C.c_int(0) for _ in range(5)]
        check(lib().yolo2_hip_conv_launch_info(self._h, ord_, *[C.byref(x) for x in v]), "conv_launch_info")
        return dict(zip(("grid_x", "grid_y", "block", "lds_bytes", "pixels_per_lane"), (x.value for x in v)))

    # ---- calibration: fp32 weights + frames -> int16 weights and Q tables (CalibratedModel below)
    def calib_reset(self):
        check(lib().yolo2_hip_calib_reset(self._h), "yolo2_hip_calib_reset")

    def calib_frames(self, frames: np.ndarray, stream: int = 0):
        """One exact fp32 pass over host frames [B][3][416][416] + the abs-max reductions, accumulated (yolo2_hip_calib_frames), on
        `stream` (0 = the null stream)."""
        buf = DevBuf(np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, 3, 416, 416))
        try:
            check(lib().yolo2_hip_calib_frames(self._h, buf.addr, buf.nbytes // (4 * 3 * 416 * 416), C.c_void_p(stream)), "yolo2_hip_calib_frames")
        finally:
            buf.free()

    def calib_images(self, images, batch: int, pixfmt=None):
        """The same from host images (uint8 arrays as run_images_host takes them), letterboxed on the GPU in chunks of `batch`."""
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        if pixfmt is None:
            pixfmt = "grey8" if imgs[0].ndim == 2 else "rgb24"
        n, ptrs, ws, hs, fmt, _keep = _image_args(imgs, pixfmt)
        check(lib().yolo2_hip_calib_images_pix_host(self._h, ptrs, ws, hs, fmt, n, batch), "yolo2_hip_calib_images_pix_host")

    def calib_stats(self):
        """dict(act_absmax [24], weight_absmax [23], bias_absmax [23], frames_seen) of the statistics accumulated so far"""
        nconv = len(net.CONVS)
        a, w, b = np.zeros(nconv + 1, np.float32), np.zeros(nconv, np.float32), np.zeros(nconv, np.float32)
        seen = C.c_long(0)
        vp = lambda v: v.ctypes.data_as(C.c_void_p)
        check(lib().yolo2_hip_calib_stats(self._h, vp(a), vp(w), vp(b), C.byref(seen)), "yolo2_hip_calib_stats")
        return {"act_absmax": a, "weight_absmax": w, "bias_absmax": b, "frames_seen": seen.value}

    def calib_q_tables(self, headroom: float = 1.0):
        nconv = len(net.CONVS)
        wq, bq, aq = np.zeros(nconv, np.int32), np.zeros(nconv, np.int32), np.zeros(nconv + 1, np.int32)
        vp = lambda v: v.ctypes.data_as(C.c_void_p)
        check(lib().yolo2_hip_calib_q_tables(self._h, headroom, vp(wq), vp(bq), vp(aq)), "yolo2_hip_calib_q_tables")
        return wq, bq, aq

    def quantize_weights(self, weight_q, bias_q):
        """The resident fp32 blobs as int16 = round(x * 2^Q) with the given tables, quantised on the GPU -> (weights, bias, clamped)."""
        wq, bq = (np.ascontiguousarray(q, dtype=np.int32) for q in (weight_q, bias_q))
        if wq.shape != (len(net.CONVS),) or bq.shape != wq.shape:
            raise ValueError(f"Q tables hold {len(net.CONVS)} entries each")
        w, b = np.empty(N_WEIGHTS, np.int16), np.empty(N_BIAS, np.int16)
        clamped = C.c_long(0)
        vp = lambda v: v.ctypes.data_as(C.c_void_p)
        check(lib().yolo2_hip_quantize_weights_int16(self._h, vp(wq), vp(bq), vp(w), w.size, vp(b), b.size, C.byref(clamped)),
              "yolo2_hip_quantize_weights_int16")
        return w, b, clamped.value

    def calibrate(self, frames=None, images=None, batch: int = 8, headroom: float = 1.0, pixfmt=None) -> "CalibratedModel":
        """fp32 weights (load_weights_fp32) + calibration frames (float [n][3][416][416]) or images -> a CalibratedModel: statistics of
        the exact fp32 pass in chunks of `batch`, the Q rule with `headroom`, the weights quantised on the GPU.  Starts from cleared
        statistics."""
        if (frames is None) == (images is None):
            raise ValueError("calibrate takes frames=... or images=..., not both")
        if batch < 1:
            raise ValueError("batch must be positive")
        self.calib_reset()
        if frames is not None:
            frames = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, 3, 416, 416)
            for i in range(0, frames.shape[0], batch):
                self.calib_frames(frames[i:i + batch])
        else:
            self.calib_images(images, batch, pixfmt)
        st = self.calib_stats()
        wq, bq, aq = self.calib_q_tables(headroom)
        w, b, clamped = self.quantize_weights(wq, bq)
        return CalibratedModel(w, b, wq, bq, aq, clamped, st["act_absmax"], st["weight_absmax"], st["bias_absmax"], st["frames_seen"])


    # ---- the int8 pass on the i8 matrix cores (include/yolo2_hip.h "int8 pass")
    def calib_q8_tables(self, headroom: float = 1.0) -> np.ndarray:
        aq = np.zeros(len(net.CONVS) + 1, np.int32)
        check(lib().yolo2_hip_calib_q8_tables(self._h, headroom, aq.ctypes.data_as(C.c_void_p)), "yolo2_hip_calib_q8_tables")
        return aq

    def quantize_weights_int8(self, act_q):
        """the resident fp32 blobs -> (w8 natural order, bias32 [10761], weight_q [10761]), quantised on the GPU"""
        aq = np.ascontiguousarray(act_q, dtype=np.int32)
        if aq.shape != (len(net.CONVS) + 1,):
            raise ValueError(f"act_q holds {len(net.CONVS) + 1} entries")
        w, b, q = np.empty(N_WEIGHTS, np.int8), np.empty(N_BIAS, np.int32), np.empty(N_BIAS, np.int32)
        vp = lambda v: v.ctypes.data_as(C.c_void_p)
        check(lib().yolo2_hip_quantize_weights_int8(self._h, vp(aq), vp(w), w.size, vp(b), b.size, vp(q)), "yolo2_hip_quantize_weights_int8")
        return w, b, q

    def calibrate_int8(self, frames=None, images=None, batch: int = 8, headroom: float = 1.0, pixfmt=None) -> "CalibratedModelI8":
        """fp32 weights (load_weights_fp32) + calibration frames or images -> a CalibratedModelI8: the statistics of calibrate(), the
        int8 Q rule with `headroom`, per-channel weight Qs, weights and biases quantised on the GPU."""
        if (frames is None) == (images is None):
            raise ValueError("calibrate_int8 takes frames=... or images=..., not both")
        if batch < 1:
            raise ValueError("batch must be positive")
        self.calib_reset()
        if frames is not None:
            frames = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, 3, 416, 416)
            for i in range(0, frames.shape[0], batch):
                self.calib_frames(frames[i:i + batch])
        else:
            self.calib_images(images, batch, pixfmt)
        st = self.calib_stats()
        aq = self.calib_q8_tables(headroom)
        w, b, q = self.quantize_weights_int8(aq)
        return CalibratedModelI8(w, b, q, aq, st["act_absmax"], st["frames_seen"])

    def load_weights_int8(self, w8, bias32, weight_q, act_q):
        w = np.ascontiguousarray(w8, dtype=np.int8)
        b, q, a = (np.ascontiguousarray(v, dtype=np.int32) for v in (bias32, weight_q, act_q))
        if q.size != b.size or a.size != len(net.CONVS) + 1:
            raise ValueError(f"weight_q holds one entry per bias ({b.size}), act_q {len(net.CONVS) + 1}")
        vp = lambda v: v.ctypes.data_as(C.c_void_p)
        check(lib().yolo2_hip_load_weights_int8(self._h, vp(w), w.size, vp(b), b.size, vp(q), vp(a)), "yolo2_hip_load_weights_int8")

    def run_batch_int8_ptr(self, frames_ptr: int, batch: int, region_ptr: int, stream: int = 0):
        check(lib().yolo2_hip_run_batch_int8(self._h, frames_ptr, batch, region_ptr, C.c_void_p(stream)), "yolo2_hip_run_batch_int8")

    def run_batch_int8_host(self, frames: np.ndarray) -> np.ndarray:
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        B = frames.shape[0]
        region = np.empty((B, 425, 13, 13), dtype=np.float32)
        check(lib().yolo2_hip_run_batch_int8_host(self._h, frames.ctypes.data_as(C.c_void_p), B, region.ctypes.data_as(C.c_void_p)),
              "yolo2_hip_run_batch_int8_host")
        return region

    def run_images_int8_host(self, images, batch: int, pixfmt=None) -> np.ndarray:
        """images (uint8 [h][w][3], [h][w] grey or - pixfmt "yuyv" - [h][w][2], any sizes) -> float32 region tensors [n][425][13][13]
        through the int8 pass; one kernel goes from the image bytes to layer 1 (yolo2_hip_run_images_pix_int8_host)."""
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        if pixfmt is None:
            pixfmt = "grey8" if imgs and imgs[0].ndim == 2 else "rgb24"
        n, ptrs, ws, hs, fmt, _keep = _image_args(imgs, pixfmt)
        region = np.empty((n, 425, 13, 13), dtype=np.float32)
        check(lib().yolo2_hip_run_images_pix_int8_host(self._h, ptrs, ws, hs, fmt, n, batch, region.ctypes.data_as(C.c_void_p)),
              "yolo2_hip_run_images_pix_int8_host")
        return region

    def images_front_kernel_int8(self) -> str:
        """What the last int8 images call ran up to layer 1: the fused kernel's name, or - option i8_no_front - the three launches
        of the frames route joined by " + " ("" before the first call)."""
        return lib().yolo2_hip_images_front_kernel_int8(self._h).decode()

    def debug_i8_tensor(self, layer_idx: int, frame: int = 0):
        """(int8 [C][H][W], Q) of layer `layer_idx`'s tensor in the last int8 run; -1 is the quantised input"""
        g = (C.c_int * 4)()
        check(lib().yolo2_hip_debug_i8_tensor(self._h, layer_idx, frame, None, 0, g), "yolo2_hip_debug_i8_tensor")
        out = np.empty((g[0], g[1], g[2]), dtype=np.int8)
        check(lib().yolo2_hip_debug_i8_tensor(self._h, layer_idx, frame, out.ctypes.data_as(C.c_void_p), out.size, g), "yolo2_hip_debug_i8_tensor")
        return out, int(g[3])


# ------------------------------------------------------------------ calibration: fp32 weights + frames -> an int16 weight set

N_WEIGHTS, N_BIAS = net.N_WEIGHTS, net.N_BIAS   # include/yolo2_hip.h YOLO2_N_WEIGHTS / YOLO2_N_BIAS


def absmax_f32(dev_addr: int, n: int, stream: int = 0):
    """(max |x|, count of Inf / NaN) of n floats in HBM (yolo2_hip_absmax_f32); non-finite values are left out of the maximum."""
    m, bad = C.c_float(0), C.c_uint32(0)
    check(lib().yolo2_hip_absmax_f32(dev_addr, n, C.byref(m), C.byref(bad), C.c_void_p(stream)), "yolo2_hip_absmax_f32")
    return np.float32(m.value), int(bad.value)


def q_tables_from_stats(act_absmax, weight_absmax, bias_absmax, headroom: float = 1.0):
    """The Q rule on explicit maxima (yolo2_hip_calib_q_from_stats; host arithmetic, no GPU): q = the largest integer in 0..15 with
    headroom * max * 2^q < 32767.5, i.e. still rounding to at most 32767 (headroom on the conv outputs only), then the concat
    fix-up.  -> (weight_q, bias_q, act_q)."""
    nconv = len(net.CONVS)
    a, w, b = (np.ascontiguousarray(v, dtype=np.float32) for v in (act_absmax, weight_absmax, bias_absmax))
    if a.shape != (nconv + 1,) or w.shape != (nconv,) or b.shape != (nconv,):
        raise ValueError(f"maxima are [{nconv + 1}] activations, [{nconv}] weights, [{nconv}] biases")
    wq, bq, aq = np.zeros(nconv, np.int32), np.zeros(nconv, np.int32), np.zeros(nconv + 1, np.int32)
    vp = lambda v: v.ctypes.data_as(C.c_void_p)
    check(lib().yolo2_hip_calib_q_from_stats(vp(a), vp(w), vp(b), headroom, vp(wq), vp(bq), vp(aq)), "yolo2_hip_calib_q_from_stats")
    return wq, bq, aq


class CalibratedModel:
    """An int16 weight set made by Yolo2Hip.calibrate / quantize_weights: what load_model, orclib.forward_i16 and the other users of
    a synth.SynthModel read (weights_i16(), bias_i16(), the three Q tables), and the reference's five files."""

    FILES = ("weights_reorg_int16.bin", "bias_int16.bin", "weight_int16_Q.bin", "bias_int16_Q.bin", "iofm_Q.bin")

    def __init__(self, weights_i16, bias_i16, weight_q, bias_q, act_q, clamped=0, act_absmax=None, weight_absmax=None,
                 bias_absmax=None, frames_seen=0):
        self._w = np.ascontiguousarray(weights_i16, dtype=np.int16)
        self._b = np.ascontiguousarray(bias_i16, dtype=np.int16)
        self.weight_q, self.bias_q, self.act_q = (np.array(q, dtype=np.int32) for q in (weight_q, bias_q, act_q))
        nconv = len(net.CONVS)
        if self._w.shape != (N_WEIGHTS,) or self._b.shape != (N_BIAS,) or self.weight_q.shape != (nconv,) or \
                self.bias_q.shape != (nconv,) or self.act_q.shape != (nconv + 1,):
            raise ValueError("not a YOLOv2 int16 weight set")
        self.clamped, self.frames_seen = int(clamped), int(frames_seen)
        self.act_absmax, self.weight_absmax, self.bias_absmax = act_absmax, weight_absmax, bias_absmax

    def weights_i16(self) -> np.ndarray:
        return self._w

    def bias_i16(self) -> np.ndarray:
        return self._b

    @staticmethod
    def _with_layer_pad(flat, lens):
        """the stream with one zero element after every odd-length layer (synth.SynthModel.write_files; yolo2_model.cpp:198-224)"""
        out, off = [], 0
        for n in lens:
            out.append(flat[off:off + n])
            if n & 1:
                out.append(np.zeros(1, dtype=flat.dtype))
            off += n
        return np.concatenate(out)

    def write_files(self, weights_dir: str):
        os.makedirs(weights_dir, exist_ok=True)
        arrays = (self._with_layer_pad(self._w, net.WEIGHT_LEN),
                  self._with_layer_pad(self._b, net.BIAS_LEN), self.weight_q, self.bias_q, self.act_q)
        paths = {}
        for name, arr in zip(self.FILES, arrays):
            paths[name] = os.path.join(weights_dir, name)
            arr.tofile(paths[name])
        return paths

    @classmethod
    def read_files(cls, weights_dir: str):
        """the five files back (per-layer pads stripped)"""
        def strip(flat, lens):
            out, off = [], 0
            for n in lens:
                out.append(flat[off:off + n])
                off += n + (n & 1)
            if off != flat.size:
                raise ValueError(f"{flat.size} elements on file, the layer table wants {off}")
            return np.concatenate(out)
        rd = lambda name, dt: np.fromfile(os.path.join(weights_dir, name), dtype=dt)
        return cls(strip(rd(cls.FILES[0], np.int16), net.WEIGHT_LEN), strip(rd(cls.FILES[1], np.int16), net.BIAS_LEN),
                   rd(cls.FILES[2], np.int32), rd(cls.FILES[3], np.int32), rd(cls.FILES[4], np.int32))


def q8_from_stats(act_absmax, headroom: float = 1.0) -> np.ndarray:
    """The int8 Q rule on explicit activation maxima [24] (yolo2_hip_calib_q8_from_stats; host arithmetic, no GPU): the largest q in
    -8..24 with headroom * max * 2^q < 127.5, then the concat fix-up -> act_q [24]."""
    a = np.ascontiguousarray(act_absmax, dtype=np.float32)
    if a.shape != (len(net.CONVS) + 1,):
        raise ValueError(f"maxima are [{len(net.CONVS) + 1}] activations")
    aq = np.zeros(a.size, np.int32)
    check(lib().yolo2_hip_calib_q8_from_stats(a.ctypes.data_as(C.c_void_p), headroom, aq.ctypes.data_as(C.c_void_p)),
          "yolo2_hip_calib_q8_from_stats")
    return aq


class CalibratedModelI8:
    """An int8 weight set made by Yolo2Hip.calibrate_int8: w8 int8 [50941792] in natural [N][C][K][K] order per layer, bias32 and
    weight_q int32 [10761] (one per output channel), act_q int32 [24].  load_model takes it."""

    FILES = ("weights_int8.bin", "bias_int32.bin", "weight_int8_Q.bin", "iofm_int8_Q.bin")

    def __init__(self, w8, bias32, weight_q, act_q, act_absmax=None, frames_seen=0):
        self.w8 = np.ascontiguousarray(w8, dtype=np.int8)
        self.bias32, self.weight_q, self.act_q = (np.array(v, dtype=np.int32) for v in (bias32, weight_q, act_q))
        if self.w8.shape != (N_WEIGHTS,) or self.bias32.shape != (N_BIAS,) or self.weight_q.shape != (N_BIAS,) or \
                self.act_q.shape != (len(net.CONVS) + 1,):
            raise ValueError("not a YOLOv2 int8 weight set")
        self.act_absmax, self.frames_seen = act_absmax, int(frames_seen)

    def write_files(self, weights_dir: str):
        os.makedirs(weights_dir, exist_ok=True)
        paths = {}
        for name, arr in zip(self.FILES, (self.w8, self.bias32, self.weight_q, self.act_q)):
            paths[name] = os.path.join(weights_dir, name)
            arr.tofile(paths[name])
        return paths

    @classmethod
    def read_files(cls, weights_dir: str):
        rd = lambda name, dt: np.fromfile(os.path.join(weights_dir, name), dtype=dt)
        return cls(rd(cls.FILES[0], np.int8), rd(cls.FILES[1], np.int32), rd(cls.FILES[2], np.int32), rd(cls.FILES[3], np.int32))


# ------------------------------------------------------------------ post-processing on the GPU

DET_DTYPE = np.dtype([("frame", np.int32), ("det", np.int32), ("cls", np.int32), ("prob", np.float32),
                      ("x", np.float32), ("y", np.float32), ("w", np.float32), ("h", np.float32)])


TAILS = ("core", "app")


def _check_tail(tail):
    if tail not in TAILS:
        raise ValueError(f"tail must be one of {TAILS}, not {tail!r}")
    return tail == "app"


def postprocess(ctx, region_ptr: int, batch: int, im_w, im_h, thresh: float, nms: float, final_q: int = None, cap: int = 256,
                want_rows: bool = False, want_proc: bool = False, stream: int = 0, tail: str = "core"):
    """yolo2_hip_postprocess_int16 (final_q given) / _f32 on a DEVICE region tensor.  Returns a dict with
    dets (structured array of the records kept), counts, and optionally rows [B][845][85], totals, proc.
    tail "core" restates the reference's src/core tail, "app" (the _app entries) its camera loop's yolo2_postprocess.c."""
    sfx = "_app" if _check_tail(tail) else ""
    iw = np.ascontiguousarray(im_w, dtype=np.int32)
    ih = np.ascontiguousarray(im_h, dtype=np.int32)
    assert iw.size == batch and ih.size == batch
    dets = np.zeros((batch, cap), dtype=DET_DTYPE)
    counts = np.zeros(batch, dtype=np.int32)
    rows = np.zeros((batch, 845, 85), dtype=np.float32) if want_rows else None
    totals = np.zeros(batch, dtype=np.int32)
    proc = np.zeros((batch, 425 * 169), dtype=np.float32) if want_proc else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    if final_q is not None:
        rc = getattr(lib(), "yolo2_hip_postprocess_int16" + sfx)(ctx._h, region_ptr, batch, int(final_q), vp(iw), vp(ih), thresh, nms, vp(dets), cap,
                                               vp(counts), vp(rows), vp(totals), vp(proc), C.c_void_p(stream))
    else:
        rc = getattr(lib(), "yolo2_hip_postprocess_f32" + sfx)(ctx._h, region_ptr, batch, vp(iw), vp(ih), thresh, nms, vp(dets), cap, vp(counts),
                                             vp(rows), vp(totals), vp(proc), C.c_void_p(stream))
    check(rc, "yolo2_hip_postprocess")
    return {"dets": [dets[f, :min(int(counts[f]), cap)] for f in range(batch)], "counts": counts, "rows": rows, "totals": totals, "proc": proc}


def live_bytes():
    """(device bytes, pinned bytes) the library's contexts and calls hold right now (yolo2_hip_debug_live_bytes, a test hook)."""
    d, p = C.c_size_t(0), C.c_size_t(0)
    check(lib().yolo2_hip_debug_live_bytes(C.byref(d), C.byref(p)), "yolo2_hip_debug_live_bytes")
    return d.value, p.value


DETS_BEST_CLASS = 1
DETS_APP_TAIL = 2


def _image_args(images, pixfmt=None):
    """(n, pointer array, widths, heights, channels - or, with a pixfmt, its YOLO2_PIX_* code -, the contiguous arrays the pointers
    point into)"""
    imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
    n = len(imgs)
    ch = (1 if imgs[0].ndim == 2 else imgs[0].shape[2]) if pixfmt is None else _pix_code(pixfmt, imgs)
    ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
    ws = (C.c_int * n)(*[im.shape[1] for im in imgs])
    hs = (C.c_int * n)(*[_pix_hw(pixfmt, im.shape)[0] for im in imgs])
    return n, ptrs, ws, hs, ch, imgs


PRECISIONS = ("int16", "fp16", "fp32fast", "int8")


def run_images_dets(handle, images, batch: int, thresh: float, nms: float, cap: int = 845, best_class: bool = True, multi: bool = False,
                    precision: str = "int16", pixfmt=None, tail: str = "core"):
    """yolo2_hip_run_images_u8_dets / yolo2_hip_multi_run_images_u8_dets: host images (uint8 [h][w][3]) -> per-frame detection
    records; letterbox, network and the tail run on the device(s), the region tensor never leaves HBM.  precision "fp16" /
    "fp32fast" (the split-fp16 pass) run the _dets_f16 entries instead (fp32 weights loaded); their final_q is None.
    precision "int8": yolo2_hip_run_images_pix_dets_int8 (int8 weights loaded, single device; final_q None).
    pixfmt "grey8" / "rgb24" / "yuyv" (arrays [h][w][2]) / "nv12" / "i420" (arrays [h * 3 / 2][w]) / "bgr24" ([h][w][3]) / "rgba32" / "bgra32" ([h][w][4]): the _pix_dets entries with that format; None infers grey / RGB.
    tail "app" sets YOLO2_DETS_APP_TAIL: the records are those of the reference's camera loop (yolo2_postprocess.c)."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, not {precision!r}")
    if precision == "int8":
        if multi:
            raise ValueError("the multi-GPU entries have no int8 form")
        if pixfmt is None:                                         # (the int8 entries are _pix entries only)
            first = np.asarray(images[0]) if len(images) else None
            pixfmt = "grey8" if first is not None and first.ndim == 2 else "rgb24"
    app_tail = _check_tail(tail)
    n, ptrs, ws, hs, ch, _keep = _image_args(images, pixfmt)
    kind = "u8" if pixfmt is None else "pix"
    dets = np.zeros((n, cap), dtype=DET_DTYPE)
    counts = np.zeros(n, dtype=np.int32)
    flags = (DETS_BEST_CLASS if best_class else 0) | (DETS_APP_TAIL if app_tail else 0)
    if precision == "int8":
        name = "yolo2_hip_run_images_pix_dets_int8"
        check(getattr(lib(), name)(handle, ptrs, ws, hs, ch, n, batch, thresh, nms, flags, dets.ctypes.data_as(C.c_void_p), cap,
                                   counts.ctypes.data_as(C.c_void_p)), name)
        return {"dets": [dets[f, :min(int(counts[f]), cap)] for f in range(n)], "counts": counts, "final_q": None}
    if precision != "int16":
        split = int(precision == "fp32fast")
        name = f"yolo2_hip_{'multi_' if multi else ''}run_images_{kind}_dets_f16"
        check(getattr(lib(), name)(handle, split, ptrs, ws, hs, ch, n, batch, thresh, nms, flags, dets.ctypes.data_as(C.c_void_p), cap,
                                   counts.ctypes.data_as(C.c_void_p)), name)
        return {"dets": [dets[f, :min(int(counts[f]), cap)] for f in range(n)], "counts": counts, "final_q": None}
    q = C.c_int(0)
    name = f"yolo2_hip_{'multi_' if multi else ''}run_images_{kind}_dets"
    check(getattr(lib(), name)(handle, ptrs, ws, hs, ch, n, batch, thresh, nms, flags, dets.ctypes.data_as(C.c_void_p), cap,
                               counts.ctypes.data_as(C.c_void_p), C.byref(q)), name)
    return {"dets": [dets[f, :min(int(counts[f]), cap)] for f in range(n)], "counts": counts, "final_q": q.value}


# ------------------------------------------------------------------ JPEG streams decoded on the GPU

class JpegInfo(C.Structure):
    """yolo2_hip_jpeg_info_t"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("components", C.c_int), ("hmax", C.c_int), ("vmax", C.c_int),
                ("restart_interval", C.c_int), ("gpu_decodable", C.c_int), ("reason", C.c_int), ("stream_bytes", C.c_size_t)]


JPEG_REASONS = ("accepted", "damaged", "progressive", "unsupported_sof", "components", "rgb_colour", "sampling", "scans", "missing_table",
                "too_large")
JPEG_PRECISIONS = {"int16": 0, "fp16": 1, "fp32fast": 2, "int8": 3}


def jpeg_probe(data) -> dict:
    """yolo2_hip_jpeg_probe (host only): the header's geometry, whether the GPU decoder takes the stream (reason: index into
    JPEG_REASONS) and stream_bytes, the offset just past EOI, which cuts a concatenated MJPEG stream."""
    buf = bytes(data)
    info = JpegInfo()
    check(lib().yolo2_hip_jpeg_probe(buf, len(buf), C.byref(info)), "yolo2_hip_jpeg_probe")
    return {k: getattr(info, k) for k, _ in JpegInfo._fields_}


_SPLIT_INFO = ("subsequences", "split_segments", "fallback_segments", "short_segments", "max_rounds", "split_bytes")


def _split_info(v) -> dict:
    d = {k: int(v[i]) for i, k in enumerate(_SPLIT_INFO)}
    d.update(split_ms=v[6], fallback_ms=v[7])
    return d


def jpeg_decode_ref(data, cap: int = None, split: int = None):
    """yolo2_hip_decode_jpeg_ref: the GPU decoder's stages run on the host -> (uint8 [h][w][3] or None, status).  A stream the probe
    refuses gives (None, 100 + reason).  split = S bytes: yolo2_hip_decode_jpeg_split_ref, the entropy stage as option jpegdec_split
    runs it (many lanes per segment, here as loops) -> (picture or None, status, info as jpeg_split_info's)."""
    buf = bytes(data)
    info = jpeg_probe(buf)
    out = np.zeros(max(1, info["width"] * info["height"] * 3) if cap is None else cap, dtype=np.uint8)
    w, h, st = C.c_int(0), C.c_int(0), C.c_int(0)
    if split is None:
        name, extra = "yolo2_hip_decode_jpeg_ref", ()
        rc = lib().yolo2_hip_decode_jpeg_ref(buf, len(buf), out.ctypes.data_as(C.c_void_p), out.size, C.byref(w), C.byref(h), C.byref(st))
    else:
        v = (C.c_double * 8)()
        name = "yolo2_hip_decode_jpeg_split_ref"
        rc = lib().yolo2_hip_decode_jpeg_split_ref(buf, len(buf), int(split), out.ctypes.data_as(C.c_void_p), out.size, C.byref(w), C.byref(h),
                                                   C.byref(st), v)
        extra = (_split_info(v),)
    if rc != YOLO2_SUCCESS and st.value < 100:
        check(rc, name)
    if st.value:
        return (None, st.value) + extra
    return (out[:w.value * h.value * 3].reshape(h.value, w.value, 3), 0) + extra


def jpeg_last_info(handle) -> dict:
    """yolo2_hip_jpeg_last_info: per-chunk kernel milliseconds (under set_profiling) and uploaded bytes of the last JPEG call"""
    v = (C.c_double * 8)()
    check(lib().yolo2_hip_jpeg_last_info(handle, v), "yolo2_hip_jpeg_last_info")
    return {"memset_ms": v[0], "entropy_ms": v[1], "idct_ms": v[2], "rgb_ms": v[3], "stream_bytes_h2d": int(v[4]), "frame_bytes_h2d": int(v[5]),
            "chunks": int(v[6]), "frames": int(v[7])}


def jpeg_split_info(handle) -> dict:
    """yolo2_hip_jpeg_split_info: what option jpegdec_split did in the last JPEG call (all zero when it was unset)"""
    v = (C.c_double * 8)()
    check(lib().yolo2_hip_jpeg_split_info(handle, v), "yolo2_hip_jpeg_split_info")
    return _split_info(v)


def _stream_args(streams):
    bufs = [bytes(s) for s in streams]
    n = len(bufs)
    ptrs = (C.c_char_p * n)(*bufs)
    sizes = (C.c_size_t * n)(*[len(b) for b in bufs])
    return n, ptrs, sizes, bufs


def jpeg_decode(handle, streams, batch: int = 64, strict: bool = True):
    """yolo2_hip_decode_jpeg_host: a list of JPEG streams -> (list of uint8 [h][w][3], status int32 [n]); the whole decoder runs on
    the device.  A stream the probe refuses raises.  A frame the decoder flags (status != 0) comes back zero-filled: with strict
    that raises too, otherwise the caller looks at status."""
    n, ptrs, sizes, bufs = _stream_args(streams)
    infos = [jpeg_probe(b) for b in bufs]
    outs = [np.zeros((max(1, i["height"]), max(1, i["width"]), 3), dtype=np.uint8) for i in infos]
    optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    caps = (C.c_size_t * n)(*[o.size for o in outs])
    ws, hs = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib().yolo2_hip_decode_jpeg_host(handle, ptrs, sizes, n, batch, optrs, caps, vp(ws), vp(hs), vp(status))
    if rc != YOLO2_SUCCESS and (strict or not status.any()):
        check(rc, "yolo2_hip_decode_jpeg_host")
    return [o[:hs[i], :ws[i]] for i, o in enumerate(outs)], status


def _mixed_stream_args(streams):
    """streams (bytes) and raw frames (uint8 [h][w][3] arrays) -> (n, pointers, sizes - 0 for a raw frame -, widths, heights, what keeps
    the buffers alive): the argument lists of the entries that take JPEG streams with raw frames mixed in"""
    keep, n = [], len(streams)
    ptrs, sizes = (C.c_void_p * n)(), (C.c_size_t * n)()
    ws, hs = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for i, s in enumerate(streams):
        if isinstance(s, np.ndarray):
            a = np.ascontiguousarray(s, dtype=np.uint8)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"frame {i}: a raw frame is uint8 [h][w][3], not {a.shape}")
            keep.append(a)
            ptrs[i], sizes[i], ws[i], hs[i] = a.ctypes.data, 0, a.shape[1], a.shape[0]
        else:
            b = C.create_string_buffer(bytes(s), len(s))
            keep.append(b)
            ptrs[i], sizes[i] = C.addressof(b), len(s)
    return n, ptrs, sizes, ws, hs, keep


def run_jpegs_dets(handle, streams, batch: int, thresh: float, nms: float, cap: int = 845, best_class: bool = True, precision: str = "int16",
                   tail: str = "core", strict: bool = True, multi: bool = False):
    """yolo2_hip_run_images_jpeg_dets / its multi form: JPEG streams (bytes) - or, mixed in, raw frames (uint8 [h][w][3] arrays, e.g. decoded on the
    host) - -> detection records, the decoder and the network on the device.  Returns run_images_dets' dictionary plus "status"
    (int32 [n], not 0: the decoder flagged the frame, its counts are 0) and "sizes" ([n] (w, h))."""
    if precision not in JPEG_PRECISIONS:
        raise ValueError(f"precision must be one of {tuple(JPEG_PRECISIONS)}, not {precision!r}")
    app_tail = _check_tail(tail)
    if multi and precision == "int8":
        raise ValueError("the multi-GPU entries have no int8 form")
    n, ptrs, sizes, ws, hs, _keep = _mixed_stream_args(streams)
    dets = np.zeros((n, cap), dtype=DET_DTYPE)
    counts, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    flags = (DETS_BEST_CLASS if best_class else 0) | (DETS_APP_TAIL if app_tail else 0)
    q = C.c_int(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    name = f"yolo2_hip_{'multi_' if multi else ''}run_images_jpeg_dets"
    rc = getattr(lib(), name)(handle, JPEG_PRECISIONS[precision], ptrs, sizes, vp(ws), vp(hs), n, batch, thresh, nms, flags, vp(dets),
                              cap, vp(counts), C.byref(q), vp(status))
    if rc != YOLO2_SUCCESS and (strict or not status.any()):
        check(rc, name)
    return {"dets": [dets[f, :min(int(counts[f]), cap)] for f in range(n)], "counts": counts, "final_q": q.value if precision == "int16" else None,
            "status": status, "sizes": [(int(ws[i]), int(hs[i])) for i in range(n)]}


# ------------------------------------------------------------------ annotated frames

def _label_args(labels):
    """(char ** or None, n_labels, what keeps the strings alive)"""
    if labels is None:
        return None, 0, None
    enc = [None if s is None else s.encode() if isinstance(s, str) else bytes(s) for s in labels]      # (None: a null entry, "class<cls>")
    arr = (C.c_char_p * max(len(enc), 1))(*enc)
    return arr, len(enc), enc


def annotate_pix(image: np.ndarray, dets, pixfmt=None, thresh: float = 0.24, labels=None, stream: int = 0):
    """yolo2_hip_annotate_pix: one image ("grey8" [h][w], "rgb24" [h][w][3], "yuyv" [h][w][2], "nv12" / "i420" [h * 3 / 2][w], "bgr24" [h][w][3], "rgba32" / "bgra32" [h][w][4]; None infers grey / RGB) and its
    records (DET_DTYPE, one per detection) -> (uint8 [h][w][3] with the reference's boxes and tags painted in, records drawn)."""
    im = np.ascontiguousarray(image, dtype=np.uint8)
    fmt = pixfmt if pixfmt is not None else ("grey8" if im.ndim == 2 else "rgb24")
    code = _pix_code(fmt, [im])
    h, w = _pix_hw(fmt, im.shape)
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE).reshape(-1)
    lab, n_labels, _keep = _label_args(labels)
    L = lib()
    src, dst = C.c_uint64(0), C.c_uint64(0)
    out = np.empty((h, w, 3), dtype=np.uint8)
    drawn = C.c_int(0)
    try:
        check(L.yolo2_hip_alloc(max(im.nbytes, 16), C.byref(src)), "alloc")
        check(L.yolo2_hip_alloc(max(out.nbytes, 16), C.byref(dst)), "alloc")
        check(L.yolo2_hip_memcpy_h2d(src, im.ctypes.data_as(C.c_void_p), im.nbytes), "h2d")
        check(L.yolo2_hip_annotate_pix(src, w, h, code, d.ctypes.data_as(C.c_void_p) if d.size else None, d.size,
                                       thresh, lab, n_labels, dst, C.byref(drawn), C.c_void_p(stream)), "yolo2_hip_annotate_pix")
        check(L.yolo2_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), dst, out.nbytes), "d2h")
    finally:
        for buf in (src, dst):
            if buf.value:
                L.yolo2_hip_free(buf)
    return out, drawn.value


def annotate_images(handle, images, dets, counts, batch: int, thresh: float, labels=None, pixfmt=None, multi: bool = False, jpeg_quality=None):
    """yolo2_hip_annotate_images_pix_host / yolo2_hip_multi_annotate_images_pix_host: host images and the records a run_images_dets call
    returned for them -> (list of uint8 [h][w][3] annotated frames, records drawn per frame).  dets: DET_DTYPE [n][cap] with counts [n]
    (frame f uses min(counts[f], cap) records), or - counts None - a list of per-frame record arrays (run_images_dets()["dets"]).
    jpeg_quality (1..100): the _jpeg_host entries instead - the frames come back as the reference's JPEG streams, a list of bytes."""
    if jpeg_quality is not None:
        return annotate_images_jpeg(handle, images, dets, counts, batch, thresh, int(jpeg_quality), labels=labels, pixfmt=pixfmt, multi=multi)
    imgs0 = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
    fmt = pixfmt if pixfmt is not None else ("grey8" if imgs0[0].ndim == 2 else "rgb24")
    n, ptrs, ws, hs, code, imgs = _image_args(imgs0, fmt)
    if counts is None:
        cap = max([len(d) for d in dets] + [1])
        packed = np.zeros((n, cap), dtype=DET_DTYPE)
        for f, d in enumerate(dets):
            packed[f, :len(d)] = d
        dets, counts = packed, [len(d) for d in dets]
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE)
    if d.ndim != 2 or d.shape[0] != n:
        raise ValueError(f"dets is [n][cap] records for {n} images, not {d.shape}")
    cnt = np.ascontiguousarray(counts, dtype=np.int32)
    lab, n_labels, _keep = _label_args(labels)
    outs = [np.empty(_pix_hw(fmt, im.shape) + (3,), dtype=np.uint8) for im in imgs]
    optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    drawn = np.zeros(n, dtype=np.int32)
    name = f"yolo2_hip_{'multi_' if multi else ''}annotate_images_pix_host"
    check(getattr(lib(), name)(handle, ptrs, ws, hs, code, n, batch, d.ctypes.data_as(C.c_void_p), d.shape[1], cnt.ctypes.data_as(C.c_void_p),
                               thresh, lab, n_labels, optrs, drawn.ctypes.data_as(C.c_void_p)), name)
    return outs, drawn


# ------------------------------------------------------------------ annotated frames as JPEG

_host_lib = None


def host_lib():
    """libyolo2_host.so: the host restatements the GPU entries are checked against"""
    global _host_lib
    if _host_lib is None:
        H = C.CDLL(HOST_LIB_PATH)
        H.y2h_write_jpg_rgb24.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        H.y2h_write_jpg_rgb24.restype = C.c_long
        H.y2h_jpg_rgb24_bound.argtypes = [C.c_int, C.c_int]
        H.y2h_jpg_rgb24_bound.restype = C.c_size_t
        H.y2h_packed_to_rgb24.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        H.y2h_packed_to_rgb24.restype = C.c_int
        H.y2h_rgb24_to_yuv420.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        H.y2h_rgb24_to_yuv420.restype = C.c_int
        H.y2h_last_error.restype = C.c_char_p
        _host_lib = H
    return _host_lib


def packed_to_rgb24_host(image, pixfmt: str) -> np.ndarray:
    """y2h_packed_to_rgb24: a "bgr24" [h][w][3] / "rgba32" / "bgra32" [h][w][4] frame -> uint8 [h][w][3] RGB24, the bytes reordered on
    the host (the fourth byte is not read) - what the GPU entries' fetch does per pixel"""
    if pixfmt not in PIXFMTS_PACKED:
        raise ValueError(f"pixfmt must be one of {PACKED_RGB}, not {pixfmt!r}")
    im = np.ascontiguousarray(image, dtype=np.uint8)
    _pix_code(pixfmt, [im])
    H = host_lib()
    out = np.empty((im.shape[0], im.shape[1], 3), dtype=np.uint8)
    if H.y2h_packed_to_rgb24(im.ctypes.data, im.shape[1], im.shape[0], PIXFMTS_PACKED[pixfmt], out.ctypes.data) != 0:
        raise ValueError(H.y2h_last_error().decode())
    return out


def rgb24_to_yuv420(im, fmt: str) -> np.ndarray:
    """y2h_rgb24_to_yuv420: an RGB24 frame uint8 [h][w][3] (w, h even) -> uint8 [h * 3 / 2][w], the "nv12" or "i420" frame the loop
    returns with out_order=fmt - the library's own integer BT.601 studio-range conversion, chroma from each 2x2 block's sums"""
    if fmt not in ("nv12", "i420"):
        raise ValueError(f"fmt must be 'nv12' or 'i420', not {fmt!r}")
    rgb = _rgb24(im)
    h, w = rgb.shape[:2]
    H = host_lib()
    out = np.empty((h * 3 // 2, w), dtype=np.uint8)
    if H.y2h_rgb24_to_yuv420(rgb.ctypes.data, w, h, 1 if fmt == "nv12" else 0, out.ctypes.data) != 0:
        raise ValueError(H.y2h_last_error().decode())
    return out


def _rgb24(rgb):
    im = np.ascontiguousarray(rgb, dtype=np.uint8)
    if im.ndim != 3 or im.shape[2] != 3:
        raise ValueError(f"an RGB24 frame is uint8 [h][w][3], not {im.shape}")
    return im


def write_jpg_host(rgb, quality: int = 80) -> bytes:
    """y2h_write_jpg_rgb24: an RGB24 frame as the JPEG stream of the reference's MJPEG streamer, encoded on the host"""
    im = _rgb24(rgb)
    H = host_lib()
    cap = H.y2h_jpg_rgb24_bound(im.shape[1], im.shape[0])
    out = np.empty(max(cap, 1), dtype=np.uint8)
    n = H.y2h_write_jpg_rgb24(im.ctypes.data, im.shape[1], im.shape[0], quality, out.ctypes.data, cap)
    if n < 0 or n > cap:
        raise ValueError(f"y2h_write_jpg_rgb24 refused a {im.shape[1]}x{im.shape[0]} frame")
    return out[:n].tobytes()


def jpeg_bound(w: int, h: int) -> int:
    """yolo2_hip_jpeg_bound: the most bytes the stream of a w x h frame can take"""
    return int(lib().yolo2_hip_jpeg_bound(w, h))


def jpeg_encode(rgb, quality: int = 80, stream: int = 0) -> bytes:
    """yolo2_hip_jpeg_encode_rgb24: the same stream as write_jpg_host, encoded on the GPU"""
    im = _rgb24(rgb)
    L = lib()
    h, w = im.shape[:2]
    cap = jpeg_bound(w, h)
    if not cap:
        raise ValueError(f"width and height are 1..65535, not {w}x{h}")
    src, dst = C.c_uint64(0), C.c_uint64(0)
    size = C.c_size_t(0)
    try:
        check(L.yolo2_hip_alloc(max(im.nbytes, 16), C.byref(src)), "alloc")
        check(L.yolo2_hip_alloc(cap, C.byref(dst)), "alloc")
        check(L.yolo2_hip_memcpy_h2d(src, im.ctypes.data_as(C.c_void_p), im.nbytes), "h2d")
        check(L.yolo2_hip_jpeg_encode_rgb24(src, w, h, quality, dst, cap, C.byref(size), C.c_void_p(stream)), "yolo2_hip_jpeg_encode_rgb24")
        out = np.empty(size.value, dtype=np.uint8)
        check(L.yolo2_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), dst, out.nbytes), "d2h")
    finally:
        for buf in (src, dst):
            if buf.value:
                L.yolo2_hip_free(buf)
    return out.tobytes()


def annotate_images_jpeg_raw(handle, images, dets, counts, batch: int, thresh: float, quality: int, caps, labels=None, pixfmt=None,
                             multi: bool = False, guard: int = 0):
    """The _jpeg_host entries as they are: caps [n] bytes of room per frame -> (return code, list of uint8 [caps[f] + guard] buffers -
    with a guard, every byte of them 0xA5 before the call -, sizes [n], records drawn [n])."""
    imgs0 = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
    fmt = pixfmt if pixfmt is not None else ("grey8" if imgs0[0].ndim == 2 else "rgb24")
    n, ptrs, ws, hs, code, imgs = _image_args(imgs0, fmt)
    if counts is None:
        cap = max([len(d) for d in dets] + [1])
        packed = np.zeros((n, cap), dtype=DET_DTYPE)
        for f, d in enumerate(dets):
            packed[f, :len(d)] = d
        dets, counts = packed, [len(d) for d in dets]
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE)
    if d.ndim != 2 or d.shape[0] != n:
        raise ValueError(f"dets is [n][cap] records for {n} images, not {d.shape}")
    cnt = np.ascontiguousarray(counts, dtype=np.int32)
    lab, n_labels, _keep = _label_args(labels)
    caps = np.ascontiguousarray(caps, dtype=np.uint64)
    if guard:
        outs = [np.full(int(caps[f]) + guard, 0xA5, dtype=np.uint8) for f in range(n)]
    else:       # (untouched pages: filling them would cost what the RGB24 entry's copy of the frames costs)
        outs = [np.empty(int(caps[f]), dtype=np.uint8) for f in range(n)]
    optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    sizes = np.zeros(n, dtype=np.uint64)
    drawn = np.zeros(n, dtype=np.int32)
    name = f"yolo2_hip_{'multi_' if multi else ''}annotate_images_pix_jpeg_host"
    rc = getattr(lib(), name)(handle, ptrs, ws, hs, code, n, batch, d.ctypes.data_as(C.c_void_p), d.shape[1], cnt.ctypes.data_as(C.c_void_p),
                              thresh, lab, n_labels, quality, optrs, caps.ctypes.data_as(C.c_void_p), sizes.ctypes.data_as(C.c_void_p),
                              drawn.ctypes.data_as(C.c_void_p))
    return rc, outs, sizes, drawn


def annotate_images_jpeg(handle, images, dets, counts, batch: int, thresh: float, quality: int = 80, labels=None, pixfmt=None, multi: bool = False):
    """yolo2_hip_annotate_images_pix_jpeg_host / its multi form: annotate_images, with the frames back as JPEG streams ->
    (list of bytes, records drawn per frame).  Room per frame: the raw frame's size, and - for the rare frame that compresses to
    more than that - a second call with the encoder's bound."""
    shapes = [_pix_hw(pixfmt, np.asarray(im).shape) for im in images]
    caps = [min(jpeg_bound(s[1], s[0]), s[0] * s[1] * 3 + 4096) for s in shapes]
    for attempt in range(2):
        rc, outs, sizes, drawn = annotate_images_jpeg_raw(handle, images, dets, counts, batch, thresh, quality, caps, labels=labels, pixfmt=pixfmt,
                                                          multi=multi)
        if rc == YOLO2_SUCCESS or attempt or not any(int(sizes[f]) > caps[f] for f in range(len(caps))):
            break
        caps = [jpeg_bound(s[1], s[0]) for s in shapes]
    check(rc, "yolo2_hip_annotate_images_pix_jpeg_host")
    return [outs[f][:int(sizes[f])].tobytes() for f in range(len(outs))], drawn


# ------------------------------------------------------------------ the camera loop as one call

LOOP_PRECISIONS = {"int16": 0, "fp16": 1, "fp32fast": 2}


class LoopInfo(C.Structure):
    """yolo2_hip_loop_info_t"""
    _fields_ = [("chunks", C.c_int), ("image_bytes_staged", C.c_uint64), ("image_bytes_h2d", C.c_uint64), ("out_bytes_d2h", C.c_uint64),
                ("items_built", C.c_uint64), ("items_kernel", C.c_char * 32)]

    def as_dict(self):
        return {"chunks": self.chunks, "image_bytes_staged": self.image_bytes_staged, "image_bytes_h2d": self.image_bytes_h2d,
                "out_bytes_d2h": self.out_bytes_d2h, "items_built": self.items_built, "items_kernel": self.items_kernel.decode()}


def loop_last_info(ctx_handle) -> dict:
    """yolo2_hip_loop_last_info: what the last loop call on this context moved and built"""
    info = LoopInfo()
    check(lib().yolo2_hip_loop_last_info(ctx_handle, C.byref(info)), "yolo2_hip_loop_last_info")
    return info.as_dict()


def loop_images_raw(handle, images, pixfmt, precision, flags, thresh, nms, batch, cap, labels, out_format, quality, caps, multi=False, guard=0):
    """The loop entries as they are: caps [n] bytes of room per frame -> (return code, dets [n][cap], counts, final_q, list of uint8
    [caps[f] + guard] buffers - with a guard, every byte of them 0xA5 before the call -, sizes [n], records drawn [n])."""
    imgs0 = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
    fmt = pixfmt if pixfmt is not None else ("grey8" if imgs0[0].ndim == 2 else "rgb24")
    n, ptrs, ws, hs, code, _imgs = _image_args(imgs0, fmt)
    dets = np.zeros((n, cap), dtype=DET_DTYPE)
    counts = np.zeros(n, dtype=np.int32)
    lab, n_labels, _keep = _label_args(labels)
    caps = np.ascontiguousarray(caps, dtype=np.uint64)
    outs = [np.full(int(caps[f]) + guard, 0xA5, dtype=np.uint8) if guard else np.empty(int(caps[f]), dtype=np.uint8) for f in range(n)]
    optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    sizes = np.zeros(n, dtype=np.uint64)
    drawn = np.zeros(n, dtype=np.int32)
    q = C.c_int(0)
    name = f"yolo2_hip_{'multi_' if multi else ''}loop_images_pix"
    rc = getattr(lib(), name)(handle, precision, ptrs, ws, hs, code, n, batch, thresh, nms, flags, dets.ctypes.data_as(C.c_void_p), cap,
                              counts.ctypes.data_as(C.c_void_p), C.byref(q), lab, n_labels, out_format, quality, optrs,
                              caps.ctypes.data_as(C.c_void_p), sizes.ctypes.data_as(C.c_void_p), drawn.ctypes.data_as(C.c_void_p))
    return rc, dets, counts, q.value, outs, sizes, drawn


def loop_images(handle, images, pixfmt=None, precision: str = "int16", tail: str = "core", thresh: float = 0.24, nms: float = 0.45,
                labels=None, jpeg_quality=None, batch: int = 64, cap: int = 845, multi: bool = False, out_order: str = "rgb"):
    """yolo2_hip_loop_images_pix / its multi form: the camera loop as one call - host images -> {"dets": per-frame record arrays (one
    per detection, best class), "counts", "final_q" (int16 only, else None), "frames": the annotated frames as uint8 [h][w][3] (or,
    with jpeg_quality 1..100, as JPEG byte strings), "drawn": records drawn per frame}.  The frames go up once; records, draw items
    and the painted frames are made on the device.  out_order "bgr": the raw frames come back as B G R (YOLO2_LOOP_OUT_BGR24, what
    cv2.imshow / cv2.VideoWriter take); "nv12" / "i420": as planar YUV 4:2:0, uint8 [h * 3 / 2][w], what video encoders take
    (YOLO2_LOOP_OUT_NV12 / _I420; even sizes only; rgb24_to_yuv420 of the "rgb" frame).  Each an error together with jpeg_quality."""
    if precision not in LOOP_PRECISIONS:
        raise ValueError(f"precision must be one of {tuple(LOOP_PRECISIONS)}, not {precision!r}")
    out_format = _loop_out_format(out_order, jpeg_quality)
    flags = DETS_BEST_CLASS | (DETS_APP_TAIL if _check_tail(tail) else 0)
    shapes = [_pix_hw(pixfmt, np.asarray(im).shape) for im in images]
    jpeg = jpeg_quality is not None
    if jpeg:
        caps = [min(jpeg_bound(s[1], s[0]), s[0] * s[1] * 3 + 4096) for s in shapes]
    else:
        caps = [_loop_raw_bytes(out_order, s) for s in shapes]
    name = f"yolo2_hip_{'multi_' if multi else ''}loop_images_pix"
    for attempt in range(2):
        rc, dets, counts, q, outs, sizes, drawn = loop_images_raw(handle, images, pixfmt, LOOP_PRECISIONS[precision], flags, thresh, nms, batch, cap,
                                                                  labels, out_format, int(jpeg_quality) if jpeg else 0, caps, multi=multi)
        if rc == YOLO2_SUCCESS or attempt or not jpeg or not any(int(sizes[f]) > caps[f] for f in range(len(caps))):
            break
        caps = [jpeg_bound(s[1], s[0]) for s in shapes]   # (the rare frame that compresses to more than its raw size)
    check(rc, name)
    if jpeg:
        frames = [outs[f][:int(sizes[f])].tobytes() for f in range(len(outs))]
    else:
        frames = [outs[f].reshape(_loop_raw_shape(out_order, shapes[f])) for f in range(len(outs))]
    return {"dets": [dets[f, :min(int(counts[f]), cap)] for f in range(len(outs))], "counts": counts,
            "final_q": q if precision == "int16" else None, "frames": frames, "drawn": drawn}


def _loop_out_format(out_order, jpeg_quality) -> int:
    """the loop entries' out_format for out_order "rgb" / "bgr" / "nv12" / "i420" and an optional JPEG quality"""
    if out_order not in _LOOP_OUT_ORDERS:
        raise ValueError(f"out_order must be one of {tuple(_LOOP_OUT_ORDERS)}, not {out_order!r}")
    if out_order != "rgb" and jpeg_quality is not None:
        raise ValueError(f"out_order {out_order!r} is a raw frame's layout: it cannot be combined with jpeg_quality")
    return LOOP_OUT_JPEG if jpeg_quality is not None else _LOOP_OUT_ORDERS[out_order]


_LOOP_OUT_ORDERS = {"rgb": LOOP_OUT_RGB24, "bgr": LOOP_OUT_BGR24, "nv12": LOOP_OUT_NV12, "i420": LOOP_OUT_I420}


def _loop_raw_bytes(out_order, hw) -> int:
    """bytes of a raw annotated frame of hw = (h, w)"""
    return hw[0] * hw[1] * 3 // 2 if out_order in ("nv12", "i420") else hw[0] * hw[1] * 3


def _loop_raw_shape(out_order, hw):
    """... and the shape it comes back in (an odd-sized 4:2:0 frame does not exist: the library refuses it)"""
    return (hw[0] * 3 // 2, hw[1]) if out_order in ("nv12", "i420") else (hw[0], hw[1], 3)


def loop_jpegs_raw(handle, streams, precision, flags, thresh, nms, batch, cap, labels, out_format, quality, caps, multi=False, guard=0):
    """The loop entries from JPEG streams as they are: caps [n] bytes of room per frame -> (return code, dets [n][cap], counts,
    final_q, list of uint8 [caps[f] + guard] buffers, sizes [n], records drawn [n], status [n], widths, heights).  With a guard every
    output is a canary before the call: the buffers' and the records' bytes 0xA5, counts / drawn / status / widths / heights of the
    streams -77, sizes 2^40 + 7."""
    n, ptrs, ssizes, ws, hs, _keep = _mixed_stream_args(streams)
    dets = np.zeros((n, cap), dtype=DET_DTYPE)
    counts, drawn, status = (np.full(n, -77 if guard else 0, dtype=np.int32) for _ in range(3))
    sizes = np.full(n, (1 << 40) + 7 if guard else 0, dtype=np.uint64)
    if guard:
        dets.view(np.uint8)[...] = 0xA5
        for i in range(n):
            if ssizes[i]:
                ws[i] = hs[i] = -77
    lab, n_labels, _keepl = _label_args(labels)
    caps = np.ascontiguousarray(caps, dtype=np.uint64)
    outs = [np.full(int(caps[f]) + guard, 0xA5, dtype=np.uint8) if guard else np.empty(int(caps[f]), dtype=np.uint8) for f in range(n)]
    optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    q = C.c_int(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    name = f"yolo2_hip_{'multi_' if multi else ''}loop_images_jpeg"
    rc = getattr(lib(), name)(handle, precision, ptrs, ssizes, vp(ws), vp(hs), n, batch, thresh, nms, flags, vp(dets), cap, vp(counts), C.byref(q),
                              lab, n_labels, out_format, quality, optrs, vp(caps), vp(sizes), vp(drawn), vp(status))
    return rc, dets, counts, q.value, outs, sizes, drawn, status, ws, hs


def loop_jpegs(handle, streams, precision: str = "int16", tail: str = "core", thresh: float = 0.24, nms: float = 0.45, labels=None,
               jpeg_quality=None, batch: int = 64, cap: int = 845, multi: bool = False, strict: bool = True, out_order: str = "rgb"):
    """yolo2_hip_loop_images_jpeg / its multi form: the camera loop as one call from JPEG streams (bytes) - or, mixed in, raw frames
    (uint8 [h][w][3] arrays, e.g. decoded on the host) - with the decoder, the network, the painter and the encoder on the device.
    Returns loop_images' dictionary plus "status" (int32 [n]; not 0: the decoder flagged the frame, its counts and drawn are 0 and
    its frame is None) and "sizes" ([n] (w, h)).  A flagged frame raises under strict.  out_order: as loop_images'."""
    if precision not in LOOP_PRECISIONS:
        raise ValueError(f"precision must be one of {tuple(LOOP_PRECISIONS)}, not {precision!r} (the loop entries have no int8 form)")
    out_format = _loop_out_format(out_order, jpeg_quality)
    flags = DETS_BEST_CLASS | (DETS_APP_TAIL if _check_tail(tail) else 0)
    shapes = []
    for i, s in enumerate(streams):
        if isinstance(s, np.ndarray):
            shapes.append((s.shape[0], s.shape[1]))
        else:
            info = jpeg_probe(s)
            shapes.append((max(info["height"], 0), max(info["width"], 0)))
    jpeg = jpeg_quality is not None
    if jpeg:
        caps = [min(jpeg_bound(s[1], s[0]), s[0] * s[1] * 3 + 4096) if s[0] and s[1] else 0 for s in shapes]
    else:
        caps = [_loop_raw_bytes(out_order, s) for s in shapes]
    name = f"yolo2_hip_{'multi_' if multi else ''}loop_images_jpeg"
    for attempt in range(2):
        rc, dets, counts, q, outs, sizes, drawn, status, ws, hs = loop_jpegs_raw(handle, streams, LOOP_PRECISIONS[precision], flags, thresh, nms, batch,
                                                                                 cap, labels, out_format, int(jpeg_quality) if jpeg else 0, caps,
                                                                                 multi=multi)
        if rc == YOLO2_SUCCESS or attempt or not jpeg or not any(int(sizes[f]) > caps[f] for f in range(len(caps))):
            break
        caps = [jpeg_bound(s[1], s[0]) for s in shapes]   # (the rare frame that compresses to more than its raw size)
    if rc != YOLO2_SUCCESS and (strict or not status.any()):
        check(rc, name)
    n = len(outs)
    if jpeg:
        frames = [None if status[f] else outs[f][:int(sizes[f])].tobytes() for f in range(n)]
    else:
        frames = [None if status[f] else outs[f].reshape(_loop_raw_shape(out_order, shapes[f])) for f in range(n)]
    return {"dets": [dets[f, :min(int(counts[f]), cap)] for f in range(n)], "counts": counts, "final_q": q if precision == "int16" else None,
            "frames": frames, "drawn": drawn, "status": status, "sizes": [(int(ws[i]), int(hs[i])) for i in range(n)]}


def draw_items_dev(ctx_handle, dets, counts, widths, heights, thresh: float, labels=None):
    """yolo2_hip_draw_items_dev, the test doorway to k_draw_items: dets DET_DTYPE [n][cap] and counts [n] are uploaded, the kernel makes
    the draw items -> (return code, items uint8 [n][cap][item size], n_items [n], unprintable [n])."""
    L = lib()
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE)
    n, cap = d.shape
    cnt = np.ascontiguousarray(counts, dtype=np.int32)
    ws = np.ascontiguousarray(widths, dtype=np.int32)
    hs = np.ascontiguousarray(heights, dtype=np.int32)
    isz = int(L.yolo2_hip_draw_item_size())
    items = np.zeros((n, cap, isz), dtype=np.uint8)
    n_items = np.zeros(n, dtype=np.int32)
    bad = np.zeros(n, dtype=np.int32)
    lab, n_labels, _keep = _label_args(labels)
    dd, dc = DevBuf(d.view(np.uint8).reshape(-1)), DevBuf(cnt)
    try:
        rc = L.yolo2_hip_draw_items_dev(ctx_handle, dd.addr, dc.addr, n, cap, ws.ctypes.data_as(C.c_void_p), hs.ctypes.data_as(C.c_void_p), thresh, lab,
                                        n_labels, items.ctypes.data_as(C.c_void_p), n_items.ctypes.data_as(C.c_void_p), bad.ctypes.data_as(C.c_void_p))
    finally:
        dd.free()
        dc.free()
    return rc, items, n_items, bad


# ------------------------------------------------------------------ more than one GPU

def shard_range(total: int, rank: int, world: int):
    lo, hi = C.c_int(0), C.c_int(0)
    check(lib().yolo2_hip_shard_range(total, rank, world, C.byref(lo), C.byref(hi)), "yolo2_hip_shard_range")
    return lo.value, hi.value


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId (rank 0): 128 bytes the launcher hands to every rank."""
    buf = (C.c_char * 128)()
    check(lib().yolo2_hip_rccl_unique_id(buf), "yolo2_hip_rccl_unique_id")
    return bytes(buf)


class RcclInfo(C.Structure):
    """yolo2_hip_rccl_info_t"""
    _fields_ = [("nranks", C.c_int), ("rank", C.c_int), ("device", C.c_int), ("version", C.c_int), ("bcasts", C.c_int),
                ("last_bcast_ms", C.c_double), ("last_bcast_bytes", C.c_uint64), ("lib_path", C.c_char * 256)]

    def as_dict(self):
        v = self.version
        return {"nranks": self.nranks, "rank": self.rank, "device": self.device, "version": v,
                "version_str": f"{v // 10000}.{v // 100 % 100}.{v % 100}" if v >= 10000 else str(v),
                "bcasts": self.bcasts, "bcast_ms": self.last_bcast_ms, "bytes": int(self.last_bcast_bytes),
                "lib_path": self.lib_path.decode()}


class _BcastMixin:
    def rccl_init_rank(self, id128: bytes, nranks: int, rank: int):
        assert len(id128) == 128
        check(lib().yolo2_hip_rccl_init_rank(self._h, self.device, C.c_char_p(id128), nranks, rank), "yolo2_hip_rccl_init_rank")
        self._in_comm = True

    def rccl_info(self) -> dict:
        """What the library's communicator reports about itself (yolo2_hip_rccl_info)."""
        info = RcclInfo()
        check(lib().yolo2_hip_rccl_info(self._h, C.byref(info)), "yolo2_hip_rccl_info")
        return info.as_dict()

    def fp16_layer_kernels(self):
        """Kernel name per layer of the fp16 launch table (after the first run at the current batch)."""
        return {i: lib().yolo2_hip_fp16_layer_kernel(self._h, i).decode() for i in range(32) if lib().yolo2_hip_fp16_layer_kernel(self._h, i)}

    def rccl_finalize(self):
        if getattr(self, "_in_comm", False):
            lib().yolo2_hip_rccl_finalize(self._h)
            self._in_comm = False

    def load_model_bcast(self, model, root: int = 0):
        """All ranks call this; `model` is the SynthModel on the root rank and None elsewhere.  One ncclBroadcast per blob
        (the library's own RCCL communicator), then every rank loads its device copy."""
        if model is not None:
            w = np.ascontiguousarray(model.weights_i16(), dtype=np.int16)
            b = np.ascontiguousarray(model.bias_i16(), dtype=np.int16)
            wq, bq, aq = (np.ascontiguousarray(a, dtype=np.int32) for a in (model.weight_q, model.bias_q, model.act_q))
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            rc = lib().yolo2_hip_load_weights_int16_bcast(self._h, vp(w), w.size, vp(b), b.size, vp(wq), wq.size, vp(bq), bq.size,
                                                          vp(aq), aq.size, root)
        else:
            rc = lib().yolo2_hip_load_weights_int16_bcast(self._h, None, 0, None, 0, None, 0, None, 0, None, 0, root)
        check(rc, "yolo2_hip_load_weights_int16_bcast")

    def load_model_fp32_bcast(self, model, root: int = 0):
        if model is not None:
            w = np.ascontiguousarray(model.weights_f32(), dtype=np.float32)
            b = np.ascontiguousarray(model.bias_f32(), dtype=np.float32)
            rc = lib().yolo2_hip_load_weights_fp32_bcast(self._h, w.ctypes.data_as(C.c_void_p), w.size, b.ctypes.data_as(C.c_void_p),
                                                         b.size, root)
        else:
            rc = lib().yolo2_hip_load_weights_fp32_bcast(self._h, None, 0, None, 0, root)
        check(rc, "yolo2_hip_load_weights_fp32_bcast")


for _name, _fn in list(vars(_BcastMixin).items()):
    if not _name.startswith("__"):
        setattr(Yolo2Hip, _name, _fn)


class Yolo2HipMulti:
    """One process, several devices (yolo2_hip_multi): contiguous frame shards, weights broadcast once."""

    def __init__(self, devices):
        devs = (C.c_int * len(devices))(*devices)
        self._m = C.c_void_p(0)
        check(lib().yolo2_hip_multi_create(devs, len(devices), C.byref(self._m)), "yolo2_hip_multi_create")
        self.devices = list(devices)

    def close(self):
        if self._m:
            lib().yolo2_hip_multi_destroy(self._m)
            self._m = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def uses_rccl(self) -> bool:
        return bool(lib().yolo2_hip_multi_uses_rccl(self._m))

    def load_model(self, model):
        w = np.ascontiguousarray(model.weights_i16(), dtype=np.int16)
        b = np.ascontiguousarray(model.bias_i16(), dtype=np.int16)
        wq, bq, aq = (np.ascontiguousarray(a, dtype=np.int32) for a in (model.weight_q, model.bias_q, model.act_q))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib().yolo2_hip_multi_load_weights_int16(self._m, vp(w), w.size, vp(b), b.size, vp(wq), wq.size, vp(bq), bq.size,
                                                       vp(aq), aq.size), "yolo2_hip_multi_load_weights_int16")

    def load_model_fp32(self, model):
        """fp32 weights on every device (the fp16 / split-fp16 passes)"""
        w = np.ascontiguousarray(model.weights_f32(), dtype=np.float32)
        b = np.ascontiguousarray(model.bias_f32(), dtype=np.float32)
        check(lib().yolo2_hip_multi_load_weights_fp32(self._m, w.ctypes.data_as(C.c_void_p), w.size, b.ctypes.data_as(C.c_void_p), b.size),
              "yolo2_hip_multi_load_weights_fp32")

    def run_frames(self, frames: np.ndarray, batch_per_device: int):
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n = frames.shape[0]
        region = np.empty((n, 425, 13, 13), dtype=np.int16)
        q = C.c_int(0)
        check(lib().yolo2_hip_multi_run_frames_int16(self._m, frames.ctypes.data_as(C.c_void_p), n, batch_per_device,
                                                     region.ctypes.data_as(C.c_void_p), C.byref(q)), "yolo2_hip_multi_run_frames_int16")
        return region, q.value

    def run_images(self, images, batch_per_device: int, pixfmt=None):
        n, ptrs, ws, hs, fmt, _keep = _image_args(images, pixfmt)
        region = np.empty((n, 425, 13, 13), dtype=np.int16)
        q = C.c_int(0)
        fn = lib().yolo2_hip_multi_run_images_u8_host if pixfmt is None else lib().yolo2_hip_multi_run_images_pix_host
        check(fn(self._m, ptrs, ws, hs, fmt, n, batch_per_device, region.ctypes.data_as(C.c_void_p), C.byref(q)),
              "yolo2_hip_multi_run_images_u8_host" if pixfmt is None else "yolo2_hip_multi_run_images_pix_host")
        return region, q.value

    def annotate_images(self, images, dets, counts, batch_per_device: int, thresh: float, labels=None, pixfmt=None, jpeg_quality=None):
        """annotated frames, shard i painted by device i (module-level annotate_images)"""
        return annotate_images(self._m, images, dets, counts, batch_per_device, thresh, labels=labels, pixfmt=pixfmt, multi=True,
                               jpeg_quality=jpeg_quality)

    def loop_images(self, images, batch_per_device: int = 64, **kw):
        """the camera loop as one call, shard i on device i (module-level loop_images)"""
        return loop_images(self._m, images, batch=batch_per_device, multi=True, **kw)

    def loop_jpegs(self, streams, batch_per_device: int = 64, **kw):
        """the camera loop as one call from JPEG streams, shard i on device i (module-level loop_jpegs)"""
        return loop_jpegs(self._m, streams, batch=batch_per_device, multi=True, **kw)

    def run_jpegs_dets(self, streams, batch_per_device: int = 64, thresh: float = 0.24, nms: float = 0.45, **kw):
        """JPEG streams -> records, shard i decoded and run by device i (module-level run_jpegs_dets)"""
        return run_jpegs_dets(self._m, streams, batch_per_device, thresh, nms, multi=True, **kw)
