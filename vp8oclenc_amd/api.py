"""ctypes binding of libvp8hip.so: the C ABI of include/vp8hip.h and include/vp8hip_host.h.

Python is plumbing here (tests, bench, multi-GPU launch); every computation of the hot path
happens behind the C ABI in hand-written HIP.  There is NO fallback: if the library is missing
or no gfx950 device is usable, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

K_NAMES = ["pack", "downsample", "search1_l4", "search1_l3", "search1_l2", "search1_l1", "search1_l0", "search2",
           "select", "mb", "filter_mask", "loop_filter", "border", "ent_count", "ent_encode", "intra", "hdr_encode"]
K_COUNT = len(K_NAMES)

DBG_NET1, DBG_NET2, DBG_BDIFF, DBG_PYRAMID, DBG_MB_MASK, DBG_MB_NZ, DBG_THIRD_CONTEXT, DBG_CURRENT_CHROMA, DBG_ARF_FRAME, DBG_REFRESH_FRAME = range(10)

# every symbol include/vp8hip.h and include/vp8hip_host.h declare
ABI_SYMBOLS = [
    "vp8hip_hw_queues", "vp8hip_profile_read_clock", "vp8hip_inter_search", "vp8hip_inter_finish", "vp8hip_export_search",
    "vp8hip_import_search", "vp8hip_export_last", "vp8hip_import_last", "vp8hip_group_rendezvous", "vp8hip_group_create", "vp8hip_group_destroy", "vp8hip_group_rank", "vp8hip_group_world", "vp8hip_group_count", "vp8hip_group_barrier", "vp8hip_group_max", "vp8hip_group_all_gather", "vp8hip_group_broadcast", "vp8hip_group_gather_bytes", "vp8hip_group_last_hip_error", "vp8hip_batch_create", "vp8hip_batch_destroy", "vp8hip_batch_lane", "vp8drv_batch_lane", "vp8hip_batch_set_current_device",
    "vp8hip_batch_auto_segments", "vp8hip_batch_inter_transform", "vp8hip_batch_loop_filter", "vp8drv_batch_create", "vp8drv_batch_destroy",
    "vp8drv_batch_encode_frame_device", "vp8hip_batch_encode_frame_begin", "vp8drv_batch_get_frame_begin", "vp8hip_profile_context_switches", "vp8hip_profile_read_search2_clock", "vp8hip_profile_search2_clock",
    "vp8hip_create", "vp8hip_destroy", "vp8hip_upload_current", "vp8hip_set_current_device", "vp8hip_upload_last",
    "vp8hip_set_last_device", "vp8hip_set_segments", "vp8hip_inter_transform", "vp8hip_download_results",
    "vp8hip_upload_mb_data", "vp8hip_upload_recon", "vp8hip_prepare_filter_mask", "vp8hip_loop_filter", "vp8hip_set_loop_filter_type",
    "vp8hip_set_quality_stats", "vp8hip_quality_result", "vp8hip_quality_summary", "vp8hip_batch_quality", "vp8drv_get_frame_quality", "vp8drv_get_quality_summary", "vp8hip_debug_quality", "vp8hip_debug_bool_code",
    "vp8hip_download_last", "vp8hip_synchronize", "vp8hip_stream", "vp8hip_last_hip_error", "vp8hip_status_string",
    "vp8hip_profile_enable", "vp8hip_profile_read", "vp8hip_debug_download", "vp8hip_count_probs", "vp8hip_encode_coefficients", "vp8hip_loopfilter_strength", "vp8hip_chroma_change", "vp8hip_chroma_change_async", "vp8hip_chroma_change_result", "vp8hip_auto_segments", "vp8hip_get_segments",
    "vp8hip_intra_transform", "vp8hip_check_ssim", "vp8hip_download_intra", "vp8hip_conformant_stream", "vp8hip_set_source_size", "vp8hip_set_source_scaling", "vp8host_scale_taps", "vp8hip_set_denoise", "vp8hip_denoise_restart", "vp8hip_denoise_result", "vp8host_denoise_frame", "vp8drv_set_denoise", "vp8drv_get_denoise_stats", "vp8hip_set_deinterlace", "vp8hip_deinterlace_restart", "vp8hip_deinterlace_result", "vp8host_deinterlace_frame", "vp8host_y4m_interlace", "vp8drv_set_deinterlace", "vp8drv_get_deinterlace_stats", "vp8hip_set_analysis", "vp8hip_analysis_restart", "vp8hip_analysis_result", "vp8host_analyse_luma", "vp8drv_set_analysis", "vp8drv_get_frame_analysis", "vp8drv_set_quantizer", "vp8drv_get_quantizer", "vp8hip_set_segment_mode", "vp8hip_segment_mode", "vp8hip_set_segment_map_device", "vp8hip_upload_segment_map", "vp8hip_download_segment_map", "vp8host_aq_segment_map", "vp8host_aq_segment", "vp8drv_set_segment_mode", "vp8drv_set_segment_map", "vp8hip_set_source_format", "vp8drv_set_source_format", "vp8host_source_plane_bytes", "vp8host_convert_frame", "vp8host_y4m_colourspace", "vp8hip_set_source_colour", "vp8drv_set_source_colour", "vp8host_convert_frame_colour", "vp8host_colour_coefficients", "vp8hip_set_source_window", "vp8hip_set_source_orientation", "vp8host_source_window", "vp8host_window_frame", "vp8host_orient_frame", "vp8drv_set_source_window", "vp8drv_set_source_orientation", "vp8hip_abi_version", "vp8hip_experiments_compiled_in", "vp8hip_batch_prep_mode", "vp8hip_device_count", "vp8hip_device_alloc", "vp8hip_device_free", "vp8hip_device_upload", "vp8hip_device_download", "vp8hip_device_synchronize", "vp8hip_device_mem_info", "vp8hip_device_pci_bus_id", "vp8hip_runtime_version", "vp8hip_shard_unique_id", "vp8hip_shard_init", "vp8hip_shard_rank", "vp8hip_shard_world", "vp8hip_shard_share_search", "vp8hip_shard_share_last", "vp8hip_shard_max", "vp8hip_encode_header", "vp8hip_encode_frame",
    "vp8hip_encode_frame_begin", "vp8hip_encode_frame_end", "vp8hip_filter_overlap",
    "vp8host_quantizer_ladders", "vp8host_loopfilter_strength", "vp8host_prepare_segments_data", "vp8host_skip_prob",
    "vp8host_gop_init", "vp8host_gop_next", "vp8host_gop_key_coded", "vp8host_gop_inter_flags",
    "vp8host_gop_frame_done", "vp8host_scene_change", "vp8host_scene_plan", "vp8hip_batch_chroma_change_async",
    "vp8drv_batch_scan_frame_device", "vp8drv_batch_scan_frame_host", "vp8drv_batch_scan_result", "vp8host_y4m_parse_header", "vp8host_y4m_frame_marker_ok",
    "vp8drv_default_config", "vp8drv_create", "vp8drv_destroy", "vp8drv_context", "vp8drv_encode_frame_device",
    "vp8drv_encode_frame_host", "vp8drv_get_stats", "vp8hip_reserve_frame_path", "vp8hip_reserve_frame_path_dense", "vp8drv_resolve", "vp8drv_ready", "vp8drv_batch_ready", "vp8drv_batches_encode_frame_device", "vp8drv_batches_encode_frames_device", "vp8drv_batches_encode_frames_host", "vp8drv_batch_encode_frame_host", "vp8hip_batch_upload_current", "vp8hip_batch_intra_transform", "vp8hip_batch_prefetch_current", "vp8hip_prefetch_current", "vp8drv_prefetch_frame_host", "vp8drv_stage_frame_host", "vp8drv_batch_prefetch_frame_host", "vp8hip_host_alloc", "vp8hip_host_free", "vp8drv_frame_check", "vp8drv_encode_video_device", "vp8hip_check_ssim_ready", "vp8hip_check_ssim_async", "vp8hip_check_ssim_result", "vp8hip_batch_check_ssim_async", "vp8drv_get_frame", "vp8drv_get_frame_begin", "vp8drv_get_frame_end",
    "vp8bs_default_probs", "vp8bs_encode_header", "vp8bs_gather_frame", "vp8bs_ivf_file_header", "vp8bs_ivf_frame_header",
    "vp8hip_arf_filter_device", "vp8hip_arf_filter_host", "vp8hip_arf_result", "vp8hip_arf_release", "vp8hip_loop_filter_hidden",
    "vp8host_arf_filter_frame", "vp8host_arf_round_divide", "vp8drv_set_arf", "vp8drv_encode_arf_device", "vp8drv_encode_arf_host",
    "vp8drv_get_arf_stats",
    "vp8hip_set_source_transfer", "vp8drv_set_source_transfer", "vp8host_tonemap_tables", "vp8host_tonemap_frame",
    "vp8hip_set_overlay_host", "vp8hip_set_overlay_device", "vp8hip_set_overlay_placement", "vp8hip_clear_overlay", "vp8hip_overlay_count",
    "vp8host_overlay_frame", "vp8drv_set_overlay_host", "vp8drv_set_overlay_device", "vp8drv_set_overlay_placement", "vp8drv_clear_overlay",
    "vp8hip_set_canvas", "vp8hip_canvas_tiles", "vp8hip_compose_current_device", "vp8hip_compose_current_host", "vp8host_tile_valid",
    "vp8host_compose_frame", "vp8drv_set_canvas", "vp8drv_encode_frame_tiles_device", "vp8drv_encode_frame_tiles_host",
    "vp8host_temporal_step", "vp8hip_loop_filter_refresh", "vp8drv_set_temporal_layers", "vp8drv_get_frame_layer",
    "vp8host_intra_refresh_forced", "vp8host_intra_refresh_count", "vp8hip_intra_refresh", "vp8drv_set_intra_refresh", "vp8drv_get_intra_refresh",
]


class Vp8HipError(RuntimeError):
    pass


ABI_VERSION = 4010  # VP8HIP_ABI_VERSION, include/vp8hip.h
ALTREF_HIDDEN = 2   # VP8HIP_ALTREF_HIDDEN: is_altref of a hidden alternate reference frame (header params, bitstream.Frame)
ARF_MAX_FRAMES = 7  # VP8HOST_ARF_MAX_FRAMES, include/vp8hip_host.h
REFRESH_LAST, REFRESH_GOLDEN, REFRESH_NONE, REFRESH_ALL = range(4)   # VP8HOST_REFRESH_* (the first three also VP8HIP_REFRESH_*)
GOLDEN_ONLY, REFRESH_NOTHING = 2, 3   # VP8HIP_GOLDEN_ONLY / VP8HIP_REFRESH_NOTHING: is_golden of a temporal layer's inter frame (header params, bitstream.Frame)
TL_KEEP_RECON = 1   # VP8DRV_TL_KEEP_RECON, include/vp8hip_driver.h
INTRA_REFRESH_MIN, INTRA_REFRESH_MAX = 4, 1024   # VP8HOST_INTRA_REFRESH_MIN / _MAX, include/vp8hip_host.h
ERR_OVERFLOW = -7   # VP8HIP_ERR_OVERFLOW, include/vp8hip.h
ERR_FORMAT = -8     # VP8HIP_ERR_FORMAT
SHARPNESS_ON_DEVICE = -2 ** 31   # VP8HIP_SHARPNESS_ON_DEVICE


class _Results(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("MB_parts", "MB_reference_frame", "MB_vectors", "MB_coeffs",
                                          "MB_segment_id", "MB_SSIM", "recon_Y", "recon_U", "recon_V")]


class GopState(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "gop_size", "altref_range", "frame_number", "frames_until_key", "frames_until_altref",
        "golden_frame_number", "altref_frame_number", "current_is_key", "current_is_golden", "current_is_altref",
        "prev_is_key", "prev_is_golden", "prev_is_altref")]


_lib = None


def load_library(path: str | None = None) -> C.CDLL:
    """dlopen libvp8hip.so (building it first if the sources are newer).  Raises if impossible."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or _build.LIB
    if path is None and _build.stale():
        try:
            _build.build()
        except Exception as e:  # no hipcc on this box: use the prebuilt file if there is one
            if not os.path.exists(p):
                raise Vp8HipError(f"libvp8hip.so is missing and cannot be built: {e}") from e
    if not os.path.exists(p):
        raise Vp8HipError(f"{p} not found: build it with `python -m vp8oclenc_amd.build`")
    lib = C.CDLL(p)
    # the struct layouts below (DrvConfig, DrvStats, ...) belong to one ABI: a library built from other sources is refused
    if not hasattr(lib, "vp8hip_abi_version") or lib.vp8hip_abi_version() != ABI_VERSION:
        raise Vp8HipError(f"{p} is not ABI {ABI_VERSION} (include/vp8hip.h): rebuild it with `python -m vp8oclenc_amd.build`")
    u8 = C.c_void_p
    vp = C.c_void_p
    lib.vp8hip_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_float, C.c_int]
    lib.vp8hip_destroy.argtypes = [vp]
    lib.vp8hip_destroy.restype = None
    for n in ("vp8hip_upload_current", "vp8hip_set_current_device", "vp8hip_upload_last", "vp8hip_set_last_device",
              "vp8hip_upload_recon", "vp8hip_download_last"):
        getattr(lib, n).argtypes = [vp, u8, u8, u8]
    lib.vp8hip_set_segments.argtypes = [vp, C.c_void_p]
    lib.vp8hip_inter_transform.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.vp8hip_download_results.argtypes = [vp, C.POINTER(_Results)]
    lib.vp8hip_upload_mb_data.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp8hip_prepare_filter_mask.argtypes = [vp, C.c_void_p]
    lib.vp8hip_loop_filter.argtypes = [vp]
    lib.vp8hip_synchronize.argtypes = [vp]
    lib.vp8hip_stream.argtypes = [vp]
    lib.vp8hip_stream.restype = C.c_void_p
    lib.vp8hip_last_hip_error.argtypes = [vp]
    lib.vp8hip_status_string.argtypes = [C.c_int]
    lib.vp8hip_status_string.restype = C.c_char_p
    lib.vp8hip_profile_enable.argtypes = [vp, C.c_uint32]
    lib.vp8hip_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.vp8hip_debug_download.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.vp8hip_count_probs.argtypes = [vp, C.c_int, C.c_void_p, C.c_void_p]
    lib.vp8hip_loopfilter_strength.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.vp8hip_chroma_change.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.vp8hip_auto_segments.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), C.c_int]
    lib.vp8hip_get_segments.argtypes = [vp, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.vp8hip_encode_coefficients.argtypes = [vp, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.vp8hip_intra_transform.argtypes = [vp]
    lib.vp8hip_check_ssim.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.vp8hip_download_intra.argtypes = [vp, C.c_void_p, C.c_void_p]
    i32p = C.POINTER(C.c_int32)
    lib.vp8host_quantizer_ladders.argtypes = [C.c_int, C.c_int, i32p, i32p]
    lib.vp8host_quantizer_ladders.restype = None
    lib.vp8host_loopfilter_strength.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, i32p]
    lib.vp8host_loopfilter_strength.restype = None
    lib.vp8host_prepare_segments_data.argtypes = [C.c_int, i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32p]
    lib.vp8host_prepare_segments_data.restype = None
    lib.vp8host_skip_prob.argtypes = [C.c_void_p, C.c_int]
    for n in ("vp8host_gop_next", "vp8host_gop_key_coded", "vp8host_gop_frame_done"):
        getattr(lib, n).argtypes = [C.POINTER(GopState)]
        getattr(lib, n).restype = None
    lib.vp8host_gop_init.argtypes = [C.POINTER(GopState), C.c_int, C.c_int]
    lib.vp8host_gop_init.restype = None
    lib.vp8host_gop_inter_flags.argtypes = [C.POINTER(GopState), i32p, i32p]
    lib.vp8host_gop_inter_flags.restype = None
    lib.vp8hip_device_alloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.vp8hip_device_free.argtypes = [C.c_int, C.c_void_p]
    lib.vp8hip_device_upload.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.vp8hip_device_download.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.vp8hip_device_synchronize.argtypes = [C.c_int]
    lib.vp8hip_device_mem_info.argtypes = [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.vp8hip_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]
    if path is None:
        _lib = lib
    return lib


class DeviceBuffer:
    """Device memory from the library's own runtime (vp8hip_device_alloc): what a host without a GPU framework of its own
    hands to vp8hip_set_current_device & co.  `data_ptr()` like a torch tensor, so call sites read the same."""

    def __init__(self, nbytes: int, device: int = 0):
        self.lib, self.device, self.nbytes = load_library(), device, int(nbytes)
        p = C.c_void_p()
        rc = self.lib.vp8hip_device_alloc(device, self.nbytes, C.byref(p))
        if rc != 0:
            raise Vp8HipError(f"vp8hip_device_alloc({self.nbytes}): {self.lib.vp8hip_status_string(rc).decode()}")
        self.ptr = p.value

    def data_ptr(self) -> int:
        return self.ptr

    def upload(self, a: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        rc = self.lib.vp8hip_device_upload(self.device, self.ptr + offset, a.ctypes.data, a.nbytes)
        if rc != 0:
            raise Vp8HipError(f"vp8hip_device_upload: {self.lib.vp8hip_status_string(rc).decode()}")
        return self

    def download(self, dtype=np.uint8, shape=None) -> np.ndarray:
        out = np.empty(self.nbytes, np.uint8)
        rc = self.lib.vp8hip_device_download(self.device, out.ctypes.data, self.ptr, self.nbytes)
        if rc != 0:
            raise Vp8HipError(f"vp8hip_device_download: {self.lib.vp8hip_status_string(rc).decode()}")
        out = out.view(dtype)
        return out.reshape(shape) if shape is not None else out

    def free(self):
        if getattr(self, "ptr", None):
            self.lib.vp8hip_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HostBuffer:
    """Page-locked host memory (vp8hip_host_alloc): planes handed to vp8hip_batch_upload_current from it are copied asynchronously."""

    def __init__(self, a: np.ndarray, device: int = 0):
        a = np.ascontiguousarray(a)
        self.lib, self.device, self.nbytes = load_library(), device, int(a.nbytes)
        p = C.c_void_p()
        self.lib.vp8hip_host_alloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
        self.lib.vp8hip_host_free.argtypes = [C.c_int, C.c_void_p]
        rc = self.lib.vp8hip_host_alloc(device, self.nbytes, C.byref(p))
        if rc != 0:
            raise Vp8HipError(f"vp8hip_host_alloc({self.nbytes}): {self.lib.vp8hip_status_string(rc).decode()}")
        self.ptr = p.value
        C.memmove(self.ptr, a.ctypes.data, self.nbytes)

    def data_ptr(self) -> int:
        return self.ptr

    def free(self):
        if getattr(self, "ptr", None):
            self.lib.vp8hip_host_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def to_device(a: np.ndarray, device: int = 0) -> DeviceBuffer:
    """a copy of the array in the device's memory (blocking)"""
    a = np.ascontiguousarray(a)
    return DeviceBuffer(a.nbytes, device).upload(a)


def device_synchronize(device: int = 0) -> None:
    rc = load_library().vp8hip_device_synchronize(device)
    if rc != 0:
        raise Vp8HipError(f"vp8hip_device_synchronize: {load_library().vp8hip_status_string(rc).decode()}")


def device_count() -> int:
    return int(load_library().vp8hip_device_count())


def device_mem_info(device: int = 0):
    f, t = C.c_size_t(), C.c_size_t()
    rc = load_library().vp8hip_device_mem_info(device, C.byref(f), C.byref(t))
    if rc != 0:
        raise Vp8HipError("vp8hip_device_mem_info failed")
    return int(f.value), int(t.value)


def device_pci_bus_id(device: int = 0) -> str:
    buf = C.create_string_buffer(32)
    rc = load_library().vp8hip_device_pci_bus_id(device, buf, 32)
    if rc != 0:
        raise Vp8HipError("vp8hip_device_pci_bus_id failed")
    return buf.value.decode().lower()


SHARD_ID_BYTES = 128     # VP8HIP_SHARD_ID_BYTES


class Group:
    """vp8hip_group_* (include/vp8hip.h): the process group of a GOP-sharded run -- one process per GPU, RCCL inside the library,
    no GPU framework in the host.  Every method is collective and blocks.

    Group.from_env(device): rank / world from RANK / WORLD_SIZE (torchrun's and bench.py's own launcher's variables), the id through a
    file named by `key` (vp8hip_group_rendezvous)."""

    def __init__(self, device: int, unique_id: bytes, rank: int, world: int, key: str | None = None):
        self.lib = load_library()
        L = self.lib
        vp = C.c_void_p
        L.vp8hip_group_create.argtypes = [C.POINTER(vp), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p]
        L.vp8hip_group_destroy.argtypes = [vp]
        L.vp8hip_group_destroy.restype = None
        for n in ("vp8hip_group_rank", "vp8hip_group_world", "vp8hip_group_count", "vp8hip_group_barrier", "vp8hip_group_last_hip_error"):
            getattr(L, n).argtypes = [vp]
        L.vp8hip_group_max.argtypes = [vp, C.POINTER(C.c_double)]
        L.vp8hip_group_all_gather.argtypes = [vp, C.c_void_p, C.c_size_t, C.c_void_p]
        L.vp8hip_group_broadcast.argtypes = [vp, C.c_int, C.c_void_p, C.c_size_t]
        L.vp8hip_group_gather_bytes.argtypes = [vp, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        assert len(unique_id) == SHARD_ID_BYTES
        h = vp()
        rc = L.vp8hip_group_create(C.byref(h), device, unique_id, rank, world, key.encode() if key else None)
        if rc != 0:
            raise Vp8HipError(f"vp8hip_group_create(rank {rank} of {world}): {L.vp8hip_status_string(rc).decode()}")
        self.h, self.rank, self.world, self.device = h, rank, world, device

    @staticmethod
    def rendezvous(key: str, rank: int, timeout_s: float = 120.0) -> bytes:
        lib = load_library()
        lib.vp8hip_group_rendezvous.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_void_p]
        buf = (C.c_uint8 * SHARD_ID_BYTES)()
        rc = lib.vp8hip_group_rendezvous(key.encode(), rank, float(timeout_s), buf)
        if rc != 0:
            raise Vp8HipError(f"vp8hip_group_rendezvous({key!r}, rank {rank}): {lib.vp8hip_status_string(rc).decode()}")
        return bytes(buf)

    @classmethod
    def from_env(cls, device: int, key: str, timeout_s: float = 120.0) -> "Group":
        rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        return cls(device, cls.rendezvous(key, rank, timeout_s), rank, world, key)

    def _chk(self, rc, what):
        if rc != 0:
            raise Vp8HipError(f"vp8hip_group_{what}: {self.lib.vp8hip_status_string(rc).decode()} (hip error {self.lib.vp8hip_group_last_hip_error(self.h)})")

    def count(self) -> int:
        """ncclCommCount: the ranks RCCL itself counts"""
        return int(self.lib.vp8hip_group_count(self.h))

    def barrier(self):
        self._chk(self.lib.vp8hip_group_barrier(self.h), "barrier")

    def max(self, value: float) -> float:
        v = C.c_double(value)
        self._chk(self.lib.vp8hip_group_max(self.h, C.byref(v)), "max")
        return float(v.value)

    def all_gather(self, record: np.ndarray) -> np.ndarray:
        """a small fixed-size record (<= 4 KB) from every rank -> [world, ...] on every rank"""
        a = np.ascontiguousarray(record)
        out = np.empty((self.world,) + a.shape, a.dtype)
        self._chk(self.lib.vp8hip_group_all_gather(self.h, a.ctypes.data, a.nbytes, out.ctypes.data), "all_gather")
        return out

    def broadcast_bytes(self, data: bytes | None, nbytes: int, root: int = 0) -> bytes:
        buf = C.create_string_buffer(data if self.rank == root else b"", nbytes) if nbytes else None
        if nbytes:
            self._chk(self.lib.vp8hip_group_broadcast(self.h, root, buf, nbytes), "broadcast")
        return buf.raw[:nbytes] if nbytes else b""

    def gather_bytes(self, data, root: int = 0):
        """every rank's bytes (any length) end to end in rank order on `root`: (buffer, counts) there, (None, counts) elsewhere.
        `data`: bytes-like or a contiguous uint8 array."""
        a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        counts = self.all_gather(np.array([a.nbytes], np.uint64)).reshape(-1).copy()
        total = int(counts.sum())
        dst = np.empty(max(total, 1), np.uint8) if self.rank == root else None
        self._chk(self.lib.vp8hip_group_gather_bytes(self.h, root, a.ctypes.data if a.nbytes else None, a.nbytes,
                                                     dst.ctypes.data if dst is not None else None, counts.ctypes.data), "gather_bytes")
        return (dst[:total] if dst is not None else None), counts

    def close(self):
        if getattr(self, "h", None):
            self.lib.vp8hip_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frame_check(h: int, frame: bytes) -> int:
    """vp8drv_frame_check (include/vp8hip_driver.h): the fold bench.py holds a run's frames against a second coding with"""
    lib = load_library()
    lib.vp8drv_frame_check.argtypes = [C.c_uint64, C.c_char_p, C.c_size_t]
    lib.vp8drv_frame_check.restype = C.c_uint64
    return int(lib.vp8drv_frame_check(h, frame, len(frame)))


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data
    if isinstance(a, DeviceBuffer):
        return a.ptr
    return int(a)  # raw device/host address (e.g. torch tensor.data_ptr())


# ---- host-side mirror (no GPU needed) -----------------------------------------------------------
def quantizer_ladders(qi_min: int = 0, qi_max: int = 48):
    lib = load_library()
    a, b = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    lib.vp8host_quantizer_ladders(qi_min, qi_max, a, b)
    return list(a), list(b)


def loopfilter_strength(y: np.ndarray):
    lib = load_library()
    r, s = C.c_int32(), C.c_int32()
    y = np.ascontiguousarray(y, np.uint8)
    lib.vp8host_loopfilter_strength(y.ctypes.data, y.shape[1], y.shape[0], C.byref(r), C.byref(s))
    return r.value, s.value


class SceneState(C.Structure):
    """vp8host_scene_state: the hold-over of scene_change() and frames.last_key_detect (vp8enc.cpp:265-311)."""
    _fields_ = [("holdover", C.c_int32), ("last_key_detect", C.c_int32)]


def scene_change(state: SceneState, Udiff: int, Vdiff: int, frame_number: int) -> bool:
    lib = load_library()
    lib.vp8host_scene_change.argtypes = [C.POINTER(SceneState), C.c_int, C.c_int, C.c_int]
    return bool(lib.vp8host_scene_change(C.byref(state), int(Udiff), int(Vdiff), int(frame_number)))


def scene_plan(udiff, vdiff, gop_size: int):
    """vp8host_scene_plan: the serial loop's key-frame schedule with scene detection on, from the chroma differences of a file's frames
    (entry 0 unused) and the GOP length -> (is_key, by_scene), two bool arrays of len(udiff)."""
    lib = load_library()
    ud, vd = np.ascontiguousarray(udiff, np.int32), np.ascontiguousarray(vdiff, np.int32)
    if ud.ndim != 1 or ud.shape != vd.shape:
        raise ValueError("scene_plan: udiff and vdiff must be two 1-D arrays of one length")
    key, scene = np.zeros(ud.size, np.uint8), np.zeros(ud.size, np.uint8)
    lib.vp8host_scene_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    if lib.vp8host_scene_plan(ud.ctypes.data, vd.ctypes.data, ud.size, int(gop_size), key.ctypes.data, scene.ctypes.data) < 0:
        raise ValueError(f"scene_plan: refused (gop_size {gop_size})")
    return key.astype(bool), scene.astype(bool)


def prepare_segments_data(is_key: bool, refqi, qi_min: int, reductor: int, sharpness: int, update_filter: bool = False,
                          shrpnss: int = 0) -> np.ndarray:
    lib = load_library()
    q = (C.c_int32 * 4)(*[int(v) for v in refqi])
    sd = (C.c_int32 * 44)()
    lib.vp8host_prepare_segments_data(int(is_key), q, qi_min, reductor, sharpness, int(update_filter), shrpnss, sd)
    return np.array(list(sd), np.int32).reshape(4, 11)


def skip_prob(nz: np.ndarray) -> int:
    nz = np.ascontiguousarray(nz, np.int32)
    return load_library().vp8host_skip_prob(nz.ctypes.data, nz.size)


class Gop:
    """Frame-type state machine of the reference main loop (vp8enc.cpp:340-374)."""

    def __init__(self, gop_size: int = 150, altref_range: int = 5):
        self.lib = load_library()
        self.s = GopState()
        self.lib.vp8host_gop_init(C.byref(self.s), gop_size, altref_range)

    def next(self):
        self.lib.vp8host_gop_next(C.byref(self.s))
        return self.s

    def key_coded(self):
        self.lib.vp8host_gop_key_coded(C.byref(self.s))

    def inter_flags(self):
        g, a = C.c_int32(), C.c_int32()
        self.lib.vp8host_gop_inter_flags(C.byref(self.s), C.byref(g), C.byref(a))
        return g.value, a.value

    def frame_done(self):
        self.lib.vp8host_gop_frame_done(C.byref(self.s))


SCALE_AREA, SCALE_LANCZOS = 0, 1   # filter of vp8hip_set_source_scaling / vp8drv_config.scale_filter
SCALE_MAX_TAPS = 32                 # VP8HOST_SCALE_MAX_TAPS, include/vp8hip_host.h


def scale_taps(n_in: int, n_out: int, kind: int = SCALE_AREA):
    """vp8host_scale_taps: one dimension of one plane of the device's scaler -> (n_taps, start [n_out] int32, coef [n_out, n_taps] int16),
    the very tables k_scale_b applies.  Raises ValueError when the pair is refused (more than 32 taps, bad arguments)."""
    lib = load_library()
    lib.vp8host_scale_taps.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    n = C.c_int32(0)
    start = np.zeros(max(int(n_out), 1), np.int32)
    coef = np.zeros((max(int(n_out), 1), SCALE_MAX_TAPS), np.int16)
    if lib.vp8host_scale_taps(int(n_in), int(n_out), int(kind), C.byref(n), start.ctypes.data, coef.ctypes.data) != 0:
        raise ValueError(f"vp8host_scale_taps({n_in} -> {n_out}, kind {kind}) refused")
    assert not coef[:, n.value:].any()
    return n.value, start, np.ascontiguousarray(coef[:, :n.value])


class DrvConfig(C.Structure):
    """vp8drv_config, include/vp8hip_driver.h"""
    _fields_ = [("gop_size", C.c_int32), ("altref_range", C.c_int32), ("qi_min", C.c_int32), ("qi_max", C.c_int32),
                ("ssim_target", C.c_float), ("device_params", C.c_int32), ("check_ssim", C.c_int32),
                ("num_partitions", C.c_int32), ("display_width", C.c_int32), ("display_height", C.c_int32),
                ("host_bitstream", C.c_int32), ("overlap_filter", C.c_int32), ("ref_mask", C.c_int32),
                ("conformant_stream", C.c_int32), ("scene_detect", C.c_int32),
                ("src_width", C.c_int32), ("src_height", C.c_int32), ("loop_filter_type", C.c_int32),
                ("in_width", C.c_int32), ("in_height", C.c_int32), ("scale_filter", C.c_int32), ("quality_stats", C.c_int32)]


class DrvStats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("frame_number", "inter_frames", "key_frames", "last_use_golden",
                                          "last_use_altref", "last_prev_is_golden", "last_prev_is_altref",
                                          "last_was_altref", "redone_as_key", "last_replaced")] + \
               [("last_new_ssim", C.c_float), ("last_min_ssim", C.c_float), ("scene_changes", C.c_int32), ("refs_searched", C.c_int32)]


class Quality(C.Structure):
    """vp8hip_quality = vp8drv_quality, include/vp8hip.h: one measured frame"""
    _fields_ = [("frame_number", C.c_int32), ("is_key", C.c_int32), ("sse", C.c_uint64 * 3), ("samples", C.c_uint64 * 3),
                ("psnr", C.c_double * 3), ("psnr_all", C.c_double), ("ssim", C.c_double * 3), ("ssim_all", C.c_double)]


class QualitySummary(C.Structure):
    """vp8hip_quality_totals = vp8drv_quality_summary, include/vp8hip.h: every frame made final so far"""
    _fields_ = [("frames", C.c_int64), ("sse", C.c_uint64 * 3), ("samples", C.c_uint64 * 3), ("psnr", C.c_double * 3),
                ("psnr_all", C.c_double), ("psnr_avg", C.c_double), ("ssim", C.c_double * 3), ("ssim_all", C.c_double),
                ("psnr_min", C.c_double), ("psnr_min_frame", C.c_int64)]


class DenoiseStats(C.Structure):
    """vp8hip_denoise_stats, include/vp8hip.h: the last frame taken in by a context with vp8hip_set_denoise"""
    _fields_ = [("frame_number", C.c_int32), ("mbs_filtered", C.c_int32), ("mbs_total", C.c_int32)]


class DeinterlaceStats(C.Structure):
    """vp8hip_deinterlace_stats, include/vp8hip.h: the last frame taken in by a context with vp8hip_set_deinterlace"""
    _fields_ = [("frame_number", C.c_int32), ("woven", C.c_int32), ("missing", C.c_int32)]


class Analysis(C.Structure):
    """vp8hip_analysis, include/vp8hip.h: the frame analysis record of a context with vp8hip_set_analysis (every field an exact integer;
    the rules: include/vp8hip_host.h)"""
    _fields_ = [("frame_number", C.c_int32), ("is_key", C.c_int32), ("have_prev", C.c_int32), ("static_mbs", C.c_int32),
                ("spatial", C.c_uint64), ("temporal_sse", C.c_uint64), ("temporal_sad", C.c_uint64),
                ("coded", C.c_int32), ("mbs_total", C.c_int32), ("mbs_intra", C.c_int32), ("mbs_split", C.c_int32),
                ("mbs_zero_mv", C.c_int32), ("mbs_no_coeffs", C.c_int32), ("mbs_ref", C.c_int32 * 3), ("segment_mbs", C.c_int32 * 4),
                ("reserved", C.c_int32), ("mv_abs_sum", C.c_uint64 * 2), ("mv_sum", C.c_int64 * 2), ("mv_sq_sum", C.c_uint64),
                ("nz_coeffs", C.c_uint64)]

    SOURCE_FIELDS = ("have_prev", "static_mbs", "spatial", "temporal_sse", "temporal_sad")
    CODING_FIELDS = ("mbs_total", "mbs_intra", "mbs_split", "mbs_zero_mv", "mbs_no_coeffs", "mbs_ref", "segment_mbs", "mv_abs_sum", "mv_sum",
                     "mv_sq_sum", "nz_coeffs")

    def as_dict(self) -> dict:
        """every field but `reserved` as Python ints (arrays as lists)"""
        out = {}
        for name, _ in self._fields_:
            if name != "reserved":
                v = getattr(self, name)
                out[name] = int(v) if isinstance(v, int) else [int(x) for x in v]
        return out

    def text_line(self, nbytes: int) -> str:
        """the line the tools' -analysis / --analysis files carry for this frame: frame number, key flag, bytes, then every field in
        the struct's order, arrays element by element, separated by single spaces"""
        d = self.as_dict()
        vals = [d["frame_number"], d["is_key"], int(nbytes)]
        for name, _ in self._fields_[2:]:
            if name != "reserved":
                v = d[name]
                vals += v if isinstance(v, list) else [v]
        return " ".join(str(x) for x in vals)


class LumaAnalysis(C.Structure):
    """vp8host_luma_analysis, include/vp8hip_host.h"""
    _fields_ = [("spatial", C.c_uint64), ("temporal_sse", C.c_uint64), ("temporal_sad", C.c_uint64), ("static_mbs", C.c_int32),
                ("have_prev", C.c_int32)]


def aq_segment_map(luma, strength: int, width: int | None = None):
    """vp8host_aq_segment_map: the variance-adaptive segment map in plain C++ (include/vp8hip_host.h) on a luma plane whose rows are
    luma.shape[1] bytes apart; width (default: the row length) is the coded width.  Returns (map, e), uint8 per macroblock."""
    lib = load_library()
    lib.vp8host_aq_segment_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    luma = np.ascontiguousarray(luma, np.uint8)
    h, stride = luma.shape
    w = stride if width is None else int(width)
    mbs = max(w // 16, 0) * max(h // 16, 0)
    m, e = np.zeros(max(mbs, 1), np.uint8), np.zeros(max(mbs, 1), np.uint8)
    rc = lib.vp8host_aq_segment_map(luma.ctypes.data, stride, w, h, int(strength), m.ctypes.data, e.ctypes.data)
    if rc != 0:
        raise ValueError(f"vp8host_aq_segment_map({w}x{h}, stride {stride}, strength {strength}) refused")
    return m[:mbs], e[:mbs]


def analyse_luma(cur, prev=None) -> dict:
    """vp8host_analyse_luma: the source side of the analysis record in plain C++ on tight luma planes of the coded size"""
    lib = load_library()
    lib.vp8host_analyse_luma.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(LumaAnalysis)]
    cur = np.ascontiguousarray(cur, np.uint8)
    h, w = cur.shape
    if prev is not None:
        prev = np.ascontiguousarray(prev, np.uint8)
        if prev.shape != cur.shape:
            raise ValueError("analyse_luma: prev has another shape than cur")
    r = LumaAnalysis()
    if lib.vp8host_analyse_luma(cur.ctypes.data, prev.ctypes.data if prev is not None else None, w, h, C.byref(r)) != 0:
        raise ValueError(f"vp8host_analyse_luma({w}x{h}) refused")
    return {k: int(getattr(r, k)) for k, _ in LumaAnalysis._fields_}


DENOISE_SUM_Y, DENOISE_SAD_Y, DENOISE_SUM_C = 512, 2560, 128   # VP8HOST_DENOISE_*, include/vp8hip_host.h


class Temporal(C.Structure):
    """vp8host_temporal, include/vp8hip_host.h"""
    _fields_ = [(n, C.c_int32) for n in ("temporal_id", "use_golden", "refresh", "layer_sync")]


class LayerInfo(C.Structure):
    """vp8drv_layer_info, include/vp8hip_driver.h"""
    _fields_ = [(n, C.c_int32) for n in ("temporal_id", "tl0_pic_idx", "layer_sync", "refresh", "use_golden", "filtered")]


class IntraRefreshInfo(C.Structure):
    """vp8drv_intra_refresh_info, include/vp8hip_driver.h"""
    _fields_ = [("period", C.c_int32), ("last_q", C.c_int32), ("last_forced", C.c_int32), ("total_forced", C.c_int64)]


def intra_refresh_forced(period: int, q: int, r: int, c: int) -> bool:
    """vp8host_intra_refresh_forced: is macroblock (row r, column c) forced at phase q of the period; ValueError where the rule refuses"""
    lib = load_library()
    lib.vp8host_intra_refresh_forced.argtypes = [C.c_int] * 4
    v = lib.vp8host_intra_refresh_forced(int(period), int(q), int(r), int(c))
    if v < 0:
        raise ValueError(f"vp8host_intra_refresh_forced({period}, {q}, {r}, {c}) refused")
    return bool(v)


def intra_refresh_count(mbw: int, mbh: int, period: int, q: int) -> int:
    """vp8host_intra_refresh_count: the forced macroblocks of a frame of mbw x mbh macroblocks at phase q; ValueError where it refuses"""
    lib = load_library()
    lib.vp8host_intra_refresh_count.argtypes = [C.c_int] * 4
    v = lib.vp8host_intra_refresh_count(int(mbw), int(mbh), int(period), int(q))
    if v < 0:
        raise ValueError(f"vp8host_intra_refresh_count({mbw}, {mbh}, {period}, {q}) refused")
    return v


def temporal_step(layers: int, p: int, ref_mask: int = 3):
    """vp8host_temporal_step: the temporal-layer rule for the frame p shown frames behind the last key frame (the key frame: p = 0) ->
    dict(temporal_id, use_golden, refresh, layer_sync); ValueError where the rule refuses"""
    lib = load_library()
    lib.vp8host_temporal_step.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(Temporal)]
    t = Temporal()
    if lib.vp8host_temporal_step(int(layers), int(p), int(ref_mask), C.byref(t)) != 0:
        raise ValueError(f"vp8host_temporal_step({layers}, {p}) refused")
    return {k: int(getattr(t, k)) for k, _ in Temporal._fields_}


class ArfStats(C.Structure):
    """vp8drv_arf_stats, include/vp8hip_driver.h"""
    _fields_ = [("hidden_frames", C.c_int32), ("last_frames", C.c_int32), ("last_use_golden", C.c_int32), ("last_use_altref", C.c_int32),
                ("last_weight", C.c_int32 * 3)]


def _plane_table(frames):
    """[(Y, U, V), ...] -> (contiguous uint8 copies that must stay alive, a C array of n x 3 addresses)"""
    keep = [tuple(np.ascontiguousarray(p, np.uint8) for p in f) for f in frames]
    h, w = keep[0][0].shape
    for y, u, v in keep:
        if y.shape != (h, w) or u.shape != (h // 2, w // 2) or v.shape != (h // 2, w // 2):
            raise ValueError("the frames of a window are tight I420 planes of one even size")
    table = (C.c_void_p * (3 * len(keep)))(*[p.ctypes.data for f in keep for p in f])
    return keep, table


def arf_filter_frame(frames, centre: int, strength: int):
    """vp8host_arf_filter_frame: the device's temporal filter in plain C++ (the rule: include/vp8hip_host.h).  frames = [(Y, U, V), ...]
    -> ((Y, U, V) filtered, weights[3], vectors[tiles][n][2])"""
    lib = load_library()
    lib.vp8host_arf_filter_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
    keep, table = _plane_table(frames)
    h, w = keep[0][0].shape
    n = len(keep)
    out = (np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8))
    weights = np.zeros(3, np.int32)
    vectors = np.zeros((((w + 15) // 16) * ((h + 15) // 16), n, 2), np.int8)
    if lib.vp8host_arf_filter_frame(table, n, int(centre), int(strength), w, h, *[p.ctypes.data for p in out], weights.ctypes.data,
                                    vectors.ctypes.data) != 0:
        raise ValueError(f"vp8host_arf_filter_frame({w}x{h}, n {n}, centre {centre}, strength {strength}) refused")
    return out, [int(x) for x in weights], vectors


def arf_round_divide(acc, count) -> np.ndarray:
    """vp8host_arf_round_divide: (acc + count / 2) / count by the reciprocal multiply the host function and the kernel share"""
    lib = load_library()
    lib.vp8host_arf_round_divide.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.vp8host_arf_round_divide.restype = None
    a, c = np.ascontiguousarray(acc, np.uint32).reshape(-1), np.ascontiguousarray(count, np.uint32).reshape(-1)
    assert a.shape == c.shape
    out = np.zeros(a.shape, np.uint32)
    lib.vp8host_arf_round_divide(a.ctypes.data, c.ctypes.data, a.size, out.ctypes.data)
    return out


def denoise_frame(src, hist, level: int, have_history: bool):
    """vp8host_denoise_frame: the device's denoiser in plain C++ on tight planes of the coded size.  src = (Y, U, V); hist = (Y, U, V)
    arrays that are updated in place when level != 0 (or None with level 0) -> ((Y, U, V) out, macroblocks filtered)"""
    lib = load_library()
    lib.vp8host_denoise_frame.argtypes = [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    src = [np.ascontiguousarray(p, np.uint8) for p in src]
    h, w = src[0].shape
    out = [np.empty_like(p) for p in src]
    if hist is not None:
        for a, b in zip(hist, src):
            if a.dtype != np.uint8 or not a.flags["C_CONTIGUOUS"] or a.shape != b.shape:
                raise ValueError("denoise_frame: the history planes are contiguous uint8 arrays of the source planes' shapes")
    hp = [a.ctypes.data for a in hist] if hist is not None else [None] * 3
    n = C.c_int32(0)
    if lib.vp8host_denoise_frame(*[p.ctypes.data for p in src], *hp, *[p.ctypes.data for p in out], w, h, int(level), int(bool(have_history)),
                                 C.byref(n)) != 0:
        raise ValueError(f"vp8host_denoise_frame({w}x{h}, level {level}) refused")
    return out, n.value


DEINTERLACE_OFF, DEINTERLACE_FIELD, DEINTERLACE_ADAPTIVE = range(3)      # the modes of vp8hip_set_deinterlace
FIELD_TOP, FIELD_BOTTOM = 0, 1                                            # ... and its keep
FIELDS_PROGRESSIVE, FIELDS_TOP_FIRST, FIELDS_BOTTOM_FIRST = range(3)      # vp8host_field_order, include/vp8hip_host.h
_DEINTERLACE_MODES = {"off": 0, "field": 1, "adaptive": 2}
_FIELDS = {"top": 0, "bottom": 1}


def deinterlace_mode(name) -> int:
    """off / field / adaptive (or the number) -> the mode of vp8hip_set_deinterlace"""
    return _DEINTERLACE_MODES[name] if isinstance(name, str) else int(name)


def deinterlace_field(name) -> int:
    """top / bottom (or the number) -> the keep of vp8hip_set_deinterlace"""
    return _FIELDS[name] if isinstance(name, str) else int(name)


def deinterlace_frame(src, hist, mode: int, keep: int, have_history: bool):
    """vp8host_deinterlace_frame: the device's deinterlacer in plain C++ on tight planes.  src = (Y, U, V); hist = (Y, U, V) arrays that
    mode 2 reads (with have_history) and replaces by src, or None in modes 0 and 1 -> ((Y, U, V) out, woven luma samples)"""
    lib = load_library()
    lib.vp8host_deinterlace_frame.argtypes = [C.c_void_p] * 9 + [C.c_int] * 5 + [C.POINTER(C.c_int32)]
    src = [np.ascontiguousarray(p, np.uint8) for p in src]
    h, w = src[0].shape
    out = [np.empty_like(p) for p in src]
    if hist is not None:
        for a, b in zip(hist, src):
            if a.dtype != np.uint8 or not a.flags["C_CONTIGUOUS"] or a.shape != b.shape:
                raise ValueError("deinterlace_frame: the history planes are contiguous uint8 arrays of the source planes' shapes")
    hp = [a.ctypes.data for a in hist] if hist is not None else [None] * 3
    n = C.c_int32(0)
    if lib.vp8host_deinterlace_frame(*[p.ctypes.data for p in src], *hp, *[p.ctypes.data for p in out], w, h, int(mode), int(keep),
                                     int(bool(have_history)), C.byref(n)) != 0:
        raise ValueError(f"vp8host_deinterlace_frame({w}x{h}, mode {mode}, keep {keep}) refused")
    return out, n.value


# vp8host_source_format, include/vp8hip_host.h: what the three pointers of a source frame are (vp8hip_set_source_format)
FORMAT_I420, FORMAT_NV12, FORMAT_I422, FORMAT_I444, FORMAT_P010, FORMAT_I010, FORMAT_I210, FORMAT_I410 = range(8)
FORMAT_NAMES = ["i420", "nv12", "i422", "i444", "p010", "i010", "i210", "i410"]
# the packed family (one plane; 8 .. 15 are no format)
FORMAT_YUY2, FORMAT_UYVY, FORMAT_BGRA, FORMAT_RGBA = range(16, 20)
PACKED_FORMAT_NAMES = {"yuy2": FORMAT_YUY2, "uyvy": FORMAT_UYVY, "bgra": FORMAT_BGRA, "rgba": FORMAT_RGBA}
# vp8host_colour_matrix: what BGRA / RGBA are read with (vp8hip_set_source_colour)
COLOUR_BT601_LIMITED, COLOUR_BT709_LIMITED, COLOUR_BT601_FULL, COLOUR_BT709_FULL = range(4)
COLOUR_MATRIX_NAMES = ["bt601", "bt709"]
COLOUR_RANGE_NAMES = ["limited", "full"]


def source_format(name) -> int:
    """a format's number from its name (any case) or number; ValueError for what vp8hip_set_source_format would refuse"""
    if isinstance(name, str) and name.lower() in FORMAT_NAMES:
        return FORMAT_NAMES.index(name.lower())
    if isinstance(name, str) and name.lower() in PACKED_FORMAT_NAMES:
        return PACKED_FORMAT_NAMES[name.lower()]
    if isinstance(name, (int, np.integer)) and (0 <= int(name) < len(FORMAT_NAMES) or int(name) in PACKED_FORMAT_NAMES.values()):
        return int(name)
    raise ValueError(f"unknown source format {name!r}: one of {', '.join(FORMAT_NAMES + list(PACKED_FORMAT_NAMES))}")


def source_format_name(fmt: int) -> str:
    fmt = source_format(fmt)
    return FORMAT_NAMES[fmt] if fmt < len(FORMAT_NAMES) else {v: k for k, v in PACKED_FORMAT_NAMES.items()}[fmt]


def source_colour(matrix="bt601", range_="limited") -> int:
    """a colour matrix's number from a matrix name (bt601, bt709) and a range (limited, full), or from its number; ValueError for
    what vp8hip_set_source_colour would refuse"""
    if isinstance(matrix, (int, np.integer)) and not isinstance(matrix, bool):
        if 0 <= int(matrix) < 4:
            return int(matrix)
        raise ValueError(f"unknown colour matrix {matrix!r}: 0 .. 3")
    m, r = str(matrix).lower(), str(range_).lower()
    if m not in COLOUR_MATRIX_NAMES or r not in COLOUR_RANGE_NAMES:
        raise ValueError(f"unknown colour matrix {matrix!r} / range {range_!r}: one of {', '.join(COLOUR_MATRIX_NAMES)} and one of {', '.join(COLOUR_RANGE_NAMES)}")
    return COLOUR_MATRIX_NAMES.index(m) + 2 * COLOUR_RANGE_NAMES.index(r)


def colour_coefficients(matrix: int):
    """vp8host_colour_coefficients: (the Y, U and V rows as a 3x3 int32 array, columns R, G, B; the luma offset)"""
    lib = load_library()
    lib.vp8host_colour_coefficients.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    c, off = (C.c_int32 * 9)(), C.c_int32(0)
    if lib.vp8host_colour_coefficients(int(matrix), c, C.byref(off)) != 0:
        raise ValueError(f"vp8host_colour_coefficients({matrix}) refused")
    return np.array(list(c), np.int32).reshape(3, 3), off.value


def source_plane_bytes(fmt: int, width: int, height: int):
    """vp8host_source_plane_bytes: bytes of the three planes a frame of this format hands in (the third is 0 for NV12 / P010)"""
    lib = load_library()
    lib.vp8host_source_plane_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    b = (C.c_size_t * 3)()
    if lib.vp8host_source_plane_bytes(int(fmt), int(width), int(height), b) != 0:
        raise ValueError(f"vp8host_source_plane_bytes(format {fmt}, {width}x{height}) refused")
    return [int(x) for x in b]


def convert_frame(fmt: int, width: int, height: int, planes, matrix: int = 0):
    """vp8host_convert_frame / vp8host_convert_frame_colour: the device's format conversion in plain C++.  planes = the format's
    one, two or three planes as contiguous arrays of exactly vp8host_source_plane_bytes bytes each (uint8, or uint16 for the 16-bit
    formats on a little-endian host); matrix = the colour matrix BGRA / RGBA are read with -> (Y, U, V) uint8 arrays, I420 of
    width x height"""
    lib = load_library()
    lib.vp8host_convert_frame.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    lib.vp8host_convert_frame_colour.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    need = source_plane_bytes(fmt, width, height)
    planes = [np.ascontiguousarray(p) for p in planes]
    while len(planes) < 3:
        planes.append(planes[-1])
    for p, n in zip(planes, need):
        if n and p.nbytes != n:
            raise ValueError(f"convert_frame: a plane of {p.nbytes} bytes where format {fmt} at {width}x{height} has {n}")
    out = (np.empty((height, width), np.uint8), np.empty((height // 2, width // 2), np.uint8), np.empty((height // 2, width // 2), np.uint8))
    if matrix:
        rc = lib.vp8host_convert_frame_colour(int(fmt), int(matrix), int(width), int(height), *[p.ctypes.data for p in planes], *[o.ctypes.data for o in out])
    else:
        rc = lib.vp8host_convert_frame(int(fmt), int(width), int(height), *[p.ctypes.data for p in planes], *[o.ctypes.data for o in out])
    if rc != 0:
        raise ValueError(f"vp8host_convert_frame(format {fmt}, matrix {matrix}, {width}x{height}) refused")
    return out


# vp8host_transfer, include/vp8hip_host.h: the transfer function P010 / I010 frames carry (vp8hip_set_source_transfer)
TRANSFER_SDR, TRANSFER_PQ, TRANSFER_HLG = range(3)
TRANSFER_NAMES = ["sdr", "pq", "hlg"]
PEAK_MIN, PEAK_MAX, PEAK_DEFAULT = 400, 10000, 1000      # VP8HOST_PEAK_MIN, VP8HOST_PEAK_MAX; the tools' default


def source_transfer(name) -> int:
    """a transfer's number from its name (sdr, pq, hlg; any case) or number; ValueError for what vp8hip_set_source_transfer would refuse"""
    if isinstance(name, str) and name.lower() in TRANSFER_NAMES:
        return TRANSFER_NAMES.index(name.lower())
    if isinstance(name, (int, np.integer)) and not isinstance(name, bool) and 0 <= int(name) < len(TRANSFER_NAMES):
        return int(name)
    raise ValueError(f"unknown source transfer {name!r}: one of {', '.join(TRANSFER_NAMES)}")


def tonemap_tables(transfer, peak: int = PEAK_DEFAULT):
    """vp8host_tonemap_tables: the four tables of the tone-mapping rule for (transfer, peak) -> (lin, gain) uint32 and (lo, hi) uint8
    arrays of 4096 entries each"""
    lib = load_library()
    lib.vp8host_tonemap_tables.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
    t = source_transfer(transfer) if isinstance(transfer, str) else int(transfer)
    out = (np.empty(4096, np.uint32), np.empty(4096, np.uint32), np.empty(4096, np.uint8), np.empty(4096, np.uint8))
    if lib.vp8host_tonemap_tables(t, int(peak), *[o.ctypes.data for o in out]) != 0:
        raise ValueError(f"vp8host_tonemap_tables(transfer {transfer}, peak {peak}) refused")
    return out


def tonemap_frame(fmt, transfer, peak: int, width: int, height: int, planes, matrix: int = 0):
    """vp8host_tonemap_frame: the device's tone mapping in plain C++.  planes = the two (P010) or three (I010) planes as contiguous
    arrays of exactly vp8host_source_plane_bytes bytes each; matrix = the colour matrix the SDR picture is written with -> (Y, U, V)
    uint8 arrays, I420 of width x height"""
    lib = load_library()
    lib.vp8host_tonemap_frame.argtypes = [C.c_int] * 6 + [C.c_void_p] * 6
    fmt = source_format(fmt) if isinstance(fmt, str) else int(fmt)
    t = source_transfer(transfer) if isinstance(transfer, str) else int(transfer)
    need = source_plane_bytes(fmt, width, height)
    planes = [np.ascontiguousarray(p) for p in planes]
    while len(planes) < 3:
        planes.append(planes[-1])
    for p, n in zip(planes, need):
        if n and p.nbytes != n:
            raise ValueError(f"tonemap_frame: a plane of {p.nbytes} bytes where format {fmt} at {width}x{height} has {n}")
    out = (np.empty((height, width), np.uint8), np.empty((height // 2, width // 2), np.uint8), np.empty((height // 2, width // 2), np.uint8))
    if lib.vp8host_tonemap_frame(fmt, t, int(peak), int(matrix), int(width), int(height), *[p.ctypes.data for p in planes], *[o.ctypes.data for o in out]) != 0:
        raise ValueError(f"vp8host_tonemap_frame(format {fmt}, transfer {transfer}, peak {peak}, matrix {matrix}, {width}x{height}) refused")
    return out


MAX_OVERLAYS = 4      # VP8HIP_MAX_OVERLAYS, include/vp8hip.h


def _layer_args(pixels, lw, lh, pitch):
    """a layer as the C entry points take it: a uint8 array of shape (lh, lw, 4), whose rows may be further apart than 4 lw bytes, or
    device memory (anything with data_ptr()) with lw, lh and, unless the rows are tight, pitch -> (keep-alive, pointer, lw, lh, pitch, on_device)"""
    if hasattr(pixels, "data_ptr"):
        if lw is None or lh is None:
            raise ValueError("a layer in device memory needs lw and lh")
        return pixels, pixels.data_ptr(), int(lw), int(lh), int(pitch if pitch is not None else 4 * lw), True
    a = np.asarray(pixels)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("a layer is a uint8 array of shape (lh, lw, 4)")
    if a.strides[2] != 1 or a.strides[1] != 4 or a.strides[0] < 4 * a.shape[1]:
        a = np.ascontiguousarray(a)
    return a, a.ctypes.data, int(a.shape[1]), int(a.shape[0]), int(a.strides[0]) if a.shape[0] > 1 else max(int(a.strides[0]), 4 * int(a.shape[1])), False


def parse_overlay(spec: str):
    """FILE:WxH:X:Y[:OPACITY], the tools' -overlay / --overlay option: FILE holds W x H pixels of raw BGRA, tight -> (pixels as a uint8
    array of shape (H, W, 4), x, y, opacity); ValueError for anything else"""
    parts = spec.rsplit(":", 4)      # (FILE may hold colons of its own: the fields are counted from the right)
    if len(parts) < 5 or "x" not in parts[1].lower():
        parts = spec.rsplit(":", 3) + ["255"]
    try:
        path, size, x, y, opacity = parts
        w, h = (int(v) for v in size.lower().split("x"))
        x, y, opacity = int(x), int(y), int(opacity)
    except ValueError:
        raise ValueError(f"overlay {spec!r}: FILE:WxH:X:Y[:OPACITY]") from None
    if not (1 <= w <= 16384 and 1 <= h <= 16384 and 0 <= opacity <= 255):
        raise ValueError(f"overlay {spec!r}: a size of 1..16384 and an opacity of 0..255")
    px = np.fromfile(path, np.uint8)
    if px.size != w * h * 4:
        raise ValueError(f"overlay {path}: {px.size} bytes, not {w} x {h} x 4 of BGRA")
    return px.reshape(h, w, 4), x, y, opacity


_OVERLAY_SET_ARGS = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 6


MAX_TILES = 16   # VP8HIP_MAX_TILES, include/vp8hip_host.h


class Tile(C.Structure):
    """vp8hip_tile: frames of in_w x in_h scaled to w x h at (x, y) of the picture; filter SCALE_AREA or SCALE_LANCZOS"""
    _fields_ = [(n, C.c_int32) for n in ("in_w", "in_h", "x", "y", "w", "h", "filter")]


class TilePlanes(C.Structure):
    """vp8hip_tile_planes: a tile's three planes of one frame, a pointer and a pitch each (0 = tight); y NULL = absent"""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("pitch_y", C.c_int32), ("pitch_u", C.c_int32), ("pitch_v", C.c_int32)]


def tiles_array(tiles):
    """[(in_w, in_h, x, y, w, h[, filter]), ...] or Tile objects -> a ctypes array of vp8hip_tile"""
    tiles = list(tiles)
    arr = (Tile * max(len(tiles), 1))()
    for k, t in enumerate(tiles):
        arr[k] = t if isinstance(t, Tile) else Tile(*[int(x) for x in t])
    return arr


def parse_tile(spec: str):
    """FILE.yuv:INWxINH:X:Y:W:H[:area|lanczos], the tools' --tile option -> (path, Tile)"""
    try:
        parts = spec.rsplit(":", 6) if spec.rsplit(":", 1)[-1].lower() in ("area", "lanczos") else spec.rsplit(":", 5) + ["area"]
        path, size, x, y, w, h, kind = parts
        iw, ih = (int(v) for v in size.lower().split("x"))
        return path, Tile(iw, ih, int(x), int(y), int(w), int(h), SCALE_LANCZOS if kind.lower() == "lanczos" else SCALE_AREA)
    except (ValueError, TypeError):
        raise ValueError(f"tile {spec!r}: FILE.yuv:INWxINH:X:Y:W:H[:area|lanczos]") from None


def tile_planes_array(frames, n=None):
    """One frame's sources, frames[k] for tile k: None (absent), three uint8 arrays of two dimensions whose rows may be strided (the
    pitch is the row stride), or (y, u, v, (pitch_y, pitch_u, pitch_v)) of addresses in host or device memory -> (a ctypes array of
    vp8hip_tile_planes, what must stay alive while it is used)"""
    frames = list(frames)
    arr = (TilePlanes * max(n or len(frames), 1))()
    keep = []
    for k, f in enumerate(frames):
        if f is None:
            continue
        if len(f) == 4:
            ptrs, pitches = [_ptr(p) for p in f[:3]], [int(p) for p in f[3]]
        else:
            ptrs, pitches = [], []
            for p in f:
                if p.dtype != np.uint8 or p.ndim != 2 or p.strides[1] != 1:
                    raise ValueError("tile planes: uint8 arrays of two dimensions with contiguous rows")
                keep.append(p)
                ptrs.append(p.ctypes.data)
                pitches.append(0 if p.strides[0] == p.shape[1] else int(p.strides[0]))
        arr[k] = TilePlanes(ptrs[0], ptrs[1], ptrs[2], pitches[0], pitches[1], pitches[2])
    return arr, keep


def compose_frame(pw: int, ph: int, tiles, frames, bg=(16, 128, 128)):
    """vp8host_compose_frame: the device's canvas rule in plain C++ -> the picture's planes (y, u, v), tight, pw x ph.  tiles as for
    tiles_array, frames as for tile_planes_array (host memory).  ValueError for what the rule refuses."""
    lib = load_library()
    tiles = list(tiles)
    ta = tiles_array(tiles)
    pa, keep = tile_planes_array(frames, len(tiles))
    lib.vp8host_compose_frame.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    out = (np.zeros((max(ph, 0), max(pw, 0)), np.uint8), np.zeros((max(ph, 0) // 2, max(pw, 0) // 2), np.uint8), np.zeros((max(ph, 0) // 2, max(pw, 0) // 2), np.uint8))
    if lib.vp8host_compose_frame(int(pw), int(ph), C.addressof(ta), len(tiles), int(bg[0]), int(bg[1]), int(bg[2]), C.addressof(pa),
                                 *[o.ctypes.data for o in out]) != 0:
        raise ValueError(f"vp8host_compose_frame({pw}x{ph}, {len(tiles)} tiles) refused")
    del keep
    return out


def overlay_frame(pixels, x: int, y: int, opacity: int, planes, fmt=None, matrix: int = 0):
    """vp8host_overlay_frame: the device's overlay rule in plain C++.  pixels = the layer, a uint8 array of shape (lh, lw, 4), BGRA
    unless fmt says RGBA; planes = (Y, U, V), I420 of the picture size -> new (Y, U, V) with the layer composed at (x, y)"""
    lib = load_library()
    lib.vp8host_overlay_frame.argtypes = [C.c_int] * 5 + [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3
    fmt = FORMAT_BGRA if fmt is None else (source_format(fmt) if isinstance(fmt, str) else int(fmt))
    keep, ptr, lw, lh, pitch, dev = _layer_args(pixels, None, None, None)
    out = [np.array(p, np.uint8, order="C") for p in planes]
    ph, pw = out[0].shape
    if out[1].shape != (ph // 2, pw // 2) or out[2].shape != (ph // 2, pw // 2):
        raise ValueError("overlay_frame: planes are not I420 of one size")
    if lib.vp8host_overlay_frame(fmt, int(matrix), lw, lh, pitch, ptr, int(x), int(y), int(opacity), pw, ph, *[o.ctypes.data for o in out]) != 0:
        raise ValueError(f"vp8host_overlay_frame(format {fmt}, matrix {matrix}, {lw}x{lh} pitch {pitch} at ({x}, {y}), opacity {opacity}, picture {pw}x{ph}) refused")
    return tuple(out)


def _pitch3(pitch):
    p = [int(x) for x in pitch] + [0, 0, 0]
    return (C.c_int32 * 3)(*p[:3])


def source_window(fmt, width: int, height: int, x: int, y: int, pitch):
    """vp8host_source_window: the window of width x height at (x, y) in a surface of format `fmt` whose planes' rows are pitch[p] bytes
    apart -> (offset[3], row_bytes[3], rows[3]); ValueError for what the rule refuses"""
    lib = load_library()
    lib.vp8host_source_window.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int32), C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    fmt = source_format(fmt) if isinstance(fmt, str) else int(fmt)
    off, rb, rows = (C.c_size_t * 3)(), (C.c_int32 * 3)(), (C.c_int32 * 3)()
    if lib.vp8host_source_window(fmt, int(width), int(height), int(x), int(y), _pitch3(pitch), off, rb, rows) != 0:
        raise ValueError(f"vp8host_source_window(format {fmt}, {width}x{height} at ({x}, {y}), pitch {list(pitch)}) refused")
    return [int(v) for v in off], [int(v) for v in rb], [int(v) for v in rows]


def window_frame(fmt, width: int, height: int, x: int, y: int, pitch, planes):
    """vp8host_window_frame: the window of a surface in plain C++.  planes = the surface's planes as contiguous uint8 arrays (as many
    as the format has) -> the window's tight planes as flat uint8 arrays"""
    lib = load_library()
    lib.vp8host_window_frame.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int32)] + [C.c_void_p] * 6
    fmt = source_format(fmt) if isinstance(fmt, str) else int(fmt)
    _, rb, rows = source_window(fmt, width, height, x, y, pitch)
    planes = [np.ascontiguousarray(p).view(np.uint8).reshape(-1) for p in planes]
    out = [np.empty(rb[p] * rows[p], np.uint8) for p in range(3) if rows[p]]
    if len(planes) < len(out):
        raise ValueError(f"window_frame: format {fmt} has {len(out)} planes")
    src = [planes[p].ctypes.data if p < len(out) else None for p in range(3)]
    dst = [out[p].ctypes.data if p < len(out) else None for p in range(3)]
    if lib.vp8host_window_frame(fmt, int(width), int(height), int(x), int(y), _pitch3(pitch), *src, *dst) != 0:
        raise ValueError("vp8host_window_frame refused")
    return out


def orient_frame(turns: int, mirror: int, planes):
    """vp8host_orient_frame: `turns` clockwise quarter turns behind a left-right flip (mirror) in plain C++.  planes = (Y, U, V), tight
    I420 as it comes in -> the upright (Y, U, V)"""
    lib = load_library()
    lib.vp8host_orient_frame.argtypes = [C.c_int] * 4 + [C.c_void_p] * 6
    src = [np.ascontiguousarray(p, np.uint8) for p in planes]
    h, w = src[0].shape
    out = [np.empty(p.shape[::-1] if int(turns) & 1 else p.shape, np.uint8) for p in src]
    if lib.vp8host_orient_frame(int(turns), int(mirror), w, h, *[p.ctypes.data for p in src], *[p.ctypes.data for p in out]) != 0:
        raise ValueError(f"vp8host_orient_frame(turns {turns}, mirror {mirror}, {w}x{h}) refused")
    return out


def planes_from_i420(fmt: int, y, u, v):
    """the planes of format `fmt` that carry this 8-bit I420 frame exactly -- chroma replicated, samples shifted up to the depth --
    as flat uint8 arrays: vp8host_convert_frame returns the frame from them (for tools and benchmarks that need frames in a format)"""
    fmt = source_format(fmt)
    if fmt in (FORMAT_YUY2, FORMAT_UYVY):      # the I422 frame's samples, interleaved
        yy = np.ascontiguousarray(y, np.uint8)
        h, w = yy.shape
        cu, cv = (np.repeat(np.asarray(p, np.uint8), 2, axis=0) for p in (u, v))
        q = np.empty((h, w // 2, 4), np.uint8)
        ly, lu = (0, 1) if fmt == FORMAT_YUY2 else (1, 0)
        q[:, :, ly], q[:, :, ly + 2], q[:, :, lu], q[:, :, lu + 2] = yy[:, 0::2], yy[:, 1::2], cu, cv
        return [q.ravel()]
    if fmt in (FORMAT_BGRA, FORMAT_RGBA):
        raise ValueError("planes_from_i420: no RGB frame carries an arbitrary I420 frame exactly")
    nv, tall, wide, deep = fmt in (FORMAT_NV12, FORMAT_P010), fmt in (FORMAT_I422, FORMAT_I444, FORMAT_I210, FORMAT_I410), \
        fmt in (FORMAT_I444, FORMAT_I410), fmt >= FORMAT_P010
    shift = 0 if not deep else (8 if fmt == FORMAT_P010 else 2)

    def plane(a):
        a = np.ascontiguousarray(a, np.uint8)
        return (a.astype("<u2") << shift).ravel().view(np.uint8) if deep else a.ravel()
    c = [np.repeat(np.repeat(p, 2 if tall else 1, axis=0), 2 if wide else 1, axis=1) for p in (np.asarray(u), np.asarray(v))]
    if nv:
        return [plane(y), plane(np.stack(c, axis=-1))]
    return [plane(y), plane(c[0]), plane(c[1])]


class NativeDriver:
    """The reference's frame loop as native host code (vp8_driver.cpp, include/vp8hip_driver.h): one call per
    frame.  `.hip` is a view of its context for downloads and taps."""

    def __init__(self, width: int, height: int, device: int = 0, **cfg):
        self.lib = load_library()
        lib = self.lib
        lib.vp8drv_default_config.argtypes = [C.POINTER(DrvConfig)]
        lib.vp8drv_default_config.restype = None
        lib.vp8drv_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.POINTER(DrvConfig)]
        lib.vp8drv_destroy.argtypes = [C.c_void_p]
        lib.vp8drv_destroy.restype = None
        lib.vp8drv_context.argtypes = [C.c_void_p]
        lib.vp8drv_context.restype = C.c_void_p
        lib.vp8drv_encode_frame_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.vp8drv_encode_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.vp8drv_get_stats.argtypes = [C.c_void_p, C.POINTER(DrvStats)]
        lib.vp8drv_get_stats.restype = None
        self.cfg = DrvConfig()
        lib.vp8drv_default_config(C.byref(self.cfg))
        for k, v in cfg.items():
            setattr(self.cfg, k, v)
        h = C.c_void_p()
        rc = lib.vp8drv_create(C.byref(h), width, height, device, C.byref(self.cfg))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_create({width}x{height}) failed: {lib.vp8hip_status_string(rc).decode()} ({rc})")
        self.h = h
        self.hip = Vp8Hip.borrowed(lib.vp8drv_context(h), width, height)

    def _ret(self, rc: int) -> bool:
        if rc < 0:
            raise Vp8HipError(f"vp8drv_encode_frame: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")
        return rc == 1

    def encode_frame_device(self, d_y: int, d_u: int, d_v: int, force_key: bool = False) -> bool:
        """True if the frame was coded as a key frame (vp8hip_intra_transform), False for an inter frame."""
        return self._ret(self.lib.vp8drv_encode_frame_device(self.h, d_y, d_u, d_v, int(force_key)))

    def encode_frame_host(self, y, u, v, force_key: bool = False) -> bool:
        y, u, v = (np.ascontiguousarray(p, np.uint8) for p in (y, u, v))
        return self._ret(self.lib.vp8drv_encode_frame_host(self.h, y.ctypes.data, u.ctypes.data, v.ctypes.data, int(force_key)))

    def encode_frame_host_ptr(self, y: int, u: int, v: int, force_key: bool = False) -> bool:
        """encode_frame_host on host ADDRESSES (page-locked buffers: HostBuffer.data_ptr())"""
        self.lib.vp8drv_encode_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        return self._ret(self.lib.vp8drv_encode_frame_host(self.h, y, u, v, int(force_key)))

    def prefetch_frame_host_ptr(self, y: int, u: int, v: int) -> None:
        """the NEXT frame's planes started on their way (vp8drv_prefetch_frame_host); hand the same addresses to the next encode_frame_host_ptr"""
        self.lib.vp8drv_prefetch_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = self.lib.vp8drv_prefetch_frame_host(self.h, y, u, v)
        if rc < 0:
            raise Vp8HipError(f"vp8drv_prefetch_frame_host: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")

    def resolve(self) -> bool:
        """check_SSIM's verdict on the frame just coded (vp8drv_resolve): True if the frame ended as a key frame"""
        self.lib.vp8drv_resolve.argtypes = [C.c_void_p]
        return self._ret(self.lib.vp8drv_resolve(self.h))

    def get_frame(self) -> bytes:
        """The frame just coded as the reference's entropy_encode() + gather_frame() emit it (vp8drv_get_frame)."""
        self.lib.vp8drv_get_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        n = C.c_size_t(0)
        while True:
            buf = self._frame_buffer()
            rc = self.lib.vp8drv_get_frame(self.h, buf.ctypes.data, len(buf), C.byref(n))
            if rc == ERR_OVERFLOW and len(buf) < self._frame_cap_max():   # the frame is still there: a larger buffer, same call
                self._frame_buf = np.zeros(min(2 * len(buf), self._frame_cap_max()), np.uint8)
                continue
            break
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_frame: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")
        return self._frame_buf[:n.value].tobytes()

    def _frame_cap_max(self) -> int:
        # the most a frame can be: 304 bools per 4x4 block at one byte each is far above it; the device scratch bound
        return self.hip.mbs * 25 * 304 // 4 + (1 << 20)

    def _frame_buffer(self):
        if getattr(self, "_frame_buf", None) is None:
            self._frame_buf = np.zeros(self.hip.mbs * 900 + 65536, np.uint8)
        return self._frame_buf

    def get_frame_begin(self) -> None:
        """Enqueue the entropy stage of the frame just coded and return (vp8drv_get_frame_begin); get_frame_end collects."""
        self.lib.vp8drv_get_frame_begin.argtypes = [C.c_void_p]
        rc = self.lib.vp8drv_get_frame_begin(self.h)
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_frame_begin: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")

    def get_frame_end(self) -> bytes:
        self.lib.vp8drv_get_frame_end.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        n = C.c_size_t(0)
        while True:
            buf = self._frame_buffer()
            rc = self.lib.vp8drv_get_frame_end(self.h, buf.ctypes.data, len(buf), C.byref(n))
            if rc == ERR_OVERFLOW and len(buf) < self._frame_cap_max():
                self._frame_buf = np.zeros(min(2 * len(buf), self._frame_cap_max()), np.uint8)
                continue
            break
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_frame_end: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")
        return self._frame_buf[:n.value].tobytes()

    def video_out_buffer(self, nframes: int) -> np.ndarray:
        """host memory for the frames of `nframes` calls' worth of video (twenty times a dense frame at the reference's default
        quantisers), every page touched: what a caller allocates ONCE, before its clock starts, and hands to encode_video_device"""
        out = np.empty(nframes * (self.hip.mbs * 64 + (1 << 16)), np.uint8)
        out.fill(0)
        return out

    def encode_video_device(self, nframes: int, frame_ptrs, start: int = 0, out: np.ndarray | None = None, views: bool = False):
        """vp8drv_encode_video_device: `nframes` frames of one video with the frames out, natively (frame t =
        frame_ptrs[(start + t) % len]); returns (list of frames, key-frame count).  The frames land back to back in `out`
        (video_out_buffer(); allocated here when None); views=True returns them as memoryviews into it instead of copies."""
        nd = len(frame_ptrs)
        F = ((C.c_void_p * 3) * nd)(*[(C.c_void_p * 3)(*p) for p in frame_ptrs])
        if out is None:
            out = np.empty(nframes * (self.hip.mbs * 64 + (1 << 16)), np.uint8)
        cap = int(out.size)
        sizes = (C.c_uint32 * max(nframes, 1))()
        keys = C.c_int(0)
        self.lib.vp8drv_encode_video_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                        C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        rc = self.lib.vp8drv_encode_video_device(self.h, int(nframes), C.cast(F, C.c_void_p), nd, int(start), out.ctypes.data, cap, sizes, C.byref(keys))
        if rc < 0:
            raise Vp8HipError(f"vp8drv_encode_video_device: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")
        frames, o = [], 0
        mv = memoryview(out)
        for t in range(nframes):
            n = int(sizes[t])
            frames.append(mv[o:o + n] if views else mv[o:o + n].tobytes())
            o += n
        return frames, int(keys.value)

    def encode_video_device_no_frames(self, nframes: int, frame_ptrs, start: int = 0):
        """vp8drv_encode_video_device with out = NULL: `nframes` frames of one video, no frames out, no interpreter in the loop"""
        nd = len(frame_ptrs)
        F = ((C.c_void_p * 3) * nd)(*[(C.c_void_p * 3)(*p) for p in frame_ptrs])
        self.lib.vp8drv_encode_video_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                        C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        rc = self.lib.vp8drv_encode_video_device(self.h, int(nframes), C.cast(F, C.c_void_p), nd, int(start), None, 0, None, None)
        if rc < 0:
            raise Vp8HipError(f"vp8drv_encode_video_device: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")

    def stats(self) -> DrvStats:
        s = DrvStats()
        self.lib.vp8drv_get_stats(self.h, C.byref(s))
        return s

    def frame_quality(self) -> Quality:
        """vp8drv_get_frame_quality (cfg quality_stats=1): PSNR / SSIM of the frame just made final (its verdict is taken first)"""
        q = Quality()
        self.lib.vp8drv_get_frame_quality.argtypes = [C.c_void_p, C.POINTER(Quality)]
        rc = self.lib.vp8drv_get_frame_quality(self.h, C.byref(q))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_frame_quality: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")
        return q

    def set_denoise(self, level: int) -> None:
        """vp8drv_set_denoise: temporal noise reduction of the source frames, level 0 (off) to 3; the history restarts at the GOP
        schedule's key frames"""
        self.lib.vp8drv_set_denoise.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.vp8drv_set_denoise(self.h, int(level))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_denoise({level}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_source_colour(self, matrix, range_="limited") -> None:
        """vp8drv_set_source_colour: BGRA / RGBA frames are read with this matrix (a COLOUR_* number, or bt601 / bt709 and a range)"""
        self.lib.vp8drv_set_source_colour.argtypes = [C.c_void_p, C.c_int]
        m = source_colour(matrix, range_) if isinstance(matrix, str) else int(matrix)
        rc = self.lib.vp8drv_set_source_colour(self.h, m)
        if rc < 0:
            raise Vp8HipError(f"vp8drv_set_source_colour({m}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_overlay(self, slot: int, pixels, x: int, y: int, opacity: int = 255, fmt=None, matrix: int = 0, lw=None, lh=None, pitch=None) -> None:
        """vp8drv_set_overlay_host / _device: the layer `pixels` (a uint8 array of shape (lh, lw, 4), or device memory with lw, lh and
        pitch; BGRA unless fmt says RGBA) is burnt into every frame taken in from now on, its top-left pixel at (x, y) of the picture"""
        fmt = FORMAT_BGRA if fmt is None else (source_format(fmt) if isinstance(fmt, str) else int(fmt))
        keep, ptr, lw, lh, pitch, dev = _layer_args(pixels, lw, lh, pitch)
        f = self.lib.vp8drv_set_overlay_device if dev else self.lib.vp8drv_set_overlay_host
        f.argtypes = _OVERLAY_SET_ARGS
        rc = f(self.h, int(slot), fmt, int(matrix), ptr, lw, lh, pitch, int(x), int(y), int(opacity))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_overlay({slot}, {lw}x{lh} at ({x}, {y})): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_canvas(self, tiles, bg=(16, 128, 128)) -> None:
        """vp8drv_set_canvas: frames are composed of these tiles (tiles_array's forms) over the background from now on; [] ends it"""
        tiles = list(tiles)
        ta = tiles_array(tiles)
        self.lib.vp8drv_set_canvas.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4
        rc = self.lib.vp8drv_set_canvas(self.h, C.addressof(ta), len(tiles), int(bg[0]), int(bg[1]), int(bg[2]))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_canvas({len(tiles)} tiles): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)
        self._canvas_tiles = len(tiles)

    def encode_tiles(self, frames, force_key: bool = False, device: bool = False) -> bool:
        """vp8drv_encode_frame_tiles_host / _device: one frame from the tiles' sources (tile_planes_array's forms; None = absent).
        True if the frame was coded as a key frame."""
        pa, keep = tile_planes_array(frames, getattr(self, "_canvas_tiles", 0))
        f = self.lib.vp8drv_encode_frame_tiles_device if device else self.lib.vp8drv_encode_frame_tiles_host
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        rc = f(self.h, C.addressof(pa), int(force_key))
        del keep
        return self._ret(rc)

    def set_overlay_placement(self, slot: int, x: int, y: int, opacity: int = 255) -> None:
        """vp8drv_set_overlay_placement: move or fade the slot's layer"""
        self.lib.vp8drv_set_overlay_placement.argtypes = [C.c_void_p] + [C.c_int] * 4
        rc = self.lib.vp8drv_set_overlay_placement(self.h, int(slot), int(x), int(y), int(opacity))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_overlay_placement({slot}, {x}, {y}, {opacity}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def clear_overlay(self, slot: int = -1) -> None:
        """vp8drv_clear_overlay: the slot's layer, or with -1 every layer, is gone from the next frame on"""
        self.lib.vp8drv_clear_overlay.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.vp8drv_clear_overlay(self.h, int(slot))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_clear_overlay({slot}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_source_transfer(self, transfer, peak: int = PEAK_DEFAULT) -> None:
        """vp8drv_set_source_transfer: P010 / I010 frames carry this transfer (a TRANSFER_* number, or sdr / pq / hlg) graded for `peak`
        nits and are tone-mapped to SDR on the device; sdr (0) = off"""
        self.lib.vp8drv_set_source_transfer.argtypes = [C.c_void_p, C.c_int, C.c_int]
        t = source_transfer(transfer) if isinstance(transfer, str) else int(transfer)
        rc = self.lib.vp8drv_set_source_transfer(self.h, t, int(peak))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_source_transfer({t}, {peak}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_source_format(self, fmt) -> None:
        """vp8drv_set_source_format: the frames handed in from now on are this format's planes (a FORMAT_* number or its name)"""
        self.lib.vp8drv_set_source_format.argtypes = [C.c_void_p, C.c_int]
        fmt = source_format(fmt) if isinstance(fmt, str) else int(fmt)
        rc = self.lib.vp8drv_set_source_format(self.h, fmt)
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_source_format({fmt}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_source_window(self, pitch, x: int = 0, y: int = 0) -> None:
        """vp8drv_set_source_window: the planes handed in are the plane bases of a surface whose rows are pitch[p] bytes apart, and the
        frame is the window of the incoming size at (x, y); pitch None = off"""
        self.lib.vp8drv_set_source_window.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int]
        rc = self.lib.vp8drv_set_source_window(self.h, None if pitch is None else _pitch3(pitch), int(x), int(y))
        if rc < 0:
            raise Vp8HipError(f"vp8drv_set_source_window({pitch}, {x}, {y}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_source_orientation(self, turns: int, mirror: int = 0) -> None:
        """vp8drv_set_source_orientation: source frames are turned by `turns` clockwise quarter turns behind a left-right flip
        (mirror) on the device; with an odd `turns` the planes handed in are the incoming height wide and the incoming width high"""
        self.lib.vp8drv_set_source_orientation.argtypes = [C.c_void_p, C.c_int, C.c_int]
        rc = self.lib.vp8drv_set_source_orientation(self.h, int(turns), int(mirror))
        if rc < 0:
            raise Vp8HipError(f"vp8drv_set_source_orientation({turns}, {mirror}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_deinterlace(self, mode, keep=0) -> None:
        """vp8drv_set_deinterlace: interlaced source frames made progressive; mode off / field / adaptive (0, 1, 2), keep top / bottom
        (0, 1); the history of adaptive restarts at the GOP schedule's key frames"""
        self.lib.vp8drv_set_deinterlace.argtypes = [C.c_void_p, C.c_int, C.c_int]
        rc = self.lib.vp8drv_set_deinterlace(self.h, deinterlace_mode(mode), deinterlace_field(keep))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_deinterlace({mode}, {keep}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def deinterlace_stats(self) -> DeinterlaceStats:
        """vp8drv_get_deinterlace_stats: the last frame taken in"""
        s = DeinterlaceStats()
        self.lib.vp8drv_get_deinterlace_stats.argtypes = [C.c_void_p, C.POINTER(DeinterlaceStats)]
        rc = self.lib.vp8drv_get_deinterlace_stats(self.h, C.byref(s))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_deinterlace_stats: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)
        return s

    def denoise_stats(self) -> DenoiseStats:
        """vp8drv_get_denoise_stats: the last frame taken in"""
        s = DenoiseStats()
        self.lib.vp8drv_get_denoise_stats.argtypes = [C.c_void_p, C.POINTER(DenoiseStats)]
        rc = self.lib.vp8drv_get_denoise_stats(self.h, C.byref(s))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_denoise_stats: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)
        return s

    def set_analysis(self, on: bool = True) -> None:
        """vp8drv_set_analysis: the frame analysis record of every frame from the next one taken in on"""
        self.lib.vp8drv_set_analysis.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.vp8drv_set_analysis(self.h, int(on))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_analysis({on}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def frame_analysis(self) -> Analysis:
        """vp8drv_get_frame_analysis: the record of the frame just made final (its verdict is taken first)"""
        a = Analysis()
        self.lib.vp8drv_get_frame_analysis.argtypes = [C.c_void_p, C.POINTER(Analysis)]
        rc = self.lib.vp8drv_get_frame_analysis(self.h, C.byref(a))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_frame_analysis: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)
        return a

    def set_arf(self, strength_plus_one: int) -> None:
        """vp8drv_set_arf: hidden alternate reference frames, 0 = off, 1..7 = on at strength 0..6 (include/vp8hip_driver.h)"""
        self.lib.vp8drv_set_arf.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.vp8drv_set_arf(self.h, int(strength_plus_one))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_arf({strength_plus_one}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def encode_arf_host(self, frames, centre: int) -> None:
        """vp8drv_encode_arf_host: a hidden frame from the window frames = [(Y, U, V), ...] in host memory, centred on frames[centre];
        get_frame() then delivers its bytes"""
        self.lib.vp8drv_encode_arf_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        keep, table = _plane_table(frames)
        rc = self.lib.vp8drv_encode_arf_host(self.h, table, len(keep), int(centre))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_encode_arf_host: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def encode_arf_device(self, ptrs, centre: int) -> None:
        """vp8drv_encode_arf_device: the same for ptrs = [(d_y, d_u, d_v), ...] device addresses of tight planes of the incoming size"""
        self.lib.vp8drv_encode_arf_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        table = (C.c_void_p * (3 * len(ptrs)))(*[a for f in ptrs for a in f])
        rc = self.lib.vp8drv_encode_arf_device(self.h, table, len(ptrs), int(centre))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_encode_arf_device: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def arf_stats(self) -> ArfStats:
        """vp8drv_get_arf_stats: hidden frames coded, and the last one's window, reference flags and tiles by block weight"""
        st = ArfStats()
        self.lib.vp8drv_get_arf_stats.argtypes = [C.c_void_p, C.POINTER(ArfStats)]
        rc = self.lib.vp8drv_get_arf_stats(self.h, C.byref(st))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_arf_stats: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)
        return st

    def set_temporal_layers(self, layers: int, flags: int = 0) -> None:
        """vp8drv_set_temporal_layers: 1 (off) to 3 temporal layers from the next key frame on; flags: TL_KEEP_RECON (include/vp8hip_driver.h)"""
        self.lib.vp8drv_set_temporal_layers.argtypes = [C.c_void_p, C.c_int, C.c_int]
        rc = self.lib.vp8drv_set_temporal_layers(self.h, int(layers), int(flags))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_temporal_layers({layers}, {flags}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_intra_refresh(self, period: int) -> None:
        """vp8drv_set_intra_refresh: cyclic intra refresh with the period (4 .. 1024; 0 = off) from the next frame on (include/vp8hip_driver.h)"""
        self.lib.vp8drv_set_intra_refresh.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.vp8drv_set_intra_refresh(self.h, int(period))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_intra_refresh({period}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def intra_refresh(self) -> IntraRefreshInfo:
        """vp8drv_get_intra_refresh: period, last_q, last_forced, total_forced"""
        info = IntraRefreshInfo()
        self.lib.vp8drv_get_intra_refresh.argtypes = [C.c_void_p, C.POINTER(IntraRefreshInfo)]
        rc = self.lib.vp8drv_get_intra_refresh(self.h, C.byref(info))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_intra_refresh: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)
        return info

    def frame_layer(self) -> LayerInfo:
        """vp8drv_get_frame_layer: temporal_id, tl0_pic_idx, layer_sync, refresh, use_golden and filtered of the frame just made final"""
        info = LayerInfo()
        self.lib.vp8drv_get_frame_layer.argtypes = [C.c_void_p, C.POINTER(LayerInfo)]
        rc = self.lib.vp8drv_get_frame_layer(self.h, C.byref(info))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_frame_layer: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)
        return info

    def set_segment_mode(self, mode: int, strength: int = 0) -> None:
        """vp8drv_set_segment_mode: 0 off, 1 the caller's segment map, 2 variance-adaptive at strength 1..3 (inter frames only)"""
        self.lib.vp8drv_set_segment_mode.argtypes = [C.c_void_p, C.c_int, C.c_int]
        rc = self.lib.vp8drv_set_segment_mode(self.h, int(mode), int(strength))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_segment_mode({mode}, {strength}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_segment_map(self, seg_map) -> None:
        """vp8drv_set_segment_map: mode 1's map, one byte 0..3 per macroblock in raster order, in force until replaced"""
        m = np.ascontiguousarray(seg_map, np.uint8).reshape(-1)
        if m.size != self.hip.mbs:
            raise ValueError(f"a segment map has one byte per macroblock: {self.hip.mbs}, not {m.size}")
        self.lib.vp8drv_set_segment_map.argtypes = [C.c_void_p, C.c_void_p]
        rc = self.lib.vp8drv_set_segment_map(self.h, m.ctypes.data)
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_segment_map: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_quantizer(self, qi_min: int, qi_max: int) -> None:
        """vp8drv_set_quantizer: both quantizer ladders made again from this pair, from the next frame coded on"""
        self.lib.vp8drv_set_quantizer.argtypes = [C.c_void_p, C.c_int, C.c_int]
        rc = self.lib.vp8drv_set_quantizer(self.h, int(qi_min), int(qi_max))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_set_quantizer({qi_min}, {qi_max}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def quantizer(self):
        """vp8drv_get_quantizer: (qi_min, qi_max) in force"""
        a, b = C.c_int32(), C.c_int32()
        self.lib.vp8drv_get_quantizer.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        rc = self.lib.vp8drv_get_quantizer(self.h, C.byref(a), C.byref(b))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_quantizer: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)
        return a.value, b.value

    def quality_summary(self) -> QualitySummary:
        """vp8drv_get_quality_summary: over every frame made final so far"""
        s = QualitySummary()
        self.lib.vp8drv_get_quality_summary.argtypes = [C.c_void_p, C.POINTER(QualitySummary)]
        rc = self.lib.vp8drv_get_quality_summary(self.h, C.byref(s))
        if rc != 0:
            raise Vp8HipError(f"vp8drv_get_quality_summary: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")
        return s

    def close(self):
        if getattr(self, "h", None):
            self.hip.close()
            self.lib.vp8drv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeBatch:
    """Up to four NativeDrivers advanced one frame at a time with ONE launch per stage (vp8drv_batch_*, include/vp8hip_driver.h)."""

    def __init__(self, drivers):
        self.lib = load_library()
        self.drivers = list(drivers)
        n = len(self.drivers)
        self.lib.vp8drv_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
        self.lib.vp8drv_batch_destroy.argtypes = [C.c_void_p]
        self.lib.vp8drv_batch_destroy.restype = None
        self.lib.vp8drv_batch_encode_frame_device.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                              C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        arr = (C.c_void_p * n)(*[d.h for d in self.drivers])
        h = C.c_void_p()
        rc = self.lib.vp8drv_batch_create(C.byref(h), arr, n)
        if rc != 0:
            raise Vp8HipError(f"vp8drv_batch_create: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")
        self.h = h
        self.n = n
        self._ptrs = [(C.c_void_p * n)() for _ in range(3)]
        self._key = (C.c_int * n)()
        self._members = (C.c_int * n)()

    def encode_frame_device(self, planes, members=None, host=False, force_key=None):
        """planes[i] = (d_y, d_u, d_v) device pointers of member i's frame (None for a member that sits this call out, or
        members[i] false); returns the list of "was a key frame" flags.  host=True: the pointers are HOST addresses
        (vp8drv_batch_encode_frame_host; the planes stay unchanged until the next call has returned).  force_key[i] true: member i's
        frame is a key frame whatever its schedule says (a chunk that starts at a planned key frame)."""
        fk = None if force_key is None else (C.c_int * self.n)(*[1 if k else 0 for k in force_key])
        for i, p in enumerate(planes):
            on = p is not None and (members is None or members[i])
            self._members[i] = 1 if on else 0
            if on:
                self._ptrs[0][i], self._ptrs[1][i], self._ptrs[2][i] = p
        fn = self.lib.vp8drv_batch_encode_frame_host if host else self.lib.vp8drv_batch_encode_frame_device
        fn.argtypes = self.lib.vp8drv_batch_encode_frame_device.argtypes
        rc = fn(self.h, self._members, self._ptrs[0], self._ptrs[1], self._ptrs[2], fk, self._key)
        if rc < 0:
            raise Vp8HipError(f"vp8drv_batch_encode_frame_{'host' if host else 'device'}: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")
        return [bool(k) for k in self._key]

    def encode_frame_host(self, planes, members=None, force_key=None):
        return self.encode_frame_device(planes, members, host=True, force_key=force_key)

    def scan_frame_device(self, planes, members=None, host=False):
        """The members' frames taken in and their chroma differences against each member's previous frame started, one launch for all
        (vp8drv_batch_scan_frame_device / _host); nothing is coded.  planes and members as in encode_frame_device; scan_result() follows."""
        for i, p in enumerate(planes):
            on = p is not None and (members is None or members[i])
            self._members[i] = 1 if on else 0
            if on:
                self._ptrs[0][i], self._ptrs[1][i], self._ptrs[2][i] = p
        fn = self.lib.vp8drv_batch_scan_frame_host if host else self.lib.vp8drv_batch_scan_frame_device
        fn.argtypes = self.lib.vp8drv_batch_encode_frame_device.argtypes[:5]
        rc = fn(self.h, self._members, self._ptrs[0], self._ptrs[1], self._ptrs[2])
        if rc != 0:
            raise Vp8HipError(f"vp8drv_batch_scan_frame_{'host' if host else 'device'}: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def scan_frame_host(self, planes, members=None):
        self.scan_frame_device(planes, members, host=True)

    def scan_result(self):
        """[(Udiff, Vdiff)] of the members of the last scan call, None for those that sat it out (vp8drv_batch_scan_result)"""
        ud, vd = (C.c_int32 * self.n)(), (C.c_int32 * self.n)()
        self.lib.vp8drv_batch_scan_result.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        rc = self.lib.vp8drv_batch_scan_result(self.h, self._members, ud, vd)
        if rc != 0:
            raise Vp8HipError(f"vp8drv_batch_scan_result: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")
        return [(ud[i], vd[i]) if self._members[i] else None for i in range(self.n)]

    def lane(self) -> int:
        """the chain stream (lane) this batch shares with other batches of its device, -1 = a stream of its own (vp8drv_batch_lane)"""
        self.lib.vp8drv_batch_lane.argtypes = [C.c_void_p]
        return int(self.lib.vp8drv_batch_lane(self.h))

    def ready(self) -> bool:
        """no member's check_SSIM verdict is still on its way: the next encode_frame_device would not wait (vp8drv_batch_ready)"""
        self.lib.vp8drv_batch_ready.argtypes = [C.c_void_p]
        return bool(self.lib.vp8drv_batch_ready(self.h))

    def get_frames_begin(self, members=None) -> None:
        """The entropy stage of the members' frames in one set of launches (vp8drv_batch_get_frame_begin); every member's
        driver then takes its frame with get_frame_end()."""
        for i in range(self.n):
            self._members[i] = 1 if (members is None or members[i]) else 0
        self.lib.vp8drv_batch_get_frame_begin.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        rc = self.lib.vp8drv_batch_get_frame_begin(self.h, self._members)
        if rc != 0:
            raise Vp8HipError(f"vp8drv_batch_get_frame_begin: {self.lib.vp8hip_status_string(rc).decode()} ({rc})")

    def close(self):
        if getattr(self, "h", None):
            self.lib.vp8drv_batch_destroy(self.h)
            self.h = None

    @staticmethod
    def encode_frames_device_all(batches, nframes, frame_ptrs, starts, frames_out=False, host=False):
        """nframes frames on every batch, one native host thread per batch (vp8drv_batches_encode_frames_device): frame t of member i of
        batch k = frame_ptrs[(starts[k][i] + t) % len(frame_ptrs)], frame_ptrs = [(d_y, d_u, d_v)].  Returns key-frame counts [k][i].
        host=True: the frames are in HOST memory (HostBuffer) and cross the link on their way in (vp8drv_batches_encode_frames_host)."""
        lib = batches[0].lib
        n, nd = len(batches), len(frame_ptrs)
        F = ((C.c_void_p * 3) * nd)(*[(C.c_void_p * 3)(*p) for p in frame_ptrs])
        st = [(C.c_int * b.n)(*[int(x) for x in s]) for b, s in zip(batches, starts)]
        ko = [(C.c_int * b.n)() for b in batches]
        bo = [(C.c_uint64 * b.n)() for b in batches]
        co = [(C.c_uint64 * b.n)() for b in batches]       # vp8drv_frame_check folded over every delivered frame, per member
        IP, UP = C.POINTER(C.c_int), C.POINTER(C.c_uint64)
        fn = lib.vp8drv_batches_encode_frames_host if host else lib.vp8drv_batches_encode_frames_device
        fn.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(IP), C.POINTER(IP), C.POINTER(UP), C.POINTER(UP)]
        rc = fn((C.c_void_p * n)(*[b.h for b in batches]), n, int(nframes), C.cast(F, C.c_void_p), nd,
                                                      (IP * n)(*[C.cast(a, IP) for a in st]), (IP * n)(*[C.cast(a, IP) for a in ko]),
                                                      (UP * n)(*[C.cast(a, UP) for a in bo]) if frames_out else None,
                                                      (UP * n)(*[C.cast(a, UP) for a in co]) if frames_out else None)
        if rc < 0:
            raise Vp8HipError(f"vp8drv_batches_encode_frames_{'host' if host else 'device'}: {lib.vp8hip_status_string(rc).decode()} ({rc})")
        if frames_out == "check":
            return [list(a) for a in ko], [list(a) for a in bo], [list(a) for a in co]
        if frames_out:
            return [list(a) for a in ko], [list(a) for a in bo]
        return [list(a) for a in ko]

    @staticmethod
    def encode_frame_device_all(batches, planes):
        """one frame on every batch, each served as its verdicts come in (vp8drv_batches_encode_frame_device); planes[k][i] = member
        i of batch k's (d_y, d_u, d_v).  Returns the per-batch lists of "was a key frame" flags."""
        lib = batches[0].lib
        n = len(batches)
        for b, pl in zip(batches, planes):
            for i, p in enumerate(pl):
                b._ptrs[0][i], b._ptrs[1][i], b._ptrs[2][i] = p
        PP = C.POINTER(C.c_void_p)
        arr = lambda j: (PP * n)(*[C.cast(b._ptrs[j], PP) for b in batches])
        keys = (C.POINTER(C.c_int) * n)(*[C.cast(b._key, C.POINTER(C.c_int)) for b in batches])
        hs = (C.c_void_p * n)(*[b.h for b in batches])
        lib.vp8drv_batches_encode_frame_device.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(PP), C.POINTER(PP), C.POINTER(PP), C.POINTER(C.POINTER(C.c_int))]
        rc = lib.vp8drv_batches_encode_frame_device(hs, n, arr(0), arr(1), arr(2), keys)
        if rc < 0:
            raise Vp8HipError(f"vp8drv_batches_encode_frame_device: {lib.vp8hip_status_string(rc).decode()} ({rc})")
        return [[bool(k) for k in b._key] for b in batches]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- device path ------------------------------------------------------------------------------
class Vp8Hip:
    """One encoder context on one MI355X (vp8hip_create ... vp8hip_destroy)."""

    def __init__(self, width: int, height: int, ssim_target: float = -1.0, device: int = 0):
        self.lib = load_library()
        self.W, self.H = width, height
        self.mbs = (width // 16) * (height // 16)
        self.b8 = self.mbs * 4
        h = C.c_void_p()
        rc = self.lib.vp8hip_create(C.byref(h), width, height, ssim_target, device)
        if rc != 0:
            raise Vp8HipError(f"vp8hip_create({width}x{height}, device {device}) failed: "
                              f"{self.lib.vp8hip_status_string(rc).decode()} ({rc}); the HIP path has no CPU fallback")
        self.h = h

    def _chk(self, rc: int, what: str):
        if rc != 0:
            raise Vp8HipError(f"{what}: {self.lib.vp8hip_status_string(rc).decode()} ({rc}), hipError "
                              f"{self.lib.vp8hip_last_hip_error(self.h)}")

    @classmethod
    def borrowed(cls, handle, width: int, height: int):
        """View of a context owned by somebody else (the native driver): same methods, no destroy."""
        self = cls.__new__(cls)
        self.lib = load_library()
        self.W, self.H = width, height
        self.mbs = (width // 16) * (height // 16)
        self.b8 = self.mbs * 4
        self.h = C.c_void_p(handle)
        self._borrowed = True
        return self

    def close(self):
        if getattr(self, "_borrowed", False):
            self.h = None
            return
        if getattr(self, "h", None):
            self.lib.vp8hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_current(self, y, u, v):
        self._chk(self.lib.vp8hip_upload_current(self.h, _ptr(y), _ptr(u), _ptr(v)), "upload_current")

    def set_current_device(self, y, u, v):
        self._chk(self.lib.vp8hip_set_current_device(self.h, _ptr(y), _ptr(u), _ptr(v)), "set_current_device")

    def upload_last(self, y, u, v):
        self._chk(self.lib.vp8hip_upload_last(self.h, _ptr(y), _ptr(u), _ptr(v)), "upload_last")

    def set_last_device(self, y, u, v):
        self._chk(self.lib.vp8hip_set_last_device(self.h, _ptr(y), _ptr(u), _ptr(v)), "set_last_device")

    def upload_recon(self, y, u, v):
        self._chk(self.lib.vp8hip_upload_recon(self.h, _ptr(y), _ptr(u), _ptr(v)), "upload_recon")

    def set_segments(self, sd):
        sd = np.ascontiguousarray(sd, np.int32).reshape(-1)
        assert sd.size == 44
        self._chk(self.lib.vp8hip_set_segments(self.h, sd.ctypes.data), "set_segments")

    def inter_transform(self, prev_is_golden, prev_is_altref, use_golden, use_altref):
        self._chk(self.lib.vp8hip_inter_transform(self.h, int(prev_is_golden), int(prev_is_altref), int(use_golden),
                                                  int(use_altref)), "inter_transform")

    def download_results(self, recon: bool = True) -> dict:
        W, H, n = self.W, self.H, self.mbs
        out = {
            "MB_parts": np.zeros(n, np.int32), "MB_reference_frame": np.zeros(n, np.int32),
            "MB_vectors": np.zeros((n, 4, 2), np.int16), "MB_coeffs": np.zeros((n, 25, 16), np.int16),
            "MB_segment_id": np.zeros(n, np.int32), "MB_SSIM": np.zeros(n, np.float32),
        }
        if recon:
            out.update(recon_Y=np.zeros((H, W), np.uint8), recon_U=np.zeros((H // 2, W // 2), np.uint8),
                       recon_V=np.zeros((H // 2, W // 2), np.uint8))
        r = _Results(**{k: a.ctypes.data for k, a in out.items()})
        self._chk(self.lib.vp8hip_download_results(self.h, C.byref(r)), "download_results")
        if recon:  # before the loop filter these are the unfiltered planes
            out["prefilter_Y"], out["prefilter_U"], out["prefilter_V"] = out.pop("recon_Y"), out.pop("recon_U"), out.pop("recon_V")
        return out

    def intra_transform(self):
        """intra_transform (intra_part.h:1089-1109): the current frame as a key frame, on the device."""
        self._chk(self.lib.vp8hip_intra_transform(self.h), "intra_transform")

    def set_source_size(self, src_width: int, src_height: int):
        """copy_with_padding on the device: current frames come as tight planes of this size (include/vp8hip.h)"""
        self.lib.vp8hip_set_source_size.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(self.lib.vp8hip_set_source_size(self.h, int(src_width), int(src_height)), "set_source_size")
        self.src = (int(src_width), int(src_height))

    def conformant_stream(self, on: bool = True):
        """NOT the reference: the stream decodes to the encoder's own reconstruction (include/vp8hip.h)"""
        self.lib.vp8hip_conformant_stream.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.vp8hip_conformant_stream(self.h, int(on)), "conformant_stream")

    def check_ssim(self):
        """check_SSIM (vp8enc.cpp:231-263) on the device: (replaced, new_SSIM, min SSIM)."""
        repl, new, mn = C.c_int32(), C.c_float(), C.c_float()
        self._chk(self.lib.vp8hip_check_ssim(self.h, C.byref(repl), C.byref(new), C.byref(mn)), "check_ssim")
        return repl.value, np.float32(new.value), np.float32(mn.value)

    def reserve_frame_path(self):
        """the entropy stage's scratch and the frame buffer now instead of at the first frame (vp8hip_reserve_frame_path)"""
        self.lib.vp8hip_reserve_frame_path.argtypes = [C.c_void_p]
        self._chk(self.lib.vp8hip_reserve_frame_path(self.h), "reserve_frame_path")

    def reserve_frame_path_dense(self):
        """... for the densest frame there can be: a caller that starts frame n + 1 before taking frame n's bytes never loses a recode"""
        self.lib.vp8hip_reserve_frame_path_dense.argtypes = [C.c_void_p]
        self._chk(self.lib.vp8hip_reserve_frame_path_dense(self.h), "reserve_frame_path_dense")

    def check_ssim_async(self, refqi, qi_min: int):
        """check_SSIM enqueued, nobody waiting (vp8hip_check_ssim_async); check_ssim_result() collects the verdict"""
        q = (C.c_int32 * 4)(*[int(x) for x in refqi])
        self.lib.vp8hip_check_ssim_async.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
        self._chk(self.lib.vp8hip_check_ssim_async(self.h, q, int(qi_min)), "check_ssim_async")

    def check_ssim_result(self):
        """(replaced, new_SSIM, min SSIM, filter updated) of the last check_ssim_async"""
        repl, new, mn, upd = C.c_int32(), C.c_float(), C.c_float(), C.c_int32()
        self.lib.vp8hip_check_ssim_result.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        self._chk(self.lib.vp8hip_check_ssim_result(self.h, C.byref(repl), C.byref(new), C.byref(mn), C.byref(upd)), "check_ssim_result")
        return repl.value, np.float32(new.value), np.float32(mn.value), bool(upd.value)

    def download_intra(self):
        """(modes[MBs][16], is_inter[MBs]) of the last intra_transform / check_ssim."""
        modes, is_inter = np.zeros((self.mbs, 16), np.int32), np.zeros(self.mbs, np.int32)
        self._chk(self.lib.vp8hip_download_intra(self.h, modes.ctypes.data, is_inter.ctypes.data), "download_intra")
        return modes, is_inter

    def encode_header(self, is_key, is_golden=0, is_altref=0, sharpness=SHARPNESS_ON_DEVICE, partitions_log2=0, use_intra_info=False,
                      loop_filter_type=0, width=0, height=0) -> np.ndarray:
        """encode_header (entropy_host.cpp:709-1256) on the device: the first partition with its frame tag."""
        class P(C.Structure):
            _fields_ = [(n, C.c_int32) for n in ("is_key", "is_golden", "is_altref", "loop_filter_type", "loop_filter_sharpness",
                                                  "partitions_log2", "width", "height", "use_intra_info")]
        p = P(int(is_key), int(is_golden), int(is_altref), loop_filter_type, int(sharpness), partitions_log2, width, height, int(use_intra_info))
        self.lib.vp8hip_encode_header.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        cap = self.mbs * 96 + 16384
        out = np.zeros(cap, np.uint8)
        n = C.c_size_t(0)
        self._chk(self.lib.vp8hip_encode_header(self.h, C.byref(p), out.ctypes.data, cap, C.byref(n)), "encode_header")
        return out[:n.value].copy()

    def _debug_set_ssim(self, ssim):
        s = np.ascontiguousarray(ssim, np.float32)
        assert s.size == self.mbs
        self.lib.vp8hip_debug_upload_ssim.argtypes = [C.c_void_p, C.c_void_p]
        self._chk(self.lib.vp8hip_debug_upload_ssim(self.h, s.ctypes.data), "debug_upload_ssim")

    def upload_mb_data(self, coeffs=None, parts=None, seg=None):
        self._chk(self.lib.vp8hip_upload_mb_data(self.h, _ptr(coeffs), _ptr(parts), _ptr(seg)), "upload_mb_data")

    def prepare_filter_mask(self, want_nz: bool = True):
        nz = np.zeros(self.mbs, np.int32) if want_nz else None
        self._chk(self.lib.vp8hip_prepare_filter_mask(self.h, _ptr(nz)), "prepare_filter_mask")
        return nz

    def loop_filter(self):
        self._chk(self.lib.vp8hip_loop_filter(self.h), "loop_filter")

    def loop_filter_hidden(self):
        """vp8hip_loop_filter_hidden: the end of a hidden frame -- the filtered reconstruction becomes ALTREF, LAST stays"""
        self.lib.vp8hip_loop_filter_hidden.argtypes = [C.c_void_p]
        self._chk(self.lib.vp8hip_loop_filter_hidden(self.h), "loop_filter_hidden")
        self.hidden_recon = tuple(self.debug(DBG_ARF_FRAME, r) for r in (3, 4, 5))

    def loop_filter_refresh(self, refresh: int, filter: bool = True):
        """vp8hip_loop_filter_refresh: the end of a shown frame of a temporal layer -- REFRESH_LAST: loop_filter(); REFRESH_GOLDEN: the
        filtered reconstruction becomes GOLDEN and LAST stays; REFRESH_NONE: it is dropped (unfiltered with filter = False)"""
        self.lib.vp8hip_loop_filter_refresh.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(self.lib.vp8hip_loop_filter_refresh(self.h, int(refresh), int(filter)), "loop_filter_refresh")

    def intra_refresh(self, period: int, q: int):
        """vp8hip_intra_refresh: the forced macroblocks of phase q of the period in the inter reconstruction in flight (asynchronous)"""
        self.lib.vp8hip_intra_refresh.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(self.lib.vp8hip_intra_refresh(self.h, int(period), int(q)), "intra_refresh")

    def refresh_frame(self):
        """(Y, U, V) of the surface the last loop_filter_refresh with REFRESH_GOLDEN or REFRESH_NONE ended (VP8HIP_DBG_REFRESH_FRAME)"""
        return tuple(self.debug(DBG_REFRESH_FRAME, r) for r in (0, 1, 2))

    def arf_filter(self, frames, centre: int, strength: int):
        """vp8hip_arf_filter_host: the window frames = [(Y, U, V), ...] (host memory, the incoming size) through the temporal filter;
        the filtered frame becomes the current frame.  Returns it as it left the filter."""
        self.lib.vp8hip_arf_filter_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        keep, table = _plane_table(frames)
        self._chk(self.lib.vp8hip_arf_filter_host(self.h, table, len(keep), int(centre), int(strength)), "arf_filter_host")
        return self.arf_frame()

    def arf_filter_device(self, ptrs, centre: int, strength: int):
        """vp8hip_arf_filter_device: the same for ptrs = [(d_y, d_u, d_v), ...] device addresses"""
        self.lib.vp8hip_arf_filter_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        table = (C.c_void_p * (3 * len(ptrs)))(*[a for f in ptrs for a in f])
        self._chk(self.lib.vp8hip_arf_filter_device(self.h, table, len(ptrs), int(centre), int(strength)), "arf_filter_device")

    def incoming_size(self):
        """size of the planes this view believes the context takes as current frames: what set_source_size / set_source_scaling of
        THIS object said last (a borrowed view of a driver's context sets .src itself), else the coded size"""
        w, h = getattr(self, "src", (0, 0))
        return (w, h) if w and h else (self.W, self.H)

    def arf_frame(self):
        """the frame as it left the last temporal filter launch: (Y, U, V), tight, the incoming size (the debug tap)"""
        return tuple(self.debug(DBG_ARF_FRAME, r) for r in (0, 1, 2))

    def arf_result(self):
        """vp8hip_arf_result: the (tile, frame) pairs of the last filter launch by block weight 0, 1, 2"""
        wgt = (C.c_int32 * 3)()
        self.lib.vp8hip_arf_result.argtypes = [C.c_void_p, C.c_void_p]
        self._chk(self.lib.vp8hip_arf_result(self.h, wgt), "arf_result")
        return [int(x) for x in wgt]

    def arf_release(self):
        self.lib.vp8hip_arf_release.argtypes = [C.c_void_p]
        self._chk(self.lib.vp8hip_arf_release(self.h), "arf_release")

    def set_loop_filter_type(self, t: int):
        """vp8hip_set_loop_filter_type: 0 = the normal loop filter (default), 1 = the simple filter (RFC 6386 section 15.2),
        from the next loop_filter on.  The frame header's filter_type must say the same."""
        self.lib.vp8hip_set_loop_filter_type.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.vp8hip_set_loop_filter_type(self.h, int(t)), "set_loop_filter_type")

    def set_source_scaling(self, in_width: int, in_height: int, dst_width: int, dst_height: int, filter: int = SCALE_AREA):
        """vp8hip_set_source_scaling: current frames come in at in_width x in_height and are scaled down to dst on the device
        (0, 0, 0, 0 = off); self.src is the size of the planes to hand over, as with set_source_size"""
        self.lib.vp8hip_set_source_scaling.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        self._chk(self.lib.vp8hip_set_source_scaling(self.h, int(in_width), int(in_height), int(dst_width), int(dst_height), int(filter)),
                  "set_source_scaling")
        self.src = (int(in_width), int(in_height))

    def set_source_colour(self, matrix, range_="limited"):
        """vp8hip_set_source_colour: BGRA / RGBA frames are read with this matrix (a COLOUR_* number, or bt601 / bt709 and a range)"""
        self.lib.vp8hip_set_source_colour.argtypes = [C.c_void_p, C.c_int]
        m = source_colour(matrix, range_) if isinstance(matrix, str) else int(matrix)
        rc = self.lib.vp8hip_set_source_colour(self.h, m)
        if rc < 0:
            raise Vp8HipError(f"set_source_colour({m}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_source_format(self, fmt):
        """vp8hip_set_source_format: current frames come in this format (a FORMAT_* number or its name) and k_convert_b makes 8-bit
        I420 of them in front of the pack or scale launch; 0 = I420, nothing runs"""
        self.lib.vp8hip_set_source_format.argtypes = [C.c_void_p, C.c_int]
        fmt = source_format(fmt) if isinstance(fmt, str) else int(fmt)
        rc = self.lib.vp8hip_set_source_format(self.h, fmt)
        if rc != 0:
            raise Vp8HipError(f"set_source_format({fmt}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_source_transfer(self, transfer, peak: int = PEAK_DEFAULT):
        """vp8hip_set_source_transfer: P010 / I010 current frames carry this transfer (a TRANSFER_* number, or sdr / pq / hlg) graded
        for `peak` nits, and k_tonemap_b makes SDR I420 of them where k_convert_b would stand; sdr (0) = off"""
        self.lib.vp8hip_set_source_transfer.argtypes = [C.c_void_p, C.c_int, C.c_int]
        t = source_transfer(transfer) if isinstance(transfer, str) else int(transfer)
        rc = self.lib.vp8hip_set_source_transfer(self.h, t, int(peak))
        if rc != 0:
            raise Vp8HipError(f"set_source_transfer({t}, {peak}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_overlay(self, slot: int, pixels, x: int, y: int, opacity: int = 255, fmt=None, matrix: int = 0, lw=None, lh=None, pitch=None):
        """vp8hip_set_overlay_host / _device: the layer `pixels` (a uint8 array of shape (lh, lw, 4), or device memory with lw, lh and
        pitch; BGRA unless fmt says RGBA) is burnt into every frame taken in from now on, its top-left pixel at (x, y) of the picture"""
        fmt = FORMAT_BGRA if fmt is None else (source_format(fmt) if isinstance(fmt, str) else int(fmt))
        keep, ptr, lw, lh, pitch, dev = _layer_args(pixels, lw, lh, pitch)
        f = self.lib.vp8hip_set_overlay_device if dev else self.lib.vp8hip_set_overlay_host
        f.argtypes = _OVERLAY_SET_ARGS
        rc = f(self.h, int(slot), fmt, int(matrix), ptr, lw, lh, pitch, int(x), int(y), int(opacity))
        if rc != 0:
            raise Vp8HipError(f"vp8hip_set_overlay({slot}, {lw}x{lh} at ({x}, {y})): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_canvas(self, tiles, bg=(16, 128, 128)):
        """vp8hip_set_canvas: current frames are composed of these tiles (tiles_array's forms) over the background; [] ends it"""
        tiles = list(tiles)
        ta = tiles_array(tiles)
        self.lib.vp8hip_set_canvas.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4
        rc = self.lib.vp8hip_set_canvas(self.h, C.addressof(ta), len(tiles), int(bg[0]), int(bg[1]), int(bg[2]))
        if rc != 0:
            raise Vp8HipError(f"vp8hip_set_canvas({len(tiles)} tiles): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)
        self._canvas_tiles = len(tiles)

    def compose_current(self, frames, device: bool = False):
        """vp8hip_compose_current_host / _device: the current frame from the tiles' sources (tile_planes_array's forms; None = absent)"""
        pa, keep = tile_planes_array(frames, getattr(self, "_canvas_tiles", 0))
        f = self.lib.vp8hip_compose_current_device if device else self.lib.vp8hip_compose_current_host
        f.argtypes = [C.c_void_p, C.c_void_p]
        rc = f(self.h, C.addressof(pa))
        del keep
        if rc != 0:
            raise Vp8HipError(f"vp8hip_compose_current: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_overlay_placement(self, slot: int, x: int, y: int, opacity: int = 255):
        """vp8hip_set_overlay_placement: move or fade the slot's layer"""
        self.lib.vp8hip_set_overlay_placement.argtypes = [C.c_void_p] + [C.c_int] * 4
        rc = self.lib.vp8hip_set_overlay_placement(self.h, int(slot), int(x), int(y), int(opacity))
        if rc != 0:
            raise Vp8HipError(f"vp8hip_set_overlay_placement({slot}, {x}, {y}, {opacity}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def clear_overlay(self, slot: int = -1):
        """vp8hip_clear_overlay: the slot's layer, or with -1 every layer, is gone from the next frame on"""
        self.lib.vp8hip_clear_overlay.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.vp8hip_clear_overlay(self.h, int(slot))
        if rc != 0:
            raise Vp8HipError(f"vp8hip_clear_overlay({slot}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_denoise(self, level: int):
        """vp8hip_set_denoise: every frame that becomes current passes through the temporal denoiser (level 1-3; 0 = off); turning it
        on or changing the level restarts the history"""
        self.lib.vp8hip_set_denoise.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.vp8hip_set_denoise(self.h, int(level)), "set_denoise")

    def denoise_restart(self):
        """vp8hip_denoise_restart: the next frame taken in passes through and becomes the history"""
        self.lib.vp8hip_denoise_restart.argtypes = [C.c_void_p]
        self._chk(self.lib.vp8hip_denoise_restart(self.h), "denoise_restart")

    def denoise_result(self) -> "DenoiseStats":
        s = DenoiseStats()
        self.lib.vp8hip_denoise_result.argtypes = [C.c_void_p, C.POINTER(DenoiseStats)]
        self._chk(self.lib.vp8hip_denoise_result(self.h, C.byref(s)), "denoise_result")
        return s

    def set_source_window(self, pitch, x: int = 0, y: int = 0):
        """vp8hip_set_source_window: the three pointers of a current frame are the plane bases of a surface whose rows are pitch[p]
        bytes apart, and the frame is the window of the incoming size at (x, y); pitch None = off"""
        self.lib.vp8hip_set_source_window.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int]
        self._chk(self.lib.vp8hip_set_source_window(self.h, None if pitch is None else _pitch3(pitch), int(x), int(y)), "set_source_window")

    def set_source_orientation(self, turns: int, mirror: int = 0):
        """vp8hip_set_source_orientation: every frame that becomes current is turned by `turns` clockwise quarter turns behind a
        left-right flip (mirror); sizes keep describing the upright frame, the planes handed in are the raw one's"""
        self.lib.vp8hip_set_source_orientation.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(self.lib.vp8hip_set_source_orientation(self.h, int(turns), int(mirror)), "set_source_orientation")

    def set_deinterlace(self, mode, keep=0):
        """vp8hip_set_deinterlace: every frame that becomes current passes through the deinterlacer (mode off / field / adaptive or
        0, 1, 2; keep top / bottom or 0, 1); turning it on or changing mode or parity restarts the history"""
        self.lib.vp8hip_set_deinterlace.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(self.lib.vp8hip_set_deinterlace(self.h, deinterlace_mode(mode), deinterlace_field(keep)), "set_deinterlace")

    def deinterlace_restart(self):
        """vp8hip_deinterlace_restart: the next frame taken in has no history"""
        self.lib.vp8hip_deinterlace_restart.argtypes = [C.c_void_p]
        self._chk(self.lib.vp8hip_deinterlace_restart(self.h), "deinterlace_restart")

    def deinterlace_result(self) -> "DeinterlaceStats":
        s = DeinterlaceStats()
        self.lib.vp8hip_deinterlace_result.argtypes = [C.c_void_p, C.POINTER(DeinterlaceStats)]
        self._chk(self.lib.vp8hip_deinterlace_result(self.h, C.byref(s)), "deinterlace_result")
        return s

    def set_analysis(self, on: bool = True):
        """vp8hip_set_analysis: every frame taken in and every coding attempt is measured (include/vp8hip.h); on from off starts
        without a history"""
        self.lib.vp8hip_set_analysis.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.vp8hip_set_analysis(self.h, int(bool(on))), "set_analysis")

    def set_segment_mode(self, mode: int, strength: int = 0):
        """vp8hip_set_segment_mode: 0 off, 1 the caller's segment map, 2 variance-adaptive at strength 1..3 (include/vp8hip.h)"""
        self.lib.vp8hip_set_segment_mode.argtypes = [C.c_void_p, C.c_int, C.c_int]
        rc = self.lib.vp8hip_set_segment_mode(self.h, int(mode), int(strength))
        if rc != 0:
            raise Vp8HipError(f"set_segment_mode({mode}, {strength}): {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def segment_mode(self):
        """vp8hip_segment_mode: (mode, strength) in force"""
        a, b = C.c_int(), C.c_int()
        self.lib.vp8hip_segment_mode.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._chk(self.lib.vp8hip_segment_mode(self.h, C.byref(a), C.byref(b)), "segment_mode")
        return a.value, b.value

    def upload_segment_map(self, seg_map):
        """vp8hip_upload_segment_map: mode 1's map from host memory, one byte 0..3 per macroblock, in force until replaced"""
        m = np.ascontiguousarray(seg_map, np.uint8).reshape(-1)
        if m.size != self.mbs:
            raise ValueError(f"a segment map has one byte per macroblock: {self.mbs}, not {m.size}")
        self.lib.vp8hip_upload_segment_map.argtypes = [C.c_void_p, C.c_void_p]
        rc = self.lib.vp8hip_upload_segment_map(self.h, m.ctypes.data)
        if rc != 0:
            raise Vp8HipError(f"upload_segment_map: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def set_segment_map_device(self, d_map):
        """vp8hip_set_segment_map_device: the same from device memory (a pointer as vp8hip_device_alloc returns it)"""
        self.lib.vp8hip_set_segment_map_device.argtypes = [C.c_void_p, C.c_void_p]
        rc = self.lib.vp8hip_set_segment_map_device(self.h, _ptr(d_map))
        if rc != 0:
            raise Vp8HipError(f"set_segment_map_device: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)

    def download_segment_map(self, with_e: bool = False):
        """vp8hip_download_segment_map: the map in force for the current frame (and, with_e in mode 2, e of the rule): uint8 per macroblock"""
        m = np.zeros(self.mbs, np.uint8)
        e = np.zeros(self.mbs, np.uint8) if with_e else None
        self.lib.vp8hip_download_segment_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        rc = self.lib.vp8hip_download_segment_map(self.h, m.ctypes.data, e.ctypes.data if with_e else None)
        if rc != 0:
            raise Vp8HipError(f"download_segment_map: {self.lib.vp8hip_status_string(rc).decode()} ({rc})", rc)
        return (m, e) if with_e else m

    def analysis_restart(self):
        """vp8hip_analysis_restart: the next frame taken in has no history (have_prev = 0)"""
        self.lib.vp8hip_analysis_restart.argtypes = [C.c_void_p]
        self._chk(self.lib.vp8hip_analysis_restart(self.h), "analysis_restart")

    def analysis_result(self) -> "Analysis":
        a = Analysis()
        self.lib.vp8hip_analysis_result.argtypes = [C.c_void_p, C.POINTER(Analysis)]
        self._chk(self.lib.vp8hip_analysis_result(self.h, C.byref(a)), "analysis_result")
        return a

    def set_quality_stats(self, on: bool = True):
        """vp8hip_set_quality_stats: PSNR / SSIM of every filtered frame against its source, on the device (on from off: a new summary)"""
        self.lib.vp8hip_set_quality_stats.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.vp8hip_set_quality_stats(self.h, int(bool(on))), "set_quality_stats")

    def quality_result(self) -> "Quality":
        q = Quality()
        self.lib.vp8hip_quality_result.argtypes = [C.c_void_p, C.POINTER(Quality)]
        self._chk(self.lib.vp8hip_quality_result(self.h, C.byref(q)), "quality_result")
        return q

    def quality_summary(self) -> "QualitySummary":
        s = QualitySummary()
        self.lib.vp8hip_quality_summary.argtypes = [C.c_void_p, C.POINTER(QualitySummary)]
        self._chk(self.lib.vp8hip_quality_summary(self.h, C.byref(s)), "quality_summary")
        return s

    def debug_quality(self, src, rec) -> "Quality":
        """vp8hip_debug_quality (test tap): the quality kernel on caller planes; src, rec = (Y, U, V) uint8 arrays, chroma
        ((w + 1) // 2) x ((h + 1) // 2)"""
        src = [np.ascontiguousarray(p, np.uint8) for p in src]
        rec = [np.ascontiguousarray(p, np.uint8) for p in rec]
        h, w = src[0].shape
        P3, I3 = C.c_void_p * 3, C.c_int32 * 3
        q = Quality()
        self.lib.vp8hip_debug_quality.argtypes = [C.c_void_p, C.c_int, C.c_int, P3, I3, P3, I3, C.POINTER(Quality)]
        self._chk(self.lib.vp8hip_debug_quality(self.h, w, h, P3(*[p.ctypes.data for p in src]), I3(*[p.shape[1] for p in src]),
                                                P3(*[p.ctypes.data for p in rec]), I3(*[p.shape[1] for p in rec]), C.byref(q)),
                  "debug_quality")
        return q

    def filter_overlap(self, on: bool = True):
        """vp8hip_filter_overlap: one video coded frame after frame -- the loop filter on a stream of its own, the next frame's GOLDEN /
        ALTREF searches beside it, the search's coarse levels as one launch (what vp8drv_config.overlap_filter turns on)"""
        self.lib.vp8hip_filter_overlap.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.vp8hip_filter_overlap(self.h, int(bool(on))), "filter_overlap")

    def loopfilter_strength(self):
        """get_loopfilter_strength (vp8enc.cpp:96-127) of the current frame, computed on the device."""
        red, sh = C.c_int32(), C.c_int32()
        self._chk(self.lib.vp8hip_loopfilter_strength(self.h, C.byref(red), C.byref(sh)), "loopfilter_strength")
        return red.value, sh.value

    def auto_segments(self, is_key: bool, refqi, qi_min: int):
        """get_loopfilter_strength + prepare_segments_data on the device, asynchronous (no host round trip)."""
        q = (C.c_int32 * 4)(*[int(x) for x in refqi])
        self._chk(self.lib.vp8hip_auto_segments(self.h, int(bool(is_key)), q, int(qi_min)), "auto_segments")

    def get_segments(self):
        sd = np.zeros(44, np.int32)
        r, s = C.c_int32(), C.c_int32()
        self._chk(self.lib.vp8hip_get_segments(self.h, sd.ctypes.data, C.byref(r), C.byref(s)), "get_segments")
        return sd.reshape(4, 11), r.value, s.value

    def chroma_change(self):
        """scene_change's Udiff, Vdiff (vp8enc.cpp:265-282) between this and the previous current frame."""
        ud, vd = C.c_int32(), C.c_int32()
        self._chk(self.lib.vp8hip_chroma_change(self.h, C.byref(ud), C.byref(vd)), "chroma_change")
        return ud.value, vd.value

    def chroma_change_async(self):
        """the same scan enqueued behind the current frame's pack, nobody waiting (vp8hip_chroma_change_async); chroma_change_result() collects it"""
        self._chk(self.lib.vp8hip_chroma_change_async(self.h), "chroma_change_async")

    def chroma_change_result(self):
        ud, vd = C.c_int32(), C.c_int32()
        self._chk(self.lib.vp8hip_chroma_change_result(self.h, C.byref(ud), C.byref(vd)), "chroma_change_result")
        return ud.value, vd.value

    def count_probs(self, num_partitions: int):
        """count_probs + num_div_denom (CPU_kernels.cl:536-778): (probs[1056], partition-0 denominators[1056])."""
        probs, denom = np.zeros(1056, np.uint32), np.zeros(1056, np.uint32)
        self._chk(self.lib.vp8hip_count_probs(self.h, num_partitions, probs.ctypes.data, denom.ctypes.data), "count_probs")
        return probs, denom

    def encode_coefficients(self, probs, num_partitions: int, partition_step: int = 0):
        """encode_coefficients (CPU_kernels.cl:347-414) on the device: list of partition byte strings."""
        probs = np.ascontiguousarray(probs, np.uint32)
        step = partition_step or (self.mbs * 25 * 16 * 3 // num_partitions + 4096)
        out = np.zeros(num_partitions * step, np.uint8)
        sizes = np.zeros(num_partitions, np.int32)
        self._chk(self.lib.vp8hip_encode_coefficients(self.h, probs.ctypes.data, num_partitions, step, out.ctypes.data,
                                                      sizes.ctypes.data), "encode_coefficients")
        return [out[p * step: p * step + sizes[p]].copy() for p in range(num_partitions)]

    def debug_bool_code(self, strings, partition_step: int = 0, out=None):
        """vp8hip_debug_bool_code (test tap): the boolean coder on bool strings, one per partition, each a uint16 sequence of
        probability | bit << 8: list of partition byte strings.  out (uint8[len(strings) * partition_step]), where given, is the
        buffer the partitions are written into."""
        strings = [np.ascontiguousarray(b, np.uint16).reshape(-1) for b in strings]
        P = len(strings)
        n = np.array([len(b) for b in strings], np.uint32)
        flat = np.ascontiguousarray(np.concatenate(strings + [np.zeros(1, np.uint16)]))
        step = partition_step or (int(n.max(initial=0)) * 7 // 8 + 16)
        if out is None:
            out = np.zeros(P * step, np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= P * step
        sizes = np.zeros(max(P, 1), np.int32)
        self.lib.vp8hip_debug_bool_code.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self._chk(self.lib.vp8hip_debug_bool_code(self.h, flat.ctypes.data, n.ctypes.data, P, step, out.ctypes.data, sizes.ctypes.data),
                  "debug_bool_code")
        return [out[p * step: p * step + sizes[p]].tobytes() for p in range(P)]

    def download_last(self):
        W, H = self.W, self.H
        y, u, v = np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)
        self._chk(self.lib.vp8hip_download_last(self.h, y.ctypes.data, u.ctypes.data, v.ctypes.data), "download_last")
        return y, u, v

    def synchronize(self):
        self._chk(self.lib.vp8hip_synchronize(self.h), "synchronize")

    @property
    def stream(self) -> int:
        return int(self.lib.vp8hip_stream(self.h) or 0)

    def profile_enable(self, kernels):
        mask = 0
        for k in kernels:
            mask |= 1 << (K_NAMES.index(k) if isinstance(k, str) else int(k))
        self._chk(self.lib.vp8hip_profile_enable(self.h, mask), "profile_enable")

    def profile_read(self) -> dict:
        ms = (C.c_double * K_COUNT)()
        n = (C.c_int64 * K_COUNT)()
        self._chk(self.lib.vp8hip_profile_read(self.h, ms, n), "profile_read")
        return {K_NAMES[i]: (ms[i], n[i]) for i in range(K_COUNT) if n[i]}

    def profile_read_clock(self):
        """(ms, launches, shader clock GHz) of the loop filter by the kernel's own clock since the last call (vp8hip_profile_read_clock)"""
        ms, n, ghz = C.c_double(0), C.c_int64(0), C.c_double(0)
        self.lib.vp8hip_profile_read_clock.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        self._chk(self.lib.vp8hip_profile_read_clock(self.h, C.byref(ms), C.byref(n), C.byref(ghz)), "profile_read_clock")
        return ms.value, n.value, ghz.value

    def profile_read_search2_clock(self):
        """(ms, launches) of k_search2 by the kernel's own clock since the last call (vp8hip_profile_read_search2_clock)"""
        ms, n = C.c_double(0), C.c_int64(0)
        self.lib.vp8hip_profile_read_search2_clock.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        self._chk(self.lib.vp8hip_profile_read_search2_clock(self.h, C.byref(ms), C.byref(n)), "profile_read_search2_clock")
        return ms.value, n.value

    def profile_search2_clock(self, on: bool) -> None:
        self.lib.vp8hip_profile_search2_clock.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.lib.vp8hip_profile_search2_clock(self.h, int(on)), "profile_search2_clock")

    def profile_context_switches(self) -> int:
        """among the launches of the last profile_read_clock(): how many had the loop filter's last wave change its hardware slot
        (vp8hip_profile_context_switches; 0 unless the process holds more queues than the part's scheduler keeps resident)"""
        self.lib.vp8hip_profile_context_switches.argtypes = [C.c_void_p]
        self.lib.vp8hip_profile_context_switches.restype = C.c_int64
        return int(self.lib.vp8hip_profile_context_switches(self.h))

    def debug(self, what: int, ref: int = 0, level: int = 0) -> np.ndarray:
        if what in (DBG_NET1, DBG_NET2):
            a = np.zeros((self.b8, 2), np.int16)
        elif what == DBG_BDIFF:
            a = np.zeros(self.b8, np.int32)
        elif what == DBG_PYRAMID:
            a = np.zeros((self.H >> level, self.W >> level), np.uint8)
        elif what == DBG_THIRD_CONTEXT:
            a = np.zeros((self.mbs, 25), np.uint8)
        elif what == DBG_CURRENT_CHROMA:
            a = np.zeros((self.H // 2, self.W // 2), np.uint8)
        elif what == DBG_ARF_FRAME:      # ref 0..2: the filtered frame at the incoming size; 3..5: the ALTREF surface at the coded size
            w, h = (self.W, self.H) if ref >= 3 else self.incoming_size()
            a = np.zeros((h, w) if ref in (0, 3) else (h // 2, w // 2), np.uint8)
        elif what == DBG_REFRESH_FRAME:  # ref 0..2: Y, U, V at the coded size
            a = np.zeros((self.H, self.W) if ref == 0 else (self.H // 2, self.W // 2), np.uint8)
        else:
            a = np.zeros(self.mbs, np.int32)
        self._chk(self.lib.vp8hip_debug_download(self.h, what, ref, level, a.ctypes.data, a.nbytes), "debug_download")
        return a
