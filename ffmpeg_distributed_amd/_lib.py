"""ctypes binding of libmjgpu.so (C-ABI declared in include/mjgpu.h).

There is no fallback: if the HIP library is missing or cannot be loaded, every entry
point raises MjgError.  Build it with `python -m ffmpeg_distributed_amd.build`
(or `__graft_entry__.build()`).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MJG_LIBRARY", os.path.join(_PKG, "libmjgpu.so"))

MJG_OK = 0
MJG_E_INVALID = -1
MJG_E_HIP = -2
MJG_E_NOMEM = -3
MJG_E_CAPACITY = -4
MJG_E_STATE = -5

MJG_F_TIMING = 1
MJG_F_DEBUG_COEFS = 2
MJG_F_SWS_NO_BITEXACT = 4
MJG_F_COM_ITU601 = 8
MJG_F_HUFFMAN_OPTIMAL = 16
MJG_F_RST = 32
MJG_F_TIMING_DETAIL = 64
MJG_F_MERGE = 1024

# mjg_config.chroma_format
CHROMA_FORMATS = {"420": 0, "422": 1, "444": 2}

KERNEL_NAMES = ("scale", "encode", "scan_bits", "count_ff", "scan_ff", "write", "huff", "tail")
MJG_NUM_KERNELS = len(KERNEL_NAMES)

# Every symbol include/mjgpu.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "mjg_version", "mjg_last_error", "mjg_device_count", "mjg_device_numa_node", "mjg_open", "mjg_open_src", "mjg_open_crop", "mjg_open_pad", "mjg_open_orient", "mjg_close",
    "mjg_frame_bytes", "mjg_header", "mjg_submit", "mjg_sync", "mjg_fetch", "mjg_fetch_host",
    "mjg_output_device", "mjg_stream", "mjg_queue_depth", "mjg_ctx_queue_depth", "mjg_submit_segments", "mjg_max_segments", "mjg_host_alloc", "mjg_host_free",
    "mjg_kernel_times", "mjg_build_header", "mjg_sws_filter", "mjg_debug_coefs",
    "mjg_debug_planes", "mjg_debug_filter", "mjg_debug_huff_build", "mjg_debug_scale_path",
    "mjg_debug_encode_path", "mjg_debug_oriented", "mjg_debug_orient",
    "mjg_open_deint", "mjg_submit_halo", "mjg_debug_deint", "mjg_debug_deint_flags",
    "mjg_open_sharp", "mjg_debug_presharp", "mjg_debug_unsharp",
    "mjg_open_lut", "mjg_debug_lut", "mjg_debug_lut_in",
    "mjg_debug_tail",
    "mjg_open_cmat", "mjg_debug_cmat", "mjg_debug_cmat_out",
    "mjg_open_chain",
    "mjg_open_sheet", "mjg_frames_out", "mjg_debug_sheet", "mjg_debug_cell",
    "mjg_hist_open", "mjg_hist_frames", "mjg_hist_close",
    "mjg_open_denoise", "mjg_submit_cont", "mjg_debug_denoise", "mjg_debug_denoise_state",
)

# mjg_open_deint's `deint`
MJG_DEINT_YADIF = 1
MJG_DEINT_NOSPATIAL = 2
MJG_DEINT_BFF = 4


class MjgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mjgpu error {code}: {msg}")
        self.code = code


class MjgConfig(C.Structure):
    _fields_ = [
        ("src_w", C.c_int32), ("src_h", C.c_int32),
        ("dst_w", C.c_int32), ("dst_h", C.c_int32),
        ("in_full_range", C.c_int32), ("qscale", C.c_int32),
        ("sar_num", C.c_int32), ("sar_den", C.c_int32),
        ("max_batch", C.c_int32), ("flags", C.c_uint32),
        ("chroma_format", C.c_int32),
    ]


class MjgUnsharp(C.Structure):
    """mjg_unsharp: -vf unsharp's sizes and amounts, the amounts as int(amount * 65536.0)."""
    _fields_ = [("lx", C.c_int32), ("ly", C.c_int32), ("la", C.c_int32),
                ("cx", C.c_int32), ("cy", C.c_int32), ("ca", C.c_int32)]


class MjgLut(C.Structure):
    """mjg_lut: a 256-entry table per plane, out = t[in]."""
    _fields_ = [("y", C.c_uint8 * 256), ("u", C.c_uint8 * 256), ("v", C.c_uint8 * 256)]


class MjgTailJob(C.Structure):
    """mjg_tail_job: chunks for mjg_debug_tail (the stuffing tail alone; tests/test_gpu_tail.py)."""
    _fields_ = [("nframes", C.c_int32), ("nseg", C.c_int32), ("nchunks", C.c_int32),
                ("chunk_bits", C.POINTER(C.c_uint32)), ("words", C.POINTER(C.c_uint32)), ("fill", C.c_uint32),
                ("hdr", C.POINTER(C.c_uint8)), ("hdr_len", C.c_int32),
                ("dht", C.POINTER(C.c_uint8)), ("nval", C.POINTER(C.c_uint32)),
                ("dht_pos", C.c_int32), ("dht_end", C.c_int32), ("out_cap", C.c_uint64)]


MJG_TAIL_GUARD = 64
MJG_TAIL_MAX_SLOTS = 8192

class MjgCmatrix(C.Structure):
    """mjg_cmatrix: the six 16.16 coefficients c2..c7 of a colour matrix."""
    _fields_ = [("yu", C.c_int32), ("yv", C.c_int32), ("uu", C.c_int32), ("uv", C.c_int32), ("vu", C.c_int32),
                ("vv", C.c_int32)]


class MjgChain(C.Structure):
    """mjg_chain: what mjg_open_chain opens, the fields in the order the stages run (mjgpu.h)."""
    _fields_ = [("src_chroma_format", C.c_int32), ("deint", C.c_int32), ("orient", C.c_int32),
                ("cmat", C.POINTER(MjgCmatrix)), ("lut_in", C.POINTER(MjgLut)),
                ("has_crop", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32),
                ("crop_w", C.c_int32), ("crop_h", C.c_int32),
                ("lut_out", C.POINTER(MjgLut)), ("unsharp", C.POINTER(MjgUnsharp)),
                ("has_pad", C.c_int32), ("pad_x", C.c_int32), ("pad_y", C.c_int32),
                ("pad_w", C.c_int32), ("pad_h", C.c_int32)]


class MjgSheet(C.Structure):
    """mjg_sheet: -vf tile's contact sheet behind the chain (mjg_open_sheet); nb_frames 0 is cols * rows."""
    _fields_ = [("cols", C.c_int32), ("rows", C.c_int32), ("nb_frames", C.c_int32), ("margin", C.c_int32),
                ("padding", C.c_int32)]


class MjgDenoise(C.Structure):
    """mjg_denoise: -vf hqdn3d's four tables (luma / chroma spatial, luma / chroma temporal) behind the deinterlacer."""
    _fields_ = [("ls", C.c_int16 * 8192), ("cs", C.c_int16 * 8192), ("lt", C.c_int16 * 8192), ("ct", C.c_int16 * 8192)]


_lib = None
_lock = threading.Lock()


def load():
    """Load libmjgpu.so (raises MjgError if it is absent: no CPU fallback exists)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise MjgError(MJG_E_STATE, f"{LIB_PATH} not built; run python -m ffmpeg_distributed_amd.build")
        L = C.CDLL(LIB_PATH)
        vp, u8p, sz = C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t
        L.mjg_version.restype = C.c_int
        L.mjg_last_error.restype = C.c_char_p
        L.mjg_device_count.restype = C.c_int
        L.mjg_device_numa_node.argtypes = [C.c_int]
        L.mjg_device_numa_node.restype = C.c_int
        L.mjg_open.argtypes = [C.c_int, C.POINTER(MjgConfig), C.POINTER(vp)]
        if hasattr(L, "mjg_open_src"):  # absent from libraries built before 1.1 (A/B builds)
            L.mjg_open_src.argtypes = [C.c_int, C.POINTER(MjgConfig), C.c_int, C.POINTER(vp)]
        if hasattr(L, "mjg_open_crop"):  # absent from libraries built before 1.2 (A/B builds)
            L.mjg_open_crop.argtypes = [C.c_int, C.POINTER(MjgConfig)] + [C.c_int] * 5 + [C.POINTER(vp)]
        if hasattr(L, "mjg_open_pad"):  # absent from libraries built before 1.4 (A/B builds)
            L.mjg_open_pad.argtypes = [C.c_int, C.POINTER(MjgConfig)] + [C.c_int] * 9 + [C.POINTER(vp)]
        if hasattr(L, "mjg_open_orient"):  # absent from libraries built before the orientation stage (A/B builds)
            L.mjg_open_orient.argtypes = [C.c_int, C.POINTER(MjgConfig)] + [C.c_int] * 10 + [C.POINTER(vp)]
            L.mjg_debug_oriented.argtypes = [vp, C.c_int, u8p, sz]
            L.mjg_debug_oriented.restype = C.c_int
            L.mjg_debug_orient.argtypes = [vp]
            L.mjg_debug_orient.restype = C.c_int
        if hasattr(L, "mjg_open_deint"):  # absent from libraries built before the deinterlacer (A/B builds)
            L.mjg_open_deint.argtypes = [C.c_int, C.POINTER(MjgConfig)] + [C.c_int] * 11 + [C.POINTER(vp)]
            L.mjg_submit_halo.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
            L.mjg_submit_halo.restype = C.c_int
            L.mjg_debug_deint.argtypes = [vp, C.c_int, u8p, sz]
            L.mjg_debug_deint.restype = C.c_int
            L.mjg_debug_deint_flags.argtypes = [vp]
            L.mjg_debug_deint_flags.restype = C.c_int
        if hasattr(L, "mjg_open_sharp"):  # absent from libraries built before the sharpen (A/B builds)
            L.mjg_open_sharp.argtypes = ([C.c_int, C.POINTER(MjgConfig)] + [C.c_int] * 7 + [C.POINTER(MjgUnsharp)]
                                         + [C.c_int] * 4 + [C.POINTER(vp)])
            L.mjg_debug_presharp.argtypes = [vp, C.c_int, u8p, sz]
            L.mjg_debug_presharp.restype = C.c_int
            L.mjg_debug_unsharp.argtypes = [vp, C.POINTER(MjgUnsharp)]
            L.mjg_debug_unsharp.restype = C.c_int
        if hasattr(L, "mjg_open_lut"):  # absent from libraries built before the table stage (A/B builds)
            L.mjg_open_lut.argtypes = ([C.c_int, C.POINTER(MjgConfig)] + [C.c_int] * 7 + [C.POINTER(MjgLut)] * 2
                                       + [C.POINTER(MjgUnsharp)] + [C.c_int] * 4 + [C.POINTER(vp)])
            L.mjg_debug_lut.argtypes = [vp, C.c_int, C.POINTER(MjgLut)]
            L.mjg_debug_lut.restype = C.c_int
            L.mjg_debug_lut_in.argtypes = [vp, C.c_int, u8p, sz]
            L.mjg_debug_lut_in.restype = C.c_int
        if hasattr(L, "mjg_open_cmat"):  # absent from libraries built before the colour matrix (A/B builds)
            L.mjg_open_cmat.argtypes = ([C.c_int, C.POINTER(MjgConfig)] + [C.c_int] * 7 + [C.POINTER(MjgCmatrix)]
                                        + [C.POINTER(MjgLut)] * 2 + [C.POINTER(MjgUnsharp)] + [C.c_int] * 4
                                        + [C.POINTER(vp)])
            L.mjg_debug_cmat.argtypes = [vp, C.POINTER(MjgCmatrix)]
            L.mjg_debug_cmat.restype = C.c_int
            L.mjg_debug_cmat_out.argtypes = [vp, C.c_int, u8p, sz]
            L.mjg_debug_cmat_out.restype = C.c_int
        if hasattr(L, "mjg_open_chain"):  # absent from libraries built before the chain descriptor (A/B builds)
            L.mjg_open_chain.argtypes = [C.c_int, C.POINTER(MjgConfig), C.POINTER(MjgChain), C.POINTER(vp)]
            L.mjg_open_chain.restype = C.c_int
        if hasattr(L, "mjg_open_sheet"):  # absent from libraries built before the contact sheet (A/B builds)
            L.mjg_open_sheet.argtypes = [C.c_int, C.POINTER(MjgConfig), C.POINTER(MjgChain), C.POINTER(MjgSheet),
                                         C.POINTER(vp)]
            L.mjg_open_sheet.restype = C.c_int
            L.mjg_frames_out.argtypes = [vp, C.c_int]
            L.mjg_frames_out.restype = C.c_int
            L.mjg_debug_sheet.argtypes = [vp, C.POINTER(MjgSheet)]
            L.mjg_debug_sheet.restype = C.c_int
            L.mjg_debug_cell.argtypes = [vp, C.c_int, u8p, sz]
            L.mjg_debug_cell.restype = C.c_int
        if hasattr(L, "mjg_hist_open"):  # absent from libraries built before the histogram object (A/B builds)
            L.mjg_hist_open.argtypes = [C.c_int] * 5 + [C.POINTER(vp)]
            L.mjg_hist_open.restype = C.c_int
            L.mjg_hist_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
            L.mjg_hist_frames.restype = C.c_int
            L.mjg_hist_close.argtypes = [vp]
            L.mjg_hist_close.restype = None
        if hasattr(L, "mjg_open_denoise"):  # absent from libraries built before the denoiser (A/B builds)
            L.mjg_open_denoise.argtypes = [C.c_int, C.POINTER(MjgConfig), C.POINTER(MjgChain), C.POINTER(MjgSheet),
                                           C.POINTER(MjgDenoise), C.POINTER(vp)]
            L.mjg_open_denoise.restype = C.c_int
            L.mjg_submit_cont.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]
            L.mjg_submit_cont.restype = C.c_int
            L.mjg_debug_denoise.argtypes = [vp, C.c_int, u8p, sz]
            L.mjg_debug_denoise.restype = C.c_int
            L.mjg_debug_denoise_state.argtypes = [vp, C.POINTER(C.c_uint16), sz]
            L.mjg_debug_denoise_state.restype = C.c_int
        L.mjg_close.argtypes = [vp]
        L.mjg_close.restype = None
        L.mjg_frame_bytes.argtypes = [vp]
        L.mjg_frame_bytes.restype = sz
        L.mjg_header.argtypes = [vp, u8p, sz, C.POINTER(sz)]
        L.mjg_submit.argtypes = [vp, vp, C.c_int, C.c_int]
        L.mjg_sync.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mjg_fetch.argtypes = [vp, vp, sz]
        L.mjg_fetch_host.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
        L.mjg_output_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.mjg_stream.argtypes = [vp]
        L.mjg_stream.restype = vp
        if hasattr(L, "mjg_queue_depth"):  # absent from libraries built before r04 (A/B builds)
            L.mjg_queue_depth.argtypes = []
            L.mjg_queue_depth.restype = C.c_int
        if hasattr(L, "mjg_ctx_queue_depth"):  # absent from libraries built before r05 (A/B builds)
            L.mjg_ctx_queue_depth.argtypes = [vp]
            L.mjg_ctx_queue_depth.restype = C.c_int
        if hasattr(L, "mjg_submit_segments"):  # absent from libraries built before r04 (A/B builds)
            L.mjg_submit_segments.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int), C.c_int]
            L.mjg_max_segments.argtypes = []
            L.mjg_max_segments.restype = C.c_int
        L.mjg_host_alloc.argtypes = [sz, C.POINTER(vp)]
        L.mjg_host_free.argtypes = [vp]
        L.mjg_kernel_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]
        L.mjg_debug_coefs.argtypes = [vp, C.c_int, C.POINTER(C.c_int16), sz]
        L.mjg_debug_planes.argtypes = [vp, C.c_int, u8p, sz]
        L.mjg_debug_filter.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int16),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        if hasattr(L, "mjg_debug_huff_build"):  # absent from libraries built before r05 (A/B builds)
            L.mjg_debug_huff_build.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.c_int, u8p, C.POINTER(C.c_uint32)]
        if hasattr(L, "mjg_debug_tail"):  # absent from libraries built before the tail hook (A/B builds)
            L.mjg_debug_tail.argtypes = [C.c_int, C.POINTER(MjgTailJob), u8p, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
            L.mjg_debug_tail.restype = C.c_int
        if hasattr(L, "mjg_debug_scale_path"):  # absent from libraries built before 1.3 (A/B builds)
            L.mjg_debug_scale_path.argtypes = [vp, C.c_int]
            L.mjg_debug_scale_path.restype = C.c_int
        if hasattr(L, "mjg_debug_encode_path"):  # absent from libraries built before 1.5 (A/B builds)
            L.mjg_debug_encode_path.argtypes = [vp]
            L.mjg_debug_encode_path.restype = C.c_int
        L.mjg_build_header.argtypes = [C.POINTER(MjgConfig), u8p, sz, C.POINTER(sz)]
        L.mjg_sws_filter.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int16), sz, C.POINTER(C.c_int32),
                                                     C.POINTER(C.c_int)]
        # fail loudly on a stale / partial build (an A/B library from before r04/r05 named by
        # MJG_LIBRARY may lack mjg_queue_depth / mjg_ctx_queue_depth: the queue is then two
        # deep, no merging; and the multi-segment submit, which encoder.submit_segments guards)
        late = (("mjg_queue_depth", "mjg_ctx_queue_depth", "mjg_submit_segments", "mjg_max_segments",
                 "mjg_debug_huff_build", "mjg_open_src", "mjg_open_crop", "mjg_open_pad", "mjg_debug_scale_path",
                 "mjg_debug_encode_path", "mjg_open_orient", "mjg_debug_oriented", "mjg_debug_orient",
                 "mjg_open_deint", "mjg_submit_halo", "mjg_debug_deint", "mjg_debug_deint_flags",
                 "mjg_open_sharp", "mjg_debug_presharp", "mjg_debug_unsharp",
                 "mjg_open_lut", "mjg_debug_lut", "mjg_debug_lut_in", "mjg_debug_tail",
                 "mjg_open_cmat", "mjg_debug_cmat", "mjg_debug_cmat_out", "mjg_open_chain",
                 "mjg_open_sheet", "mjg_frames_out", "mjg_debug_sheet", "mjg_debug_cell",
                 "mjg_hist_open", "mjg_hist_frames", "mjg_hist_close",
                 "mjg_open_denoise", "mjg_submit_cont", "mjg_debug_denoise", "mjg_debug_denoise_state")
                if os.environ.get("MJG_LIBRARY") else ())
        for name in EXPORTS:
            if name not in late:
                getattr(L, name)
        _lib = L
        return L


def check(rc: int) -> int:
    if rc < 0:
        msg = load().mjg_last_error().decode(errors="replace")
        raise MjgError(rc, msg)
    return rc


def device_count() -> int:
    return check(load().mjg_device_count())


def device_numa_node(device: int) -> int:
    """NUMA node of the device (-1: unknown)."""
    return check(load().mjg_device_numa_node(int(device)))


def build_header(dst_w: int, dst_h: int, qscale: int, sar=(1, 1), com_itu601: bool = False,
                 chroma: str = "420", rst: bool = False) -> bytes:
    """The per-config JPEG header, computed on the host (no GPU needed)."""
    L = load()
    flags = (MJG_F_COM_ITU601 if com_itu601 else 0) | (MJG_F_RST if rst else 0)
    cfg = MjgConfig(dst_w, dst_h, dst_w, dst_h, 1, qscale, sar[0], sar[1], 1, flags,
                    CHROMA_FORMATS[str(chroma)])
    n = C.c_size_t()
    check(L.mjg_build_header(C.byref(cfg), None, 0, C.byref(n)))
    buf = (C.c_uint8 * n.value)()
    check(L.mjg_build_header(C.byref(cfg), buf, n.value, C.byref(n)))
    return bytes(buf)


def sws_filter(src_len, dst_len, one, align, bitexact=True, src_pos=128, dst_pos=128):
    """swscale bicubic filter table as the library generates it (host side)."""
    import numpy as np
    L = load()
    taps = C.c_int()
    check(L.mjg_sws_filter(src_len, dst_len, one, align, int(bitexact), src_pos, dst_pos, None, 0,
                           None, C.byref(taps)))
    coeff = np.zeros(dst_len * taps.value, np.int16)
    pos = np.zeros(dst_len, np.int32)
    check(L.mjg_sws_filter(src_len, dst_len, one, align, int(bitexact), src_pos, dst_pos,
                           coeff.ctypes.data_as(C.POINTER(C.c_int16)), coeff.size,
                           pos.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(taps)))
    return coeff.reshape(dst_len, taps.value), pos
