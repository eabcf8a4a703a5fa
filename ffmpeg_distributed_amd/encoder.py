"""GPU MJPEG encoder: the per-segment encode that the reference's worker runs
(`ffmpeg -f matroska -i pipe: <remote_args> -f matroska pipe:`,
ffmpeg_distributed.py:131-141), restricted to the profile
`[-vf [yadif,][vflip|transpose=N,...][crop=w:h:x:y,][scale=W:H:flags=bicubic][,unsharp[=lx:ly:la:cx:cy:ca]][,pad=W:H:x:y]] -c:v mjpeg -q:v N -dct int [-huffman default|optimal] -bitexact`
(and one `eq=...` in front of the scale or directly behind it)
(+ `-slices N` / `-thread_type slice` for the RST layout).

Host-side wrapper over libmjgpu.so; frames are packed planar YUV (yuv420p / yuvj420p by
default, 4:2:2 and 4:4:4 with `chroma=`), i.e. what `ffmpeg -f rawvideo -pix_fmt yuv4xxp`
writes.  `src_chroma=` names the input frames' format when `-pix_fmt` asks for another one
than the input's (`chroma=` is then the encoded format): the chroma planes are resampled on
the GPU as swscale does it.  `crop=(x, y, w, h)` makes a rectangle of the input frames the
encoder's (or the scaler's) input; the frames handed over stay whole.  `pad=(x, y, W, H)` puts
the picture (dst_w x dst_h) at (x, y) of a black W x H canvas, which is what gets encoded
(`-vf ...,pad=W:H:x:y`).  `orient=` (0..7: T | FX << 1 | FY << 2, what a run of hflip /
vflip / transpose filters composes to, profile.compose_orient; the profile itself parses vflip and transpose) turns or mirrors every plane of
the input frames on the GPU before anything else: the frames handed over stay the decoded ones,
src_w x src_h, while the crop, dst_w / dst_h and the pad refer to the oriented frame (src_h x
src_w under a transpose).  `deint=` (MJG_DEINT_YADIF | MJG_DEINT_NOSPATIAL | MJG_DEINT_BFF of
_lib: `-vf yadif` modes 0 / 2, tff / bff) deinterlaces the decoded frames on the GPU in front of
the orientation: every output frame is made from the frames before and after it, a submit (and
each segment of a submit_segments) is a whole sequence, and `submit(..., halo=)` hands over a
piece of a longer one with its neighbour frames.  `unsharp=` (lx, ly, la, cx, cy, ca: `-vf unsharp`
behind the scale and in front of the pad, the amounts as floats) sharpens or blurs the sws stage's
output planes on the GPU; the encoder then reads the sharpened planes.  `lut_in=` /
`lut_out=` ((3, 256) uint8, rows Y, U, V) map every sample through a table per plane on the GPU,
in front of the sws stage and directly behind it: `-vf eq=...` in front of the scale or
directly behind it, with profile.eq_tables.  `cmat=` (c2, ..., c7: six 16.16 ints) is a colour matrix
on whole frames behind the orientation and in front of `lut_in`: `-vf
colormatrix=SRC:DST` with profile.colormatrix_coefs.  `sheet=` (cols, rows, nb_frames, margin, padding:
`-vf tile` as the last filter) puts every nb_frames frames (0: cols * rows) on one contact sheet on the
GPU: dst_w x dst_h stay the cell, the JPEGs are the sheets (enc_w x enc_h), a submit of n frames yields
frames_out(n) of them, and every submit (every segment of a submit_segments) is a sequence of its own;
such an encoder opens through mjg_open_sheet.  `denoise=` ((4, 8192) int16, rows luma spatial, chroma
spatial, luma temporal, chroma temporal: `-vf hqdn3d` as the first filter or directly behind the yadif, with
profile.hqdn3d_tables) runs the denoiser's three scans on the GPU behind the deinterlacer; a submit is a
sequence of its own unless `submit(..., cont=True)` continues the one before, and such an encoder opens
through mjg_open_denoise.  An encoder with any of these opens as one
mjg_chain (include/mjgpu.h, which says what each stage does) through mjg_open_chain; one with none
through mjg_open / mjg_open_src.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from collections import deque
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import MjgConfig, MjgError, check


CHROMA_SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}


def chroma_size(w: int, h: int, chroma: str = "420"):
    """(width, height) of a chroma plane: ((w + hs) >> hs, (h + vs) >> vs)."""
    hs, vs = CHROMA_SHIFTS[str(chroma)]
    return (w + hs) >> hs, (h + vs) >> vs


def i420_frame_bytes(w: int, h: int, chroma: str = "420") -> int:
    cw, ch = chroma_size(w, h, chroma)
    return w * h + 2 * cw * ch


def split_i420(frame: np.ndarray, w: int, h: int, chroma: str = "420"):
    """Views (Y, U, V) of one packed planar frame (I420 unless `chroma` says otherwise)."""
    cw, ch = chroma_size(w, h, chroma)
    f = np.asarray(frame, dtype=np.uint8).reshape(-1)
    y = f[: w * h].reshape(h, w)
    u = f[w * h: w * h + cw * ch].reshape(ch, cw)
    v = f[w * h + cw * ch: w * h + 2 * cw * ch].reshape(ch, cw)
    return y, u, v


def pack_i420(y, u, v) -> np.ndarray:
    return np.concatenate([np.asarray(p, np.uint8).reshape(-1) for p in (y, u, v)])


class MjpegEncoder:
    """One encoder context on one GPU (owns a HIP stream and device buffers)."""

    def __init__(self, device: int, src_w: int, src_h: int, dst_w: Optional[int] = None,
                 dst_h: Optional[int] = None, full_range: bool = False, qscale: int = 5,
                 sar=(1, 1), max_batch: int = 16, timing: bool = False,
                 debug_coefs: bool = False, sws_bitexact: bool = True, com_itu601: bool = False,
                 huffman: str = "default", chroma: str = "420", rst: bool = False,
                 merge: bool = False, src_chroma: Optional[str] = None, crop=None, pad=None, orient: int = 0,
                 deint: Optional[int] = None, unsharp=None, lut_in=None, lut_out=None, cmat=None, sheet=None,
                 denoise=None):
        self._L = _lib.load()
        self.device = int(device)
        self.src_w, self.src_h = int(src_w), int(src_h)
        # crop: (x, y, w, h) in luma samples of the src_w x src_h frames, resolved as
        # profile.resolve_crop does (x, y multiples of the source's sub-sampling); the encoded
        # size defaults to the rectangle's.  None: whole frames
        self.crop = None if crop is None else tuple(int(v) for v in crop)
        if self.crop is not None and len(self.crop) != 4:
            raise ValueError(f"crop {crop!r}: (x, y, w, h)")
        # orient: T | FX << 1 | FY << 2, the first filter behind a deinterlacer; or_w x or_h is the oriented
        # frame, which the crop, the encoded size and the pad refer to
        self.orient = int(orient)
        self.or_w, self.or_h = (self.src_h, self.src_w) if self.orient & 1 else (self.src_w, self.src_h)
        in_w, in_h = (self.or_w, self.or_h) if self.crop is None else self.crop[2:]
        self.dst_w = int(dst_w if dst_w is not None else in_w)
        self.dst_h = int(dst_h if dst_h is not None else in_h)
        # pad: (x, y, W, H) in luma samples of the encoded frames, resolved as profile.resolve_pad
        # does: the picture (dst_w x dst_h, the sws stage's output) at (x, y) of a W x H canvas.
        # enc_w x enc_h is what the JPEGs hold: the canvas, or the picture without a pad
        self.pad = None if pad is None else tuple(int(v) for v in pad)
        if self.pad is not None and len(self.pad) != 4:
            raise ValueError(f"pad {pad!r}: (x, y, W, H)")
        self.enc_w, self.enc_h = (self.dst_w, self.dst_h) if self.pad is None else self.pad[2:]
        # sheet: (cols, rows, nb_frames, margin, padding), `-vf tile` behind everything else: dst_w x dst_h
        # is the cell, enc_w x enc_h the sheet, sheet_n the frames a sheet holds (1: no sheet, or the
        # trivial one, which the library opens as none).  None, the default, opens as without it
        self.sheet = None if sheet is None else tuple(int(v) for v in sheet)
        if self.sheet is not None and len(self.sheet) != 5:
            raise ValueError(f"sheet {sheet!r}: (cols, rows, nb_frames, margin, padding)")
        self.pic_w, self.pic_h = self.enc_w, self.enc_h  # the sws stage's output frame
        self.sheet_n = 1
        if self.sheet is not None:
            cols, rows, nb, margin, padding = self.sheet
            if cols * rows != 1 or margin != 0:
                self.sheet_n = nb or cols * rows
                self.enc_w = cols * self.dst_w + (cols - 1) * padding + 2 * margin
                self.enc_h = rows * self.dst_h + (rows - 1) * padding + 2 * margin
        self.max_batch = int(max_batch)
        flags = 0
        if timing == "detail":
            flags |= _lib.MJG_F_TIMING_DETAIL
        elif timing:
            flags |= _lib.MJG_F_TIMING
        if debug_coefs:
            flags |= _lib.MJG_F_DEBUG_COEFS
        if not sws_bitexact:
            flags |= _lib.MJG_F_SWS_NO_BITEXACT
        if com_itu601:
            flags |= _lib.MJG_F_COM_ITU601
        if huffman == "optimal":
            flags |= _lib.MJG_F_HUFFMAN_OPTIMAL
        elif huffman != "default":
            raise ValueError(f"huffman {huffman!r}")
        if rst:
            flags |= _lib.MJG_F_RST
        # library-side merging of single-segment device submits (MJG_F_MERGE, opt-in): a device
        # submit is held and launched with the next one, so its frames must stay unchanged until
        # its own sync; merge=False: every submit is a launch of its own, launched in submit()
        if merge:
            flags |= _lib.MJG_F_MERGE
        self.huffman = huffman
        self.chroma = str(chroma)
        if self.chroma not in _lib.CHROMA_FORMATS:
            raise ValueError(f"chroma {chroma!r}")
        # the input frames' format (None: the encoded one); frame_bytes follows it
        self.src_chroma = self.chroma if src_chroma is None else str(src_chroma)
        if self.src_chroma not in _lib.CHROMA_FORMATS:
            raise ValueError(f"src_chroma {src_chroma!r}")
        self.rst = bool(rst)
        sar = sar or (0, 0)
        cfg = MjgConfig(self.src_w, self.src_h, self.dst_w, self.dst_h, int(bool(full_range)),
                        int(qscale), int(sar[0]), int(sar[1]), self.max_batch, flags,
                        _lib.CHROMA_FORMATS[self.chroma])
        h = C.c_void_p()
        # deint: 0, or MJG_DEINT_YADIF | MJG_DEINT_NOSPATIAL | MJG_DEINT_BFF: yadif on the decoded
        # frames, in front of the orientation.  Every submit is then a whole sequence (or a piece of
        # one: submit(..., halo=)).  deint=0 and None, the default, are both no deinterlacer (chain
        # field 0); deint=0 opens through mjg_open_chain all the same
        self.deint = int(deint or 0)
        # unsharp: (lx, ly, la, cx, cy, ca), `-vf unsharp` between the sws stage and the pad; the
        # amounts are floats and become the filter's integers here, (int)(amount * 65536.0).  None,
        # the default, opens as without it
        self.unsharp = None
        if unsharp is not None:
            if len(unsharp) != 6:
                raise ValueError(f"unsharp {unsharp!r}: (lx, ly, la, cx, cy, ca)")
            lx, ly, la, cx, cy, ca = unsharp
            self.unsharp = (int(lx), int(ly), int(float(la) * 65536.0), int(cx), int(cy), int(float(ca) * 65536.0))
        # lut_in / lut_out: a (3, 256) uint8 array each, rows Y, U, V, out = t[in]: in front
        # of the sws stage on the frames behind the orientation, and on the sws stage's output picture
        # in front of the unsharp.  `-vf eq` is profile.eq_tables.  None, the default, opens as without them
        luts = []
        for name, t in (("lut_in", lut_in), ("lut_out", lut_out)):
            if t is not None:
                t = np.ascontiguousarray(t)
                if t.shape != (3, 256) or t.dtype != np.uint8:
                    raise ValueError(f"{name}: a (3, 256) uint8 array, not {t.shape} {t.dtype}")
            luts.append(t)
        self.lut_in, self.lut_out = luts
        # cmat: (c2, c3, c4, c5, c6, c7), the six 16.16 coefficients of a colour matrix on the frames behind
        # the orientation, in front of lut_in.  `-vf colormatrix` is
        # profile.colormatrix_coefs.  None, the default, opens as without it
        self.cmat = None
        if cmat is not None:
            if len(cmat) != 6:
                raise ValueError(f"cmat {cmat!r}: (c2, c3, c4, c5, c6, c7)")
            self.cmat = tuple(int(v) for v in cmat)
        # denoise: a (4, 8192) int16 array, the tables ls, cs, lt, ct of `-vf hqdn3d` (profile.hqdn3d_tables), behind
        # the deinterlacer and in front of the orientation.  None, the default, opens as without it
        self.denoise = None
        if denoise is not None:
            t = np.ascontiguousarray(denoise)
            if t.shape != (4, 8192) or t.dtype != np.int16:
                raise ValueError(f"denoise: a (4, 8192) int16 array, not {t.shape} {t.dtype}")
            self.denoise = t
        # one open: a chain with nothing in it through mjg_open / mjg_open_src (which every library
        # has, an older one named by MJG_LIBRARY too), everything else as one mjg_chain
        src_cf = _lib.CHROMA_FORMATS[self.src_chroma]
        if (self.crop is None and self.pad is None and not self.orient and deint is None and unsharp is None
                and lut_in is None and lut_out is None and self.cmat is None and self.sheet is None
                and self.denoise is None):
            if self.src_chroma == self.chroma:
                check(self._L.mjg_open(self.device, C.byref(cfg), C.byref(h)))
            elif not hasattr(self._L, "mjg_open_src"):
                raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_open_src")
            else:
                check(self._L.mjg_open_src(self.device, C.byref(cfg), src_cf, C.byref(h)))
        elif not hasattr(self._L, "mjg_open_chain"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_open_chain")
        elif self.sheet is not None and not hasattr(self._L, "mjg_open_sheet"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_open_sheet")
        elif self.denoise is not None and not hasattr(self._L, "mjg_open_denoise"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_open_denoise")
        else:
            chain = _lib.MjgChain(src_chroma_format=src_cf, deint=self.deint, orient=self.orient)
            if self.cmat is not None:
                chain.cmat = C.pointer(_lib.MjgCmatrix(*self.cmat))
            if self.lut_in is not None:
                chain.lut_in = C.pointer(_lib.MjgLut.from_buffer_copy(self.lut_in.tobytes()))
            if self.crop is not None:
                chain.has_crop = 1
                chain.crop_x, chain.crop_y, chain.crop_w, chain.crop_h = self.crop
            if self.lut_out is not None:
                chain.lut_out = C.pointer(_lib.MjgLut.from_buffer_copy(self.lut_out.tobytes()))
            if self.unsharp is not None:
                chain.unsharp = C.pointer(_lib.MjgUnsharp(*self.unsharp))
            if self.pad is not None:
                chain.has_pad = 1
                chain.pad_x, chain.pad_y, chain.pad_w, chain.pad_h = self.pad
            if self.denoise is not None:
                sheet_p = None if self.sheet is None else C.byref(_lib.MjgSheet(*self.sheet))
                check(self._L.mjg_open_denoise(self.device, C.byref(cfg), C.byref(chain), sheet_p,
                                               C.byref(_lib.MjgDenoise.from_buffer_copy(self.denoise.tobytes())),
                                               C.byref(h)))
            elif self.sheet is not None:
                check(self._L.mjg_open_sheet(self.device, C.byref(cfg), C.byref(chain),
                                             C.byref(_lib.MjgSheet(*self.sheet)), C.byref(h)))
            else:
                check(self._L.mjg_open_chain(self.device, C.byref(cfg), C.byref(chain), C.byref(h)))
        self._h = h
        self.frame_bytes = int(self._L.mjg_frame_bytes(h))
        self._queued = deque()        # (nframes, host buffer kept alive) per queued submit
        self._synced_since_submit = False
        self._last_sizes = np.zeros(0, np.uint64)
        # (under a sheet each of up to mjg_max_segments() segments may end with a partial sheet)
        self._sizes = np.zeros(self.max_batch + (1 if self.sheet_n == 1 else 4), np.uint64)

    # ------------------------------------------------------------------ basics
    def close(self):
        if getattr(self, "_h", None):
            self._L.mjg_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return int(self._L.mjg_stream(self._h) or 0)

    def header(self) -> bytes:
        n = C.c_size_t()
        check(self._L.mjg_header(self._h, None, 0, C.byref(n)))
        buf = (C.c_uint8 * n.value)()
        check(self._L.mjg_header(self._h, buf, n.value, C.byref(n)))
        return bytes(buf)

    def frames_out(self, n: int) -> int:
        """JPEGs a submit (or one segment of a submit_segments) of `n` frames yields: n without a
        sheet, ceil(n / sheet_n) with one (mjg_frames_out)."""
        if hasattr(self._L, "mjg_frames_out"):
            return int(self._L.mjg_frames_out(self._h, int(n)))
        return int(n)

    # ------------------------------------------------------------------ encode
    @property
    def pending(self) -> int:
        """Submits queued and not yet synced (at most `depth`)."""
        return len(self._queued)

    @property
    def depth(self) -> int:
        """Device-pointer submits (submit(device_ptr=...)) pending at most before one must be
        synced (mjg_ctx_queue_depth: two launches, of up to two merged submits each with
        merge=True)."""
        if hasattr(self._L, "mjg_ctx_queue_depth"):
            return int(self._L.mjg_ctx_queue_depth(self._h))
        return self.host_depth

    @property
    def host_depth(self) -> int:
        """Host-buffer submits and submit_segments() calls pending at most before one must be
        synced: each takes a launch of its own (mjg_queue_depth)."""
        return int(self._L.mjg_queue_depth()) if hasattr(self._L, "mjg_queue_depth") else 2

    def submit(self, frames=None, nframes: Optional[int] = None, device_ptr: Optional[int] = None, halo: int = 0,
               cont: bool = False):
        """Queue `nframes` packed frames: a host buffer (numpy / bytes) or a device pointer
        (`device_ptr`, e.g. torch_tensor.data_ptr() on this GPU, kept alive until its sync).
        Up to `host_depth` host submits may be queued (each one's k_encode runs beside the
        previous one's drain and tail kernels), up to `depth` device submits: with merge=True the
        library holds a device submit and launches it with the next one.
        `halo` (an encoder with `deint`; mjg_submit_halo): bit 1, the buffer starts with one extra
        frame that is only read, as the first encoded frame's previous one; bit 2, one such frame
        follows the last encoded one.  `nframes` counts the encoded frames only (a host buffer's
        default: its frames less the halo ones).
        `cont` (an encoder with `denoise`; mjg_submit_cont): the frames continue the sequence of the submit
        before, so the denoiser's time scan starts from the state that one left."""
        halo = int(halo)
        nhalo = (halo & 1) + ((halo >> 1) & 1)
        if halo and not hasattr(self._L, "mjg_submit_halo"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_submit_halo")

        if cont and not hasattr(self._L, "mjg_submit_cont"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_submit_cont")

        def call(ptr, n, dev):
            if cont:
                check(self._L.mjg_submit_cont(self._h, ptr, n, dev, halo, 1))
            elif halo:
                check(self._L.mjg_submit_halo(self._h, ptr, n, dev, halo))
            else:
                check(self._L.mjg_submit(self._h, ptr, n, dev))

        if device_ptr is not None:
            if nframes is None:
                raise ValueError("nframes is required with device_ptr")
            call(C.c_void_p(int(device_ptr)), int(nframes), 1)
            self._queued.append((self.frames_out(nframes), None))
            self._synced_since_submit = False
            return
        arr = np.ascontiguousarray(np.frombuffer(frames, dtype=np.uint8)
                                   if isinstance(frames, (bytes, bytearray, memoryview))
                                   else np.asarray(frames, dtype=np.uint8))
        if arr.size % self.frame_bytes:
            raise ValueError(f"buffer of {arr.size} bytes is not a whole number of "
                             f"{self.frame_bytes}-byte frames")
        n = arr.size // self.frame_bytes - nhalo if nframes is None else int(nframes)
        if halo and (n + nhalo) * self.frame_bytes > arr.size:
            raise ValueError(f"buffer of {arr.size} bytes holds fewer than {n} frames and {nhalo} halo frame(s)")
        call(C.c_void_p(arr.ctypes.data), n, 0)
        self._queued.append((self.frames_out(n), arr))  # the async H2D copy reads arr until its sync
        self._synced_since_submit = False

    def submit_segments(self, segments):
        """Queue several segments as ONE submit (mjg_submit_segments): `segments` is a list of
        (device_ptr, nframes) on this GPU, at most mjg_max_segments() of them, totalling at
        most max_batch frames.  One launch per kernel covers them
        all; sync() then returns the frames' sizes in segment order and fetch() their JPEGs,
        the same bytes as one submit() per segment.  Every segment's device buffer must stay
        alive until this submit is synced (the kernels read it in place)."""
        if not hasattr(self._L, "mjg_submit_segments"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_submit_segments")
        k = len(segments)
        ptrs = (C.c_void_p * max(k, 1))(*[C.c_void_p(int(p)) for p, _ in segments])
        ns = (C.c_int * max(k, 1))(*[int(n) for _, n in segments])
        check(self._L.mjg_submit_segments(self._h, ptrs, ns, k))
        self._queued.append((sum(self.frames_out(n) for _, n in segments), None))
        self._synced_since_submit = False

    @property
    def max_segments(self) -> int:
        """Most segments one submit_segments() may carry (mjg_max_segments)."""
        if not hasattr(self._L, "mjg_max_segments"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_max_segments")
        return int(self._L.mjg_max_segments())

    def sync(self) -> np.ndarray:
        """Complete the oldest queued submit; its per-frame JPEG sizes."""
        if not self._queued:
            return self._last_sizes.copy()
        total = C.c_uint64()
        check(self._L.mjg_sync(self._h, self._sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                               C.byref(total)))
        n, _ = self._queued.popleft()
        self._synced_since_submit = True
        self._last_sizes = self._sizes[:n].copy()
        return self._last_sizes.copy()

    def fetch(self) -> List[bytes]:
        """Packed JPEGs of the last synced submit (syncing the oldest queued one first when
        sync() was not called since the last submit)."""
        if self._queued and not self._synced_since_submit:
            self.sync()
        sizes = self._last_sizes
        data, n = C.c_void_p(), C.c_size_t()
        check(self._L.mjg_fetch_host(self._h, C.byref(data), C.byref(n)))  # page-locked copy
        if int(n.value) != int(sizes.sum()):
            raise MjgError(_lib.MJG_E_STATE, "fetch size mismatch")
        out, o = [], int(data.value or 0)
        for s in sizes:
            out.append(C.string_at(o, int(s)))
            o += int(s)
        return out

    def fetch_views(self) -> List[memoryview]:
        """fetch() with one copy: the packed JPEGs copied once out of the page-locked buffer,
        returned as memoryview slices (valid as long as the views are referenced)."""
        if self._queued and not self._synced_since_submit:
            self.sync()
        sizes = self._last_sizes
        data, n = C.c_void_p(), C.c_size_t()
        check(self._L.mjg_fetch_host(self._h, C.byref(data), C.byref(n)))
        if int(n.value) != int(sizes.sum()):
            raise MjgError(_lib.MJG_E_STATE, "fetch size mismatch")
        mv = memoryview(C.string_at(int(data.value or 0), int(n.value)) if n.value else b"")
        out, o = [], 0
        for s in sizes:
            out.append(mv[o:o + int(s)])
            o += int(s)
        return out

    def fetch_into(self, buf: "PinnedBuffer") -> List[memoryview]:
        """The packed JPEGs of the last synced submit DMA'd straight into `buf` (page-locked,
        PinnedBuffer: mjg_fetch's one-DMA path, no host copy), returned as memoryview slices of
        it; MjgError(MJG_E_CAPACITY) when `buf` is too small (see last_total)."""
        if self._queued and not self._synced_since_submit:
            self.sync()
        sizes = self._last_sizes
        total = int(sizes.sum())
        check(self._L.mjg_fetch(self._h, C.c_void_p(buf.ptr), int(buf.nbytes)))
        mv = memoryview(buf.array)[:total]
        out, o = [], 0
        for s in sizes:
            out.append(mv[o:o + int(s)])
            o += int(s)
        return out

    @property
    def last_total(self) -> int:
        """Packed bytes of the last synced submit."""
        return int(self._last_sizes.sum())

    def encode(self, frames) -> List[bytes]:
        """Encode host frames (any count; split into max_batch submits).  With `deint` the frames
        are one sequence: up to max_batch of them one submit, more of them halo submits that carry
        each piece's neighbour frames, which gives the same bytes.  With a `sheet` the frames are one
        sequence too: every submit but the last is a whole number of sheets."""
        arr = np.ascontiguousarray(np.asarray(frames, dtype=np.uint8)).reshape(-1)
        n = arr.size // self.frame_bytes
        out: List[bytes] = []
        step = self.max_batch // self.sheet_n * self.sheet_n
        if n > self.max_batch and not step:
            raise ValueError(f"a sheet of {self.sheet_n} frames does not fit max_batch {self.max_batch}")
        for i in range(0, n, step or self.max_batch):
            k = min(step or self.max_batch, n - i)
            cont = {"cont": True} if self.denoise is not None and i else {}  # one sequence through the denoiser too
            if self.deint and n > self.max_batch:
                lo, hi = (1 if i else 0), (1 if i + k < n else 0)
                self.submit(arr[(i - lo) * self.frame_bytes:(i + k + hi) * self.frame_bytes], k, halo=lo | hi << 1, **cont)
            elif cont:
                self.submit(arr[i * self.frame_bytes:(i + k) * self.frame_bytes], k, **cont)
            else:
                self.submit(arr[i * self.frame_bytes:(i + k) * self.frame_bytes], k)
            out.extend(self.fetch())
        return out

    def output_device(self):
        data, offs = C.c_void_p(), C.c_void_p()
        check(self._L.mjg_output_device(self._h, C.byref(data), C.byref(offs)))
        return int(data.value or 0), int(offs.value or 0)

    # ------------------------------------------------------------------ timing/debug
    def kernel_times(self, reset: bool = False):
        ms = (C.c_double * _lib.MJG_NUM_KERNELS)()
        n = C.c_int()
        check(self._L.mjg_kernel_times(self._h, ms, C.byref(n), int(bool(reset))))
        return {k: ms[i] for i, k in enumerate(_lib.KERNEL_NAMES)}, n.value

    def debug_coefs(self, frame: int = 0) -> np.ndarray:
        mcu_w = 8 if self.chroma == "444" else 16
        nmcu = ((self.enc_w + mcu_w - 1) // mcu_w) * ((self.enc_h + 15) // 16)
        out = np.zeros((nmcu * (8 if self.chroma == "422" else 6), 64), np.int16)
        check(self._L.mjg_debug_coefs(self._h, int(frame), out.ctypes.data_as(C.POINTER(C.c_int16)),
                                      out.shape[0]))
        return out

    def debug_planes(self, frame: int = 0) -> np.ndarray:
        """The encoder-input planes (after the scale / range / chroma stage) of a frame of the
        last synced submit: packed planar, enc_w x enc_h (dst size; the canvas under a pad), the
        encoded format `chroma`.  Under a `sheet`: sheet `frame` of that submit."""
        return self._debug_frame("mjg_debug_planes", i420_frame_bytes(self.enc_w, self.enc_h, self.chroma), frame)

    def debug_cell(self, frame: int = 0) -> np.ndarray:
        """k_tile_plane's input frame `frame` of the last synced submit, one of its input frames: the
        cell, packed planar, dst_w x dst_h in the encoded format (under a sharpen the sharpened planes).
        Only for an encoder opened with a `sheet` that is not the trivial one; debug_planes() then
        returns a sheet."""
        return self._debug_frame("mjg_debug_cell", i420_frame_bytes(self.pic_w, self.pic_h, self.chroma), frame)

    def debug_sheet(self):
        """(cols, rows, nb_frames, margin, padding) as the context holds them (nb_frames resolved), or
        None for a context without a sheet.  Host state only."""
        if not hasattr(self._L, "mjg_debug_sheet"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_debug_sheet")
        sh = _lib.MjgSheet()
        rc = self._L.mjg_debug_sheet(self._h, C.byref(sh))
        if rc < 0:
            check(rc)
        return (sh.cols, sh.rows, sh.nb_frames, sh.margin, sh.padding) if rc else None

    def _debug_frame(self, symbol: str, nbytes: int, frame: int) -> np.ndarray:
        """A frame readback of the library (mjg_debug_planes and its kin): `nbytes` bytes of frame
        `frame` of the last synced submit."""
        if not hasattr(self._L, symbol):
            raise MjgError(_lib.MJG_E_STATE, f"library lacks {symbol}")
        out = np.zeros(nbytes, np.uint8)
        check(getattr(self._L, symbol)(self._h, int(frame), out.ctypes.data_as(C.POINTER(C.c_uint8)), nbytes))
        return out

    def debug_oriented(self, frame: int = 0) -> np.ndarray:
        """The oriented frame (k_orient_plane's output) of a frame of the last synced submit:
        packed planar, or_w x or_h in the input format `src_chroma`, frame_bytes bytes.  Only for
        an encoder opened with a non-zero `orient`."""
        return self._debug_frame("mjg_debug_oriented", self.frame_bytes, frame)

    def debug_presharp(self, frame: int = 0) -> np.ndarray:
        """The sws stage's output (k_unsharp_plane's input) of a frame of the last synced submit, laid
        out as debug_planes(), which under a sharpen returns the sharpened planes.  Only for an
        encoder opened with an `unsharp` whose amounts are not both 0."""
        return self._debug_frame("mjg_debug_presharp", i420_frame_bytes(self.pic_w, self.pic_h, self.chroma), frame)

    def debug_unsharp(self):
        """(lx, ly, la, cx, cy, ca) as the context holds them (la, ca the filter's integers), or None
        for a context without a sharpen.  Host state only."""
        if not hasattr(self._L, "mjg_debug_unsharp"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_debug_unsharp")
        us = _lib.MjgUnsharp()
        rc = self._L.mjg_debug_unsharp(self._h, C.byref(us))
        if rc < 0:
            check(rc)
        return (us.lx, us.ly, us.la, us.cx, us.cy, us.ca) if rc else None

    def debug_lut_in(self, frame: int = 0) -> np.ndarray:
        """k_lut_plane's slot-"in" output of a frame of the last synced submit: a whole frame behind the
        orientation in the input format `src_chroma`, frame_bytes bytes.  Only for an encoder opened
        with a `lut_in` that is not three identity tables."""
        return self._debug_frame("mjg_debug_lut_in", self.frame_bytes, frame)

    def debug_cmat_out(self, frame: int = 0) -> np.ndarray:
        """k_cmat_frame's output of a frame of the last synced submit: a whole frame behind the
        orientation in the input format `src_chroma`, frame_bytes bytes (mapped by `lut_in`, which runs in
        place behind the stage, when there is one).  Only for an encoder opened with a `cmat` that is not
        the identity."""
        return self._debug_frame("mjg_debug_cmat_out", self.frame_bytes, frame)

    def debug_cmat(self):
        """The six coefficients the context holds, or None without a matrix (none given, or the
        identity).  Host state only."""
        if not hasattr(self._L, "mjg_debug_cmat"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_debug_cmat")
        m = _lib.MjgCmatrix()
        rc = self._L.mjg_debug_cmat(self._h, C.byref(m))
        if rc < 0:
            check(rc)
        return (m.yu, m.yv, m.uu, m.uv, m.vu, m.vv) if rc else None

    def debug_lut(self, slot: str = "in"):
        """The (3, 256) tables the context holds for slot "in" or "out", or None without (none given,
        or three identity tables).  Host state only."""
        if not hasattr(self._L, "mjg_debug_lut"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_debug_lut")
        t = _lib.MjgLut()
        rc = self._L.mjg_debug_lut(self._h, {"in": 0, "out": 1}[slot], C.byref(t))
        if rc < 0:
            check(rc)
        return np.frombuffer(bytes(t), np.uint8).reshape(3, 256).copy() if rc else None

    def debug_deint(self, frame: int = 0) -> np.ndarray:
        """The deinterlaced frame (k_yadif_plane's output) of a frame of the last synced submit:
        packed planar, src_w x src_h in the input format `src_chroma`, frame_bytes bytes.  Only for
        an encoder opened with a non-zero `deint`."""
        return self._debug_frame("mjg_debug_deint", self.frame_bytes, frame)

    def debug_denoise(self, frame: int = 0) -> np.ndarray:
        """The denoised frame (k_dn_time's output) of a frame of the last synced submit: packed planar,
        src_w x src_h in the input format `src_chroma`, frame_bytes bytes.  Only for an encoder opened with
        `denoise`."""
        return self._debug_frame("mjg_debug_denoise", self.frame_bytes, frame)

    def debug_denoise_state(self) -> np.ndarray:
        """The carried state of the denoiser's time scan: frame_bytes uint16 values, packed planar like a
        frame.  Syncs every queued submit first.  Only for an encoder opened with `denoise`."""
        if not hasattr(self._L, "mjg_debug_denoise_state"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_debug_denoise_state")
        while self._queued:
            self.sync()
        out = np.zeros(self.frame_bytes, np.uint16)
        check(self._L.mjg_debug_denoise_state(self._h, out.ctypes.data_as(C.POINTER(C.c_uint16)), out.size))
        return out

    def scale_path(self, plane: int) -> int:
        """Which kernel the sws stage runs for a plane (0 luma, 1 chroma): 0 none, 1 k_plane_copy,
        2 k_scale (one LDS tile), 3 k_scale_stream (past about 4:1, or MJG_SCALE_STREAM=1),
        4 k_pad_plane (the plane keeps its size under a pad)."""
        return check(self._L.mjg_debug_scale_path(self._h, int(plane)))

    def encode_path(self) -> int:
        """Which k_encode the context launches, as bits (mjg_debug_encode_path): 1 it reads the
        source frames in place (no sws stage), 2 the UA instantiation (a crop read in place whose
        geometry can fail the 8-byte alignment test)."""
        if not hasattr(self._L, "mjg_debug_encode_path"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_debug_encode_path")
        return check(self._L.mjg_debug_encode_path(self._h))

    def debug_filter(self, plane: int, direction: int):
        taps, ln = C.c_int(), C.c_int()
        check(self._L.mjg_debug_filter(self._h, plane, direction, None, None, C.byref(taps),
                                       C.byref(ln)))
        coeff = np.zeros((ln.value, taps.value), np.int16)
        pos = np.zeros(ln.value, np.int32)
        check(self._L.mjg_debug_filter(self._h, plane, direction,
                                       coeff.ctypes.data_as(C.POINTER(C.c_int16)),
                                       pos.ctypes.data_as(C.POINTER(C.c_int32)),
                                       C.byref(taps), C.byref(ln)))
        return coeff, pos


class PinnedBuffer:
    """Page-locked host buffer from mjg_host_alloc (fast async H2D for submits)."""

    def __init__(self, nbytes: int):
        self._L = _lib.load()
        p = C.c_void_p()
        check(self._L.mjg_host_alloc(int(nbytes), C.byref(p)))
        self.ptr = int(p.value)
        self.nbytes = int(nbytes)
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr))

    def free(self):
        if self.ptr:
            self._L.mjg_host_free(C.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class FrameHist:
    """Per-frame, per-plane histograms of decoded frames on one GPU (mjg_hist, k_frame_hist): what `-vf
    thumbnail` selects by (profile.thumbnail_pick).  An object of its own with its own stream and buffers,
    no encoder context: the worker's reader thread counts while the submit thread owns the encoder.  Frames
    are w x h, 8 bits, packed planar in `chroma`, frame_bytes apart.  No CPU fallback."""

    def __init__(self, device: int, w: int, h: int, chroma: str = "420", max_frames: int = 16):
        self._L = _lib.load()
        if not hasattr(self._L, "mjg_hist_open"):
            raise MjgError(_lib.MJG_E_STATE, "library lacks mjg_hist_open")
        if str(chroma) not in _lib.CHROMA_FORMATS:
            raise ValueError(f"chroma {chroma!r}")
        self.device, self.w, self.h, self.chroma = int(device), int(w), int(h), str(chroma)
        self.max_frames = int(max_frames)
        h_ = C.c_void_p()
        check(self._L.mjg_hist_open(self.device, self.w, self.h, _lib.CHROMA_FORMATS[self.chroma], self.max_frames,
                                    C.byref(h_)))
        self._h = h_
        self.frame_bytes = i420_frame_bytes(self.w, self.h, self.chroma)

    def count(self, frames=None, nframes: Optional[int] = None, device_ptr: Optional[int] = None) -> np.ndarray:
        """The (n, 768) uint32 histograms of n frames: row f, entry 256 p + v is the number of samples of
        value v in plane p (0 Y, 1 U, 2 V) of frame f.  `frames` is a host buffer (numpy / bytes; n defaults
        to its frames), or `device_ptr` the frames on this GPU with `nframes`.  Synchronous; every call counts
        from zero."""
        if device_ptr is not None:
            if nframes is None:
                raise ValueError("nframes is required with device_ptr")
            ptr, n, dev, keep = C.c_void_p(int(device_ptr)), int(nframes), 1, None
        else:
            keep = np.ascontiguousarray(np.frombuffer(frames, dtype=np.uint8)
                                        if isinstance(frames, (bytes, bytearray, memoryview))
                                        else np.asarray(frames, dtype=np.uint8))
            if keep.size % self.frame_bytes:
                raise ValueError(f"buffer of {keep.size} bytes is not a whole number of {self.frame_bytes}-byte frames")
            n = keep.size // self.frame_bytes if nframes is None else int(nframes)
            if n * self.frame_bytes > keep.size:
                raise ValueError(f"buffer of {keep.size} bytes holds fewer than {n} frames")
            ptr, dev = C.c_void_p(keep.ctypes.data), 0
        out = np.zeros((max(n, 0), 768), np.uint32)
        check(self._L.mjg_hist_frames(self._h, ptr, n, dev, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.mjg_hist_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["MjpegEncoder", "MjgError", "PinnedBuffer", "FrameHist", "i420_frame_bytes", "split_i420",
           "pack_i420"]
