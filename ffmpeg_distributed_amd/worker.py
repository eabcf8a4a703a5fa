"""The `gpu:N` segment worker: the process the dispatcher starts in place of
`nice -n10 ionice -c3 ffmpeg -f matroska -i pipe: <remote_args> -f matroska pipe:`
(ffmpeg_distributed.py:131-141), with the same contract: one segment on stdin, the
encoded Matroska segment on stdout, ffmpeg-style `Duration:` / `frame= ... speed=Nx`
lines on stderr (parsed at ffmpeg_distributed.py:39-40,62-73), exit code 0 on success.

    python -m ffmpeg_distributed_amd.worker --device N <remote_args...>

remote_args inside the GPU profile (profile.parse) are encoded on GPU N; anything else
runs the reference command line with the real ffmpeg as a child (same output, CPU).

Input: Matroska with V_UNCOMPRESSED I420/Y42B/444P video and YUV4MPEG2 are read natively;
any other codec (the splitter's lossless x264 segments, fd.py:198-202) is decoded by an
`ffmpeg ... -f yuv4mpegpipe` child feeding this process (SURVEY §8f "splitter decode").
A -pix_fmt with fewer chroma samples than the input's (444 -> 422, 444 -> 420, 422 -> 420) is
converted on the GPU (`resample_plan`); one with more needs an up-sampling nobody asks for:
the decoded frames then go to the real ffmpeg as y4m (`ffmpeg_fallthrough`).
A `-vf crop=...` is resolved against the segment's input (profile.resolve_crop) and read by
the GPU as a rectangle of the whole frames; a request that does not fit the input fails as
ffmpeg does (one line on stderr, exit code 1).
A `pad=...` at the end of the graph is resolved against the picture it follows (the scale's
output, the crop's rectangle or the input: profile.resolve_pad) and encoded as a black canvas
around it; a picture whose size is no multiple of the format's chroma sub-sampling, and a pad
with a -pix_fmt conversion but no scale in front of it, go to the real ffmpeg.
A leading run of `vflip` / `transpose` filters (profile.Profile.orient) is applied by the
GPU to the whole decoded frames before anything else; the crop, the scale, the SAR and the pad
then start from the oriented size (height x width under a transpose, the SAR inverted as
vf_transpose does).  A transpose of a 4:2:2 input goes to the real ffmpeg, which converts the
format first.
A `yadif` as the very first filter (profile.Profile.deint) is run by the GPU on the decoded
frames before all of that.  Its parity is the one given, or with `auto` the input's field order
(container.StreamInfo.field; resolve_deint): a stream of mixed or unknown order, and one with a
plane below 3 x 3, go to the real ffmpeg, which is told the source's field order in the y4m header.
Every output frame reads the frame before and the frame after it, so with a deinterlacer the
page-locked batches hold two more frames, the reader keeps one frame of look-ahead and copies the
previous batch's last frame and its look-ahead frame to the head of the next (deint_step is the
schedule; Pipeline.read_deint follows it), and each batch is a halo submit (encoder.submit(halo=)).
An `unsharp` behind the crop and the scale (profile.Profile.unsharp) is run by the GPU on the sws
stage's output.  Without a scale in the graph FFmpeg sharpens the decoded frames and converts them
afterwards, so a tv-range or to-be-converted input then goes to the real ffmpeg
(unsharp_fallthrough_reason).
One `eq` (profile.Profile.eq) becomes three byte tables (profile.eq_tables) that the GPU applies in
front of the sws stage (slot "in": the decoded samples, before any conversion) or on its output (slot
"out": directly behind the scale); eq_fallthrough_reason names the inputs that still go to the real
ffmpeg.
One `colormatrix=SRC:DST` (profile.Profile.colormatrix) becomes six 16.16 coefficients
(profile.colormatrix_coefs) that the GPU applies to the decoded frames behind the yadif and the
orientation, in front of everything else; cmat_fallthrough_reason names the inputs that still go to
the real ffmpeg.
A `tile` as the last filter (profile.SheetProfile.tile) is run by the GPU behind everything else: every
nb_frames frames become one sheet, a batch is a whole number of sheets (sheet_batch), and the muxer and
the progress lines run at the input rate / nb_frames; tile_fallthrough_reason names the inputs that still
go to the real ffmpeg.  A `framestep=N` as the first filter never reaches the GPU: the reader keeps
frame i of the segment when i % N == 0 and passes over the rest (Source.skip, which reads nothing of
them from a regular file), and the output runs at the input rate / N.  Such a graph resolves to a
SheetPlan; every other graph to the SegmentPlan it always did.
A `thumbnail=N` in front of such a graph (profile.ThumbProfile; a ThumbPlan) never reaches the encoder either:
the reader collects every N frames (behind the framestep) in a page-locked group store, has the GPU count
their histograms as they arrive (encoder.FrameHist, an object with a stream of its own, so the reader thread
uses it while the submit thread owns the encoder), selects one with profile.thumbnail_pick when the group
closes or the input ends, and copies that frame into the batch (Pipeline.read_thumb).  The submit side sees a
plain frame sequence, and the output runs at the rate it has without the thumbnail, as the filter leaves its
link's frame rate alone; thumbnail_fallthrough_reason names the inputs that still go to the real ffmpeg.
A `hqdn3d` as the first filter or directly behind the yadif (profile.DenoiseProfile) is run by the GPU behind the
deinterlacer: three scans with the filter's four tables.  Its time scan runs through the whole
segment, so a segment's first batch is a plain submit and every later one continues it (encoder.submit(cont=True),
together with the halo a deinterlaced batch has); denoise_fallthrough_reason names the inputs that still go to
the real ffmpeg.
All of this is resolved against the segment's input by plan_segment, a pure function, before run()
binds to the GPU's NUMA node: a SegmentPlan, a Fallthrough (the real ffmpeg) or a CropError / PadError.
run() is then a sequence: Context.acquire opens the encoder and its page-locked buffers (or takes the serve
cache's), a Pipeline (reader thread, submit / drain loop, muxer thread; no GPU import of its own, so it runs
with stand-ins) takes the segment through them, Pipeline.stop ends the threads and closes the source, and
Context.settle keeps, frees or leaks what the context holds.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import queue
import subprocess
import sys
import threading
import time
from fractions import Fraction
from dataclasses import dataclass
from typing import List, Optional

from . import container, profile

DECODE_ARGV = ["ffmpeg", "-v", "error", "-f", "matroska", "-i", "pipe:", "-map", "0:v:0",
               "-f", "yuv4mpegpipe", "-strict", "-1", "pipe:"]
# frames per submit: MJG_WORKER_BATCH, or as many as fit BATCH_BYTES of input (at most 32).
# The three page-locked batch buffers are allocated per segment process, and pinning is a
# large part of its start-up: 4K batches of 32 frames pinned 1.2 GB, of 8 frames 0.3 GB.
BATCH = int(os.environ.get("MJG_WORKER_BATCH", "0"))
BATCH_BYTES = int(os.environ.get("MJG_WORKER_BATCH_BYTES", str(96 << 20)))
# serve mode (and the resident encoder) pins its batches once for many segments.  128 MiB (10 4K
# frames) measured ahead of 256 MiB end to end: a segment's first H2D starts after a smaller
# first read and its last batch drains sooner (per-segment process 3,490-3,649 vs 3,304-3,392 4K
# fps, two clients 3,755-3,790 vs 3,289-3,466; profiles/r05/e2e_batch_ab.txt); every batch holds
# at least 4 frames (an 8K batch of 1 frame leaves the GPU waiting on every sync)
SERVE_BATCH_BYTES = int(os.environ.get("MJG_SERVE_BATCH_BYTES", str(128 << 20)))
MIN_BATCH_FRAMES = 4


def batch_frames(opts, frame_bytes: int) -> int:
    """Frames per page-locked batch: MJG_WORKER_BATCH if set, else what batch_bytes holds,
    clamped to [MIN_BATCH_FRAMES, 32]."""
    return opts.batch or max(MIN_BATCH_FRAMES, min(32, opts.batch_bytes // max(frame_bytes, 1)))
# FFmpeg builds differ in the pix_fmt their CLI hands the mjpeg encoder for yuv420p input
# (yuvj420p: no COM; yuv420p + full range: COM "CS=ITU601"); default = yuvj420p.
COM_ITU601 = os.environ.get("MJG_COM_ITU601", "0") == "1"


def reference_argv(args: List[str]) -> List[str]:
    """The command the reference runs for one segment (fd.py:133-135, without nice/ionice)."""
    return ["ffmpeg", "-f", "matroska", "-i", "pipe:", *args, "-f", "matroska", "pipe:"]


def _hms(t: float) -> str:
    h, r = divmod(max(t, 0.0), 3600)
    m, s = divmod(r, 60)
    return f"{int(h):02d}:{int(m):02d}:{s:05.2f}"


class Progress:
    """ffmpeg-shaped stderr lines so FFMPEGProc's progress regex follows the GPU worker."""

    def __init__(self, err, fps: Fraction, qscale: int):
        self.err, self.fps, self.q = err, fps, qscale
        self.t0 = time.monotonic()
        self.last = 0.0
        self.bytes = 0

    def duration(self, seconds: Optional[float]):
        if seconds is not None:
            self.err.write(f"  Duration: {_hms(seconds)}, start: 0.000000, bitrate: N/A\n")
            self.err.flush()

    def update(self, frames: int, nbytes: int, final: bool = False):
        self.bytes += nbytes
        now = time.monotonic()
        if not final and now - self.last < 0.5:
            return
        self.last = now
        el = max(now - self.t0, 1e-6)
        t = float(frames / self.fps) if self.fps else 0.0
        kb = self.bytes // 1024
        br = (self.bytes * 8 / t / 1000) if t > 0 else 0.0
        self.err.write(f"frame={frames:5d} fps={int(frames / el):3d} q={self.q:.1f} "
                       f"size={kb:8d}KiB time={_hms(t)} bitrate={br:7.1f}kbits/s "
                       f"speed={t / el:.3f}x\n")
        self.err.flush()


# 8: 84 GB/s from the page cache for a 4K segment against 61 GB/s with 4 (r05, bench e2e trace)
READ_THREADS = int(os.environ.get("MJG_READ_THREADS", "8"))
# page-locked batch buffers per encoder context (MJG_WORKER_BUFFERS): the reader fills one
# while two submits are queued and a third waits for the sync
NBUF = max(3, int(os.environ.get("MJG_WORKER_BUFFERS", "4")))
NOUT = 6  # page-locked output buffers: one being filled, up to four queued to the muxer, one in its write
# MJG_WORKER_TRACE=1: one `mjg-trace:` stderr line per segment with where its time went
# (reader, submit, sync, fetch, mux) and the process's CPU / NUMA placement.
TRACE = os.environ.get("MJG_WORKER_TRACE", "0") == "1"


@dataclass(frozen=True)
class Options:
    """Per-segment settings.  A worker process takes them from its environment (the module
    values above); the resident encoder (resident.py) takes them from each request, i.e. from
    the environment of the mjg_client process that sent the segment."""
    batch: int = 0                  # MJG_WORKER_BATCH: frames per submit (0: by bytes)
    batch_bytes: int = 96 << 20     # MJG_WORKER_BATCH_BYTES
    com_itu601: bool = False        # MJG_COM_ITU601
    read_threads: int = 8           # MJG_READ_THREADS
    trace: bool = False             # MJG_WORKER_TRACE
    client_t0: float = 0.0          # trace: the mjg_client's start (MJG_CLIENT_T0, monotonic ns)
    t_accept: float = 0.0           # trace: when the resident encoder accepted the request

    @classmethod
    def from_env(cls, env, batch_bytes: Optional[int] = None, t_accept: float = 0.0) -> "Options":
        """From NAME=VALUE settings (absent names take the defaults above)."""
        try:
            client_t0 = int(env.get("MJG_CLIENT_T0", "0") or 0) / 1e9
        except ValueError:
            client_t0 = 0.0
        return cls(batch=int(env.get("MJG_WORKER_BATCH", "0") or 0),
                   batch_bytes=int(env.get("MJG_WORKER_BATCH_BYTES", "0") or 0) or batch_bytes or (96 << 20),
                   com_itu601=env.get("MJG_COM_ITU601", "0") == "1",
                   read_threads=max(1, int(env.get("MJG_READ_THREADS", "8") or 8)),
                   trace=env.get("MJG_WORKER_TRACE", "0") == "1", client_t0=client_t0, t_accept=t_accept)


def process_options(batch_bytes: Optional[int] = None) -> Options:
    """This process's settings (the module values, read from its environment at import)."""
    return Options(batch=BATCH, batch_bytes=batch_bytes or BATCH_BYTES, com_itu601=COM_ITU601,
                   read_threads=READ_THREADS, trace=TRACE)
# Bind the worker to its GPU's NUMA node (CPUs, and preferred memory for its page-locked
# batches), see bind_numa.  MJG_NUMA_BIND=0 leaves placement to the scheduler.
NUMA_BIND = os.environ.get("MJG_NUMA_BIND", "1") == "1"
_bound_node: Optional[int] = None
_gpu_node = -1


def bind_numa(device: int) -> int:
    """Run the calling thread, and the threads it starts from here on, on the CPUs of
    `device`'s NUMA node and prefer that node for their memory: the segment's positional
    reads copy page-cache pages into page-locked batches that the GPU then reads over PCIe,
    and both the copy and the DMA cross the socket interconnect when the process sits on the
    other node.  Affinity and memory policy are per thread on Linux: threads started later
    (reader, pread pool) inherit them, threads that already exist (the HIP runtime's, which
    the NUMA query itself starts) do not.  When the node's CPUs are not among the allowed
    ones nothing changes (no remote memory preference for a thread that cannot run there).
    Returns the node (-1: unknown / not bound)."""
    global _bound_node, _gpu_node
    if _bound_node is not None:
        return _bound_node
    _bound_node = -1
    from . import _lib
    try:
        node = _gpu_node = _lib.device_numa_node(device)
    except Exception:
        return -1
    if node < 0 or not NUMA_BIND:
        return -1
    try:
        with open(f"/sys/devices/system/node/node{node}/cpulist") as f:
            cpus = _cpulist(f.read().strip()) & os.sched_getaffinity(0)
        if not cpus:
            return -1
        os.sched_setaffinity(0, cpus)
    except OSError:
        return -1
    _prefer_node(node)
    _bound_node = node
    return node


def _prefer_node(node: int) -> None:
    """set_mempolicy(MPOL_PREFERRED, {node}) for the calling thread (x86-64 Linux)."""
    import ctypes
    import platform
    if platform.machine() != "x86_64" or node >= 64:
        return
    try:
        libc = ctypes.CDLL(None, use_errno=True)
        mask = ctypes.c_ulong(1 << node)
        libc.syscall(238, 1, ctypes.byref(mask), ctypes.c_ulong(64))  # SYS_set_mempolicy
    except (OSError, AttributeError):
        pass


def placement() -> str:
    """CPUs this process may run on, the NUMA nodes they span and the cgroup's CPU
    throttling counters (tracing only; Linux /proc and /sys, best effort)."""
    out = []
    try:
        cpus = sorted(os.sched_getaffinity(0))
        out.append(f"cpus={len(cpus)}")
        nodes = {}
        base = "/sys/devices/system/node"
        for d in os.listdir(base):
            if d.startswith("node") and d[4:].isdigit():
                with open(f"{base}/{d}/cpulist") as f:
                    lst = _cpulist(f.read().strip())
                k = len(lst & set(cpus))
                if k:
                    nodes[int(d[4:])] = k
        out.append("nodes=" + ",".join(f"{n}:{k}" for n, k in sorted(nodes.items())))
    except OSError:
        pass
    try:
        with open("/sys/fs/cgroup/cpu.stat") as f:
            st = dict(line.split() for line in f if line.strip())
        out.append(f"throttled={st.get('nr_throttled', '?')}/{st.get('nr_periods', '?')}"
                   f" throttled_ms={int(st.get('throttled_usec', 0)) // 1000}")
    except (OSError, ValueError):
        pass
    out.append(f"cpu_now={_current_cpu()} gpu_node={_gpu_node} bound={_bound_node}")
    return " ".join(out)


def _cpulist(text: str) -> set:
    cpus = set()
    for part in text.split(","):
        if "-" in part:
            a, b = part.split("-")
            cpus.update(range(int(a), int(b) + 1))
        elif part:
            cpus.add(int(part))
    return cpus


def _current_cpu() -> int:
    try:
        with open("/proc/thread-self/stat") as f:
            return int(f.read().rsplit(")", 1)[1].split()[36])
    except (OSError, ValueError, IndexError):
        return -1


def _regular_file_fd(f) -> Optional[int]:
    """The descriptor of a seekable regular file behind `f`, else None (pipes, sockets,
    in-memory streams read sequentially)."""
    import stat
    try:
        fd = f.fileno()
        if stat.S_ISREG(os.fstat(fd).st_mode) and f.seekable():
            return fd
    except (AttributeError, OSError, ValueError):
        pass
    return None


def _pread_exact(fd: int, dest, off: int) -> None:
    got = 0
    while got < len(dest):
        k = os.preadv(fd, [dest[got:]], off + got)
        if k <= 0:
            raise ValueError(f"segment file ends inside a frame at byte {off + got}")
        got += k


class Source:
    """Packed planar frames from stdin: .info (StreamInfo), .read_into(buf, n) -> count."""

    def __init__(self, raw, read_threads: int = READ_THREADS, stderr=None):
        self.child = None
        self.feeder = None
        head = raw.read(4)
        if head.startswith(b"YUV4"):
            self._y4m(container.Y4MReader(raw, head))
            self.duration = None
            return
        if head != b"\x1a\x45\xdf\xa3":
            raise ValueError("input is neither Matroska nor YUV4MPEG2")
        mkv = container.MkvReader(raw, head, record=True)
        tr = next((t for t in mkv.tracks if t.codec.startswith("V_")), None)
        if tr is None:
            raise ValueError("no video track in the segment")
        self.duration = mkv.duration_seconds()
        info = mkv.info(tr.number)
        if tr.codec == "V_UNCOMPRESSED" and tr.colour_space in container.MKV_FOURCC_CHROMA:
            self.info = info
            mkv.stop_recording()
            self._mkv, self._track = mkv, tr.number
            self.read_into = self._read_mkv
            self._fd = _regular_file_fd(raw)
            if self._fd is not None:  # a file (the dispatcher's segment): parallel positional reads
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(read_threads)
                self.read_into = self._read_mkv_pread
            return
        # any other codec: ffmpeg decodes, we read its y4m
        self.child = subprocess.Popen(DECODE_ARGV, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                      stderr=_fd_or_none(stderr))
        self.feeder = threading.Thread(target=self._feed, args=(mkv, raw), daemon=True)
        self.feeder.start()
        self._y4m(container.Y4MReader(self.child.stdout))

    def _feed(self, mkv, raw):
        # the decoder gets the exact bytes we consumed: replay them, then the rest
        try:
            self.child.stdin.write(mkv.replay_bytes())
            while True:
                b = raw.read(1 << 20)
                if not b:
                    break
                self.child.stdin.write(b)
        except BrokenPipeError:
            pass
        finally:
            try:
                self.child.stdin.close()
            except BrokenPipeError:
                pass

    def _y4m(self, rd):
        self.info = rd.info
        self.read_into = rd.read_into

    def skip(self, n: int) -> int:
        """Pass over the next n frames (-vf framestep: the frames the reader does not keep); returns how
        many there were.  A regular-file Matroska advances without reading the frames' bytes (the
        positional reads are never issued); a pipe or a y4m stream reads them into a scratch frame."""
        if n <= 0:
            return 0
        if getattr(self, "_scratch", None) is None:
            self._scratch = bytearray(self.info.frame_bytes)
        if getattr(self, "_fd", None) is not None:
            try:  # the block headers are parsed, the offsets advance, and no positional read is issued
                return self._mkv.frames_into_pread(self._track, [memoryview(self._scratch)] * n, lambda off, dest: None)
            except ValueError as e:
                raise ValueError(f"V_UNCOMPRESSED {e}") from None
        for i in range(n):
            if self.read_into(self._scratch, 1) < 1:
                return i
        return n

    def _read_mkv(self, buf, n):
        fb = self.info.frame_bytes
        mv = memoryview(buf).cast("B")
        for i in range(n):
            try:
                ts = self._mkv.read_frame_into(self._track, mv[i * fb:(i + 1) * fb])
            except ValueError as e:
                raise ValueError(f"V_UNCOMPRESSED {e}") from None
            if ts is None:
                return i
        return n

    def _read_mkv_pread(self, buf, n):
        fb = self.info.frame_bytes
        mv = memoryview(buf).cast("B")
        futs = []

        def pread(off, dest):
            futs.append(self._pool.submit(_pread_exact, self._fd, dest, off))

        try:
            got = self._mkv.frames_into_pread(self._track, [mv[i * fb:(i + 1) * fb] for i in range(n)], pread)
        except ValueError as e:
            raise ValueError(f"V_UNCOMPRESSED {e}") from None
        finally:
            # every positional read has finished before the batch buffer is handed on (or
            # freed on an error path), failed or not; then the first failure is raised
            from concurrent.futures import wait
            wait(futs)
        for f in futs:
            f.result()
        return got

    def close(self, kill: bool = False) -> int:
        """Stop reading: join the pread pool; close the decoder child's output and wait for
        it (kill=True, on an error path: terminate it first).  Returns its exit code."""
        pool = getattr(self, "_pool", None)
        if pool is not None:
            pool.shutdown(wait=True)
            self._pool = None
        if self.child is None:
            return 0
        if kill and self.child.poll() is None:
            self.child.kill()
        try:
            self.child.stdout.close()
        except OSError:
            pass
        rc = self.child.wait()
        self.child = None
        return rc


def _fd_or_none(f):
    try:
        return f.fileno()
    except (AttributeError, OSError, ValueError):
        return None


def passthrough(args: List[str], stdin=None, stdout=None, stderr=None) -> int:
    """Outside the GPU profile: run exactly what the reference runs (on this segment's
    input, output and error streams: the process's own stdin / stdout / stderr unless given;
    in the resident encoder they are the client's descriptors, so ffmpeg's own `Duration:` /
    `frame=` lines reach the dispatcher as they would from the reference's worker)."""
    err = stderr or sys.stderr
    err.flush()  # our own lines before the child's
    try:
        return subprocess.call(reference_argv(args), stdin=_fd_or_none(stdin), stdout=_fd_or_none(stdout),
                               stderr=_fd_or_none(err))
    except FileNotFoundError:
        err.write("ffmpeg not found for a non-GPU profile\n")
        err.flush()
        return 127


def ffmpeg_fallthrough(src: Source, args: List[str], stdout, stderr=None) -> int:
    """The reference command on the CPU for frames already being read: the decoded frames
    go to `ffmpeg -f yuv4mpegpipe -i pipe: <remote_args> -f matroska pipe:` as y4m (its
    stderr is the segment's, see passthrough)."""
    err = stderr or sys.stderr
    argv = ["ffmpeg", "-f", "yuv4mpegpipe", "-i", "pipe:", *args, "-f", "matroska", "pipe:"]
    err.flush()
    try:
        child = subprocess.Popen(argv, stdin=subprocess.PIPE, stdout=stdout, stderr=_fd_or_none(err))
    except FileNotFoundError:
        err.write("ffmpeg not found for a non-GPU profile\n")
        err.flush()
        src.close()
        return 127
    fb = src.info.frame_bytes
    buf = bytearray(fb * 8)
    try:
        child.stdin.write(container.y4m_header(src.info))
        while True:
            n = src.read_into(buf, 8)
            for i in range(n):
                child.stdin.write(b"FRAME\n")
                child.stdin.write(memoryview(buf)[i * fb:(i + 1) * fb])
            if n < 8:
                break
        child.stdin.close()
    except BrokenPipeError:
        pass
    rc = child.wait()
    return rc or src.close()


_CHROMA_SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}

# -pix_fmt conversions the GPU path takes: (input sampling, requested sampling)
GPU_RESAMPLE_PAIRS = {("444", "422"), ("444", "420"), ("422", "420")}


def resample_plan(prof, info):
    """What -pix_fmt means for a segment: (src_chroma, dst_chroma), the input frames' format
    and the one to encode (equal without -pix_fmt or when it names the input's), or, for a
    conversion outside the GPU path (the up-sampling pairs), the reason as a str."""
    src = info.chroma
    dst = prof.chroma or src
    if dst == src or (src, dst) in GPU_RESAMPLE_PAIRS:
        return src, dst
    return f"-pix_fmt needs {src} -> {dst} chroma resampling"


def encoder_key(prof, info, dst_w, dst_h, sar, com_itu601, batch, rect=None, pad=None, orient=0, deint=0,
                unsharp=None, luts=None, cmat=None, denoise=None):
    """What an encoder context kept between segments (serve / resident mode) depends on: the
    input's shape and format and everything of the profile the context is opened with, the
    encoded chroma format (-pix_fmt), the resolved crop rectangle (x, y, w, h), the resolved
    pad (x, y, W, H), the orientation (0..7) and the deinterlacer (the resolved MJG_DEINT_* bits,
    resolve_deint: the batch buffers of such a context hold two more frames) included, and the
    six values of an unsharp (profile.Profile.unsharp; None without one), and the bytes of the
    tables in front of and behind the sws stage (luts: (lut_in, lut_out), each a (3, 256) uint8
    array or None: two eq filters with different options are different contexts), and the six
    coefficients of a colour matrix (cmat; without one the key is what it was), and the four strengths
    of a hqdn3d (denoise: (ls, cs, lt, ct), resolved; without one the key is what it was)."""
    src_chroma, dst_chroma = resample_plan(prof, info)
    key = (info.width, info.height, dst_w, dst_h, info.full_range, prof.qscale, sar,
           com_itu601, prof.huffman, src_chroma, dst_chroma, prof.rst, batch,
           None if rect is None else tuple(rect), None if pad is None else tuple(pad), int(orient), int(deint),
           tuple(None if t is None else t.tobytes() for t in (luts or (None, None))),
           None if unsharp is None else tuple(unsharp))
    key = key if cmat is None else key + (("cmat",) + tuple(int(v) for v in cmat),)
    return key if denoise is None else key + (("hqdn3d",) + tuple(float(v) for v in denoise),)


def resolve_deint(spec, info):
    """The MJG_DEINT_* bits of a yadif request (profile.Profile.deint) for a segment's input, or
    the reason (a str) it runs on the CPU.  parity=tff / bff is used as given; auto takes the
    stream's field order (container.StreamInfo.field): unflagged and top-field-first streams are
    tff, bottom-field-first ones bff, and a stream that declares anything else (y4m `Im`, a
    Matroska FieldOrder other than 1 and 6) has no single parity.  A plane below 3 x 3 is outside
    the filter's row and column clamps as the library restates them."""
    if spec is None:
        return 0
    hs, vs = _CHROMA_SHIFTS[str(info.chroma)]
    if min(info.width, info.height, (info.width + hs) >> hs, (info.height + vs) >> vs) < 3:
        return f"yadif of a {info.width}x{info.height} {info.chroma} input: a plane smaller than 3x3"
    parity = spec["parity"]
    if parity < 0:
        if info.field not in ("p", "t", "b"):
            return (f"yadif parity=auto on a stream of mixed or unknown field order (I{info.field}): per-frame field "
                    f"flags are not GPU-accelerated")
        parity = 1 if info.field == "b" else 0
    return 1 | (2 if spec["mode"] == 2 else 0) | (4 if parity else 0)


def deint_step(done: int, read: int, batch: int, eof: bool):
    """One submit of a deinterlaced segment: `done` frames are encoded, `read` frames have been
    read (the reader keeps one frame of look-ahead: read == done + batch + 1 unless the input
    ended, `eof`).  Returns (first, n, has_prev, has_next): frames [first, first + n) are encoded,
    with frame first - 1 in front of them and frame first + n behind them in the buffer when the
    flags say so.  n may be 0 at the end of the input."""
    n = max(0, min(batch, read - done - (0 if eof else 1)))
    return done, n, done > 0, done + n < read


def deint_schedule(nframes: int, batch: int):
    """Every submit of a segment of `nframes` frames, as run()'s reader makes them (deint_step on
    what it has read): the last one has no next frame, a segment of one frame neither neighbour."""
    out, done, read = [], 0, 0
    while True:
        want = done + batch + 1
        read = min(nframes, want)
        eof = read < want
        first, n, hp, hn = deint_step(done, read, batch, eof)
        if n:
            out.append((first, n, hp, hn))
        done += n
        if eof:
            return out


def oriented_size(w: int, h: int, orient: int):
    """The size of a w x h frame after the orientation (T | FX << 1 | FY << 2): h x w under T."""
    return (h, w) if orient & 1 else (w, h)


def oriented_sar(sar, orient: int):
    """The SAR after the orientation: vf_transpose sets 1 / SAR when the input's is known (its
    numerator is not 0), the flips keep it; an unknown SAR stays unknown."""
    if orient & 1 and sar and sar[0] > 0 and sar[1] > 0:
        return (sar[1], sar[0])
    return sar


def pad_fallthrough_reason(prof, in_size, src_chroma, dst_chroma) -> Optional[str]:
    """Why a graph that ends in `pad` runs on the CPU for this input, or None: in_size is the
    pad's input (the picture).  A picture whose width or height is no multiple of the format's
    sub-sampling: vf_pad copies the area rounded down and paints the last column or row, which
    the GPU path does not restate.  A -pix_fmt conversion without a scale: FFmpeg's converter
    then runs after the pad and filters across the border."""
    if prof.scale is None and src_chroma != dst_chroma:
        return (f"pad before the {src_chroma} -> {dst_chroma} -pix_fmt conversion (no scale in the graph: the "
                f"converter runs after the pad)")
    hs, vs = _CHROMA_SHIFTS[str(dst_chroma)]
    w, h = in_size
    if w & ((1 << hs) - 1) or h & ((1 << vs) - 1):
        return (f"pad of a {w}x{h} picture in {dst_chroma}: the size is no multiple of the chroma "
                f"sub-sampling ({1 << hs}x{1 << vs})")
    return None


def unsharp_fallthrough_reason(prof, full_range, src_chroma, dst_chroma) -> Optional[str]:
    """Why a graph with an `unsharp` runs on the CPU for this input, or None.  With a scale directly
    in front of it, format negotiation lets that scaler deliver the encoder's full-range format (as
    the pad assumes), so the filter sees what the sws stage produces.  Without a scale
    FFmpeg sharpens the decoded frames and converts afterwards, which equals the GPU path (sharpen
    behind the sws stage) only when nothing is converted: a full-range source in the encoded format."""
    if prof.unsharp is None or prof.scale is not None:
        return None
    if not full_range or src_chroma != dst_chroma:
        return "unsharp without a scale on a tv-range / converted input: FFmpeg sharpens before its converter"
    return None


def eq_fallthrough_reason(prof, info) -> Optional[str]:
    """Why a graph with an `eq` runs on the CPU for this input, or None.  The tables are the filter's
    8-bit path: samples of more than 8 bits go through another one."""
    if prof.eq is None:
        return None
    # slot "out" is directly behind a scale (profile._take_eq gives no other)
    assert prof.eq["slot"] == "in" or prof.scale is not None, prof
    bits = int(getattr(info, "bits", 8))
    if bits != 8:
        return f"eq on a {bits}-bit input: only the filter's 8-bit path is GPU-accelerated"
    return None


def cmat_fallthrough_reason(prof, info) -> Optional[str]:
    """Why a graph with a `colormatrix` runs on the CPU for this input, or None.  The filter takes
    yuv420p / yuv422p / yuv444p (and uyvy422): FFmpeg converts a full-range (yuvj) input to one of them
    first, which is not restated; and the coefficients are the 8-bit path's."""
    if prof.colormatrix is None:
        return None
    if info.full_range:
        return ("colormatrix on a full-range (yuvj) input: the filter takes yuv420p / yuv422p / yuv444p, and FFmpeg "
                "converts the range first, which is not GPU-accelerated")
    bits = int(getattr(info, "bits", 8))
    if bits != 8:
        return f"colormatrix on a {bits}-bit input: only the filter's 8-bit planar path is GPU-accelerated"
    return None


def denoise_fallthrough_reason(prof, info) -> Optional[str]:
    """Why a graph with a `hqdn3d` runs on the CPU for this input, or None.  The scans are the filter's 8-bit
    path: samples of more than 8 bits go through another one (and the library's frames are bytes)."""
    if getattr(prof, "hqdn3d", None) is None:
        return None
    bits = int(getattr(info, "bits", 8))
    if bits != 8:
        return f"hqdn3d on a {bits}-bit input: only the filter's 8-bit path is GPU-accelerated"
    hs, vs = _CHROMA_SHIFTS[str(info.chroma)]
    eight = info.width * info.height + 2 * ((info.width + hs) >> hs) * ((info.height + vs) >> vs)
    if getattr(info, "frame_bytes", eight) != eight:
        return (f"hqdn3d on an input of {info.frame_bytes} bytes a frame ({eight} at 8 bits): more than 8 bits a sample "
                f"are not GPU-accelerated")
    return None


def eq_luts(prof):
    """(lut_in, lut_out) for MjpegEncoder: the eq's tables in its slot, None elsewhere."""
    if prof.eq is None:
        return None, None
    tabs = profile.eq_tables(prof.eq)
    return (tabs, None) if prof.eq["slot"] == "in" else (None, tabs)


def scale_cascade_reason(in_size, out_size, src_chroma, dst_chroma) -> Optional[str]:
    """None when the sws stage takes in_size -> out_size (luma and chroma planes, both
    directions), else the reason: a bicubic filter of 256 taps or more, for which swscale
    cascades two scalers and the library has no kernel.  Device-free (mjg_sws_filter)."""
    from . import _lib
    L = _lib.load()
    (sw, sh), (dw, dh) = in_size, out_size
    planes = [((sw, sh), (dw, dh))]
    (shs, svs), (dhs, dvs) = _CHROMA_SHIFTS[str(src_chroma)], _CHROMA_SHIFTS[str(dst_chroma)]
    planes.append((((sw + shs) >> shs, (sh + svs) >> svs), ((dw + dhs) >> dhs, (dh + dvs) >> dvs)))
    for (pw, ph), (qw, qh) in planes:
        if (pw, ph) == (qw, qh):
            continue  # the plane keeps its size: no filter
        taps = C.c_int()
        for s_len, d_len, one, align in ((pw, qw, 1 << 14, 4), (ph, qh, 1 << 12, 2)):
            if L.mjg_sws_filter(s_len, d_len, one, align, 1, 128, 128, None, 0, None, C.byref(taps)) < 0:
                return f"scale {sw}x{sh} -> {dw}x{dh} needs swscale's cascade"
    return None


class Fallthrough(Exception):
    """This segment runs on the CPU ffmpeg; str() is the reason.  (The other way out of plan_segment is
    profile.CropError / PadError: FFmpeg itself fails to configure the filter, nothing is passed through.)"""


@dataclass(frozen=True, eq=False)
class SegmentPlan:
    """A profile resolved against one segment's input (plan_segment): what the encoder context is
    opened with and the muxer told, beyond what Profile and StreamInfo hold themselves."""
    src_chroma: str                  # the input frames' format and the one to encode (resample_plan)
    dst_chroma: str
    deint: int                       # the MJG_DEINT_* bits (resolve_deint); 0: no deinterlacer
    orient: int                      # T | FX << 1 | FY << 2; the fields below are of the oriented frame
    rect: Optional[tuple]            # the crop's (x, y, w, h), or None
    in_size: tuple                   # the sws stage's input: the rectangle's size, or the oriented frame's
    dst_w: int                       # the picture: the scale's output, or in_size
    dst_h: int
    pad: Optional[tuple]             # the picture's place and the canvas, (x, y, W, H), or None
    enc_w: int                       # what is encoded and muxed: the canvas, or the picture
    enc_h: int
    unsharp: Optional[tuple]
    lut_in: object                   # the eq's (3, 256) uint8 tables in its slot, None elsewhere
    lut_out: object
    cmat: Optional[tuple]            # the colormatrix's six coefficients, or None
    sar: tuple                       # of the picture (a crop and a pad leave it alone)

    # what only a SheetPlan decides: plain class attributes here, fields there (fields() and key() stay as they are)
    framestep = 1
    sheet = None
    # ... and what only a DenoisePlan decides
    denoise = None

    def rate(self, info):
        """What the muxer and the progress lines run at: the input's frame rate."""
        return info.fps

    def batch(self, b: int) -> int:
        """Frames per batch for b = batch_frames(...)."""
        return b

    def encoder_kwargs(self) -> dict:
        """The MjpegEncoder keyword arguments this plan decides (dst_w and dst_h go by position)."""
        return dict(sar=self.sar, chroma=self.dst_chroma, src_chroma=self.src_chroma, crop=self.rect, pad=self.pad,
                    orient=self.orient, deint=self.deint or None, unsharp=self.unsharp, lut_in=self.lut_in,
                    lut_out=self.lut_out, cmat=self.cmat)

    def key(self, prof, info, com_itu601, batch):
        """encoder_key of a context opened with this plan."""
        return encoder_key(prof, info, self.dst_w, self.dst_h, self.sar, com_itu601, batch, self.rect, self.pad,
                           self.orient, self.deint, self.unsharp, (self.lut_in, self.lut_out), self.cmat)


@dataclass(frozen=True, eq=False)
class DenoisePlan(SegmentPlan):
    """The plan of a profile.DenoiseProfile: the SegmentPlan plus the denoiser's four tables.  A segment is one
    sequence: its first batch is a plain submit and every later one continues it (Pipeline.run)."""
    denoise: object = None           # the (4, 8192) int16 tables (profile.hqdn3d_tables)
    strengths: tuple = ()            # the four strengths they were made from: what the cache key holds

    def encoder_kwargs(self) -> dict:
        return dict(super().encoder_kwargs(), denoise=self.denoise)

    def key(self, prof, info, com_itu601, batch):
        return encoder_key(prof, info, self.dst_w, self.dst_h, self.sar, com_itu601, batch, self.rect, self.pad,
                           self.orient, self.deint, self.unsharp, (self.lut_in, self.lut_out), self.cmat, self.strengths)


TILE_MAX_SIDE = 16384    # the pad's canvas limit (mjg_open_sheet refuses more)
TILE_MAX_FRAMES = 32     # a sheet never spans two submits, and 32 frames is the most a batch holds (batch_frames)


def tile_fallthrough_reason(prof, cell, src_chroma, dst_chroma) -> Optional[str]:
    """Why a graph that ends in `tile` runs on the CPU for this input, or None: `cell` is the tile's input
    picture.  The pad's two cases, for the same reasons (pad_fallthrough_reason): a -pix_fmt conversion without
    a scale would run behind the tile and filter across cell borders, and a cell that is no multiple of the
    sub-sampling gets a painted last column or row.  Then the sheet's own: a margin or padding that is no
    multiple of the sub-sampling (the chroma cells would not sit where vf_tile puts them), a sheet side
    beyond the canvas limit, and more frames a sheet than a batch holds."""
    t = prof.tile
    if prof.scale is None and src_chroma != dst_chroma:
        return (f"tile before the {src_chroma} -> {dst_chroma} -pix_fmt conversion (no scale in the graph: the "
                f"converter runs after the tile)")
    hs, vs = _CHROMA_SHIFTS[str(dst_chroma)]
    w, h = cell
    if w & ((1 << hs) - 1) or h & ((1 << vs) - 1):
        return (f"tile of {w}x{h} cells in {dst_chroma}: the size is no multiple of the chroma sub-sampling "
                f"({1 << hs}x{1 << vs})")
    m = (1 << max(hs, vs)) - 1
    if t["margin"] & m or t["padding"] & m:
        return (f"tile margin {t['margin']} / padding {t['padding']} in {dst_chroma}: no multiple of the chroma "
                f"sub-sampling ({1 << hs}x{1 << vs})")
    W, H = sheet_size(w, h, t)
    if W > TILE_MAX_SIDE or H > TILE_MAX_SIDE:
        return f"tile {t['cols']}x{t['rows']} of {w}x{h} cells: a {W}x{H} sheet, a side beyond {TILE_MAX_SIDE}"
    n = t["nb_frames"] or t["cols"] * t["rows"]
    if n > TILE_MAX_FRAMES:
        return f"tile of {n} frames a sheet: more than the {TILE_MAX_FRAMES} frames a submit holds"
    return None


def sheet_size(w: int, h: int, t: dict):
    """The sheet of w x h cells: (cols w + (cols - 1) padding + 2 margin, rows h + (rows - 1) padding + 2 margin)."""
    return (t["cols"] * w + (t["cols"] - 1) * t["padding"] + 2 * t["margin"],
            t["rows"] * h + (t["rows"] - 1) * t["padding"] + 2 * t["margin"])


def sheet_batch(b: int, n: int) -> int:
    """Frames per batch under a sheet of n frames: whole sheets, max(n, (b // n) * n) for b = batch_frames(...)."""
    return max(n, (b // n) * n)


@dataclass(frozen=True, eq=False)
class SheetPlan(SegmentPlan):
    """The plan of a profile.SheetProfile (a graph with a tile or a framestep above 1): enc_w x enc_h is
    the sheet."""
    sheet: Optional[tuple] = None    # (cols, rows, nb_frames, margin, padding), nb_frames resolved; None: framestep alone
    framestep: int = 1               # the reader keeps every framestep-th frame
    out_fps: Fraction = Fraction(25)  # what the muxer and the progress lines run at: fps / (framestep * nb_frames)

    def rate(self, info):
        return self.out_fps

    def batch(self, b: int) -> int:
        return b if self.sheet is None else sheet_batch(b, self.sheet[2])  # whole sheets

    def encoder_kwargs(self) -> dict:
        return dict(super().encoder_kwargs(), sheet=self.sheet)

    def key(self, prof, info, com_itu601, batch):
        return super().key(prof, info, com_itu601, batch) + (("sheet", self.sheet),)


THUMB_MAX_STORE = 2 << 30  # bytes of page-locked host memory a group may take (a guard, not a measured limit)


def thumbnail_fallthrough_reason(prof, info) -> Optional[str]:
    """Why a graph with a `thumbnail` runs on the CPU for this input, or None: the group store holds N decoded
    frames in page-locked host memory (100 4K 4:2:0 frames are 1.24 GB), and the histograms are of 8-bit
    samples."""
    hs, vs = _CHROMA_SHIFTS[str(info.chroma)]
    eight = info.width * info.height + 2 * ((info.width + hs) >> hs) * ((info.height + vs) >> vs)
    if info.frame_bytes != eight:
        return (f"thumbnail of an input of {info.frame_bytes} bytes a frame ({eight} at 8 bits): more than 8 bits a "
                f"sample are not GPU-accelerated")
    if prof.thumbnail * info.frame_bytes > THUMB_MAX_STORE:
        return (f"thumbnail={prof.thumbnail} of {info.width}x{info.height} {info.chroma} frames: a group of "
                f"{prof.thumbnail * info.frame_bytes} bytes, beyond the {THUMB_MAX_STORE} bytes of the page-locked group store")
    return None


@dataclass(frozen=True, eq=False)
class ThumbPlan(SheetPlan):
    """The plan of a profile.ThumbProfile: a SheetPlan whose reader keeps one frame of every `thumbnail`.  The
    rate, the batch and the encoder are the SheetPlan's: the filter does not change its link's frame rate."""
    thumbnail: int = 100

    def key(self, prof, info, com_itu601, batch):
        return super().key(prof, info, com_itu601, batch) + (("thumbnail", self.thumbnail),)


def plan_segment(prof, info) -> SegmentPlan:
    """Resolve a profile against a segment's input (container.StreamInfo): no device, no streams.
    Raises Fallthrough(reason) for a segment the CPU ffmpeg runs, and lets profile.CropError /
    PadError through for a request FFmpeg fails to configure.  The order of the checks decides which
    reason a user reads."""
    formats = resample_plan(prof, info)
    if isinstance(formats, str):
        raise Fallthrough(formats)
    src_chroma, dst_chroma = formats
    # -vf yadif in front of everything: the parity from the request or the stream's field order
    deint = resolve_deint(prof.deint, info)
    if isinstance(deint, str):
        raise Fallthrough(deint)
    # -vf vflip / transpose in front: everything below starts from the oriented frame.
    # vf_transpose takes only formats whose two chroma shifts are equal
    orient = prof.orient
    if orient & 1 and src_chroma == "422":
        raise Fallthrough("transpose of a 4:2:2 input: FFmpeg converts the format first")
    or_w, or_h = oriented_size(info.width, info.height, orient)
    # -vf crop: the rectangle of this input (the filter sees the decoded format); the scale
    # filter, the SAR and the encoded size then start from its size
    rect = None if prof.crop is None else profile.resolve_crop(prof.crop, or_w, or_h, src_chroma)
    in_size = (or_w, or_h) if rect is None else (rect[2], rect[3])
    dst_w, dst_h = prof.scale or in_size
    # -vf ...,pad: the canvas around the picture (dst_w x dst_h).  With a scale in front the pad
    # sees the encoded format (the scale converts), else the input's, which is then the encoded one
    pad = None
    if prof.pad is not None:
        why = pad_fallthrough_reason(prof, (dst_w, dst_h), src_chroma, dst_chroma)
        if why is not None:
            raise Fallthrough(why)
        pad = profile.resolve_pad(prof.pad, dst_w, dst_h, dst_chroma)
    enc_w, enc_h = (dst_w, dst_h) if pad is None else pad[2:]
    # -vf ...,unsharp: behind the sws stage; without a scale only when nothing is converted.
    # -vf ...,eq: tables in front of or behind the sws stage.  -vf ...,colormatrix: six coefficients
    # on the decoded frames.  Last the one scale the library refuses (a filter of 256 taps or more,
    # about 64:1), decided without a device
    why = (unsharp_fallthrough_reason(prof, info.full_range, src_chroma, dst_chroma)
           or eq_fallthrough_reason(prof, info) or cmat_fallthrough_reason(prof, info)
           or denoise_fallthrough_reason(prof, info)
           or scale_cascade_reason(in_size, (dst_w, dst_h), src_chroma, dst_chroma))
    if why is not None:
        raise Fallthrough(why)
    lut_in, lut_out = eq_luts(prof)
    cmat = None if prof.colormatrix is None else profile.colormatrix_coefs(*prof.colormatrix)
    # (a crop leaves the SAR as it is: keep_aspect=0; scaled_sar of equal sizes only reduces it;
    # a pad leaves it alone too: the scale's SAR, from the picture's size, not the canvas's)
    # (a transpose hands on 1 / SAR when the SAR is known: vf_transpose config_props_output)
    sar = profile.scaled_sar(oriented_sar(info.sar, orient), in_size, (dst_w, dst_h))
    if isinstance(prof, profile.SheetProfile):  # -vf framestep=N,...,tile: frames dropped in front, sheets behind (SAR: the cell's)
        sheet, n = None, 1
        if prof.tile is not None:
            why = tile_fallthrough_reason(prof, (dst_w, dst_h), src_chroma, dst_chroma)
            if why is not None:
                raise Fallthrough(why)
            t = prof.tile
            n = t["nb_frames"] or t["cols"] * t["rows"]
            sheet = (t["cols"], t["rows"], n, t["margin"], t["padding"])
            enc_w, enc_h = sheet_size(dst_w, dst_h, t)
        cls, more = SheetPlan, {}
        if isinstance(prof, profile.ThumbProfile):  # -vf [framestep=S,]thumbnail=N,...,tile: one frame of every N, picked by the reader
            why = thumbnail_fallthrough_reason(prof, info)
            if why is not None:
                raise Fallthrough(why)
            cls, more = ThumbPlan, dict(thumbnail=prof.thumbnail)
        return cls(src_chroma=src_chroma, dst_chroma=dst_chroma, deint=deint, orient=orient, rect=rect,
                   in_size=in_size, dst_w=dst_w, dst_h=dst_h, pad=pad, enc_w=enc_w, enc_h=enc_h,
                   unsharp=prof.unsharp, lut_in=lut_in, lut_out=lut_out, cmat=cmat, sar=sar,
                   sheet=sheet, framestep=prof.framestep, out_fps=Fraction(info.fps) / (prof.framestep * n), **more)
    cls, more = SegmentPlan, {}
    if isinstance(prof, profile.DenoiseProfile):  # -vf [yadif,]hqdn3d,...: the tables, behind the deinterlacer
        cls = DenoisePlan
        more = dict(denoise=profile.hqdn3d_tables(prof.hqdn3d),
                    strengths=tuple(float(prof.hqdn3d[k]) for k in profile.HQDN3D_NAMES))
    return cls(src_chroma=src_chroma, dst_chroma=dst_chroma, deint=deint, orient=orient, rect=rect,
               in_size=in_size, dst_w=dst_w, dst_h=dst_h, pad=pad, enc_w=enc_w, enc_h=enc_h,
               unsharp=prof.unsharp, lut_in=lut_in, lut_out=lut_out, cmat=cmat, sar=sar, **more)


JOIN_TIMEOUT = 5.0  # Pipeline.stop: what the reader and the muxer thread each get to end; one still alive after it is stuck


class Pipeline:
    """One segment through an open encoder: a reader thread fills the batch buffers from `src`, run()
    submits them and drains the synced submits into output buffers, a muxer thread writes those to `mkv`.
    All it works with is handed in, so it runs without a GPU: `enc` is used through frame_bytes, host_depth,
    submit(arr, n, halo=), sync(), last_total and fetch_into(buf); `bufs` through .array; `obufs` (a list
    filled and regrown here; None: not made yet) through .nbytes, .free() and what fetch_into needs;
    `new_obuf(nbytes)` makes one.  `batch` frames a submit, every `step`-th frame kept, `deint`: halo submits,
    `denoise`: submit(arr, n, halo=, cont=), the first of the segment plain and every later one cont=True.
    `thumb` (a ThumbPlan): (hist, store, N), `hist` used through count(frames, nframes) -> (n, 768) counters,
    `store` a page-locked buffer of N frames through .array; the reader keeps one frame of every N.

    The reader fills one batch while two are queued on the GPU (the encoder takes a second submit before
    the first is synced, so its kernels run back to back); a batch returns to the reader as soon as its
    submit is synced (the H2D has read it), before the packets are fetched, so the reader never waits on
    the fetch.  The reader posts (buffer, encoded frames, halo bits) to `full`, None at the end of the
    input, or the exception that stopped it.  After run(), failed or not, comes stop()."""

    def __init__(self, enc, bufs, obufs, new_obuf, src, mkv, prog, batch: int, step: int = 1, deint: bool = False,
                 thumb=None, denoise: bool = False):
        self.enc, self.bufs, self.obufs, self.new_obuf = enc, bufs, obufs, new_obuf
        self.thumb = thumb
        self.denoise = denoise      # the segment is one sequence: every submit but the first continues it
        self.submits = 0            # submits of this segment so far
        self.gn, self.ghists = 0, []  # read_thumb: the open group's frames in the store and their histograms
        self.src, self.mkv, self.prog = src, mkv, prog
        self.batch, self.step, self.deint, self.fb = batch, step, deint, enc.frame_bytes
        self.done = self.nread = 0  # read_deint: frames encoded and frames read so far
        self.prev = None            # read_deint: the previous buffer and the slot of its last encoded frame
        self.free: "queue.Queue[int]" = queue.Queue()
        self.full: "queue.Queue" = queue.Queue()
        # the muxer thread writes each synced submit's packets while the main thread keeps the
        # GPU fed (a 4K segment's 120 JPEGs are ~20 MB of writes)
        self.outq: "queue.Queue" = queue.Queue(maxsize=4)
        self.ofree: "queue.Queue[int]" = queue.Queue()  # output buffers the muxer has written
        for i in range(len(bufs)):
            self.free.put(i)
        for i in range(len(obufs)):
            self.ofree.put(i)
        self.abort = threading.Event()
        self.mux_err: list = []
        self.queued: list = []  # buffer index and frame count per submit, oldest first
        self.frames = 0
        self.tr = {"read": 0.0, "submit": 0.0, "sync": 0.0, "fetch": 0.0, "mux": 0.0, "wait": 0.0}
        self.failed, self.reader_stuck, self.muxer_stuck = True, False, False
        self.th = threading.Thread(target=self.reader, daemon=True)
        self.mt = threading.Thread(target=self.muxer, daemon=True)

    def read_plain(self, i):
        n = self.src.read_into(self.bufs[i].array, self.batch)
        return n, 0, n < self.batch

    def read_step(self, i):
        """-vf framestep: frame k of the segment is kept when k % step == 0, the rest passed over."""
        n, arr, fb = 0, self.bufs[i].array, self.fb
        while n < self.batch and self.src.read_into(arr[n * fb:(n + 1) * fb], 1) == 1:
            n += 1
            self.src.skip(self.step - 1)
        return n, 0, n < self.batch

    def read_thumb(self, i):
        """-vf [framestep=S,]thumbnail=N: the frames kept by the framestep go into the group store, in runs of at
        most a batch, each counted by the GPU as it arrives (hist.count, synchronous, on its own stream); when the
        store holds N frames, or the input ends with at least one in it, profile.thumbnail_pick selects one and it
        is copied into the batch buffer.  Groups restart with the segment."""
        hist, store, N = self.thumb
        arr, fb, n, eof = self.bufs[i].array, self.fb, 0, False
        while n < self.batch and not eof:
            while self.gn < N:
                run = min(self.batch, N - self.gn)
                dst = store.array[self.gn * fb:(self.gn + run) * fb]
                if self.step > 1:
                    got = 0
                    while got < run and self.src.read_into(dst[got * fb:(got + 1) * fb], 1) == 1:
                        got += 1
                        self.src.skip(self.step - 1)
                else:
                    got = self.src.read_into(dst, run)
                if got:
                    self.ghists.extend(hist.count(dst[:got * fb], got))
                    self.gn += got
                if got < run:
                    eof = True
                    break
            if self.gn:  # the group is closed: N frames, or what was left of the input
                k = profile.thumbnail_pick(self.ghists)
                arr[n * fb:(n + 1) * fb] = store.array[k * fb:(k + 1) * fb]
                n += 1
                self.gn, self.ghists = 0, []
        return n, 0, eof

    def read_deint(self, i):
        """A deinterlaced segment: a batch needs the frame in front of it and the one behind it, so the
        reader keeps one frame of look-ahead and every buffer but the first starts with the previous
        buffer's last encoded frame and its look-ahead frame (two host frame copies per batch; the
        previous buffer is only read, the reader thread is the only writer).  The encoded frames come
        after the halo frame in front (deint_step is the schedule)."""
        arr, fb, base = self.bufs[i].array, self.fb, 0
        if self.prev is not None:
            pi, slot = self.prev
            if pi == i:
                raise RuntimeError("deinterlacer: the previous batch buffer came back before the next was filled")
            arr[:2 * fb] = self.bufs[pi].array[slot * fb:(slot + 2) * fb]
            base = 2
        want = self.done + self.batch + 1 - self.nread
        got = self.src.read_into(arr[base * fb:(base + want) * fb], want)
        self.nread += got
        eof = got < want
        _, n, hp, hn = deint_step(self.done, self.nread, self.batch, eof)
        self.prev = (i, int(hp) + n - 1)
        self.done += n
        return n, int(hp) | int(hn) << 1, eof

    def reader(self):
        """The reader thread: one of the four strategies above fills buffer i and returns (encoded
        frames, halo bits, end of input)."""
        read = (self.read_thumb if self.thumb else self.read_deint if self.deint else self.read_step if self.step > 1
                else self.read_plain)
        try:
            while True:
                i = self.free.get()
                if i < 0 or self.abort.is_set():
                    return
                t0 = time.monotonic()
                n, halo, eof = read(i)
                self.tr["read"] += time.monotonic() - t0
                self.full.put((i, n, halo))
                if eof:
                    self.full.put(None)
                    return
        except BaseException as e:   # surfaced by run()
            self.full.put(e)

    def muxer(self):
        while True:
            try:
                item = self.outq.get(timeout=0.1)
            except queue.Empty:
                if self.abort.is_set():  # error path: the main thread may not be able to post None
                    return
                continue
            if item is None:
                return
            packets, ob = item
            if self.mux_err:
                self.ofree.put(ob)
                continue  # drain after a failure
            try:
                t0 = time.monotonic()
                for p in packets:
                    self.mkv.write_frame(p)
                self.mkv.flush_pending()  # the packets leave buffer `ob` before it is reused
                self.tr["mux"] += time.monotonic() - t0
                self.frames += len(packets)  # (under a sheet fewer than the frames submitted)
                self.prog.update(self.frames, sum(len(p) for p in packets))
            except BaseException as e:  # surfaced by the main thread
                self.mux_err.append(e)
            self.ofree.put(ob)

    def drain_one(self):
        enc, obufs = self.enc, self.obufs
        j = self.queued.pop(0)
        t0 = time.monotonic()
        enc.sync()
        self.free.put(j)  # consumed by its H2D: back to the reader before the fetch
        t1 = time.monotonic()
        while True:  # a written output buffer (the muxer returns them); a muxer that failed returns no more
            try:
                ob = self.ofree.get(timeout=0.1)
                break
            except queue.Empty:
                if self.mux_err:
                    raise self.mux_err[0]
        need = enc.last_total
        # page-locked output buffers: the packets are DMA'd into one (enc.fetch_into) and the
        # muxer writes them from it; regrown when a submit's JPEGs do not fit
        if obufs[ob] is None or obufs[ob].nbytes < need:
            if obufs[ob] is not None:
                obufs[ob].free()
            obufs[ob] = self.new_obuf(max(need + need // 2, 1 << 20))
        packets = enc.fetch_into(obufs[ob])  # one DMA into page-locked memory, no copy
        self.tr["sync"] += t1 - t0
        self.tr["fetch"] += time.monotonic() - t1
        if self.mux_err:
            raise self.mux_err[0]
        self.outq.put((packets, ob))

    def run(self) -> None:
        enc, tr, fb = self.enc, self.tr, self.fb
        self.th.start()
        self.mt.start()
        while True:
            t0 = time.monotonic()
            item = self.full.get()
            tr["wait"] += time.monotonic() - t0
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            i, n, halo = item
            if not n:  # the input ended on a batch boundary: nothing in this buffer
                self.free.put(i)
                continue
            if len(self.queued) == enc.host_depth:  # host submits: one launch each
                self.drain_one()
            t0 = time.monotonic()
            nh = (halo & 1) + (halo >> 1)
            if self.denoise:  # the first batch starts the sequence (a cached context's state is another segment's)
                enc.submit(self.bufs[i].array[:(n + nh) * fb], n, halo=halo, cont=self.submits > 0)
            else:
                enc.submit(self.bufs[i].array[:(n + nh) * fb], n, halo=halo)
            self.submits += 1
            tr["submit"] += time.monotonic() - t0
            self.queued.append(i)
        while self.queued:
            self.drain_one()
        self.outq.put(None)
        self.mt.join()
        if self.mux_err:
            raise self.mux_err[0]
        self.mkv.close()
        self.prog.update(self.frames, 0, final=True)
        self.failed = False

    def stop(self) -> int:
        """After run(), however it ended: nothing may be freed while a reader could still write into a
        batch buffer, so stop the reader thread (it finishes at most the read in flight, whose
        positional reads it waits for), killing a decoder child whose pipe it may be blocked on, and
        then close the source.  Returns the decoder's exit code."""
        self.abort.set()
        self.free.put(-1)
        if self.mt.is_alive():  # error path: let the muxer finish what it holds, then stop
            try:  # never block here: a full queue means the muxer is inside a write, and it
                self.outq.put_nowait(None)  # sees `abort` once that write returns
            except queue.Full:
                pass
            self.mt.join(timeout=JOIN_TIMEOUT)
        self.th.join(timeout=JOIN_TIMEOUT)
        if self.th.is_alive():
            self.src.close(kill=True)
            self.th.join(timeout=JOIN_TIMEOUT)
        self.reader_stuck = self.th.is_alive()  # blocked on a stdin pipe that never delivers
        self.muxer_stuck = self.mt.is_alive()   # inside a write to a stdout pipe that does not drain
        return self.src.close(kill=self.failed)


class Context:
    """An encoder context with its page-locked buffers: NBUF batch buffers and NOUT output buffers, the
    latter made and regrown by the pipeline that fetches into them.  Under a ThumbPlan also the histogram
    object and the page-locked group store of N frames, which the reader thread alone uses.  acquire() opens
    one or takes the serve / resident cache's, settle() decides after the segment whether it is kept, freed or
    leaked."""
    hist = store = None

    def __init__(self, device: int, prof, info, plan: SegmentPlan, batch: int, com_itu601: bool):
        from .encoder import MjpegEncoder, PinnedBuffer   # GPU work starts here
        self.enc = MjpegEncoder(device, info.width, info.height, plan.dst_w, plan.dst_h, full_range=info.full_range,
                                qscale=prof.qscale, max_batch=batch, com_itu601=com_itu601, huffman=prof.huffman,
                                rst=prof.rst, **plan.encoder_kwargs())
        # (a deinterlacer: room for the frame in front of a batch and the one behind it)
        self.bufs = [PinnedBuffer((batch + (2 if plan.deint else 0)) * self.enc.frame_bytes) for _ in range(NBUF)]
        self.obufs = [None] * NOUT
        self.new_obuf = PinnedBuffer
        n = getattr(plan, "thumbnail", 0)
        if n:
            from .encoder import FrameHist
            self.hist = FrameHist(device, info.width, info.height, plan.src_chroma, batch)
            self.store = PinnedBuffer(n * self.enc.frame_bytes)

    def thumb(self, plan):
        """Pipeline's `thumb` for this context: (hist, store, N) under a ThumbPlan, else None."""
        return None if self.hist is None else (self.hist, self.store, plan.thumbnail)

    @classmethod
    def acquire(cls, cache, device: int, prof, info, plan: SegmentPlan, batch: int, com_itu601: bool) -> "Context":
        """The cache's context when it was opened for the same plan.key(...), else a new one, in
        place of whatever the cache (a dict, or None: one segment) held."""
        key = plan.key(prof, info, com_itu601, batch)
        if cache is not None and cache.get("key") == key:
            return cache["ctx"]
        if cache is not None:
            release(cache)
        ctx = cls(device, prof, info, plan, batch, com_itu601)
        if cache is not None:
            cache.update(key=key, ctx=ctx)
        return ctx

    def settle(self, cache, pipe: Pipeline) -> None:
        """After pipe.stop(): the cache keeps the context of a segment that went through.  A failed
        segment, or one with a stuck thread, may have a submit queued: its cache entry goes and the next
        segment starts afresh.  The encoder is closed here, after the reader has stopped and the source is
        closed.  A stuck reader may yet write into a batch buffer, and a stuck muxer holds packets that are
        views into the output buffers: such buffers are leaked, never freed."""
        if cache is not None and not (pipe.failed or pipe.reader_stuck or pipe.muxer_stuck):
            return
        if cache is not None:
            cache.pop("key", None)
            cache.pop("ctx", None)
        self.free(bufs=not pipe.reader_stuck, obufs=not pipe.muxer_stuck)

    def free(self, bufs: bool = True, obufs: bool = True) -> None:
        self.enc.close()
        if self.hist is not None and bufs:  # (a stuck reader may be inside a count)
            self.hist.close()
        for b in (self.bufs + [self.store] if bufs else []) + (self.obufs if obufs else []):
            if b is not None:
                b.free()


def release(cache) -> None:
    """Close the encoder context and free the buffers a serve cache holds."""
    ctx = cache.pop("ctx", None)
    cache.pop("key", None)
    if ctx is not None:
        ctx.free()


def trace_line(opts: Options, pipe: Pipeline, t_run: float, t_seg: float) -> str:
    """MJG_WORKER_TRACE's line for a segment that went through (bench.py parses it)."""
    hand = ""  # the resident's hand-off: client start -> accept -> worker.run
    if opts.t_accept:
        hand += f"handoff={t_run - opts.t_accept:.4f} "
        if opts.client_t0:
            hand += f"client={opts.t_accept - opts.client_t0:.4f} "
    return (f"mjg-trace: frames={pipe.frames} total={time.monotonic() - t_seg:.4f} setup={t_seg - t_run:.4f} {hand}"
            + " ".join(f"{k}={v:.4f}" for k, v in pipe.tr.items()) + f" {placement()}\n")


def run(device: int, args: List[str], stdin=None, stdout=None, stderr=None, cache=None,
        batch_bytes: Optional[int] = None, opts: Optional[Options] = None) -> int:
    """One segment, stdin -> stdout.  `cache` (serve / resident mode): a dict that keeps the
    encoder context and its page-locked buffers between segments of the same stream
    shape.  `opts`: the segment's settings (default: this process's, process_options)."""
    t_run = time.monotonic()
    opts = opts or process_options(batch_bytes)
    stdin = stdin or sys.stdin.buffer
    stdout = stdout or sys.stdout.buffer
    stderr = stderr or sys.stderr
    prof, why = profile.try_parse(args)
    if prof is None:
        stderr.write(f"gpu:{device}: {why}; running ffmpeg on the CPU\n")
        stderr.flush()
        return passthrough(args, stdin, stdout, stderr)

    src = Source(stdin, opts.read_threads, stderr)
    info = src.info
    try:
        plan = plan_segment(prof, info)
    except Fallthrough as e:
        stderr.write(f"gpu:{device}: {e}; running ffmpeg on the CPU\n")
        stderr.flush()
        return ffmpeg_fallthrough(src, args, stdout, stderr)
    except (profile.CropError, profile.PadError) as e:  # ffmpeg fails to configure the filter: no pass-through
        stderr.write(f"gpu:{device}: {e.filter}: {e}\n")
        stderr.flush()
        src.close(kill=True)
        return 1
    bind_numa(device)  # before the reader threads and the batch buffers
    batch = plan.batch(batch_frames(opts, info.frame_bytes))
    ctx = Context.acquire(cache, device, prof, info, plan, batch, opts.com_itu601 and not info.full_range)
    out_fps = plan.rate(info)
    prog = Progress(stderr, out_fps, prof.qscale)
    prog.duration(src.duration)
    mkv = container.MkvWriter(stdout, plan.enc_w, plan.enc_h, out_fps, plan.sar)
    pipe = Pipeline(ctx.enc, ctx.bufs, ctx.obufs, ctx.new_obuf, src, mkv, prog, batch, plan.framestep, bool(plan.deint),
                    ctx.thumb(plan), plan.denoise is not None)
    t_seg = time.monotonic()
    try:
        pipe.run()
        if opts.trace:
            stderr.write(trace_line(opts, pipe, t_run, t_seg))
            stderr.flush()
    finally:
        rc = pipe.stop()
        ctx.settle(cache, pipe)
    if rc:
        stderr.write(f"decoder exited with {rc}\n")
        return 1
    return 0


SERVE_DONE = "mjg-serve: segment done rc="


def serve(device: int, args: List[str], requests=None, stderr=None) -> int:
    """Persistent worker (dispatcher --persistent-gpu-workers): one process per `-H gpu:N`
    entry encodes segment after segment, keeping its HIP context, encoder and page-locked
    buffers, so a segment no longer pays process start + HIP init + allocation (~0.5 s).
    Each request line on stdin is a JSON array `[INPUT, OUTPUT]` (dispatcher.serve_request:
    any path survives, tabs and newlines included); the segment runs exactly as `run`
    runs it for one process (same output bytes, same ffmpeg-style stderr lines), then
    `mjg-serve: segment done rc=N` on stderr ends it.  EOF on stdin ends the server."""
    requests = requests or sys.stdin
    stderr = stderr or sys.stderr
    cache: dict = {}
    try:
        for line in requests:
            line = line.rstrip("\n")
            if not line:
                continue
            try:
                src, dst = json.loads(line)
                with open(src, "rb") as fin, open(dst, "wb") as fout:
                    rc = run(device, args, stdin=fin, stdout=fout, stderr=stderr, cache=cache,
                             batch_bytes=SERVE_BATCH_BYTES)
            except Exception as e:
                stderr.write(f"gpu:{device}: {type(e).__name__}: {e}\n")
                rc = 1
            stderr.write(f"{SERVE_DONE}{rc}\n")
            stderr.flush()
    finally:
        release(cache)
    return 0


def main(argv=None) -> int:
    # no -h/--help and no abbreviations: every other argument is ffmpeg's (remote_args), and
    # argparse would read `-huffman default` as `-h uffman`
    ap = argparse.ArgumentParser(prog="ffmpeg_distributed_amd.worker", add_help=False, allow_abbrev=False)
    ap.add_argument("--device", type=int, required=True)
    ap.add_argument("--serve", action="store_true")
    ns, rest = ap.parse_known_args(argv)
    if ns.serve:
        return serve(ns.device, rest)
    try:
        return run(ns.device, rest)
    except Exception as e:  # the dispatcher re-queues the segment on a nonzero exit
        sys.stderr.write(f"gpu:{ns.device}: {type(e).__name__}: {e}\n")
        return 1


if __name__ == "__main__":
    sys.exit(main())
