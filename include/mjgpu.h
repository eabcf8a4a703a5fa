/*
 * mjgpu.h -- C-ABI of libmjgpu.so, the MI355X (gfx950) MJPEG segment encoder.
 *
 * Drop-in boundary.  The reference (Rouji/ffmpeg_distributed) has no FFI: its hot
 * path is the per-segment worker process built at ffmpeg_distributed.py:131-138
 *     nice -n10 ionice -c3 ffmpeg -f matroska -i pipe: <remote_args> -f matroska pipe:
 * and launched/supervised at ffmpeg_distributed.py:139-141 (FFMPEGProc.run,
 * ffmpeg_distributed.py:59-91).  For the north-star profile
 *     [-vf [yadif[=0|2],][vflip|transpose=N,...][crop=w:h:x:y,][scale=W:H:flags=bicubic][,unsharp[=lx:ly:la:cx:cy:ca]][,pad=W:H:x:y]] -c:v mjpeg -q:v N -dct int -huffman default -bitexact
 * (every filter is a field of mjg_chain, which documents the stages in the order they run: `-pix_fmt
 * yuvj420p|yuvj422p` from a 4:4:4 or 4:2:2 input, src_chroma_format: the chroma down-sampling
 * FFmpeg's auto-inserted scaler does, taken to be its default bicubic; `yadif` as the very first
 * filter, frame-rate modes 0 and 2, deint: the deinterlacer, a restatement of the filter's C path
 * that no FFmpeg build has been compared with yet; a leading run of vflip / transpose, orient: one of
 * eight plane maps; one `colormatrix=SRC:DST` behind the yadif and the orientation and in front of
 * any eq and the scale, cmat: six 16.16 coefficients on whole frames, a restatement of
 * vf_colormatrix.c's 8-bit planar path that no FFmpeg build has been compared with yet; one `eq=...`
 * in front of the scale, or directly behind it, lut_in / lut_out: a table per plane, a restatement of
 * vf_eq.c's 8-bit path that no FFmpeg build has been compared with yet; `-vf crop=...` alone or
 * before the scale, the crop group: a rectangle of the decoded frames; `unsharp` behind the scale and
 * in front of the pad, unsharp: the sharpen, a restatement of vf_unsharp.c's 8-bit path that no
 * FFmpeg build has been compared with yet; `pad=...` as the last filter, the pad group: the picture
 * on a black canvas; `tile=...` as the last filter is mjg_sheet, and the `thumbnail=N` in front of a
 * storyboard's chain is no stage at all: mjg_hist counts the decoded frames' histograms and the
 * caller selects, a restatement of vf_thumbnail.c's planar path that no FFmpeg build has been
 * compared with yet; `hqdn3d` as the very first filter or directly behind the yadif is mjg_denoise, four
 * tables and three scans behind the deinterlacer, a restatement of vf_hqdn3d.c's 8-bit path that no FFmpeg
 * build has been compared with yet)
 * this library replaces the arithmetic that worker runs (swscale bicubic + tv->pc
 * range conversion, jfdctint + quantiser + default-table Huffman + 0xFF stuffing)
 * and the Python host code in ffmpeg_distributed_amd/ (worker.py, dispatcher.py)
 * replaces the process around it with the same stdin/stdout/stderr/exit-code
 * contract.  Plain C types only; no torch types cross this boundary.
 *
 * Threading: one mjg_ctx per (device, caller thread); a ctx owns its HIP stream,
 * device buffers and filter tables.  Calls on different contexts may run
 * concurrently.  The library never writes to stdout (stdout is the data stream).
 * Every call returns MJG_OK (0) or a negative MJG_E_* code; mjg_last_error()
 * returns a thread-local description of the last failure.
 */
#ifndef MJGPU_H
#define MJGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MJG_OK 0
#define MJG_E_INVALID (-1)     /* bad argument / unsupported geometry */
#define MJG_E_HIP (-2)         /* HIP runtime error (no device, launch failure ...) */
#define MJG_E_NOMEM (-3)       /* device or pinned-host allocation failed */
#define MJG_E_CAPACITY (-4)    /* caller buffer too small */
#define MJG_E_STATE (-5)       /* call out of order (e.g. fetch before submit) */

/* mjg_config.flags */
#define MJG_F_TIMING 1u        /* record HIP events around every kernel launch */
#define MJG_F_DEBUG_COEFS 2u   /* keep quantized coefficients of every block (tests) */
#define MJG_F_SWS_NO_BITEXACT 4u /* swscale filter tables without SWS_BITEXACT */
#define MJG_F_COM_ITU601 8u    /* add COM "CS=ITU601" (FFmpeg builds whose CLI hands the encoder
                                  yuv420p+full-range instead of yuvj420p; mjpegenc_common.c
                                  jpeg_put_comments) */
#define MJG_F_HUFFMAN_OPTIMAL 16u /* -huffman optimal (FFmpeg's default): per-frame Huffman tables
                                  from the frame's symbol counts (mjpegenc_huffman.c); the
                                  header's DHT then differs per frame */
#define MJG_F_RST 32u          /* slice-threaded bitstream (-slices N / -thread_type slice): DRI =
                                  MCUs per row, every MCU row its own entropy-coded segment
                                  (DC predictors reset, 1-bit padded, RST0..7 between rows;
                                  mpegvideo_enc.c encode_thread rtp_mode + mjpegenc.c
                                  ff_mjpeg_encode_stuffing).  Implies -huffman default, as
                                  FFmpeg forces; MJG_F_RST | MJG_F_HUFFMAN_OPTIMAL is invalid */

/* mjg_config.chroma_format */
#define MJG_CHROMA_420 0       /* yuv(j)420p: MCU 16x16, Y 2x2 Cb 1x1 Cr 1x1 */
#define MJG_CHROMA_422 1       /* yuv(j)422p: MCU 16x16, Y 2x2 Cb 1x2 Cr 1x2 */
#define MJG_CHROMA_444 2       /* yuv(j)444p: MCU 8x16, every component 1x2 (ff_mjpeg_init_hvsample) */

#define MJG_F_TIMING_DETAIL 64u /* MJG_F_TIMING plus events around every tail kernel (scan, 0xFF
                                  count, write: MJG_K_SCAN_BITS .. MJG_K_WRITE); each event adds
                                  ~10 us of GPU idle between those short kernels */
#define MJG_F_MERGE 1024u      /* opt-in library-side merging: single-segment device submits are held
                                  and launched two at a time (see mjg_submit; the caller keeps each
                                  submit's frames valid until its own mjg_sync).  Without it every
                                  mjg_submit is a launch of its own, launched inside the call */

/* Kernel ids for mjg_kernel_times() */
#define MJG_K_SCALE 0          /* bicubic hscale + range + vscale (per plane; a plane that keeps
                                  its size: the streaming copy) */
#define MJG_K_ENCODE 1         /* load + FDCT + quant + Huffman -> chunk bits */
#define MJG_K_SCAN_BITS 2      /* per-frame exclusive scan of chunk bit lengths      */
#define MJG_K_COUNT_FF 3       /* realign chunk bits, pad, count 0xFF per chunk group */
#define MJG_K_SCAN_FF 4        /* per-frame scan of 0xFF counts -> frame sizes, offsets */
#define MJG_K_WRITE 5          /* header + stuffed scan + EOI into packed output     */
#define MJG_K_HUFF 6           /* -huffman optimal: symbol-count pass + table build   */
#define MJG_K_TAIL 7           /* MJG_K_SCAN_BITS .. MJG_K_WRITE as one interval (MJG_F_TIMING) */
#define MJG_NUM_KERNELS 8

typedef struct mjg_config {
  int32_t src_w, src_h;      /* decoded frame size (packed I420: Y, then U, then V)    */
  int32_t dst_w, dst_h;      /* encoded size; == src when remote_args has no -vf scale */
  int32_t in_full_range;     /* 1: yuvj420p input; 0: yuv420p (tv) -> tv->pc as swscale */
  int32_t qscale;            /* effective mpegvideo qscale, 2..31 (see -q:v mapping)   */
  int32_t sar_num, sar_den;  /* JFIF APP0 density; 0/0 omits APP0 (unknown SAR)        */
  int32_t max_batch;         /* most frames one mjg_submit() may carry                 */
  uint32_t flags;            /* MJG_F_*                                                */
  int32_t chroma_format;     /* MJG_CHROMA_* of the encoded JPEG (and of the input frames unless
                                mjg_open_src says otherwise); packed planar Y, Cb, Cr   */
} mjg_config;

typedef struct mjg_ctx mjg_ctx;

/* Library version (major*10000 + minor*100 + patch). */
int mjg_version(void);
/* Thread-local text of the last error (never NULL). */
const char *mjg_last_error(void);
/* Number of visible HIP devices, or a negative MJG_E_* code. */
int mjg_device_count(void);
/* NUMA node of `device` (its PCI function's numa_node in sysfs), -1 when the platform does
 * not say, or a negative MJG_E_* code.  The worker binds its reader threads to that node. */
int mjg_device_numa_node(int device);

/* Create a context on `device`: validates cfg, builds quant/Huffman/filter tables,
 * allocates device buffers for cfg->max_batch frames.  Replaces one
 * `ffmpeg ... <remote_args>` worker's codec/scaler initialisation
 * (ffmpeg_distributed.py:131-138).  -vf scale: any size pair whose bicubic filters stay below
 * 256 taps per direction and plane (down to about 64:1; mjg_sws_filter tells, without a device).
 * Past that swscale cascades two scalers, which the library does not: MJG_E_INVALID ("needs
 * swscale's cascade").  Planes down to about 4:1 run on k_scale (one LDS tile per output tile),
 * steeper ones on k_scale_stream (mjg_debug_scale_path). */
int mjg_open(int device, const mjg_config *cfg, mjg_ctx **out);

/* mjg_chain.deint */
#define MJG_DEINT_YADIF 1      /* -vf yadif, mode 0 (send_frame), deint=all */
#define MJG_DEINT_NOSPATIAL 2  /* ... mode 2 (send_frame_nospatial): no spatial interlacing check */
#define MJG_DEINT_BFF 4        /* bottom field first (parity=bff): the even rows are interpolated; without
                                  it top field first, the odd rows */

/* -vf unsharp: luma and chroma matrix sizes (odd, 3..23) and amounts as the filter holds them,
 * (int)(amount * 65536.0) with C truncation; the filter's defaults are {5, 5, 65536, 5, 5, 0}. */
typedef struct mjg_unsharp { int32_t lx, ly, la, cx, cy, ca; } mjg_unsharp;

/* A table per plane: out = t[in].  `-vf eq` on 8-bit planar frames is three such tables
 * (profile.eq_tables makes them); the library knows tables, not the filter. */
typedef struct mjg_lut { uint8_t y[256], u[256], v[256]; } mjg_lut;   /* out = t[in], per plane */

/* A colour matrix on whole frames: the six 16.16 coefficients c2..c7 of
 *   u = U - 128, v = V - 128          (U, V: the chroma pair of the luma sample's cell)
 *   Y' = clip8((65536 (Y - 16) + yu u + yv v + 1081344) >> 16)
 *   U' = clip8((uu u + uv v + 8421376) >> 16),  V' = clip8((vu u + vv v + 8421376) >> 16)
 * in C int with an arithmetic shift.  `-vf colormatrix=SRC:DST` on 8-bit planar frames is six such
 * numbers (profile.colormatrix_coefs makes them); the library knows the numbers, not the filter. */
typedef struct mjg_cmatrix { int32_t yu, yv, uu, uv, vu, vv; } mjg_cmatrix;

/* What a context does to the frames handed over before it encodes them: the filter chain, one
 * field (or group) per stage, in the order the stages run.  A chain that is all zeros apart from
 * src_chroma_format has no stage but the sws stage's format conversion: it is mjg_open_src.  The
 * structs the pointers name are read during mjg_open_chain only.  Fields are only ever appended to
 * this struct, and a new field's zero means "as before" (a caller zeroes the struct and sets what
 * it knows).
 *
 * Common to every stage.  cfg->src_w / src_h stay the decoded frame's size whatever the chain holds:
 * mjg_frame_bytes, host submits and device pointers are whole decoded frames.  Every refusal below
 * is MJG_E_INVALID before any HIP call (so on a host without a GPU too), with a message that starts
 * with the prefix given.  The stages in front of the sws stage (deint, orient, cmat, lut_in) work on
 * whole frames in the source format, same bytes per frame, no range conversion, and never write the
 * caller's frames; their launches, lut_out's and the sharpen's are part of the MJG_K_SCALE interval,
 * which any one of them alone opens too.  A stage that is "none" has no buffer and no launch: the
 * context then launches exactly what it would without the field.  All stages but deint work per
 * frame: MJG_F_MERGE, mjg_submit_segments and mjg_submit_halo are unchanged by them.
 *
 * src_chroma_format  (`-pix_fmt`; "src_chroma_format")  The frames are src_w x src_h in this format
 *   (MJG_CHROMA_*), the JPEGs in cfg->chroma_format.  The conversion is swscale's and belongs to the
 *   sws stage: one bicubic pass per plane from the source plane size to the encoded one (default
 *   chroma siting; tv->pc in the same pass; a plane that keeps its size, luma without -vf scale,
 *   goes through one-tap identity filters, which the library runs as a streaming copy with the tv->pc
 *   byte table).  Any pair of formats is accepted; the worker sends the down-sampling pairs
 *   (444->422, 444->420, 422->420).  Formats that differ force the sws stage.  Refused: a value
 *   that is no MJG_CHROMA_*.
 *
 * deint  (`-vf yadif[=0|2]` as the first filter of the graph; "deint")  0, or MJG_DEINT_YADIF |
 *   MJG_DEINT_NOSPATIAL | MJG_DEINT_BFF.  Acts on the decoded frames, every plane filtered alike.
 *   k_yadif_plane (scale.hip, which restates the filter: the C path of FFmpeg's vf_yadif.c /
 *   yadif_common.c as this project's issue text gives it, not checked against an FFmpeg build here;
 *   DESIGN §4.13) writes the deinterlaced frames into a buffer of the launch slot; the orientation
 *   stage, the sws stage, or without either k_encode in place, reads that buffer.  Frame i of a
 *   sequence of n is made from frames max(i - 1, 0), i and min(i + 1, n - 1): n outputs for n
 *   inputs.  On such a context every mjg_submit is a whole sequence and every segment of a
 *   mjg_submit_segments is one (the bytes of one mjg_submit per segment, as ever); a sequence longer
 *   than a submit is handed over with mjg_submit_halo.  The context neither holds nor merges submits:
 *   MJG_F_MERGE is accepted and has no effect, mjg_ctx_queue_depth is mjg_queue_depth().  Refused:
 *   unknown bits, option bits without MJG_DEINT_YADIF, and a source whose luma or chroma plane is
 *   smaller than 3 x 3.
 *
 * orient  (`-vf hflip`, `vflip`, `transpose=N`, any run of them at the front of the graph, behind a
 *   yadif; "orient")  orient = (T ? 1 : 0) | (FX ? 2 : 0) | (FY ? 4 : 0) maps every plane P (w x h) of
 *   the frame, the chroma planes as planes of their own, to
 *       out[y][x] = in'[FY ? H-1-y : y][FX ? W-1-x : x],   in' = T ? transpose(P) : P   (W x H),
 *   so hflip is 2, vflip 4, the half turn 6, transpose=0 (cclock_flip) 1, transpose=1 (clock) 3,
 *   transpose=2 (cclock) 5 and transpose=3 (clock_flip) 7; 0 is none.  Everything behind it -- the
 *   matrix, the tables, the crop rectangle, dst_w / dst_h and the pad -- refers to the oriented frame,
 *   src_h x src_w when orient & 1.  k_orient_plane writes the oriented frames into a buffer of the
 *   launch slot, from the submit's segments or the deinterlacer's buffer; the sws stage, or without
 *   one k_encode in place, reads that buffer.  Refused: an orient outside 0..7, and orient & 1 with a
 *   4:2:2 source (vf_transpose converts such a format first).
 *
 * cmat  (`-vf colormatrix=SRC:DST` behind the yadif and the orientation; "cmatrix")  NULL, or the
 *   identity (0, 0, 65536, 0, 0, 65536), is none.  Acts on whole frames, in front of lut_in, the crop
 *   and the sws stage.  k_cmat_frame (scale.hip) covers all three planes of every frame
 *   of a submit in one launch.  Behind a deinterlacer or an orientation it runs in place in that
 *   stage's buffer (so mjg_debug_oriented, or mjg_debug_deint without an orientation, then return the
 *   converted frames); otherwise it writes the buffer of the launch slot that a lut_in alone would
 *   write, and a lut_in then runs in place there.  Refused: a coefficient outside [-262144, 262144]
 *   (four times unity: every sum then stays below 2^27 and int32 holds it).
 *
 * lut_in  (`-vf eq=...` in front of the scale)  NULL, or three identity tables, is none.  Acts on the
 *   frames that enter the sws stage, or k_encode in place: behind the deinterlacer, the orientation
 *   and the matrix, on whole frames, in front of the crop.  k_lut_plane (scale.hip)
 *   writes them into a buffer of the launch slot, which the sws stage or k_encode then reads.  Behind
 *   a deinterlacer, an orientation or a matrix the stage runs in place in that stage's buffer instead
 *   (so mjg_debug_oriented, or mjg_debug_deint without an orientation, then return the mapped
 *   frames).  A plane whose table is the identity is copied by the same launch, or left alone in
 *   place.  Nothing is refused: every table is valid.
 *
 * has_crop, crop_x, crop_y, crop_w, crop_h  (`-vf crop=w:h:x:y`, alone or before `scale`; "crop")
 *   has_crop 0 is the whole oriented frame and the four values are not read.  Otherwise crop_w x
 *   crop_h luma samples at (crop_x, crop_y) of the oriented frame, its chroma planes at (crop_x >>
 *   hs, crop_y >> vs) with the chroma size of a crop_w x crop_h frame (hs, vs: the source format's
 *   sub-sampling shifts).  No launch of its own: the rectangle is the input of the sws stage, which
 *   runs when crop_w x crop_h != dst_w x dst_h or the formats differ (its filters are made for the
 *   rectangle: the edge taps replicate the crop's edge), and else of k_encode, which then reads the
 *   frames in place.  The full rectangle (0, 0, the oriented size) is has_crop 0, with the same
 *   launches.  MJG_UNALIGNED_FETCH=0 in the environment at open keeps k_encode's aligned-only row
 *   fetch for a crop read in place (misaligned blocks then load byte by byte; A/B runs and tests).
 *   Refused, with a message that names the rectangle: a non-positive size, a rectangle outside the
 *   oriented frame, or a crop_x / crop_y that is not a multiple of the source format's sub-sampling.
 *
 * the sws stage  (`-vf scale=W:H:flags=bicubic`; no field: cfg->dst_w / dst_h)  See mjg_open.  It
 *   runs when the size or the format changes, and whenever a lut_out, a sharpen or a pad needs its
 *   output buffer.
 *
 * lut_out  (`-vf eq=...` directly behind the scale)  NULL, or three identity tables, is none.  Forces
 *   the sws stage, as a pad and a sharpen do, and acts in place on the picture rectangle of its
 *   output (dst_w x dst_h and its chroma size, at the canvas stride under a pad), behind every sws
 *   pass, the pad's border among them, and in front of the sharpen; the border is never mapped.  A
 *   plane whose table is the identity is left alone.  k_lut_plane, as lut_in.  Under a lut_out,
 *   mjg_debug_planes and mjg_debug_presharp return the mapped planes.  Nothing is refused.
 *
 * unsharp  (`unsharp[=lx:ly:la:cx:cy:ca]` behind the scale, in front of the pad; "unsharp")  NULL, or
 *   la == 0 and ca == 0, is none (the sizes of a given struct are checked all the same).  Otherwise
 *   the sws stage always runs, as it does with a pad (a plane that keeps its size goes through
 *   k_plane_copy / k_pad_plane with the tv->pc table), and k_unsharp_plane (scale.hip, which restates
 *   the filter: the 8-bit planar path of FFmpeg's vf_unsharp.c as this project's issue text gives it,
 *   not checked against an FFmpeg build) makes from every plane of its output the same
 *   plane of a second buffer of the launch slot, which k_encode reads:
 *     blur = (sum_j sum_i C(2sy, j) C(2sx, i) P[clamp(y + j - sy)][clamp(x + i - sx)] + half) >> scalebits
 *     out  = clip_uint8(P[y][x] + (((P[y][x] - blur) * amount) >> 16))
 *   with sx = size_x / 2, sy = size_y / 2, scalebits = 2 (sx + sy), half = 1 << (scalebits - 1), the
 *   indices clamped into the picture (dst_w x dst_h; its chroma planes at their own size with cx, cy,
 *   ca) and C int arithmetic.  A plane whose amount is 0 (the default chroma) is copied by the same
 *   launch.  Under a pad the launch covers the canvas: the border is copied and never enters a sum.
 *   Refused: an even size, a size outside 3..23, an amount outside [-2 * 65536, 5 * 65536], and
 *   size_x / 2 + size_y / 2 > 12 for a plane whose amount is not 0: the filter's 32-bit sum would wrap.
 *
 * has_pad, pad_x, pad_y, pad_w, pad_h  (`-vf pad=W:H:x:y` as the last filter; "pad")  has_pad 0 is
 *   no pad and the four values are not read.  Otherwise the JPEGs are pad_w x pad_h with the picture
 *   -- the sws stage's output, cfg->dst_w x dst_h, which stay the picture's size -- at (pad_x, pad_y)
 *   and black everywhere else: Y = 0, Cb = Cr = 128 in the full-range encoder input, for tv and for
 *   full-range sources alike.  mjg_header, the MCU grid and mjg_debug_planes follow the canvas,
 *   mjg_frame_bytes the source.  With a pad the sws stage always runs: a plane whose size changes is
 *   written into the canvas by k_scale / k_scale_stream (rows at the canvas stride), the border by
 *   k_pad_plane, which also copies a plane that keeps its size (through the tv->pc byte table).  The
 *   trivial rectangle (0, 0, dst_w, dst_h) is has_pad 0, with the same launches.  Refused, with a
 *   message that names the pad: a non-positive canvas size or one beyond 16384, a picture outside the
 *   canvas, and, when the rectangle is not the trivial one, a pad_x / pad_y / pad_w / pad_h or a
 *   dst_w / dst_h that is not a multiple of the encoded format's sub-sampling. */
typedef struct mjg_chain {
  int32_t src_chroma_format;                 /* MJG_CHROMA_* of the frames handed over */
  int32_t deint;                             /* MJG_DEINT_* bits; 0: none */
  int32_t orient;                            /* T | FX << 1 | FY << 2; 0: none */
  const mjg_cmatrix *cmat;                   /* NULL or the identity: none */
  const mjg_lut *lut_in;                     /* NULL or three identity tables: none */
  int32_t has_crop, crop_x, crop_y, crop_w, crop_h;  /* has_crop 0: the whole oriented frame, the four values unread */
  const mjg_lut *lut_out;
  const mjg_unsharp *unsharp;                /* NULL, or both amounts 0: none */
  int32_t has_pad, pad_x, pad_y, pad_w, pad_h;       /* has_pad 0: no pad, the four values unread */
} mjg_chain;
/* mjg_open with a filter chain: cfg as for mjg_open, *chain as above.  MJG_E_INVALID ("null
 * argument") for a NULL cfg, chain or out.  (Added without a version step: mjg_version() stays 105,
 * which tests/test_abi.py pins; a caller that may meet an older library looks for the symbol, as
 * _lib.py does.) */
int mjg_open_chain(int device, const mjg_config *cfg, const mjg_chain *chain, mjg_ctx **out);

/* A contact sheet behind the chain (`-vf tile=COLSxROWS:nb_frames:margin:padding` as the last filter;
 * "sheet"): several frames on one picture.  The cell is the sws stage's output (under a sharpen, its
 * output), cfg->dst_w x dst_h, which stay the cell's size as they stay the picture's under a pad.  The
 * JPEGs are sheets of W = cols dst_w + (cols - 1) padding + 2 margin by H = rows dst_h + (rows - 1)
 * padding + 2 margin.  With N = nb_frames (0: cols rows), frame i of a sequence goes to sheet i / N,
 * cell t = i % N, whose place is (margin + (dst_w + padding) (t % cols), margin + (dst_h + padding)
 * (t / cols)), the chroma planes at that place shifted by the encoded format's sub-sampling.  Whatever
 * is not a cell that holds a frame -- the margin, the padding, the cells N .. cols rows - 1 of every
 * sheet, the cells of a sequence's last sheet behind its last frame -- is the pad's black: Y = 0,
 * Cb = Cr = 128 in the full-range encoder input, for tv and for full-range sources alike.
 *   Every submit is a whole sequence, and so is every segment of mjg_submit_segments: a sheet never
 * spans two.  max_batch and every nframes count input frames; a submit of n frames yields
 * mjg_frames_out(ctx, n) = ceil(n / N) JPEGs (a segment list: the sum over its segments, each
 * segment's sheets behind those of the one before).  mjg_sync's frame_sizes has that many entries, and
 * mjg_fetch, mjg_output_device's offsets, mjg_debug_coefs and mjg_debug_planes index sheets;
 * mjg_debug_cell and the debug readbacks of the stages in front (mjg_debug_presharp, mjg_debug_deint,
 * ...) index input frames.  mjg_header, the MCU grid and mjg_debug_planes follow the sheet,
 * mjg_frame_bytes the source.  RST and -huffman optimal work per sheet.
 *   Like a deinterlacer context a sheet context neither holds nor merges submits: MJG_F_MERGE is
 * accepted and has no effect.  A sheet composes with a deinterlacer and mjg_submit_halo, whose nframes
 * are the encoded input frames as without one.  With a sheet the sws stage always runs, as under a pad
 * or a sharpen; k_tile_plane reads its buffer (the sharpen's) and writes the sheets, which k_encode
 * then reads.  Its launches are part of the MJG_K_SCALE interval.
 *   NULL, or a sheet of one cell without margin (cols = rows = 1, nb_frames 0 or 1, margin 0), is
 * exactly mjg_open_chain: the context launches what it launches without a sheet.
 *   Refused with MJG_E_INVALID and a message that starts with "sheet", before any HIP call: cols or
 * rows below 1, nb_frames below 0 or above cols rows, a negative margin or padding, a sheet side
 * above 16384, a pad in the chain (one that is not the trivial rectangle), and a dst_w, dst_h, margin
 * or padding that is not a multiple of the encoded format's sub-sampling.  The chain's own refusals
 * come first.  (Added without a version step, as mjg_open_chain.) */
typedef struct mjg_sheet { int32_t cols, rows, nb_frames, margin, padding; } mjg_sheet;
int mjg_open_sheet(int device, const mjg_config *cfg, const mjg_chain *chain, const mjg_sheet *sheet, mjg_ctx **out);
/* A denoiser behind the deinterlacer (`-vf hqdn3d` as the very first filter, or directly behind a leading
 * yadif; "denoise"): the chain's first recursive filter.  The library knows tables, not the filter, as mjg_lut
 * does: four tables of 8192 int16, the luma and chroma spatial ones (ls, cs) and the luma and chroma temporal
 * ones (lt, ct); profile.hqdn3d_tables makes them from the filter's four strengths.  With L(v) = (v << 8) + 127
 * and c(tab, a, b) = b + tab[4096 + ((a - b) >> 4)] (C int, arithmetic shift; the index clamped into 0..8191
 * before it is used), every plane s (w x h; Y with S = ls, M = lt; U and V each with S = cs, M = ct, at their
 * own size) of frame t of a sequence becomes
 *     P[y][0] = y ? L(s[y][0]) : c(S, L(s[0][0]), L(s[0][0]));   P[y][x] = c(S, P[y][x-1], L(s[y][x]))
 *     V[0][x] = P[0][x];                                          V[y][x] = c(S, V[y-1][x], P[y][x])
 *     A_t[y][x] = c(M, A_{t-1}[y][x], V_t[y][x]),  A_{-1} = L(s_0);   out_t[y][x] = A_t[y][x] >> 8
 * (k_dn_rows, k_dn_cols, k_dn_time in scale.hip).  This restates the 8-bit C path of FFmpeg's
 * vf_hqdn3d.c from memory; no FFmpeg build has been compared with it yet.  n outputs
 * for n inputs, same bytes per frame, no range conversion.  Values stay within uint16 for the tables the
 * filter makes; with other tables they wrap, and no table can make an address outside a buffer.
 *   The stage order is deint -> denoise -> orient -> cmat -> lut_in -> ...  The stage works on whole decoded
 * frames in the source format and never writes the caller's frames: it writes the denoised frames into a
 * buffer of the launch slot, which the next stage reads the way it reads the deinterlacer's: cmat and lut_in
 * run in place in it (mjg_debug_denoise then returns the converted / mapped frames), and the orientation, the
 * sws stage, or without either k_encode in place read it.  Its launches are part of the MJG_K_SCALE interval.
 * Each launch slot holds a uint16 buffer of max_batch frames (P, then V) beside that byte buffer, and the
 * context one uint16 frame: A, the state of the time scan.
 *   Sequences.  On such a context every mjg_submit, every mjg_submit_halo and every segment of a
 * mjg_submit_segments is a sequence of its own, behind a deinterlacer too: its first frame starts the time scan
 * from its own samples.
 * mjg_submit_cont continues the sequence of the submit before.  Like a deinterlacer context it neither holds
 * nor merges submits: MJG_F_MERGE is accepted and has no effect.  Submits on the two launch slots run on
 * streams of their own; the state is ordered by an event behind each submit's time scan that the next
 * submit's stream waits for, so submits may be queued without a sync in between.
 *   A NULL dn is exactly mjg_open_sheet.  Refused with MJG_E_INVALID and a message that starts with "denoise",
 * before any HIP call: a sheet (one that is not the trivial one) together with a denoiser.  The chain's and the
 * sheet's own refusals come first.  mjg_config cannot describe samples of more than 8 bits, so there is nothing
 * to refuse there: the caller keeps such inputs away (worker.denoise_fallthrough_reason).  (Added without a
 * version step, as mjg_open_chain.) */
typedef struct mjg_denoise { int16_t ls[8192], cs[8192], lt[8192], ct[8192]; } mjg_denoise;
int mjg_open_denoise(int device, const mjg_config *cfg, const mjg_chain *chain, const mjg_sheet *sheet,
                     const mjg_denoise *dn, mjg_ctx **out);
/* JPEGs a submit (or one segment of mjg_submit_segments) of nframes frames yields: nframes without
 * a sheet, ceil(nframes / N) with one.  0 for a NULL ctx or nframes below 1. */
int mjg_frames_out(const mjg_ctx *ctx, int nframes);

/* The entry points from before mjg_chain.  Each is mjg_open_chain with the chain it names: the
 * fields not listed are zero, and a rectangle that is listed always has its has_crop / has_pad set,
 * so a caller without a crop or a pad passes the full rectangle (0, 0, the oriented size) or the
 * trivial one (0, 0, dst_w, dst_h). */
/* {src_chroma_format}; mjg_open(d, cfg, out) = mjg_open_src(d, cfg, cfg->chroma_format, out).
 * (mjg_version() >= 101.) */
int mjg_open_src(int device, const mjg_config *cfg, int src_chroma_format, mjg_ctx **out);
/* {src_chroma_format, crop}: a crop and no pad.  (mjg_version() >= 102.) */
int mjg_open_crop(int device, const mjg_config *cfg, int src_chroma_format,
                  int crop_x, int crop_y, int crop_w, int crop_h, mjg_ctx **out);
/* {src_chroma_format, crop, pad}.  (mjg_version() >= 104.) */
int mjg_open_pad(int device, const mjg_config *cfg, int src_chroma_format,
                 int crop_x, int crop_y, int crop_w, int crop_h,
                 int pad_x, int pad_y, int pad_w, int pad_h, mjg_ctx **out);
/* {src_chroma_format, orient, crop, pad}.  (This one and those below: added without a version
 * step, as mjg_open_chain.) */
int mjg_open_orient(int device, const mjg_config *cfg, int src_chroma_format, int orient,
                    int crop_x, int crop_y, int crop_w, int crop_h,
                    int pad_x, int pad_y, int pad_w, int pad_h, mjg_ctx **out);
/* {src_chroma_format, deint, orient, crop, pad}. */
int mjg_open_deint(int device, const mjg_config *cfg, int src_chroma_format, int deint, int orient,
                   int crop_x, int crop_y, int crop_w, int crop_h,
                   int pad_x, int pad_y, int pad_w, int pad_h, mjg_ctx **out);
/* {src_chroma_format, deint, orient, crop, unsharp = us, pad}. */
int mjg_open_sharp(int device, const mjg_config *cfg, int src_chroma_format, int deint, int orient,
                   int crop_x, int crop_y, int crop_w, int crop_h, const mjg_unsharp *us,
                   int pad_x, int pad_y, int pad_w, int pad_h, mjg_ctx **out);
/* {src_chroma_format, deint, orient, lut_in, crop, lut_out, unsharp = us, pad}. */
int mjg_open_lut(int device, const mjg_config *cfg, int src_chroma_format, int deint, int orient,
                 int crop_x, int crop_y, int crop_w, int crop_h,
                 const mjg_lut *lut_in, const mjg_lut *lut_out, const mjg_unsharp *us,
                 int pad_x, int pad_y, int pad_w, int pad_h, mjg_ctx **out);
/* {src_chroma_format, deint, orient, cmat = cm, lut_in, crop, lut_out, unsharp = us, pad}: every
 * field. */
int mjg_open_cmat(int device, const mjg_config *cfg, int src_chroma_format, int deint, int orient,
                  int crop_x, int crop_y, int crop_w, int crop_h, const mjg_cmatrix *cm,
                  const mjg_lut *lut_in, const mjg_lut *lut_out, const mjg_unsharp *us,
                  int pad_x, int pad_y, int pad_w, int pad_h, mjg_ctx **out);
void mjg_close(mjg_ctx *ctx);

/* Bytes of one packed planar input frame (src_w x src_h in the source chroma format). */
size_t mjg_frame_bytes(const mjg_ctx *ctx);
/* The per-config JPEG header (SOI .. SOS) every frame starts with.  With
 * MJG_F_HUFFMAN_OPTIMAL each frame carries its own DHT; this returns the header with the
 * default tables (same layout, different DHT contents). */
int mjg_header(const mjg_ctx *ctx, uint8_t *out, size_t cap, size_t *len);

/* Encode `nframes` (<= max_batch) packed I420 frames, asynchronously: H2D, scale and
 * k_encode on a launch slot's stream, the scan/stuff/write tail on the ctx's tail stream
 * after the launch's k_encode.  mjg_queue_depth() launches may be queued (each has its own
 * output and scratch buffers and its own stream): the next one's k_encode runs beside the
 * previous one's drain and tail.  src_is_device = 0: `frames` is host memory (copied H2D
 * through the slot's staging buffer; pinned memory from mjg_host_alloc() makes this
 * asynchronous), a launch of its own; src_is_device = 1: `frames` is device memory on ctx's
 * device, read in place.  Without MJG_F_MERGE every submit is launched (stream-ordered) inside
 * this call.  With MJG_F_MERGE (opt-in; MJG_MERGE=1 in the environment turns it off again) a
 * device submit is held and launched together with the next device submit, as one segment
 * list (mjg_submit_segments' kernels), or alone when the caller syncs it; each submit stays a
 * job of its own for mjg_sync / mjg_fetch with exactly the bytes of an unmerged launch.  A held
 * submit's kernels read its frames after this call returns, so with MJG_F_MERGE the frames must
 * stay valid and unchanged until the job is synced (stream order on the caller's side does not
 * protect them).  Up to mjg_ctx_queue_depth(ctx) device submits may be pending; MJG_E_STATE
 * past that (or when no launch slot is free for a host submit).
 * Replaces the per-segment encode the reference runs at ffmpeg_distributed.py:139-141. */
int mjg_submit(mjg_ctx *ctx, const uint8_t *frames, int nframes, int src_is_device);
/* mjg_submit for a piece of a longer sequence, on a context with a deinterlacer: halo bit 1,
 * `frames` starts with one extra frame that is only read (the first encoded frame's `prev`); bit
 * 2, one extra frame follows the last encoded one (its `next`).  nframes counts the encoded frames
 * only (<= max_batch); a host submit copies nframes plus the halo frames (its staging holds
 * max_batch + 2).  The kernel reads no frame outside [first encoded - (halo & 1), last encoded +
 * (halo >> 1)].  halo 0 is mjg_submit; a non-zero halo on a context without a deinterlacer, or one
 * outside 0..3, is MJG_E_INVALID.  (With mjg_open_deint.) */
int mjg_submit_halo(mjg_ctx *ctx, const uint8_t *frames, int nframes, int src_is_device, int halo);
/* mjg_submit_halo for a piece of a longer sequence on a context with a denoiser (mjg_open_denoise): with
 * cont != 0 the frames continue the sequence of the previous submit on this context, so the time scan starts
 * from the carried state and not from the first frame.  cont 0 is mjg_submit_halo.  It composes with a
 * deinterlacer: the halo frames feed yadif, and the denoiser sees the nframes deinterlaced frames.  A
 * non-zero cont on a context without a denoiser, or before any submit on it, is MJG_E_INVALID.  (With
 * mjg_open_denoise.) */
int mjg_submit_cont(mjg_ctx *ctx, const uint8_t *frames, int nframes, int src_is_device, int halo, int cont);
/* Several segments in one submit: segment k's seg_nframes[k] packed I420 frames at device
 * pointer seg_frames[k] (on ctx's device), nsegs in 1..mjg_max_segments(), the total within
 * max_batch.  One launch of each kernel (the sws stage's, k_encode, the tail) covers all
 * of them, so the launch's ramp and drain are paid once; the output is the frames in segment
 * order, exactly the bytes of one mjg_submit per segment.  The resident encoder / a GPU worker
 * with several segments queued on one GPU (ffmpeg_distributed.py:139-141 once per segment)
 * hands them over together. */
int mjg_submit_segments(mjg_ctx *ctx, const uint8_t *const *seg_frames, const int *seg_nframes, int nsegs);
/* Most segments one mjg_submit_segments() may carry (4). */
int mjg_max_segments(void);
/* Wait for the oldest pending submit (with none pending: report the last synced one again;
 * a held one is launched first).
 * frame_sizes (may be NULL) receives its nframes JPEG sizes; *total (may be NULL) the packed
 * total.  Grows the output buffer and re-runs the final kernel if the packed output
 * exceeded its capacity. */
int mjg_sync(mjg_ctx *ctx, uint64_t *frame_sizes, uint64_t *total);
/* Copy the packed JPEGs of the last synced submit (frame after frame) to host memory; syncs
 * the oldest queued submit first when mjg_sync was not called since the last mjg_submit.
 * Page-locked `out` (from mjg_host_alloc) receives them by one DMA; pageable memory through
 * the context's page-locked buffer (mjg_fetch_host) and one host copy. */
int mjg_fetch(mjg_ctx *ctx, uint8_t *out, size_t cap);
/* The same bytes without the copy into caller memory: *data points at the context's
 * page-locked copy (DMA'd from the device), *len its size; valid until the next
 * mjg_fetch / mjg_fetch_host or mjg_close. */
int mjg_fetch_host(mjg_ctx *ctx, const uint8_t **data, size_t *len);
/* Device pointers of the packed output and of the per-frame byte offsets (nframes+1
 * entries, valid after mjg_sync). */
int mjg_output_device(mjg_ctx *ctx, const uint8_t **data, const uint64_t **offsets);
/* The hipStream_t the next submit launches H2D, scale and k_encode on (for event timing by
 * the caller; the tail kernels run on another stream ordered after k_encode).  Consecutive
 * submits rotate over mjg_queue_depth() such streams. */
void *mjg_stream(mjg_ctx *ctx);
/* How many launches may be queued before one must be synced (2): the depth for host submits
 * and mjg_submit_segments, which each take a launch of their own. */
int mjg_queue_depth(void);
/* How many single-segment device submits (mjg_submit, src_is_device = 1) ctx holds pending
 * before one must be synced: with MJG_F_MERGE mjg_queue_depth() launches of up to two merged
 * submits each (4), else mjg_queue_depth(). */
int mjg_ctx_queue_depth(const mjg_ctx *ctx);

/* Pinned host memory for mjg_submit / mjg_fetch. */
int mjg_host_alloc(size_t bytes, void **ptr);
int mjg_host_free(void *ptr);

/* Per-frame histograms of decoded frames (k_frame_hist), what `-vf thumbnail` selects its frames by.
 * An object of its own, not a stage of a context: the worker's reader thread counts while its submit
 * thread owns the mjg_ctx, and one ctx belongs to one thread.  It knows histograms, not the filter, as
 * mjg_lut knows tables: the selection (FFmpeg's vf_thumbnail.c, restated in DESIGN §4.18 and profile.py's
 * thumbnail_pick; no FFmpeg build has been compared with it yet) is the caller's.
 *   Frames are w x h, 8 bits, packed planar in chroma_format (MJG_CHROMA_*), the decoder's bytes with
 * no range conversion, frame_bytes apart at any byte alignment.  hist[f][256 p + v] is the number of
 * samples of value v in plane p (0 Y, 1 U, 2 V) of frame f, each plane at its own size.
 *   The object owns a stream, a device buffer of max_frames frames for host input, and the device and
 * page-locked histogram buffers.  mjg_hist_frames is synchronous: H2D copy (asynchronous from
 * mjg_host_alloc memory; src_is_device: none, the frames are read where they lie), zero, one launch,
 * D2H copy, wait; every call starts from zero.  It touches no mjg_ctx and may run beside one's calls
 * from another thread; one mjg_hist per caller thread.
 *   MJG_E_INVALID with a message that starts with "hist", before any HIP call: a null pointer, w or h
 * outside 1..16384, a chroma_format that is no MJG_CHROMA_* value, max_frames below 1 (or so many that
 * workgroups per frame x frames passes 2^31 - 1), nframes outside 1..max_frames.  (Added without a
 * version step, as mjg_open_chain.) */
typedef struct mjg_hist mjg_hist;
int mjg_hist_open(int device, int w, int h, int chroma_format, int max_frames, mjg_hist **out);
int mjg_hist_frames(mjg_hist *h, const uint8_t *frames, int nframes, int src_is_device,
                    uint32_t *hist /* host, [nframes][768] */);
void mjg_hist_close(mjg_hist *h);

/* Average device time (ms) per launch of each kernel (MJG_K_*) since the last reset,
 * and the number of submits it was averaged over.  Needs MJG_F_TIMING. */
int mjg_kernel_times(mjg_ctx *ctx, double *ms /* [MJG_NUM_KERNELS] */, int *launches, int reset);

/* Device-free helpers (no HIP call; usable on a host without a GPU). */
/* The per-config JPEG header (SOI .. SOS) for cfg (dst_w/dst_h/qscale/sar/chroma_format and the
 * MJG_F_COM_ITU601 / MJG_F_RST flags are read). */
int mjg_build_header(const mjg_config *cfg, uint8_t *out, size_t cap, size_t *len);
/* swscale bicubic filter table the scale stage applies: one = 1<<14 (horizontal) or 1<<12
 * (vertical); align = 4 / 2 (x86 swscale); pos = swscale local position (128 = centred).
 * coeff receives dst_len*taps int16, pos_out dst_len int32; query taps with coeff == NULL. */
int mjg_sws_filter(int src_len, int dst_len, int one, int align, int bitexact, int src_pos,
                   int dst_pos, int16_t *coeff, size_t coeff_cap, int32_t *pos_out, int *taps);

/* Test hooks (tests/ only). */
/* Quantized coefficients (natural order) of frame `frame` of the last submit, blocks
 * in coding order (4:2:0: Y0 Y1 Y2 Y3 Cb Cr per MCU).  Needs MJG_F_DEBUG_COEFS. */
int mjg_debug_coefs(mjg_ctx *ctx, int frame, int16_t *out, size_t nblocks);
/* The full-range encoder-input planes (after scale/range stage) of frame `frame`,
 * packed planar at dst size (under a pad: the canvas size) in the encoded chroma format.  Only for a config whose sws stage
 * runs (src size != dst size, or source chroma format != encoded one).  Under a sharpen
 * (mjg_open_sharp) these are the sharpened planes, k_unsharp_plane's output. */
int mjg_debug_planes(mjg_ctx *ctx, int frame, uint8_t *out, size_t cap);
/* The sws stage's output under a sharpen (k_unsharp_plane's input; layout as mjg_debug_planes).
 * MJG_E_STATE for a context without a sharpen.  (With mjg_open_sharp.) */
int mjg_debug_presharp(mjg_ctx *ctx, int frame, uint8_t *out, size_t cap);
/* 1 and the context's sheet in *out (which may be NULL; nb_frames resolved: 0 has become cols rows)
 * when it has one, 0 without (mjg_open_chain, a NULL or a trivial sheet), or a negative MJG_E_* code
 * for a null context.  Host state only.  (With mjg_open_sheet.) */
int mjg_debug_sheet(mjg_ctx *ctx, mjg_sheet *out);
/* k_tile_plane's input frame `frame` of the last synced submit, an input frame of it: the cell, packed
 * planar at dst size in the encoded chroma format, full range (under a sharpen the sharpened planes).
 * Under a sheet mjg_debug_planes returns sheet `frame` instead.  MJG_E_STATE for a context without a
 * sheet.  (With mjg_open_sheet.) */
int mjg_debug_cell(mjg_ctx *ctx, int frame, uint8_t *out, size_t cap);
/* 1 and the context's sizes and amounts in *out (which may be NULL) when it has a sharpen, 0
 * without one, or a negative MJG_E_* code for a null context.  Host state only.  (With
 * mjg_open_sharp.) */
int mjg_debug_unsharp(mjg_ctx *ctx, mjg_unsharp *out);
/* 1 and the tables of slot 0 ("in") or 1 ("out") in *out (which may be NULL) when the context has
 * them, 0 without (none given, or three identity tables), or a negative MJG_E_* code.  Host state
 * only.  (With mjg_open_lut.) */
int mjg_debug_lut(mjg_ctx *ctx, int slot, mjg_lut *out);
/* k_lut_plane's slot-"in" output for frame `frame` of the last synced submit: a whole frame in the
 * source format (behind the orientation: the oriented one), from wherever the stage left it.
 * MJG_E_STATE for a context without a lut_in.  Under a lut_out, mjg_debug_planes and
 * mjg_debug_presharp return the mapped planes.  (With mjg_open_lut.) */
int mjg_debug_lut_in(mjg_ctx *ctx, int frame, uint8_t *out, size_t cap);
/* 1 and the colour matrix in *out (which may be NULL) when the context has one, 0 without (none
 * given, or the identity), or a negative MJG_E_* code for a null context.  Host state only.  (With
 * mjg_open_cmat.) */
int mjg_debug_cmat(mjg_ctx *ctx, mjg_cmatrix *out);
/* k_cmat_frame's output for frame `frame` of the last synced submit: a whole frame in the source
 * format (behind the orientation: the oriented one), from wherever the stage left it.  A lut_in
 * runs in place behind the stage, so with one these are the mapped frames.  MJG_E_STATE for a
 * context without a matrix.  (With mjg_open_cmat.) */
int mjg_debug_cmat_out(mjg_ctx *ctx, int frame, uint8_t *out, size_t cap);
/* Which kernel the sws stage runs for a plane (0 = luma, 1 = chroma): 0 no sws stage for it (the
 * context has none), 1 k_plane_copy (the plane keeps its size), 2 k_scale (one LDS tile per 64-column
 * tile: down to about 4:1), 3 k_scale_stream (any ratio whose filters stay below 256 taps, about
 * 64:1; also every resized plane with MJG_SCALE_STREAM=1 in the environment at open, for A/B runs
 * and tests), 4 k_pad_plane (the plane keeps its size under a pad: copied into the canvas with its
 * border; mjg_version() >= 104).  A negative MJG_E_* code for a bad argument.  (mjg_version() >= 103.) */
int mjg_debug_scale_path(mjg_ctx *ctx, int plane);
/* Which k_encode the context launches, as bits: 1 k_encode reads the source frames in place (no
 * sws stage: same size, same format, no pad; under a crop the rectangle at the source's strides),
 * 2 the UA instantiation (fetch_rows at any alignment: a crop read in place with a plane offset,
 * a row stride or the frame stride that is no multiple of 8, unless MJG_UNALIGNED_FETCH=0 at
 * open).  A negative MJG_E_* code for a null context.  Host state only.  (mjg_version() >= 105.) */
int mjg_debug_encode_path(mjg_ctx *ctx);
/* The oriented frame (k_orient_plane's output: packed planar, mjg_frame_bytes bytes, the oriented
 * size in the source format) of frame `frame` of the last synced submit.  MJG_E_STATE for a
 * context without orientation.  (With mjg_open_orient.) */
int mjg_debug_oriented(mjg_ctx *ctx, int frame, uint8_t *out, size_t cap);
/* The orientation of the context (0..7; mjg_open_orient), or a negative MJG_E_* code for a null
 * context.  Host state only.  (With mjg_open_orient.) */
int mjg_debug_orient(mjg_ctx *ctx);
/* The deinterlaced frame (k_yadif_plane's output: packed planar, mjg_frame_bytes bytes, the decoded
 * size in the source format) of frame `frame` of the last synced submit.  MJG_E_STATE for a
 * context without a deinterlacer.  (With mjg_open_deint.) */
int mjg_debug_deint(mjg_ctx *ctx, int frame, uint8_t *out, size_t cap);
/* The denoised frame (k_dn_time's output: packed planar, mjg_frame_bytes bytes, the decoded size in the
 * source format; converted / mapped when a cmat or a lut_in ran in place behind the stage) of frame `frame`
 * of the last synced submit.  MJG_E_STATE for a context without a denoiser.  (With mjg_open_denoise.) */
int mjg_debug_denoise(mjg_ctx *ctx, int frame, uint8_t *out, size_t cap);
/* The carried state of the time scan, A of the last frame submitted: mjg_frame_bytes uint16 values, packed
 * planar like a frame (cap counts values).  Every pending submit is synced first.  MJG_E_STATE for a context
 * without a denoiser.  (With mjg_open_denoise.) */
int mjg_debug_denoise_state(mjg_ctx *ctx, uint16_t *out_u16, size_t cap);
/* The context's `deint` value (mjg_open_deint; 0 without a deinterlacer), or a negative MJG_E_*
 * code for a null context.  Host state only.  (With mjg_open_deint.) */
int mjg_debug_deint_flags(mjg_ctx *ctx);
/* Filter tables the context generated: plane 0 = luma, 1 = chroma; dir 0 = horizontal,
 * 1 = vertical.  taps/len may be queried with coeff == NULL.  As mjg_debug_planes: only when
 * the sws stage runs. */
int mjg_debug_filter(mjg_ctx *ctx, int plane, int dir, int16_t *coeff, int32_t *pos,
                     int *taps, int *len);
/* -huffman optimal's table builder (k_huff_build) on given symbol counts, on GPU `device`:
 * hist[f][544] (AC luma 0-255, AC chroma 256-511, DC luma 512-527, DC chroma 528-543) for
 * nframes frames -> dht[f][t][272] (BITS[1..16] then HUFFVAL; t: 0 DC luma, 1 DC chroma,
 * 2 AC luma, 3 AC chroma) and nval[f][t] (HUFFVAL entries).  Replaces the table build of
 * ff_mjpeg_encode_huffman_close (libavcodec/mjpegenc_huffman.c); tests compare it with the oracle. */
int mjg_debug_huff_build(int device, const uint32_t *hist, int nframes, uint8_t *dht, uint32_t *nval);
/* The stuffing tail (k_scan_bits or k_scan_bits_seg, k_count_ff, k_scan_ff, k_write: a submit's launches
 * after k_encode, same blocks and grids) on given chunks, on GPU `device`: no context, buffers of its
 * own, the default stream.  The scratch image is built on the host: every slot word `fill`, then each
 * chunk's words at the start of its slot.
 * Domain, as k_encode leaves its chunks (64 blocks of 2 bits or more): no chunk of 0 bits, and
 * every chunk but its segment's last has 32 bits or more, so that it covers the start of a word of the
 * segment (a word belongs to the chunk that holds its first bit).  A length above the slot's bits is
 * accepted, and clamped by the scan as in a submit; `words` then holds the slot's words.  At most
 * MJG_TAIL_MAX_SLOTS chunks in all.  What is outside the domain, a null pointer or a size below 1 is
 * MJG_E_INVALID with a message, before any HIP call (so on a host without a GPU too).
 * out: out_cap + MJG_TAIL_GUARD bytes, all 0xA5 before k_write and all copied back, so a byte written
 * past a frame's end, past out_cap or into a frame k_write refused shows.  frame_offsets: nframes + 1.
 * group_ff: NULL, or k_count_ff's 0xFF count per group of 32 chunks (nframes * nseg *
 * ceil(nchunks / 32)).  *status: k_write's overflow flag (1: a frame ended past out_cap).  The
 * counters and the flag the scan kernel zeroes in a submit are non-zero before it here; a unit counter
 * it leaves non-zero is MJG_E_STATE. */
typedef struct mjg_tail_job {
  int32_t nframes, nseg, nchunks; /* nseg entropy-coded segments a frame (1: no RST; above 1:
                                     k_scan_bits_seg, segment sizes and offsets, RSTn), nchunks
                                     chunks a segment */
  const uint32_t *chunk_bits;     /* [nframes * nseg * nchunks] bit lengths (unclamped) */
  const uint32_t *words;          /* the chunks' slot words, chunk after chunk: ceil(min(L, slot
                                     bits) / 32) words each, bits MSB first, zero past the last bit */
  uint32_t fill;                  /* every other word of the scratch image */
  const uint8_t *hdr;             /* the bytes every frame starts with */
  int32_t hdr_len;                /* 1..65536 */
  const uint8_t *dht;             /* NULL, or -huffman optimal's tables a frame, as k_huff_build */
  const uint32_t *nval;           /* leaves them: dht[f][4][272], nval[f][4] (each <= 256); hdr then */
  int32_t dht_pos, dht_end;       /* holds the default DHT (420 bytes) at [dht_pos, dht_end) */
  uint64_t out_cap;               /* k_write's capacity (<= 2^30) */
} mjg_tail_job;
#define MJG_TAIL_GUARD 64
#define MJG_TAIL_MAX_SLOTS 8192
int mjg_debug_tail(int device, const mjg_tail_job *job, uint8_t *out, uint64_t *frame_offsets,
                   uint32_t *group_ff, uint32_t *status);

#ifdef __cplusplus
}
#endif
#endif /* MJGPU_H */
