// C-ABI of libmjgpu.so (declarations and boundary citations: include/mjgpu.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "mjgpu.h"
#include "jpeg_tables.h"
#include "kernels.hip"
#include "scale.hip"
#include "sws_filter.h"

using namespace mjg;

namespace {

thread_local std::string g_err = "no error";

int set_err(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) return set_err(MJG_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// JPEG header of the profile: mjpegenc_common.c ff_mjpeg_encode_picture_header for
// AV_CODEC_ID_MJPEG, -bitexact (no COM), equal luma/chroma matrices (one DQT), DRI only
// with slice threading (RST mode), -huffman default (one DHT with DC0, DC1, AC0, AC1);
// SOF0 sampling factors from ff_mjpeg_init_hvsample.
struct ByteWriter {
  std::vector<uint8_t> b;
  void u8(int v) { b.push_back((uint8_t)v); }
  void u16(int v) { u8(v >> 8); u8(v); }
};

// (h, v) sampling factors of Y, Cb, Cr (ff_mjpeg_init_hvsample; 4:4:4 is all 1x2).
void hvsample(int cfmt, int hs[3], int vs[3]) {
  if (cfmt == MJG_CHROMA_444) {
    hs[0] = hs[1] = hs[2] = 1;
    vs[0] = vs[1] = vs[2] = 2;
    return;
  }
  hs[0] = vs[0] = 2;
  hs[1] = hs[2] = 1;
  vs[1] = vs[2] = cfmt == MJG_CHROMA_422 ? 2 : 1;
}

std::vector<uint8_t> build_header(int w, int h, const uint8_t mprime[64], int sar_num, int sar_den,
                                  bool com_itu601, int cfmt, bool rst, size_t *dht_pos = nullptr,
                                  size_t *dht_end = nullptr) {
  int hs[3], vs[3];
  hvsample(cfmt, hs, vs);
  ByteWriter o;
  o.u16(0xFFD8);
  if (sar_num > 0 && sar_den > 0) {
    o.u16(0xFFE0);
    o.u16(16);
    for (char c : {'J', 'F', 'I', 'F', '\0'}) o.u8(c);
    o.u16(0x0102);
    o.u8(0);
    o.u16(sar_num);
    o.u16(sar_den);
    o.u8(0);
    o.u8(0);
  }
  if (com_itu601) {  // jpeg_put_comments: COM "CS=ITU601" when the encoder pix_fmt is yuv420p
    o.u16(0xFFFE);
    o.u16(12);
    for (char ch : {'C', 'S', '=', 'I', 'T', 'U', '6', '0', '1', '\0'}) o.u8(ch);
  }
  o.u16(0xFFDB);
  o.u16(2 + 65);
  o.u8(0x00);
  for (int i = 0; i < 64; i++) o.u8(mprime[kZigzag[i]]);
  if (rst) {  // jpeg_table_header: DRI, interval = MCUs per MCU row
    o.u16(0xFFDD);
    o.u16(4);
    o.u16((w - 1) / (8 * hs[0]) + 1);
  }
  if (dht_pos) *dht_pos = o.b.size();
  o.u16(0xFFC4);
  const size_t len_at = o.b.size();
  o.u16(0);
  auto table = [&](int cls_id, const uint8_t *bits, const uint8_t *vals) {
    o.u8(cls_id);
    int n = 0;
    for (int i = 1; i <= 16; i++) {
      o.u8(bits[i]);
      n += bits[i];
    }
    for (int i = 0; i < n; i++) o.u8(vals[i]);
  };
  table(0x00, kBitsDcLum, kValDc);
  table(0x01, kBitsDcChr, kValDc);
  table(0x10, kBitsAcLum, kValAcLum);
  table(0x11, kBitsAcChr, kValAcChr);
  const size_t dht_len = o.b.size() - len_at;
  o.b[len_at] = (uint8_t)(dht_len >> 8);
  o.b[len_at + 1] = (uint8_t)dht_len;
  if (dht_end) *dht_end = o.b.size();
  o.u16(0xFFC0);
  o.u16(17);
  o.u8(8);
  o.u16(h);
  o.u16(w);
  o.u8(3);
  for (int c = 0; c < 3; c++) {
    o.u8(c + 1);
    o.u8((hs[c] << 4) | vs[c]);
    o.u8(0);
  }
  o.u16(0xFFDA);
  o.u16(12);
  o.u8(3);
  o.u8(1); o.u8(0x00);
  o.u8(2); o.u8(0x11);
  o.u8(3); o.u8(0x11);
  o.u8(0); o.u8(63); o.u8(0);
  return o.b;
}

template <typename T>
int dmalloc(T **p, size_t count) {
  *p = nullptr;
  if (count == 0) return MJG_OK;
  if (hipMalloc((void **)p, count * sizeof(T)) != hipSuccess) {
    *p = nullptr;
    (void)hipGetLastError();
    return set_err(MJG_E_NOMEM, "hipMalloc(%zu bytes) failed", count * sizeof(T));
  }
  return MJG_OK;
}

// ceil(2^40 / d) for k_encode's task index (EncGeom); scale.hip's magic32 is ceil(2^32 / d)
unsigned long long magic40(unsigned long long d) { return (((unsigned long long)1 << 40) + d - 1) / d; }

// mpegvideo_enc.c encode_picture FMT_MJPEG matrix + ff_convert_matrix (qscale -> 8); qmat may be null
void quant_matrix(int qscale, uint8_t mprime[64], int32_t *qmat) {
  for (int i = 0; i < 64; i++) {
    const int v = std::min(255, i == 0 ? 8 : ((kMpeg1Intra[i] * qscale) >> 3));
    mprime[i] = (uint8_t)v;
    if (qmat) qmat[i] = (int32_t)((2ull << 21) / (uint64_t)(16 * v));
  }
}

// all of a launch's frames in one buffer: one segment at p
SegList one_seg(const uint8_t *p) {
  SegList sl;
  for (int k = 0; k < kMaxSegs; k++) sl.p[k] = p, sl.f0[k] = k ? INT_MAX : 0;
  return sl;
}

// a launch's frames in one buffer, frame f at p + f * frame_bytes, with the segment starts of `in`: for a stage
// that reads another stage's buffer and still treats every segment as a sequence of its own
SegList seg_starts(const SegList &in, const uint8_t *p, size_t frame_bytes) {
  SegList sl;
  for (int k = 0; k < kMaxSegs; k++) {
    const bool used = in.f0[k] != INT_MAX;
    sl.f0[k] = in.f0[k];
    sl.p[k] = used ? p + (size_t)in.f0[k] * frame_bytes : p;
  }
  return sl;
}

// an environment switch, read at open
int env_int(const char *name, int unset) {
  const char *e = getenv(name);
  return e ? atoi(e) : unset;
}

bool is_tail_kernel(int k) { return k == MJG_K_SCAN_BITS || k == MJG_K_COUNT_FF || k == MJG_K_SCAN_FF || k == MJG_K_WRITE; }

struct PlaneScale {
  SwsFilter hf, vf;
  int32_t *hcp = nullptr, *hp = nullptr, *vcp = nullptr, *vps = nullptr, *hsum = nullptr;
  int32_t *mfb = nullptr;  // k_scale's matrix-core h-pass: the B fragments (ScaleGeom::mf_*)
  bool d4 = false;  // h coefficients in the v_dot4 hi/lo byte layout (k_scale D4)
  ScaleGeom g{};    // the plane's sizes and strides (plan_geometry) and its filters' fields (plan_plane_scale)
  size_t lds = 0;
  dim3 grid;
  int th = 32;  // k_scale tile height (64: the 2:1 filters, scale.hip)
  bool copy = false;  // the plane keeps its size: k_plane_copy instead of k_scale's identity filters
  bool stream = false;  // k_scale_stream: the tile's window does not fit LDS (or MJG_SCALE_STREAM=1)
  bool hcl = false;     // ... with the strip's h coefficients staged in LDS
  StreamGeom sq{};
};

// One launch of the sws stage's plan, built at open (build_plan): per plane (0 luma, 1 chroma: U
// and V share it) under a pad the border (k_pad_plane), then the picture (k_scale, k_scale_stream
// or k_plane_copy; a padded plane that keeps its size is k_pad_plane<.., COPY> alone).  `launch`
// (null: no such pass) is the launcher of the kernel instantiation the plane's filters, range and
// geometry select; g holds every ScaleGeom field that no submit changes (submit_impl adds nf, the
// U+V pairing and V's offsets).
struct Pass;
using PassFn = void (*)(const Pass &p, const ScaleGeom &g, const SegList &in, uint8_t *dst, int nz, hipStream_t st);
struct Pass {
  PassFn launch = nullptr;
  int block = 0;    // threads per workgroup; the grid is g.gxy workgroups per (plane, frame)
  size_t lds = 0;   // dynamic LDS bytes
  ScaleGeom g{};
  PadGeom pad{};    // k_pad_plane
  const PlaneScale *ps = nullptr;  // the filters' device tables and StreamGeom
};

// One launch of the orientation stage (k_orient_plane; 0 luma, 1 chroma: U and V share it), built
// at open like the sws stage's: the launcher of the instantiation and the plane's geometry.
using OrientFn = void (*)(const OrientGeom &g, const SegList &in, uint8_t *dst, int nz, hipStream_t st);
struct OrientPass {
  OrientFn launch = nullptr;
  OrientGeom g{};
};

// One launch of the deinterlacer (k_yadif_plane; 0 luma, 1 chroma: U and V share it), built at open
// like the orientation stage's.
using DeintFn = void (*)(const DeintGeom &g, const SegList &in, uint8_t *dst, int nz, hipStream_t st);
struct DeintPass {
  DeintFn launch = nullptr;
  DeintGeom g{};
};

// One launch of the sharpen (k_unsharp_plane; 0 luma, 1 chroma: U and V share it), built at open like
// the orientation stage's: the sws stage's output buffer -> the slot's d_sharp.
using SharpFn = void (*)(const SharpGeom &g, const uint8_t *src, uint8_t *dst, int nz, hipStream_t st);
struct SharpPass {
  SharpFn launch = nullptr;
  SharpGeom g{};
};

struct Slot;
using EncodeFn = void (*)(const mjg_ctx *c, Slot &S, const SegList &enc_in, int wgs, int ntasks);

// Per-submit state.  A context has kSlots slots so further mjg_submits can be queued before
// the first is synced; everything a submit's results and its overflow re-write need lives
// in its slot.  Slots 1.. are allocated on the first pipelined submits.  Each slot has its
// own stream for H2D, scale and k_encode; the tail stream runs a submit's scan/stuff/write
// kernels after its k_encode (event enc_done), so the latency-bound tail of submit A runs
// beside the VALU-bound k_encode of submit B.  A slot is reused only after the host synced
// its previous submit (mjg_sync waits for `done`), so no device-side wait guards it.
// Two deep: a persistent k_encode holds every CU until its drain, so the host's sync of
// submit s-1 (whose slot submit s+1 reuses) waits for its tail, which gets CUs only as submit
// s's k_encode drains; the tail stream therefore runs at the highest priority (its
// workgroups dispatch before the next k_encode's).  Three slots measured 10% slower: three
// k_encode launches then share the CUs (DESIGN §4 streams; tools/patches.py slots3).
constexpr int kSlots = 2;
// Library-side merging (r05): single-segment device submits are held while the GPU has a
// launch queued and launched kMerge at a time as one segment list (submit_impl's SegList),
// so the launch's ramp and drain (T(n) = 0.115 ms + 4.48 us n per 4K launch) is
// paid once per kMerge submits.  Each submit stays a job of its own for mjg_sync / mjg_fetch.
constexpr int kMerge = 2;
// k_emit_syms workgroups per k_encode workgroup: the replay waits on memory most of its time
// and needs 54 VGPRs and 8.7 KB of LDS, so more waves per SIMD than k_encode's four hide that
// latency.  Since each wave replays a run of consecutive chunks (one table load per frame
// instead of one per chunk), x2 is the best grid: bench c1 x1 / x2 / x4 0.526-0.529 /
// 0.508-0.512 / 0.506-0.522 ms per step (profiles/r05/c1_emit_runs_ab.txt; with strided chunks
// x4 was best, profiles/r05/c1_emit_grid_bench.txt)
constexpr int kEmitGridMul = 2;
// merging is off when the slots' doubled scratch would take more than this share of the
// device's free memory (slot buffers scale with the frames a launch may carry)
constexpr double kMergeMemShare = 0.25;
struct Slot {
  bool alloc = false, pending = false;
  int njobs = 0, nsynced = 0;       // submits (jobs) this launch carries / already synced
  int jf0[kMaxSegs] = {}, jn[kMaxSegs] = {};  // each job's first frame in the launch, frames
  hipStream_t st = nullptr;        // H2D, scale and k_encode of this slot's submits
  uint8_t *d_stage = nullptr;      // H2D staging for host submits (allocated on first use)
  uint8_t *d_scaled = nullptr;     // -vf scale: k_scale's output planes
  uint8_t *d_orient = nullptr;     // -vf hflip / vflip / transpose: k_orient_plane's output frames
  uint8_t *d_deint = nullptr;      // -vf yadif: k_yadif_plane's output frames
  uint8_t *d_sharp = nullptr;      // -vf unsharp: k_unsharp_plane's output, the encoder's input
  uint8_t *d_lut = nullptr;        // a table in front of the sws stage on a caller's frames: k_lut_plane's output frames
  uint8_t *d_tile = nullptr;       // -vf tile: k_tile_plane's output, the sheets, the encoder's input
  uint16_t *d_dn16 = nullptr;      // -vf hqdn3d: P, then V, of every frame (DnGeom's uint16 layout)
  uint8_t *d_dn = nullptr;         // ... and k_dn_time's output, the denoised frames
  hipEvent_t dn_done = nullptr;    // ... recorded behind k_dn_time: the next submit's time scan waits for it
  uint32_t *d_stage_bits = nullptr;  // k_encode: per wave, lane-major staging of blocks past 128 bits
  int n = 0;  // frames of the launch (under a sheet: the sheets, the frames k_encode codes)
  int nin = 0;  // ... and its input frames (the same without a sheet)
  uint32_t *d_scratch = nullptr;
  uint32_t *d_stream = nullptr;  // k_count_ff's realigned words, per segment (k_write reads them)
  uint32_t *d_chunk_bits = nullptr, *d_chunk_off = nullptr, *d_group_ff = nullptr, *d_ff_off = nullptr;
  uint32_t *d_frame_bits = nullptr, *d_status = nullptr;
  uint32_t *d_work = nullptr;  // k_encode's batch counter (zero; reset by the slot's scan kernel)
  uint64_t *d_frame_size = nullptr, *d_frame_offsets = nullptr;
  uint32_t *d_seg_size = nullptr;  // RST mode: stuffed segment sizes and offsets after the header
  uint32_t *d_seg_off = nullptr;
  uint32_t *d_done = nullptr;      // k_scan_ff's frame ticket (one word, zeroed by k_scan_bits)
  uint8_t *d_out = nullptr;
  size_t out_cap = 0;
  uint32_t *d_hist = nullptr, *d_ftabs = nullptr, *d_dht_nval = nullptr, *d_hdr_lens = nullptr;  // optimal
  uint32_t *d_syms = nullptr, *d_symn = nullptr;  // optimal: per block, the symbols the counting pass saw
  uint8_t *d_dht = nullptr;
  int16_t *d_dbg = nullptr;
  uint64_t *h_sizes = nullptr;
  uint32_t *h_status = nullptr;
  hipEvent_t done = nullptr, enc_done = nullptr;
  hipEvent_t ev[MJG_NUM_KERNELS][2] = {};
};

}  // namespace

struct mjg_ctx {
  int device = 0;
  mjg_config cfg{};
  hipStream_t stream = nullptr;  // H2D, scale, k_encode of slot 0's submits
  hipStream_t more[kSlots - 1] = {};  // ... of slots 1..: consecutive submits' k_encode launches
                                      // overlap (the next starts on the CUs the previous drain frees)
  hipStream_t tail = nullptr;    // scans, stuffing, write, D2H of the sizes
  EncGeom geom{};
  int32_t qmat[64];
  int enc_grid = 0;             // persistent k_encode workgroups: every CU full (kEmitDefault)
  int enc_grid_cnt = 0;         // the same for the -huffman optimal counting pass (kCount: more LDS)
  bool scale = false;           // the sws stage runs: the sizes or the chroma formats differ
  // -vf hflip / vflip / transpose (mjg_open_orient): T | FX << 1 | FY << 2, the first filter; every
  // size and offset below then refers to the oriented frame (src_h x src_w when orient & 1)
  int orient = 0;
  OrientPass opass[2];          // its launches: 0 luma, 1 chroma
  // -vf yadif (mjg_open_deint): MJG_DEINT_* bits, 0 none; in front of the orientation, on the decoded
  // frames.  Every submit (every segment of one) is a sequence of its own: no merging
  int deint = 0;
  DeintPass dpass[2];           // its launches: 0 luma, 1 chroma
  // -vf unsharp (mjg_open_sharp): behind the sws stage (which then always runs) and in front of
  // the pad's border; k_encode reads its buffer
  bool sharp = false;
  mjg_unsharp us{};
  SharpPass shpass[2];          // its launches: 0 luma, 1 chroma
  // the tables (mjg_open_lut): [0] slot "in", behind the deinterlacer and the orientation, on whole
  // frames in the source format (in place in d_deint / d_orient, else into the slot's d_lut, which
  // the sws stage or k_encode then reads); [1] slot "out", in place on the picture in d_scaled
  // (the sws stage then always runs), in front of the sharpen.  Identity tables are no table
  bool has_lut[2] = {false, false};
  mjg_lut lut[2];
  LutGeom lpass[2][2];          // their launches: [slot][0 luma, 1 chroma]
  uint8_t *d_luts = nullptr;    // both slots' tables, 768 bytes each
  // the colour matrix (mjg_open_cmat): behind the deinterlacer and the orientation and in front of
  // lut[0], on whole frames in the source format (in place in d_deint / d_orient, else into the
  // slot's d_lut, where lut[0] then runs in place).  The identity is no matrix
  bool has_cmat = false;
  mjg_cmatrix cmat{};
  CmatGeom cgeom{};             // its launch
  void (*cmat_launch)(const SegList &, uint8_t *, const CmatGeom &, const CmatCoef &, int, hipStream_t) = nullptr;
  // -vf tile (mjg_open_sheet): behind the sws stage (which then always runs) and the sharpen; k_encode
  // reads the sheets in d_tile.  geom, enc_frame_bytes, the header and the output-side slot buffers are
  // then the sheet's, pic_* the cell's.  Every submit (every segment of one) is a sequence of its own:
  // no merging
  bool sheet = false;
  mjg_sheet sh{};               // nb_frames resolved (1..cols rows)
  TileGeom tpass[2];            // its launches: 0 luma, 1 chroma
  // -vf hqdn3d (mjg_open_denoise): behind the deinterlacer and in front of the orientation, on whole frames
  // in the source format; the orientation, cmat / lut_in in place, the sws stage or k_encode read d_dn.
  // The time scan's state lives here, one frame of uint16, and goes from submit to submit (mjg_submit_cont);
  // dn_last is the event behind the last submit's k_dn_time, which the next one's stream waits for.  Every
  // submit is a sequence of its own or a piece of one: no merging
  bool dn = false;
  std::vector<mjg_denoise> dn_tabs; // host copy of the tables (one, or none)
  DnGeom dnpass[2];             // its geometry: 0 luma, 1 chroma (the three kernels' grids: dn_grids)
  int dn_grid[2][3] = {};       // workgroups per (plane, frame) of k_dn_rows, k_dn_cols; per plane of k_dn_time
  size_t dn_felems = 0;         // uint16 elements of a frame of d_dn16
  int16_t *d_dn_tabs = nullptr;
  uint16_t *d_dn_state = nullptr;
  hipEvent_t dn_last = nullptr;
  bool dn_started = false;      // a submit has written the state
  size_t in_frame_bytes = 0, enc_frame_bytes = 0;
  // the sws stage's output frame (the picture, the canvas under a pad; k_encode's input without a
  // sheet): its bytes, its U plane's offset and the bytes of a chroma plane
  size_t pic_frame_bytes = 0;
  long long pic_u_off = 0, pic_cplane = 0;
  // the crop rectangle (mjg_open_crop; the whole frame otherwise): the input of the sws stage,
  // or of k_encode without one
  long long src_off[3] = {0, 0, 0};  // byte offsets of the rectangle's Y, U, V planes in a source frame
  long long src_cplane = 0;     // bytes of one source chroma plane (U to V)
  // -vf pad (mjg_open_pad): the encoded frames are a canvas with the sws stage's output (the
  // picture, cfg.dst_w x dst_h) at (pad_x, pad_y); has_pad is false for the trivial rectangle
  bool has_pad = false;
  PadGeom pad[2] = {};          // 0 luma, 1 chroma: the canvas plane, the picture's place, the border byte
  bool enc_ua = false;          // k_encode<.., UA>: a crop read in place whose geometry can fail
                                // fetch_rows' alignment test (MJG_UNALIGNED_FETCH=0: never)
  std::vector<uint8_t> hdr;
  uint8_t mprime[64];

  uint32_t *d_tabs = nullptr;
  uint8_t *d_hdr = nullptr;
  size_t stage_cols = 0;       // staging columns per slot (persistent waves of k_encode / k_emit_syms)
  bool rst = false;            // RST mode (MJG_F_RST, more than one MCU row)
  bool optimal = false;        // -huffman optimal
  size_t dht_pos = 0, dht_end = 0;
  PlaneScale ps[2];  // 0 luma, 1 chroma (U and V share)
  Pass pass[2][2];   // ... and their launches
  EncodeFn enc_count = nullptr, enc_emit = nullptr;  // k_encode<.., kCount / kEmitDefault, ..> of this context
  size_t slot_B = 0, slot_NC = 0, slot_NS = 0;  // slot sizes: frames, chunks and segments per frame
  size_t slot_BO = 0;  // ... and encoded frames (slot_B; under a sheet the sheets a launch may yield)

  Slot slot[kSlots];
  int head = 0;   // slot of the next launch
  int nout = 0;   // launches with jobs not yet synced (0..kSlots)
  int last = -1;  // slot of the last synced job (fetch / output_device / debug read it)
  int last_job = 0;            // that job's index in its launch
  uint64_t last_off = 0, last_total = 0;  // its packed bytes' offset in the launch's d_out, size
  bool synced_since_submit = false;
  int merge = 1;               // jobs per launch for single-segment device submits (kMerge or 1)
  bool hold_idle = true;       // hold a lone device job even on an idle GPU (MJG_MERGE_HOLD=0: launch it)
  int held = 0;                // device jobs held for the next launch (0..merge)
  const uint8_t *held_p[kMaxSegs] = {};
  int held_n[kMaxSegs] = {};
  int launches = 0;            // launches since open (tests / diagnostics)

  bool timing = false, timing_detail = false;
  bool timing_tail = false;  // MJG_F_TIMING's tail interval (MJG_TIMING_NOTAIL=1: off, A/B of the events' cost)
  uint8_t *h_fetch = nullptr;  // page-locked copy of the last fetched output (mjg_fetch_host)
  size_t h_fetch_cap = 0;
  double t_acc[MJG_NUM_KERNELS] = {0};
  int t_n = 0;
};

namespace {

void free_ctx(mjg_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (hipStream_t st : c->more)
    if (st) (void)hipStreamSynchronize(st);
  if (c->tail) (void)hipStreamSynchronize(c->tail);
  void *ptrs[] = {c->d_tabs, c->d_hdr, c->d_luts, c->d_dn_tabs, c->d_dn_state, c->ps[0].hcp,
                  c->ps[0].vcp, c->ps[0].hp, c->ps[0].vps, c->ps[1].hcp, c->ps[1].vcp, c->ps[1].hp,
                  c->ps[0].hsum, c->ps[1].hsum, c->ps[1].vps, c->ps[0].mfb, c->ps[1].mfb};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  for (Slot &S : c->slot) {
    void *sp[] = {S.d_stage, S.d_scaled, S.d_orient, S.d_deint, S.d_sharp, S.d_lut, S.d_tile, S.d_dn16, S.d_dn, S.d_stage_bits, S.d_scratch, S.d_stream, S.d_work, S.d_chunk_bits, S.d_chunk_off, S.d_group_ff, S.d_ff_off, S.d_frame_bits,
                  S.d_status, S.d_frame_size, S.d_frame_offsets, S.d_seg_size, S.d_seg_off, S.d_done, S.d_out,
                  S.d_hist, S.d_ftabs, S.d_dht_nval, S.d_hdr_lens, S.d_dht, S.d_dbg, S.d_syms, S.d_symn};
    for (void *p : sp)
      if (p) (void)hipFree(p);
    if (S.h_sizes) (void)hipHostFree(S.h_sizes);
    if (S.h_status) (void)hipHostFree(S.h_status);
    if (S.done) (void)hipEventDestroy(S.done);
    if (S.enc_done) (void)hipEventDestroy(S.enc_done);
    if (S.dn_done) (void)hipEventDestroy(S.dn_done);
    for (auto &e : S.ev) {
      if (e[0]) (void)hipEventDestroy(e[0]);
      if (e[1]) (void)hipEventDestroy(e[1]);
    }
  }
  if (c->h_fetch) (void)hipHostFree(c->h_fetch);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  for (hipStream_t st : c->more)
    if (st) (void)hipStreamDestroy(st);
  if (c->tail && c->tail != c->stream) (void)hipStreamDestroy(c->tail);
  delete c;
}

// k_scale_stream's chunk rows, ring, window stride and LDS bytes (scale.hip) for a plane whose
// widest strip window is max_nw dwords: the most rows per chunk that fit 64 KB (two window
// halves and a ring of npv + R pairs), with the strip's h coefficients and the band's v filter
// rows staged beside them when they fit.  False when nothing fits (no filter below 256 taps:
// the ring is at most 130 pairs, 33 KB, and two halves of two window rows at most 18 KB).
bool plan_scale_stream(int max_nw, int ht, int npv, StreamGeom *q, bool *hcl, size_t *lds) {
  const int npc = max_nw / 4;  // (max_nw is a multiple of 4)
  for (int R = 16; R >= 2; R >>= 1)
    for (int stage = 3; stage >= 0; stage--) {  // bit 1: h coefficients, bit 0: v filter rows
      const int rp = npv + R;
      const size_t need = (2 * (size_t)R * max_nw + (size_t)rp * kScaleTileW +
                           ((stage & 2) ? (size_t)kScaleTileW * (ht / 2) : 0) +
                           ((stage & 1) ? (size_t)kStreamBand * npv : 0)) * 4;
      if (need > 64 * 1024 || R * npc > kStreamThreads * kStreamMaxPieces) continue;
      q->R = R;
      q->rp = rp;
      q->rs = max_nw;
      q->npc = npc;
      q->npc_magic = magic32((uint32_t)npc);
      q->vcl = stage & 1;
      *hcl = (stage & 2) != 0;
      *lds = need;
      return true;
    }
  return false;
}

// A context's rectangles, resolved by check_config
struct Layout {
  int deint;                   // MJG_DEINT_* bits (0: no deinterlacer)
  bool sharp;                  // -vf unsharp with a non-zero amount
  mjg_unsharp us;              // ... its sizes and amounts
  const mjg_lut *lut[2];       // the tables of slot "in" and slot "out" (null: none, or three identity tables)
  const mjg_cmatrix *cm;       // the colour matrix (null: none, or the identity)
  int orient, ow, oh;          // the orientation and the oriented frame's size (orient 0: the source's)
  int cx, cy, crw, crh;        // the crop rectangle in the oriented frame: the sws stage's / k_encode's input
  int px, py, pw, ph;          // the picture's place in the canvas and the canvas size (no pad: the picture)
  bool has_pad;                // false for the trivial rectangle
  int s_hsh, s_vsh, hsh, vsh;  // chroma shifts of the source format and of the encoded one
  bool has_sheet;              // a contact sheet behind the sws stage (check_sheet; false for the trivial one)
  mjg_sheet sheet;             // ... nb_frames resolved
  int tw, th;                  // ... and its size, the encoded frame's
  const mjg_denoise *dn;       // the denoiser's tables (mjg_open_denoise; null: none)
};

// A plane's filter tables as the kernels read them (plan_plane_scale), before their upload
struct ScaleTabs {
  std::vector<int32_t> hcp, vcp, vps, hsum, mfb;  // mfb empty: no matrix-core pass
};

// The host step of a plane's scale setup, for the sizes in p.g: the two SwsFilters, the
// coefficient / position tables and the tile, stream and matrix-core decisions (p.g's filter
// fields, p.lds, p.grid).  chroma: the plane's subsampling shifts in the source format and in the
// encoded one select the siting get_local_pos(shift, -513) of each side (swscale's src / dst
// pixel formats; with the default siting every one comes to 128)
int plan_plane_scale(PlaneScale &p, ScaleTabs &t, const Layout &lay, bool chroma, bool bitexact, bool force_stream) {
  const int sw = p.g.sw, sh = p.g.sh, dw = p.g.dw, dh = p.g.dh;
  auto pos = [&](int shift) { return chroma ? sws_local_pos(shift, -513) : sws_local_pos(0, 0); };
  if (!make_sws_filter(sw, dw, 1 << 14, 4, bitexact, pos(lay.s_hsh), pos(lay.hsh), &p.hf) ||
      !make_sws_filter(sh, dh, 1 << 12, 2, bitexact, pos(lay.s_vsh), pos(lay.vsh), &p.vf))
    return set_err(MJG_E_INVALID, "scale %dx%d -> %dx%d needs swscale's cascade (unsupported)", sw, sh, dw, dh);
  for (int i = 1; i < dw; i++)
    if (p.hf.pos[i] < p.hf.pos[i - 1]) return set_err(MJG_E_INVALID, "non-monotone hscale");
  for (int i = 1; i < dh; i++)
    if (p.vf.pos[i] < p.vf.pos[i - 1]) return set_err(MJG_E_INVALID, "non-monotone vscale");
  // h taps padded with zero coefficients to a multiple of 4 (k_scale takes 4 taps per step),
  // v taps of any count (the pair table below zero-pads).  A window may run past the row
  // end (tiny sources, padded taps): initFilter zeroes every coefficient past srcW, so the
  // bytes k_scale stages there never count.
  const int ht0 = p.hf.taps, vt = p.vf.taps;
  const int ht = (ht0 + 3) & ~3;
  std::vector<int16_t> hpad((size_t)dw * ht, 0);
  for (int x = 0; x < dw; x++)
    for (int k = 0; k < ht0; k++) hpad[(size_t)x * ht + k] = p.hf.coeff[(size_t)x * ht0 + k];
  // h: coefficient pairs per output column; v: pairs starting at the even row <= pos[y],
  // shifted by its parity and zero-padded to npv = vt/2 + 1 pairs
  const int npv = vt / 2 + 1;
  std::vector<int32_t> &hcp = t.hcp, &vcp = t.vcp, &vps = t.vps, &hsum = t.hsum;
  hcp.assign((size_t)dw * (ht / 2), 0);
  vcp.assign((size_t)dh * npv, 0);
  vps.assign(dh, 0);
  hsum.assign(dw, 0);
  // D4 layout when every coefficient splits as 128 ch + cl, ch int8, cl in [-64, 64): per 4
  // taps one word of ch bytes and one of cl bytes (else the int16 pair layout)
  p.d4 = true;
  for (size_t i = 0; i < p.hf.coeff.size(); i++)
    if (p.hf.coeff[i] < -128 * 128 - 64 || p.hf.coeff[i] >= 127 * 128 + 64) p.d4 = false;
  for (int x = 0; x < dw; x++) {
    const int16_t *cx = &hpad[(size_t)x * ht];
    for (int k = 0; k < ht; k++) hsum[x] += cx[k];
    for (int k = 0; k < ht / 2; k++) {
      uint32_t wv;
      if (p.d4) {
        const int g4 = k >> 1, lo_part = k & 1;  // word 2j: ch of taps 4j..4j+3, word 2j+1: cl
        wv = 0;
        for (int b = 0; b < 4; b++) {
          const int cv = cx[4 * g4 + b], cl = ((cv + 64) & 127) - 64, ch = (cv - cl) / 128;
          wv |= (uint32_t)(uint8_t)(int8_t)(lo_part ? cl : ch) << (8 * b);
        }
      } else {
        wv = (uint32_t)(uint16_t)cx[2 * k] | ((uint32_t)(uint16_t)cx[2 * k + 1] << 16);
      }
      hcp[(size_t)x * (ht / 2) + k] = (int32_t)wv;
    }
  }
  for (int y = 0; y < dh; y++) {
    const int r = p.vf.pos[y], par = r & 1;
    vps[y] = r >> 1;
    for (int k = 0; k < npv; k++) {
      const int j0 = 2 * k - par, j1 = j0 + 1;
      const uint16_t c0 = (j0 >= 0 && j0 < vt) ? (uint16_t)p.vf.coeff[(size_t)y * vt + j0] : 0;
      const uint16_t c1 = (j1 >= 0 && j1 < vt) ? (uint16_t)p.vf.coeff[(size_t)y * vt + j1] : 0;
      vcp[(size_t)y * npv + k] = (int32_t)((uint32_t)c0 | ((uint32_t)c1 << 16));
    }
  }
  // k_scale's tile height: 64 rows for the 2:1 filters when every window fits the fast path
  // at a 36-dword row stride (scale.hip), else 32
  auto tile_pairs = [&](int th) {
    int m = 0;
    for (int y0 = 0; y0 < dh; y0 += th) m = std::max(m, vps[std::min(y0 + th, dh) - 1] + npv - vps[y0]);
    return m;
  };
  int max_nw = 0;
  for (int x0 = 0; x0 < dw; x0 += kScaleTileW) {  // same formula as k_scale's window
    const int xe = std::min(x0 + kScaleTileW, dw), cb = p.hf.pos[x0] & ~3;
    max_nw = std::max(max_nw, ((((p.hf.pos[xe - 1] + ht - cb + 3) >> 2) + 1) + 3) & ~3);
  }
  const int th2 = 64;  // tile height for the 2:1 filters
  const int th = (ht == 8 && npv == 5 && max_nw <= kScaleAliasWords && sw >= 16 &&
                  2 * tile_pairs(th2) <= scale_waves(th2) * scale_loads_per_wave(th2) * kScaleLoadRows) ? th2 : 32;
  const int max_pairs = tile_pairs(th);
  p.th = th;
  ScaleGeom &g = p.g;
  g.htaps = ht;
  g.vtaps = vt;
  g.npv = npv;
  g.lds_pairs = max_pairs;
  if (th >= 64) {  // pair image over the window rows (scale.hip: ALIAS)
    g.lds_win_words = 2 * max_pairs * kScaleAliasWords;
    p.lds = (size_t)g.lds_win_words * 4 + 64;  // v filter rows by scalar loads; the matrix-core
                                               // h-pass reads 16 bytes past the last row
  } else {
    g.lds_win_words = 2 * max_pairs * max_nw;
    p.lds = ((size_t)g.lds_win_words + (size_t)max_pairs * kScaleTileW + (size_t)th * (npv + 1)) * 4;
  }
  p.grid = dim3((dw + kScaleTileW - 1) / kScaleTileW, (dh + th - 1) / th, 1);
  // past one LDS tile (about 4:1), or on request for a plane whose size changes: k_scale_stream
  p.stream = p.lds > 64 * 1024 || (force_stream && (sw != dw || sh != dh));
  if (p.stream) {
    if (!plan_scale_stream(max_nw, ht, npv, &p.sq, &p.hcl, &p.lds))
      return set_err(MJG_E_INVALID, "scale %dx%d -> %dx%d: no streaming plan fits LDS", sw, sh, dw, dh);
    p.grid = dim3((dw + kScaleTileW - 1) / kScaleTileW, (dh + kStreamBand - 1) / kStreamBand, 1);
  }
  // The matrix-core h-pass (scale.hip, scale_hpass_mf) for the interior tile columns when they
  // all share one filter at a 2-byte step (exact 2:1): B[k][n] = the hi (lo) byte of tap
  // k - 2n - d of that filter (0 outside the 8 taps), k the byte of a 64-byte window that starts
  // at the column block's aligned byte 32 cj, d = the first column's byte offset in its dword.
  // Lane l holds B[16 (l >> 4) + j][l & 15] in byte j (the same k map as its A fragment).
  g.mf_bx0 = g.mf_bx1 = 0;
  g.mf_hs = 0;
  const int gxt = (dw + kScaleTileW - 1) / kScaleTileW;
  if (!p.stream && p.d4 && ht == 8 && th >= 64 && gxt >= 3) {
    const int xa = kScaleTileW, xb = kScaleTileW * (gxt - 1);
    bool ok = true;
    for (int x = xa; x < xb && ok; x++) {
      ok = p.hf.pos[x] == p.hf.pos[xa] + 2 * (x - xa) && hsum[x] == hsum[xa];
      for (int k = 0; k < ht / 2 && ok; k++) ok = hcp[(size_t)x * (ht / 2) + k] == hcp[(size_t)xa * (ht / 2) + k];
    }
    if (ok) {
      const int d = p.hf.pos[xa] & 3;
      std::vector<int32_t> &mfb = t.mfb;
      mfb.assign(kMvFragOff + 3 * 64 * 4, 0);
      for (int l = 0; l < 64; l++)
        for (int j = 0; j < 16; j++) {
          const int k = 16 * (l >> 4) + j, n = l & 15, t = k - 2 * n - d;
          if (t < 0 || t >= 8) continue;
          const uint32_t hi = ((uint32_t)hcp[(size_t)xa * (ht / 2) + 2 * (t >> 2)] >> (8 * (t & 3))) & 255u;
          const uint32_t lo = ((uint32_t)hcp[(size_t)xa * (ht / 2) + 2 * (t >> 2) + 1] >> (8 * (t & 3))) & 255u;
          mfb[(size_t)l * 8 + (j >> 2)] |= (int32_t)(hi << (8 * (j & 3)));
          mfb[(size_t)l * 8 + 4 + (j >> 2)] |= (int32_t)(lo << (8 * (j & 3)));
        }
      // The matrix-core v-pass (scale.hip) for the interior tile rows of those columns when they
      // all share one v filter at a 2-row step: A[m][k] = tap k - 2m - delta of it (0 outside the
      // 8 taps), delta = the parity of its first row (the window starts at the even row below),
      // split as tap = 128 fh + fl: fragments fh, fl and 2 fl, lane l holding A[l & 15][16 (l >> 4)
      // + j] in byte j (the h-pass's k map)
      const int gyt = (dh + th - 1) / th, ya = th, yb = th * (gyt - 1);
      bool vok = gyt >= 3 && vt == 8 && 2 * 64 * kPlaneStride + 16 <= (int)p.lds;
      for (int y = ya; y < yb && vok; y++) {
        vok = p.vf.pos[y] == p.vf.pos[ya] + 2 * (y - ya);
        for (int k = 0; k < vt && vok; k++) vok = p.vf.coeff[(size_t)y * vt + k] == p.vf.coeff[(size_t)ya * vt + k];
      }
      int fsum = 0;
      for (int k = 0; k < vt && vok; k++) {
        const int cv = p.vf.coeff[(size_t)ya * vt + k], fl = ((cv + 64) & 127) - 64;
        vok = (cv - fl) / 128 >= -128 && (cv - fl) / 128 <= 127;
        fsum += cv;
      }
      g.mv_by0 = g.mv_by1 = 0;
      g.mv_k = 0;
      if (vok) {
        const int delta = p.vf.pos[ya] & 1;
        for (int l = 0; l < 64; l++)
          for (int j = 0; j < 16; j++) {
            const int m = l & 15, k = 16 * (l >> 4) + j, t = k - 2 * m - delta;
            const int cv = (t >= 0 && t < 8) ? p.vf.coeff[(size_t)ya * vt + t] : 0;
            const int fl = ((cv + 64) & 127) - 64, fh = (cv - fl) / 128;
            const int vals[3] = {fh, fl, 2 * fl};
            for (int f = 0; f < 3; f++)
              mfb[kMvFragOff + (size_t)(f * 64 + l) * 4 + (j >> 2)] |= (int32_t)((uint32_t)(uint8_t)(int8_t)vals[f] << (8 * (j & 3)));
          }
        g.mv_by0 = 1;
        g.mv_by1 = gyt - 1;
        g.mv_k = 128 * fsum + (64 << 12);
      }
      g.mf_bx0 = 1;
      g.mf_bx1 = gxt - 1;
      g.mf_hs = hsum[xa];
    }
  }
  return MJG_OK;
}

// ... and the upload step
int upload_plane_scale(PlaneScale &p, const ScaleTabs &t) {
  const std::pair<int32_t **, const std::vector<int32_t> *> up[] = {
      {&p.hsum, &t.hsum}, {&p.hcp, &t.hcp}, {&p.hp, &p.hf.pos}, {&p.vcp, &t.vcp}, {&p.vps, &t.vps}, {&p.mfb, &t.mfb}};
  for (const auto &u : up) {
    if (const int rc = dmalloc(u.first, u.second->size())) return rc;
    if (!u.second->empty())
      HIP_TRY(hipMemcpy(*u.first, u.second->data(), u.second->size() * 4, hipMemcpyHostToDevice));
  }
  return MJG_OK;
}

hipStream_t slot_stream(const mjg_ctx *c, int i) { return i ? c->more[i - 1] : c->stream; }

int alloc_slot(mjg_ctx *c, Slot &S) {
  const size_t BI = c->slot_B, B = c->slot_BO, NC = c->slot_NC, NS = c->slot_NS;  // input frames, encoded frames
  const EncGeom &g = c->geom;
  int rc;
  // Each slot on its own stream: consecutive submits (queued kSlots deep) overlap, so the next
  // submit's launches start on the CUs the previous one's drain frees.  A persistent k_encode's
  // waves finish its last work units over ~140 us (the SIMD arbiter runs its oldest wave 2.2x
  // faster than its youngest), and a workgroup's slot frees when its last wave
  // ends.  A/B: c2 +5.4% (bench.py, r04), c5 +1.6%, c1 +24% and c4 +1.7% (r03, chains of
  // launches).  Each launch's own event interval then includes its neighbour's overlap.
  S.st = slot_stream(c, (int)(&S - c->slot));
  if ((rc = dmalloc(&S.d_stage_bits, c->stage_cols * 64 * kStageWords))) return rc;
  if (c->scale && (rc = dmalloc(&S.d_scaled, BI * c->pic_frame_bytes))) return rc;
  if (c->orient && (rc = dmalloc(&S.d_orient, BI * c->in_frame_bytes))) return rc;
  if (c->deint && (rc = dmalloc(&S.d_deint, BI * c->in_frame_bytes))) return rc;
  if (c->sharp && (rc = dmalloc(&S.d_sharp, BI * c->pic_frame_bytes))) return rc;
  if ((c->has_lut[0] || c->has_cmat) && !c->orient && !c->deint && !c->dn && (rc = dmalloc(&S.d_lut, BI * c->in_frame_bytes))) return rc;
  if (c->dn && ((rc = dmalloc(&S.d_dn16, BI * c->dn_felems)) || (rc = dmalloc(&S.d_dn, BI * c->in_frame_bytes)))) return rc;
  if (c->dn) HIP_TRY(hipEventCreateWithFlags(&S.dn_done, hipEventDisableTiming));
  if (c->sheet && (rc = dmalloc(&S.d_tile, B * c->enc_frame_bytes))) return rc;
  if ((rc = dmalloc(&S.d_scratch, B * NC * (size_t)kSlotWords)) ||
      (rc = dmalloc(&S.d_stream, B * NC * (size_t)kSlotWords)) ||
      (rc = dmalloc(&S.d_chunk_bits, B * NC)) || (rc = dmalloc(&S.d_chunk_off, B * NC)) ||
      (rc = dmalloc(&S.d_group_ff, B * NC)) || (rc = dmalloc(&S.d_ff_off, B * NC)) ||
      (rc = dmalloc(&S.d_frame_bits, B * NS)) || (rc = dmalloc(&S.d_status, 4)) ||
      (rc = dmalloc(&S.d_frame_size, B)) || (rc = dmalloc(&S.d_frame_offsets, B + 1)) ||
      (rc = dmalloc(&S.d_done, 1)) ||
      (rc = dmalloc(&S.d_work, (size_t)kXcds * kCtrStride)))
    return rc;
  HIP_TRY(hipMemset(S.d_work, 0, (size_t)kXcds * kCtrStride * sizeof(uint32_t)));
  if (c->rst && ((rc = dmalloc(&S.d_seg_size, B * NS)) || (rc = dmalloc(&S.d_seg_off, B * NS)))) return rc;
  S.out_cap = B * (c->enc_frame_bytes + c->hdr.size() + 4096 + 2 * NS);
  if ((rc = dmalloc(&S.d_out, S.out_cap))) return rc;
  if (c->optimal &&
      ((rc = dmalloc(&S.d_hist, B * kFrameTabWords)) || (rc = dmalloc(&S.d_ftabs, B * kFrameTabWords)) ||
       (rc = dmalloc(&S.d_dht, B * 4 * kDhtSlot)) || (rc = dmalloc(&S.d_dht_nval, B * 4)) ||
       (rc = dmalloc(&S.d_hdr_lens, B)) || (rc = dmalloc(&S.d_syms, B * NC * (size_t)kSymCap * 64)) ||
       (rc = dmalloc(&S.d_symn, B * NC * 64))))
    return rc;
  if (g.debug_coefs && (rc = dmalloc(&S.d_dbg, B * (size_t)g.nmcu * g.bpm * 64))) return rc;
  HIP_TRY(hipHostMalloc((void **)&S.h_sizes, (B + 1) * sizeof(uint64_t), hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void **)&S.h_status, 16, hipHostMallocDefault));
  HIP_TRY(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&S.enc_done, hipEventDisableTiming));
  if (c->timing)
    for (auto &e : S.ev) {
      HIP_TRY(hipEventCreate(&e[0]));
      HIP_TRY(hipEventCreate(&e[1]));
    }
  S.alloc = true;
  return MJG_OK;
}

// open, step 1: the config and the chain (no device, no environment).  mjgpu.h says what each field of
// ch means; the crop is in luma samples of the oriented frame, the pad (the picture's place and the
// canvas size) in luma samples of the encoded one.  The structs ch points to are read here and, through
// lay, until open_ctx returns.
int check_config(const mjg_config &k, const mjg_chain &ch, Layout *lay) {
  const int src_cf = ch.src_chroma_format, deint = ch.deint, orient = ch.orient;
  const mjg_cmatrix *cm = ch.cmat;
  const mjg_unsharp *us = ch.unsharp;
  if (std::min({k.src_w, k.src_h, k.dst_w, k.dst_h}) < 1 || std::max({k.src_w, k.src_h, k.dst_w, k.dst_h}) > 16384)
    return set_err(MJG_E_INVALID, "bad frame size %dx%d -> %dx%d", k.src_w, k.src_h, k.dst_w, k.dst_h);
  if (k.qscale < 1 || k.qscale > 31) return set_err(MJG_E_INVALID, "qscale %d not in 1..31", k.qscale);
  if (k.max_batch < 1 || k.max_batch > 65535) return set_err(MJG_E_INVALID, "max_batch %d not in 1..65535", k.max_batch);
  if (k.sar_num < 0 || k.sar_den < 0 || k.sar_num > 65535 || k.sar_den > 65535)
    return set_err(MJG_E_INVALID, "bad SAR %d:%d", k.sar_num, k.sar_den);
  if (k.chroma_format < MJG_CHROMA_420 || k.chroma_format > MJG_CHROMA_444)
    return set_err(MJG_E_INVALID, "chroma_format %d", k.chroma_format);
  if (src_cf < MJG_CHROMA_420 || src_cf > MJG_CHROMA_444)
    return set_err(MJG_E_INVALID, "src_chroma_format %d", src_cf);
  const int s_hsh = src_cf == MJG_CHROMA_444 ? 0 : 1, s_vsh = src_cf == MJG_CHROMA_420 ? 1 : 0;
  // the deinterlacer: yadif with the two option bits; its row and column clamps need 3 x 3 planes
  if (deint) {
    if ((deint & ~(MJG_DEINT_YADIF | MJG_DEINT_NOSPATIAL | MJG_DEINT_BFF)) || !(deint & MJG_DEINT_YADIF))
      return set_err(MJG_E_INVALID, "deint %d: not 0 or MJG_DEINT_YADIF (1) | MJG_DEINT_NOSPATIAL (2) | MJG_DEINT_BFF (4)",
                     deint);
    const int scw = (k.src_w + s_hsh) >> s_hsh, sch = (k.src_h + s_vsh) >> s_vsh;
    if (std::min({k.src_w, k.src_h, scw, sch}) < 3)
      return set_err(MJG_E_INVALID, "deint %d (yadif): a %dx%d frame has a plane smaller than 3x3 (chroma %dx%d)", deint,
                     k.src_w, k.src_h, scw, sch);
  }
  // the orientation: vf_transpose takes only formats whose two chroma shifts are equal
  if (orient < 0 || orient > 7)
    return set_err(MJG_E_INVALID, "orient %d not in 0..7 (T | FX << 1 | FY << 2)", orient);
  if ((orient & 1) && src_cf == MJG_CHROMA_422)
    return set_err(MJG_E_INVALID, "orient %d transposes a 4:2:2 source (only 4:2:0 and 4:4:4 keep their format)", orient);
  const int ow = (orient & 1) ? k.src_h : k.src_w, oh = (orient & 1) ? k.src_w : k.src_h;
  // the rectangle (the frame sizes and the source format are valid here)
  const int cx = ch.has_crop ? ch.crop_x : 0, cy = ch.has_crop ? ch.crop_y : 0;
  const int crw = ch.has_crop ? ch.crop_w : ow, crh = ch.has_crop ? ch.crop_h : oh;  // the sws stage's / k_encode's input size
  if (crw < 1 || crh < 1)
    return set_err(MJG_E_INVALID, "crop %dx%d at (%d,%d): the size is not positive", crw, crh, cx, cy);
  if (cx < 0 || cy < 0 || cx > ow - crw || cy > oh - crh)
    return set_err(MJG_E_INVALID, "crop %dx%d at (%d,%d) is outside the %dx%d frame%s", crw, crh, cx, cy, ow, oh,
                   orient ? " (the oriented one)" : "");
  if ((cx & ((1 << s_hsh) - 1)) || (cy & ((1 << s_vsh) - 1)))
    return set_err(MJG_E_INVALID, "crop %dx%d at (%d,%d): the position is not a multiple of the source's chroma "
                   "sub-sampling (%dx%d)", crw, crh, cx, cy, 1 << s_hsh, 1 << s_vsh);
  // the pad (the encoded format and the picture size are valid here): the trivial rectangle is no pad
  const int e_hsh = k.chroma_format == MJG_CHROMA_444 ? 0 : 1, e_vsh = k.chroma_format == MJG_CHROMA_420 ? 1 : 0;
  const int px = ch.has_pad ? ch.pad_x : 0, py = ch.has_pad ? ch.pad_y : 0;
  const int pw = ch.has_pad ? ch.pad_w : k.dst_w, ph = ch.has_pad ? ch.pad_h : k.dst_h;
  if (pw < 1 || ph < 1)
    return set_err(MJG_E_INVALID, "pad %dx%d with the picture at (%d,%d): the size is not positive", pw, ph, px, py);
  if (pw > 16384 || ph > 16384)
    return set_err(MJG_E_INVALID, "pad %dx%d with the picture at (%d,%d): the size is beyond 16384", pw, ph, px, py);
  if (px < 0 || py < 0 || px > pw - k.dst_w || py > ph - k.dst_h)
    return set_err(MJG_E_INVALID, "pad %dx%d with the picture at (%d,%d): the %dx%d picture is outside the canvas",
                   pw, ph, px, py, k.dst_w, k.dst_h);
  const bool has_pad = px != 0 || py != 0 || pw != k.dst_w || ph != k.dst_h;
  if (has_pad) {
    const int mh = (1 << e_hsh) - 1, mv = (1 << e_vsh) - 1;
    if ((px & mh) || (pw & mh) || (py & mv) || (ph & mv))
      return set_err(MJG_E_INVALID, "pad %dx%d with the picture at (%d,%d): not multiples of the encoded format's "
                     "chroma sub-sampling (%dx%d)", pw, ph, px, py, 1 << e_hsh, 1 << e_vsh);
    if ((k.dst_w & mh) || (k.dst_h & mv))
      return set_err(MJG_E_INVALID, "pad %dx%d with the picture at (%d,%d): the %dx%d picture is not a multiple of "
                     "the encoded format's chroma sub-sampling (%dx%d)", pw, ph, px, py, k.dst_w, k.dst_h,
                     1 << e_hsh, 1 << e_vsh);
  }
  constexpr uint32_t kKnownFlags = MJG_F_TIMING | MJG_F_DEBUG_COEFS | MJG_F_SWS_NO_BITEXACT | MJG_F_COM_ITU601 |
                                   MJG_F_HUFFMAN_OPTIMAL | MJG_F_RST | MJG_F_TIMING_DETAIL | MJG_F_MERGE;
  if (k.flags & ~kKnownFlags)  // retired bits (128, 256, 512: r05's FUSED / DCT_MFMA / DCT_VALU) included
    return set_err(MJG_E_INVALID, "unknown flags 0x%x", k.flags & ~kKnownFlags);
  if ((k.flags & MJG_F_RST) && (k.flags & MJG_F_HUFFMAN_OPTIMAL))
    return set_err(MJG_E_INVALID, "RST (slice threading) forces -huffman default");
  // the sharpen: odd sizes 3..23, amounts within the filter's option range, and for a plane that is
  // filtered a sum that fits the filter's 32-bit accumulator
  mjg_unsharp u{};
  const bool sharp = us && (us->la != 0 || us->ca != 0);
  if (us) {
    u = *us;
    const int sz[4] = {u.lx, u.ly, u.cx, u.cy};
    const char *nm[4] = {"lx", "ly", "cx", "cy"};
    for (int i = 0; i < 4; i++) {
      if (sz[i] < 3 || sz[i] > 23) return set_err(MJG_E_INVALID, "unsharp %s %d: size not in 3..23", nm[i], sz[i]);
      if (!(sz[i] & 1)) return set_err(MJG_E_INVALID, "unsharp %s %d: size is even (odd sizes only)", nm[i], sz[i]);
    }
    const int am[2] = {u.la, u.ca};
    for (int i = 0; i < 2; i++) {
      if (am[i] < -2 * 65536 || am[i] > 5 * 65536)
        return set_err(MJG_E_INVALID, "unsharp %s %d: amount outside [-2, 5] * 65536", i ? "ca" : "la", am[i]);
      const int hs = sz[2 * i] / 2 + sz[2 * i + 1] / 2;
      if (am[i] && hs > kSharpMaxHalfSum)
        return set_err(MJG_E_INVALID, "unsharp %s %dx%d: sx + sy = %d > %d, the 32-bit sum of the filter wraps",
                       i ? "chroma" : "luma", sz[2 * i], sz[2 * i + 1], hs, kSharpMaxHalfSum);
    }
  }
  const mjg_lut *luts[2] = {ch.lut_in, ch.lut_out};
  for (const mjg_lut *&l : luts) {
    bool id = true;
    for (int i = 0; l && i < 256; i++) id = id && l->y[i] == i && l->u[i] == i && l->v[i] == i;
    if (id) l = nullptr;
  }
  // the colour matrix: |coefficient| <= 2^18, four times unity.  With |U - 128|, |V - 128| <= 128 a sum
  // of two products is at most 2^26 and, with the rounding term (< 2^24), below 2^27: int32 holds it
  if (cm) {
    const int32_t v[6] = {cm->yu, cm->yv, cm->uu, cm->uv, cm->vu, cm->vv};
    const char *nm[6] = {"yu", "yv", "uu", "uv", "vu", "vv"};
    for (int i = 0; i < 6; i++)
      if (v[i] > kCmatMaxCoef || v[i] < -kCmatMaxCoef)
        return set_err(MJG_E_INVALID, "cmatrix %s %d: outside [-%d, %d] (four times 65536)", nm[i], (int)v[i], kCmatMaxCoef,
                       kCmatMaxCoef);
    if (v[0] == 0 && v[1] == 0 && v[2] == 65536 && v[3] == 0 && v[4] == 0 && v[5] == 65536) cm = nullptr;
  }
  Layout &l = *lay;
  l.deint = deint;
  l.sharp = sharp, l.us = u;
  l.lut[0] = luts[0], l.lut[1] = luts[1];
  l.cm = cm;
  l.orient = orient, l.ow = ow, l.oh = oh;
  l.cx = cx, l.cy = cy, l.crw = crw, l.crh = crh;
  l.px = px, l.py = py, l.pw = pw, l.ph = ph;
  l.has_pad = has_pad;
  l.s_hsh = s_hsh, l.s_vsh = s_vsh, l.hsh = e_hsh, l.vsh = e_vsh;
  l.has_sheet = false, l.sheet = mjg_sheet{}, l.tw = l.th = 0;
  l.dn = nullptr;
  return MJG_OK;
}

// open, step 1b: the sheet (mjg_open_sheet; null: none) on the layout check_config resolved.  The
// trivial sheet is no sheet.
int check_sheet(const mjg_config &k, const mjg_sheet *sp, Layout *lay) {
  if (!sp) return MJG_OK;
  const mjg_sheet &s = *sp;
  if (s.cols < 1 || s.rows < 1) return set_err(MJG_E_INVALID, "sheet %dx%d: cols or rows below 1", s.cols, s.rows);
  const long long cells = (long long)s.cols * s.rows;
  if (s.nb_frames < 0 || s.nb_frames > cells)
    return set_err(MJG_E_INVALID, "sheet %dx%d: nb_frames %d not in 0..%lld (cols x rows)", s.cols, s.rows, s.nb_frames, cells);
  if (s.margin < 0 || s.padding < 0)
    return set_err(MJG_E_INVALID, "sheet %dx%d: margin %d or padding %d is negative", s.cols, s.rows, s.margin, s.padding);
  const long long W = (long long)s.cols * k.dst_w + (long long)(s.cols - 1) * s.padding + 2ll * s.margin;
  const long long H = (long long)s.rows * k.dst_h + (long long)(s.rows - 1) * s.padding + 2ll * s.margin;
  if (W > 16384 || H > 16384)
    return set_err(MJG_E_INVALID, "sheet %dx%d of %dx%d cells, margin %d, padding %d: %lldx%lld, a side is beyond 16384",
                   s.cols, s.rows, k.dst_w, k.dst_h, s.margin, s.padding, W, H);
  if (cells == 1 && s.margin == 0) return MJG_OK;  // one cell that is the picture: no sheet
  if (lay->has_pad) return set_err(MJG_E_INVALID, "sheet %dx%d behind a pad: the chain's has_pad is set", s.cols, s.rows);
  const int mh = (1 << lay->hsh) - 1, mv = (1 << lay->vsh) - 1;
  if ((k.dst_w & mh) || (k.dst_h & mv) || (s.margin & (mh | mv)) || (s.padding & (mh | mv)))
    return set_err(MJG_E_INVALID, "sheet %dx%d of %dx%d cells, margin %d, padding %d: not multiples of the encoded "
                   "format's chroma sub-sampling (%dx%d)", s.cols, s.rows, k.dst_w, k.dst_h, s.margin, s.padding,
                   1 << lay->hsh, 1 << lay->vsh);
  lay->has_sheet = true;
  lay->sheet = s;
  if (!s.nb_frames) lay->sheet.nb_frames = (int)cells;
  lay->tw = (int)W, lay->th = (int)H;
  return MJG_OK;
}

// open, step 1c: the denoiser (mjg_open_denoise; null: none) on the layout the two steps above resolved.
// The tables are taken as they are: the kernels clamp every index, so no table can make an address.
int check_denoise(const mjg_denoise *dn, Layout *lay) {
  if (!dn) return MJG_OK;
  if (lay->has_sheet)
    return set_err(MJG_E_INVALID, "denoise in front of a sheet (%dx%d): a denoiser context has no contact sheet",
                   lay->sheet.cols, lay->sheet.rows);
  lay->dn = dn;
  return MJG_OK;
}

// open, step 2: the geometry (no device, no environment): EncGeom, PadGeom, the source offsets,
// the frame byte counts, scale / has_pad / rst, enc_ua (unaligned_fetch: MJG_UNALIGNED_FETCH is
// not 0) and the sizes and strides of the sws stage's planes.
int plan_geometry(const mjg_config &k, int src_cf, const Layout &lay, bool unaligned_fetch, mjg_ctx *c) {
  const int cx = lay.cx, cy = lay.cy, crw = lay.crw, crh = lay.crh, px = lay.px, py = lay.py;
  const int s_hsh = lay.s_hsh, s_vsh = lay.s_vsh, hsh = lay.hsh, vsh = lay.vsh;
  // the frame everything downstream reads: the oriented one (the source itself with orient 0; the
  // same bytes per frame either way, the formats that transpose have equal chroma shifts)
  const int fw = lay.ow, fh = lay.oh;
  c->orient = lay.orient;
  c->deint = lay.deint;
  c->has_pad = lay.has_pad;
  // the sws stage: a resize, or a -pix_fmt conversion (source format != encoded format; in
  // FFmpeg one swscale context does both, and tv->pc in the same pass)
  const int cf = k.chroma_format;
  // (a pad always runs it: k_encode then reads the canvas in d_scaled as any other sws output)
  // (so does a sharpen: k_unsharp_plane reads full-range encoder-input samples from d_scaled)
  c->sharp = lay.sharp;
  c->us = lay.us;
  // (and a table behind it: k_lut_plane maps the picture in d_scaled)
  for (int i = 0; i < 2; i++) {
    c->has_lut[i] = lay.lut[i] != nullptr;
    if (lay.lut[i]) c->lut[i] = *lay.lut[i];
  }
  c->has_cmat = lay.cm != nullptr;
  if (lay.cm) c->cmat = *lay.cm;
  // (and a sheet: k_tile_plane reads the cells from d_scaled / d_sharp)
  c->sheet = lay.has_sheet;
  c->sh = lay.sheet;
  c->scale = (crw != k.dst_w || crh != k.dst_h || src_cf != cf || c->has_pad || c->sharp || c->has_lut[1] || c->sheet);
  const int scw = (fw + s_hsh) >> s_hsh, sch = (fh + s_vsh) >> s_vsh;
  // the rectangle's chroma planes: at (cx >> hs, cy >> vs), the chroma size of a crw x crh frame
  // (inside the source's: cx, cy are multiples of the sub-sampling)
  const int ccw = (crw + s_hsh) >> s_hsh, cch = (crh + s_vsh) >> s_vsh;
  c->src_cplane = (long long)scw * sch;
  c->src_off[0] = (long long)cy * fw + cx;
  c->src_off[1] = (long long)fw * fh + (long long)(cy >> s_vsh) * scw + (cx >> s_hsh);
  c->src_off[2] = c->src_off[1] + c->src_cplane;
  // the encoded frame: the canvas under a pad, else the picture (the sws stage's output, or the
  // source rectangle itself); pcw x pch: the picture's chroma planes
  const int pcw = (k.dst_w + hsh) >> hsh, pch = (k.dst_h + vsh) >> vsh;
  {
    const int w = lay.pw, h = lay.ph, cw = (w + hsh) >> hsh, ch = (h + vsh) >> vsh;
    for (int p = 0; p < 2; p++) {
      PadGeom &q = c->pad[p];
      q.cw = p ? cw : w;
      q.ch = p ? ch : h;
      q.cw_magic = magic32((uint32_t)q.cw);
      q.px = p ? px >> hsh : px;
      q.py = p ? py >> vsh : py;
      q.fill = p ? 128 : 0;
    }
    c->pic_frame_bytes = (size_t)w * h + 2 * (size_t)cw * ch;
    c->pic_u_off = (long long)w * h;
    c->pic_cplane = (long long)cw * ch;
  }
  c->in_frame_bytes = (size_t)fw * fh + 2 * (size_t)scw * sch;
  // ... and under a sheet the sheet, which k_tile_plane makes of the sws stage's output
  const int w = lay.has_sheet ? lay.tw : lay.pw, h = lay.has_sheet ? lay.th : lay.ph;
  const int cw = (w + hsh) >> hsh, ch = (h + vsh) >> vsh;
  c->enc_frame_bytes = (size_t)w * h + 2 * (size_t)cw * ch;

  EncGeom &g = c->geom;
  g.w = w;
  g.h = h;
  g.cw = cw;
  g.ch = ch;
  g.bpm = cf == MJG_CHROMA_422 ? 8 : 6;
  g.bpm_magic = magic32((uint32_t)g.bpm);
  g.lmw = cf == MJG_CHROMA_444 ? 8 : 16;
  g.cmh = cf == MJG_CHROMA_420 ? 8 : 16;
  g.mbw = (w + g.lmw - 1) / g.lmw;
  const int mbh = (h + 15) / 16;
  g.nmcu = g.mbw * mbh;
  g.mbw_magic = magic32((uint32_t)g.mbw);
  if ((uint64_t)(g.nmcu + 64) * (uint64_t)g.mbw >= ((uint64_t)1 << 32))
    return set_err(MJG_E_INVALID, "frame too large (%d MCUs)", g.nmcu);
  // RST: one segment per MCU row (mpegvideo clips the slice count to mb_height, so a
  // single-row picture has no restart markers)
  c->rst = (k.flags & MJG_F_RST) && mbh > 1;
  g.nseg = c->rst ? mbh : 1;
  g.seg_blocks = (c->rst ? g.mbw : g.nmcu) * g.bpm;
  g.nchunks = (g.seg_blocks + 63) / 64;  // chunks of 64 blocks (one wave each) per segment
  g.nchunks_magic = magic40((unsigned long long)g.nchunks);
  g.nseg_magic = magic40((unsigned long long)g.nseg);
  // task t / nchunks by magic (exact while t * nchunks < 2^40, t < max_batch * nseg * nchunks)
  // (under a sheet the sheets a launch may yield: each of up to kMaxSegs segments ends with a partial one)
  const int N = lay.has_sheet ? lay.sheet.nb_frames : 1;
  const unsigned long long max_enc = lay.has_sheet ? (unsigned long long)((k.max_batch + N - 1) / N + kMaxSegs - 1) : k.max_batch;
  if (max_enc * g.nseg * g.nchunks * g.nchunks >= ((unsigned long long)1 << 40))
    return set_err(MJG_E_INVALID, "max_batch %d too large for this frame size", k.max_batch);
  // k_encode reads the sws stage's packed output, or the source frames in place: rows at the
  // source planes' strides, the block offsets from the rectangle's first luma byte (submit_impl
  // adds src_off[0] to the frame pointers), the planes w x h / cw x ch of it (fetch_rows_edge's
  // clamps).  The whole frame in place: exactly the packed values.
  g.y_stride = c->scale ? w : fw;
  g.c_stride = c->scale ? cw : scw;
  g.u_off = c->scale ? (long long)w * h : c->src_off[1] - c->src_off[0];
  g.v_off = c->scale ? g.u_off + (long long)cw * ch : c->src_off[2] - c->src_off[0];
  g.frame_stride = (long long)(c->scale ? c->enc_frame_bytes : c->in_frame_bytes);
  // k_encode addresses a frame with 32-bit offsets
  if (c->enc_frame_bytes >= ((size_t)1 << 32) || (!c->scale && c->in_frame_bytes >= ((size_t)1 << 32)))
    return set_err(MJG_E_INVALID, "frame of %zu bytes", std::max(c->enc_frame_bytes, c->in_frame_bytes));
  // the fetch at any alignment: only for a crop read in place, and only when a plane offset, a
  // row stride or the frame stride is no multiple of 8 (else every interior block already
  // passes the alignment test, given an aligned frame pointer, as for uncropped frames)
  const bool is_crop = cx || cy || crw != fw || crh != fh;
  const long long bits = c->src_off[0] | c->src_off[1] | c->src_off[2] | g.y_stride | g.c_stride | g.frame_stride;
  c->enc_ua = is_crop && !c->scale && (bits & 7) != 0 && unaligned_fetch;
  g.range_convert = (!c->scale && !k.in_full_range) ? 1 : 0;
  g.debug_coefs = (k.flags & MJG_F_DEBUG_COEFS) ? 1 : 0;
  for (int p = 0; p < 2 && c->scale; p++) {  // the sws stage's planes: the rectangle's -> the picture's
    ScaleGeom &sg = c->ps[p].g;
    sg.sw = p ? ccw : crw;
    sg.sh = p ? cch : crh;
    sg.dw = p ? pcw : k.dst_w;
    sg.dh = p ? pch : k.dst_h;
    sg.s_stride = p ? scw : fw;  // rows of the source plane (wider than sw under a crop)
    sg.sw_magic = magic32((uint32_t)sg.sw);
    sg.d_stride = c->pad[p].cw;  // the encoded plane's rows: dw, or the wider canvas under a pad
    sg.s_fstride = (long long)c->in_frame_bytes;
    sg.d_fstride = (long long)c->pic_frame_bytes;
    sg.range = k.in_full_range ? 0 : (p ? 2 : 1);
  }
  return MJG_OK;
}

// open, step 3 (no device, no environment): the device table block for an encoded format cf
// (bpm blocks per MCU) and the quantiser qmat.  [0,256) AC luma, [256,512) AC chroma, [512,528)
// DC luma, [528,544) DC chroma ((len << 16) | code), [544,608) qmat column-major ([col][row]),
// [608,672) k_encode's screening thresholds B^2 (fp32 bits, [col][row]): a quantised AC
// coefficient is nonzero iff |u| >= T = ceil(5*2^18 / qmat) (dct_quantize_c intra
// rounding), i.e. |pass-2 sum| >= 16T - 8 (rows 0, 4: DESCALE 4, exact in fp32) or
// >= T*2^17 - 2^16 (other rows); the latter is widened by 2048 > the fp32 error (< 2^9).
void build_tabs(int cf, int bpm, const int32_t qmat[64], uint32_t tabs[kTabWords]) {
  memset(tabs, 0, kTabWords * sizeof(uint32_t));
  build_huffman(tabs, kBitsAcLum, kValAcLum);
  build_huffman(tabs + 256, kBitsAcChr, kValAcChr);
  uint32_t dc[256];
  build_huffman(dc, kBitsDcLum, kValDc);
  for (int i = 0; i < 16; i++) tabs[512 + i] = dc[i];
  build_huffman(dc, kBitsDcChr, kValDc);
  for (int i = 0; i < 16; i++) tabs[528 + i] = dc[i];
  for (int i = 0; i < 64; i++) tabs[544 + (i & 7) * 8 + (i >> 3)] = (uint32_t)qmat[i];  // [col][row]
  for (int i = 1; i < 64; i++) {
    const int ro = i >> 3;
    const uint32_t qm = (uint32_t)qmat[i];
    const double Ti = (double)(((5u << 18) + qm - 1) / qm);  // ceil(5*2^18 / qmat)
    const double B = (ro == 0 || ro == 4) ? 16.0 * Ti - 8.5 : Ti * 131072.0 - 65536.0 - 2048.0;
    const float b2 = (float)(B * B);
    memcpy(&tabs[608 + (i & 7) * 8 + ro], &b2, 4);
  }
  // [680, 686): k_encode's column-skip limits for columns 2-7, one fp32 word per column
  // (words 686-703 are free).  A column's AC outputs all quantise to zero if
  //   row 0:  |S| = |sum u_r| <= 16 T - 9          <= 8 max|u_r|, max|u_r| <= amax = 2T - 2
  //   row 4:  |S| = |sum +-u_r| <= 16 T - 9        <= 4 R  (the +-1 row sums to 0)
  //   others: |S| <= T 2^17 - 2^16 - 1             <= L1(row) R / 2
  // (T = ceil(5 2^18 / qmat) of that output, R = max - min of the column's row-pass values
  // u_r, S the pass-2 sum before DESCALE; dct_quantize_c gives 0 iff |DESCALE(S)| < T), i.e.
  // if max|u_r| <= amax and R <= Rmax, Rmax the smallest of the rows' limits on R.  Since
  // R <= 2 max|u_r|, both hold when max|u_r| <= A = min(amax, floor(Rmax / 2)).  row_pass
  // tests the fp32 value v_r it has before its rounding add: u_r = RNE(v_r), v_r a multiple
  // of 2^-10 and never a tie, so |v_r| <= A + 1/2 - 2^-10  <=>  |u_r| <= A.  Column 4's v_r is
  // u_r / 16 (an integer), its limit is scaled alike.  A <= 2 * 1275 - 2: the limit is exact
  // in fp32.  A column with A = 0 never skips (limit -1 < 0 <= max|v_r|).
  {
    static const int kDot[64] = MJG_PASS2_DOT;
    for (int col = 2; col < 8; col++) {
      long long rmax = 65535, amax = 0;
      for (int ro = 0; ro < 8; ro++) {
        const long long qm = qmat[ro * 8 + col];
        const long long T = ((5ll << 18) + qm - 1) / qm;
        if (ro == 0) {
          amax = std::max(0ll, 2 * T - 2);
        } else if (ro == 4) {
          rmax = std::min(rmax, 4 * T - 3);
        } else {
          long long l1 = 0;
          for (int r = 0; r < 8; r++) l1 += std::abs(kDot[ro * 8 + r]);
          rmax = std::min(rmax, (2 * (T * 131072 - 65536 - 1)) / l1);
        }
      }
      const long long A = std::min(amax, std::max(0ll, rmax) / 2);
      float lim = A > 0 ? (float)((double)A + 0.5 - 1.0 / 1024) : -1.0f;
      if (col == 4 && A > 0) lim *= 1.0f / 16;
      memcpy(&tabs[680 + col - 2], &lim, 4);
    }
  }
  // [672, 680): block-of-MCU descriptors in coding order (EncGeom): plane | chroma table << 2 |
  // dx8 << 3 | dy8 << 4 | DC predecessor distance << 8 (ff_mjpeg_encode_mb order; the
  // predecessor is the previous block of the same component)
  {
    static const uint8_t kPlane[3][8] = {{0, 0, 0, 0, 1, 2}, {0, 0, 0, 0, 1, 1, 2, 2}, {0, 0, 1, 1, 2, 2}};
    static const uint8_t kDx[3][8] = {{0, 1, 0, 1, 0, 0}, {0, 1, 0, 1, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
    static const uint8_t kDy[3][8] = {{0, 0, 1, 1, 0, 0}, {0, 0, 1, 1, 0, 1, 0, 1}, {0, 1, 0, 1, 0, 1}};
    for (int j = 0; j < bpm; j++) {
      const int pl = kPlane[cf][j];
      int delta = 0;  // distance back to the previous block of plane pl (wrapping to the previous MCU)
      for (int d = 1; d <= bpm && !delta; d++)
        if (kPlane[cf][((j - d) % bpm + bpm) % bpm] == pl) delta = d;
      tabs[672 + j] = (uint32_t)pl | (pl ? 4u : 0u) | ((uint32_t)kDx[cf][j] << 3) |
                      ((uint32_t)kDy[cf][j] << 4) | ((uint32_t)delta << 8);
    }
  }
}

// The launchers of the plan, one instantiation per kernel instantiation; build_plan and
// pick_encode choose among them with the context's values.
template <int HT, int NPV, bool D4, int RANGE, int TH>
void launch_tile(const Pass &p, const ScaleGeom &g, const SegList &in, uint8_t *dst, int nz, hipStream_t st) {
  const PlaneScale &t = *p.ps;
  k_scale<HT, NPV, D4, RANGE, TH><<<g.gxy * nz, p.block, p.lds, st>>>(in, dst, g, t.hcp, t.hp, t.vcp, t.vps, t.hsum, t.mfb);
}
template <bool D4, int RANGE, bool HCL>
void launch_stream(const Pass &p, const ScaleGeom &g, const SegList &in, uint8_t *dst, int nz, hipStream_t st) {
  const PlaneScale &t = *p.ps;
  k_scale_stream<D4, RANGE, HCL><<<g.gxy * nz, p.block, p.lds, st>>>(in, dst, g, t.sq, t.hcp, t.hp, t.vcp, t.vps, t.hsum);
}
template <int RANGE, bool RECT>
void launch_copy(const Pass &p, const ScaleGeom &g, const SegList &in, uint8_t *dst, int nz, hipStream_t st) {
  k_plane_copy<RANGE, RECT><<<g.gxy * nz, p.block, 0, st>>>(in, dst, g);
}
template <int RANGE, bool COPY>
void launch_pad(const Pass &p, const ScaleGeom &g, const SegList &in, uint8_t *dst, int nz, hipStream_t st) {
  k_pad_plane<RANGE, COPY><<<g.gxy * nz, p.block, 0, st>>>(in, dst, g, p.pad);
}

// A run-time flag or range (ScaleGeom::range, 0..2) as a compile-time constant: f gets it as a
// std::integral_constant, so one expression instantiates every cell of a kernel family
template <int V>
using int_c = std::integral_constant<int, V>;
template <typename F>
auto with_bool(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <typename F>
auto with_range(int r, F f) { return r == 1 ? f(int_c<1>{}) : r == 2 ? f(int_c<2>{}) : f(int_c<0>{}); }

// The sws stage's launches for luma and chroma (mjg_ctx::pass) from the planes' geometry and filters
void build_plan(mjg_ctx *c) {
  // workgroups per (plane, frame) of the copy kernels, and their magic, for a plane of `bytes`
  auto copy_grid = [](Pass &q, size_t bytes) {
    const size_t pieces = bytes >> 4, per = (size_t)kCopyThreads * kCopyVecs;
    q.block = kCopyThreads;
    q.g.gxy = (int)std::max<size_t>(1, (pieces + per - 1) / per);
    q.g.gxy_magic = magic32((uint32_t)q.g.gxy);
  };
  for (int p = 0; p < 2; p++) {
    const PlaneScale &ps = c->ps[p];
    Pass *next = c->pass[p];
    ScaleGeom g = ps.g;
    const long long plane_off = p ? c->pic_u_off : 0;  // the picture's (canvas) plane in a frame of the stage's output
    g.s_off = c->src_off[p];               // the (cropped) plane's first byte in a source frame
    g.d_off = plane_off + (long long)c->pad[p].py * c->pad[p].cw + c->pad[p].px;  // the picture's first byte in it
    // one dimension: tiles x planes x frames (scale.hip decodes it by multiply-high)
    g.gx = (int)ps.grid.x;
    g.gxy = (int)(ps.grid.x * ps.grid.y);
    g.gx_magic = magic32((uint32_t)g.gx);
    g.gxy_magic = magic32((uint32_t)g.gxy);
    if (c->has_pad) {  // the border, and with it a plane that keeps its size (scale.hip k_pad_plane)
      Pass &b = *next++;
      b.pad = c->pad[p];
      b.g = g;
      b.g.d_off = plane_off;
      copy_grid(b, (size_t)b.pad.cw * (size_t)b.pad.ch);
      b.launch = launch_pad<0, false>;
      if (ps.copy) b.launch = with_range(g.range, [](auto r) -> PassFn { return launch_pad<decltype(r)::value, true>; });
      if (ps.copy) continue;
    }
    Pass &m = *next;
    m.ps = &ps;
    m.g = g;
    if (ps.copy) {  // the plane keeps its size: streamed (scale.hip k_plane_copy)
      copy_grid(m, (size_t)g.sw * (size_t)g.sh);
      m.launch = with_range(g.range, [&](auto r) -> PassFn {
        if (g.s_stride != g.sw) return launch_copy<decltype(r)::value, true>;  // a rectangle of wider rows (crop)
        return launch_copy<decltype(r)::value, false>;
      });
      continue;
    }
    m.block = ps.stream ? kStreamThreads : 64 * scale_waves(ps.th);
    m.lds = ps.lds;
    m.launch = with_bool(ps.d4, [&](auto d4) {
      return with_range(g.range, [&](auto r) -> PassFn {
        constexpr bool D4 = decltype(d4)::value;
        constexpr int R = decltype(r)::value;
        if (ps.stream && ps.hcl) return launch_stream<D4, R, true>;  // past one LDS tile: strips x bands
        if (ps.stream) return launch_stream<D4, R, false>;
        if (g.htaps == 8 && g.npv == 5 && ps.th == 64) return launch_tile<8, 5, D4, R, 64>;  // 2:1 downscale (4K -> 1080p)
        if (g.htaps == 8 && g.npv == 5) return launch_tile<8, 5, D4, R, 32>;  // ... whose windows miss the 64-row fast path
        if (g.htaps == 4 && g.npv == 3) return launch_tile<4, 3, D4, R, 32>;  // upscale / mild downscale
        return launch_tile<0, 0, D4, R, 32>;
      });
    });
  }
}

template <bool T, bool FX>
void launch_orient(const OrientGeom &g, const SegList &in, uint8_t *dst, int nz, hipStream_t st) {
  k_orient_plane<T, FX><<<g.gxy * nz, kCopyThreads, 0, st>>>(in, dst, g);
}

// The orientation stage's launches for luma and chroma (mjg_ctx::opass; no device, no
// environment): the decoded frame's planes in the source format -> the same planes of the
// oriented frame, both packed planar and in_frame_bytes apart
void plan_orient(const mjg_config &k, const Layout &lay, mjg_ctx *c) {
  if (!lay.orient) return;
  const bool T = lay.orient & 1, FX = (lay.orient & 2) != 0;
  for (int p = 0; p < 2; p++) {
    OrientPass &q = c->opass[p];
    OrientGeom &g = q.g;
    g.sw = p ? (k.src_w + lay.s_hsh) >> lay.s_hsh : k.src_w;
    g.sh = p ? (k.src_h + lay.s_vsh) >> lay.s_vsh : k.src_h;
    g.s_off = g.d_off = p ? (long long)k.src_w * k.src_h : 0;
    g.s_fstride = g.d_fstride = (long long)c->in_frame_bytes;
    g.fy = (lay.orient & 4) ? 1 : 0;
    g.sw_magic = magic32((uint32_t)g.sw);
    g.tx = (g.sw + kOrientTile - 1) / kOrientTile;
    g.ntiles = g.tx * ((g.sh + kOrientTileH - 1) / kOrientTileH);
    g.tx_magic = magic32((uint32_t)g.tx);
    const size_t pieces = ((size_t)g.sw * g.sh) >> 4, per = (size_t)kCopyThreads * kCopyVecs;
    g.gxy = T ? (g.ntiles + kOrientWaves - 1) / kOrientWaves : (int)std::max<size_t>(1, (pieces + per - 1) / per);
    g.gxy_magic = magic32((uint32_t)g.gxy);
    q.launch = with_bool(T, [&](auto t) {
      return with_bool(FX, [](auto fx) -> OrientFn { return launch_orient<decltype(t)::value, decltype(fx)::value>; });
    });
  }
}

template <bool NOSPATIAL>
void launch_deint(const DeintGeom &g, const SegList &in, uint8_t *dst, int nz, hipStream_t st) {
  k_yadif_plane<NOSPATIAL><<<g.gxy * nz, kDeintThreads, 0, st>>>(in, dst, g);
}

// The deinterlacer's launches for luma and chroma (mjg_ctx::dpass; no device, no environment): the
// decoded frame's planes in the source format -> the same planes of the deinterlaced frame, both
// packed planar and in_frame_bytes apart.  submit_impl adds nf, the U+V pairing and the segments'
// readable frames.
void plan_deint(const mjg_config &k, const Layout &lay, mjg_ctx *c) {
  if (!lay.deint) return;
  for (int p = 0; p < 2; p++) {
    DeintPass &q = c->dpass[p];
    DeintGeom &g = q.g;
    g.w = p ? (k.src_w + lay.s_hsh) >> lay.s_hsh : k.src_w;
    g.h = p ? (k.src_h + lay.s_vsh) >> lay.s_vsh : k.src_h;
    g.off = p ? (long long)k.src_w * k.src_h : 0;
    g.fstride = (long long)c->in_frame_bytes;
    g.parity = (lay.deint & MJG_DEINT_BFF) ? 1 : 0;  // parity = tff ^ 1
    g.w_magic = magic32((uint32_t)g.w);
    const size_t pieces = ((size_t)g.w * g.h) >> 4;
    g.gxy = (int)std::max<size_t>(1, (pieces + kDeintThreads - 1) / kDeintThreads);
    g.gxy_magic = magic32((uint32_t)g.gxy);
    q.launch = with_bool((lay.deint & MJG_DEINT_NOSPATIAL) != 0,
                         [](auto ns) -> DeintFn { return launch_deint<decltype(ns)::value>; });
  }
}

// The denoiser's geometry for luma and chroma (mjg_ctx::dnpass, dn_grid, dn_felems; no device, no
// environment): the decoded frame's planes in the source format -> the same planes of the denoised frame,
// both packed planar and in_frame_bytes apart, through the uint16 layout of d_dn16 (rows a multiple of 64
// elements apart).  dn_launch adds nf, cont, the kernel's grid and the U + V pairing.
void plan_dn(const mjg_config &k, const Layout &lay, mjg_ctx *c) {
  c->dn = lay.dn != nullptr;
  if (!lay.dn) return;
  c->dn_tabs.assign(1, *lay.dn);
  const int cw = (k.src_w + lay.s_hsh) >> lay.s_hsh, ch = (k.src_h + lay.s_vsh) >> lay.s_vsh;
  const int py = (k.src_w + 63) & ~63, pc = (cw + 63) & ~63;
  c->dn_felems = (size_t)py * k.src_h + 2 * (size_t)pc * ch;
  for (int p = 0; p < 2; p++) {
    DnGeom &g = c->dnpass[p];
    g = DnGeom{};
    g.w = p ? cw : k.src_w, g.h = p ? ch : k.src_h;
    g.pitch = p ? pc : py;
    g.off = p ? (long long)k.src_w * k.src_h : 0;
    g.fstride = (long long)c->in_frame_bytes;
    g.off16 = p ? (long long)py * k.src_h : 0;
    g.fstride16 = (long long)c->dn_felems;
    g.tab = p;
    g.w_magic = magic32((uint32_t)g.w);
    c->dn_grid[p][0] = (g.h + 64 * kDnRowWaves - 1) / (64 * kDnRowWaves);
    c->dn_grid[p][1] = (g.w + 8 * kDnColThreads - 1) / (8 * kDnColThreads);
    const size_t pieces = ((size_t)g.w * g.h) >> 4;
    c->dn_grid[p][2] = (int)std::max<size_t>(1, (pieces + kDnTimeThreads - 1) / kDnTimeThreads);
  }
}

template <int MX, int MY>
void launch_sharp(const SharpGeom &g, const uint8_t *src, uint8_t *dst, int nz, hipStream_t st) {
  k_unsharp_plane<MX, MY><<<g.gxy * nz, kSharpThreads, 0, st>>>(src, dst, g);
}

// The sharpen's launches for luma and chroma (mjg_ctx::shpass; no device, no environment): the
// encoded frame's planes (the canvas planes under a pad, the picture at the pad's place) of the
// sws stage's buffer -> the same planes of d_sharp.  A plane whose amount is 0 is copied by the
// same kernel.  submit_impl adds nf and the U + V pairing.
void plan_sharp(const mjg_config &k, const Layout &lay, mjg_ctx *c) {
  if (!lay.sharp) return;
  for (int p = 0; p < 2; p++) {
    const PadGeom &q = c->pad[p];
    const int w = p ? (k.dst_w + lay.hsh) >> lay.hsh : k.dst_w, h = p ? (k.dst_h + lay.vsh) >> lay.vsh : k.dst_h;
    const int mx = p ? lay.us.cx : lay.us.lx, my = p ? lay.us.cy : lay.us.ly;
    SharpPass &s = c->shpass[p];
    s.g = sharp_geom(q.cw, q.ch, q.px, q.py, w, h, p ? c->pic_u_off : 0, (long long)c->pic_frame_bytes, mx, my,
                     p ? lay.us.ca : lay.us.la);
    s.launch = mx == 5 && my == 5 ? launch_sharp<5, 5> : launch_sharp<0, 0>;
  }
}

// The sheet's launches for luma and chroma (mjg_ctx::tpass; no device, no environment): the cell's
// planes in the sws stage's (the sharpen's) buffer -> the sheet's planes in d_tile.  submit_impl adds
// ns, the U + V pairing and the segments' sheets and frames.
void plan_tile(const mjg_config &k, const Layout &lay, mjg_ctx *c) {
  if (!lay.has_sheet) return;
  const mjg_sheet &s = lay.sheet;
  const EncGeom &e = c->geom;
  for (int p = 0; p < 2; p++) {
    const int hs = p ? lay.hsh : 0, vs = p ? lay.vsh : 0;
    TileGeom &g = c->tpass[p];
    g = TileGeom{};
    g.w = k.dst_w >> hs, g.h = k.dst_h >> vs;  // (multiples of the sub-sampling: check_sheet)
    g.W = p ? e.cw : e.w, g.H = p ? e.ch : e.h;
    g.pw = g.w + (s.padding >> hs), g.ph = g.h + (s.padding >> vs);
    g.mx = s.margin >> hs, g.my = s.margin >> vs;
    g.cols = s.cols, g.ncells = s.cols * s.rows, g.N = s.nb_frames;
    g.fill = p ? 128 : 0;
    g.s_off = p ? c->pic_u_off : 0, g.d_off = p ? e.u_off : 0;
    g.s_fstride = (long long)c->pic_frame_bytes, g.d_fstride = (long long)c->enc_frame_bytes;
    g.W_magic = magic32((uint32_t)g.W), g.pw_magic = magic32((uint32_t)g.pw), g.ph_magic = magic32((uint32_t)g.ph);
    g.gxy = tile_gxy(g.W, g.H);
    g.gxy_magic = magic32((uint32_t)g.gxy);
  }
}

// The table stages' launches for luma and chroma (mjg_ctx::lpass; no device, no environment).  Slot
// "in": the whole planes of the frame behind the orientation, source format, frames in_frame_bytes
// apart on both sides.  Slot "out": the picture's planes in d_scaled, at the canvas stride and the
// picture's place under a pad, in place.  submit_impl adds nf, the U + V pairing and, for slot
// "in", whether the stage runs in place.
void plan_lut(const mjg_config &k, const Layout &lay, mjg_ctx *c) {
  for (int slot = 0; slot < 2; slot++) {
    if (!c->has_lut[slot]) continue;
    const mjg_lut &L = c->lut[slot];
    int ident = 0;
    const uint8_t *t[3] = {L.y, L.u, L.v};
    for (int i = 0; i < 3; i++) {
      bool id = true;
      for (int v = 0; v < 256; v++) id = id && t[i][v] == v;
      ident |= id ? 1 << i : 0;
    }
    for (int p = 0; p < 2; p++) {
      LutGeom &g = c->lpass[slot][p];
      g = LutGeom{};
      if (!slot) {
        const int w = p ? (lay.ow + lay.s_hsh) >> lay.s_hsh : lay.ow, h = p ? (lay.oh + lay.s_vsh) >> lay.s_vsh : lay.oh;
        lut_geom_rect(g, w, h, w, w);
        g.s_off = g.d_off = p ? (long long)lay.ow * lay.oh : 0;
        g.s_fstride = g.d_fstride = (long long)c->in_frame_bytes;
      } else {
        const PadGeom &pg = c->pad[p];
        const int w = p ? (k.dst_w + lay.hsh) >> lay.hsh : k.dst_w, h = p ? (k.dst_h + lay.vsh) >> lay.vsh : k.dst_h;
        lut_geom_rect(g, w, h, pg.cw, pg.cw);
        g.s_off = g.d_off = (p ? c->pic_u_off : 0) + (long long)pg.py * pg.cw + pg.px;
        g.s_fstride = g.d_fstride = (long long)c->pic_frame_bytes;
      }
      g.tab = p;
      g.ident = ident;
      g.ds_magic = magic32((uint32_t)g.d_stride);
      g.gxy_magic = magic32((uint32_t)g.gxy);
    }
  }
}

template <int HS, int VS>
void launch_cmat(const SegList &in, uint8_t *dst, const CmatGeom &g, const CmatCoef &cm, int n, hipStream_t st) {
  k_cmat_frame<HS, VS><<<g.gxy * n, kCmatThreads, 0, st>>>(in, dst, g, cm);
}

// The colour matrix's launch (mjg_ctx::cgeom, cmat_launch; no device, no environment): the whole
// frame behind the orientation, source format, frames in_frame_bytes apart on both sides.
void plan_cmat(const Layout &lay, mjg_ctx *c) {
  if (!c->has_cmat) return;
  CmatGeom &g = c->cgeom;
  g = CmatGeom{};
  cmat_geom_frame(g, lay.ow, lay.oh, lay.s_hsh, lay.s_vsh);
  g.s_fstride = g.d_fstride = (long long)c->in_frame_bytes;
  g.ppr_magic = magic32((uint32_t)g.ppr);
  g.gxy_magic = magic32((uint32_t)g.gxy);
  c->cmat_launch = !lay.s_hsh ? launch_cmat<0, 0> : lay.s_vsh ? launch_cmat<1, 1> : launch_cmat<1, 0>;
}

// RC, DBG, UA: EncGeom's range_convert and debug_coefs, and the context's enc_ua (a crop read in
// place at any alignment, fetch_rows<UA>)
template <bool RC, int MODE, bool DBG, bool UA>
void launch_encode(const mjg_ctx *c, Slot &S, const SegList &enc_in, int wgs, int ntasks) {
  k_encode<RC, MODE, DBG, UA><<<wgs, 64 * kWavesPerWg, 0, S.st>>>(enc_in, c->geom, c->d_tabs, S.d_scratch, S.d_chunk_bits,
      S.d_dbg, S.d_work, ntasks, S.d_hist, S.d_stage_bits, S.d_syms, S.d_symn);
}
template <int MODE>
EncodeFn pick_encode(const mjg_ctx *c) {
  return with_bool(c->geom.range_convert, [&](auto rc) {
    return with_bool(c->geom.debug_coefs, [&](auto dbg) {
      return with_bool(c->enc_ua, [](auto ua) -> EncodeFn {
        return launch_encode<decltype(rc)::value, MODE, decltype(dbg)::value, decltype(ua)::value>;
      });
    });
  });
}

// open, step 4: the device part: streams, the merge depth, the tables' upload, the sws stage's
// filters and launch plan, the k_encode launchers and grid, slot 0
int open_device(mjg_ctx *c, const Layout &lay, const uint32_t *tabs) {
  const mjg_config &k = c->cfg;
  const EncGeom &g = c->geom;
  const int device = c->device;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return set_err(MJG_E_INVALID, "device %d of %d", device, ndev);
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  for (hipStream_t &st : c->more) HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  int least = 0, greatest = 0;  // the tail's workgroups first (see kSlots)
  HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
  HIP_TRY(hipStreamCreateWithPriority(&c->tail, hipStreamNonBlocking, greatest));

  c->slot_NC = (size_t)g.nchunks * g.nseg;
  c->slot_NS = (size_t)g.nseg;
  // merging (kMerge): opt-in with MJG_F_MERGE (a held submit's frames are read after mjg_submit
  // returns); MJG_MERGE=1 turns it off for a process (A/B), =2..4 sets the jobs per launch
  c->merge = (k.flags & MJG_F_MERGE) ? std::max(1, std::min(kMaxSegs, env_int("MJG_MERGE", kMerge))) : 1;
  if (c->deint || c->sheet || c->dn) c->merge = 1;  // a deint, a denoise or a sheet context neither holds nor merges submits (mjgpu.h)
  c->hold_idle = env_int("MJG_MERGE_HOLD", 1) != 0;
  if (c->merge > 1) {  // slot buffers for merge * max_batch frames: within a share of free memory
    size_t fr = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fr, &tot));
    const double per_frame = 2.0 * (double)c->slot_NC * kSlotWords * 4 + 2.0 * (double)c->enc_frame_bytes +
                             (c->orient ? (double)c->in_frame_bytes : 0.0) +  // (a deinterlacer never merges)
                             (c->sharp ? (double)c->enc_frame_bytes : 0.0) +
                             ((c->has_lut[0] || c->has_cmat) && !c->orient ? (double)c->in_frame_bytes : 0.0);
    if (kSlots * (double)c->merge * (double)k.max_batch * per_frame > kMergeMemShare * (double)fr) c->merge = 1;
  }
  if ((unsigned long long)k.max_batch * c->merge * g.nseg * g.nchunks * g.nchunks >= ((unsigned long long)1 << 40))
    c->merge = 1;  // merged launches would overflow k_encode's task magic (checked for max_batch above)
  c->slot_B = (size_t)k.max_batch * (size_t)c->merge;  // frames one launch may carry
  // ... and the frames it may encode: under a sheet ceil(count / N) sheets for each of up to kMaxSegs segments
  c->slot_BO = c->sheet ? (size_t)((k.max_batch + c->sh.nb_frames - 1) / c->sh.nb_frames + kMaxSegs - 1) : c->slot_B;
  // k_cmat_frame's grid is workgroups per frame x frames in x alone
  if (c->has_cmat && (unsigned long long)c->cgeom.gxy * c->slot_B > (unsigned long long)INT_MAX)
    return set_err(MJG_E_INVALID, "cmatrix: %d workgroups a frame x %zu frames a launch is past 2^31 - 1", c->cgeom.gxy,
                   c->slot_B);
  int rc;
  if ((rc = dmalloc(&c->d_tabs, kTabWords)) || (rc = dmalloc(&c->d_hdr, c->hdr.size()))) return rc;
  c->timing = (k.flags & (MJG_F_TIMING | MJG_F_TIMING_DETAIL)) != 0;
  c->timing_detail = (k.flags & MJG_F_TIMING_DETAIL) != 0;
  c->timing_tail = c->timing && !c->timing_detail && !env_int("MJG_TIMING_NOTAIL", 0);
  HIP_TRY(hipMemcpy(c->d_tabs, tabs, kTabWords * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_hdr, c->hdr.data(), c->hdr.size(), hipMemcpyHostToDevice));
  if (c->has_lut[0] || c->has_lut[1]) {
    if ((rc = dmalloc(&c->d_luts, 2 * sizeof(mjg_lut)))) return rc;
    HIP_TRY(hipMemcpy(c->d_luts, c->lut, 2 * sizeof(mjg_lut), hipMemcpyHostToDevice));
  }
  if (c->dn) {  // the four tables and the time scan's state (written before it is read: a first submit starts it)
    if ((rc = dmalloc(&c->d_dn_tabs, 4 * (size_t)kDnTabLen)) || (rc = dmalloc(&c->d_dn_state, c->in_frame_bytes))) return rc;
    HIP_TRY(hipMemcpy(c->d_dn_tabs, c->dn_tabs.data(), sizeof(mjg_denoise), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->d_dn_state, 0, c->in_frame_bytes * sizeof(uint16_t)));
  }

  if (c->scale) {
    const bool bitexact = !(k.flags & MJG_F_SWS_NO_BITEXACT);
    // the filters for the rectangle's planes: their edge taps replicate the crop's edge
    // MJG_SCALE_STREAM=1: every plane whose size changes through k_scale_stream (A/B, tests);
    // unset or auto: only the planes past one k_scale tile
    const bool force_stream = env_int("MJG_SCALE_STREAM", 0) == 1;
    // a plane that keeps its size (luma of a pure -pix_fmt conversion) is streamed by
    // k_plane_copy; MJG_PLANE_COPY=0 sends it through k_scale's identity filters (A/B, tests)
    const bool plane_copy = env_int("MJG_PLANE_COPY", 1) != 0;
    for (int p = 0; p < 2; p++) {
      PlaneScale &ps = c->ps[p];
      ScaleTabs t;
      if ((rc = plan_plane_scale(ps, t, lay, p != 0, bitexact, force_stream)) || (rc = upload_plane_scale(ps, t))) return rc;
      ps.copy = plane_copy && ps.g.sw == ps.g.dw && ps.g.sh == ps.g.dh;
    }
    build_plan(c);
  }
  c->enc_count = pick_encode<kCount>(c);
  c->enc_emit = pick_encode<kEmitDefault>(c);

  // persistent k_encode grid: every CU filled with as many workgroups as fit
  int ncu = 0, per_cu = 0;
  HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_encode<true, kEmitDefault>, 64 * kWavesPerWg, 0));
  c->enc_grid = std::max(1, ncu * std::max(1, per_cu));
  // -huffman optimal's counting pass is launched with the same grid (4 workgroups per CU: its
  // histograms are 16-bit counter pairs, profiles/r05/c1_count_occupancy_ab.txt)
  c->enc_grid_cnt = c->enc_grid;
  c->stage_cols = (size_t)c->enc_grid * kWavesPerWg * (c->optimal ? kEmitGridMul : 1);
  return alloc_slot(c, c->slot[0]);
}

// open, steps 1 and 2 as one: the checks, the geometry and every stage's launches (no device, no
// environment: unaligned_fetch is plan_geometry's).  A host program can call it on a `new mjg_ctx()`
// and walk the launches the *_launch functions below make of the plan (tools/stage_host.hip).
int plan_ctx(const mjg_config &k, const mjg_chain &chain, const mjg_sheet *sheet, bool unaligned_fetch, mjg_ctx *c,
             Layout *lay, const mjg_denoise *dn = nullptr) {
  int rc;
  if ((rc = check_config(k, chain, lay)) || (rc = check_sheet(k, sheet, lay)) || (rc = check_denoise(dn, lay))) return rc;
  if ((rc = plan_geometry(k, chain.src_chroma_format, *lay, unaligned_fetch, c))) return rc;
  plan_orient(k, *lay, c);
  plan_deint(k, *lay, c);
  plan_dn(k, *lay, c);
  plan_sharp(k, *lay, c);
  plan_lut(k, *lay, c);
  plan_cmat(*lay, c);
  plan_tile(k, *lay, c);
  return MJG_OK;
}

int open_ctx(int device, const mjg_config &k, const mjg_chain &chain, const mjg_sheet *sheet, const mjg_denoise *dn, mjg_ctx *c) {
  c->device = device;
  c->cfg = k;
  Layout lay;
  int rc;
  if ((rc = plan_ctx(k, chain, sheet, env_int("MJG_UNALIGNED_FETCH", 1) != 0, c, &lay, dn))) return rc;
  quant_matrix(k.qscale, c->mprime, c->qmat);
  c->hdr = build_header(c->geom.w, c->geom.h, c->mprime, k.sar_num, k.sar_den, (k.flags & MJG_F_COM_ITU601) != 0,
                        k.chroma_format, c->rst, &c->dht_pos, &c->dht_end);
  c->optimal = (k.flags & MJG_F_HUFFMAN_OPTIMAL) != 0;
  uint32_t tabs[kTabWords];
  build_tabs(k.chroma_format, c->geom.bpm, c->qmat, tabs);
  return open_device(c, lay, tabs);
}

// HIP events: with MJG_F_TIMING around scale, huff, encode and the whole tail (scan .. write,
// reported as MJG_K_TAIL); with MJG_F_TIMING_DETAIL around every kernel (each event record
// costs ~10 us of GPU idle between the short tail kernels).
void tmark(mjg_ctx *c, Slot &S, int k, int end) {
  if (!c->timing) return;
  const bool tail = is_tail_kernel(k);
  if (tail && !c->timing_detail) return;
  (void)hipEventRecord(S.ev[k][end], tail ? c->tail : S.st);
}

// The stuffing tail's launch sizes, one place for submit_impl, launch_write and mjg_debug_tail:
// groups a segment; k_scan_bits_seg's workgroups (a wave per segment, 4 a workgroup); k_count_ff's
// and k_write's (a wave per group, 4 a workgroup).  k_scan_bits and k_scan_ff take a workgroup a
// frame (1024 and 256 threads).
inline int tail_gps(int nchunks) { return (nchunks + kChunksPerWave - 1) / kChunksPerWave; }
inline int tail_seg_wgs(int nsegs) { return (nsegs + 3) / 4; }
inline int tail_group_wgs(int ngroups) { return (ngroups + 3) / 4; }
constexpr int kTailDone = 1;  // k_scan_ff's frame ticket: the `done` words k_scan_bits zeroes

// status: reset the overflow flag first (the regrow path; a submit's scan kernel resets it)
int launch_write(mjg_ctx *c, Slot &S, int n, bool reset_status) {
  const EncGeom &g = c->geom;
  const int gps = tail_gps(g.nchunks), ngroups = gps * n * g.nseg;
  if (reset_status) HIP_TRY(hipMemsetAsync(S.d_status, 0, 4, c->tail));
  tmark(c, S, MJG_K_WRITE, 0);
  k_write<<<tail_group_wgs(ngroups), 256, 0, c->tail>>>(
      S.d_stream, S.d_chunk_bits, S.d_chunk_off, S.d_frame_bits, S.d_ff_off, g.nchunks, gps, g.nseg, n,
      S.d_seg_size, S.d_seg_off, S.d_frame_offsets, c->d_hdr, (int)c->hdr.size(),
      c->optimal ? S.d_hdr_lens : nullptr, (int)c->dht_pos, (int)c->dht_end, S.d_dht,
      c->optimal ? S.d_dht_nval : nullptr, S.d_out, (uint64_t)S.out_cap, S.d_status);
  tmark(c, S, MJG_K_WRITE, 1);
  if (c->timing_tail && !reset_status) (void)hipEventRecord(S.ev[MJG_K_TAIL][1], c->tail);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(S.h_sizes, S.d_frame_size, n * sizeof(uint64_t), hipMemcpyDeviceToHost,
                         c->tail));
  HIP_TRY(hipMemcpyAsync(S.h_status, S.d_status, 4, hipMemcpyDeviceToHost, c->tail));
  HIP_TRY(hipEventRecord(S.done, c->tail));
  return MJG_OK;
}

}  // namespace

extern "C" {

int mjg_version(void) { return 105; }

const char *mjg_last_error(void) { return g_err.c_str(); }

int mjg_device_count(void) {
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  return n;
}

int mjg_device_numa_node(int device) {
  char bus[64] = {0};
  HIP_TRY(hipDeviceGetPCIBusId(bus, (int)sizeof bus, device));
  for (char *p = bus; *p; p++) *p = (char)tolower((unsigned char)*p);
  char path[160];
  snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
  FILE *f = fopen(path, "r");
  if (!f) return -1;
  int node = -1;
  if (fscanf(f, "%d", &node) != 1) node = -1;
  fclose(f);
  return node < 0 ? -1 : node;
}

int mjg_open_chain(int device, const mjg_config *cfg, const mjg_chain *chain, mjg_ctx **out) {
  return mjg_open_sheet(device, cfg, chain, nullptr, out);
}

int mjg_open_sheet(int device, const mjg_config *cfg, const mjg_chain *chain, const mjg_sheet *sheet, mjg_ctx **out) {
  return mjg_open_denoise(device, cfg, chain, sheet, nullptr, out);
}

int mjg_open_denoise(int device, const mjg_config *cfg, const mjg_chain *chain, const mjg_sheet *sheet,
                     const mjg_denoise *dn, mjg_ctx **out) {
  if (!cfg || !chain || !out) return set_err(MJG_E_INVALID, "null argument");
  *out = nullptr;
  mjg_ctx *c = new mjg_ctx();
  const int rc = open_ctx(device, *cfg, *chain, sheet, dn, c);
  if (rc) {
    const std::string keep = g_err;
    free_ctx(c);
    g_err = keep;
    return rc;
  }
  *out = c;
  return MJG_OK;
}

// The entry points from before mjg_chain: each is the chain it fills here, member by member.
// mjg_open_src gives neither rectangle, mjg_open_crop a crop and no pad, the others both.
int mjg_open_cmat(int device, const mjg_config *cfg, int src_chroma_format, int deint, int orient, int crop_x,
                  int crop_y, int crop_w, int crop_h, const mjg_cmatrix *cm, const mjg_lut *lut_in,
                  const mjg_lut *lut_out, const mjg_unsharp *us, int pad_x, int pad_y, int pad_w, int pad_h,
                  mjg_ctx **out) {
  mjg_chain ch{};
  ch.src_chroma_format = src_chroma_format, ch.deint = deint, ch.orient = orient;
  ch.cmat = cm;
  ch.lut_in = lut_in;
  ch.has_crop = 1, ch.crop_x = crop_x, ch.crop_y = crop_y, ch.crop_w = crop_w, ch.crop_h = crop_h;
  ch.lut_out = lut_out;
  ch.unsharp = us;
  ch.has_pad = 1, ch.pad_x = pad_x, ch.pad_y = pad_y, ch.pad_w = pad_w, ch.pad_h = pad_h;
  return mjg_open_chain(device, cfg, &ch, out);
}

int mjg_open_lut(int device, const mjg_config *cfg, int src_chroma_format, int deint, int orient, int crop_x,
                 int crop_y, int crop_w, int crop_h, const mjg_lut *lut_in, const mjg_lut *lut_out,
                 const mjg_unsharp *us, int pad_x, int pad_y, int pad_w, int pad_h, mjg_ctx **out) {
  mjg_chain ch{};
  ch.src_chroma_format = src_chroma_format, ch.deint = deint, ch.orient = orient;
  ch.lut_in = lut_in;
  ch.has_crop = 1, ch.crop_x = crop_x, ch.crop_y = crop_y, ch.crop_w = crop_w, ch.crop_h = crop_h;
  ch.lut_out = lut_out;
  ch.unsharp = us;
  ch.has_pad = 1, ch.pad_x = pad_x, ch.pad_y = pad_y, ch.pad_w = pad_w, ch.pad_h = pad_h;
  return mjg_open_chain(device, cfg, &ch, out);
}

int mjg_open_sharp(int device, const mjg_config *cfg, int src_chroma_format, int deint, int orient, int crop_x,
                   int crop_y, int crop_w, int crop_h, const mjg_unsharp *us, int pad_x, int pad_y, int pad_w,
                   int pad_h, mjg_ctx **out) {
  mjg_chain ch{};
  ch.src_chroma_format = src_chroma_format, ch.deint = deint, ch.orient = orient;
  ch.has_crop = 1, ch.crop_x = crop_x, ch.crop_y = crop_y, ch.crop_w = crop_w, ch.crop_h = crop_h;
  ch.unsharp = us;
  ch.has_pad = 1, ch.pad_x = pad_x, ch.pad_y = pad_y, ch.pad_w = pad_w, ch.pad_h = pad_h;
  return mjg_open_chain(device, cfg, &ch, out);
}

int mjg_open_deint(int device, const mjg_config *cfg, int src_chroma_format, int deint, int orient, int crop_x,
                   int crop_y, int crop_w, int crop_h, int pad_x, int pad_y, int pad_w, int pad_h, mjg_ctx **out) {
  mjg_chain ch{};
  ch.src_chroma_format = src_chroma_format, ch.deint = deint, ch.orient = orient;
  ch.has_crop = 1, ch.crop_x = crop_x, ch.crop_y = crop_y, ch.crop_w = crop_w, ch.crop_h = crop_h;
  ch.has_pad = 1, ch.pad_x = pad_x, ch.pad_y = pad_y, ch.pad_w = pad_w, ch.pad_h = pad_h;
  return mjg_open_chain(device, cfg, &ch, out);
}

int mjg_open_orient(int device, const mjg_config *cfg, int src_chroma_format, int orient, int crop_x, int crop_y,
                    int crop_w, int crop_h, int pad_x, int pad_y, int pad_w, int pad_h, mjg_ctx **out) {
  mjg_chain ch{};
  ch.src_chroma_format = src_chroma_format, ch.orient = orient;
  ch.has_crop = 1, ch.crop_x = crop_x, ch.crop_y = crop_y, ch.crop_w = crop_w, ch.crop_h = crop_h;
  ch.has_pad = 1, ch.pad_x = pad_x, ch.pad_y = pad_y, ch.pad_w = pad_w, ch.pad_h = pad_h;
  return mjg_open_chain(device, cfg, &ch, out);
}

int mjg_open_pad(int device, const mjg_config *cfg, int src_chroma_format, int crop_x, int crop_y, int crop_w,
                 int crop_h, int pad_x, int pad_y, int pad_w, int pad_h, mjg_ctx **out) {
  mjg_chain ch{};
  ch.src_chroma_format = src_chroma_format;
  ch.has_crop = 1, ch.crop_x = crop_x, ch.crop_y = crop_y, ch.crop_w = crop_w, ch.crop_h = crop_h;
  ch.has_pad = 1, ch.pad_x = pad_x, ch.pad_y = pad_y, ch.pad_w = pad_w, ch.pad_h = pad_h;
  return mjg_open_chain(device, cfg, &ch, out);
}

int mjg_open_crop(int device, const mjg_config *cfg, int src_chroma_format, int crop_x, int crop_y, int crop_w,
                  int crop_h, mjg_ctx **out) {
  mjg_chain ch{};
  ch.src_chroma_format = src_chroma_format;
  ch.has_crop = 1, ch.crop_x = crop_x, ch.crop_y = crop_y, ch.crop_w = crop_w, ch.crop_h = crop_h;
  return mjg_open_chain(device, cfg, &ch, out);
}

int mjg_open_src(int device, const mjg_config *cfg, int src_chroma_format, mjg_ctx **out) {
  mjg_chain ch{};
  ch.src_chroma_format = src_chroma_format;
  return mjg_open_chain(device, cfg, &ch, out);
}

int mjg_open(int device, const mjg_config *cfg, mjg_ctx **out) {
  if (!cfg || !out) return set_err(MJG_E_INVALID, "null argument");
  return mjg_open_src(device, cfg, cfg->chroma_format, out);
}

void mjg_close(mjg_ctx *ctx) { free_ctx(ctx); }

size_t mjg_frame_bytes(const mjg_ctx *ctx) { return ctx ? ctx->in_frame_bytes : 0; }

int mjg_header(const mjg_ctx *ctx, uint8_t *out, size_t cap, size_t *len) {
  if (!ctx) return set_err(MJG_E_INVALID, "null ctx");
  if (len) *len = ctx->hdr.size();
  if (!out) return MJG_OK;
  if (cap < ctx->hdr.size()) return set_err(MJG_E_CAPACITY, "header needs %zu bytes", ctx->hdr.size());
  memcpy(out, ctx->hdr.data(), ctx->hdr.size());
  return MJG_OK;
}

namespace {
// where slot "in"'s table stage and the colour matrix leave their frames: the buffer of the stage in front of them (in place), else d_lut
uint8_t *lut_in_buf(const mjg_ctx *c, const Slot &S) { return c->orient ? S.d_orient : c->dn ? S.d_dn : c->deint ? S.d_deint : S.d_lut; }

// The per-submit geometry: what a submit adds to the plan of open (plan_ctx).  No HIP call, so the
// host checks walk these very launches (tools/stage_host.hip).  A plane stage launches luma (p = 0),
// then U and V: in one launch (p = 1; V's blocks behind U's, reached through poff) while uv1, else
// in one each (p = 1 and 2; V alone moves off).  uv1 is uv_paired(frames): 2n fits the grid's z
// range.  Launch p has gxy * uv_nz(p, uv1, frames) workgroups.
constexpr bool uv_paired(int n) { return 2 * n <= 65535; }
static_assert(uv_paired(32767) && !uv_paired(32768), "submit_impl's three `uv1` locals state 65535 (tests/chain_geom.py)");
int uv_launches(bool uv1) { return uv1 ? 2 : 3; }
int uv_nz(int p, bool uv1, int n) { return p && uv1 ? 2 * n : n; }
// off, poff: one side's fields of the chroma plan's geom; cplane: bytes from the U to the V plane there
void uv_place(int p, bool uv1, long long cplane, long long &off, long long &poff) {
  if (p && uv1) poff = cplane;
  if (p == 2) off += cplane;
}

// frames of segment k of a submit of n: up to the next segment's first, or n (an unused one: 0)
int seg_count(const SegList &in, int k, int n) {
  if (in.f0[k] == INT_MAX) return 0;
  return (k + 1 < kMaxSegs && in.f0[k + 1] != INT_MAX ? in.f0[k + 1] : n) - in.f0[k];
}

// each segment is a sequence of its own: its frames [0, count), widened by the halo frames
DeintGeom deint_launch(const mjg_ctx *c, int p, bool uv1, int n, const SegList &in, int halo) {
  DeintGeom g = c->dpass[p ? 1 : 0].g;
  g.nf = n;
  for (int k = 0; k < kMaxSegs; k++) {
    g.lo[k] = -(halo & 1);
    g.hi[k] = in.f0[k] == INT_MAX ? 0 : seg_count(in, k, n) - 1 + ((halo >> 1) & 1);
  }
  uv_place(p, uv1, c->src_cplane, g.off, g.poff);
  return g;
}

// One launch of the denoiser's kernel `kern` (0 k_dn_rows, 1 k_dn_cols, 2 k_dn_time): its workgroups are
// g.gxy * dn_nz(kern, p, uv1, n).  The time scan runs over the frames inside a thread, so its grid has
// planes only: U and V paired is two of them.
DnGeom dn_launch(const mjg_ctx *c, int kern, int p, bool uv1, int n, int cont) {
  DnGeom g = c->dnpass[p ? 1 : 0];
  g.nf = n;
  g.cont = cont ? 1 : 0;
  g.gxy = c->dn_grid[p ? 1 : 0][kern];
  g.gxy_magic = magic32((uint32_t)g.gxy);
  uv_place(p, uv1, c->src_cplane, g.off, g.poff);
  const DnGeom &q = c->dnpass[1];
  uv_place(p, uv1, (long long)q.pitch * q.h, g.off16, g.poff16);
  return g;
}
int dn_nz(int kern, int p, bool uv1, int n) { return kern == 2 ? (p && uv1 ? 2 : 1) : uv_nz(p, uv1, n); }

OrientGeom orient_launch(const mjg_ctx *c, int p, bool uv1, int n) {
  OrientGeom g = c->opass[p ? 1 : 0].g;
  g.nf = n;
  uv_place(p, uv1, c->src_cplane, g.s_off, g.s_poff);
  uv_place(p, uv1, c->src_cplane, g.d_off, g.d_poff);
  return g;
}

// One launch of a table stage (slot 0 "in": source planes; 1 "out": the picture's).  in_place: dst
// holds the frames already, so a launch whose planes all have the identity table is left out
// (false); otherwise it copies them.
bool lut_launch(const mjg_ctx *c, int slot, int p, bool uv1, int n, bool in_place, LutGeom *out) {
  LutGeom &g = *out = c->lpass[slot][p ? 1 : 0];
  g.nf = n;
  const long long cplane = slot ? c->pic_cplane : c->src_cplane;
  uv_place(p, uv1, cplane, g.s_off, g.s_poff);
  uv_place(p, uv1, cplane, g.d_off, g.d_poff);
  if (p == 2) g.tab = 2;
  const int tabs = p && uv1 ? 6 : 1 << g.tab;  // the launch's tables, as bits of g.ident
  return !(in_place && (g.ident & tabs) == tabs);
}

ScaleGeom scale_launch(const mjg_ctx *c, const Pass &ps, int p, bool uv1, int n) {
  ScaleGeom g = ps.g;
  g.nf = n;
  uv_place(p, uv1, c->src_cplane, g.s_off, g.s_poff);
  uv_place(p, uv1, c->pic_cplane, g.d_off, g.d_poff);
  return g;
}

SharpGeom sharp_launch(const mjg_ctx *c, int p, bool uv1, int n) {
  SharpGeom g = c->shpass[p ? 1 : 0].g;
  g.nf = n;
  uv_place(p, uv1, c->pic_cplane, g.off, g.poff);
  return g;
}

// The frames k_encode codes: the n input frames, or under a sheet ceil(count / N) sheets for each
// segment, a sequence of its own (TileGeom's per-segment fields)
struct SheetSplit {
  int m, sheet0[kMaxSegs], first[kMaxSegs], count[kMaxSegs];
};
SheetSplit sheet_split(const mjg_ctx *c, const SegList &in, int n) {
  SheetSplit s{};
  s.m = n;
  if (!c->sheet) return s;
  s.m = 0;
  for (int k = 0; k < kMaxSegs; k++) {
    const bool used = in.f0[k] != INT_MAX;
    s.sheet0[k] = used ? s.m : INT_MAX;
    s.first[k] = used ? in.f0[k] : 0;
    s.count[k] = seg_count(in, k, n);
    s.m += (s.count[k] + c->sh.nb_frames - 1) / c->sh.nb_frames;
  }
  return s;
}

// the cells of each segment onto its sheets (uv1 is of the s.m sheets)
TileGeom tile_launch(const mjg_ctx *c, int p, bool uv1, const SheetSplit &s) {
  TileGeom g = c->tpass[p ? 1 : 0];
  g.ns = s.m;
  for (int k = 0; k < kMaxSegs; k++) g.sheet0[k] = s.sheet0[k], g.first[k] = s.first[k], g.count[k] = s.count[k];
  uv_place(p, uv1, c->pic_cplane, g.s_off, g.s_poff);
  uv_place(p, uv1, (long long)c->geom.cw * c->geom.ch, g.d_off, g.d_poff);
  return g;
}

// One table stage of a submit
void launch_lut(const mjg_ctx *c, const Slot &S, int slot, const SegList &in, uint8_t *dst, int n, bool uv1, bool in_place) {
  for (int p = 0; p < uv_launches(uv1); p++) {
    LutGeom g;
    if (!lut_launch(c, slot, p, uv1, n, in_place, &g)) continue;
    k_lut_plane<<<g.gxy * uv_nz(p, uv1, n), kCopyThreads, 0, S.st>>>(in, dst, c->d_luts + slot * sizeof(mjg_lut), g);
  }
}

// mjg_submit's body; segs (mjg_submit_segments: device frames) replaces the one segment at
// `frames` as the input of the sws stage, or of k_encode without one.  halo (a deint context's
// single-segment submit, mjg_submit_halo): bit 1, `frames` starts with one frame that is only
// read; bit 2, one such frame follows the n encoded ones.  cont (a denoise context's single-segment
// submit, mjg_submit_cont): the time scan starts from the carried state
int submit_impl(mjg_ctx *c, const uint8_t *frames, int n, int src_is_device, const SegList *segs, int halo = 0, int cont = 0) {
  if (n < 1 || (size_t)n > c->slot_B || (!src_is_device && n > c->cfg.max_batch))
    return set_err(MJG_E_INVALID, "nframes %d not in 1..%d", n, c->cfg.max_batch);
  if (c->nout == kSlots) return set_err(MJG_E_STATE, "%d submits queued: sync one first", kSlots);
  HIP_TRY(hipSetDevice(c->device));
  const EncGeom &g = c->geom;
  Slot &S = c->slot[c->head];
  if (!S.alloc) {  // slots 1.., on the first pipelined submits
    const int rc = alloc_slot(c, S);
    if (rc) return rc;
  }
  const uint8_t *src = frames;
  const int hp = halo & 1, hn = (halo >> 1) & 1;  // halo frames in front of and behind the encoded ones
  if (!src_is_device) {
    if (!S.d_stage) {  // staging for host submits, allocated on first use (a deinterlacer: room for the two halo frames)
      const int rc = dmalloc(&S.d_stage, (size_t)(c->cfg.max_batch + (c->deint ? 2 : 0)) * c->in_frame_bytes);
      if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(S.d_stage, frames, (size_t)(n + hp + hn) * c->in_frame_bytes, hipMemcpyHostToDevice, S.st));
    src = S.d_stage;
  }
  src += (size_t)hp * c->in_frame_bytes;  // the first encoded frame
  SegList in_sl = segs ? *segs : one_seg(src);  // the submit's input frames: the caller's segments, or one at src
  const SheetSplit sheets = sheet_split(c, in_sl, n);
  const int m = sheets.m;  // the frames k_encode codes
  if (c->scale || c->orient || c->deint || c->dn || c->has_lut[0] || c->has_cmat) tmark(c, S, MJG_K_SCALE, 0);
  if (c->deint) {  // in front of everything; the rest reads one buffer
    const bool uv1 = 2 * n <= 65535;
    for (int p = 0; p < uv_launches(uv1); p++)
      c->dpass[p ? 1 : 0].launch(deint_launch(c, p, uv1, n, in_sl, halo), in_sl, S.d_deint, uv_nz(p, uv1, n), S.st);
    HIP_TRY(hipGetLastError());
    // one buffer from here on; the denoiser still restarts at every segment's first frame
    in_sl = c->dn ? seg_starts(in_sl, S.d_deint, c->in_frame_bytes) : one_seg(S.d_deint);
  }
  if (c->dn) {  // behind the deinterlacer: rows, columns, then time, which carries the context's state
    const bool uv1 = uv_paired(n);
    for (int p = 0; p < uv_launches(uv1); p++) {
      const DnGeom g = dn_launch(c, 0, p, uv1, n, cont);
      k_dn_rows<<<g.gxy * dn_nz(0, p, uv1, n), kDnRowThreads, 0, S.st>>>(in_sl, S.d_dn16, c->d_dn_tabs, g);
    }
    for (int p = 0; p < uv_launches(uv1); p++) {
      const DnGeom g = dn_launch(c, 1, p, uv1, n, cont);
      k_dn_cols<<<g.gxy * dn_nz(1, p, uv1, n), kDnColThreads, 0, S.st>>>(S.d_dn16, c->d_dn_tabs, g);
    }
    // the state: the other slot's stream wrote it last (two streams, no host wait in between)
    if (c->dn_last) HIP_TRY(hipStreamWaitEvent(S.st, c->dn_last, 0));
    for (int p = 0; p < uv_launches(uv1); p++) {
      const DnGeom g = dn_launch(c, 2, p, uv1, n, cont);
      k_dn_time<<<g.gxy * dn_nz(2, p, uv1, n), kDnTimeThreads, 0, S.st>>>(in_sl, S.d_dn16, c->d_dn_state, S.d_dn,
                                                                        c->d_dn_tabs, g);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S.dn_done, S.st));
    c->dn_last = S.dn_done;
    c->dn_started = true;
    in_sl = one_seg(S.d_dn);
  }
  if (c->orient) {  // the first filter; the rest reads one buffer
    const bool uv1 = 2 * n <= 65535;
    for (int p = 0; p < uv_launches(uv1); p++)
      c->opass[p ? 1 : 0].launch(orient_launch(c, p, uv1, n), in_sl, S.d_orient, uv_nz(p, uv1, n), S.st);
    HIP_TRY(hipGetLastError());
    in_sl = one_seg(S.d_orient);
  }
  if (c->has_cmat) {  // behind the orientation: in place in that stage's buffer, else the caller's frames -> d_lut
    uint8_t *buf = lut_in_buf(c, S);
    const mjg_cmatrix &m = c->cmat;
    c->cmat_launch(in_sl, buf, c->cgeom, CmatCoef{m.yu, m.yv, m.uu, m.uv, m.vu, m.vv}, n, S.st);
    HIP_TRY(hipGetLastError());
    in_sl = one_seg(buf);
  }
  if (c->has_lut[0]) {  // behind the colour matrix: in place in the buffer in front, else the caller's frames -> d_lut
    uint8_t *buf = lut_in_buf(c, S);
    launch_lut(c, S, 0, in_sl, buf, n, uv_paired(n), buf != S.d_lut || c->has_cmat);
    HIP_TRY(hipGetLastError());
    in_sl = one_seg(buf);
  }
  SegList enc_in = in_sl;
  if (c->scale) {
    const bool uv1 = 2 * n <= 65535;
    for (int p = 0; p < uv_launches(uv1); p++)  // (U and V: the same filters)
      for (const Pass &ps : c->pass[p ? 1 : 0])
        if (ps.launch) ps.launch(ps, scale_launch(c, ps, p, uv1, n), in_sl, S.d_scaled, uv_nz(p, uv1, n), S.st);
    // a table on the picture, in place: behind every sws pass, in front of the sharpen
    if (c->has_lut[1]) launch_lut(c, S, 1, one_seg(S.d_scaled), S.d_scaled, n, uv1, true);
    const uint8_t *enc_buf = S.d_scaled;
    if (c->sharp) {  // behind the sws stage's passes (the pad's border among them)
      for (int p = 0; p < uv_launches(uv1); p++)
        c->shpass[p ? 1 : 0].launch(sharp_launch(c, p, uv1, n), S.d_scaled, S.d_sharp, uv_nz(p, uv1, n), S.st);
      enc_buf = S.d_sharp;
    }
    if (c->sheet) {  // behind the sharpen: the cells of each segment onto its sheets
      const bool tuv1 = uv_paired(m);
      for (int p = 0; p < uv_launches(tuv1); p++) {
        const TileGeom tg = tile_launch(c, p, tuv1, sheets);
        k_tile_plane<<<tg.gxy * uv_nz(p, tuv1, m), kCopyThreads, 0, S.st>>>(enc_buf, S.d_tile, tg);
      }
      enc_buf = S.d_tile;
    }
    tmark(c, S, MJG_K_SCALE, 1);
    HIP_TRY(hipGetLastError());
    enc_in = one_seg(enc_buf);  // k_encode reads the scaled (the sharpened) frames, one buffer
  } else {  // in place: EncGeom's offsets count from the rectangle's first luma byte (0: whole frames)
    if (c->orient || c->deint || c->dn || c->has_lut[0] || c->has_cmat) tmark(c, S, MJG_K_SCALE, 1);  // an orientation / a deinterlacer / a table / a matrix alone: the interval holds its passes
    for (int k = 0; k < kMaxSegs; k++) enc_in.p[k] += c->src_off[0];
  }
  const int ntasks = g.nchunks * g.nseg * m;
  const int nsegs = g.nseg * m;  // entropy-coded segments of this submit
  const int wgs = std::min((ntasks + kWavesPerWg - 1) / kWavesPerWg, c->enc_grid);
  if (c->optimal) {  // pass 1: symbol counts per frame, then the frame's tables
    tmark(c, S, MJG_K_HUFF, 0);
    HIP_TRY(hipMemsetAsync(S.d_hist, 0, (size_t)m * kFrameTabWords * 4, S.st));
    c->enc_count(c, S, enc_in, std::min(wgs, c->enc_grid_cnt), ntasks);
    HIP_TRY(hipMemsetAsync(S.d_work, 0, (size_t)kXcds * kCtrStride * 4, S.st));  // unit counters for pass 2
    k_huff_build<<<m * 4, 64, 0, S.st>>>(S.d_hist, S.d_ftabs, S.d_dht, S.d_dht_nval);
    tmark(c, S, MJG_K_HUFF, 1);
    HIP_TRY(hipGetLastError());
  }
  tmark(c, S, MJG_K_ENCODE, 0);
  if (c->optimal)
    k_emit_syms<<<c->enc_grid * kEmitGridMul, 64 * kWavesPerWg, 0, S.st>>>(g, c->d_tabs, S.d_ftabs, S.d_syms, S.d_symn,
                                                                           S.d_scratch, S.d_chunk_bits, S.d_stage_bits, ntasks);
  else
    c->enc_emit(c, S, enc_in, wgs, ntasks);
  tmark(c, S, MJG_K_ENCODE, 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(S.enc_done, S.st));
  HIP_TRY(hipStreamWaitEvent(c->tail, S.enc_done, 0));
  if (c->timing_tail) (void)hipEventRecord(S.ev[MJG_K_TAIL][0], c->tail);
  tmark(c, S, MJG_K_SCAN_BITS, 0);
  const int ndone = kTailDone;
  if (c->rst)
    k_scan_bits_seg<<<tail_seg_wgs(nsegs), 256, 0, c->tail>>>(S.d_chunk_bits, S.d_chunk_off, S.d_frame_bits, g.nchunks, nsegs,
                                                          S.d_work, S.d_status, S.d_done, ndone);
  else
    k_scan_bits<<<m, 1024, 0, c->tail>>>(S.d_chunk_bits, S.d_chunk_off, S.d_frame_bits, g.nchunks,
                                           S.d_work, S.d_status, S.d_done, ndone);
  tmark(c, S, MJG_K_SCAN_BITS, 1);
  HIP_TRY(hipGetLastError());
  tmark(c, S, MJG_K_COUNT_FF, 0);
  const int gps = tail_gps(g.nchunks);
  k_count_ff<<<tail_group_wgs(gps * nsegs), 256, 0, c->tail>>>(S.d_scratch, S.d_chunk_bits, S.d_chunk_off,
                                                           S.d_frame_bits, S.d_group_ff, g.nchunks, gps,
                                                           gps * nsegs, S.d_stream);
  tmark(c, S, MJG_K_COUNT_FF, 1);
  HIP_TRY(hipGetLastError());
  // segment and frame sizes, the frames' packed offsets
  tmark(c, S, MJG_K_SCAN_FF, 0);
  k_scan_ff<<<m, 256, 0, c->tail>>>(S.d_group_ff, S.d_ff_off, S.d_frame_bits, g.nchunks, gps, g.nseg, (int)c->hdr.size(),
                                      c->optimal ? S.d_dht_nval : nullptr, S.d_hdr_lens, S.d_seg_size,
                                      S.d_seg_off, S.d_frame_size, S.d_frame_offsets, S.d_done);
  tmark(c, S, MJG_K_SCAN_FF, 1);
  HIP_TRY(hipGetLastError());
  int rc = launch_write(c, S, m, false);
  if (rc) return rc;
  S.n = m;
  S.nin = n;
  S.pending = true;
  S.njobs = 1;  // the caller records a merged launch's jobs
  S.nsynced = 0;
  S.jf0[0] = 0;
  S.jn[0] = m;
  c->head = (c->head + 1) % kSlots;
  c->nout++;
  c->launches++;
  c->synced_since_submit = false;
  return MJG_OK;
}

// Jobs submitted and not yet synced: those of the queued launches plus the held ones.
int pending_jobs(const mjg_ctx *c) {
  int p = c->held;
  for (int i = 0; i < c->nout; i++) {
    const Slot &S = c->slot[(c->head + kSlots - c->nout + i) % kSlots];
    p += S.njobs - S.nsynced;
  }
  return p;
}

// One launch for the held device jobs: their frames as a segment list (one job: the plain
// single-segment launch), each job's frames recorded for mjg_sync.
int launch_held(mjg_ctx *c) {
  SegList sl;
  int n = 0;
  for (int k = 0; k < kMaxSegs; k++) {
    sl.p[k] = c->held_p[k < c->held ? k : 0];
    sl.f0[k] = k < c->held ? n : INT_MAX;
    if (k < c->held) n += c->held_n[k];
  }
  Slot &S = c->slot[c->head];
  const int rc = submit_impl(c, c->held_p[0], n, 1, c->held > 1 ? &sl : nullptr);
  if (rc) return rc;  // the jobs stay held
  S.njobs = c->held;
  for (int k = 0, f = 0; k < c->held; f += c->held_n[k], k++) {
    S.jf0[k] = f;
    S.jn[k] = c->held_n[k];
  }
  c->held = 0;
  return MJG_OK;
}

// Launch the held jobs when a launch slot is free and they are `merge` jobs (with hold_idle off,
// also when the GPU has nothing else queued); a lone held job launches at its own mjg_sync (or
// before a host submit).  Holding even on an idle GPU keeps every launch of a stream of device
// submits a full pair: A/B with prewarmed clocks (profiles/r05/merge_prewarm_ab.txt) c5 +6%, c1 +3.5%,
// c4 +1.5%, c2 +0-1% against no merging; launching a lone job on an idle GPU made the first
// launch a single and lost that gain on c2.  At mjg_sync the slot of the job just synced stays
// untouched: its results are read (mjg_fetch, mjg_output_device) until the caller's next submit.
int try_launch_held(mjg_ctx *c, bool at_sync) {
  if (!c->held || c->nout == kSlots) return MJG_OK;
  if (c->held < c->merge && (c->nout > 0 || c->hold_idle)) return MJG_OK;
  if (at_sync && c->head == c->last) return MJG_OK;
  return launch_held(c);
}

// The readers of the last synced job (fetch, debug_coefs): with no mjg_sync since the last
// mjg_submit they sync the oldest queued job first (the submit -> fetch pattern)
int sync_for_read(mjg_ctx *c) {
  if (pending_jobs(c) > 0 && !c->synced_since_submit)
    if (const int rc = mjg_sync(c, nullptr, nullptr)) return rc;
  return c->last < 0 ? set_err(MJG_E_STATE, "nothing submitted") : MJG_OK;
}

// The frame readbacks (mjg_debug_planes and its kin): frame `frame` of the latest synced submit, out of
// the buffer `buf` names in that submit's slot, whose frames are nbytes apart.  Pending submits are
// synced first.  input: the buffer holds the submit's input frames, which under a sheet are not the
// frames it encoded (a sheet context's launch is one job)
int read_frame(mjg_ctx *c, int frame, uint8_t *out, size_t cap, size_t nbytes,
               uint8_t *(*buf)(const mjg_ctx *, const Slot &), bool input = true) {
  if (pending_jobs(c) > 0) {
    const int rc = mjg_sync(c, nullptr, nullptr);
    if (rc) return rc;
  }
  if (pending_jobs(c) > 0 || c->last < 0) return set_err(MJG_E_STATE, "sync every queued submit first");
  const Slot &L = c->slot[c->last];
  if (frame < 0 || frame >= (input && c->sheet ? L.nin : L.jn[c->last_job])) return set_err(MJG_E_INVALID, "frame %d", frame);
  if (cap < nbytes) return set_err(MJG_E_CAPACITY, "need %zu bytes", nbytes);
  const size_t f = (size_t)L.jf0[c->last_job] + (size_t)frame;
  HIP_TRY(hipMemcpy(out, buf(c, L) + f * nbytes, nbytes, hipMemcpyDeviceToHost));
  return MJG_OK;
}
}  // namespace

int mjg_submit(mjg_ctx *c, const uint8_t *frames, int n, int src_is_device) {
  if (!c || !frames) return set_err(MJG_E_INVALID, "null argument");
  if (n < 1 || n > c->cfg.max_batch)
    return set_err(MJG_E_INVALID, "nframes %d not in 1..%d", n, c->cfg.max_batch);
  if (src_is_device && c->merge > 1) {  // held, and launched with the next one(s)
    // a full held group whose launch waited at mjg_sync (its slot was the one just synced, whose
    // results stay readable until this call): launched now, before the new job is held
    if (c->held == c->merge && c->nout < kSlots) {
      const int rc = launch_held(c);
      if (rc) return rc;
    }
    if (pending_jobs(c) >= kSlots * c->merge || c->held == c->merge)
      return set_err(MJG_E_STATE, "%d submits queued: sync one first", pending_jobs(c));
    c->held_p[c->held] = frames;
    c->held_n[c->held] = n;
    c->held++;
    c->synced_since_submit = false;
    const int rc = try_launch_held(c, false);
    if (rc) c->held--;
    return rc;
  }
  // host frames (H2D through the slot's staging) or merging off: a launch of its own, after
  // a launch of the jobs held before it
  if (c->nout + (c->held ? 1 : 0) >= kSlots)
    return set_err(MJG_E_STATE, "%d launches queued: sync one first", kSlots);
  if (c->held) {
    const int rc = launch_held(c);
    if (rc) return rc;
  }
  return submit_impl(c, frames, n, src_is_device, nullptr);
}

namespace {
// A piece of a longer sequence (a halo, a continued state, or both) on a context that holds nothing (a
// deinterlacer or a denoiser: merge is 1): the checks mjg_submit_halo and mjg_submit_cont share, and the launch
int submit_piece(mjg_ctx *c, const uint8_t *frames, int n, int src_is_device, int halo, int cont) {
  if (halo && !c->deint) return set_err(MJG_E_INVALID, "halo %d on a context without a deinterlacer (deint 0)", halo);
  if (halo & ~3) return set_err(MJG_E_INVALID, "halo %d: not 0..3 (1: a frame in front, 2: a frame behind)", halo);
  if (n < 1 || n > c->cfg.max_batch)
    return set_err(MJG_E_INVALID, "nframes %d not in 1..%d", n, c->cfg.max_batch);
  if (c->nout >= kSlots) return set_err(MJG_E_STATE, "%d launches queued: sync one first", kSlots);
  return submit_impl(c, frames, n, src_is_device, nullptr, halo, cont);
}
}  // namespace

int mjg_submit_halo(mjg_ctx *c, const uint8_t *frames, int n, int src_is_device, int halo) {
  if (!halo) return mjg_submit(c, frames, n, src_is_device);
  if (!c || !frames) return set_err(MJG_E_INVALID, "null argument");
  return submit_piece(c, frames, n, src_is_device, halo, 0);
}

int mjg_submit_cont(mjg_ctx *c, const uint8_t *frames, int n, int src_is_device, int halo, int cont) {
  if (!cont) return mjg_submit_halo(c, frames, n, src_is_device, halo);
  if (!c || !frames) return set_err(MJG_E_INVALID, "null argument");
  if (!c->dn) return set_err(MJG_E_INVALID, "cont %d on a context without a denoiser", cont);
  if (!c->dn_started) return set_err(MJG_E_INVALID, "cont %d before any submit: there is no sequence to continue", cont);
  return submit_piece(c, frames, n, src_is_device, halo, 1);
}

int mjg_max_segments(void) { return kMaxSegs; }

int mjg_submit_segments(mjg_ctx *c, const uint8_t *const *seg_frames, const int *seg_nframes, int nsegs) {
  if (!c || !seg_frames || !seg_nframes) return set_err(MJG_E_INVALID, "null argument");
  if (nsegs < 1 || nsegs > kMaxSegs) return set_err(MJG_E_INVALID, "nsegs %d not in 1..%d", nsegs, kMaxSegs);
  SegList sl;
  int n = 0;
  for (int k = 0; k < kMaxSegs; k++) {
    if (k < nsegs) {
      if (!seg_frames[k] || seg_nframes[k] < 1 || seg_nframes[k] > c->cfg.max_batch)
        return set_err(MJG_E_INVALID, "segment %d: null frames or nframes not in 1..%d", k, c->cfg.max_batch);
      sl.p[k] = seg_frames[k];
      sl.f0[k] = n;
      n += seg_nframes[k];
    } else {
      sl.p[k] = seg_frames[0];
      sl.f0[k] = INT_MAX;
    }
  }
  if (n > c->cfg.max_batch) return set_err(MJG_E_INVALID, "%d frames in the segments, max_batch %d", n, c->cfg.max_batch);
  if (c->nout + (c->held ? 1 : 0) >= kSlots)
    return set_err(MJG_E_STATE, "%d launches queued: sync one first", kSlots);
  if (c->held) {
    const int rc = launch_held(c);
    if (rc) return rc;
  }
  return submit_impl(c, seg_frames[0], n, 1, &sl);
}

int mjg_ctx_queue_depth(const mjg_ctx *c) { return c ? kSlots * c->merge : 0; }

// Completes the oldest queued job (or, with none queued, reports the last synced one).  The
// first job of a launch waits for it (and regrows its output on overflow); the others of the
// same launch are then ready.
int mjg_sync(mjg_ctx *c, uint64_t *frame_sizes, uint64_t *total) {
  if (!c) return set_err(MJG_E_INVALID, "null ctx");
  if (c->nout == 0 && c->held == 0 && c->last < 0) return set_err(MJG_E_STATE, "nothing submitted");
  HIP_TRY(hipSetDevice(c->device));
  if (c->nout == 0 && c->held) {  // the oldest job is held: launch it now
    const int rc = launch_held(c);
    if (rc) return rc;
  }
  if (c->nout > 0) {
    const int si = (c->head + kSlots - c->nout) % kSlots;  // oldest queued launch
    Slot &S = c->slot[si];
    if (S.nsynced == 0) {
      HIP_TRY(hipEventSynchronize(S.done));
      const int n = S.n;
      uint64_t t = 0;
      for (int i = 0; i < n; i++) t += S.h_sizes[i];
      if (*S.h_status & 1u) {  // packed output overflowed: grow, re-run the write pass only
        HIP_TRY(hipFree(S.d_out));
        S.d_out = nullptr;
        S.out_cap = t + t / 4 + 4096;
        int rc = dmalloc(&S.d_out, S.out_cap);
        if (rc) return rc;
        if ((rc = launch_write(c, S, n, true))) return rc;
        HIP_TRY(hipEventSynchronize(S.done));
        if (*S.h_status & 1u) return set_err(MJG_E_HIP, "output overflow persisted");
      }
      if (c->timing) {
        for (int k = 0; k < MJG_NUM_KERNELS; k++) {
          if (k == MJG_K_SCALE && !c->scale && !c->orient && !c->deint && !c->dn && !c->has_lut[0] && !c->has_cmat) continue;
          if (k == MJG_K_HUFF && !c->optimal) continue;
          const bool tail = is_tail_kernel(k);
          if (tail != c->timing_detail && (tail || k == MJG_K_TAIL)) continue;
          if (k == MJG_K_TAIL && !c->timing_tail) continue;
          float ms = 0.f;
          if (hipEventElapsedTime(&ms, S.ev[k][0], S.ev[k][1]) == hipSuccess) c->t_acc[k] += ms;
        }
        c->t_n++;
      }
    }
    const int j = S.nsynced;
    uint64_t off = 0, t = 0;
    for (int i = 0; i < S.jf0[j]; i++) off += S.h_sizes[i];
    for (int i = S.jf0[j]; i < S.jf0[j] + S.jn[j]; i++) t += S.h_sizes[i];
    if (++S.nsynced == S.njobs) {
      S.pending = false;
      c->nout--;
    }
    c->last = si;
    c->last_job = j;
    c->last_off = off;
    c->last_total = t;
    (void)try_launch_held(c, true);  // a failed launch leaves the jobs held: their own sync reports it
  }
  c->synced_since_submit = true;
  const Slot &L = c->slot[c->last];
  if (frame_sizes) memcpy(frame_sizes, L.h_sizes + L.jf0[c->last_job], L.jn[c->last_job] * sizeof(uint64_t));
  if (total) *total = c->last_total;
  return MJG_OK;
}

// The packed JPEGs of the last synced submit, copied D2H into the context's page-locked
// buffer (grown as needed); with no mjg_sync since the last mjg_submit it syncs the oldest
// queued submit first (the submit -> fetch pattern).  A DMA into page-locked memory: a copy
// into pageable memory goes through the runtime's staging and page pinning, which measured
// 0.1 s per 1080p segment in some worker processes and 2 ms in others.
int mjg_fetch_host(mjg_ctx *c, const uint8_t **data, size_t *len) {
  if (!c || !data) return set_err(MJG_E_INVALID, "null argument");
  if (const int rc = sync_for_read(c)) return rc;
  const Slot &L = c->slot[c->last];
  const uint64_t total = c->last_total;
  HIP_TRY(hipSetDevice(c->device));
  if (total > c->h_fetch_cap) {
    if (c->h_fetch) HIP_TRY(hipHostFree(c->h_fetch));
    c->h_fetch = nullptr;
    c->h_fetch_cap = 0;
    const size_t cap = total + total / 4 + 4096;
    if (const int rc = mjg_host_alloc(cap, (void **)&c->h_fetch)) return rc;
    c->h_fetch_cap = cap;
  }
  if (total) HIP_TRY(hipMemcpy(c->h_fetch, L.d_out + c->last_off, total, hipMemcpyDeviceToHost));
  *data = c->h_fetch;
  if (len) *len = total;
  return MJG_OK;
}

// The last synced job's packed JPEGs into the caller's memory: one DMA when it is page-locked
// (mjg_host_alloc), else mjg_fetch_host and a copy.
int mjg_fetch(mjg_ctx *c, uint8_t *out, size_t cap) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (const int rc = sync_for_read(c)) return rc;
  if (cap < c->last_total) return set_err(MJG_E_CAPACITY, "fetch needs %llu bytes", (unsigned long long)c->last_total);
  HIP_TRY(hipSetDevice(c->device));
  // page-locked caller memory (mjg_host_alloc): one DMA straight into it, no staging copy
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, out) == hipSuccess && at.type == hipMemoryTypeHost) {
    if (c->last_total)
      HIP_TRY(hipMemcpy(out, c->slot[c->last].d_out + c->last_off, c->last_total, hipMemcpyDeviceToHost));
    return MJG_OK;
  }
  (void)hipGetLastError();  // pageable memory: not a HIP pointer
  const uint8_t *p = nullptr;
  size_t n = 0;
  const int rc = mjg_fetch_host(c, &p, &n);
  if (rc) return rc;
  if (n) memcpy(out, p, n);
  return MJG_OK;
}

// The launch's packed output and the job's frame offsets into it (data + offsets[i] is the
// job's frame i; with merged launches offsets[0] is the job's place in the launch's output).
int mjg_output_device(mjg_ctx *c, const uint8_t **data, const uint64_t **offsets) {
  if (!c) return set_err(MJG_E_INVALID, "null ctx");
  const Slot &L = c->slot[c->last < 0 ? 0 : c->last];
  if (data) *data = L.d_out;
  if (offsets) *offsets = L.d_frame_offsets + (c->last < 0 ? 0 : L.jf0[c->last_job]);
  return MJG_OK;
}

void *mjg_stream(mjg_ctx *c) {
  if (!c) return nullptr;
  return (void *)slot_stream(c, c->head);
}

int mjg_queue_depth(void) { return kSlots; }

int mjg_host_alloc(size_t bytes, void **ptr) {
  if (!ptr) return set_err(MJG_E_INVALID, "null argument");
  if (hipHostMalloc(ptr, bytes, hipHostMallocDefault) != hipSuccess) {
    *ptr = nullptr;
    (void)hipGetLastError();
    return set_err(MJG_E_NOMEM, "hipHostMalloc(%zu) failed", bytes);
  }
  return MJG_OK;
}

int mjg_host_free(void *ptr) {
  if (ptr) HIP_TRY(hipHostFree(ptr));
  return MJG_OK;
}

// The histogram object (mjgpu.h): k_frame_hist on a stream and buffers of its own, no mjg_ctx
struct mjg_hist {
  int device = 0, max_frames = 0;
  size_t frame_bytes = 0;
  HistGeom g{};
  hipStream_t stream = nullptr;
  uint8_t *d_frames = nullptr;  // max_frames frames, for host input
  uint32_t *d_hist = nullptr;   // [max_frames][768]
  uint32_t *h_hist = nullptr;   // the same, page-locked
};

namespace {
// The object's launch for w x h frames of one format and calls of up to max_frames (no HIP call: the
// host check walks it, tools/stage_host.hip); a call of n frames launches g.gpf * n workgroups
int hist_plan(int w, int h, int cf, int max_frames, HistGeom *g, size_t *frame_bytes) {
  if (w < 1 || h < 1 || w > 16384 || h > 16384) return set_err(MJG_E_INVALID, "hist: %dx%d not in 1..16384", w, h);
  if (cf != MJG_CHROMA_420 && cf != MJG_CHROMA_422 && cf != MJG_CHROMA_444)
    return set_err(MJG_E_INVALID, "hist: chroma_format %d is no MJG_CHROMA_* value", cf);
  if (max_frames < 1) return set_err(MJG_E_INVALID, "hist: max_frames %d below 1", max_frames);
  const int hs = cf != MJG_CHROMA_444, vs = cf == MJG_CHROMA_420;
  *g = HistGeom{};
  g->nb[0] = w * h;
  g->nb[1] = ((w + hs) >> hs) * ((h + vs) >> vs);
  g->fstride = (long long)g->nb[0] + 2 * (long long)g->nb[1];
  g->gy = hist_wgs(g->nb[0]), g->gc = hist_wgs(g->nb[1]);
  g->gpf = g->gy + 2 * g->gc;
  g->gpf_magic = magic32((uint32_t)g->gpf);
  // k_frame_hist's grid is workgroups per frame x frames in x alone (and deint_div forms q d <= t + d)
  if ((long long)g->gpf * ((long long)max_frames + 1) > (long long)INT_MAX)
    return set_err(MJG_E_INVALID, "hist: %d workgroups a frame x %d frames a call is past 2^31 - 1", g->gpf, max_frames);
  *frame_bytes = (size_t)g->fstride;
  return MJG_OK;
}

void free_hist(mjg_hist *h) {
  if (!h) return;
  if (h->stream) {  // (without one nothing was allocated, and the device may be none)
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->d_frames) (void)hipFree(h->d_frames);
    if (h->d_hist) (void)hipFree(h->d_hist);
    if (h->h_hist) (void)hipHostFree(h->h_hist);
    (void)hipStreamDestroy(h->stream);
  }
  delete h;
}

int open_hist(mjg_hist *h) {
  int ndev = 0, rc;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (h->device < 0 || h->device >= ndev) return set_err(MJG_E_INVALID, "hist: device %d of %d", h->device, ndev);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  if ((rc = dmalloc(&h->d_frames, (size_t)h->max_frames * h->frame_bytes)) || (rc = dmalloc(&h->d_hist, (size_t)h->max_frames * 768)))
    return rc;
  if (hipHostMalloc((void **)&h->h_hist, (size_t)h->max_frames * 768 * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
    h->h_hist = nullptr;
    (void)hipGetLastError();
    return set_err(MJG_E_NOMEM, "hist: hipHostMalloc(%zu) failed", (size_t)h->max_frames * 768 * sizeof(uint32_t));
  }
  return MJG_OK;
}
}  // namespace

int mjg_hist_open(int device, int w, int h, int chroma_format, int max_frames, mjg_hist **out) {
  if (!out) return set_err(MJG_E_INVALID, "hist: null argument");
  *out = nullptr;
  mjg_hist *o = new mjg_hist();
  o->device = device, o->max_frames = max_frames;
  int rc = hist_plan(w, h, chroma_format, max_frames, &o->g, &o->frame_bytes);
  if (rc) {
    delete o;  // (no HIP call was made)
    return rc;
  }
  if ((rc = open_hist(o))) {
    free_hist(o);
    return rc;
  }
  *out = o;
  return MJG_OK;
}

int mjg_hist_frames(mjg_hist *h, const uint8_t *frames, int n, int src_is_device, uint32_t *hist) {
  if (!h || !frames || !hist) return set_err(MJG_E_INVALID, "hist: null argument");
  if (n < 1 || n > h->max_frames) return set_err(MJG_E_INVALID, "hist: nframes %d not in 1..%d", n, h->max_frames);
  HIP_TRY(hipSetDevice(h->device));
  const size_t words = (size_t)n * 768;
  if (!src_is_device)
    HIP_TRY(hipMemcpyAsync(h->d_frames, frames, (size_t)n * h->frame_bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemsetAsync(h->d_hist, 0, words * sizeof(uint32_t), h->stream));  // the kernel adds: every call from zero
  (void)hipGetLastError();  // (an earlier call's error is not this launch's)
  k_frame_hist<<<h->g.gpf * n, kHistThreads, 0, h->stream>>>(one_seg(src_is_device ? frames : h->d_frames), h->d_hist, h->g);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->h_hist, h->d_hist, words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  memcpy(hist, h->h_hist, words * sizeof(uint32_t));
  return MJG_OK;
}

void mjg_hist_close(mjg_hist *h) { free_hist(h); }

int mjg_kernel_times(mjg_ctx *c, double *ms, int *launches, int reset) {
  if (!c) return set_err(MJG_E_INVALID, "null ctx");
  if (!c->timing) return set_err(MJG_E_STATE, "context opened without MJG_F_TIMING");
  for (int k = 0; k < MJG_NUM_KERNELS; k++)
    if (ms) ms[k] = c->t_n ? c->t_acc[k] / c->t_n : 0.0;
  if (launches) *launches = c->t_n;
  if (reset) {
    for (double &t : c->t_acc) t = 0;
    c->t_n = 0;
  }
  return MJG_OK;
}

int mjg_build_header(const mjg_config *cfg, uint8_t *out, size_t cap, size_t *len) {
  if (!cfg) return set_err(MJG_E_INVALID, "null cfg");
  if (cfg->dst_w < 1 || cfg->dst_h < 1 || cfg->dst_w > 65535 || cfg->dst_h > 65535 ||
      cfg->qscale < 1 || cfg->qscale > 31 || cfg->chroma_format < MJG_CHROMA_420 ||
      cfg->chroma_format > MJG_CHROMA_444)
    return set_err(MJG_E_INVALID, "bad size / qscale / chroma_format");
  if (cfg->sar_num < 0 || cfg->sar_den < 0 || cfg->sar_num > 65535 || cfg->sar_den > 65535)
    return set_err(MJG_E_INVALID, "bad SAR %d:%d", cfg->sar_num, cfg->sar_den);
  uint8_t mp[64];
  quant_matrix(cfg->qscale, mp, nullptr);
  const bool rst = (cfg->flags & MJG_F_RST) && (cfg->dst_h + 15) / 16 > 1;
  const std::vector<uint8_t> h = build_header(cfg->dst_w, cfg->dst_h, mp, cfg->sar_num, cfg->sar_den,
                                             (cfg->flags & MJG_F_COM_ITU601) != 0, cfg->chroma_format, rst);
  if (len) *len = h.size();
  if (!out) return MJG_OK;
  if (cap < h.size()) return set_err(MJG_E_CAPACITY, "header needs %zu bytes", h.size());
  memcpy(out, h.data(), h.size());
  return MJG_OK;
}

int mjg_sws_filter(int src_len, int dst_len, int one, int align, int bitexact, int src_pos,
                   int dst_pos, int16_t *coeff, size_t coeff_cap, int32_t *pos_out, int *taps) {
  SwsFilter f;
  if (!make_sws_filter(src_len, dst_len, one, align, bitexact != 0, src_pos, dst_pos, &f))
    return set_err(MJG_E_INVALID, "unsupported filter %d -> %d", src_len, dst_len);
  if (taps) *taps = f.taps;
  if (!coeff) return MJG_OK;
  if (coeff_cap < f.coeff.size()) return set_err(MJG_E_CAPACITY, "need %zu taps", f.coeff.size());
  memcpy(coeff, f.coeff.data(), f.coeff.size() * sizeof(int16_t));
  if (pos_out) memcpy(pos_out, f.pos.data(), f.pos.size() * sizeof(int32_t));
  return MJG_OK;
}

int mjg_debug_coefs(mjg_ctx *c, int frame, int16_t *out, size_t nblocks) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (!c->geom.debug_coefs) return set_err(MJG_E_STATE, "context opened without MJG_F_DEBUG_COEFS");
  if (const int rc = sync_for_read(c)) return rc;
  const Slot &L = c->slot[c->last];
  const size_t nb = (size_t)c->geom.nmcu * c->geom.bpm;  // dbg buffer: frame-major, coding order
  if (frame < 0 || frame >= L.jn[c->last_job]) return set_err(MJG_E_INVALID, "frame %d", frame);
  if (nblocks < nb) return set_err(MJG_E_CAPACITY, "need %zu blocks", nb);
  // the kernel stores each quantised block in natural (raster) order
  const size_t f = (size_t)L.jf0[c->last_job] + (size_t)frame;
  HIP_TRY(hipMemcpy(out, L.d_dbg + f * nb * 64, nb * 64 * sizeof(int16_t), hipMemcpyDeviceToHost));
  return MJG_OK;
}

int mjg_debug_scale_path(mjg_ctx *c, int plane) {
  if (!c) return set_err(MJG_E_INVALID, "null context");
  if (plane < 0 || plane > 1) return set_err(MJG_E_INVALID, "plane must be 0 (luma) or 1 (chroma)");
  if (!c->scale) return 0;
  const PlaneScale &p = c->ps[plane];
  return p.copy ? (c->has_pad ? 4 : 1) : p.stream ? 3 : 2;
}

int mjg_debug_encode_path(mjg_ctx *c) {
  if (!c) return set_err(MJG_E_INVALID, "null context");
  return (c->scale ? 0 : 1) | (c->enc_ua ? 2 : 0);
}

int mjg_debug_planes(mjg_ctx *c, int frame, uint8_t *out, size_t cap) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (!c->scale) return set_err(MJG_E_STATE, "context has no sws stage (same size, same chroma format)");
  // the encoder's input: under a sharpen its output, under a sheet the sheets
  return read_frame(c, frame, out, cap, c->enc_frame_bytes,
                    [](const mjg_ctx *x, const Slot &S) { return x->sheet ? S.d_tile : x->sharp ? S.d_sharp : S.d_scaled; }, false);
}

int mjg_debug_cell(mjg_ctx *c, int frame, uint8_t *out, size_t cap) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (!c->sheet) return set_err(MJG_E_STATE, "context has no sheet (mjg_open_chain, or a trivial sheet)");
  return read_frame(c, frame, out, cap, c->pic_frame_bytes,
                    [](const mjg_ctx *x, const Slot &S) { return x->sharp ? S.d_sharp : S.d_scaled; });
}

int mjg_debug_sheet(mjg_ctx *c, mjg_sheet *out) {
  if (!c) return set_err(MJG_E_INVALID, "null context");
  if (c->sheet && out) *out = c->sh;
  return c->sheet ? 1 : 0;
}

int mjg_frames_out(const mjg_ctx *c, int nframes) {
  if (!c || nframes < 1) return 0;
  return c->sheet ? (nframes + c->sh.nb_frames - 1) / c->sh.nb_frames : nframes;
}

int mjg_debug_presharp(mjg_ctx *c, int frame, uint8_t *out, size_t cap) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (!c->sharp) return set_err(MJG_E_STATE, "context has no sharpen (no unsharp, or both amounts 0)");
  return read_frame(c, frame, out, cap, c->pic_frame_bytes, [](const mjg_ctx *, const Slot &S) { return S.d_scaled; });
}

int mjg_debug_unsharp(mjg_ctx *c, mjg_unsharp *out) {
  if (!c) return set_err(MJG_E_INVALID, "null context");
  if (c->sharp && out) *out = c->us;
  return c->sharp ? 1 : 0;
}

int mjg_debug_lut(mjg_ctx *c, int slot, mjg_lut *out) {
  if (!c) return set_err(MJG_E_INVALID, "null context");
  if (slot < 0 || slot > 1) return set_err(MJG_E_INVALID, "slot %d: not 0 (in) or 1 (out)", slot);
  if (c->has_lut[slot] && out) *out = c->lut[slot];
  return c->has_lut[slot] ? 1 : 0;
}

int mjg_debug_lut_in(mjg_ctx *c, int frame, uint8_t *out, size_t cap) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (!c->has_lut[0]) return set_err(MJG_E_STATE, "context has no table in front of the sws stage (none, or identity tables)");
  // (in place in the buffer of the stage in front of it, else d_lut)
  return read_frame(c, frame, out, cap, c->in_frame_bytes, lut_in_buf);
}

int mjg_debug_cmat(mjg_ctx *c, mjg_cmatrix *out) {
  if (!c) return set_err(MJG_E_INVALID, "null context");
  if (c->has_cmat && out) *out = c->cmat;
  return c->has_cmat ? 1 : 0;
}

int mjg_debug_cmat_out(mjg_ctx *c, int frame, uint8_t *out, size_t cap) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (!c->has_cmat) return set_err(MJG_E_STATE, "context has no colour matrix (none, or the identity)");
  // (in place in the buffer of the stage in front of it, else d_lut; a lut_in has mapped it there)
  return read_frame(c, frame, out, cap, c->in_frame_bytes, lut_in_buf);
}

int mjg_debug_oriented(mjg_ctx *c, int frame, uint8_t *out, size_t cap) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (!c->orient) return set_err(MJG_E_STATE, "context has no orientation (orient 0)");
  return read_frame(c, frame, out, cap, c->in_frame_bytes, [](const mjg_ctx *, const Slot &S) { return S.d_orient; });
}

int mjg_debug_orient(mjg_ctx *c) {
  if (!c) return set_err(MJG_E_INVALID, "null context");
  return c->orient;
}

int mjg_debug_deint(mjg_ctx *c, int frame, uint8_t *out, size_t cap) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (!c->deint) return set_err(MJG_E_STATE, "context has no deinterlacer (deint 0)");
  return read_frame(c, frame, out, cap, c->in_frame_bytes, [](const mjg_ctx *, const Slot &S) { return S.d_deint; });
}

int mjg_debug_denoise(mjg_ctx *c, int frame, uint8_t *out, size_t cap) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (!c->dn) return set_err(MJG_E_STATE, "context has no denoiser");
  return read_frame(c, frame, out, cap, c->in_frame_bytes, [](const mjg_ctx *, const Slot &S) { return S.d_dn; });
}

int mjg_debug_denoise_state(mjg_ctx *c, uint16_t *out, size_t cap) {
  if (!c || !out) return set_err(MJG_E_INVALID, "null argument");
  if (!c->dn) return set_err(MJG_E_STATE, "context has no denoiser");
  if (cap < c->in_frame_bytes) return set_err(MJG_E_CAPACITY, "need %zu uint16", c->in_frame_bytes);
  while (pending_jobs(c) > 0)
    if (const int rc = mjg_sync(c, nullptr, nullptr)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  for (int i = 0; i < kSlots; i++)  // (a synced submit's time scan is long done; the streams are idle)
    if (c->slot[i].alloc) HIP_TRY(hipStreamSynchronize(c->slot[i].st));
  HIP_TRY(hipMemcpy(out, c->d_dn_state, c->in_frame_bytes * sizeof(uint16_t), hipMemcpyDeviceToHost));
  return MJG_OK;
}

int mjg_debug_deint_flags(mjg_ctx *c) {
  if (!c) return set_err(MJG_E_INVALID, "null context");
  return c->deint;
}

int mjg_debug_huff_build(int device, const uint32_t *hist, int nframes, uint8_t *dht, uint32_t *nval) {
  if (!hist || !dht || !nval || nframes < 1 || nframes > 4096) return set_err(MJG_E_INVALID, "bad arguments");
  HIP_TRY(hipSetDevice(device));
  const size_t nh = (size_t)nframes * kFrameTabWords, nd = (size_t)nframes * 4 * kDhtSlot, nv = (size_t)nframes * 4;
  uint32_t *d_hist = nullptr, *d_ftabs = nullptr, *d_nval = nullptr;
  uint8_t *d_dht = nullptr;
  int rc = MJG_OK;
  if (hipMalloc((void **)&d_hist, nh * 4) != hipSuccess || hipMalloc((void **)&d_ftabs, nh * 4) != hipSuccess ||
      hipMalloc((void **)&d_dht, nd) != hipSuccess || hipMalloc((void **)&d_nval, nv * 4) != hipSuccess) {
    (void)hipGetLastError();
    rc = set_err(MJG_E_NOMEM, "hipMalloc failed");
  }
  if (rc == MJG_OK && (hipMemcpy(d_hist, hist, nh * 4, hipMemcpyHostToDevice) != hipSuccess ||
                       hipMemset(d_dht, 0, nd) != hipSuccess)) rc = set_err(MJG_E_HIP, "copy in failed");
  if (rc == MJG_OK) {
    k_huff_build<<<nframes * 4, 64>>>(d_hist, d_ftabs, d_dht, d_nval);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(dht, d_dht, nd, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(nval, d_nval, nv * 4, hipMemcpyDeviceToHost) != hipSuccess)
      rc = set_err(MJG_E_HIP, "k_huff_build failed");
  }
  (void)hipFree(d_hist);
  (void)hipFree(d_ftabs);
  (void)hipFree(d_dht);
  (void)hipFree(d_nval);
  return rc;
}

int mjg_debug_tail(int device, const mjg_tail_job *job, uint8_t *out, uint64_t *frame_offsets, uint32_t *group_ff,
                   uint32_t *status) {
  // every check before any HIP call: a host without a GPU answers them
  if (!job || !out || !frame_offsets || !status) return set_err(MJG_E_INVALID, "null argument");
  const mjg_tail_job &j = *job;
  if (!j.chunk_bits || !j.words || !j.hdr) return set_err(MJG_E_INVALID, "null chunk_bits, words or hdr");
  if (j.nframes < 1 || j.nseg < 1 || j.nchunks < 1 || j.hdr_len < 1 || j.hdr_len > 65536)
    return set_err(MJG_E_INVALID, "nframes %d, nseg %d, nchunks %d or hdr_len %d: below 1 (hdr_len: or above 65536)",
                   j.nframes, j.nseg, j.nchunks, j.hdr_len);
  const uint64_t nslots64 = (uint64_t)j.nframes * (uint64_t)j.nseg * (uint64_t)j.nchunks;
  if (nslots64 > MJG_TAIL_MAX_SLOTS)
    return set_err(MJG_E_INVALID, "%d frames x %d segments x %d chunks: more than %d slots", j.nframes, j.nseg,
                   j.nchunks, MJG_TAIL_MAX_SLOTS);
  if (j.out_cap > (1ull << 30)) return set_err(MJG_E_INVALID, "out_cap above 2^30");
  const bool optimal = j.nval != nullptr;
  if (optimal) {
    if (!j.dht) return set_err(MJG_E_INVALID, "nval without dht");
    // frame_hdr_len takes the default DHT for 4 + 4 * 17 + 348 bytes
    if (j.dht_pos < 0 || j.dht_end != j.dht_pos + 420 || j.dht_end > j.hdr_len)
      return set_err(MJG_E_INVALID, "dht_pos %d, dht_end %d: not a 420-byte DHT inside the %d header bytes", j.dht_pos,
                     j.dht_end, j.hdr_len);
    for (size_t i = 0; i < (size_t)j.nframes * 4; i++)
      if (j.nval[i] > 256) return set_err(MJG_E_INVALID, "nval[%zu] = %u: above 256", i, j.nval[i]);
  }
  const size_t nslots = (size_t)nslots64, nsegs = (size_t)j.nframes * j.nseg;
  constexpr uint32_t kSlotBits = (uint32_t)kSlotWords * 32u;
  for (size_t i = 0; i < nslots; i++) {
    const uint32_t L = j.chunk_bits[i];
    const bool last = (i + 1) % (size_t)j.nchunks == 0;
    if (L == 0) return set_err(MJG_E_INVALID, "chunk %zu has 0 bits", i);
    if (L < 32 && !last)
      return set_err(MJG_E_INVALID, "chunk %zu has %u bits and is not its segment's last: every other chunk covers "
                     "a word start (32 bits or more)", i, L);
  }
  // the scratch image: every slot word `fill`, then each chunk's words at its slot
  std::vector<uint32_t> image(nslots * (size_t)kSlotWords, j.fill);
  {
    const uint32_t *w = j.words;
    for (size_t i = 0; i < nslots; i++) {
      const size_t nw = (std::min(j.chunk_bits[i], kSlotBits) + 31u) / 32u;
      memcpy(image.data() + i * (size_t)kSlotWords, w, nw * 4);
      w += nw;
    }
  }
  HIP_TRY(hipSetDevice(device));
  const int gps = tail_gps(j.nchunks), ngroups = gps * (int)nsegs;
  const size_t nwork = (size_t)kXcds * kCtrStride, nout = (size_t)j.out_cap + MJG_TAIL_GUARD;
  uint32_t *d_scratch = nullptr, *d_stream = nullptr, *d_bits = nullptr, *d_off = nullptr, *d_gff = nullptr;
  uint32_t *d_ffo = nullptr, *d_segb = nullptr, *d_status = nullptr, *d_done = nullptr, *d_work = nullptr;
  uint32_t *d_segsz = nullptr, *d_segoff = nullptr, *d_hl = nullptr, *d_nval = nullptr;
  uint64_t *d_fsz = nullptr, *d_fo = nullptr;
  uint8_t *d_hdr = nullptr, *d_dht = nullptr, *d_out = nullptr;
  const size_t ndht = (size_t)j.nframes * 4 * kDhtSlot;
  auto run = [&]() -> int {
    int rc;
    if ((rc = dmalloc(&d_scratch, image.size())) || (rc = dmalloc(&d_stream, image.size())) ||
        (rc = dmalloc(&d_bits, nslots)) || (rc = dmalloc(&d_off, nslots)) || (rc = dmalloc(&d_gff, (size_t)ngroups)) ||
        (rc = dmalloc(&d_ffo, (size_t)ngroups)) || (rc = dmalloc(&d_segb, nsegs)) || (rc = dmalloc(&d_status, 1)) ||
        (rc = dmalloc(&d_done, (size_t)kTailDone)) || (rc = dmalloc(&d_work, nwork)) ||
        (rc = dmalloc(&d_fsz, (size_t)j.nframes)) || (rc = dmalloc(&d_fo, (size_t)j.nframes + 1)) ||
        (rc = dmalloc(&d_hdr, (size_t)j.hdr_len)) || (rc = dmalloc(&d_out, nout)))
      return rc;
    if (j.nseg > 1 && ((rc = dmalloc(&d_segsz, nsegs)) || (rc = dmalloc(&d_segoff, nsegs)))) return rc;
    if (optimal && ((rc = dmalloc(&d_hl, (size_t)j.nframes)) || (rc = dmalloc(&d_nval, (size_t)j.nframes * 4)) ||
                    (rc = dmalloc(&d_dht, ndht))))
      return rc;
    HIP_TRY(hipMemcpy(d_scratch, image.data(), image.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_bits, j.chunk_bits, nslots * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_hdr, j.hdr, (size_t)j.hdr_len, hipMemcpyHostToDevice));
    if (optimal) {
      HIP_TRY(hipMemcpy(d_nval, j.nval, (size_t)j.nframes * 16, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(d_dht, j.dht, ndht, hipMemcpyHostToDevice));
    }
    // the counters and the flag non-zero: the scan kernel is what zeroes them.  Offsets and
    // counts that no kernel wrote come back as 0xFF.., the stream's unwritten words as 0x5A..
    HIP_TRY(hipMemset(d_work, 0xFF, nwork * 4));
    HIP_TRY(hipMemset(d_status, 0xFF, 4));
    HIP_TRY(hipMemset(d_done, 0xFF, (size_t)kTailDone * 4));
    HIP_TRY(hipMemset(d_fo, 0xFF, ((size_t)j.nframes + 1) * 8));
    HIP_TRY(hipMemset(d_gff, 0xFF, (size_t)ngroups * 4));
    HIP_TRY(hipMemset(d_stream, 0x5A, image.size() * 4));
    HIP_TRY(hipMemset(d_out, 0xA5, nout));
    if (j.nseg > 1)
      k_scan_bits_seg<<<tail_seg_wgs((int)nsegs), 256>>>(d_bits, d_off, d_segb, j.nchunks, (int)nsegs, d_work, d_status,
                                                         d_done, kTailDone);
    else
      k_scan_bits<<<j.nframes, 1024>>>(d_bits, d_off, d_segb, j.nchunks, d_work, d_status, d_done, kTailDone);
    HIP_TRY(hipGetLastError());
    k_count_ff<<<tail_group_wgs(ngroups), 256>>>(d_scratch, d_bits, d_off, d_segb, d_gff, j.nchunks, gps, ngroups,
                                                 d_stream);
    HIP_TRY(hipGetLastError());
    k_scan_ff<<<j.nframes, 256>>>(d_gff, d_ffo, d_segb, j.nchunks, gps, j.nseg, j.hdr_len, optimal ? d_nval : nullptr,
                                  d_hl, d_segsz, d_segoff, d_fsz, d_fo, d_done);
    HIP_TRY(hipGetLastError());
    k_write<<<tail_group_wgs(ngroups), 256>>>(d_stream, d_bits, d_off, d_segb, d_ffo, j.nchunks, gps, j.nseg, j.nframes,
                                              d_segsz, d_segoff, d_fo, d_hdr, j.hdr_len, optimal ? d_hl : nullptr,
                                              j.dht_pos, j.dht_end, d_dht, optimal ? d_nval : nullptr, d_out, j.out_cap,
                                              d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(frame_offsets, d_fo, ((size_t)j.nframes + 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(status, d_status, 4, hipMemcpyDeviceToHost));
    if (group_ff) HIP_TRY(hipMemcpy(group_ff, d_gff, (size_t)ngroups * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> work(nwork);
    HIP_TRY(hipMemcpy(work.data(), d_work, nwork * 4, hipMemcpyDeviceToHost));
    for (int x = 0; x < kXcds; x++)
      if (work[(size_t)x * kCtrStride]) return set_err(MJG_E_STATE, "the scan left work counter %d at %u", x, work[(size_t)x * kCtrStride]);
    return MJG_OK;
  };
  const int rc = run();
  void *bufs[] = {d_scratch, d_stream, d_bits, d_off, d_gff, d_ffo, d_segb, d_status, d_done, d_work,
                  d_segsz, d_segoff, d_hl, d_nval, d_fsz, d_fo, d_hdr, d_dht, d_out};
  for (void *p : bufs) (void)hipFree(p);
  return rc;
}

int mjg_debug_filter(mjg_ctx *c, int plane, int dir, int16_t *coeff, int32_t *pos, int *taps,
                     int *len) {
  if (!c) return set_err(MJG_E_INVALID, "null ctx");
  if (!c->scale) return set_err(MJG_E_STATE, "context has no sws stage (same size, same chroma format)");
  if (plane < 0 || plane > 1 || dir < 0 || dir > 1) return set_err(MJG_E_INVALID, "plane/dir");
  const SwsFilter &f = dir ? c->ps[plane].vf : c->ps[plane].hf;
  if (taps) *taps = f.taps;
  if (len) *len = f.dst_len;
  if (coeff) memcpy(coeff, f.coeff.data(), f.coeff.size() * sizeof(int16_t));
  if (pos) memcpy(pos, f.pos.data(), f.pos.size() * sizeof(int32_t));
  return MJG_OK;
}

}  // extern "C"

