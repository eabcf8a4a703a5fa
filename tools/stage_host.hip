// The plane stages' kernel bodies (scale.hip's __host__ __device__ *_work functions) on the CPU, over the library's
// own launch plan: a sub-command builds the mjg_config / mjg_chain / mjg_sheet of its arguments, runs api.hip's
// plan_ctx on a `new mjg_ctx()` and walks every (workgroup, thread) of the launches that the per-submit functions
// (deint_launch, lut_launch, sharp_launch, sheet_split / tile_launch; the colour matrix's one launch is the plan's
// cgeom) make of it, in the instantiation the plan chose.  No geometry is filled in here, so a wrong plan or a
// wrong per-submit adjustment is walked as the GPU would run it.  Every buffer is allocated at exactly the size the
// plan's frame bytes give, so that AddressSanitizer sees any access outside a readable frame; a refused
// configuration is exit status 5 with the library's message.  Makes no HIP call.  Built and driven by
// tools/host_check.py for the seven *_host_check.py scripts:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//     -I ffmpeg_distributed_amd/csrc -o stage_host tools/stage_host.hip ffmpeg_distributed_amd/csrc/sws_filter.cpp
// Frames are packed planar with chroma shifts hshift, vshift.  split: 0, or the lengths of up to kMaxSegs segments as
// a,b,... (their sum nframes): each segment in an allocation of its own (mjg_submit_segments' SegList).  apart: 1, U
// and V in a launch each whatever nframes is (the functions' uv1 false); without it they are paired as submit_impl
// pairs them (uv_paired), apart from 32,768 frames on.
//   stage_host yadif IN OUT w h hshift vshift nospatial parity nframes halo split [apart]
//     IN: nframes + halo frames (halo bit 1: one in front, bit 2: one behind; no split then).
//   stage_host lut IN TABS OUT w h hshift vshift nframes split apart inplace [cw ch px py]
//     TABS: the Y, U and V table, 768 bytes.  Without the last four values slot "in": whole planes, into a second
//     buffer or (inplace 1, one segment) where they lie; segments start one byte into their allocations.  With them
//     slot "out": the frames are cw x ch canvases and the w x h picture at (px, py) is mapped in place.
//   stage_host cmat IN OUT w h hshift vshift nframes split inplace yu yv uu uv vu vv
//     segments and inplace as for lut.
//   stage_host tile IN OUT w h hshift vshift cols rows N margin padding segs apart shift
//     IN: the cell frames of all segments in one buffer (the sws stage's output); OUT: each segment's sheets behind
//     those of the one before.  shift: both buffers start this many bytes into their allocations (0..15: the
//     alignment of the sheet planes, which the pieces are cut on).
//   stage_host unsharp IN OUT PW PH hshift vshift PX PY W H lx ly la cx cy ca nframes apart
//     IN: frames of the encoded size PW x PH, the W x H picture at (PX, PY); la / ca: the filter's integers.  Asserts
//     besides that every staged load (a byte, or a dword of four consecutive bytes) lies inside the picture, that
//     every other load is the copy of a sample outside it (or of a plane whose amount is 0) from its own place, and
//     that every byte of every plane of every frame is stored exactly once; LDS arrays at exactly the kernel's sizes.
//   stage_host hist IN OUT w h hshift vshift nframes split lead
//     k_frame_hist over the launch that hist_plan (mjg_hist_open's plan, no mjg_ctx) gives; OUT: nframes x 768
//     uint32 counters; lead: the frames (each segment's) start this many bytes into their allocation (0..15: the
//     alignment of the source, which the pieces are cut on); the LDS histogram at exactly the kernel's size.
//   stage_host hqdn3d IN TABS OUT STATE w h hshift vshift nframes split lead chunks [behind]
//     k_dn_rows, k_dn_cols and k_dn_time over the launches that plan_ctx and dn_launch give, the bodies split at their
//     barriers.  TABS: mjg_denoise, 4 x 8192 int16; OUT: the denoised frames; STATE: the carried state behind the last
//     submit, mjg_frame_bytes uint16.  split: one submit of segments, as above.  chunks: 0, or the lengths a,b,... of
//     consecutive submits of one buffer, the first plain and every later one continued (mjg_submit_cont); no split
//     then.  lead: the frames and the output start this many bytes into their allocations (0..15: the alignment the
//     time scan cuts its pieces on).  behind: 1, the segments of `split` lie in one buffer, as the deinterlacer leaves
//     them, and the kernels get that buffer with the segments' starts (api.hip's seg_starts).  The uint16 buffer, the state and the LDS tiles are at exactly the library's sizes.
#include "api.hip"

#include <cstdio>

namespace {

#define CHECK(c, ...)               \
  do {                              \
    if (!(c)) {                     \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      exit(4);                      \
    }                               \
  } while (0)

std::vector<int> lengths(const char *p) {
  std::vector<int> v;
  while (*p) {
    char *e;
    const int x = (int)strtol(p, &e, 10);
    if (x > 0) v.push_back(x);
    p = *e ? e + 1 : e;
  }
  CHECK((int)v.size() <= kMaxSegs, "more than %d segments", kMaxSegs);
  return v;
}

// A context planned as open_ctx plans it, for sw x sh frames -> dw x dh in one format and submits of up to n frames
mjg_ctx *plan(int sw, int sh, int dw, int dh, int hs, int vs, int n, mjg_chain chain, const mjg_sheet *sheet = nullptr) {
  mjg_config k{};
  k.src_w = sw, k.src_h = sh, k.dst_w = dw, k.dst_h = dh;
  k.in_full_range = 1, k.qscale = 5, k.sar_num = k.sar_den = 1, k.max_batch = n;
  k.chroma_format = chain.src_chroma_format = !hs ? MJG_CHROMA_444 : vs ? MJG_CHROMA_420 : MJG_CHROMA_422;
  mjg_ctx *c = new mjg_ctx();
  Layout lay;
  if (plan_ctx(k, chain, sheet, true, c, &lay)) {
    fprintf(stderr, "refused: %s\n", mjg_last_error());
    exit(5);
  }
  return c;
}

// The frames of a submit on exact-size allocations: one for `total` frames, `lead` bytes in, the submit's first frame
// `skip` frames behind that; or one per segment, each seg_lead bytes in
struct Input {
  std::vector<uint8_t *> bufs;
  SegList sl;
  uint8_t *first;  // the first frame
};
Input load(const char *path, size_t fb, int total, int skip, int lead, const std::vector<int> &lens = {}, int seg_lead = 0) {
  Input in;
  FILE *f = fopen(path, "rb");
  CHECK(f, "cannot read %s", path);
  auto take = [&](size_t frames, int at) {
    uint8_t *b = (uint8_t *)malloc(frames * fb + at);
    CHECK(fread(b + at, 1, frames * fb, f) == frames * fb, "%s: fewer than %zu frames of %zu bytes", path, frames, fb);
    in.bufs.push_back(b);
    return b + at;
  };
  if (lens.empty()) {
    in.sl = one_seg(in.first = take(total, lead) + skip * fb);
  } else {
    int n = 0;
    for (int k = 0; k < kMaxSegs; k++) {  // as mjg_submit_segments fills them
      const bool used = k < (int)lens.size();
      in.sl.p[k] = used ? take(lens[k], seg_lead) : in.sl.p[0];
      in.sl.f0[k] = used ? n : INT_MAX;
      if (used) n += lens[k];
    }
    CHECK(n == total && !skip, "the segments' frames are not nframes");
    in.first = in.bufs[0] + seg_lead;
  }
  fclose(f);
  return in;
}

void save(const char *path, const uint8_t *p, size_t bytes) {
  FILE *f = fopen(path, "wb");
  CHECK(f && fwrite(p, 1, bytes, f) == bytes, "cannot write %s", path);
  fclose(f);
}

int yadif(int argc, char **a) {
  if (argc < 11) return 2;
  const int w = atoi(a[2]), h = atoi(a[3]), n = atoi(a[8]), halo = atoi(a[9]);
  const std::vector<int> lens = lengths(a[10]);
  const bool apart = argc > 11 && atoi(a[11]);
  CHECK(lens.empty() || !halo, "segments with a halo");
  mjg_chain ch{};
  ch.deint = MJG_DEINT_YADIF | (atoi(a[6]) ? MJG_DEINT_NOSPATIAL : 0) | (atoi(a[7]) ? MJG_DEINT_BFF : 0);
  mjg_ctx *c = plan(w, h, w, h, atoi(a[4]), atoi(a[5]), n, ch);
  const size_t fb = c->in_frame_bytes;
  const int hp = halo & 1, hn = (halo >> 1) & 1;
  Input in = load(a[0], fb, n + hp + hn, hp, 0, lens);
  uint8_t *dst = (uint8_t *)malloc(n * fb);
  const bool uv1 = uv_paired(n) && !apart;
  for (int p = 0; p < uv_launches(uv1); p++) {
    const DeintGeom g = deint_launch(c, p, uv1, n, in.sl, halo);
    const bool nospatial = c->dpass[p ? 1 : 0].launch == launch_deint<true>;
    for (int t = 0; t < g.gxy * uv_nz(p, uv1, n); t++)
      for (int tid = 0; tid < kDeintThreads; tid++) {
        if (nospatial) yadif_work<true>(in.sl, dst, g, t, tid);
        else yadif_work<false>(in.sl, dst, g, t, tid);
      }
  }
  save(a[1], dst, n * fb);
  for (uint8_t *b : in.bufs) free(b);
  free(dst);
  delete c;
  return 0;
}

int lut(int argc, char **a) {
  if (argc < 11) return 2;
  const int w = atoi(a[3]), h = atoi(a[4]), n = atoi(a[7]), slot = argc >= 15;
  const std::vector<int> lens = lengths(a[8]);
  const bool apart = atoi(a[9]) != 0, inplace = atoi(a[10]) != 0 || slot;
  CHECK(lens.empty() || !inplace, "segments in place");
  mjg_lut tabs;
  FILE *f = fopen(a[1], "rb");
  CHECK(f && fread(&tabs, 1, sizeof tabs, f) == sizeof tabs, "cannot read %s", a[1]);
  fclose(f);
  mjg_chain ch{};
  (slot ? ch.lut_out : ch.lut_in) = &tabs;
  if (slot) ch.has_pad = 1, ch.pad_w = atoi(a[11]), ch.pad_h = atoi(a[12]), ch.pad_x = atoi(a[13]), ch.pad_y = atoi(a[14]);
  mjg_ctx *c = plan(w, h, w, h, atoi(a[5]), atoi(a[6]), n, ch);
  CHECK(c->has_lut[slot], "three identity tables: no stage");
  const size_t fb = slot ? c->pic_frame_bytes : c->in_frame_bytes;
  Input in = load(a[0], fb, n, 0, 0, lens, 1);
  uint8_t *dst = inplace ? in.first : (uint8_t *)malloc(n * fb);
  const bool uv1 = uv_paired(n) && !apart;
  for (int p = 0; p < uv_launches(uv1); p++) {
    LutGeom g;
    if (!lut_launch(c, slot, p, uv1, n, inplace, &g)) continue;
    for (int t = 0; t < g.gxy * uv_nz(p, uv1, n); t++)
      for (int tid = 0; tid < kCopyThreads; tid++) lut_work(in.sl, dst, g, (const uint8_t *)&c->lut[slot], t, tid);
  }
  save(a[2], dst, n * fb);
  if (!inplace) free(dst);
  for (uint8_t *b : in.bufs) free(b);
  delete c;
  return 0;
}

template <int HS, int VS>
void walk_cmat(const SegList &sl, uint8_t *dst, const CmatGeom &g, const CmatCoef &cm, int n) {
  for (int t = 0; t < g.gxy * n; t++)
    for (int tid = 0; tid < kCmatThreads; tid++) cmat_work<HS, VS>(sl, dst, g, cm, t, tid);
}

int cmat(int argc, char **a) {
  if (argc < 15) return 2;
  const int w = atoi(a[2]), h = atoi(a[3]), n = atoi(a[6]);
  const std::vector<int> lens = lengths(a[7]);
  const bool inplace = atoi(a[8]) != 0;
  CHECK(lens.empty() || !inplace, "segments in place");
  const mjg_cmatrix cm{atoi(a[9]), atoi(a[10]), atoi(a[11]), atoi(a[12]), atoi(a[13]), atoi(a[14])};
  mjg_chain ch{};
  ch.cmat = &cm;
  mjg_ctx *c = plan(w, h, w, h, atoi(a[4]), atoi(a[5]), n, ch);
  CHECK(c->has_cmat, "the identity: no stage");
  const size_t fb = c->in_frame_bytes;
  Input in = load(a[0], fb, n, 0, 0, lens, 1);
  uint8_t *dst = inplace ? in.first : (uint8_t *)malloc(n * fb);
  if (!inplace) memset(dst, 0xA5, n * fb);  // (a byte the stage leaves out shows)
  const mjg_cmatrix &m = c->cmat;
  const CmatCoef coef{m.yu, m.yv, m.uu, m.uv, m.vu, m.vv};
  if (c->cmat_launch == launch_cmat<0, 0>) walk_cmat<0, 0>(in.sl, dst, c->cgeom, coef, n);
  else if (c->cmat_launch == launch_cmat<1, 1>) walk_cmat<1, 1>(in.sl, dst, c->cgeom, coef, n);
  else walk_cmat<1, 0>(in.sl, dst, c->cgeom, coef, n);
  save(a[1], dst, n * fb);
  if (!inplace) free(dst);
  for (uint8_t *b : in.bufs) free(b);
  delete c;
  return 0;
}

int tile(int argc, char **a) {
  if (argc < 14) return 2;
  const int w = atoi(a[2]), h = atoi(a[3]), shift = atoi(a[13]);
  const mjg_sheet sheet{atoi(a[6]), atoi(a[7]), atoi(a[8]), atoi(a[9]), atoi(a[10])};
  const std::vector<int> lens = lengths(a[11]);
  const bool apart = atoi(a[12]) != 0;
  CHECK(!lens.empty() && shift >= 0 && shift <= 15, "no segment, or a shift outside 0..15");
  int n = 0;
  SegList sl = one_seg(nullptr);  // (the stage reads one buffer: only the segments' first frames matter)
  for (int k = 0; k < (int)lens.size(); k++) sl.f0[k] = n, n += lens[k];
  mjg_ctx *c = plan(w, h, w, h, atoi(a[4]), atoi(a[5]), n, mjg_chain{}, &sheet);
  CHECK(c->sheet, "one cell without a margin: no stage");
  const SheetSplit sheets = sheet_split(c, sl, n);
  const int m = sheets.m;
  Input in = load(a[0], c->pic_frame_bytes, n, 0, shift);
  uint8_t *dbase = (uint8_t *)malloc(m * c->enc_frame_bytes + shift);
  memset(dbase + shift, 0x5A, m * c->enc_frame_bytes);  // (a byte the kernel leaves out shows)
  const bool uv1 = uv_paired(m) && !apart;
  for (int p = 0; p < uv_launches(uv1); p++) {
    const TileGeom g = tile_launch(c, p, uv1, sheets);
    for (int t = 0; t < g.gxy * uv_nz(p, uv1, m); t++)
      for (int tid = 0; tid < kCopyThreads; tid++) tile_work(in.first, dbase + shift, g, t, tid);
  }
  save(a[1], dbase + shift, m * c->enc_frame_bytes);
  free(in.bufs[0]);
  free(dbase);
  delete c;
  return 0;
}

int hist(int argc, char **a) {
  if (argc < 9) return 2;
  const int w = atoi(a[2]), h = atoi(a[3]), hs = atoi(a[4]), vs = atoi(a[5]), n = atoi(a[6]), lead = atoi(a[8]);
  const std::vector<int> lens = lengths(a[7]);
  HistGeom g;
  size_t fb;
  if (hist_plan(w, h, !hs ? MJG_CHROMA_444 : vs ? MJG_CHROMA_420 : MJG_CHROMA_422, n, &g, &fb)) {
    fprintf(stderr, "refused: %s\n", mjg_last_error());
    exit(5);
  }
  Input in = load(a[0], fb, n, 0, lead, lens, lead);
  uint32_t *out = (uint32_t *)calloc((size_t)n * 768, sizeof(uint32_t));
  uint32_t *lh = (uint32_t *)malloc(sizeof(uint32_t) * 256 * kHistCopies);  // the kernel's LDS, at exactly its size
  for (int t = 0; t < g.gpf * n; t++) {  // the two steps, thread by thread, with the workgroup barrier between them
    memset(lh, 0, sizeof(uint32_t) * 256 * kHistCopies);
    for (int tid = 0; tid < kHistThreads; tid++) hist_count(in.sl, lh, g, t, tid);
    for (int tid = 0; tid < kHistThreads; tid++) hist_flush(lh, out, g, t, tid);
  }
  save(a[1], (const uint8_t *)out, (size_t)n * 768 * sizeof(uint32_t));
  printf("%d workgroups a frame (Y %d, U and V %d each), %d frames\n", g.gpf, g.gy, g.gc, n);
  for (uint8_t *b : in.bufs) free(b);
  free(out);
  free(lh);
  return 0;
}

int hqdn3d(int argc, char **a) {
  if (argc < 12) return 2;
  const int w = atoi(a[4]), h = atoi(a[5]), n = atoi(a[8]), lead = atoi(a[10]);
  const std::vector<int> lens = lengths(a[9]);
  std::vector<int> chunks = lengths(a[11]);
  CHECK(lens.empty() || chunks.empty(), "segments in continued submits");
  CHECK(lead >= 0 && lead <= 15, "a lead outside 0..15");
  if (chunks.empty()) chunks.push_back(n);
  mjg_denoise *tabs = new mjg_denoise;
  FILE *f = fopen(a[1], "rb");
  CHECK(f && fread(tabs, 1, sizeof *tabs, f) == sizeof *tabs, "cannot read %s", a[1]);
  fclose(f);
  mjg_config k{};
  k.src_w = k.dst_w = w, k.src_h = k.dst_h = h;
  k.in_full_range = 1, k.qscale = 5, k.sar_num = k.sar_den = 1, k.max_batch = n;
  mjg_chain chain{};
  k.chroma_format = chain.src_chroma_format = !atoi(a[6]) ? MJG_CHROMA_444 : atoi(a[7]) ? MJG_CHROMA_420 : MJG_CHROMA_422;
  mjg_ctx *c = new mjg_ctx();
  Layout lay;
  if (plan_ctx(k, chain, nullptr, true, c, &lay, tabs)) {
    fprintf(stderr, "refused: %s\n", mjg_last_error());
    exit(5);
  }
  CHECK(c->dn, "no denoiser in the plan");
  const size_t fb = c->in_frame_bytes;
  const bool behind = argc > 12 && atoi(a[12]) && !lens.empty();
  Input in = load(a[0], fb, n, 0, lead, behind ? std::vector<int>{} : lens, lead);
  if (behind) {
    SegList starts = one_seg(nullptr);
    for (int k = 0, at = 0; k < kMaxSegs; k++) {
      starts.f0[k] = k < (int)lens.size() ? at : INT_MAX;
      if (k < (int)lens.size()) at += lens[k];
    }
    in.sl = seg_starts(starts, in.first, fb);
  }
  uint8_t *dbase = (uint8_t *)malloc(n * fb + lead), *dst = dbase + lead;
  memset(dst, 0xA5, n * fb);
  uint16_t *state = (uint16_t *)malloc(fb * sizeof(uint16_t));
  memset(state, 0x5A, fb * sizeof(uint16_t));
  // the kernels' LDS, at exactly their sizes; a lane's carry lives in a register
  uint8_t *ls = (uint8_t *)malloc(kDnRowWaves * 64 * kDnSrcStride);
  uint16_t *lp16 = (uint16_t *)malloc(sizeof(uint16_t) * kDnRowWaves * 64 * kDnPStride);
  int done = 0;
  for (size_t ci = 0; ci < chunks.size(); ci++) {
    const int m = chunks[ci], cont = ci > 0;
    CHECK(done + m <= n, "the submits' frames are more than nframes");
    uint16_t *p16 = (uint16_t *)malloc(sizeof(uint16_t) * m * c->dn_felems);  // a slot's buffer, for this submit's frames
    memset(p16, 0xEE, sizeof(uint16_t) * m * c->dn_felems);
    SegList sl = in.sl;
    if (lens.empty()) sl = one_seg(in.first + (size_t)done * fb);
    uint8_t *d = dst + (size_t)done * fb;
    const bool uv1 = uv_paired(m);
    for (int p = 0; p < uv_launches(uv1); p++) {
      const DnGeom g = dn_launch(c, 0, p, uv1, m, cont);
      const int16_t *S = (const int16_t *)tabs + g.tab * kDnTabLen;
      for (int t = 0; t < g.gxy * dn_nz(0, p, uv1, m); t++) {
        int carry[kDnRowThreads] = {};
        for (int ti = 0; ti < (g.w + 63) >> 6; ti++) {  // the three steps, thread by thread, with the barriers between them
          for (int tid = 0; tid < kDnRowThreads; tid++) dn_rows_stage(sl, ls, g, t, tid, ti);
          for (int tid = 0; tid < kDnRowThreads; tid++) dn_rows_walk(ls, lp16, S, g, t, tid, ti, &carry[tid]);
          for (int tid = 0; tid < kDnRowThreads; tid++) dn_rows_store(lp16, p16, g, t, tid, ti);
        }
      }
    }
    for (int p = 0; p < uv_launches(uv1); p++) {
      const DnGeom g = dn_launch(c, 1, p, uv1, m, cont);
      const int16_t *S = (const int16_t *)tabs + g.tab * kDnTabLen;
      for (int t = 0; t < g.gxy * dn_nz(1, p, uv1, m); t++)
        for (int tid = 0; tid < kDnColThreads; tid++) dn_cols_work(p16, S, g, t, tid);
    }
    for (int p = 0; p < uv_launches(uv1); p++) {
      const DnGeom g = dn_launch(c, 2, p, uv1, m, cont);
      const int16_t *M = (const int16_t *)tabs + (2 + g.tab) * kDnTabLen;
      for (int t = 0; t < g.gxy * dn_nz(2, p, uv1, m); t++)
        for (int tid = 0; tid < kDnTimeThreads; tid++) dn_time_work(sl, p16, state, d, M, g, t, tid);
    }
    free(p16);
    done += m;
  }
  CHECK(done == n, "the submits' frames are not nframes");
  save(a[2], dst, n * fb);
  save(a[3], (const uint8_t *)state, fb * sizeof(uint16_t));
  for (uint8_t *b : in.bufs) free(b);
  free(dbase), free(state), free(ls), free(lp16);
  delete tabs;
  delete c;
  return 0;
}

long g_loads = 0, g_copies = 0;

template <int MX, int MY>
void walk_sharp(const SharpGeom &g, const uint8_t *src, uint8_t *dst, int nz, std::vector<uint8_t> &written) {
  // the kernel's LDS, at exactly its sizes
  uint8_t *lb = (uint8_t *)malloc(sharp_lds_bytes(MX, MY));
  uint32_t *ls = (uint32_t *)malloc(sizeof(uint32_t) * sharp_lds_sums(MY));
  const int sx = MX ? MX / 2 : g.sx, sy = MY ? MY / 2 : g.sy;
  const int nst = (sharp_pitch(sx) / 4 * sharp_rows(sy) + kSharpThreads - 1) / kSharpThreads;
  for (int t = 0; t < g.gxy * nz; t++) {
    long long pa;
    const SharpTile T = sharp_block(g, t, &pa);
    // the address walk
    for (int tid = 0; tid < kSharpThreads; tid++) {
      for (int it = 0; T.filt && it < nst + 1; it++) {
        int lat;
        long long at[4];
        bool whole;
        if (!sharp_fetch(g, T, sx, sy, tid, it, &lat, at, &whole)) continue;
        for (int k = 0; k < 4; k++) {
          const int y = (int)(at[k] / g.cw), x = (int)(at[k] % g.cw);
          CHECK(x >= g.px && x < g.px + g.w && y >= g.py && y < g.py + g.h, "load at (%d, %d) outside the picture", x, y);
          CHECK(!whole || at[k] == at[0] + k, "a dword load of bytes that are not consecutive");
          g_loads++;
        }
        CHECK(lat >= 0 && lat % 4 == 0 && lat + 4 <= sharp_lds_bytes(MX, MY), "LDS byte %d", lat);
      }
      for (int it = 0; it < kSharpQuads / kSharpThreads; it++) {
        int col, row, n, pic;
        long long at;
        if (!sharp_store(g, T, tid, it, &col, &row, &at, &n, &pic)) continue;
        CHECK(n >= 1 && n <= 4 && at >= 0 && at + n <= (long long)g.cw * g.ch, "store at %lld outside the plane", at);
        for (int k = 0; k < n; k++) {
          const int y = (int)((at + k) / g.cw), x = (int)((at + k) % g.cw);
          CHECK(((pic >> k) & 1) == (x >= g.px && x < g.px + g.w && y >= g.py && y < g.py + g.h), "pic at (%d, %d)", x, y);
          CHECK(pa + at + k >= 0 && (size_t)(pa + at + k) < written.size(), "store at frame byte %lld", pa + at + k);
          CHECK(written[pa + at + k] == 0, "byte %lld written twice", pa + at + k);
          written[pa + at + k] = 1;
          if (!T.filt || !((pic >> k) & 1)) g_copies++;
        }
        CHECK((pic >> n) == 0, "pic bits past the plane");
      }
    }
    // the three steps, thread by thread, with the workgroup barriers between them
    if (T.filt) {
      for (int tid = 0; tid < kSharpThreads; tid++) sharp_stage<MX, MY>(src + pa, g, T, tid, lb);
      for (int tid = 0; tid < kSharpThreads; tid++) sharp_hpass<MX, MY>(g, tid, lb, ls);
    }
    for (int tid = 0; tid < kSharpThreads; tid++) sharp_vpass<MX, MY>(src + pa, dst + pa, g, T, tid, lb, ls);
  }
  free(lb);
  free(ls);
}

int unsharp(int argc, char **a) {
  if (argc < 18) return 2;
  int v[16];
  for (int i = 0; i < 16; i++) v[i] = atoi(a[2 + i]);
  const int n = v[14];
  const mjg_unsharp us{v[8], v[9], v[10], v[11], v[12], v[13]};
  mjg_chain ch{};
  ch.unsharp = &us;
  ch.has_pad = 1, ch.pad_w = v[0], ch.pad_h = v[1], ch.pad_x = v[4], ch.pad_y = v[5];
  mjg_ctx *c = plan(v[6], v[7], v[6], v[7], v[2], v[3], n, ch);
  CHECK(c->sharp, "both amounts 0: no stage");
  const size_t fb = c->pic_frame_bytes;
  Input in = load(a[0], fb, n, 0, 0);
  uint8_t *dst = (uint8_t *)malloc(n * fb);
  memset(dst, 0xA5, n * fb);
  std::vector<uint8_t> written(n * fb, 0);
  const bool uv1 = uv_paired(n) && !v[15];
  for (int p = 0; p < uv_launches(uv1); p++) {
    const SharpGeom g = sharp_launch(c, p, uv1, n);
    if (c->shpass[p ? 1 : 0].launch == launch_sharp<5, 5>) walk_sharp<5, 5>(g, in.first, dst, uv_nz(p, uv1, n), written);
    else walk_sharp<0, 0>(g, in.first, dst, uv_nz(p, uv1, n), written);
  }
  for (size_t i = 0; i < n * fb; i++) CHECK(written[i] == 1, "byte %zu never written", i);
  save(a[1], dst, n * fb);
  printf("%ld staged loads inside the picture, %ld copied samples, %zu bytes each stored once\n", g_loads, g_copies, n * fb);
  free(in.bufs[0]);
  free(dst);
  delete c;
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const struct {
    const char *name;
    int (*run)(int, char **);
  } stages[] = {{"yadif", yadif}, {"lut", lut}, {"cmat", cmat}, {"tile", tile}, {"unsharp", unsharp}, {"hist", hist},
                {"hqdn3d", hqdn3d}};
  for (const auto &s : stages)
    if (argc > 1 && !strcmp(argv[1], s.name)) return s.run(argc - 2, argv + 2);
  fprintf(stderr, "usage: stage_host yadif|lut|cmat|tile|unsharp|hist|hqdn3d ...\n");
  return 2;
}
