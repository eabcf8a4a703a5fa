// k_lut_plane's body (scale.hip lut_work, __host__ __device__) on the CPU: every (workgroup, thread) of the
// luma and the U + V launch of one table stage, on buffers allocated at exactly the frames' sizes, so that
// AddressSanitizer sees any access outside them.  Built and driven by tools/lut_host_check.py (hipcc
// -Xarch_host -fsanitize=address,undefined); makes no HIP call.
//   lut_host IN TABS OUT w h hshift vshift nframes split apart inplace [cw ch px py]
// IN: nframes frames, packed planar; TABS: the Y, U and V table, 768 bytes.
// Without the last four values the stage is slot "in" (api.hip plan_lut): whole planes of w x h frames.
//   split: 0, or the lengths of up to kMaxSegs segments as a,b,... (their sum nframes): each segment in an
//   allocation of its own (mjg_submit_segments' SegList), one byte into it.
//   inplace: 1, the frames are mapped where they lie (one segment), 0 into a second exact allocation.
// With them it is slot "out": the frames are cw x ch canvases, the w x h picture at (px, py) is mapped in
// place and no other byte is read or written (the check compares the border).
// apart: 1, U and V in a launch each whatever nframes is (launch_lut's `p == 2`); without it they are
// apart from 32,768 frames on.  A launch whose planes all have the identity table is left out in place.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "kernels.hip"
#include "scale.hip"
using namespace mjg;

static uint32_t magic32(uint32_t d) { return d > 1 ? (uint32_t)((((uint64_t)1 << 32) + d - 1) / d) : 0u; }

int main(int argc, char **argv) {
  if (argc < 12) return 2;
  const char *in = argv[1], *tabp = argv[2], *outp = argv[3];
  const int w = atoi(argv[4]), h = atoi(argv[5]), hs = atoi(argv[6]), vs = atoi(argv[7]), n = atoi(argv[8]);
  std::vector<int> lens;
  for (const char *p = argv[9]; *p;) {
    char *e;
    const int v = (int)strtol(p, &e, 10);
    if (v > 0) lens.push_back(v);
    p = *e ? e + 1 : e;
  }
  const int nsegs = (int)lens.size();
  const bool apart = atoi(argv[10]) != 0, out_slot = argc >= 16;
  const bool inplace = atoi(argv[11]) != 0 || out_slot;
  if (nsegs > kMaxSegs || (nsegs && inplace)) return 2;
  const int cw = out_slot ? atoi(argv[12]) : w, ch = out_slot ? atoi(argv[13]) : h;
  const int px = out_slot ? atoi(argv[14]) : 0, py = out_slot ? atoi(argv[15]) : 0;
  const int ccw = (cw + hs) >> hs, cch = (ch + vs) >> vs;  // the frame's chroma planes
  const size_t fb = (size_t)cw * ch + 2 * (size_t)ccw * cch;
  uint8_t tabs[768];
  FILE *f = fopen(tabp, "rb");
  if (!f || fread(tabs, 1, 768, f) != 768) return 3;
  fclose(f);
  int ident = 0;
  for (int i = 0; i < 3; i++) {
    bool id = true;
    for (int v = 0; v < 256; v++) id = id && tabs[256 * i + v] == v;
    ident |= id ? 1 << i : 0;
  }
  f = fopen(in, "rb");
  if (!f) return 3;
  // exact-size buffers: one for the submit, or one per segment (each one byte into an allocation of a byte more)
  std::vector<uint8_t *> bufs;
  SegList sl;
  if (!nsegs) {
    bufs.push_back((uint8_t *)malloc((size_t)n * fb));
    if (fread(bufs[0], 1, (size_t)n * fb, f) != (size_t)n * fb) return 3;
    for (int k = 0; k < kMaxSegs; k++) sl.p[k] = bufs[0], sl.f0[k] = k ? INT_MAX : 0;
  } else {
    int at = 0;
    for (int k = 0; k < nsegs; k++) {
      bufs.push_back((uint8_t *)malloc(lens[k] * fb + 1));
      if (fread(bufs[k] + 1, 1, lens[k] * fb, f) != lens[k] * fb) return 3;
      sl.p[k] = bufs[k] + 1, sl.f0[k] = at;
      at += lens[k];
    }
    if (at != n) return 2;
    for (int k = nsegs; k < kMaxSegs; k++) sl.p[k] = sl.p[0], sl.f0[k] = INT_MAX;  // as mjg_submit_segments fills them
  }
  fclose(f);
  uint8_t *dbase = inplace ? bufs[0] : (uint8_t *)malloc((size_t)n * fb);
  const bool uv1 = 2 * n <= 65535 && !apart;
  const long long cplane = (long long)ccw * cch;
  for (int p = 0; p < (uv1 ? 2 : 3); p++) {
    LutGeom g{};
    const int rw = p ? (w + hs) >> hs : w, rh = p ? (h + vs) >> vs : h;  // the rectangle
    const int stride = p ? ccw : cw;
    lut_geom_rect(g, rw, rh, stride, stride);
    g.s_off = g.d_off = (p ? (long long)cw * ch : 0) + (long long)(p ? py >> vs : py) * stride + (p ? px >> hs : px);
    g.s_fstride = g.d_fstride = (long long)fb;
    g.tab = p;
    g.ident = ident;
    g.ds_magic = magic32((uint32_t)g.d_stride);
    g.gxy_magic = magic32((uint32_t)g.gxy);
    g.nf = n;
    if (p && uv1) g.s_poff = g.d_poff = cplane;
    if (p == 2) g.s_off += cplane, g.d_off += cplane, g.tab = 2;
    const int tb = p && uv1 ? 6 : 1 << g.tab;
    if (inplace && (g.ident & tb) == tb) continue;
    const int nz = p && uv1 ? 2 * n : n;
    for (int t = 0; t < g.gxy * nz; t++)
      for (int tid = 0; tid < kCopyThreads; tid++) lut_work(sl, dbase, g, tabs, t, tid);
  }
  f = fopen(outp, "wb");
  fwrite(dbase, 1, (size_t)n * fb, f);
  fclose(f);
  if (!inplace) free(dbase);
  for (uint8_t *b : bufs) free(b);
  return 0;
}
