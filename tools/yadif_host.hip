// k_yadif_plane's body (scale.hip yadif_work, __host__ __device__) on the CPU: every (workgroup, thread) of
// the luma and the U + V launch of one submit, on source and destination buffers allocated at exactly
// their sizes, so that AddressSanitizer sees any access outside a readable frame.  Built and driven by
// tools/yadif_host_check.py (hipcc -Xarch_host -fsanitize=address,undefined); makes no HIP call.
//   yadif_host IN OUT w h hshift vshift nospatial parity nframes halo split [apart]
// IN: nframes + halo frames, packed planar; split: 0, or the lengths of up to kMaxSegs segments as a,b,...
// (their sum nframes, no halo): each segment in an allocation of its own (mjg_submit_segments' SegList).
// apart: 1, U and V in a launch each whatever nframes is (submit_impl's `p == 2`: poff 0, off advanced by the
// chroma plane, nz = nframes); without it they are apart from 32,768 frames on, as submit_impl launches them.
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
  const char *in = argv[1], *outp = argv[2];
  const int w = atoi(argv[3]), h = atoi(argv[4]), hs = atoi(argv[5]), vs = atoi(argv[6]);
  const int nosp = atoi(argv[7]), parity = atoi(argv[8]), n = atoi(argv[9]), halo = atoi(argv[10]);
  std::vector<int> lens;  // the segments' lengths; empty: one segment of n frames and its halo
  for (const char *p = argv[11]; *p;) {
    char *e;
    const int v = (int)strtol(p, &e, 10);
    if (v > 0) lens.push_back(v);
    p = *e ? e + 1 : e;
  }
  const int nsegs = (int)lens.size();
  if (nsegs > kMaxSegs || (nsegs && halo)) return 2;
  const int hp = halo & 1, hn = (halo >> 1) & 1;
  const bool uv1 = 2 * n <= 65535 && !(argc > 12 && atoi(argv[12]));  // U and V in one launch
  const int cw = (w + hs) >> hs, ch = (h + vs) >> vs;
  const size_t fb = (size_t)w * h + 2 * (size_t)cw * ch;
  const size_t tot = (size_t)(n + hp + hn) * fb;
  FILE *f = fopen(in, "rb");
  // exact-size buffers: one for the submit and its halo, or one per segment
  std::vector<uint8_t *> bufs;
  SegList sl;
  if (!nsegs) {
    bufs.push_back((uint8_t *)malloc(tot));
    if (fread(bufs[0], 1, tot, f) != tot) return 3;
    for (int k = 0; k < kMaxSegs; k++) sl.p[k] = bufs[0] + hp * fb, sl.f0[k] = k ? INT_MAX : 0;
  } else {
    int at = 0;
    for (int k = 0; k < nsegs; k++) {
      bufs.push_back((uint8_t *)malloc(lens[k] * fb));
      if (fread(bufs[k], 1, lens[k] * fb, f) != lens[k] * fb) return 3;
      sl.p[k] = bufs[k], sl.f0[k] = at;
      at += lens[k];
    }
    if (at != n) return 2;
    for (int k = nsegs; k < kMaxSegs; k++) sl.p[k] = bufs[0], sl.f0[k] = INT_MAX;  // as mjg_submit_segments fills them
  }
  fclose(f);
  // destination at an odd alignment inside an exact allocation: d + 1
  uint8_t *dbase = (uint8_t *)malloc(n * fb);
  for (int p = 0; p < (uv1 ? 2 : 3); p++) {
    DeintGeom g{};
    g.w = p ? cw : w;
    g.h = p ? ch : h;
    g.off = p ? (long long)w * h : 0;
    g.fstride = (long long)fb;
    g.parity = parity;
    g.w_magic = magic32(g.w);
    const size_t pieces = ((size_t)g.w * g.h) >> 4;
    g.gxy = (int)std::max<size_t>(1, (pieces + kDeintThreads - 1) / kDeintThreads);
    g.gxy_magic = magic32(g.gxy);
    g.nf = n;
    for (int k = 0; k < kMaxSegs; k++) {
      const int end = k + 1 < kMaxSegs && sl.f0[k + 1] != INT_MAX ? sl.f0[k + 1] : n;
      g.lo[k] = -hp;
      g.hi[k] = sl.f0[k] == INT_MAX ? 0 : end - sl.f0[k] - 1 + hn;
    }
    if (p && uv1) g.poff = (long long)cw * ch;
    if (p == 2) g.off += (long long)cw * ch;
    const int nz = p && uv1 ? 2 * n : n;
    for (int t = 0; t < g.gxy * nz; t++)
      for (int tid = 0; tid < kDeintThreads; tid++) {
        if (nosp) yadif_work<true>(sl, dbase, g, t, tid);
        else yadif_work<false>(sl, dbase, g, t, tid);
      }
  }
  f = fopen(outp, "wb");
  fwrite(dbase, 1, n * fb, f);
  fclose(f);
  for (uint8_t *b : bufs) free(b);
  free(dbase);
  return 0;
}
