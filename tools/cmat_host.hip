// k_cmat_frame's body (scale.hip cmat_work, __host__ __device__) on the CPU: every (workgroup, thread) of the
// one launch of a colour-matrix stage, on buffers allocated at exactly the frames' sizes, so that
// AddressSanitizer sees any access outside them.  Built and driven by tools/cmat_host_check.py (hipcc
// -Xarch_host -fsanitize=address,undefined); makes no HIP call.
//   cmat_host IN OUT w h hshift vshift nframes split inplace c2 c3 c4 c5 c6 c7
// IN: nframes frames, packed planar, w x h with the chroma shifts given (api.hip plan_cmat: whole frames).
//   split: 0, or the lengths of up to kMaxSegs segments as a,b,... (their sum nframes): each segment in an
//   allocation of its own (mjg_submit_segments' SegList), one byte into it.
//   inplace: 1, the frames are converted where they lie (one segment), 0 into a second exact allocation.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "kernels.hip"
#include "scale.hip"
using namespace mjg;

static uint32_t magic32(uint32_t d) { return d > 1 ? (uint32_t)((((uint64_t)1 << 32) + d - 1) / d) : 0u; }

template <int HS, int VS>
static void walk(const SegList &sl, uint8_t *dst, const CmatGeom &g, const CmatCoef &cm, int n) {
  for (int t = 0; t < g.gxy * n; t++)
    for (int tid = 0; tid < kCmatThreads; tid++) cmat_work<HS, VS>(sl, dst, g, cm, t, tid);
}

int main(int argc, char **argv) {
  if (argc < 16) return 2;
  const char *in = argv[1], *outp = argv[2];
  const int w = atoi(argv[3]), h = atoi(argv[4]), hs = atoi(argv[5]), vs = atoi(argv[6]), n = atoi(argv[7]);
  std::vector<int> lens;
  for (const char *p = argv[8]; *p;) {
    char *e;
    const int v = (int)strtol(p, &e, 10);
    if (v > 0) lens.push_back(v);
    p = *e ? e + 1 : e;
  }
  const int nsegs = (int)lens.size();
  const bool inplace = atoi(argv[9]) != 0;
  if (nsegs > kMaxSegs || (nsegs && inplace)) return 2;
  const CmatCoef cm{atoi(argv[10]), atoi(argv[11]), atoi(argv[12]), atoi(argv[13]), atoi(argv[14]), atoi(argv[15])};
  CmatGeom g{};
  cmat_geom_frame(g, w, h, hs, vs);
  const size_t fb = (size_t)w * h + 2 * (size_t)g.cw * g.ch;
  g.s_fstride = g.d_fstride = (long long)fb;
  g.ppr_magic = magic32((uint32_t)g.ppr);
  g.gxy_magic = magic32((uint32_t)g.gxy);
  FILE *f = fopen(in, "rb");
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
  if (!inplace) memset(dbase, 0xA5, (size_t)n * fb);  // (a byte the stage leaves out shows)
  if (!hs) walk<0, 0>(sl, dbase, g, cm, n);
  else if (vs) walk<1, 1>(sl, dbase, g, cm, n);
  else walk<1, 0>(sl, dbase, g, cm, n);
  f = fopen(outp, "wb");
  fwrite(dbase, 1, (size_t)n * fb, f);
  fclose(f);
  if (!inplace) free(dbase);
  for (uint8_t *b : bufs) free(b);
  return 0;
}
