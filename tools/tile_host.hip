// k_tile_plane's body (scale.hip tile_work, __host__ __device__) on the CPU: every (workgroup, thread) of the
// luma and the U + V launch of one submit, on buffers allocated at exactly the frames' sizes, so that
// AddressSanitizer sees any access outside them.  Built and driven by tools/tile_host_check.py (hipcc
// -Xarch_host -fsanitize=address,undefined); makes no HIP call.
//   tile_host IN OUT w h hshift vshift cols rows N margin padding segs apart shift
// IN: the cell frames of the submit, packed planar w x h, one buffer (the sws stage's output).
//   segs: the frames of each of up to kMaxSegs segments as a,b,... (api.hip submit_impl: each a sequence of
//   its own, its sheets behind those of the one before).
//   apart: 1, U and V in a launch each whatever the sheet count is (submit_impl's `p == 2`).
//   shift: both buffers start this many bytes into an allocation that many bytes larger (0..15: the
//   alignment of the sheet planes, which the pieces are cut on).
// OUT: the sheets, packed planar.  The geometry is api.hip's plan_tile and submit_impl.
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
  if (argc < 15) return 2;
  const char *in = argv[1], *outp = argv[2];
  const int w = atoi(argv[3]), h = atoi(argv[4]), hs = atoi(argv[5]), vs = atoi(argv[6]);
  const int cols = atoi(argv[7]), rows = atoi(argv[8]), N = atoi(argv[9]), margin = atoi(argv[10]), padding = atoi(argv[11]);
  std::vector<int> lens;
  for (const char *p = argv[12]; *p;) {
    char *e;
    const int v = (int)strtol(p, &e, 10);
    if (v > 0) lens.push_back(v);
    p = *e ? e + 1 : e;
  }
  const bool apart = atoi(argv[13]) != 0;
  const int shift = atoi(argv[14]);
  const int nsegs = (int)lens.size();
  if (nsegs < 1 || nsegs > kMaxSegs || N < 1 || N > cols * rows || shift < 0 || shift > 15) return 2;
  const int W = cols * w + (cols - 1) * padding + 2 * margin, H = rows * h + (rows - 1) * padding + 2 * margin;
  const int cw = (w + hs) >> hs, ch = (h + vs) >> vs, CW = (W + hs) >> hs, CH = (H + vs) >> vs;
  const size_t cell_b = (size_t)w * h + 2 * (size_t)cw * ch, sheet_b = (size_t)W * H + 2 * (size_t)CW * CH;
  int n = 0, m = 0, sheet0[kMaxSegs], first[kMaxSegs], count[kMaxSegs];
  for (int k = 0; k < kMaxSegs; k++) {
    const bool used = k < nsegs;
    sheet0[k] = used ? m : INT_MAX, first[k] = used ? n : 0, count[k] = used ? lens[k] : 0;
    if (used) n += lens[k], m += (lens[k] + N - 1) / N;
  }
  uint8_t *sbase = (uint8_t *)malloc((size_t)n * cell_b + shift), *dbase = (uint8_t *)malloc((size_t)m * sheet_b + shift);
  FILE *f = fopen(in, "rb");
  if (!f || fread(sbase + shift, 1, (size_t)n * cell_b, f) != (size_t)n * cell_b) return 3;
  fclose(f);
  memset(dbase + shift, 0x5A, (size_t)m * sheet_b);  // (a byte the kernel leaves out shows)
  const bool uv1 = 2 * m <= 65535 && !apart;
  for (int p = 0; p < (uv1 ? 2 : 3); p++) {
    const int phs = p ? hs : 0, pvs = p ? vs : 0;
    TileGeom g{};
    g.w = w >> phs, g.h = h >> pvs;
    g.W = p ? CW : W, g.H = p ? CH : H;
    g.pw = g.w + (padding >> phs), g.ph = g.h + (padding >> pvs);
    g.mx = margin >> phs, g.my = margin >> pvs;
    g.cols = cols, g.ncells = cols * rows, g.N = N;
    g.fill = p ? 128 : 0;
    g.s_off = p ? (long long)w * h : 0, g.d_off = p ? (long long)W * H : 0;
    g.s_fstride = (long long)cell_b, g.d_fstride = (long long)sheet_b;
    g.W_magic = magic32((uint32_t)g.W), g.pw_magic = magic32((uint32_t)g.pw), g.ph_magic = magic32((uint32_t)g.ph);
    g.gxy = tile_gxy(g.W, g.H);
    g.gxy_magic = magic32((uint32_t)g.gxy);
    g.ns = m;
    for (int k = 0; k < kMaxSegs; k++) g.sheet0[k] = sheet0[k], g.first[k] = first[k], g.count[k] = count[k];
    const long long s_cplane = (long long)cw * ch, d_cplane = (long long)CW * CH;
    if (p && uv1) g.s_poff = s_cplane, g.d_poff = d_cplane;
    if (p == 2) g.s_off += s_cplane, g.d_off += d_cplane;
    const int nz = p && uv1 ? 2 * m : m;
    for (int t = 0; t < g.gxy * nz; t++)
      for (int tid = 0; tid < kCopyThreads; tid++) tile_work(sbase + shift, dbase + shift, g, t, tid);
  }
  f = fopen(outp, "wb");
  fwrite(dbase + shift, 1, (size_t)m * sheet_b, f);
  fclose(f);
  free(sbase);
  free(dbase);
  return 0;
}
