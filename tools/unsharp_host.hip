// k_unsharp_plane's three steps and its address arithmetic (scale.hip sharp_block / sharp_fetch / sharp_store /
// sharp_stage / sharp_hpass / sharp_vpass, all __host__ __device__) on the CPU: every (workgroup, thread, iteration)
// of the luma and the U + V launch of one submit, on source and destination buffers allocated at exactly the frames'
// size and LDS arrays allocated at exactly the kernel's, so that AddressSanitizer sees any access outside them.  It
// asserts besides that every staged load (a byte, or a dword of four consecutive bytes) lies inside the picture
// rectangle, that every other load is the copy of a sample outside the picture (or of a plane whose amount is 0) from
// its own place, and that every byte of every plane of every frame is stored exactly once.  Built and driven by tools/unsharp_host_check.py (hipcc -Xarch_host
// -fsanitize=address,undefined), which compares the output with tests/unsharp_ref.py; makes no HIP call.
//   unsharp_host IN OUT PW PH hshift vshift PX PY W H lx ly la cx cy ca nframes split
// IN: nframes frames of the encoded size PW x PH (the canvas under a pad; else PX = PY = 0, W x H = PW x PH), packed
// planar, the W x H picture at (PX, PY); la / ca are the filter's integers; split: U and V in a launch each (poff 0, V's
// off advanced by the chroma plane, nz = nframes), as always past 32,767 frames.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "kernels.hip"
#include "scale.hip"
using namespace mjg;

static long g_loads = 0, g_copies = 0;

#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      fprintf(stderr, __VA_ARGS__);   \
      fprintf(stderr, "\n");          \
      exit(4);                        \
    }                                 \
  } while (0)

template <int MX, int MY>
static void run_launch(const SharpGeom &g, const uint8_t *src, uint8_t *dst, int nz, std::vector<uint8_t> &written) {
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

int main(int argc, char **argv) {
  if (argc < 19) return 2;
  const char *in = argv[1], *outp = argv[2];
  int a[16];
  for (int i = 0; i < 16; i++) a[i] = atoi(argv[3 + i]);
  const int PW = a[0], PH = a[1], hs = a[2], vs = a[3], PX = a[4], PY = a[5], W = a[6], H = a[7];
  const int us[6] = {a[8], a[9], a[10], a[11], a[12], a[13]};
  const int n = a[14], split = a[15] || 2 * n > 65535;  // past 32,767 frames submit_impl launches U and V apart
  const int cw = (PW + hs) >> hs, ch = (PH + vs) >> vs;
  const size_t fb = (size_t)PW * PH + 2 * (size_t)cw * ch;
  uint8_t *src = (uint8_t *)malloc(n * fb), *dst = (uint8_t *)malloc(n * fb);
  FILE *f = fopen(in, "rb");
  if (!f || fread(src, 1, n * fb, f) != n * fb) return 3;
  fclose(f);
  memset(dst, 0xA5, n * fb);
  std::vector<uint8_t> written(n * fb, 0);
  for (int p = 0; p < (split ? 3 : 2); p++) {
    const int c = p ? 1 : 0;
    SharpGeom g = sharp_geom(c ? cw : PW, c ? ch : PH, c ? PX >> hs : PX, c ? PY >> vs : PY, c ? (W + hs) >> hs : W,
                             c ? (H + vs) >> vs : H, c ? (long long)PW * PH : 0, (long long)fb, us[3 * c], us[3 * c + 1],
                             us[3 * c + 2]);
    g.nf = n;
    if (p && !split) g.poff = (long long)cw * ch;
    if (p == 2) g.off += (long long)cw * ch;
    const int nz = p && !split ? 2 * n : n;
    if (us[3 * c] == 5 && us[3 * c + 1] == 5) run_launch<5, 5>(g, src, dst, nz, written);
    else run_launch<0, 0>(g, src, dst, nz, written);
  }
  for (size_t i = 0; i < n * fb; i++) CHECK(written[i] == 1, "byte %zu never written", i);
  f = fopen(outp, "wb");
  fwrite(dst, 1, n * fb, f);
  fclose(f);
  printf("%ld staged loads inside the picture, %ld copied samples, %zu bytes each stored once\n", g_loads, g_copies, n * fb);
  free(src);
  free(dst);
  return 0;
}
