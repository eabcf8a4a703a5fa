// Host-side check of the open path's device-free steps (check_config, and plan_ctx for what it accepts)
// for the eight orientations of the test shapes, meant for a sanitizer build on a machine without
// a GPU: no HIP call is made.  Every geometry is checked against the sizes computed here: the
// frame byte count, the plane offsets and strides of the oriented frame, and that each orientation
// pass's tiles and pieces cover its plane and nothing more.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     -I include -I ffmpeg_distributed_amd/csrc -o orient_host_check tools/orient_host_check.hip \
//     ffmpeg_distributed_amd/csrc/sws_filter.cpp && ./orient_host_check
#include "api.hip"

#include <cstdio>

namespace {
int fails = 0;
void expect(bool ok, const char *what, int w, int h, int cf, int orient) {
  if (ok) return;
  fails++;
  fprintf(stderr, "FAIL %s: %dx%d format %d orient %d (%s)\n", what, w, h, cf, orient, mjg_last_error());
}
}  // namespace

int main() {
  struct Shape { int w, h, cf; };
  const Shape shapes[] = {{130, 66, MJG_CHROMA_420}, {130, 66, MJG_CHROMA_444}, {131, 67, MJG_CHROMA_420},
                          {33, 17, MJG_CHROMA_444},  {8, 8, MJG_CHROMA_420},    {130, 66, MJG_CHROMA_422},
                          {70, 150, MJG_CHROMA_420}, {3840, 2160, MJG_CHROMA_420}};
  int ran = 0;
  for (const Shape &s : shapes)
    for (int orient = -1; orient <= 8; orient++) {
      const int T = orient & 1, ow = T ? s.h : s.w, oh = T ? s.w : s.h;
      mjg_config k{};
      k.src_w = s.w, k.src_h = s.h, k.dst_w = ow, k.dst_h = oh;
      k.in_full_range = 0, k.qscale = 5, k.sar_num = k.sar_den = 1, k.max_batch = 3, k.chroma_format = s.cf;
      mjg_chain chain{};
      chain.src_chroma_format = s.cf, chain.orient = orient;
      Layout lay{};
      const int rc = check_config(k, chain, &lay);
      const bool bad = orient < 0 || orient > 7 || (T && s.cf == MJG_CHROMA_422);
      expect((rc == MJG_E_INVALID) == bad && (rc == MJG_OK) == !bad, "check_config", s.w, s.h, s.cf, orient);
      if (rc) continue;
      // a crop that fits the source but not the oriented frame
      if (T && s.w != s.h) {
        mjg_chain c2 = chain;
        c2.has_crop = 1, c2.crop_w = s.w, c2.crop_h = s.h;
        Layout l2{};
        expect(check_config(k, c2, &l2) == MJG_E_INVALID, "crop of the source size", s.w, s.h, s.cf, orient);
      }
      mjg_ctx *c = new mjg_ctx();
      expect(plan_ctx(k, chain, nullptr, true, c, &lay) == MJG_OK, "plan_ctx", s.w, s.h, s.cf, orient);
      const int hs = s.cf == MJG_CHROMA_444 ? 0 : 1, vs = s.cf == MJG_CHROMA_420 ? 1 : 0;
      const int cw = (s.w + hs) >> hs, ch = (s.h + vs) >> vs;
      const int ocw = (ow + hs) >> hs, och = (oh + vs) >> vs;
      const size_t fb = (size_t)s.w * s.h + 2 * (size_t)cw * ch;
      expect(c->in_frame_bytes == fb && c->enc_frame_bytes == fb && !c->scale, "frame bytes", s.w, s.h, s.cf, orient);
      expect(c->geom.w == ow && c->geom.h == oh && c->geom.y_stride == ow && c->geom.c_stride == ocw &&
                 c->geom.u_off == (long long)ow * oh && c->geom.v_off == (long long)ow * oh + (long long)ocw * och &&
                 c->src_cplane == (long long)cw * ch && c->orient == orient,
             "oriented geometry", s.w, s.h, s.cf, orient);
      for (int p = 0; p < 2 && orient; p++) {
        const OrientGeom &g = c->opass[p].g;
        const int pw = p ? cw : s.w, ph = p ? ch : s.h;
        bool ok = c->opass[p].launch != nullptr && g.sw == pw && g.sh == ph && g.s_off == g.d_off &&
                  g.s_off == (p ? (long long)s.w * s.h : 0) && g.s_off + (long long)(p ? 2 : 1) * pw * ph <= (long long)fb &&
                  g.fy == ((orient >> 2) & 1) && g.gxy >= 1;
        if (T) {
          ok = ok && g.tx * kOrientTile >= pw && (g.tx - 1) * kOrientTile < pw && g.ntiles % g.tx == 0 &&
               (g.ntiles / g.tx) * kOrientTileH >= ph && (g.ntiles / g.tx - 1) * kOrientTileH < ph &&
               g.gxy * kOrientWaves >= g.ntiles && (g.gxy - 1) * kOrientWaves < g.ntiles;
        } else {
          ok = ok && (size_t)g.gxy * kCopyThreads * kCopyVecs * 16 + 15 >= (size_t)pw * ph;
        }
        expect(ok, p ? "chroma pass" : "luma pass", s.w, s.h, s.cf, orient);
      }
      delete c;  // (no stream, no buffer: nothing for free_ctx to release)
      ran++;
    }
  printf("%d geometries planned, %d failures\n", ran, fails);
  return fails ? 1 : 0;
}
