// Bicubic resize of one plane for the `-vf scale=W:H:flags=bicubic` leg of the
// reference worker's remote_args (ffmpeg_distributed.py:134).  Applies swscale's
// fixed-point tables (sws_filter.cpp) exactly as libswscale's C path does:
//   hScale8To15_c: min((sum src*f) >> 7, 32767)            (14-bit coeffs)
//   lumRangeToJpeg_c / chrRangeToJpeg_c on that int16       (tv -> pc, if requested)
//   yuv2planeX_8_c: clip_u8(((64 << 12) + sum h*f) >> 19)  (12-bit coeffs, flat dither)
//
// One workgroup = a 64 x TH output tile (4 waves, lane = output column).  TH = 64 for the 2:1
// filters (8 h taps, 5 v pairs: 4K -> 1080p, windows of <= 36 dwords x 140 rows; the host
// checks) with the row-pair image written over the window rows it was computed from (a
// pair's two rows are read only by the wave that writes it, in program order), so the LDS of
// a 64-row tile is that of the 32-row one, and rows at a fixed 36-dword stride (pair stride
// 72: constant LDS offsets in the v-pass); TH = 32 otherwise.
//   load:   the tile's source window (rows x dword-aligned columns, rows padded to 16-byte
//           pieces) is staged in LDS from 16-byte loads, 7 rows x 9 pieces per wave-instruction,
//           all issued before any is waited on.  (Measured on MI355X, c4: a persistent
//           variant that loads the next tile's window during this tile's passes ran ~20%
//           slower -- tile index arithmetic, and 7 instead of 8 workgroups per CU -- and
//           unaligned ds_read_b64 tap reads instead of the funnel shifts ran ~2x slower.)
//   h-pass: wave w computes source row pairs p0+w, p0+w+4, ... of the window for its lane's
//           column: taps funnel-shifted out of aligned LDS dwords (v_alignbit), widened to
//           u16 pairs with v_perm and multiplied with v_dot2_i32_i16 against the column's
//           coefficient pairs (registers).  Rows 2p and 2p+1 go to LDS as one int16 pair.
//           D4 (every coefficient c = 128 ch + cl with int8 ch, cl in [-64, 64)): the window
//           is staged level-shifted (byte ^ 0x80 = p - 128 as int8) and four taps are one
//           v_dot4_i32_i8 against the hi and one against the lo bytes, no widening:
//           sum p c >> 7 = ah + (al >> 7) + sum c (exact: 128 (ah + sum c) is a multiple of 128).
//   v-pass: output row y reads the pairs [vps[y], vps[y] + npv) of its column and dot2s
//           them against that row's coefficient pairs, which the host pre-shifts by the
//           parity of the first tap row (zero-padded), so odd and even starts cost the same.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mjg {

typedef short short2_t __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kScaleTileW = 64;
constexpr int kScaleLoadRows = 7;  // fast window path: rows x 9 pieces per wave-instruction
__host__ __device__ constexpr int scale_loads_per_wave(int th) { return th >= 64 ? 5 : 3; }
// waves per workgroup for a tile height (128-row tiles, which no context launches: 8 waves, 512 threads)
__host__ __device__ constexpr int scale_waves(int th) { return th == 128 ? 8 : 4; }
constexpr int kScaleAliasWords = 36;  // TH 64: LDS row stride (dwords), the widest fast window
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a1 __attribute__((aligned(1)));  // window pieces start at any byte

struct ScaleGeom {
  int sw, sh, dw, dh;            // plane sizes
  int s_stride, d_stride;
  long long s_off, d_off;        // plane offset inside a frame
  long long s_fstride, d_fstride;  // frame strides
  int nf;                        // frames per plane: blockIdx.z >= nf is the next plane (U, V in one launch)
  uint32_t sw_magic;             // k_plane_copy of a rectangle: ceil(2^32 / sw) (0 when sw == 1); in
                                 // the padding before s_poff, so the fields after it stay where they were
  long long s_poff, d_poff;      // that plane's offset from this one
  int htaps, vtaps;              // htaps multiple of 4 (filterAlign 4), vtaps even
  int npv;                       // coefficient pairs per output row (vtaps/2 + 1)
  int range;                     // 0 none, 1 luma tv->pc, 2 chroma tv->pc
  int lds_pairs;                 // max row pairs any tile needs
  int lds_win_words;             // max source-window dwords any tile needs (TH 64: rows at
                                 // kScaleAliasWords, the pair image inside it)
  // the launch is a 1-D grid of gx * gy * (planes x frames) tiles; tile t -> (bx, by, z) by
  // multiply-high with ceil(2^32 / d), not by two scalar divisions (div_magic)
  int gx, gxy;
  uint32_t gx_magic, gxy_magic;  // 0 when the divisor is 1
  int mf_bx0, mf_bx1, mf_hs;     // tile columns [mf_bx0, mf_bx1) take the matrix-core h-pass
                                 // (one filter, hsum mf_hs; the host checks: api.hip)
  int mv_by0, mv_by1, mv_k;      // of those, tile rows [mv_by0, mv_by1) take the matrix-core v-pass
                                 // (one filter; mv_k = 128 * its tap sum + (64 << 12))
};

// The matrix-core v-pass's byte planes (k_scale): per output column, the h values of the tile's
// window rows as hi bytes ([col][row], this stride) and then as lo bytes ^ 0x80
constexpr int kPlaneStride = 144;  // >= the 136 window rows of a 64-row 2:1 tile, 16-byte multiple
constexpr int kMvFragOff = 512;    // words of mfb before the v-pass A fragments (3 x 64 lanes x 16 B)

// t / d for 0 <= t < 2^31: with m = ceil(2^32 / d), umulhi(t, m) is t / d or one more (the
// error t (m - 2^32/d) / 2^32 < 1), corrected by one compare; d = 1: m = 0
__device__ __forceinline__ int div_magic(int t, uint32_t magic, int d) {
  if (!magic) return t;
  const int q = (int)__umulhi((uint32_t)t, magic);
  return q * d > t ? q - 1 : q;
}
// ... and that m for the geoms' *_magic fields (host)
inline uint32_t magic32(uint32_t d) { return d > 1 ? (uint32_t)((((uint64_t)1 << 32) + d - 1) / d) : 0u; }

__device__ __forceinline__ int sws_range(int v, int range) {
  if (range == 1) {  // |v| < 2^15: the 24-bit multiply is exact
    v = min(v, 30189);
    return (__mul24(v, 19077) - 39057361) >> 14;
  }
  if (range == 2) {
    v = min(v, 30775);
    return (__mul24(v, 4663) - 9289992) >> 12;
  }
  return v;
}

// hScale8To15 of one source row (taps = the `htaps` bytes at byte offset `off` of an LDS
// row), then range conversion.  Bytes are fetched as aligned dwords and funnel-shifted.
template <int HT, bool D4>  // HT 0: runtime htaps
__device__ __forceinline__ int hscale_lds(const uint32_t *row, int off, const int32_t *hcp, int htaps_rt,
                                          int range, int hs) {
  const int htaps = HT ? HT : htaps_rt;
  const uint32_t *q = row + (off >> 2);
  const uint32_t sh = (uint32_t)(off & 3) * 8;
  uint32_t lo = q[0];
  if (D4) {
    int ah = 0, al = 0;
    for (int k = 0; k < htaps; k += 4) {  // (HT > 0: unrolled by the compiler)
      const uint32_t hi = q[(k >> 2) + 1];
      const int w = (int)__builtin_amdgcn_alignbit(hi, lo, sh);  // taps k..k+3, int8 p - 128
      lo = hi;
      ah = __builtin_amdgcn_sdot4(w, hcp[k >> 1], ah, false);
      al = __builtin_amdgcn_sdot4(w, hcp[(k >> 1) + 1], al, false);
    }
    return sws_range(min(ah + (al >> 7) + hs, 32767), range);
  }
  int acc = 0;
  for (int k = 0; k < htaps; k += 4) {
    const uint32_t hi = q[(k >> 2) + 1];
    const uint32_t w = __builtin_amdgcn_alignbit(hi, lo, sh);  // taps k..k+3 (bytes, LE)
    lo = hi;
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, __builtin_amdgcn_perm(0u, w, 0x0c010c00u)),
                                 __builtin_bit_cast(short2_t, hcp[k >> 1]), acc, false);
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, __builtin_amdgcn_perm(0u, w, 0x0c030c02u)),
                                 __builtin_bit_cast(short2_t, hcp[(k >> 1) + 1]), acc, false);
  }
  return sws_range(min(acc >> 7, 32767), range);
}

typedef uint32_t u32_unaligned __attribute__((aligned(1)));

// HT / NPV: compile-time tap counts for the common filters (0 = runtime, any ratio); TH: tile
// height (64 only with HT 8, NPV 5)
template <int HT, int NPV, bool D4, int RANGE, int TH>  // RANGE: g.range as a compile-time value
__global__ __launch_bounds__(64 * scale_waves(TH)) void k_scale(const SegList src,  // the submit's input frames (kernels.hip)
                                               uint8_t *__restrict__ dst, ScaleGeom g,
                                               const int32_t *__restrict__ hcp,   // [dw][htaps/2]
                                               const int32_t *__restrict__ hp,    // [dw]
                                               const int32_t *__restrict__ vcp,   // [dh][npv]
                                               const int32_t *__restrict__ vps,   // [dh] pair start
                                               const int32_t *__restrict__ hsum,  // D4: [dw] sum of taps
                                               const int32_t *__restrict__ mfb) {  // matrix-core h-pass B fragments
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  constexpr int LPW = scale_loads_per_wave(TH), NWV = scale_waves(TH), NT = 64 * NWV;
  constexpr bool ALIAS = TH >= 64;
  static_assert(!ALIAS || (HT == 8 && NPV == 5), "64/128-row tiles: 2:1 filters only");
  // wave index as a uniform value: the v-pass rows (and their filter rows) are wave-uniform
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int t = blockIdx.x;  // the tile, raster order within a (plane, frame), then z
  if (ALIAS) {
    // XCD-contiguous tile order: workgroup i runs on XCD i % 8 (round-robin dispatch), so XCD
    // j takes the j-th eighth of the tiles in raster order and horizontally adjacent tiles --
    // whose windows share the 128-byte lines at their edges -- meet in the same L2
    const int i = t, n = gridDim.x, j = i & 7, q = n >> 3, r = n & 7;
    t = j * q + min(j, r) + (i >> 3);
  }
  const int z = div_magic(t, g.gxy_magic, g.gxy), rem = t - z * g.gxy;
  const int by = div_magic(rem, g.gx_magic, g.gx), bx = rem - by * g.gx;
  const int x0 = bx * kScaleTileW, y0 = by * TH;
  const int pl = z >= g.nf, f = z - (pl ? g.nf : 0);
  const uint8_t *s = seg_frame(src, f, g.s_fstride) + g.s_off + (pl ? g.s_poff : 0);
  uint8_t *d = dst + (size_t)f * g.d_fstride + g.d_off + (pl ? g.d_poff : 0);
  const int xe = min(x0 + kScaleTileW, g.dw), ye = min(y0 + TH, g.dh);
  const int p0 = vps[y0], p1 = vps[ye - 1] + g.npv;  // row pairs [p0, p1)
  const int nrows = 2 * (p1 - p0);
  const int npv = NPV ? NPV : g.npv;
  // source window: dwords [cb, cb + nw) of rows [2 p0, 2 p1) (rows clamped to the plane;
  // the rows past it only meet zero coefficients), staged with coalesced dword loads
  const int cb = hp[x0] & ~3;
  // +1: the funnel shift reads one past; rows padded to whole 16-byte pieces
  const int nw = ((((hp[xe - 1] + g.htaps - cb + 3) >> 2) + 1) + 3) & ~3;
  const int rs = ALIAS ? kScaleAliasWords : nw;  // LDS row stride (dwords)
  uint32_t *win = smem;                                       // [nrows][rs]
  // [p1 - p0][ps]: ALIAS, pair p over window rows 2p, 2p+1; else after the window
  const int ps = ALIAS ? 2 * rs : 64;
  uint32_t *pairs = ALIAS ? smem : smem + g.lds_win_words;
  uint32_t *vtab = smem + g.lds_win_words + g.lds_pairs * kScaleTileW;  // !ALIAS: [ye - y0][1 + npv]
  // ALIAS: wave w owns the row pairs [w ppw, (w + 1) ppw) of the window: it loads their rows
  // itself and runs their h-pass with no workgroup barrier in between (its own LDS stores and
  // loads are ordered), so the waves of a tile start computing as their own rows land
  const int np = p1 - p0, ppw = ALIAS ? (np + NWV - 1) / NWV : 0;
  const bool fast = nw <= 36 && g.sw >= 16 &&
                    (ALIAS ? 2 * ppw <= LPW * kScaleLoadRows : nrows <= NWV * LPW * kScaleLoadRows);
  const int rr = lane / 9, pc = lane - 9 * rr, col = cb + 16 * pc;  // fast loads: row, piece
  // The matrix-core h-pass (2:1 interior tiles): the window is loaded as on the VALU path, then
  // wave w computes column block w (16 output columns) of every 16-row block of the window as
  // v_mfma_i32_16x16x64_i8 products: A = 16 window rows x 64 bytes from the column block's
  // aligned byte 32 w (one ds_read_b128 per lane: lane l row l & 15, bytes 16 (l >> 4) .. +15),
  // B = the shared filter's hi / lo tap bytes on the band (host-built, the same k map), so D =
  // ah / al of hscale_lds for rows 4 (l >> 4) + i, column l & 15.  Every wave reads every row,
  // so the pairs are written over the window after a barrier.
  if (TH == 64 && D4 && HT == 8 && fast && bx >= g.mf_bx0 && bx < g.mf_bx1) {
    const int ppw2 = (p1 - p0 + NWV - 1) / NWV;  // the VALU path's row split for the loads
    u32x4 wv[LPW];
#pragma unroll
    for (int i = 0; i < LPW; i++) {
      const int r = 2 * ppw2 * wave + kScaleLoadRows * i + rr;
      const uint8_t *rp = s + (size_t)min(2 * p0 + r, g.sh - 1) * g.s_stride;
      if (col + 16 <= g.sw) {
        wv[i] = *(const u32x4_a1 *)(rp + col);
      } else {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int cc = col + 4 * k, lc = min(cc, g.sw - 4);
          w[k] = cc < g.sw ? *(const u32_unaligned *)(rp + lc) >> ((cc - lc) * 8) : 0u;
        }
        wv[i] = u32x4{w[0], w[1], w[2], w[3]};
      }
    }
    const u32x4 bhi = ((const u32x4 *)mfb)[2 * lane], blo = ((const u32x4 *)mfb)[2 * lane + 1];
#pragma unroll
    for (int i = 0; i < LPW; i++) {
      const int r = 2 * ppw2 * wave + kScaleLoadRows * i + rr;
      if (rr < kScaleLoadRows && r < nrows && 4 * pc < nw && kScaleLoadRows * i + rr < 2 * ppw2)
        *(u32x4 *)(win + r * rs + 4 * pc) = wv[i] ^ 0x80808080u;
    }
    __syncthreads();
    const int g4 = lane >> 4, n = lane & 15;
    constexpr int kMfBlocks = 9;  // 16-row blocks: >= the 136 rows of a 64-row tile
    uint32_t pk[kMfBlocks][2];
#pragma unroll
    for (int m = 0; m < kMfBlocks; m++) {
      pk[m][0] = pk[m][1] = 0u;
      if (16 * m < nrows) {
        const int row = min(16 * m + n, nrows - 1);
        const v4i av = __builtin_bit_cast(v4i, *(const u32x4 *)(win + row * rs + 8 * wave + 4 * g4)), z = {0, 0, 0, 0};
        const v4i hi = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, __builtin_bit_cast(v4i, bhi), z, 0, 0, 0);
        const v4i lo = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, __builtin_bit_cast(v4i, blo), z, 0, 0, 0);
        int h[4];
#pragma unroll
        for (int i = 0; i < 4; i++) h[i] = sws_range(min(hi[i] + (lo[i] >> 7) + g.mf_hs, 32767), RANGE);
        pk[m][0] = ((uint32_t)h[0] & 0xffffu) | ((uint32_t)h[1] << 16);
        pk[m][1] = ((uint32_t)h[2] & 0xffffu) | ((uint32_t)h[3] << 16);
      }
    }
    __syncthreads();  // every wave's window reads done: the pairs go over the rows
    if (by >= g.mv_by0 && by < g.mv_by1) {
      // The v-pass on the matrix cores as well (interior tile rows: one v filter, pos[y] = 2y + c).
      // With h = 256 hi + lo (hi: the int16's high byte as int8; lo its low byte, stored as
      // lo ^ 0x80 = lo - 128) and each tap f = 128 fh + fl (fl in [-64, 64)):
      //   sum h f = 32768 S1 + 128 X + S4 + 128 F,  S1 = sum hi fh,  X = sum hi (2 fl) + sum lo' fh,
      //   S4 = sum lo' fl  (F = the tap sum),
      // four v_mfma_i32_16x16x64_i8 per 16 x 16 block of outputs, every product exact in i32:
      // A = 64 plane bytes (window rows 32 rb ..) of 16 columns, B = the filter's band (host-built:
      // output row n of the block reads window rows 2n + delta + j), so D's lane (n, g4) holds
      // output row n, columns 4 g4 .. 4 g4 + 3 of the block.  Each wave writes the planes of the
      // columns it computed in the h-pass, then (after a barrier) takes row block rb = wave.
      uint8_t *phi = (uint8_t *)smem, *plo = phi + 64 * kPlaneStride;
      const int colw = 16 * wave + n;
#pragma unroll
      for (int m = 0; m < kMfBlocks; m++) {
        if (16 * m < nrows) {  // (rows past nrows repeat the last one: finite, met by zero taps)
          const uint32_t hw = __builtin_amdgcn_perm(pk[m][1], pk[m][0], 0x07050301u);
          const uint32_t lw = __builtin_amdgcn_perm(pk[m][1], pk[m][0], 0x06040200u) ^ 0x80808080u;
          *(uint32_t *)(phi + colw * kPlaneStride + 16 * m + 4 * g4) = hw;
          *(uint32_t *)(plo + colw * kPlaneStride + 16 * m + 4 * g4) = lw;
        }
      }
      const u32x4 *mva = (const u32x4 *)(mfb + kMvFragOff);
      const v4i bfh = __builtin_bit_cast(v4i, mva[lane]), bfl = __builtin_bit_cast(v4i, mva[64 + lane]),
                b2fl = __builtin_bit_cast(v4i, mva[128 + lane]);
      const v4i z = {0, 0, 0, 0}, kv = {g.mv_k, g.mv_k, g.mv_k, g.mv_k};
      __syncthreads();  // every column's planes written
      uint32_t W[4];  // W[cb]: output row n, columns 16 cb + 4 g4 .. + 3 (bytes)
#pragma unroll
      for (int cb = 0; cb < 4; cb++) {
        // rows 32 wave .. 32 wave + 63 of column 16 cb + n (the last block's reads run past the
        // column into the next one: bytes met by zero taps)
        const int off = (16 * cb + n) * kPlaneStride + 32 * wave + 16 * g4;
        const v4i ah = __builtin_bit_cast(v4i, *(const u32x4 *)(phi + off));
        const v4i al = __builtin_bit_cast(v4i, *(const u32x4 *)(plo + off));
        const v4i s1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bfh, z, 0, 0, 0);
        v4i x = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, b2fl, z, 0, 0, 0);
        x = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bfh, x, 0, 0, 0);
        const v4i s4 = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bfl, kv, 0, 0, 0);
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (uint32_t)min(max(((s1[i] << 15) + (x[i] << 7) + s4[i]) >> 19, 0), 255);
        W[cb] = __builtin_amdgcn_perm(v[1], v[0], 0x0c0c0400u) | __builtin_amdgcn_perm(v[3], v[2], 0x04000c0cu);
      }
      // 4 x 4 transpose of (cb, g4) across lanes n, n + 16, n + 32, n + 48: then lane (n, g4)
      // holds columns 16 g4 .. 16 g4 + 15 of row n, one 16-byte store (a wave: 16 full rows)
      auto swap32 = [](uint32_t &a_, uint32_t &b_) {
        const auto r = __builtin_amdgcn_permlane32_swap(a_, b_, false, false);
        a_ = r[0];
        b_ = r[1];
      };
      auto swap16 = [](uint32_t &a_, uint32_t &b_) {
        const auto r = __builtin_amdgcn_permlane16_swap(a_, b_, false, false);
        a_ = r[0];
        b_ = r[1];
      };
      swap32(W[0], W[2]);
      swap32(W[1], W[3]);
      swap16(W[0], W[1]);
      swap16(W[2], W[3]);
      // (d_stride = dw, or the wider canvas row under a pad, and the plane / frame offsets are any
      // byte count: a 501-wide chroma plane at an odd offset, so the store's type promises no
      // alignment; still one 16-byte store.  These tiles are whole: columns x0 .. x0 + 63 < dw)
      *(u32x4_a1 *)(d + (size_t)(y0 + 16 * wave + n) * g.d_stride + x0 + 16 * g4) = u32x4{W[0], W[1], W[2], W[3]};
      return;
    }
#pragma unroll
    for (int m = 0; m < kMfBlocks; m++) {
      const int pa = 8 * m + 2 * g4;  // the pairs of D rows 4 g4 .. 4 g4 + 3 of block m
      if (pa < np) pairs[pa * ps + 16 * wave + n] = pk[m][0];
      if (pa + 1 < np) pairs[(pa + 1) * ps + 16 * wave + n] = pk[m][1];
    }
  } else {
  // Every global load of the tile is issued before any is waited on: the window rows, this
  // lane's h filter (column x), and the tile's v filter rows (one entry per thread).
  // fast path: 16-byte pieces, 7 rows of 9 pieces per wave-instruction, 3 per wave (84 rows
  // of <= 144 bytes)
  u32x4 v[LPW];
  if (fast) {
#pragma unroll
    for (int i = 0; i < LPW; i++) {
      const int r = ALIAS ? 2 * ppw * wave + kScaleLoadRows * i + rr : kScaleLoadRows * (LPW * wave + i) + rr;
      const uint8_t *rp = s + (size_t)min(2 * p0 + r, g.sh - 1) * g.s_stride;
      if (col + 16 <= g.sw) {
        v[i] = *(const u32x4_a1 *)(rp + col);
      } else {  // the piece crosses the row end: dwords loaded in-row and shifted down (bytes
                // >= sw meet no tap)
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int cc = col + 4 * k, lc = min(cc, g.sw - 4);
          w[k] = cc < g.sw ? *(const u32_unaligned *)(rp + lc) >> ((cc - lc) * 8) : 0u;
        }
        v[i] = u32x4{w[0], w[1], w[2], w[3]};
      }
    }
  }
  const int x = min(x0 + lane, g.dw - 1);  // clamped: tail lanes redo the last column
  const int32_t *hc = hcp + (size_t)x * (g.htaps >> 1);
  int32_t hreg[HT ? HT / 2 : 8];  // HT taps (or up to 16 at runtime) in registers
#pragma unroll
  for (int k = 0; k < (HT ? HT / 2 : 8); k++) hreg[k] = (2 * k < g.htaps) ? hc[k] : 0;
  const int hpx = hp[x];
  const int hs = D4 ? hsum[x] : 0;
  // v filter rows staged in LDS (ALIAS: read per output row with scalar loads instead -- the
  // row is wave-uniform -- so the tile's LDS is the window alone: 8 workgroups per CU)
  const int nvt = ALIAS ? 0 : (ye - y0) * (npv + 1);
  uint32_t vt = 0;
  int vi = tid;
  if (vi < nvt) {
    const int yy = vi / (npv + 1), k = vi - yy * (npv + 1);
    vt = k == 0 ? (uint32_t)vps[y0 + yy] : (uint32_t)vcp[(size_t)(y0 + yy) * g.npv + (k - 1)];
  }
  if (fast) {
#pragma unroll
    for (int i = 0; i < LPW; i++) {
      const int r = ALIAS ? 2 * ppw * wave + kScaleLoadRows * i + rr : kScaleLoadRows * (LPW * wave + i) + rr;
      const u32x4 w = D4 ? v[i] ^ 0x80808080u : v[i];
      // (ALIAS: only this wave's rows -- a neighbour may already have its pairs over its own)
      if (rr < kScaleLoadRows && r < nrows && 4 * pc < nw && (!ALIAS || kScaleLoadRows * i + rr < 2 * ppw))
        *(u32x4 *)(win + r * rs + 4 * pc) = w;
    }
  } else {
    for (int i = tid; i < nrows * nw; i += NT) {
      const int r = i / nw, c = i - r * nw;  // (LDS word r * rs + c)
      const uint8_t *rp = s + (size_t)min(2 * p0 + r, g.sh - 1) * g.s_stride;
      const int cc = cb + 4 * c;
      uint32_t w = 0;
      for (int bb = 0; bb < 4; bb++)
        if (cc + bb < g.sw) w |= (uint32_t)rp[cc + bb] << (8 * bb);
      win[r * rs + c] = w ^ (D4 ? 0x80808080u : 0u);
    }
  }
#pragma unroll 1
  for (; vi < nvt; vi += NT) {  // (one pass unless npv > 7)
    if (vi != tid) {
      const int yy = vi / (npv + 1), k = vi - yy * (npv + 1);
      vt = k == 0 ? (uint32_t)vps[y0 + yy] : (uint32_t)vcp[(size_t)(y0 + yy) * g.npv + (k - 1)];
    }
    vtab[vi] = vt;
  }
  const int off = hpx - cb;
  if (!(ALIAS && fast)) __syncthreads();  // (uniform: the tile's geometry)
  const int pb = ALIAS ? ppw * wave : wave, pe = ALIAS ? min(pb + ppw, np) : np, pstep = ALIAS ? 1 : NWV;
#pragma unroll 2
  for (int p = pb; p < pe; p += pstep) {
    int a, b;
    if (HT || g.htaps <= 16) {
      a = hscale_lds<HT, D4>(win + (2 * p) * rs, off, hreg, g.htaps, RANGE, hs);
      b = hscale_lds<HT, D4>(win + (2 * p + 1) * rs, off, hreg, g.htaps, RANGE, hs);
    } else {
      a = hscale_lds<0, D4>(win + (2 * p) * rs, off, hc, g.htaps, RANGE, hs);
      b = hscale_lds<0, D4>(win + (2 * p + 1) * rs, off, hc, g.htaps, RANGE, hs);
    }
    pairs[p * ps + lane] = ((uint32_t)a & 0xffffu) | ((uint32_t)b << 16);
  }
  }  // (the VALU h-pass)
  __syncthreads();
  if (x0 + lane >= g.dw) return;
  for (int y = y0 + wave; y < ye; y += NWV) {
    const uint32_t *vr = vtab + (y - y0) * (npv + 1);  // uniform address: LDS broadcast
    const int32_t *vg = vcp + (size_t)y * npv;         // ALIAS: uniform address: scalar loads
    const uint32_t *cp = pairs + ((ALIAS ? vps[y] : (int)vr[0]) - p0) * ps + lane;
    int acc = 64 << 12;
#pragma unroll
    for (int k = 0; k < npv; k++)
      acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, cp[k * ps]),
                                   __builtin_bit_cast(short2_t, ALIAS ? (uint32_t)vg[k] : vr[1 + k]), acc, false);
    d[(size_t)y * g.d_stride + x0 + lane] = (uint8_t)min(max(acc >> 19, 0), 255);
  }
}

// k_scale_stream: the same arithmetic for the ratios whose tile window does not fit LDS (past
// about 4:1).  One workgroup (4 waves) = one strip of 64 output columns x one band
// of kStreamBand output rows of a (plane, frame).  It walks down the band's source row pairs
// [vps[y0], vps[ye - 1] + npv) in chunks of q.R rows, one barrier per chunk:
//   load:   the chunk's rows of the strip's byte window (dwords [cb, cb + q.rs) of each row, one
//           row stride for every strip) as 16-byte pieces at any alignment, thread t pieces
//           t, t + 256, ..: the LDS image is the pieces in order, chunk c in half c & 1 of a
//           double window.  Chunk c + 2 is issued (to registers) in iteration c and stored in
//           iteration c + 1, after that iteration's h-pass: a whole iteration hides the loads.
//           A piece that crosses the row end is gathered byte by byte inside the row.
//   h-pass: a wave takes row pairs of the chunk (R 16: four rows at once, each coefficient word
//           read once for the four), lane = output column, and writes the int16 pair into a
//           ring of q.rp pair rows: pair p in slot (p - p0) % rp.  The coefficients are staged
//           once per workgroup as [word][lane] (HCL) or, when a wide filter leaves no room,
//           read from the table in global memory.
//   v-pass: after the barrier, the output rows whose last pair is now in the ring (one ballot
//           over the band's pair starts, which a wave holds one per lane) go to the waves
//           round-robin: the filter row from LDS (q.vcl: the band's rows staged once) or by
//           scalar loads, npv ring rows of the lane's column, one byte stored per lane.
// rp >= npv + R: while a wave still reads the rows that chunk c completed (they start after pair
// e - R/2 - npv, e = the end of chunk c), another may write chunk c + 1's pairs [e, e + R/2), into
// slots that held pairs < e + R/2 - rp.
struct StreamGeom {
  int R;               // source rows per chunk: 16, 8, 4 or 2
  int rp;              // ring slots (row pairs)
  int rs;              // window row stride (dwords) = 4 npc
  int npc;             // 16-byte pieces per window row
  uint32_t npc_magic;  // ceil(2^32 / npc), 0 when npc == 1
  int vcl;             // 1: the band's v filter rows staged in LDS
};
constexpr int kStreamThreads = 256;
constexpr int kStreamMaxPieces = 4;  // pieces per thread and chunk (the host keeps R npc within it)
constexpr int kStreamBand = 64;

// hScale8To15 + range conversion of NR consecutive window rows for one output column: the
// arithmetic of hscale_lds<0, D4>, the coefficient words (stride hstr) read once for all rows
template <int NR, bool D4>
__device__ __forceinline__ void hscale_rows(const uint32_t *win, int rs, int off, const int32_t *hc, int hstr,
                                            int htaps, int range, int hs, int *out) {
  const uint32_t *q = win + (off >> 2);
  const uint32_t sh = (uint32_t)(off & 3) * 8;
  uint32_t lo[NR];
  int a0[NR], a1[NR];
#pragma unroll
  for (int r = 0; r < NR; r++) {
    lo[r] = q[r * rs];
    a0[r] = a1[r] = 0;
  }
#pragma unroll 2
  for (int k = 0; k < htaps; k += 4) {
    const int32_t c0 = hc[(k >> 1) * hstr], c1 = hc[((k >> 1) + 1) * hstr];
#pragma unroll
    for (int r = 0; r < NR; r++) {
      const uint32_t hi = q[r * rs + (k >> 2) + 1];
      const uint32_t w = __builtin_amdgcn_alignbit(hi, lo[r], sh);  // taps k..k+3
      lo[r] = hi;
      if (D4) {
        a0[r] = __builtin_amdgcn_sdot4((int)w, c0, a0[r], false);
        a1[r] = __builtin_amdgcn_sdot4((int)w, c1, a1[r], false);
      } else {
        a0[r] = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, __builtin_amdgcn_perm(0u, w, 0x0c010c00u)),
                                       __builtin_bit_cast(short2_t, c0), a0[r], false);
        a0[r] = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, __builtin_amdgcn_perm(0u, w, 0x0c030c02u)),
                                       __builtin_bit_cast(short2_t, c1), a0[r], false);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NR; r++)
    out[r] = sws_range(min(D4 ? a0[r] + (a1[r] >> 7) + hs : a0[r] >> 7, 32767), range);
}

template <bool D4, int RANGE, bool HCL>
__global__ __launch_bounds__(kStreamThreads) void k_scale_stream(const SegList src, uint8_t *__restrict__ dst,
                                                                 ScaleGeom g, StreamGeom q,
                                                                 const int32_t *__restrict__ hcp,    // [dw][htaps/2]
                                                                 const int32_t *__restrict__ hp,     // [dw]
                                                                 const int32_t *__restrict__ vcp,    // [dh][npv]
                                                                 const int32_t *__restrict__ vps,    // [dh]
                                                                 const int32_t *__restrict__ hsum) {  // D4: [dw]
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = blockIdx.x;  // strip, band, then (plane, frame): ScaleGeom's 1-D grid
  const int z = div_magic(t, g.gxy_magic, g.gxy), rem = t - z * g.gxy;
  const int by = div_magic(rem, g.gx_magic, g.gx), bx = rem - by * g.gx;
  const int x0 = bx * kScaleTileW, y0 = by * kStreamBand;
  const int pl = z >= g.nf, f = z - (pl ? g.nf : 0);
  const uint8_t *s = seg_frame(src, f, g.s_fstride) + g.s_off + (pl ? g.s_poff : 0);
  uint8_t *d = dst + (size_t)f * g.d_fstride + g.d_off + (pl ? g.d_poff : 0);
  const int xe = min(x0 + kScaleTileW, g.dw), ye = min(y0 + kStreamBand, g.dh);
  const int npv = g.npv, hw = g.htaps >> 1, R = q.R, hr = R >> 1, rs = q.rs, rp = q.rp;
  const int p0 = vps[y0], p1 = vps[ye - 1] + npv;  // row pairs [p0, p1)
  const int cb = hp[x0] & ~3;
  uint32_t *win = smem;                     // [2][R][rs]: chunk c in half c & 1
  uint32_t *ring = smem + 2 * R * rs;       // [rp][64]
  uint32_t *hcl = ring + rp * 64;           // HCL: [hw][64]
  uint32_t *vcl = hcl + (HCL ? 64 * hw : 0);  // q.vcl: the band's v filter rows, [ye - y0][npv]
  const int x = min(x0 + lane, g.dw - 1);  // clamped: tail lanes redo the last column
  const int off = hp[x] - cb;
  const int hs = D4 ? hsum[x] : 0;
  const int vpl = vps[min(y0 + lane, ye - 1)];  // the band's pair starts, row y0 + lane (a band: 64 rows)
  if (HCL)
    for (int i = tid; i < 64 * hw; i += kStreamThreads)
      hcl[i] = (uint32_t)hcp[(size_t)min(x0 + (i & 63), g.dw - 1) * hw + (i >> 6)];
  if (q.vcl)
    for (int i = tid; i < (ye - y0) * npv; i += kStreamThreads) vcl[i] = (uint32_t)vcp[(size_t)y0 * npv + i];
  const int32_t *hc = HCL ? (const int32_t *)hcl + lane : hcp + (size_t)x * hw;
  const int hstr = HCL ? 64 : 1;
  const int npieces = R * q.npc;
  u32x4 v[kStreamMaxPieces];
  // the pieces of the chunk that starts at row pair pc (rows clamped to the plane: the rows past
  // it only meet zero coefficients, as do the bytes past the row end, staged as zeros)
  auto load_chunk = [&](int pc) {
#pragma unroll
    for (int i = 0; i < kStreamMaxPieces; i++) {
      const int idx = tid + kStreamThreads * i;
      v[i] = u32x4{0, 0, 0, 0};
      if (idx < npieces) {
        const int r = div_magic(idx, q.npc_magic, q.npc), col = cb + 16 * (idx - r * q.npc);
        const uint8_t *rpn = s + (size_t)min(2 * pc + r, g.sh - 1) * g.s_stride;
        if (col + 16 <= g.sw) {
          v[i] = *(const u32x4_a1 *)(rpn + col);
        } else if (col < g.sw) {  // the piece crosses the row end: its bytes inside the row only
          // (a rolled loop: at most one piece per row takes it, and sixteen predicated byte
          // loads per piece and call site would be most of the kernel's code)
          uint64_t wl = 0, wh = 0;
#pragma unroll 1
          for (int b = 0; b < min(g.sw - col, 8); b++) wl |= (uint64_t)rpn[col + b] << (8 * b);
#pragma unroll 1
          for (int b = 8; b < g.sw - col; b++) wh |= (uint64_t)rpn[col + b] << (8 * (b - 8));
          v[i] = u32x4{(uint32_t)wl, (uint32_t)(wl >> 32), (uint32_t)wh, (uint32_t)(wh >> 32)};
        }
      }
    }
  };
  auto store_chunk = [&](int half) {
#pragma unroll
    for (int i = 0; i < kStreamMaxPieces; i++) {
      const int idx = tid + kStreamThreads * i;
      if (idx < npieces) *(u32x4 *)(win + half * R * rs + 4 * idx) = D4 ? v[i] ^ 0x80808080u : v[i];
    }
  };
  load_chunk(p0);
  store_chunk(0);
  if (p0 + hr < p1) load_chunk(p0 + hr);
  __syncthreads();
  int ynext = y0, sb = 0, half = 0;  // the first row not yet written; the chunk's first ring slot
  for (int pc = p0; pc < p1; pc += hr) {
    const int pend = pc + hr;
    const uint32_t *wc = win + half * R * rs;
    if (R == 16) {
      int h[4];
      hscale_rows<4, D4>(wc + 4 * wave * rs, rs, off, hc, hstr, g.htaps, RANGE, hs, h);
      int sl = sb + 2 * wave;
      sl -= sl >= rp ? rp : 0;
      ring[sl * 64 + lane] = ((uint32_t)h[0] & 0xffffu) | ((uint32_t)h[1] << 16);
      sl = sl + 1 == rp ? 0 : sl + 1;
      ring[sl * 64 + lane] = ((uint32_t)h[2] & 0xffffu) | ((uint32_t)h[3] << 16);
    } else {
      for (int i = wave; i < hr; i += kStreamThreads / 64) {
        int h[2];
        hscale_rows<2, D4>(wc + 2 * i * rs, rs, off, hc, hstr, g.htaps, RANGE, hs, h);
        int sl = sb + i;
        sl -= sl >= rp ? rp : 0;
        ring[sl * 64 + lane] = ((uint32_t)h[0] & 0xffffu) | ((uint32_t)h[1] << 16);
      }
    }
    // the next chunk (loaded a whole iteration ago) into the other half, then the one after it
    // into the registers: one barrier per chunk orders the window halves and the ring
    if (pend < p1) {
      store_chunk(half ^ 1);
      if (pend + hr < p1) load_chunk(pend + hr);
    }
    __syncthreads();
    // the rows this chunk completes: [ynext, yr) (vps is monotone: a prefix of the lanes)
    const int yr = y0 + __popcll(__ballot(y0 + lane < ye && vpl + npv <= pend));
    for (int y = ynext + wave; y < yr; y += kStreamThreads / 64) {
      const int yb = __builtin_amdgcn_readfirstlane(y - y0);
      // vps[y] > pc - npv (the row was not complete before this chunk), < pc + R/2
      int sl = sb + (__builtin_amdgcn_readlane(vpl, yb) - pc);
      sl += sl < 0 ? rp : 0;
      sl -= sl >= rp ? rp : 0;
      int acc = 64 << 12;
      if (q.vcl) {
        const uint32_t *vr = vcl + yb * npv;  // uniform address: LDS broadcast
        for (int k = 0; k < npv; k++) {
          acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, ring[sl * 64 + lane]),
                                       __builtin_bit_cast(short2_t, vr[k]), acc, false);
          sl = sl + 1 == rp ? 0 : sl + 1;
        }
      } else {
        const int32_t *vg = vcp + (size_t)(y0 + yb) * npv;  // uniform address: scalar loads
        for (int k = 0; k < npv; k++) {
          acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, ring[sl * 64 + lane]),
                                       __builtin_bit_cast(short2_t, vg[k]), acc, false);
          sl = sl + 1 == rp ? 0 : sl + 1;
        }
      }
      if (x0 + lane < xe) d[(size_t)y * g.d_stride + x0 + lane] = (uint8_t)min(max(acc >> 19, 0), 255);
    }
    ynext = yr;
    sb += hr;
    sb -= sb >= rp ? rp : 0;
    half ^= 1;
  }
}

// A plane the sws stage leaves at its size (sw == dw, sh == dh: luma of a pure -pix_fmt
// conversion, 4:4:4 -> yuvj420p).  swscale still runs it through the 15-bit intermediate with
// one-tap identity filters (16384, 4096): per byte p
//   clip_u8(((64 << 12) + 4096 range(p << 7)) >> 19)
// which is p itself without a range conversion, and else a function of the byte alone: a
// 256-entry table in LDS, built here with k_scale's own sws_range.  The plane's rows are
// contiguous on both sides (strides = widths), so it is one byte string per (plane, frame):
// streamed as 16-byte pieces aligned on the destination (d_scaled; the frames there are
// enc_frame_bytes apart and the plane offsets any byte count), loaded from the source at
// whatever alignment that leaves (frames in_frame_bytes apart, a caller's device pointer),
// with the bytes before the first and after the last whole piece copied one by one by the
// (plane, frame)'s first workgroup.  ScaleGeom as for k_scale (sizes, offsets, nf, range);
// gxy = workgroups per (plane, frame), each kCopyThreads x kCopyVecs pieces.
// RECT (a cropped source): the plane is a rectangle of wider rows, sw bytes of
// every s_stride, and the destination the same byte string as before.  Byte j of it is column
// j % sw of row j / sw (multiply-high, div_magic: j < 2^28); a piece inside one source row is
// still one unaligned 16-byte load, a piece that runs over a row end is gathered byte by byte
// (16 / sw of the pieces).  The loads of all of a thread's pieces, gathered ones included, are
// issued before its first store.  The context launches RECT only when s_stride != sw.
constexpr int kCopyThreads = 256;  // = the table's entries
constexpr int kCopyVecs = 4;       // pieces per thread, all loaded before the first is stored
template <int RANGE, bool RECT = false>
__global__ __launch_bounds__(kCopyThreads) void k_plane_copy(const SegList src, uint8_t *__restrict__ dst,
                                                             ScaleGeom g) {
  __shared__ __attribute__((aligned(16))) uint8_t tab[256];
  const int tid = threadIdx.x;
  if (RANGE) {
    const int h = sws_range(tid << 7, RANGE);  // (255 << 7 < 32767: hScale8To15's clip never acts)
    tab[tid] = (uint8_t)min(max(((64 << 12) + h * 4096) >> 19, 0), 255);
    __syncthreads();
  }
  const int t = blockIdx.x;
  const int z = div_magic(t, g.gxy_magic, g.gxy), blk = t - z * g.gxy;
  const int pl = z >= g.nf, f = z - (pl ? g.nf : 0);
  const uint8_t *s = seg_frame(src, f, g.s_fstride) + g.s_off + (pl ? g.s_poff : 0);
  uint8_t *d = dst + (size_t)f * g.d_fstride + g.d_off + (pl ? g.d_poff : 0);
  const size_t nb = (size_t)g.sw * (size_t)g.sh;
  const size_t head = min((size_t)(-(uintptr_t)d & 15), nb);
  const size_t nv = (nb - head) >> 4;  // whole pieces: bytes [head, head + 16 nv) of the plane
  auto conv = [&](uint32_t w) -> uint32_t {
    if (!RANGE) return w;
    return (uint32_t)tab[w & 255u] | ((uint32_t)tab[(w >> 8) & 255u] << 8) |
           ((uint32_t)tab[(w >> 16) & 255u] << 16) | ((uint32_t)tab[w >> 24] << 24);
  };
  // the 16 source bytes of the piece at byte j of the plane (RECT: j < nb - 15 < 2^28)
  auto piece = [&](size_t j) -> u32x4 {
    if (!RECT) return *(const u32x4_a1 *)(s + j);
    int row = div_magic((int)j, g.sw_magic, g.sw), col = (int)j - row * g.sw;
    const uint8_t *rp = s + (size_t)row * g.s_stride;
    if (col + 16 <= g.sw) return *(const u32x4_a1 *)(rp + col);
    u32x4 w = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
      if (col >= g.sw) {  // (sw >= 1: at most one row step per byte)
        col = 0;
        rp += g.s_stride;
      }
      w[i >> 2] |= (uint32_t)rp[col++] << (8 * (i & 3));
    }
    return w;
  };
  auto byte_at = [&](size_t j) -> uint8_t {  // one source byte (the head and the tail)
    if (!RECT) return s[j];
    const int row = div_magic((int)j, g.sw_magic, g.sw);
    return s[(size_t)row * g.s_stride + ((int)j - row * g.sw)];
  };
  const size_t k0 = (size_t)blk * (kCopyThreads * kCopyVecs) + tid;
  u32x4 v[kCopyVecs];
#pragma unroll
  for (int i = 0; i < kCopyVecs; i++) {
    const size_t k = k0 + (size_t)i * kCopyThreads;
    v[i] = k < nv ? piece(head + 16 * k) : u32x4{0, 0, 0, 0};
  }
#pragma unroll
  for (int i = 0; i < kCopyVecs; i++) {
    const size_t k = k0 + (size_t)i * kCopyThreads;
    if (k < nv)
      *(u32x4 *)(d + head + 16 * k) = u32x4{conv(v[i][0]), conv(v[i][1]), conv(v[i][2]), conv(v[i][3])};
  }
  if (blk == 0 && tid < 16) {
    const size_t a = (size_t)tid, b = head + 16 * nv + (size_t)tid;
    if (a < head) d[a] = RANGE ? tab[byte_at(a)] : byte_at(a);
    if (b < nb) d[b] = RANGE ? tab[byte_at(b)] : byte_at(b);
  }
}

// k_pad_plane: `-vf pad`.  The encoder's input is a canvas of q.cw x q.ch bytes
// per plane with the picture (g.dw x g.dh: the sws stage's output plane) at column q.px, row
// q.py and a constant byte (q.fill: 0 luma, 128 chroma) everywhere else.  Destination-driven as
// k_plane_copy: the canvas plane of a (plane, frame) is one byte string (rows at their width),
// cut into 16-byte pieces aligned on the destination; piece k covers bytes [head + 16 k, + 16),
// byte j is column j % cw of row j / cw (multiply-high, div_magic: j < 2^28).  ScaleGeom as for
// k_plane_copy (the source rectangle: sw, sh, s_stride, s_off, s_fstride, s_poff; nf, gxy) with
// d_off / d_poff the canvas plane's offset in a frame and the next plane's from it.
//   COPY (the plane keeps its size: the picture comes straight from the source rectangle, through
//   the tv->pc byte table of k_plane_copy): a piece inside one picture row is one unaligned
//   16-byte load, a piece in the border the constant, any other piece is put together byte by
//   byte (picture bytes loaded, the rest constant); every piece is then one aligned 16-byte
//   store, after all of the thread's loads.
//   !COPY (k_scale / k_scale_stream write the picture into the canvas, d_stride = cw): no loads.
//   Pieces inside the picture are skipped, pieces in the border are one 16-byte store, the others
//   store their border bytes one by one and touch no picture byte, so the launch order of the
//   two kernels does not matter.
// The up to 15 bytes before the first and after the last whole piece go byte by byte in the
// (plane, frame)'s first workgroup.
struct PadGeom {
  int cw, ch;         // canvas plane size
  uint32_t cw_magic;  // ceil(2^32 / cw), 0 when cw == 1
  int px, py;         // the picture's first column and row in the canvas plane
  int fill;           // the border byte
};

template <int RANGE, bool COPY>
__global__ __launch_bounds__(kCopyThreads) void k_pad_plane(const SegList src, uint8_t *__restrict__ dst,
                                                            ScaleGeom g, PadGeom q) {
  __shared__ __attribute__((aligned(16))) uint8_t tab[256];
  const int tid = threadIdx.x;
  if (COPY && RANGE) {
    const int h = sws_range(tid << 7, RANGE);
    tab[tid] = (uint8_t)min(max(((64 << 12) + h * 4096) >> 19, 0), 255);
    __syncthreads();
  }
  const int t = blockIdx.x;
  const int z = div_magic(t, g.gxy_magic, g.gxy), blk = t - z * g.gxy;
  const int pl = z >= g.nf, f = z - (pl ? g.nf : 0);
  const uint8_t *s = COPY ? seg_frame(src, f, g.s_fstride) + g.s_off + (pl ? g.s_poff : 0) : nullptr;
  uint8_t *d = dst + (size_t)f * g.d_fstride + g.d_off + (pl ? g.d_poff : 0);
  const int nb = q.cw * q.ch;  // < 2^28 (16384 x 16384)
  const int head = min((int)(-(uintptr_t)d & 15), nb);
  const int nv = (nb - head) >> 4;
  const int pxe = q.px + g.dw, pye = q.py + g.dh;  // the picture's end column and row (COPY: dw = sw, dh = sh)
  const uint32_t fw = (uint32_t)q.fill * 0x01010101u;
  auto conv1 = [&](uint32_t b) -> uint32_t { return RANGE ? (uint32_t)tab[b] : b; };
  auto conv = [&](uint32_t w) -> uint32_t {
    if (!RANGE) return w;
    return (uint32_t)tab[w & 255u] | ((uint32_t)tab[(w >> 8) & 255u] << 8) |
           ((uint32_t)tab[(w >> 16) & 255u] << 16) | ((uint32_t)tab[w >> 24] << 24);
  };
  auto in_pic = [&](int row, int col) -> bool { return row >= q.py && row < pye && col >= q.px && col < pxe; };
  // piece kinds: 0 inside the picture (COPY: v holds its source bytes, to convert), 1 border,
  // 2 mixed (COPY: v holds the final bytes)
  const int k0 = blk * (kCopyThreads * kCopyVecs) + tid;
  u32x4 v[kCopyVecs];
  int kind[kCopyVecs], prow[kCopyVecs], pcol[kCopyVecs];
#pragma unroll
  for (int i = 0; i < kCopyVecs; i++) {
    const int k = k0 + i * kCopyThreads;
    v[i] = u32x4{fw, fw, fw, fw};
    kind[i] = 1;
    prow[i] = pcol[i] = 0;
    if (k < nv) {
      const int j = head + 16 * k;
      const int r0 = div_magic(j, q.cw_magic, q.cw), c0 = j - r0 * q.cw;
      const int r1 = div_magic(j + 15, q.cw_magic, q.cw);
      prow[i] = r0;
      pcol[i] = c0;
      if (r1 < q.py || r0 >= pye || (r0 == r1 && (c0 + 16 <= q.px || c0 >= pxe))) {
        kind[i] = 1;
      } else if (r0 == r1 && c0 >= q.px && c0 + 16 <= pxe) {
        kind[i] = 0;
        if (COPY) v[i] = *(const u32x4_a1 *)(s + (size_t)(r0 - q.py) * g.s_stride + (c0 - q.px));
      } else {
        kind[i] = 2;
        if (COPY) {  // (rolled: a few pieces per row take it)
          uint64_t wl = 0, wh = 0;
          int row = r0, col = c0;
#pragma unroll 1
          for (int b = 0; b < 16; b++) {
            if (col >= q.cw) {  // (cw >= 1: at most one row step per byte)
              col = 0;
              row++;
            }
            const uint64_t x = in_pic(row, col)
                                   ? conv1(s[(size_t)(row - q.py) * g.s_stride + (col - q.px)])
                                   : (uint32_t)q.fill;
            if (b < 8) wl |= x << (8 * b);
            else wh |= x << (8 * (b - 8));
            col++;
          }
          v[i] = u32x4{(uint32_t)wl, (uint32_t)(wl >> 32), (uint32_t)wh, (uint32_t)(wh >> 32)};
        }
      }
    }
  }
  // the head and tail bytes (first workgroup): loaded here, stored last
  const bool edge = blk == 0 && tid < 16;
  const int ja = tid, jb = head + 16 * nv + tid;
  bool wa = false, wb = false;
  uint32_t va = (uint32_t)q.fill, vb = (uint32_t)q.fill;
  if (edge) {
    if (ja < head) {
      const int row = div_magic(ja, q.cw_magic, q.cw), col = ja - row * q.cw;
      const bool in = in_pic(row, col);
      wa = COPY || !in;
      if (COPY && in) va = conv1(s[(size_t)(row - q.py) * g.s_stride + (col - q.px)]);
    }
    if (jb < nb) {
      const int row = div_magic(jb, q.cw_magic, q.cw), col = jb - row * q.cw;
      const bool in = in_pic(row, col);
      wb = COPY || !in;
      if (COPY && in) vb = conv1(s[(size_t)(row - q.py) * g.s_stride + (col - q.px)]);
    }
  }
#pragma unroll
  for (int i = 0; i < kCopyVecs; i++) {
    const int k = k0 + i * kCopyThreads;
    if (k >= nv) continue;
    uint8_t *dp = d + head + 16 * (size_t)k;
    if (kind[i] == 1 || (COPY && kind[i] == 2)) {
      *(u32x4 *)dp = v[i];
    } else if (kind[i] == 0) {
      if (COPY) *(u32x4 *)dp = u32x4{conv(v[i][0]), conv(v[i][1]), conv(v[i][2]), conv(v[i][3])};
    } else {  // !COPY, mixed: the border bytes only
      int row = prow[i], col = pcol[i];
#pragma unroll 1
      for (int b = 0; b < 16; b++) {
        if (col >= q.cw) {
          col = 0;
          row++;
        }
        if (!in_pic(row, col)) dp[b] = (uint8_t)q.fill;
        col++;
      }
    }
  }
  if (wa) d[ja] = (uint8_t)va;
  if (wb) d[jb] = (uint8_t)vb;
}

// k_orient_plane: `-vf hflip / vflip / transpose`, the first filter of the chain.
// Every plane P (sw x sh) of the decoded frame becomes
//   out[y][x] = in'[FY ? H - 1 - y : y][FX ? W - 1 - x : x],  in' = T ? transpose(P) : P  (W x H)
// in a packed planar frame of the same byte count (the slot's d_orient), the bytes unchanged (no
// range conversion: that stays with the sws stage or k_encode).  The source is the submit's
// SegList (whole frames at any byte alignment), the destination one buffer; U and V go in one
// launch (blockIdx >= gxy * nf is V, at s_poff / d_poff).  T and FX are template arguments, FY a
// run-time flag.
//   T = 0: a streaming copy as k_plane_copy's: the output plane of a (plane, frame) is one byte
//   string cut into 16-byte pieces aligned on the destination; piece k covers bytes [head + 16 k,
//   + 16), byte j is column j % sw of row j / sw (multiply-high, div_magic: j < 2^28).  A piece
//   inside one output row is one unaligned 16-byte load from source row (FY ? sh - 1 - row : row)
//   at column col (FX: at sw - 16 - col, the 16 bytes reversed in registers: the dwords swapped
//   and each byte-swapped); a piece that runs over a row end is gathered byte by byte (16 / sw of
//   the pieces).  Head and tail bytes go singly in the (plane, frame)'s first workgroup.
//   T = 1: a tiled byte transpose without LDS.  A wave takes a tile of 128 rows x 64 columns of
//   the source plane; lane (lr = lane & 15, lc = lane >> 4) loads 16 bytes of each of the source
//   rows 8 lr .. 8 lr + 7 at tile column 16 lc (every load instruction covers 16 rows x 64
//   contiguous bytes), transposes its eight 4 x 4 byte blocks with v_perm_b32 and stores 16 dword
//   pairs: pair m holds source column 16 lc + m of its eight rows, i.e. eight consecutive bytes of
//   output row (FY ? sw - 1 - col : col) at output column 8 lr (FX: sh - 8 - 8 lr, the eight bytes
//   reversed: by the selectors inside a dword, and the dwords swapped); every store instruction
//   covers 4 output rows x 128 contiguous bytes.  (Four rows per lane and 64-byte row pieces
//   measured 14% slower: half of its write requests were partial lines)  The
//   stores land at whatever alignment the plane offset and the output width sh leave.  A lane
//   whose 8 x 16 block is not whole inside the plane (the partial tiles of a plane whose sizes
//   are no multiples of the tile) moves its bytes one by one and reads nothing past the plane.
struct OrientGeom {
  int sw, sh;                      // the source plane (the output plane: sw x sh, T: sh x sw)
  long long s_off, d_off;          // the plane's offset inside a source / an oriented frame
  long long s_fstride, d_fstride;  // frame strides
  long long s_poff, d_poff;        // the next plane's offset from this one (V from U)
  int nf;                          // frames per plane
  int fy;                          // FY
  uint32_t sw_magic;               // T = 0: ceil(2^32 / sw), 0 when sw == 1
  int tx;                          // T = 1: tile columns, ceil(sw / kOrientTile), and the plane's tiles
  int ntiles;
  uint32_t tx_magic;
  int gxy;                         // workgroups per (plane, frame)
  uint32_t gxy_magic;
};

constexpr int kOrientTile = 64;     // T = 1: source columns per tile
constexpr int kOrientWaves = kCopyThreads / 64;  // T = 1: tiles per workgroup
constexpr int kOrientTileH = 128;  // T = 1: source rows per tile (the tile: kOrientTileH rows x kOrientTile columns)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_a1 __attribute__((aligned(1)));  // output rows start at any byte

__device__ __forceinline__ uint32_t reverse_bytes(uint32_t w) { return __builtin_bswap32(w); }

template <bool T, bool FX>
__global__ __launch_bounds__(kCopyThreads) void k_orient_plane(const SegList src, uint8_t *__restrict__ dst,
                                                               OrientGeom g) {
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  const int z = div_magic(t, g.gxy_magic, g.gxy), blk = t - z * g.gxy;
  const int pl = z >= g.nf, f = z - (pl ? g.nf : 0);
  const uint8_t *s = seg_frame(src, f, g.s_fstride) + g.s_off + (pl ? g.s_poff : 0);
  uint8_t *d = dst + (size_t)f * g.d_fstride + g.d_off + (pl ? g.d_poff : 0);
  const int sw = g.sw, sh = g.sh;
  if (!T) {
    const int nb = sw * sh;  // < 2^28 (16384 x 16384)
    const int head = min((int)(-(uintptr_t)d & 15), nb);
    const int nv = (nb - head) >> 4;
    // the source byte of output byte (row, col)
    auto byte_at = [&](int j) -> uint8_t {
      const int row = div_magic(j, g.sw_magic, sw), col = j - row * sw;
      return s[(size_t)(g.fy ? sh - 1 - row : row) * sw + (FX ? sw - 1 - col : col)];
    };
    auto piece = [&](int j) -> u32x4 {
      const int row = div_magic(j, g.sw_magic, sw), col = j - row * sw;
      if (col + 16 <= sw) {
        const uint8_t *rp = s + (size_t)(g.fy ? sh - 1 - row : row) * sw;
        if (!FX) return *(const u32x4_a1 *)(rp + col);
        const u32x4 w = *(const u32x4_a1 *)(rp + (sw - 16 - col));
        return u32x4{reverse_bytes(w[3]), reverse_bytes(w[2]), reverse_bytes(w[1]), reverse_bytes(w[0])};
      }
      uint64_t wl = 0, wh = 0;  // (rolled: 16 / sw of the pieces take it)
#pragma unroll 1
      for (int b = 0; b < 16; b++) {
        const uint64_t x = byte_at(j + b);
        if (b < 8) wl |= x << (8 * b);
        else wh |= x << (8 * (b - 8));
      }
      return u32x4{(uint32_t)wl, (uint32_t)(wl >> 32), (uint32_t)wh, (uint32_t)(wh >> 32)};
    };
    const int k0 = blk * (kCopyThreads * kCopyVecs) + tid;
    u32x4 v[kCopyVecs];
#pragma unroll
    for (int i = 0; i < kCopyVecs; i++) {
      const int k = k0 + i * kCopyThreads;
      v[i] = k < nv ? piece(head + 16 * k) : u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < kCopyVecs; i++) {
      const int k = k0 + i * kCopyThreads;
      if (k < nv) *(u32x4 *)(d + head + 16 * (size_t)k) = v[i];
    }
    if (blk == 0 && tid < 16) {
      const int a = tid, b = head + 16 * nv + tid;
      if (a < head) d[a] = byte_at(a);
      if (b < nb) d[b] = byte_at(b);
    }
  } else {
    const int tile = blk * kOrientWaves + (tid >> 6);
    if (tile >= g.ntiles) return;
    const int ty = div_magic(tile, g.tx_magic, g.tx), txi = tile - ty * g.tx;
    const int lane = tid & 63, lr = lane & 15, lc = lane >> 4;
    const int r0 = ty * kOrientTileH + 8 * lr, c0 = txi * kOrientTile + 16 * lc;  // the lane's 8 x 16 source block
    if (r0 >= sh || c0 >= sw) return;
    // output row of source column c, output column of source row r (the output rows are sh wide)
    auto orow = [&](int c) -> size_t { return (size_t)(g.fy ? sw - 1 - c : c) * sh; };
    if (r0 + 8 <= sh && c0 + 16 <= sw) {
      u32x4 w[8];
#pragma unroll
      for (int k = 0; k < 8; k++) w[k] = *(const u32x4_a1 *)(s + (size_t)(r0 + k) * sw + c0);
      const int oc = FX ? sh - 8 - r0 : r0;
#pragma unroll
      for (int q = 0; q < 4; q++) {  // the two 4 x 4 blocks at columns 4 q: rows a, b, c, e of each
        uint32_t o[2][4];
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const uint32_t a = w[4 * h][q], b = w[4 * h + 1][q], c = w[4 * h + 2][q], e = w[4 * h + 3][q];
          // (v_perm_b32: selector bytes 0..3 pick from the second operand, 4..7 from the first)
          const uint32_t ab_lo = __builtin_amdgcn_perm(b, a, FX ? 0x01050004u : 0x05010400u);  // a0 b0 a1 b1 (FX: b0 a0 b1 a1)
          const uint32_t ab_hi = __builtin_amdgcn_perm(b, a, FX ? 0x03070206u : 0x07030602u);  // a2 b2 a3 b3
          const uint32_t ce_lo = __builtin_amdgcn_perm(e, c, FX ? 0x01050004u : 0x05010400u);
          const uint32_t ce_hi = __builtin_amdgcn_perm(e, c, FX ? 0x03070206u : 0x07030602u);
          // column j of the block: bytes a_j b_j c_j e_j (FX: e_j c_j b_j a_j)
          if (!FX) {
            o[h][0] = __builtin_amdgcn_perm(ce_lo, ab_lo, 0x05040100u);
            o[h][1] = __builtin_amdgcn_perm(ce_lo, ab_lo, 0x07060302u);
            o[h][2] = __builtin_amdgcn_perm(ce_hi, ab_hi, 0x05040100u);
            o[h][3] = __builtin_amdgcn_perm(ce_hi, ab_hi, 0x07060302u);
          } else {
            o[h][0] = __builtin_amdgcn_perm(ab_lo, ce_lo, 0x05040100u);
            o[h][1] = __builtin_amdgcn_perm(ab_lo, ce_lo, 0x07060302u);
            o[h][2] = __builtin_amdgcn_perm(ab_hi, ce_hi, 0x05040100u);
            o[h][3] = __builtin_amdgcn_perm(ab_hi, ce_hi, 0x07060302u);
          }
        }
        // eight output bytes per source column (FX: the rows 4..7 block first)
#pragma unroll
        for (int j = 0; j < 4; j++)
          *(u32x2_a1 *)(d + orow(c0 + 4 * q + j) + oc) = u32x2{o[FX ? 1 : 0][j], o[FX ? 0 : 1][j]};
      }
    } else {  // a partial block at the plane's right or bottom edge: byte by byte, inside the plane
      const int nr = min(8, sh - r0), nc = min(16, sw - c0);
#pragma unroll 1
      for (int k = 0; k < nr; k++)
#pragma unroll 1
        for (int j = 0; j < nc; j++)
          d[orow(c0 + j) + (FX ? sh - 1 - (r0 + k) : r0 + k)] = s[(size_t)(r0 + k) * sw + c0 + j];
    }
  }
}

// k_yadif_plane: `-vf yadif`, modes 0 (send_frame) and 2 (send_frame_nospatial), deint=all (DESIGN
// §4.13), in front of every other filter.  Every plane (w x h, rows at their width, the chroma
// planes as planes of their own) of frame i of a sequence becomes, with prev = frame max(i - 1,
// first), cur = frame i, next = frame min(i + 1, last) and prev2 = prev, next2 = cur:
//   rows with (y ^ parity) & 1 == 0: cur's bytes;
//   the other rows, per byte x, in C int arithmetic (ym = y ? y - 1 : y + 1, yp = y + 1 < h ? y + 1
//   : y - 1, y2m = y ? y - 2 : y + 2, y2p = y + 1 < h ? y + 2 : y - 2; A = cur[ym], B = cur[yp]):
//     c = A[x], e = B[x], d = (prev2[y][x] + next2[y][x]) >> 1
//     diff = max(|prev2[y][x] - next2[y][x]| >> 1, (|prev[ym][x] - c| + |prev[yp][x] - e|) >> 1,
//                (|next[ym][x] - c| + |next[yp][x] - e|) >> 1)
//     sp = (c + e) >> 1; for 3 <= x < w - 3 the edge-directed search: with S(j) = |A[x-1+j] -
//     B[x-1-j]| + |A[x+j] - B[x-j]| + |A[x+1+j] - B[x+1-j]| and score = S(0) - 1, for s = -1 and then
//     s = +1 (against the score the first left): S(s) < score takes score = S(s), sp = (A[x+s] +
//     B[x-s]) >> 1, and then S(2s) < score takes that one in the same way
//     unless NOSPATIAL or y == 1 or y + 2 == h: b = (prev2[y2m][x] + next2[y2m][x]) >> 1, f the same
//     at y2p; diff = max(diff, min(d - e, d - c, max(b - c, f - e)), -max(d - e, d - c, min(b - c, f - e)))
//     out = clip(sp, d - diff, d + diff)
// into a packed planar frame of the same byte count (the slot's d_deint), no range conversion.
// Every row index above is inside the plane for h >= 3 except y2m / y2p of the rows y == 1 and
// y + 2 == h, which the formula does not use: they are replaced by y before any address is made.
// The frames come from the submit's SegList; a segment is a sequence of its own, and g.lo / g.hi
// give per segment the first and last frame that may be read, counted from the segment's first
// encoded frame (0 and n - 1; -1 / n with a halo frame in front of / behind them, mjg_submit_halo):
// the neighbour indices are clamped to them, so a missing neighbour is cur itself.
// Layout: as k_plane_copy, the output plane of a (plane, frame) is one byte string cut into 16-byte
// pieces aligned on the destination, one piece per thread; piece k covers bytes [head + 16 k, + 16),
// byte j is column j % w of row j / w (multiply-high: j < 2^28).  A piece inside one kept row is one
// unaligned 16-byte load and one store.  A piece inside one interpolated row takes twelve unaligned
// 16-byte loads (cur[ym, yp, y, y2m, y2p], prev[ym, yp, y, y2m, y2p], next[ym, yp]) and the 3-byte
// aprons of cur[ym] and cur[yp] as one dword on each side, loaded inside the row and shifted into
// place where the row ends sooner (the bytes outside [0, w) are zeros, which only the columns
// outside [3, w - 3) would meet, and those keep sp = (c + e) >> 1); all of them are issued before
// the arithmetic, which then runs on the packed dwords: a sum S(j) is one v_sad_u8 of a 3-byte
// window of each row (v_perm_b32), the temporal absolute differences v_sad_u8 on byte values
// (measured: 17% less time than subtractions and maxes on unpacked ints).  A piece that runs over a row end (16 / w
// of them; every piece of a plane narrower than 16) and the bytes before the first and after the
// last whole piece (the (plane, frame)'s first workgroup) go byte by byte through yadif_byte, which
// loads nothing outside [x - 3, x + 3] of a row.  U and V share a launch (blockIdx >= gxy * nf is V).
// The body is a __host__ __device__ function so that a host program can run it over every
// (workgroup, thread) of a launch on exactly-sized buffers.
struct DeintGeom {
  int w, h;                // the plane
  long long off;           // its offset inside a frame (source and destination alike)
  long long fstride;       // frame stride (both sides)
  long long poff;          // the next plane's offset from this one (V from U)
  int nf;                  // frames per plane
  int parity;              // rows with (y ^ parity) & 1 are interpolated: 0 top field first, 1 bottom
  uint32_t w_magic;        // ceil(2^32 / w)
  int gxy;                 // workgroups per (plane, frame)
  uint32_t gxy_magic;
  int lo[kMaxSegs], hi[kMaxSegs];  // per segment: the first and last readable frame, from its first encoded one
};

constexpr int kDeintThreads = 256;  // one piece per thread: a workgroup covers 4096 bytes of a plane's byte string

__host__ __device__ __forceinline__ int deint_div(int t, uint32_t magic, int d) {  // div_magic, for both sides
  if (!magic) return t;
  const int q = (int)(((uint64_t)(uint32_t)t * magic) >> 32);
  return q * d > t ? q - 1 : q;
}
__host__ __device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ int iabs(int a) { return a < 0 ? -a : a; }

// acc + the sum of the absolute differences of the four bytes of a and b: v_sad_u8 on the device (one
// instruction for |a - b| of two byte values, and for a three-tap sum S(j) on 3-byte windows), the
// same sum in plain C on the host (the two are overloads by target)
__device__ __forceinline__ uint32_t sad_u8(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }
__host__ inline uint32_t sad_u8(uint32_t a, uint32_t b, uint32_t acc) {
  for (int k = 0; k < 32; k += 8) acc += (uint32_t)iabs((int)((a >> k) & 255u) - (int)((b >> k) & 255u));
  return acc;
}
// bytes s, s + 1, s + 2 (s in 0..3) of the eight bytes hi:lo, and a zero byte on top
__device__ __forceinline__ uint32_t win3(uint32_t lo, uint32_t hi, uint32_t s) {
  return __builtin_amdgcn_perm(hi, lo, 0x0c000000u | ((s + 2) << 16) | ((s + 1) << 8) | s);
}
__host__ inline uint32_t win3(uint32_t lo, uint32_t hi, uint32_t s) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * s)) & 0xffffffu;
}

// the temporal part and the clip, shared by both forms: p* prev, n* next, q* = prev2 / next2 rows
// (every argument a byte value)
__host__ __device__ __forceinline__ int yadif_clip(bool nosp, int sp, int c, int e, int py, int cy, int pm, int pp,
                                                   int nm, int np, int p2m, int c2m, int p2p, int c2p) {
  const int d = (py + cy) >> 1;
  const int t0 = (int)sad_u8((uint32_t)py, (uint32_t)cy, 0u);
  const int t1 = (int)sad_u8((uint32_t)pp, (uint32_t)e, sad_u8((uint32_t)pm, (uint32_t)c, 0u));
  const int t2 = (int)sad_u8((uint32_t)np, (uint32_t)e, sad_u8((uint32_t)nm, (uint32_t)c, 0u));
  int diff = imax(imax(t0 >> 1, t1 >> 1), t2 >> 1);
  if (!nosp) {
    const int b = (p2m + c2m) >> 1, f = (p2p + c2p) >> 1;
    const int mx = imax(imax(d - e, d - c), imin(b - c, f - e));
    const int mn = imin(imin(d - e, d - c), imax(b - c, f - e));
    diff = imax(imax(diff, mn), -mx);
  }
  return imin(imax(sp, d - diff), d + diff);  // (diff >= 0: the clip in either order)
}

// One output byte of an interpolated row y, every load inside the plane
template <bool NOSPATIAL>
__host__ __device__ inline int yadif_byte(const uint8_t *pv, const uint8_t *cu, const uint8_t *nx, int w, int h, int y,
                                          int x) {
  const int ym = y ? y - 1 : y + 1, yp = y + 1 < h ? y + 1 : y - 1;
  const bool nosp = NOSPATIAL || y == 1 || y + 2 == h;
  const int y2m = nosp ? y : (y ? y - 2 : y + 2), y2p = nosp ? y : (y + 1 < h ? y + 2 : y - 2);
  const uint8_t *A = cu + (size_t)ym * w, *B = cu + (size_t)yp * w;
  const int c = A[x], e = B[x];
  int sp = (c + e) >> 1;
  if (x >= 3 && x < w - 3) {
    auto S = [&](int j) {
      return iabs(A[x - 1 + j] - B[x - 1 - j]) + iabs(A[x + j] - B[x - j]) + iabs(A[x + 1 + j] - B[x + 1 - j]);
    };
    int score = S(0) - 1;
#pragma unroll 1
    for (int s = -1; s <= 1; s += 2)
      if (S(s) < score) {
        score = S(s);
        sp = (A[x + s] + B[x - s]) >> 1;
        if (S(2 * s) < score) {
          score = S(2 * s);
          sp = (A[x + 2 * s] + B[x - 2 * s]) >> 1;
        }
      }
  }
  const size_t o = (size_t)y * w + x, om = (size_t)ym * w + x, op = (size_t)yp * w + x;
  const size_t o2m = (size_t)y2m * w + x, o2p = (size_t)y2p * w + x;
  return yadif_clip(nosp, sp, c, e, pv[o], cu[o], pv[om], pv[op], nx[om], nx[op], pv[o2m], cu[o2m], pv[o2p], cu[o2p]);
}

template <bool NOSPATIAL>
__host__ __device__ __forceinline__ void yadif_work(const SegList &src, uint8_t *dst, const DeintGeom &g, int t, int tid) {
  const int z = deint_div(t, g.gxy_magic, g.gxy), blk = t - z * g.gxy;
  const int pl = z >= g.nf, f = z - (pl ? g.nf : 0);
  // the frame's segment, its index there and its neighbours inside [lo, hi]
  int k = 0;
#pragma unroll
  for (int j = 1; j < kMaxSegs; j++)
    if (f >= src.f0[j]) k = j;
  const int i = f - (k ? src.f0[k] : 0);
  const int ip = imax(i - 1, g.lo[k]), in = imin(i + 1, g.hi[k]);
  const long long po = g.off + (pl ? g.poff : 0);
  const uint8_t *cu = src.p[k] + (long long)i * g.fstride + po;
  const uint8_t *pv = src.p[k] + (long long)ip * g.fstride + po;
  const uint8_t *nx = src.p[k] + (long long)in * g.fstride + po;
  uint8_t *d = dst + (long long)f * g.fstride + po;
  const int w = g.w, h = g.h;
  const int nb = w * h;  // < 2^28 (16384 x 16384)
  const int head = imin((int)(-(uintptr_t)d & 15), nb);
  const int nv = (nb - head) >> 4;
  auto byte_at = [&](int j) -> uint32_t {
    const int row = deint_div(j, g.w_magic, w), col = j - row * w;
    if (!((row ^ g.parity) & 1)) return cu[j];
    return (uint32_t)yadif_byte<NOSPATIAL>(pv, cu, nx, w, h, row, col);
  };
  const int kp = blk * kDeintThreads + tid;
  if (kp < nv) {
    const int j = head + 16 * kp;
    const int y = deint_div(j, g.w_magic, w), col = j - y * w;
    u32x4 v;
    if (col + 16 > w) {  // over a row end (rolled: 16 / w of the pieces)
      uint64_t wl = 0, wh = 0;
#pragma unroll 1
      for (int b = 0; b < 16; b++) {
        const uint64_t x = byte_at(j + b);
        if (b < 8) wl |= x << (8 * b);
        else wh |= x << (8 * (b - 8));
      }
      v = u32x4{(uint32_t)wl, (uint32_t)(wl >> 32), (uint32_t)wh, (uint32_t)(wh >> 32)};
    } else if (!((y ^ g.parity) & 1)) {
      v = *(const u32x4_a1 *)(cu + j);
    } else {
      const int ym = y ? y - 1 : y + 1, yp = y + 1 < h ? y + 1 : y - 1;
      const bool nosp = NOSPATIAL || y == 1 || y + 2 == h;
      const int y2m = nosp ? y : (y ? y - 2 : y + 2), y2p = nosp ? y : (y + 1 < h ? y + 2 : y - 2);
      const size_t om = (size_t)ym * w + col, op = (size_t)yp * w + col, o = (size_t)j;
      const size_t o2m = (size_t)y2m * w + col, o2p = (size_t)y2p * w + col;
      // the aprons: bytes [col - 4, col) and [col + 16, col + 20) of the row, loaded inside it (w >= 16 here)
      const int la = imax(col - 4, 0), ra = imin(col + 16, w - 4);
      const uint32_t lsh = 8u * (uint32_t)(la - (col - 4)), rsh = 8u * (uint32_t)(col + 16 - ra);  // 0..32
      uint32_t A[7], B[7];  // the rows' windows: bytes [col - 4, col + 20), and a zero dword
      A[6] = B[6] = 0u;
      A[0] = *(const u32_unaligned *)(cu + (size_t)ym * w + la);
      B[0] = *(const u32_unaligned *)(cu + (size_t)yp * w + la);
      A[5] = *(const u32_unaligned *)(cu + (size_t)ym * w + ra);
      B[5] = *(const u32_unaligned *)(cu + (size_t)yp * w + ra);
      const u32x4 am = *(const u32x4_a1 *)(cu + om), ap = *(const u32x4_a1 *)(cu + op);
      const u32x4 cy = *(const u32x4_a1 *)(cu + o), c2m = *(const u32x4_a1 *)(cu + o2m), c2p = *(const u32x4_a1 *)(cu + o2p);
      const u32x4 pm = *(const u32x4_a1 *)(pv + om), pp = *(const u32x4_a1 *)(pv + op), py = *(const u32x4_a1 *)(pv + o);
      const u32x4 p2m = *(const u32x4_a1 *)(pv + o2m), p2p = *(const u32x4_a1 *)(pv + o2p);
      const u32x4 nm = *(const u32x4_a1 *)(nx + om), np = *(const u32x4_a1 *)(nx + op);
      A[0] = lsh >= 32 ? 0u : A[0] << lsh;
      B[0] = lsh >= 32 ? 0u : B[0] << lsh;
      A[5] = rsh >= 32 ? 0u : A[5] >> rsh;
      B[5] = rsh >= 32 ? 0u : B[5] >> rsh;
#pragma unroll
      for (int q = 0; q < 4; q++) A[1 + q] = am[q], B[1 + q] = ap[q];
      auto bx = [](const u32x4 &r, int b) -> int { return (int)((r[b >> 2] >> (8 * (b & 3))) & 255u); };
      uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
      for (int b = 0; b < 16; b++) {
        // window byte 4 + b + k is column col + b + k of the row, k in -3..3
        auto a = [&](int kk) -> int { return (int)((A[(4 + b + kk) >> 2] >> (8 * ((4 + b + kk) & 3))) & 255u); };
        auto bb = [&](int kk) -> int { return (int)((B[(4 + b + kk) >> 2] >> (8 * ((4 + b + kk) & 3))) & 255u); };
        // S(j): one sum of absolute differences of the 3-byte windows at columns x - 1 + j of A and x - 1 - j of B
        auto w3 = [&](const uint32_t *W, int kk) -> uint32_t {
          const int t = 4 + b + kk;
          return win3(W[t >> 2], W[(t >> 2) + 1], (uint32_t)(t & 3));
        };
        auto S = [&](int jj) -> int { return (int)sad_u8(w3(A, jj - 1), w3(B, -1 - jj), 0u); };
        const int c = a(0), e = bb(0);
        int sp = (c + e) >> 1;
        {
          int score = S(0) - 1, sx = sp;
#pragma unroll
          for (int s = -1; s <= 1; s += 2) {
            const int s1 = S(s), s2 = S(2 * s);
            const bool t1 = s1 < score;
            const int sc1 = t1 ? s1 : score, sp1 = t1 ? (a(s) + bb(-s)) >> 1 : sx;
            const bool t2 = t1 && s2 < sc1;
            score = t2 ? s2 : sc1;
            sx = t2 ? (a(2 * s) + bb(-2 * s)) >> 1 : sp1;
          }
          const int x = col + b;
          sp = (x >= 3 && x < w - 3) ? sx : sp;
        }
        const int r = yadif_clip(nosp, sp, c, e, bx(py, b), bx(cy, b), bx(pm, b), bx(pp, b), bx(nm, b), bx(np, b),
                                 bx(p2m, b), bx(c2m, b), bx(p2p, b), bx(c2p, b));
        out[b >> 2] |= (uint32_t)r << (8 * (b & 3));
      }
      v = u32x4{out[0], out[1], out[2], out[3]};
    }
    *(u32x4 *)(d + j) = v;
  }
  if (blk == 0 && tid < 16) {
    const int a = tid, b = head + 16 * nv + tid;
    if (a < head) d[a] = (uint8_t)byte_at(a);
    if (b < nb) d[b] = (uint8_t)byte_at(b);
  }
}

template <bool NOSPATIAL>
__global__ __launch_bounds__(kDeintThreads) void k_yadif_plane(const SegList src, uint8_t *__restrict__ dst,
                                                               DeintGeom g) {
  yadif_work<NOSPATIAL>(src, dst, g, (int)blockIdx.x, (int)threadIdx.x);
}

// k_unsharp_plane: `-vf unsharp`, behind the sws stage and in front of the pad's
// border: one plane of the sws stage's output (full-range encoder-input samples) -> the same plane
// of a second buffer of the same layout (the slot's d_sharp), which k_encode then reads.  With
// sx = mx / 2, sy = my / 2, scalebits = 2 (sx + sy), half = 1 << (scalebits - 1), amount =
// (int)(amount * 65536.0), C(n, k) the binomial coefficient, P the w x h picture plane and its
// indices clamped into it (edge replication):
//   blur[y][x] = (sum_j sum_i C(2sy, j) C(2sx, i) P[clamp(y + j - sy)][clamp(x + i - sx)] + half) >> scalebits
//   out[y][x]  = clip_uint8(P[y][x] + (((P[y][x] - blur[y][x]) * amount) >> 16))     (C int, arithmetic >>)
// which is what vf_unsharp.c's running pair sums come to while 8 + scalebits <= 32 (the host refuses
// anything else for a plane whose amount is not 0).  A plane with amount == 0 is copied.
// The launch covers the whole plane of the encoded frame: cw x ch, rows cw apart; under a pad that
// is the canvas and the picture sits at (px, py) in it, else the picture is the plane.  Samples
// outside the picture are copied (the border k_pad_plane wrote); samples inside clamp at the
// picture's edges, so no border byte enters a sum.
// One workgroup makes one kSharpTileW x kSharpTileH tile of the plane, four samples of a row (a
// quad) per thread and step:
//   1. the tile and its sx / sy apron, (64 + 2sx) x (32 + 2sy) bytes, go into LDS rows of a
//      multiple of four bytes, a quad at a time; the coordinates are clamped into the picture before
//      an address is formed (sharp_fetch), and a quad that no clamp touches is one unaligned dword
//      load, any other four byte loads;
//   2. the horizontal pass: for each of the 32 + 2sy staged rows and each quad of the tile's 64
//      columns the four sums over i of C(2sx, i) * byte, each a uint32 (<= 255 * 2^22), from the
//      row's aligned dwords into LDS rows of 64 dwords as one 16-byte write;
//   3. the vertical pass: per quad the four sums over j of C(2sy, j) * row sum (<= 255 * 2^24 <
//      2^32) from 16-byte reads, the rounding shift, the centre bytes from the staged tile, the
//      sharpen and one unaligned dword store (sharp_store); a quad that leaves the plane or the
//      picture goes byte by byte, its samples outside the picture loaded from their own place.
// In 2 a wave reads 16 quads of each of four rows: rows a multiple of four bytes apart, eight-byte
// reads at consecutive dwords of a row, no conflict beyond the row change; its writes and the reads
// of 3 are consecutive 16-byte pieces of 256-byte rows.  A tile that misses the picture, and every
// tile of a plane with amount 0, is a copy by quads and skips 1 and 2.  The binomials come with the
// geometry (scalar loads at a uniform index; the horizontal products are 24-bit multiplies); <5, 5>,
// the filter's default and the commonest size, has them as constants and its loops unrolled, <0, 0>
// is every other size.  LDS: at most 3,672 bytes of samples and 54 x 64 dwords of row sums, 17.5 KB
// (<5, 5>: 11.7 KB), so eight workgroups fit a CU.  U and V share a launch (blockIdx >= gxy * nf is
// V).  The address arithmetic and the three steps are __host__ __device__ functions:
// tools/stage_host.hip walks every (workgroup, thread, iteration) of a launch on the CPU.
constexpr int kSharpTileW = 64;
constexpr int kSharpTileH = 32;
constexpr int kSharpThreads = 256;
constexpr int kSharpMaxTaps = 23;     // sizes 3..23
constexpr int kSharpMaxHalfSum = 12;  // sx + sy of a filtered plane: 8 + 2 (sx + sy) <= 32
constexpr int kSharpQuads = kSharpTileW * kSharpTileH / 4;  // output quads per tile
struct SharpGeom {
  int cw, ch;              // the plane of the encoded frame (the canvas plane under a pad): rows cw apart
  int px, py, w, h;        // the picture inside it (no pad: 0, 0, cw, ch)
  long long off;           // the plane's offset inside a frame (source and destination alike)
  long long fstride;       // frame stride (both sides)
  long long poff;          // the next plane's offset from this one (V from U)
  int nf;                  // frames per plane
  int sx, sy;              // half sizes
  int amount;              // (int)(amount * 65536.0); 0: the plane is copied
  int tx;                  // tiles per tile row
  uint32_t tx_magic;
  int gxy;                 // workgroups (tiles) per (plane, frame)
  uint32_t gxy_magic;
  uint32_t nq_magic;       // ceil(2^32 / (sharp_pitch(sx) / 4)): staged quads per row
  uint32_t bx[kSharpMaxTaps], by[kSharpMaxTaps];  // C(2sx, i), C(2sy, j)
};

__host__ __device__ constexpr int sharp_pitch(int sx) { return (kSharpTileW + 2 * sx + 3) & ~3; }
__host__ __device__ constexpr int sharp_rows(int sy) { return kSharpTileH + 2 * sy; }
// bytes of staged samples: the most over the sizes a filtered plane can have
__host__ __device__ constexpr int sharp_lds_bytes(int mx, int my) {
  if (mx) return sharp_pitch(mx / 2) * sharp_rows(my / 2);
  int m = 0;
  for (int sx = 1; sx <= kSharpMaxTaps / 2; sx++)
    for (int sy = 1; sy <= kSharpMaxTaps / 2 && sx + sy <= kSharpMaxHalfSum; sy++)
      m = sharp_pitch(sx) * sharp_rows(sy) > m ? sharp_pitch(sx) * sharp_rows(sy) : m;
  return m;
}
__host__ __device__ constexpr int sharp_lds_sums(int my) {
  return sharp_rows(my ? my / 2 : kSharpMaxTaps / 2) * kSharpTileW;
}

// The geometry of one plane's launch (host; submit adds nf and the U + V pairing)
inline SharpGeom sharp_geom(int cw, int ch, int px, int py, int w, int h, long long off, long long fstride, int mx,
                            int my, int amount) {
  SharpGeom g{};
  g.cw = cw, g.ch = ch, g.px = px, g.py = py, g.w = w, g.h = h;
  g.off = off, g.fstride = fstride;
  g.sx = mx / 2, g.sy = my / 2, g.amount = amount;
  g.tx = (cw + kSharpTileW - 1) / kSharpTileW;
  g.gxy = g.tx * ((ch + kSharpTileH - 1) / kSharpTileH);
  g.tx_magic = magic32((uint32_t)g.tx);
  g.gxy_magic = magic32((uint32_t)g.gxy);
  g.nq_magic = magic32((uint32_t)(sharp_pitch(g.sx) / 4));
  for (int d = 0; d < 2; d++) {  // a row of Pascal's triangle by pair sums, as the filter's own cascade
    uint32_t *b = d ? g.by : g.bx;
    const int n = 2 * (d ? g.sy : g.sx);
    b[0] = 1;
    for (int k = 1; k <= n; k++) {
      b[k] = 1;
      for (int i = k - 1; i > 0; i--) b[i] += b[i - 1];
    }
  }
  return g;
}

struct SharpTile {
  int x0, y0;  // the tile's first column and row in the plane
  bool filt;   // it holds picture samples of a plane with a non-zero amount
};

__host__ __device__ __forceinline__ SharpTile sharp_tile(const SharpGeom &g, int blk) {
  const int ty = deint_div(blk, g.tx_magic, g.tx);
  SharpTile T;
  T.x0 = (blk - ty * g.tx) * kSharpTileW;
  T.y0 = ty * kSharpTileH;
  T.filt = g.amount != 0 && T.x0 < g.px + g.w && T.x0 + kSharpTileW > g.px && T.y0 < g.py + g.h &&
           T.y0 + kSharpTileH > g.py;
  return T;
}

// Staged quad `it * kSharpThreads + tid` of a tile: false past the window; else its index in the
// LDS byte tile and the offsets of its four samples in the plane, each clamped into the picture.
// whole: no clamp moved a column, the four are consecutive bytes
__host__ __device__ __forceinline__ bool sharp_fetch(const SharpGeom &g, const SharpTile &T, int sx, int sy, int tid,
                                                     int it, int *lds_at, long long at[4], bool *whole) {
  const int nq = sharp_pitch(sx) / 4, idx = it * kSharpThreads + tid;
  if (idx >= nq * sharp_rows(sy)) return false;
  const int r = deint_div(idx, g.nq_magic, nq), q = idx - r * nq;
  const int y = imin(imax(T.y0 - sy + r, g.py), g.py + g.h - 1);
  const int x = T.x0 - sx + 4 * q;
  *lds_at = r * sharp_pitch(sx) + 4 * q;
#pragma unroll
  for (int k = 0; k < 4; k++) at[k] = (long long)y * g.cw + imin(imax(x + k, g.px), g.px + g.w - 1);
  *whole = x >= g.px && x + 3 < g.px + g.w;
  return true;
}

// Output quad `it * kSharpThreads + tid` of a tile (it < kSharpQuads / kSharpThreads): false outside
// the plane; else its first column and its row in the tile, its first sample's offset in the plane,
// how many of its samples lie inside the plane (n, 1..4) and which of those inside the picture (bit
// k of pic: sample k)
__host__ __device__ __forceinline__ bool sharp_store(const SharpGeom &g, const SharpTile &T, int tid, int it, int *col,
                                                     int *row, long long *at, int *n, int *pic) {
  const int idx = it * kSharpThreads + tid;
  *col = 4 * (idx & (kSharpTileW / 4 - 1));
  *row = idx / (kSharpTileW / 4);
  const int x = T.x0 + *col, y = T.y0 + *row;
  if (x >= g.cw || y >= g.ch) return false;
  *at = (long long)y * g.cw + x;
  *n = imin(4, g.cw - x);
  const bool yin = y >= g.py && y < g.py + g.h;
  int m = 0;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (k < *n && yin && x + k >= g.px && x + k < g.px + g.w) m |= 1 << k;
  *pic = m;
  return true;
}

template <int M>
__host__ __device__ __forceinline__ uint32_t sharp_coef(const uint32_t *b, int i) {
  if (M == 5) return i == 2 ? 6u : (i == 1 || i == 3) ? 4u : 1u;
  return b[i];
}

// bytes s..s + 3 (s in 0..3) of the eight bytes hi:lo
__host__ __device__ __forceinline__ uint32_t sharp_win(uint32_t lo, uint32_t hi, int s) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * s));
}

// step 1 for one thread: the window into the LDS byte tile
template <int MX, int MY>
__host__ __device__ __forceinline__ void sharp_stage(const uint8_t *s, const SharpGeom &g, const SharpTile &T, int tid,
                                                     uint8_t *lb) {
  const int sx = MX ? MX / 2 : g.sx, sy = MY ? MY / 2 : g.sy;
  const int n = sharp_pitch(sx) / 4 * sharp_rows(sy);
  for (int it = 0; it * kSharpThreads < n; it++) {
    int lat;
    long long at[4];
    bool whole;
    if (!sharp_fetch(g, T, sx, sy, tid, it, &lat, at, &whole)) continue;
    uint32_t v;
    if (whole) v = *(const u32_unaligned *)(s + at[0]);
    else v = (uint32_t)s[at[0]] | ((uint32_t)s[at[1]] << 8) | ((uint32_t)s[at[2]] << 16) | ((uint32_t)s[at[3]] << 24);
    *(uint32_t *)(lb + lat) = v;
  }
}

// step 2 for one thread: the row sums, a quad at a time
template <int MX, int MY>
__host__ __device__ __forceinline__ void sharp_hpass(const SharpGeom &g, int tid, const uint8_t *lb, uint32_t *ls) {
  const int sx = MX ? MX / 2 : g.sx, sy = MY ? MY / 2 : g.sy;
  const int pitch = sharp_pitch(sx), n = sharp_rows(sy) * (kSharpTileW / 4);
  for (int idx = tid; idx < n; idx += kSharpThreads) {
    const int r = idx / (kSharpTileW / 4), col = 4 * (idx & (kSharpTileW / 4 - 1));
    const uint32_t *p = (const uint32_t *)(lb + r * pitch + col);  // the quad's window: bytes [0, 4 + 2sx)
    uint32_t a[4] = {0, 0, 0, 0};
    uint32_t lo = p[0], hi = 0;
    if (MX) {
#pragma unroll
      for (int t = 0; t < (MX ? MX : 1); t++) {
        if ((t & 3) == 0 && t) lo = hi;
        if ((t & 3) == 0 && t + 1 < MX) hi = p[t / 4 + 1];
        if ((t & 3) == 0 && t + 1 >= MX) hi = 0;
        const uint32_t wd = sharp_win(lo, hi, t & 3), c = sharp_coef<MX>(g.bx, t);
#pragma unroll
        for (int o = 0; o < 4; o++) a[o] += c * ((wd >> (8 * o)) & 255u);
      }
    } else {
      for (int t = 0; t <= 2 * sx; t++) {
        if ((t & 3) == 0) {  // the next aligned dword, while a later tap needs it (it lies inside the row)
          if (t) lo = hi;
          hi = t < 2 * sx ? p[t / 4 + 1] : 0u;
        }
        const uint32_t wd = sharp_win(lo, hi, t & 3), c = g.bx[t] & 0xffffffu;  // (24-bit factors: one multiply-add)
#pragma unroll
        for (int o = 0; o < 4; o++) a[o] += c * ((wd >> (8 * o)) & 255u);
      }
    }
    *(u32x4 *)(ls + r * kSharpTileW + col) = u32x4{a[0], a[1], a[2], a[3]};
  }
}

// step 3 for one thread: the column sums, the sharpen and the stores; without a filter the copy
template <int MX, int MY>
__host__ __device__ __forceinline__ void sharp_vpass(const uint8_t *s, uint8_t *d, const SharpGeom &g, const SharpTile &T,
                                                     int tid, const uint8_t *lb, const uint32_t *ls) {
  const int sx = MX ? MX / 2 : g.sx, sy = MY ? MY / 2 : g.sy;
  const int pitch = sharp_pitch(sx), scalebits = 2 * (sx + sy);
#pragma unroll
  for (int it = 0; it < kSharpQuads / kSharpThreads; it++) {
    int col, row, n, pic;
    long long at;
    if (!sharp_store(g, T, tid, it, &col, &row, &at, &n, &pic)) continue;
    if (!T.filt || !pic) {  // a copy
      if (n == 4) {
        *(u32_unaligned *)(d + at) = *(const u32_unaligned *)(s + at);
      } else {
        for (int k = 0; k < n; k++) d[at + k] = s[at + k];
      }
      continue;
    }
    const uint32_t *q = ls + row * kSharpTileW + col;
    uint32_t a[4] = {0, 0, 0, 0};
    if (MY) {
#pragma unroll
      for (int j = 0; j < (MY ? MY : 1); j++) {
        const u32x4 v = *(const u32x4 *)(q + j * kSharpTileW);
        const uint32_t c = sharp_coef<MY>(g.by, j);
#pragma unroll
        for (int o = 0; o < 4; o++) a[o] += c * v[o];
      }
    } else {
      for (int j = 0; j <= 2 * sy; j++) {
        const u32x4 v = *(const u32x4 *)(q + j * kSharpTileW);
        const uint32_t c = g.by[j];
#pragma unroll
        for (int o = 0; o < 4; o++) a[o] += c * v[o];
      }
    }
    const uint8_t *ctr = lb + (row + sy) * pitch + col + sx;
    uint32_t out = 0;
#pragma unroll
    for (int o = 0; o < 4; o++) {
      const int blur = (int)((a[o] + (1u << (scalebits - 1))) >> scalebits);
      const int p = ctr[o];
      const int r = p + (((p - blur) * g.amount) >> 16);
      out |= (uint32_t)imin(imax(r, 0), 255) << (8 * o);
    }
    if (n == 4 && pic == 15) {
      *(u32_unaligned *)(d + at) = out;
    } else {
      for (int k = 0; k < n; k++) d[at + k] = (pic >> k) & 1 ? (uint8_t)(out >> (8 * k)) : s[at + k];
    }
  }
}

// workgroup t of a launch: its tile, and the plane of its (plane, frame) in the source and the destination
__host__ __device__ __forceinline__ SharpTile sharp_block(const SharpGeom &g, int t, long long *plane_at) {
  const int z = deint_div(t, g.gxy_magic, g.gxy), blk = t - z * g.gxy;
  const int pl = z >= g.nf, f = z - (pl ? g.nf : 0);
  *plane_at = (long long)f * g.fstride + g.off + (pl ? g.poff : 0);
  return sharp_tile(g, blk);
}

template <int MX, int MY>  // 0, 0: the sizes at run time
__global__ __launch_bounds__(kSharpThreads) void k_unsharp_plane(const uint8_t *__restrict__ src,
                                                                 uint8_t *__restrict__ dst, SharpGeom g) {
  __shared__ __attribute__((aligned(16))) uint8_t lb[sharp_lds_bytes(MX, MY)];
  __shared__ __attribute__((aligned(16))) uint32_t ls[sharp_lds_sums(MY)];
  const int tid = threadIdx.x;
  long long pa;
  const SharpTile T = sharp_block(g, (int)blockIdx.x, &pa);
  if (T.filt) {  // (uniform over the workgroup)
    sharp_stage<MX, MY>(src + pa, g, T, tid, lb);
    __syncthreads();
    sharp_hpass<MX, MY>(g, tid, lb, ls);
    __syncthreads();
  }
  sharp_vpass<MX, MY>(src + pa, dst + pa, g, T, tid, lb, ls);
}

// k_lut_plane: a table per plane, out = T[in] (`-vf eq` is three such tables, and the
// library knows only the tables).  A w x h rectangle of one plane of every frame of a launch, with row
// strides, plane and frame offsets of their own on either side; dst may be src (every byte is read and
// written by the same thread, and no byte outside the rectangle is read or written).  Streamed as
// k_plane_copy streams: the destination's span of a (plane, frame), the (h - 1) d_stride + w bytes from
// the rectangle's first to its last, is cut into 16-byte pieces aligned on the destination, piece k at
// span bytes [head + 16 k, + 16); span byte j is column j % d_stride of row j / d_stride (multiply-high:
// j < 2^28 + 2^14) and belongs to the rectangle when the column is below w.  A piece inside one row
// is one unaligned 16-byte load, sixteen LDS byte reads and one aligned store, kCopyVecs pieces per
// thread with every load issued before the first store; a piece between two rows is skipped; a piece
// that runs over a row end, and the bytes before the first and after the last whole piece (the (plane,
// frame)'s first workgroup), go byte by byte.  A rectangle whose rows are contiguous on both sides
// comes as one row of w h bytes (lut_geom), so whole planes have no row ends at all.
// The three tables (Y, U, V; 768 bytes at `tabs`) sit in LDS; a launch's first plane uses table
// g.tab and its second (V behind U: blockIdx >= gxy * nf) the next.  A plane whose table is the
// identity (g.ident) is copied without the lookups, or left alone when dst is src.  The LDS reads
// are k_plane_copy<RANGE>'s: byte reads at data-dependent addresses of a 256-byte table, 64 banks of
// one dword, so a wave's conflicts are those of 64 random draws from 64 banks.
// The body is a __host__ __device__ function, as yadif_work is, for tools/stage_host.hip.
struct LutGeom {
  int w, h;                    // the rectangle
  int s_stride, d_stride;      // its row strides
  long long s_off, d_off;      // its first byte inside a frame
  long long s_fstride, d_fstride;
  long long s_poff, d_poff;    // the next plane's rectangle from this one's (V from U)
  int nf;                      // frames per plane
  int tab;                     // the first plane's table: 0 Y, 1 U, 2 V
  int ident;                   // bit i: table i is the identity
  uint32_t ds_magic;           // ceil(2^32 / d_stride)
  int gxy;                     // workgroups per (plane, frame)
  uint32_t gxy_magic;
};

// The geometry of a w x h rectangle (nf, tab, ident, the plane offsets and the magics of the two
// divisors are the caller's): rows contiguous on both sides fold into one
inline void lut_geom_rect(LutGeom &g, int w, int h, int s_stride, int d_stride) {
  const bool flat = s_stride == w && d_stride == w;
  g.w = flat ? w * h : w;  // (<= 2^28)
  g.h = flat ? 1 : h;
  g.s_stride = flat ? g.w : s_stride;
  g.d_stride = flat ? g.w : d_stride;
  const size_t pieces = ((size_t)(g.h - 1) * g.d_stride + g.w) >> 4, per = (size_t)kCopyThreads * kCopyVecs;
  g.gxy = (int)(pieces ? (pieces + per - 1) / per : 1);
}

__host__ __device__ __forceinline__ void lut_work(const SegList &src, uint8_t *dst, const LutGeom &g,
                                                  const uint8_t *tabs, int t, int tid) {
  const int z = deint_div(t, g.gxy_magic, g.gxy), blk = t - z * g.gxy;
  const int pl = z >= g.nf, f = z - (pl ? g.nf : 0);
  int k = 0;
#pragma unroll
  for (int j = 1; j < kMaxSegs; j++)
    if (f >= src.f0[j]) k = j;
  const uint8_t *s = src.p[k] + (long long)(f - (k ? src.f0[k] : 0)) * g.s_fstride + g.s_off + (pl ? g.s_poff : 0);
  uint8_t *d = dst + (long long)f * g.d_fstride + g.d_off + (pl ? g.d_poff : 0);
  const int ti = g.tab + pl;
  const bool id = (g.ident >> ti) & 1;
  if (id && s == d) return;  // (uniform over the workgroup)
  const uint8_t *T = tabs + 256 * ti;
  const int w = g.w, ss = g.s_stride, ds = g.d_stride;
  const int nb = (g.h - 1) * ds + w;
  const int head = imin((int)(-(uintptr_t)d & 15), nb);
  const int nv = (nb - head) >> 4;
  auto map4 = [&](uint32_t x) -> uint32_t {
    if (id) return x;
    return (uint32_t)T[x & 255u] | ((uint32_t)T[(x >> 8) & 255u] << 8) | ((uint32_t)T[(x >> 16) & 255u] << 16) |
           ((uint32_t)T[x >> 24] << 24);
  };
  auto byte_at = [&](int j) {  // span byte j, when it is one of the rectangle's
    const int row = deint_div(j, g.ds_magic, ds), col = j - row * ds;
    if (col < w) {
      const uint8_t x = s[(size_t)row * ss + col];
      d[j] = id ? x : T[x];
    }
  };
  const int k0 = blk * (kCopyThreads * kCopyVecs) + tid;
  u32x4 v[kCopyVecs];
  bool whole[kCopyVecs];
#pragma unroll
  for (int i = 0; i < kCopyVecs; i++) {
    const int kp = k0 + i * kCopyThreads;
    whole[i] = false;
    v[i] = u32x4{0, 0, 0, 0};
    if (kp < nv) {
      const int j = head + 16 * kp;
      const int row = deint_div(j, g.ds_magic, ds), col = j - row * ds;
      if (col + 16 <= w) {
        whole[i] = true;
        v[i] = *(const u32x4_a1 *)(s + (size_t)row * ss + col);
      } else if (col < w || col + 16 > ds) {  // over a row end (rolled: 16 / d_stride of the pieces)
#pragma unroll 1
        for (int b = 0; b < 16; b++) byte_at(j + b);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kCopyVecs; i++) {
    const int kp = k0 + i * kCopyThreads;
    if (whole[i]) *(u32x4 *)(d + head + 16 * kp) = u32x4{map4(v[i][0]), map4(v[i][1]), map4(v[i][2]), map4(v[i][3])};
  }
  if (blk == 0 && tid < 16) {
    const int a = tid, b = head + 16 * nv + tid;
    if (a < head) byte_at(a);
    if (b < nb) byte_at(b);
  }
}

__global__ __launch_bounds__(kCopyThreads) void k_lut_plane(const SegList src, uint8_t *dst,
                                                            const uint8_t *__restrict__ tabs, LutGeom g) {
  __shared__ __attribute__((aligned(16))) uint8_t tab[768];
  const int tid = threadIdx.x;
  if (tid < 192) ((uint32_t *)tab)[tid] = ((const uint32_t *)tabs)[tid];
  __syncthreads();
  lut_work(src, dst, g, tab, (int)blockIdx.x, tid);
}

// k_cmat_frame: a 3 x 3 colour matrix on whole frames (`-vf colormatrix` is six 16.16
// coefficients, and the library knows only the coefficients).  Per sample, C int and arithmetic >>, with
// (U, V) the chroma pair of the luma sample's cell (x >> HS, y >> VS):
//   u = U - 128, v = V - 128, k = (yu u + yv v + 1081344) >> 16
//   Y' = clip8(Y - 16 + k)                        (= clip8((65536 (Y - 16) + yu u + yv v + 1081344) >> 16))
//   U' = clip8((uu u + uv v + 8421376) >> 16), V' = clip8((vu u + vv v + 8421376) >> 16)
// so a luma sample depends on the chroma pair above it, and one launch covers all three planes of every
// frame of a submit.  The work item is a piece: 16 chroma samples of one chroma row (piece p of row r:
// columns [16 p, 16 p + 16)) with the luma cell rows above them, 16 U bytes, 16 V bytes and 1 << VS rows
// of 16 << HS luma bytes.  A piece that lies inside the three planes is 2 + (1 << VS) (1 << HS) unaligned
// 16-byte loads, all issued before the first store, and as many stores; the second luma row that the
// last cell row of an odd height lacks is left out.  A piece over a chroma row's end (the last of a row whose width is no
// multiple of 16, every piece of a plane narrower than 16), and one whose last chroma column has a
// single luma column (odd width), goes sample by sample.  Every byte is read and written by the thread
// of its piece alone, so dst may be src, and no byte outside the three planes is touched; frames lie at
// any alignment (33 x 17 4:4:4 has odd frame bytes), with frame strides of their own on either side.
// The grid's x is workgroups per frame x frames, nothing else: no plane is a grid index, so there is no
// 2 n <= 65,535 as for the plane kernels and no launch for V alone.  38,000 frames fit because x runs
// to 2^31 - 1 and a frame of up to 256 pieces is one workgroup (38,000 of them); open refuses a context
// whose gxy x frames would pass 2^31 - 1.
// Sums: |coefficient| <= 2^18 (mjg_open_cmat) and |u|, |v| <= 128, so |yu u + yv v| <= 2^26 and every
// sum is below 2^26 + 2^24 in magnitude: int32 holds it, and k fits an int16.
// The body is a __host__ __device__ function, as lut_work is, for tools/stage_host.hip.
struct CmatCoef { int yu, yv, uu, uv, vu, vv; };
struct CmatGeom {
  int w, h;                    // the luma plane
  int cw, ch;                  // the chroma planes: (w + HS) >> HS, (h + VS) >> VS
  long long s_fstride, d_fstride;
  int ppr;                     // pieces per chroma row: ceil(cw / 16)
  uint32_t ppr_magic;
  int np;                      // pieces per frame: ppr * ch
  int gxy;                     // workgroups per frame
  uint32_t gxy_magic;
};

constexpr int kCmatThreads = 256;  // one piece per thread
constexpr int kCmatMaxCoef = 262144;  // |coefficient| <= 2^18, four times unity (mjg_open_cmat refuses more)

// The geometry of w x h frames with chroma shifts hs, vs (the frame strides and the magics of the two
// divisors are the caller's)
inline void cmat_geom_frame(CmatGeom &g, int w, int h, int hs, int vs) {
  g.w = w;
  g.h = h;
  g.cw = (w + hs) >> hs;
  g.ch = (h + vs) >> vs;
  g.ppr = (g.cw + 15) >> 4;
  g.np = g.ppr * g.ch;  // (<= 2^10 * 2^14)
  g.gxy = (g.np + kCmatThreads - 1) / kCmatThreads;
}

__host__ __device__ __forceinline__ int cmat_clip8(int x) { return x < 0 ? 0 : x > 255 ? 255 : x; }

// clip8(x >> 16), with the clamp in front of the shift: [0, 0xFFFFFF] >> 16 is [0, 255].  Written
// as clip8(x >> 16), pairs of these become gfx950's v_ashr_pk_u8_i32, which writes 16 bits of its
// register and keeps the other 16, and hipcc (ROCm 7.x) then ORs bytes 2 and 3 into that register as
// if they were zero: byte 2 came out OR-ed with the unclipped byte 0 on the MI355X
__host__ __device__ __forceinline__ int cmat_clip8_16(int x) {
  x = x < 0 ? 0 : x > 0xFFFFFF ? 0xFFFFFF : x;
  return (int)((uint32_t)x >> 16);
}

// A coefficient as the compiler can see it: sign-extended from 24 bits, which changes no value that
// mjg_open_cmat lets through (|c| <= 2^18).  With |u|, |v| <= 128 both factors are then inside 24 bits
// and the device takes the full-rate 24-bit multiply-add (a 32-bit multiply is quarter rate)
__host__ __device__ __forceinline__ int cmat_c24(int c) { return (int)((uint32_t)c << 8) >> 8; }

// One chroma pair: what its cell's luma samples gain (k - 16), and U', V'
__host__ __device__ __forceinline__ void cmat_uv(const CmatCoef &cm, int U, int V, int &d, int &uo, int &vo) {
  const int u = U - 128, v = V - 128;
  d = ((cm.yu * u + cm.yv * v + 1081344) >> 16) - 16;
  uo = cmat_clip8_16(cm.uu * u + cm.uv * v + 8421376);
  vo = cmat_clip8_16(cm.vu * u + cm.vv * v + 8421376);
}

template <int HS, int VS>
__host__ __device__ __forceinline__ void cmat_work(const SegList &src, uint8_t *dst, const CmatGeom &g,
                                                   const CmatCoef &coef, int t, int tid) {
  const CmatCoef cm{cmat_c24(coef.yu), cmat_c24(coef.yv), cmat_c24(coef.uu), cmat_c24(coef.uv), cmat_c24(coef.vu),
                    cmat_c24(coef.vv)};
  const int f = deint_div(t, g.gxy_magic, g.gxy), blk = t - f * g.gxy;
  const int piece = blk * kCmatThreads + tid;
  if (piece >= g.np) return;
  int k = 0;
#pragma unroll
  for (int j = 1; j < kMaxSegs; j++)
    if (f >= src.f0[j]) k = j;
  const uint8_t *s = src.p[k] + (long long)(f - (k ? src.f0[k] : 0)) * g.s_fstride;
  uint8_t *d = dst + (long long)f * g.d_fstride;
  const int w = g.w, cw = g.cw;
  const size_t uo = (size_t)w * g.h, vo = uo + (size_t)cw * g.ch;  // the U and the V plane in a frame
  const int r = deint_div(piece, g.ppr_magic, g.ppr), c0 = (piece - r * g.ppr) << 4;
  const int y0 = r << VS, x0 = c0 << HS;
  const int nr = imin(1 << VS, g.h - y0);  // the cell rows the frame has
  const size_t ci = (size_t)r * cw + c0;
  if (c0 + 16 <= cw && x0 + (16 << HS) <= w) {
    const u32x4 U = *(const u32x4_a1 *)(s + uo + ci), V = *(const u32x4_a1 *)(s + vo + ci);
    u32x4 Y[1 << VS][1 << HS];
#pragma unroll
    for (int ry = 0; ry < (1 << VS); ry++)
#pragma unroll
      for (int j = 0; j < (1 << HS); j++)
        Y[ry][j] = ry < nr ? *(const u32x4_a1 *)(s + (size_t)(y0 + ry) * w + x0 + 16 * j) : u32x4{0, 0, 0, 0};
    int dy[16];
    u32x4 Uo, Vo;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      uint32_t a = 0, b = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        int pu, pv;
        cmat_uv(cm, (int)((U[q] >> (8 * i)) & 255u), (int)((V[q] >> (8 * i)) & 255u), dy[4 * q + i], pu, pv);
        a |= (uint32_t)pu << (8 * i);
        b |= (uint32_t)pv << (8 * i);
      }
      Uo[q] = a;
      Vo[q] = b;
    }
#pragma unroll
    for (int ry = 0; ry < (1 << VS); ry++)
#pragma unroll
      for (int j = 0; j < (1 << HS); j++) {
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          uint32_t a = 0;
#pragma unroll
          for (int i = 0; i < 4; i++)  // luma byte 16 j + 4 q + i of the piece: chroma sample (16 j + 4 q + i) >> HS
            a |= (uint32_t)cmat_clip8((int)((Y[ry][j][q] >> (8 * i)) & 255u) + dy[(16 * j + 4 * q + i) >> HS]) << (8 * i);
          o[q] = a;
        }
        if (ry < nr) *(u32x4_a1 *)(d + (size_t)(y0 + ry) * w + x0 + 16 * j) = o;
      }
    *(u32x4_a1 *)(d + uo + ci) = Uo;
    *(u32x4_a1 *)(d + vo + ci) = Vo;
    return;
  }
  // over a row end, or the last column's cell is one luma sample wide (rolled: at most one piece a chroma row)
  const int ce = imin(c0 + 16, cw);
#pragma unroll 1
  for (int c = c0; c < ce; c++) {
    const size_t cj = (size_t)r * cw + c;
    int dl, pu, pv;
    cmat_uv(cm, s[uo + cj], s[vo + cj], dl, pu, pv);
    const int xe = imin((c + 1) << HS, w);
    for (int ry = 0; ry < nr; ry++)
      for (int x = c << HS; x < xe; x++) {
        const size_t yi = (size_t)(y0 + ry) * w + x;
        d[yi] = (uint8_t)cmat_clip8((int)s[yi] + dl);
      }
    d[uo + cj] = (uint8_t)pu;
    d[vo + cj] = (uint8_t)pv;
  }
}

template <int HS, int VS>
__global__ __launch_bounds__(kCmatThreads) void k_cmat_frame(const SegList src, uint8_t *dst, CmatGeom g, CmatCoef cm) {
  cmat_work<HS, VS>(src, dst, g, cm, (int)blockIdx.x, (int)threadIdx.x);
}

// k_tile_plane: `-vf tile`, several frames on one picture (mjg_open_sheet).  The input is
// the sws stage's output (under a sharpen, its output): nf cell frames, packed planar, full range, one
// buffer, s_fstride apart.  The output is the sheets, packed planar in the same format, d_fstride apart.
// A sheet plane is W x H; cell t of it is the w x h rectangle at (mx + pw (t % cols), my + ph (t / cols)),
// pw = w + padding, ph = h + padding, every value in samples of this plane (the margin, the padding and
// the cell are multiples of the sub-sampling, so the chroma values are the luma ones shifted).  Every
// byte outside a cell that holds a frame is `fill` (the pad's black: 0 luma, 128 chroma).
// Which frame a cell holds: each segment of the submit is a sequence of its own, and the geometry
// gives per segment its first sheet, its first frame and its frame count.  Sheet s of the submit is
// sheet j = s - sheet0[k] of the last segment k with sheet0[k] <= s; its cell t holds the frame
// first[k] + j N + t when t < N and j N + t < count[k], and is blank otherwise.
// Layout: as k_plane_copy, the sheet plane of a (plane, sheet) is one byte string of W H bytes (at most
// 2^28) cut into 16-byte pieces aligned on the destination, kCopyVecs pieces a thread; piece k covers
// bytes [head + 16 k, + 16), byte i is column i % W of row i / W, and its cell comes from two more
// multiply-high divisions, by pw and by ph.  A piece inside one row of a cell that holds a frame is one
// unaligned 16-byte load.  A piece that is blank as a whole is the constant: a piece inside one sheet
// row that lies in a row of the margin or the padding, in the left margin, in one blank cell (with the
// gap behind it), in the gap behind a cell or behind the row's last cell.  Any other piece (over a cell edge,
// over a row end, every piece of a cell narrower than 16) is put together byte by byte in a rolled loop.
// Each piece is then one aligned 16-byte store, behind all of the thread's loads.  The bytes before the
// first and behind the last whole piece go byte by byte in the (plane, sheet)'s first workgroup.
// U and V share a launch (blockIdx >= gxy * ns is V).
// Addresses.  A load is made only for a cell that holds a frame: f = first[k] + j N + t with t < N
// and 0 <= j N + t < count[k], so f is one of the segment's frames [first[k], first[k] + count[k]), which
// the host takes from the submit's nf frames; inside it the byte is (yy, xx) with 0 <= yy < h and
// 0 <= xx < w (a vector load: xx + 16 <= w) of the plane at s_off (+ s_poff), so every load lies inside a
// plane of one of the nf cell frames.  No address is formed for a blank cell.  A store is an aligned
// piece inside [head, head + 16 nv) or a byte i < W H of the sheet plane at d_off (+ d_poff) of sheet
// s < ns (the grid has gxy workgroups for each of them and no more), so every store lies inside it.
// The body is a __host__ __device__ function, as yadif_work is, for tools/stage_host.hip.
struct TileGeom {
  int w, h;                 // the cell plane
  int W, H;                 // the sheet plane
  int pw, ph;               // the cell pitches: w + padding, h + padding
  int mx, my;               // the margin
  int cols, ncells, N;      // cells a row, cells a sheet, frames a sheet
  int fill;                 // the blank byte
  long long s_off, d_off;   // the plane's first byte inside a cell frame / a sheet frame
  long long s_fstride, d_fstride;
  long long s_poff, d_poff; // the next plane's offset from this one (V from U)
  int ns;                   // sheets per plane
  uint32_t W_magic, pw_magic, ph_magic;  // ceil(2^32 / W), / pw, / ph
  int gxy;                  // workgroups per (plane, sheet)
  uint32_t gxy_magic;
  int sheet0[kMaxSegs], first[kMaxSegs], count[kMaxSegs];  // per segment: its first sheet (INT_MAX: unused), first frame, frames
};

// workgroups per (plane, sheet) for a sheet plane of W x H
inline int tile_gxy(int W, int H) {
  const size_t pieces = ((size_t)W * H) >> 4, per = (size_t)kCopyThreads * kCopyVecs;
  return (int)(pieces ? (pieces + per - 1) / per : 1);
}

__host__ __device__ __forceinline__ void tile_work(const uint8_t *src, uint8_t *dst, const TileGeom &g, int t, int tid) {
  const int z = deint_div(t, g.gxy_magic, g.gxy), blk = t - z * g.gxy;
  const int pl = z >= g.ns, sh = z - (pl ? g.ns : 0);
  int k = 0;
#pragma unroll
  for (int i = 1; i < kMaxSegs; i++)
    if (sh >= g.sheet0[i]) k = i;
  const int jn = (sh - g.sheet0[k]) * g.N;        // the sheet's first frame in its segment
  const int left = g.count[k] - jn;               // cells t < left (and < N) hold a frame
  const uint8_t *s = src + (long long)(g.first[k] + jn) * g.s_fstride + g.s_off + (pl ? g.s_poff : 0);  // cell 0's plane
  uint8_t *d = dst + (long long)sh * g.d_fstride + g.d_off + (pl ? g.d_poff : 0);
  const int w = g.w, h = g.h, W = g.W, pw = g.pw, ph = g.ph, cols = g.cols;
  const int nb = W * g.H;
  const int head = imin((int)(-(uintptr_t)d & 15), nb);
  const int nv = (nb - head) >> 4;
  const uint32_t fill = (uint32_t)g.fill;
  auto holds = [&](int c) { return c < g.N && c < left; };
  auto byte_at = [&](int i) -> uint32_t {  // byte i of the sheet plane
    const int row = deint_div(i, g.W_magic, W), col = i - row * W;
    const int ry = row - g.my, cx = col - g.mx;
    if (ry < 0 || cx < 0) return fill;
    const int r = deint_div(ry, g.ph_magic, ph), yy = ry - r * ph;
    const int cc = deint_div(cx, g.pw_magic, pw), xx = cx - cc * pw;
    const int c = r * cols + cc;
    if (yy >= h || xx >= w || cc >= cols || c >= g.ncells || !holds(c)) return fill;
    return s[(long long)c * g.s_fstride + (size_t)yy * w + xx];
  };
  const int k0 = blk * (kCopyThreads * kCopyVecs) + tid;
  const u32x4 blank = u32x4{fill * 0x01010101u, fill * 0x01010101u, fill * 0x01010101u, fill * 0x01010101u};
  u32x4 v[kCopyVecs];
#pragma unroll
  for (int i = 0; i < kCopyVecs; i++) {
    const int kp = k0 + i * kCopyThreads;
    v[i] = blank;
    if (kp >= nv) continue;
    const int j = head + 16 * kp;
    const int row = deint_div(j, g.W_magic, W), col = j - row * W;
    const int ry = row - g.my, cx = col - g.mx;
    int kind = 2;  // 0 blank, 1 one load, 2 byte by byte
    const uint8_t *at = s;
    if (col + 16 <= W) {
      const int r = ry < 0 ? 0 : deint_div(ry, g.ph_magic, ph), yy = ry - r * ph;
      if (ry < 0 || yy >= h || r * cols >= g.ncells || col + 16 <= g.mx) {
        kind = 0;
      } else if (cx >= 0) {
        const int cc = deint_div(cx, g.pw_magic, pw), xx = cx - cc * pw;
        const int c = r * cols + cc;
        if (cc >= cols || (xx >= w && (xx + 16 <= pw || cc == cols - 1)) || (xx + 16 <= pw && !holds(c))) {
          kind = 0;
        } else if (xx + 16 <= w) {  // (the cell holds a frame)
          kind = 1;
          at = s + (long long)c * g.s_fstride + (size_t)yy * w + xx;
        }
      }
    }
    if (kind == 1) {
      v[i] = *(const u32x4_a1 *)at;
    } else if (kind == 2) {  // rolled: pieces over a cell edge or a row end
#pragma unroll 1
      for (int q = 0; q < 4; q++) {
        uint32_t a = 0;
#pragma unroll 1
        for (int b = 0; b < 4; b++) a |= byte_at(j + 4 * q + b) << (8 * b);
        v[i][q] = a;
      }
    }
  }
  uint32_t ha = 0, hb = 0;  // the head and tail bytes: the (plane, sheet)'s first workgroup
  const int ia = tid, ib = head + 16 * nv + tid;
  const bool edge = blk == 0 && tid < 16;
  if (edge && ia < head) ha = byte_at(ia);
  if (edge && ib < nb) hb = byte_at(ib);
#pragma unroll
  for (int i = 0; i < kCopyVecs; i++) {
    const int kp = k0 + i * kCopyThreads;
    if (kp < nv) *(u32x4 *)(d + head + 16 * kp) = v[i];
  }
  if (edge && ia < head) d[ia] = (uint8_t)ha;
  if (edge && ib < nb) d[ib] = (uint8_t)hb;
}

__global__ __launch_bounds__(kCopyThreads) void k_tile_plane(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                             TileGeom g) {
  tile_work(src, dst, g, (int)blockIdx.x, (int)threadIdx.x);
}

// k_frame_hist: the per-frame, per-plane histograms that `-vf thumbnail` selects by (DESIGN §4.18;
// mjg_hist_open).  The input is a SegList of decoded frames, packed planar in the source format, fstride
// apart; the output is hist[nframes][768] uint32 counters, zeroed by the caller: hist[f][256 p + v] is
// the number of samples of value v in plane p (0 Y, 1 U, 2 V) of frame f, each plane at its own size.
// The chain's first reduction: nothing is written but counters.
// Layout: a plane of a frame is one byte string of nb bytes, cut into 16-byte pieces aligned on the
// SOURCE (there is no destination to align on), kHistVecs pieces a thread, so a workgroup covers 16 KiB
// of one plane of one frame.  One launch covers all three planes of every frame: the grid's x is
// workgroups per frame (gy for Y, then gc for U, then gc for V) x frames, split by multiply-high as in
// the other stage kernels, so no plane and no frame is a grid index and there is no 32,767-frame limit;
// open refuses a gpf x frames past 2^31 - 1.  The bytes before the first and behind the last whole piece
// (up to 15 each; all of a plane below one piece) are counted one by one by the (plane, frame)'s first
// workgroup.
// Counting: a workgroup counts into LDS, kHistCopies copies of the 256 bins interleaved as
// lh[v kHistCopies + copy] with copy = lane % kHistCopies: a flat plane, where all 64 lanes of a wave add
// to one bin, lands on kHistCopies addresses in as many banks (4 lanes each) and not on one.  All of a
// thread's loads are issued before its first add.  Behind a barrier thread v sums bin v's copies and
// adds a non-zero sum to hist with one global integer atomic: at most 256 a workgroup.  Integer adds
// commute, so the counts are exact whatever the order; a counter holds 2^32 - 1 and a plane at most
// 2^28 samples.
// Addresses.  A piece is bytes [head + 16 k, + 16) of the plane with k < nv = (nb - head) >> 4, so it
// ends at or before byte nb; a single byte is a < head <= nb or b < nb.  The plane is [off, off + nb)
// of frame f < nf of its segment, so every load lies inside a plane of a frame of the call.  The stores
// are hist[f][256 p + v] with f < nf, p < 3, v < 256.
// The body is two __host__ __device__ functions (count, flush; a barrier between them), as yadif_work
// is one, for tools/stage_host.hip: on the host the adds are plain.
struct HistGeom {
  int nb[2];           // bytes of the Y plane, of a chroma plane (<= 2^28)
  long long fstride;   // frame bytes
  int gy, gc;          // workgroups of the Y plane, of a chroma plane
  int gpf;             // workgroups per frame: gy + 2 gc
  uint32_t gpf_magic;
};

constexpr int kHistThreads = 256;  // = the bins: thread v flushes bin v
constexpr int kHistVecs = 4;       // pieces per thread, all loaded before the first is counted
constexpr int kHistCopies = 16;    // LDS copies of a bin, on consecutive banks

// workgroups of a plane of nb >= 1 bytes: its at most nb / 16 pieces (a plane below one piece: one, for its bytes)
inline int hist_wgs(int nb) { return (nb + kHistThreads * kHistVecs * 16 - 1) / (kHistThreads * kHistVecs * 16); }

__device__ __forceinline__ void hist_add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
__host__ inline void hist_add(uint32_t *p, uint32_t v) { *p += v; }

// the (plane, frame) of workgroup t and its index inside that plane
__host__ __device__ __forceinline__ void hist_block(const HistGeom &g, int t, int *f, int *pl, int *pblk) {
  *f = deint_div(t, g.gpf_magic, g.gpf);
  const int blk = t - *f * g.gpf;
  *pl = blk < g.gy ? 0 : blk < g.gy + g.gc ? 1 : 2;
  *pblk = blk - (*pl ? g.gy : 0) - (*pl == 2 ? g.gc : 0);
}

__host__ __device__ __forceinline__ void hist_count(const SegList &src, uint32_t *lh, const HistGeom &g, int t, int tid) {
  int f, pl, pblk;
  hist_block(g, t, &f, &pl, &pblk);
  int k = 0;
#pragma unroll
  for (int j = 1; j < kMaxSegs; j++)
    if (f >= src.f0[j]) k = j;
  const long long off = pl ? (long long)g.nb[0] + (pl == 2 ? g.nb[1] : 0) : 0;
  const uint8_t *s = src.p[k] + (long long)(f - (k ? src.f0[k] : 0)) * g.fstride + off;
  const int nb = g.nb[pl ? 1 : 0];
  const int head = imin((int)(-(uintptr_t)s & 15), nb);
  const int nv = (nb - head) >> 4;  // whole pieces: bytes [head, head + 16 nv) of the plane
  uint32_t *mine = lh + (tid & (kHistCopies - 1));
  auto count = [&](uint32_t v) { hist_add(mine + v * kHistCopies, 1u); };
  const int k0 = pblk * (kHistThreads * kHistVecs) + tid;
  u32x4 v[kHistVecs];
#pragma unroll
  for (int i = 0; i < kHistVecs; i++) {
    const int kp = k0 + i * kHistThreads;
    if (kp < nv) v[i] = *(const u32x4 *)(s + head + 16 * (size_t)kp);
  }
#pragma unroll
  for (int i = 0; i < kHistVecs; i++) {
    const int kp = k0 + i * kHistThreads;
    if (kp < nv) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t x = v[i][q];
        count(x & 255u), count((x >> 8) & 255u), count((x >> 16) & 255u), count(x >> 24);
      }
    }
  }
  if (pblk == 0 && tid < 16) {
    const int a = tid, b = head + 16 * nv + tid;
    if (a < head) count(s[a]);
    if (b < nb) count(s[b]);
  }
}

__host__ __device__ __forceinline__ void hist_flush(const uint32_t *lh, uint32_t *hist, const HistGeom &g, int t, int tid) {
  int f, pl, pblk;
  hist_block(g, t, &f, &pl, &pblk);
  uint32_t sum = 0;
#pragma unroll
  for (int c = 0; c < kHistCopies; c++) sum += lh[tid * kHistCopies + c];
  if (sum) hist_add(hist + (size_t)f * 768 + 256 * pl + tid, sum);
}

__global__ __launch_bounds__(kHistThreads) void k_frame_hist(const SegList src, uint32_t *__restrict__ hist, HistGeom g) {
  __shared__ __attribute__((aligned(16))) uint32_t lh[256 * kHistCopies];
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < kHistCopies / 4; c++) ((u32x4 *)lh)[c * kHistThreads + tid] = u32x4{0, 0, 0, 0};
  __syncthreads();
  hist_count(src, lh, g, (int)blockIdx.x, tid);
  __syncthreads();
  hist_flush(lh, hist, g, (int)blockIdx.x, tid);
}

// k_dn_rows, k_dn_cols, k_dn_time: `-vf hqdn3d` (mjg_open_denoise), the chain's first
// recursive filter: on every plane of every frame a scan along each row (P), a scan down each column (V)
// and a scan through time (A), each step c(tab, a, b) = b + tab[4096 + ((a - b) >> 4)] with
// L(v) = (v << 8) + 127, in C int with an arithmetic shift:
//   P[y][0] = y ? L(s[y][0]) : c(S, L(s[0][0]), L(s[0][0]));   P[y][x] = c(S, P[y][x-1], L(s[y][x]))
//   V[0][x] = P[0][x];                                          V[y][x] = c(S, V[y-1][x], P[y][x])
//   A_t[y][x] = c(M, A_{t-1}[y][x], V_t[y][x]), A_{-1} = L(s_0);  out_t = A_t >> 8
// S / M: the plane's spatial / temporal table of 8192 int16 (mjg_denoise: luma ls, lt; chroma cs, ct).
// A step is a table lookup, so no scan can be split: the parallelism is across rows, across columns and
// across samples, never along a scan.  Each kernel keeps its one 16 KiB table in LDS, and the index is
// clamped into 0..8191 before an address is made of it.  Every value fits uint16 for tables the filter
// makes (within about 8 of the span of a step's arguments); other tables wrap, and stay
// inside every buffer.
// Buffers.  The source is the submit's SegList (or the deinterlacer's buffer): packed planar bytes, never
// written.  p16 is the slot's uint16 buffer, a layout of its own: the rows of a plane are g.pitch elements
// apart, a multiple of 64 (whole tiles, and every 8-element piece 16-byte aligned), the planes and the
// frames multiples of 64 elements apart (g.off16, g.poff16, g.fstride16).  The columns [w, pitch) of a row
// are written with zeros where a stored piece reaches past w, and never read by the time scan.  state
// is the context's one frame of uint16, packed planar with the byte frame's offsets; dst the slot's
// denoised frames, packed planar bytes like the source.
// k_dn_rows: a lane per row, a wave per 64 rows, kDnRowWaves waves a workgroup.  Tile by tile along the
// row: the wave stages 64 rows x 64 source bytes in LDS as 16-byte pieces (four a row; a piece over the
// row's end byte by byte), each lane walks its own row of the tile a dword at a time and leaves P as
// uint16 pairs in a second LDS tile, and the wave stores that tile as 16-byte pieces, eight a row.  The
// tiles' rows are 17 and 33 dwords apart: ds_read_b32 / ds_write_b32 bank on (address / 4) % 32 within
// each half of the wave, and in the walk an odd stride puts a half's 32 rows on 32 banks.  (The staging writes,
// four dwords a piece and four pieces a row, are 2-way conflicted at that stride: rows r and r + 4 of a half
// meet on one bank.  Not tuned: the walk is where the time goes.)  The carry from tile to tile is a
// register.  Rows >= h and tiles' columns >= w load and store nothing.
// k_dn_cols: a lane per 8 adjacent columns (one 16-byte piece of every row), in place over P: eight
// independent chains a lane, four rows' loads in flight before their steps.  Row 0 stays as it is.
// k_dn_time: a thread per 16-byte piece of a plane's byte string, cut as k_plane_copy cuts it on the
// first frame's destination; the thread keeps its 16 states in registers over the submit's frames in
// order, loads them from `state` when the submit continues a sequence (g.cont), starts them from the
// source bytes at every segment's first frame otherwise, and stores them once at the end.  A piece over
// a row's end, and the bytes before the first and behind the last whole piece, go sample by sample.
// The bodies are __host__ __device__ functions, split at the barriers, as yadif_work and hist_count /
// hist_flush are, for tools/stage_host.hip.
struct DnGeom {
  int w, h;                 // the plane
  int pitch;                // uint16 row pitch of p16 (a multiple of 64)
  long long off, fstride, poff;        // bytes: the plane in a frame, frame stride, V from U (source, dst, state)
  long long off16, fstride16, poff16;  // the same in p16, in elements
  int nf;                   // frames of the submit
  int tab;                  // 0 luma, 1 chroma: S = tabs + tab * 8192, M = tabs + (2 + tab) * 8192
  int cont;                 // k_dn_time: the first frame continues the carried state
  int gxy;                  // workgroups per (plane, frame) (k_dn_time: per plane)
  uint32_t gxy_magic;
  uint32_t w_magic;         // ceil(2^32 / w)
};

constexpr int kDnTabLen = 8192;
constexpr int kDnRowWaves = 2;               // k_dn_rows: 128 rows a workgroup
constexpr int kDnRowThreads = 64 * kDnRowWaves;
constexpr int kDnSrcStride = 68;             // bytes between the rows of the staged source tile (17 dwords)
constexpr int kDnPStride = 66;               // uint16 between the rows of the P tile (33 dwords)
constexpr int kDnColThreads = 64;            // k_dn_cols: 512 columns a workgroup
constexpr int kDnTimeThreads = 256;          // k_dn_time: one piece a thread

__host__ __device__ __forceinline__ int dn_L(int v) { return (v << 8) + 127; }
__host__ __device__ __forceinline__ int dn_c(const int16_t *tab, int a, int b) {
  int i = 4096 + ((a - b) >> 4);
  i = i < 0 ? 0 : i > kDnTabLen - 1 ? kDnTabLen - 1 : i;
  return b + tab[i];
}

// the (plane, frame) of workgroup t of k_dn_rows / k_dn_cols and its index there; the source plane
struct DnBlock {
  int pl, f, blk;
};
__host__ __device__ __forceinline__ DnBlock dn_block(const DnGeom &g, int t) {
  const int z = deint_div(t, g.gxy_magic, g.gxy);
  DnBlock b;
  b.blk = t - z * g.gxy;
  b.pl = z >= g.nf;
  b.f = z - (b.pl ? g.nf : 0);
  return b;
}
__host__ __device__ __forceinline__ const uint8_t *dn_src_plane(const SegList &src, const DnGeom &g, int f, int pl) {
  int k = 0;
#pragma unroll
  for (int j = 1; j < kMaxSegs; j++)
    if (f >= src.f0[j]) k = j;
  return src.p[k] + (long long)(f - (k ? src.f0[k] : 0)) * g.fstride + g.off + (pl ? g.poff : 0);
}

// tile ti (columns [64 ti, 64 ti + 64)) of the wave's 64 rows -> ls (kDnRowWaves tiles of 64 x kDnSrcStride bytes)
__host__ __device__ __forceinline__ void dn_rows_stage(const SegList &src, uint8_t *ls, const DnGeom &g, int t, int tid, int ti) {
  const DnBlock B = dn_block(g, t);
  const uint8_t *s = dn_src_plane(src, g, B.f, B.pl);
  const int wave = tid >> 6, lane = tid & 63, y0 = (B.blk * kDnRowWaves + wave) * 64, x0 = 64 * ti;
  uint8_t *tile = ls + wave * 64 * kDnSrcStride;
#pragma unroll
  for (int it = 0; it < 4; it++) {
    const int p = it * 64 + lane, row = p >> 2, y = y0 + row, x = x0 + 16 * (p & 3);
    if (y >= g.h || x >= g.w) continue;
    const uint8_t *sp = s + (size_t)y * g.w + x;
    uint8_t *lp = tile + row * kDnSrcStride + 16 * (p & 3);
    if (x + 16 <= g.w) {
      const u32x4 v = *(const u32x4_a1 *)sp;
#pragma unroll
      for (int q = 0; q < 4; q++) ((uint32_t *)lp)[q] = v[q];
    } else {
#pragma unroll 1
      for (int b = 0; x + b < g.w; b++) lp[b] = sp[b];
    }
  }
}

// the lane's row of the staged tile -> its row of the P tile lp16 (kDnRowWaves tiles of 64 x kDnPStride uint16);
// carry: P[y][64 ti - 1], then P[y][the tile's last column]
__host__ __device__ __forceinline__ void dn_rows_walk(const uint8_t *ls, uint16_t *lp16, const int16_t *S, const DnGeom &g,
                                                      int t, int tid, int ti, int *carry) {
  const DnBlock B = dn_block(g, t);
  const int wave = tid >> 6, lane = tid & 63, y = (B.blk * kDnRowWaves + wave) * 64 + lane, x0 = 64 * ti;
  if (y >= g.h) return;
  const uint32_t *sr = (const uint32_t *)(ls + (wave * 64 + lane) * kDnSrcStride);
  uint32_t *pr = (uint32_t *)(lp16 + (wave * 64 + lane) * kDnPStride);
  int cy = *carry;
#pragma unroll 4
  for (int k = 0; k < 16; k++) {
    if (x0 + 4 * k >= g.w) {
      pr[2 * k] = pr[2 * k + 1] = 0u;
      continue;
    }
    const uint32_t d = sr[k];
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int x = x0 + 4 * k + j, L = dn_L((int)((d >> (8 * j)) & 255u));
      if (x >= g.w) {
        o[j] = 0u;
        continue;
      }
      cy = x ? dn_c(S, cy, L) : y ? L : dn_c(S, L, L);
      o[j] = (uint32_t)cy & 0xffffu;
    }
    pr[2 * k] = o[0] | o[1] << 16;
    pr[2 * k + 1] = o[2] | o[3] << 16;
  }
  *carry = cy;
}

// the wave's P tile -> p16, 16-byte pieces
__host__ __device__ __forceinline__ void dn_rows_store(const uint16_t *lp16, uint16_t *p16, const DnGeom &g, int t, int tid, int ti) {
  const DnBlock B = dn_block(g, t);
  uint16_t *d = p16 + (long long)B.f * g.fstride16 + g.off16 + (B.pl ? g.poff16 : 0);
  const int wave = tid >> 6, lane = tid & 63, y0 = (B.blk * kDnRowWaves + wave) * 64, x0 = 64 * ti;
#pragma unroll
  for (int it = 0; it < 8; it++) {
    const int p = it * 64 + lane, row = p >> 3, y = y0 + row, x = x0 + 8 * (p & 7);
    if (y >= g.h || x >= g.w) continue;
    const uint32_t *pr = (const uint32_t *)(lp16 + (wave * 64 + row) * kDnPStride + 8 * (p & 7));
    *(u32x4 *)(d + (size_t)y * g.pitch + x) = u32x4{pr[0], pr[1], pr[2], pr[3]};
  }
}

// a 16 KiB table into LDS, 16-byte pieces
template <int THREADS>
__device__ __forceinline__ void dn_load_tab(int16_t *lt, const int16_t *tab, int tid) {
#pragma unroll
  for (int i = 0; i < kDnTabLen * 2 / 16 / THREADS; i++) ((u32x4 *)lt)[i * THREADS + tid] = ((const u32x4 *)tab)[i * THREADS + tid];
}

__global__ __launch_bounds__(kDnRowThreads) void k_dn_rows(const SegList src, uint16_t *__restrict__ p16,
                                                           const int16_t *__restrict__ tabs, DnGeom g) {
  __shared__ __attribute__((aligned(16))) int16_t lt[kDnTabLen];
  __shared__ __attribute__((aligned(16))) uint8_t ls[kDnRowWaves * 64 * kDnSrcStride];
  __shared__ __attribute__((aligned(16))) uint16_t lp16[kDnRowWaves * 64 * kDnPStride];
  const int tid = threadIdx.x, t = blockIdx.x;
  dn_load_tab<kDnRowThreads>(lt, tabs + g.tab * kDnTabLen, tid);
  int carry = 0;
  const int ntiles = (g.w + 63) >> 6;
#pragma unroll 1
  for (int ti = 0; ti < ntiles; ti++) {
    dn_rows_stage(src, ls, g, t, tid, ti);
    __syncthreads();
    dn_rows_walk(ls, lp16, lt, g, t, tid, ti, &carry);
    __syncthreads();
    dn_rows_store(lp16, p16, g, t, tid, ti);
  }
}

__host__ __device__ __forceinline__ void dn_cols_work(uint16_t *p16, const int16_t *S, const DnGeom &g, int t, int tid) {
  const DnBlock B = dn_block(g, t);
  const int x = (B.blk * kDnColThreads + tid) * 8;
  if (x >= g.w) return;
  uint16_t *d = p16 + (long long)B.f * g.fstride16 + g.off16 + (B.pl ? g.poff16 : 0) + x;
  int v[8];
  {
    const u32x4 r = *(const u32x4 *)d;
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = (int)((r[i >> 1] >> (16 * (i & 1))) & 0xffffu);
  }
#pragma unroll 1
  for (int y = 1; y < g.h; y += 4) {
    u32x4 r[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (y + j < g.h) r[j] = *(const u32x4 *)(d + (size_t)(y + j) * g.pitch);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (y + j < g.h) {
        uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; i++) {
          v[i] = dn_c(S, v[i], (int)((r[j][i >> 1] >> (16 * (i & 1))) & 0xffffu));
          o[i >> 1] |= ((uint32_t)v[i] & 0xffffu) << (16 * (i & 1));
        }
        *(u32x4 *)(d + (size_t)(y + j) * g.pitch) = u32x4{o[0], o[1], o[2], o[3]};
      }
  }
}

__global__ __launch_bounds__(kDnColThreads) void k_dn_cols(uint16_t *p16, const int16_t *__restrict__ tabs, DnGeom g) {
  __shared__ __attribute__((aligned(16))) int16_t lt[kDnTabLen];
  dn_load_tab<kDnColThreads>(lt, tabs + g.tab * kDnTabLen, (int)threadIdx.x);
  __syncthreads();
  dn_cols_work(p16, lt, g, (int)blockIdx.x, (int)threadIdx.x);
}

// sample j of the plane through the submit's frames, one by one
__host__ __device__ inline void dn_time_sample(const SegList &src, const uint16_t *v, uint16_t *st, uint8_t *d,
                                               const int16_t *M, const DnGeom &g, int pl, int j) {
  const int row = deint_div(j, g.w_magic, g.w), col = j - row * g.w;
  const size_t vj = (size_t)row * g.pitch + col;
  int a = g.cont ? (int)st[j] : 0;
#pragma unroll 1
  for (int f = 0; f < g.nf; f++) {
    bool first = f == 0;
#pragma unroll
    for (int k = 1; k < kMaxSegs; k++) first = first || f == src.f0[k];
    if (first && !(f == 0 && g.cont)) a = dn_L(dn_src_plane(src, g, f, pl)[j]);
    a = dn_c(M, a, (int)v[(long long)f * g.fstride16 + vj]);
    d[(long long)f * g.fstride + j] = (uint8_t)(a >> 8);
  }
  st[j] = (uint16_t)a;
}

__host__ __device__ __forceinline__ void dn_time_work(const SegList &src, const uint16_t *p16, uint16_t *state, uint8_t *dst,
                                                      const int16_t *M, const DnGeom &g, int t, int tid) {
  const int pl = deint_div(t, g.gxy_magic, g.gxy), blk = t - pl * g.gxy;
  const long long po = g.off + (pl ? g.poff : 0);
  const uint16_t *v = p16 + g.off16 + (pl ? g.poff16 : 0);
  uint16_t *st = state + po;
  uint8_t *d = dst + po;  // the plane in the first frame
  const int w = g.w, nb = w * g.h;
  const int head = imin((int)(-(uintptr_t)d & 15), nb);
  const int nv = (nb - head) >> 4;
  const int kp = blk * kDnTimeThreads + tid;
  if (kp < nv) {
    const int j = head + 16 * kp;
    const int row = deint_div(j, g.w_magic, w), col = j - row * w;
    if (col + 16 > w) {  // over a row end (rolled: 16 / w of the pieces)
#pragma unroll 1
      for (int b = 0; b < 16; b++) dn_time_sample(src, v, st, d, M, g, pl, j + b);
    } else {
      const size_t vj = (size_t)row * g.pitch + col;
      int a[16];
      if (g.cont) {
        const u32x4 s0 = *(const u32x4_a1 *)(st + j), s1 = *(const u32x4_a1 *)(st + j + 8);
#pragma unroll
        for (int b = 0; b < 8; b++) {
          a[b] = (int)((s0[b >> 1] >> (16 * (b & 1))) & 0xffffu);
          a[8 + b] = (int)((s1[b >> 1] >> (16 * (b & 1))) & 0xffffu);
        }
      } else {
#pragma unroll
        for (int b = 0; b < 16; b++) a[b] = 0;
      }
#pragma unroll 1
      for (int f = 0; f < g.nf; f++) {
        bool first = f == 0;
#pragma unroll
        for (int k = 1; k < kMaxSegs; k++) first = first || f == src.f0[k];
        const uint16_t *vf = v + (long long)f * g.fstride16 + vj;
        const u32x4 v0 = *(const u32x4_a1 *)vf, v1 = *(const u32x4_a1 *)(vf + 8);
        if (first && !(f == 0 && g.cont)) {
          const u32x4 s = *(const u32x4_a1 *)(dn_src_plane(src, g, f, pl) + j);
#pragma unroll
          for (int b = 0; b < 16; b++) a[b] = dn_L((int)((s[b >> 2] >> (8 * (b & 3))) & 255u));
        }
        uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; b++) {
          const u32x4 &vv = b < 8 ? v0 : v1;
          a[b] = dn_c(M, a[b], (int)((vv[(b & 7) >> 1] >> (16 * (b & 1))) & 0xffffu));
          o[b >> 2] |= (((uint32_t)a[b] >> 8) & 255u) << (8 * (b & 3));
        }
        *(u32x4_a1 *)(d + (long long)f * g.fstride + j) = u32x4{o[0], o[1], o[2], o[3]};
      }
      uint32_t o[8];
#pragma unroll
      for (int b = 0; b < 8; b++) o[b] = ((uint32_t)a[2 * b] & 0xffffu) | ((uint32_t)a[2 * b + 1] & 0xffffu) << 16;
      *(u32x4_a1 *)(st + j) = u32x4{o[0], o[1], o[2], o[3]};
      *(u32x4_a1 *)(st + j + 8) = u32x4{o[4], o[5], o[6], o[7]};
    }
  }
  if (blk == 0 && tid < 16) {
    const int a = tid, b = head + 16 * nv + tid;
    if (a < head) dn_time_sample(src, v, st, d, M, g, pl, a);
    if (b < nb) dn_time_sample(src, v, st, d, M, g, pl, b);
  }
}

__global__ __launch_bounds__(kDnTimeThreads) void k_dn_time(const SegList src, const uint16_t *__restrict__ p16,
                                                            uint16_t *state, uint8_t *__restrict__ dst,
                                                            const int16_t *__restrict__ tabs, DnGeom g) {
  __shared__ __attribute__((aligned(16))) int16_t lt[kDnTabLen];
  dn_load_tab<kDnTimeThreads>(lt, tabs + (2 + g.tab) * kDnTabLen, (int)threadIdx.x);
  __syncthreads();
  dn_time_work(src, p16, state, dst, lt, g, (int)blockIdx.x, (int)threadIdx.x);
}

}  // namespace mjg
