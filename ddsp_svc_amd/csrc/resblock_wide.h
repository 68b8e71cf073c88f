// NSF-HiFiGAN ResBlock1 at 128 and 256 channels (nsf_hifigan/models.py:37-68): the wide form, ONE convolution per launch, two
// launches per pair, f32 MFMA GEMMs.  Included from api.hip only, behind resblock.h (whose row_stride and lrelu it shares).
//
// resblock.h keeps the x image [C][rs] and the intermediate [C][144] of a tile in LDS; at C = 128 that is already 72 KB.  Here the
// intermediate of a pair goes through memory: at C = 128, k = 3 an unfused pair still does 1 536 FLOP per output element against
// 20 bytes moved, 77 FLOP / B against a machine balance near 20, so it stays matrix-bound, and without the fusion there is no
// halo to recompute: a workgroup keeps all 128 columns of its tile for every k.
//
// k_conv_wide<C, K, MODE>: y = conv1d(lrelu(src), w, b, dilation d, 'same' zero padding), then the epilogue of MODE.
//   grid (ceil(T / 128), C / 64, utterances), 4 waves; a workgroup makes 64 output rows x 128 columns, wave v the columns
//   [32 v, 32 v + 32) as 4 row blocks x 2 column fragments (conv_tile's shape at C = 64: 32 accumulator registers).
//   The input channels go through LDS in chunks of 64: lrelu(src) for the 128 + (K - 1) d columns the tile reaches, zeros outside
//   [0, T) -- so every convolution pads ITS OWN input --, [64][rs] with rs = 16 mod 32 (resblock.h's conflict-free stride).
//   Each chunk is ONE chain of 16 K MFMA steps (at most 704 products, as at C = 64); the chunks' partial sums are added in chunk
//   order afterwards.  One chain over all C K products (2 816 at C = 256, k = 11) lands at 5.6 x the error of torch's own
//   float32 conv, outside the project's bar of 4; per-chunk partials land at 1.7 x.  Chunk 0's chain starts at
//   the bias.  The order depends on (C, K, d) only, never on the batch.
//   MODE 0 (the first conv of a pair): store.  The next launch applies lrelu on its way into LDS.
//   MODE 1 (the second): + res (the pair's input), then y = (acc_in + y) / div as in resblock.h: acc_in optional (may be y: each
//   element is read and written by the same lane), div = 0: no division, otherwise a true division.
// Weights: packed once on the host in fragment order per (64-row output slice, 64-channel chunk), [slice][chunk][16-row block]
// [k-step][lane]; one coalesced 256-byte read per fragment, from L2, never staged in LDS.
//
// LDS: 64 rs floats <= 64 KB, so a dilation is accepted while 64 (16 + 32 ceil((112 + (K - 1) d) / 32)) <= 16384: d <= 11 at
// K = 11, 18 at 7, 56 at 3 -- the range resblock.h has at C = 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "resblock.h"
#include "tuning.h"

namespace ddsp {
namespace resblock_wide {

using resblock::f32x4r;
using resblock::kLdsFloats;
using resblock::kMaxPairs;
using resblock::kThreads;
using resblock::lrelu;
using resblock::row_stride;

constexpr int kTile = 128;                             // output columns per workgroup, for every k
constexpr int kChunk = 64;                             // input channels per LDS image and per summation chain
constexpr int kSlice = 64;                             // output rows per workgroup

inline bool shape_ok(int C, int k) { return (C == 128 || C == 256) && (k == 3 || k == 7 || k == 11); }
inline bool dilation_ok(int k, long d) { return d >= 1 && d <= kLdsFloats && (long)kChunk * row_stride(k, d) <= kLdsFloats; }
inline size_t pair_floats(int C, int k) { return 2 * (size_t)C * C * k + 2 * (size_t)C; }

struct Args {
  const float* src; float* y;                          // [B, C, T] contiguous; y must not be src
  const float* A; const float* bias;                   // this conv's packed fragments and its [C] bias
  const float* res;                                    // MODE 1: the pair's input
  const float* acc_in; float div;                      // MODE 1: y = (acc_in + y) / div
  long T; long b0;
  int d, rs;
};

template <int C, int K, int MODE>
__global__ __launch_bounds__(kThreads) void k_conv_wide(Args a) {
  HIP_DYNAMIC_SHARED(float, lds)
  constexpr int NC = C / kChunk, KS = 16 * K, H = (K - 1) / 2;
  constexpr size_t kFrag = (size_t)4 * KS * 64;        // floats of one (slice, chunk): 4 row blocks of KS fragments
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slice = blockIdx.y;
  const long b = a.b0 + blockIdx.z;
  const long t0 = (long)blockIdx.x * kTile;
  const long T = a.T;
  const int d = a.d, rs = a.rs;
  const int xw = kTile + (K - 1) * d;                  // <= rs
  const long p0 = t0 - (long)H * d;                    // src column of LDS column 0
  const float* sb = a.src + b * C * T;
  const float* bias = a.bias + kSlice * slice;

  f32x4r tot[4][2], acc[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[m][0][r] = acc[m][1][r] = bias[16 * m + 4 * (lane >> 4) + r];
      tot[m][0][r] = tot[m][1][r] = 0.f;
    }

  // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
  const float* pb = lds + (lane >> 4) * rs + 32 * wave + (lane & 15);
  for (int c = 0; c < NC; ++c) {
    if (c) __syncthreads();                            // every wave is done with the chunk before
    const float* sc = sb + (long)c * kChunk * T;
    for (int ci = wave; ci < kChunk; ci += kThreads / 64)
      for (int m = lane; m < xw; m += 64) {
        const long p = p0 + m;
        lds[ci * rs + m] = (p >= 0 && p < T) ? lrelu(sc[ci * T + p]) : 0.f;
      }
    __syncthreads();

    const float* pa = a.A + ((size_t)slice * NC + c) * kFrag + lane;
    for (int j = 0; j < K; ++j) {
      const float* pbj = pb + j * d;
#pragma unroll 4
      for (int cs = 0; cs < 16; ++cs) {
        const int s = j * 16 + cs;
        const float v0 = pbj[4 * cs * rs], v1 = pbj[4 * cs * rs + 16];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const float av = pa[(m * KS + s) * 64];
          acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, v0, acc[m][0], 0, 0, 0);
          acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, v1, acc[m][1], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        tot[m][n] += acc[m][n];
        acc[m][n] = f32x4r{0.f, 0.f, 0.f, 0.f};
      }
  }

  // D: col = l & 15, row = 4 (l >> 4) + r
  const long off = (b * C + (long)kSlice * slice) * T;
  float* yb = a.y + off;
  const float* rb = MODE ? a.res + off : nullptr;
  const float* ab = MODE && a.acc_in ? a.acc_in + off : nullptr;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const long t = t0 + 32 * wave + 16 * n + (lane & 15);
      if (t >= T) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long e = (16 * m + 4 * (lane >> 4) + r) * T + t;
        float v = tot[m][n][r];
        if (MODE) {
          v = v + rb[e];
          if (ab) v = ab[e] + v;
          if (a.div != 0.f) v = __fdiv_rn(v, a.div);
        }
        yb[e] = v;
      }
    }
}

template <int C, int K, int MODE>
inline void launch_conv_ckm(Args a, int B, hipStream_t st) {
  const long tiles = (a.T + kTile - 1) / kTile;
  const size_t lds = (size_t)kChunk * a.rs * sizeof(float);
  const long split = batch_split();
  for (long b0 = 0; b0 < B; b0 += split) {
    a.b0 = b0;
    const long nb = B - b0 < split ? B - b0 : split;
    hipLaunchKernelGGL((k_conv_wide<C, K, MODE>), dim3((unsigned)tiles, C / kSlice, (unsigned)nb), dim3(kThreads), lds, st, a);
  }
}

template <int C, int MODE>
inline void launch_conv_cm(const Args& a, int B, int k, hipStream_t st) {
  if (k == 3) launch_conv_ckm<C, 3, MODE>(a, B, st);
  else if (k == 7) launch_conv_ckm<C, 7, MODE>(a, B, st);
  else launch_conv_ckm<C, 11, MODE>(a, B, st);
}

template <int MODE>
inline void launch_conv(const Args& a, int B, int C, int k, hipStream_t st) {
  if (C == 128) launch_conv_cm<128, MODE>(a, B, k, st);
  else launch_conv_cm<256, MODE>(a, B, k, st);
}

}  // namespace resblock_wide

// ---- host side ---------------------------------------------------------------------------------------------------------------

size_t resblock_wide_pack_bytes(int C, int k, int pairs) {
  if (!resblock_wide::shape_ok(C, k) || pairs < 1 || pairs > resblock_wide::kMaxPairs) return 0;
  return pairs * resblock_wide::pair_floats(C, k) * sizeof(float);
}

// w: [2 pairs][C][C][k] (convs1[0], convs2[0], convs1[1], ...), b: [2 pairs][C], both host memory; out: host memory.
// Per pair: the fragments of conv 1, of conv 2, then b1, b2.  A conv's fragments are [C / 64 slices][C / 64 chunks][4][16 k][64]:
// element (sl, c, m, s, l) is W[64 sl + 16 m + (l & 15)][64 c + 4 (s mod 16) + (l >> 4)][s / 16].
void resblock_wide_pack(const float* w, const float* b, int C, int k, int pairs, float* out) {
  const int NC = C / resblock_wide::kChunk, KS = 16 * k;
  const size_t wn = (size_t)C * C * k;
  for (int p = 0; p < pairs; ++p) {
    float* o = out + p * resblock_wide::pair_floats(C, k);
    for (int c = 0; c < 2; ++c) {
      const float* W = w + (2 * p + c) * wn;
      float* A = o + c * wn;
      for (int sl = 0; sl < NC; ++sl)
        for (int ch = 0; ch < NC; ++ch)
          for (int m = 0; m < 4; ++m)
            for (int s = 0; s < KS; ++s)
              for (int l = 0; l < 64; ++l) {
                const int co = 64 * sl + 16 * m + (l & 15), ci = 64 * ch + 4 * (s % 16) + (l >> 4), j = s / 16;
                A[((((size_t)sl * NC + ch) * 4 + m) * KS + s) * 64 + l] = W[((size_t)co * C + ci) * k + j];
              }
      for (int i = 0; i < C; ++i) o[2 * wn + c * C + i] = b[(size_t)(2 * p + c) * C + i];
    }
  }
}

// the intermediate of a pair, and between the pairs one buffer for two pairs, two (ping-pong) beyond
size_t resblock_wide_ws_bytes(long B, int C, long T, int pairs) {
  const int n = pairs <= 1 ? 1 : pairs == 2 ? 2 : 3;
  return (size_t)n * B * C * T * sizeof(float);
}

// 2 pairs launches per 65 535 utterances.  packed: resblock_wide_pack's floats on the device.
void launch_resblock1_wide(const float* x, float* y, const float* packed, int B, int C, long T, int k, const int* dil, int pairs,
                           const float* acc_in, float div, float* ws, hipStream_t st) {
  using namespace resblock_wide;
  const size_t wn = (size_t)C * C * k, act = (size_t)B * C * T;
  float* mid = ws;
  const float* src = x;
  for (int p = 0; p < pairs; ++p) {
    const bool last = p == pairs - 1;
    const float* o = packed + p * pair_floats(C, k);
    Args a;
    a.src = src; a.y = mid;
    a.A = o; a.bias = o + 2 * wn;
    a.res = nullptr; a.acc_in = nullptr; a.div = 0.f;
    a.T = T; a.b0 = 0;
    a.d = dil[p]; a.rs = (int)row_stride(k, dil[p]);
    launch_conv<0>(a, B, C, k, st);
    a.src = mid; a.y = last ? y : ws + (size_t)(1 + (p & 1)) * act;
    a.A = o + wn; a.bias = o + 2 * wn + C;
    a.res = src;
    a.acc_in = last ? acc_in : nullptr;
    a.div = last ? div : 0.f;
    a.d = 1; a.rs = (int)row_stride(k, 1);
    launch_conv<1>(a, B, C, k, st);
    src = a.y;
  }
}

}  // namespace ddsp
