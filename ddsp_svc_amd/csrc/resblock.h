// NSF-HiFiGAN ResBlock1 (nsf_hifigan/models.py:37-68): one conv pair per launch, both convolutions as f32 MFMA GEMMs, the
// intermediate kept in LDS.  Included from api.hip only (one translation unit holds the kernels).
//
// A pair, for C channels, k (odd) taps and dilation d:
//     xt = conv1d(lrelu(x), w1, b1, dilation = d, padding = (k - 1) / 2 d)
//     y  = conv1d(lrelu(xt), w2, b2, dilation = 1, padding = (k - 1) / 2) + x      (then the MRF epilogue, below)
// Each conv zero-pads ITS OWN input: lrelu(xt) is 0 at columns outside [0, T), not lrelu(b1 + the conv of zeros).
//
// A convolution is the GEMM D[co][t] = sum over (j, ci) of W[co][ci][j] X[ci][t + j d]: M = C output channels, N = time, the
// sum over C k products.  v_mfma_f32_16x16x4_f32 takes four consecutive input channels of one tap per instruction; time runs
// along the lanes, so the B fragment of tap j is the LDS row shifted by j d floats, whatever d is.
//
// k_resblock_pair<C, K>: grid (ceil(T / TT), B), 4 waves, TT = 128 - (K - 1) output columns per workgroup.
//   1. lrelu(x) for the TT + (K - 1)(d + 1) columns the tile reaches, zeros outside [0, T) -> LDS [C][rs].  rs = 16 mod 32: the
//      lane quarters of a B fragment read rows 1 apart, 16 banks apart, so the 32 lanes of a half wave hit 32 banks.
//   2. conv 1 on 128 columns (the tile and conv 2's halo): wave v takes columns [32 v, 32 v + 32) as two 16-column fragments for
//      every 16-row block of output channels, so each weight fragment it loads feeds two independent accumulators (C / 16 x 2
//      chains per wave).  Accumulators start at the bias.
//   3. barrier; lrelu and the zeroing of columns outside [0, T); the intermediate goes over the x image, [C][144].
//   4. conv 2 on the tile; + x (read again from memory: it is in cache), the epilogue, store.
// Weights come from a table packed once on the host in fragment order ([conv][16-row block][k-step][lane]): one coalesced
// 256-byte read per fragment, the same for all four waves of a workgroup and all workgroups.
//
// Epilogue of the last pair of a block (the MRF sum, models.py:253-259): y = (acc_in + y) / div, acc_in optional (may be y:
// each element is read and written by the same lane), div = 0: no division.  A true division, as the reference's xs / 3.
//
// LDS: C rs floats, at most 64 KB, so a dilation is accepted while C (16 + 32 ceil((112 + (K - 1) d) / 32)) <= 16384 floats.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "tuning.h"

namespace ddsp {
namespace resblock {

typedef float f32x4r __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kNW = 128;                               // columns of the intermediate per workgroup
constexpr int kRS2 = 144;                              // row stride of the intermediate: 16 mod 32, >= kNW + 10
constexpr int kLdsFloats = 16384;
constexpr int kMaxPairs = 8;

inline bool shape_ok(int C, int k) { return (C == 16 || C == 32 || C == 64) && (k == 3 || k == 7 || k == 11); }
inline int tile_of(int k) { return kNW - (k - 1); }
// row stride of the x image: >= 128 + (k - 1) d and 16 mod 32 (never below kRS2)
inline long row_stride(int k, long d) { return (kNW + (k - 1) * d - 16 + 31) / 32 * 32 + 16; }
inline bool dilation_ok(int C, int k, long d) { return d >= 1 && d <= kLdsFloats && (long)C * row_stride(k, d) <= kLdsFloats; }
inline size_t pair_floats(int C, int k) { return 2 * (size_t)C * C * k + 2 * (size_t)C; }

struct Args {
  const float* x; float* y;                            // [B, C, T] contiguous
  const float* a1; const float* a2;                    // packed weight fragments of the two convs
  const float* b1; const float* b2;                    // [C] biases
  const float* acc_in; float div;                      // epilogue: y = (acc_in + y) / div
  long T; long b0;
  int d, rs;
};

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : v * 0.1f; }

// acc[m][n][r] = bias[16 m + 4 (lane >> 4) + r] + sum over taps j and channels ci of W[.][ci][j] src[ci rs + col + j d],
// col = 32 wave + 16 n + (lane & 15)
template <int C, int K>
__device__ __forceinline__ void conv_tile(const float* src, int rs, int d, const float* A, const float* bias, int lane,
                                          int wave, f32x4r (&acc)[C / 16][2]) {
  constexpr int MT = C / 16, CS = C / 4, KS = CS * K;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[m][0][r] = acc[m][1][r] = bias[16 * m + 4 * (lane >> 4) + r];
  // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
  const float* pb = src + (lane >> 4) * rs + 32 * wave + (lane & 15);
  const float* pa = A + lane;
  for (int j = 0; j < K; ++j) {
    const float* pbj = pb + j * d;
#pragma unroll 4
    for (int cs = 0; cs < CS; ++cs) {
      const int s = j * CS + cs;
      const float v0 = pbj[4 * cs * rs], v1 = pbj[4 * cs * rs + 16];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const float av = pa[(m * KS + s) * 64];
        acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, v0, acc[m][0], 0, 0, 0);
        acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, v1, acc[m][1], 0, 0, 0);
      }
    }
  }
}

template <int C, int K>
__global__ __launch_bounds__(kThreads) void k_resblock_pair(Args a) {
  HIP_DYNAMIC_SHARED(float, lds)
  constexpr int MT = C / 16, H2 = (K - 1) / 2, TT = kNW - (K - 1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = a.b0 + blockIdx.y;
  const long t0 = (long)blockIdx.x * TT;
  const long T = a.T;
  const float* xb = a.x + b * C * T;
  const int d = a.d, rs = a.rs;
  const int xw = kNW + (K - 1) * d;                    // <= rs
  const long p0 = t0 - H2 - (long)H2 * d;              // x column of LDS column 0

  for (int ci = wave; ci < C; ci += kThreads / 64)
    for (int m = lane; m < xw; m += 64) {
      const long p = p0 + m;
      lds[ci * rs + m] = (p >= 0 && p < T) ? lrelu(xb[ci * T + p]) : 0.f;
    }
  __syncthreads();

  f32x4r acc[MT][2];
  conv_tile<C, K>(lds, rs, d, a.a1, a.b1, lane, wave, acc);
  __syncthreads();                                     // every wave is done with the x image
  // D: col = l & 15, row = 4 (l >> 4) + r
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int col = 32 * wave + 16 * n + (lane & 15);
      const long u = t0 - H2 + col;
      const bool in = u >= 0 && u < T;
#pragma unroll
      for (int r = 0; r < 4; ++r) lds[(16 * m + 4 * (lane >> 4) + r) * kRS2 + col] = in ? lrelu(acc[m][n][r]) : 0.f;
    }
  __syncthreads();

  // columns [128, 128 + K - 1) of a row hold what the x image left there: only outputs q >= TT read them, and those are dropped
  conv_tile<C, K>(lds, kRS2, 1, a.a2, a.b2, lane, wave, acc);
  float* yb = a.y + b * C * T;
  const float* ab = a.acc_in ? a.acc_in + b * C * T : nullptr;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int q = 32 * wave + 16 * n + (lane & 15);
      const long t = t0 + q;
      if (q >= TT || t >= T) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long e = (16 * m + 4 * (lane >> 4) + r) * T + t;
        float v = acc[m][n][r] + xb[e];
        if (ab) v = ab[e] + v;
        if (a.div != 0.f) v = __fdiv_rn(v, a.div);
        yb[e] = v;
      }
    }
}

template <int C, int K>
inline void launch_pair_ck(Args a, int B, hipStream_t st) {
  const long tiles = (a.T + tile_of(K) - 1) / tile_of(K);
  const size_t lds = (size_t)C * a.rs * sizeof(float);
  const long split = batch_split();
  for (long b0 = 0; b0 < B; b0 += split) {
    a.b0 = b0;
    const long nb = B - b0 < split ? B - b0 : split;
    hipLaunchKernelGGL((k_resblock_pair<C, K>), dim3((unsigned)tiles, (unsigned)nb), dim3(kThreads), lds, st, a);
  }
}

template <int C>
inline void launch_pair_c(const Args& a, int B, int k, hipStream_t st) {
  if (k == 3) launch_pair_ck<C, 3>(a, B, st);
  else if (k == 7) launch_pair_ck<C, 7>(a, B, st);
  else launch_pair_ck<C, 11>(a, B, st);
}

}  // namespace resblock

// ---- host side ---------------------------------------------------------------------------------------------------------------

size_t resblock_pack_bytes(int C, int k, int pairs) {
  if (!resblock::shape_ok(C, k) || pairs < 1 || pairs > resblock::kMaxPairs) return 0;
  return pairs * resblock::pair_floats(C, k) * sizeof(float);
}

// w: [2 pairs][C][C][k] (convs1[0], convs2[0], convs1[1], ...), b: [2 pairs][C], both host memory; out: host memory.
// Per pair: the fragments of conv 1, of conv 2 ([C / 16][C k / 4][64]: element (m, s, l) is W[16 m + (l & 15)][4 (s mod C / 4)
// + (l >> 4)][s / (C / 4)]), then b1, b2.
void resblock_pack(const float* w, const float* b, int C, int k, int pairs, float* out) {
  const int CS = C / 4, KS = CS * k, MT = C / 16;
  const size_t wn = (size_t)C * C * k;
  for (int p = 0; p < pairs; ++p) {
    float* o = out + p * resblock::pair_floats(C, k);
    for (int c = 0; c < 2; ++c) {
      const float* W = w + (2 * p + c) * wn;
      float* A = o + c * wn;
      for (int m = 0; m < MT; ++m)
        for (int s = 0; s < KS; ++s)
          for (int l = 0; l < 64; ++l) {
            const int co = 16 * m + (l & 15), ci = 4 * (s % CS) + (l >> 4), j = s / CS;
            A[((size_t)m * KS + s) * 64 + l] = W[((size_t)co * C + ci) * k + j];
          }
      for (int i = 0; i < C; ++i) o[2 * wn + c * C + i] = b[(size_t)(2 * p + c) * C + i];
    }
  }
}

// buffers between the pairs of a block: none for one pair, one for two, two (ping-pong) beyond
size_t resblock_ws_bytes(long B, int C, long T, int pairs) {
  const int n = pairs <= 1 ? 0 : pairs == 2 ? 1 : 2;
  return (size_t)n * B * C * T * sizeof(float);
}

// pairs launches per 65 535 utterances.  packed: resblock_pack's floats on the device.
void launch_resblock1(const float* x, float* y, const float* packed, int B, int C, long T, int k, const int* dil, int pairs,
                      const float* acc_in, float div, float* ws, hipStream_t st) {
  using namespace resblock;
  const size_t wn = (size_t)C * C * k;
  const float* src = x;
  for (int p = 0; p < pairs; ++p) {
    const bool last = p == pairs - 1;
    const float* o = packed + p * pair_floats(C, k);
    Args a;
    a.x = src;
    a.y = last ? y : ws + (size_t)(p & 1) * B * C * T;
    a.a1 = o; a.a2 = o + wn; a.b1 = o + 2 * wn; a.b2 = o + 2 * wn + C;
    a.acc_in = last ? acc_in : nullptr;
    a.div = last ? div : 0.f;
    a.T = T; a.b0 = 0;
    a.d = dil[p]; a.rs = (int)row_stride(k, dil[p]);
    if (C == 16) launch_pair_c<16>(a, B, k, st);
    else if (C == 32) launch_pair_c<32>(a, B, k, st);
    else launch_pair_c<64>(a, B, k, st);
    src = a.y;
  }
}

}  // namespace ddsp
