// What lies between and behind the residual blocks of the NSF-HiFiGAN generator (nsf_hifigan/models.py:249-252, :260-262): the
// upsampling seam of a stage and the output head.  Included from api.hip only (one translation unit holds the kernels).
//
// The seam, for CO output channels, CI = 2 CO input channels, stride u, k = 2 u taps, p = u / 2, noise stride s:
//     y[b, co, t] = bu[co] + sum over (ci, j) of lrelu_0.1(x)[b, ci, q] Wu[ci, co, j]       over t = u q - p + j  (ConvTranspose1d)
//                 + bn[co] + sum over m of src[b, t s - s / 2 + m] Wn[co, 0, m]              (Conv1d(1, CO, 2 s, s, s / 2); s = 1:
//                                                                                            Conv1d(1, CO, 1)), zeros outside
// With k = 2 u an output column t = u q + r has exactly two taps: j0 = (r + p) mod u on input q + sh, sh = (r + p) div u, and
// j0 + u on input q + sh - 1.  Per phase r that is a GEMM with M = CO, N = input columns and a sum over 2 CI products, on
// v_mfma_f32_16x16x4_f32 as conv_tile of resblock.h: time along the lanes, the B fragment an LDS row read at a one-column shift.
//
// k_upsample_seam<CO, U>: grid (ceil(Tin / TQ), B), 4 waves, TQ = 64 NF input columns per workgroup.
//   1. lrelu(x) of CK = min(CI, 64) input channels for the TQ columns and one halo column per side, zeros outside [0, Tin) ->
//      LDS [CK][rs], rs = TQ + 16 = 16 mod 32 (the lane quarters of a B fragment read rows 1 apart, 16 banks apart).  CI = 128
//      takes two such rounds: the image stays within 37 KB.  The tile's slice of src (TQ U s + s samples, zeros outside [0, L))
//      and the noise weights are staged once beside it.
//   2. wave v takes NF 16-column fragments; for every phase it keeps an accumulator per 16-row block, CO / 16 x U x NF chains
//      started at bu + bn.  The three B fragments of a k-step (columns q - 1, q, q + 1) feed all 2 U taps.
//   3. the noise conv: at most 8 vector FMAs per output from the staged slice.
//   4. a lane holds the U phases of its column, i.e. U consecutive output samples of a row: one 8 / 16 / 32-byte store per row,
//      and the 16 lanes of a fragment row write 16 U consecutive floats.  No pass of the output through LDS.
// Weights come from a table packed once on the host in fragment order ([phase][tap][16-row block][k-step][lane]), then bu + bn,
// then the noise taps in rows of 9 floats.
//
// The head: y[b, 0, t] = tanh(bp + sum over (ci, j < 7) of lrelu_slope(x)[b, ci, t + j - 3] Wp[0, ci, j]), zeros outside [0, T).
// One output channel leaves the matrix pipe nothing to do: k_output_head<C>, grid (ceil(T / 1024), B), 256 threads of 4 outputs.
// Four rows at a time go through LDS (coalesced reads, lrelu applied, a halo of 3 padded to 4 so that a thread's twelve values
// are three 16-byte LDS reads); the weights are uniform loads.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "tuning.h"

namespace ddsp {
namespace gentail {

typedef float f32x4t __attribute__((ext_vector_type(4)));
typedef float f32x2t __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr int kNoiseRow = 9;                           // row stride of the staged noise taps: rows 4 apart land on banks 4 apart
constexpr int kHeadTile = 1024;                        // outputs per workgroup of the head
constexpr int kHeadRows = 4;                           // channels staged at a time
constexpr int kHeadRS = kHeadTile + 8;                 // LDS column c is sample t0 - 4 + c
constexpr int kHeadTaps = 7;

inline bool seam_shape_ok(int CO, int u, int s) {
  return (CO == 16 || CO == 32 || CO == 64) && (u == 2 || u == 4 || u == 8) && (s == 1 || s == 2 || s == 4);
}
// fragments per wave: two wherever CO / 16 x U x 2 accumulators stay within 128 registers
constexpr int seam_nf(int CO, int u) { return (CO / 16) * u > 16 ? 1 : 2; }
inline int seam_tile(int CO, int u) { return 64 * seam_nf(CO, u); }
inline int noise_taps(int s) { return s > 1 ? 2 * s : 1; }
inline size_t seam_pack_floats(int CO, int u) { return (size_t)2 * CO * CO * 2 * u + CO + (size_t)kNoiseRow * CO; }
inline bool head_shape_ok(int C) { return C == 16 || C == 32 || C == 64; }

struct SeamArgs {
  const float* x; const float* src; float* y;          // [B, 2 CO, Tin], [B, s U Tin], [B, CO, U Tin] contiguous
  const float* packed;
  long Tin; long b0;
  int s; int vec;                                      // vec: y is aligned for the U-float stores
};

__device__ __forceinline__ float lrelu01(float v) { return v > 0.f ? v : v * 0.1f; }

template <int CO, int U>
__global__ __launch_bounds__(kThreads) void k_upsample_seam(SeamArgs a) {
  HIP_DYNAMIC_SHARED(float, lds)
  constexpr int CI = 2 * CO, MT = CO / 16, KS = CI / 4, NF = seam_nf(CO, U), TQ = 64 * NF, RS = TQ + 16;
  constexpr int CK = CI < 64 ? CI : 64, P = U / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = a.b0 + blockIdx.y;
  const long q0 = (long)blockIdx.x * TQ;
  const long Tin = a.Tin, Tout = Tin * U;
  const int s = a.s, ks = s > 1 ? 2 * s : 1, off = s > 1 ? s / 2 : 0;
  const long L = Tout * s;
  float* img = lds;                                    // [CK][RS]: column c is input q0 - 1 + c
  float* wn = lds + CK * RS;                           // [CO][kNoiseRow]
  float* sl = wn + CO * kNoiseRow;                     // [TQ U s + ks - s]: element c is src[q0 U s - off + c]
  const float* A = a.packed;
  const float* bias = A + (size_t)CI * CO * 2 * U;
  const float* xb = a.x + b * CI * Tin;

  for (int i = tid; i < CO * kNoiseRow; i += kThreads) wn[i] = bias[CO + i];
  {
    const float* sb = a.src + b * L;
    const long p0 = q0 * U * s - off;
    const int n = TQ * U * s + ks - s;
    for (int i = tid; i < n; i += kThreads) {
      const long p = p0 + i;
      sl[i] = (p >= 0 && p < L) ? sb[p] : 0.f;
    }
  }

  f32x4t acc[MT][U][NF];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float bv = bias[16 * m + 4 * (lane >> 4) + r];
#pragma unroll
      for (int ph = 0; ph < U; ++ph)
#pragma unroll
        for (int n = 0; n < NF; ++n) acc[m][ph][n][r] = bv;
    }

  const int ql = 16 * NF * wave + (lane & 15);         // the lane's column of fragment 0; fragment n is 16 n further
  for (int c0 = 0; c0 < CI; c0 += CK) {
    if (c0) __syncthreads();                           // every wave is done with the previous channels
    for (int ci = wave; ci < CK; ci += kThreads / 64)
      for (int c = lane; c < TQ + 2; c += 64) {
        const long q = q0 - 1 + c;
        img[ci * RS + c] = (q >= 0 && q < Tin) ? lrelu01(xb[(c0 + ci) * Tin + q]) : 0.f;
      }
    __syncthreads();
    // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
    const float* pb = img + (lane >> 4) * RS + ql;
    const float* pa = A + (size_t)(c0 / 4) * 64 + lane;
#pragma unroll 2
    for (int cs = 0; cs < CK / 4; ++cs) {
      float v[NF][3];                                  // inputs q - 1, q, q + 1
#pragma unroll
      for (int n = 0; n < NF; ++n)
#pragma unroll
        for (int dlt = 0; dlt < 3; ++dlt) v[n][dlt] = pb[4 * cs * RS + 16 * n + dlt];
#pragma unroll
      for (int ph = 0; ph < U; ++ph) {
        const int sh = (ph + P) / U;                   // tap j0 reads input q + sh, tap j0 + u input q + sh - 1
#pragma unroll
        for (int tap = 0; tap < 2; ++tap)
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const float av = pa[(((size_t)(ph * 2 + tap) * MT + m) * KS + cs) * 64];
#pragma unroll
            for (int n = 0; n < NF; ++n)
              acc[m][ph][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, v[n][1 + sh - tap], acc[m][ph][n], 0, 0, 0);
          }
      }
    }
  }

  // the noise conv: y[co][u q + ph] += sum over mm of src[(u q + ph) s - off + mm] Wn[co][mm]
  for (int mm = 0; mm < ks; ++mm) {
    float sv[NF][U];
#pragma unroll
    for (int n = 0; n < NF; ++n)
#pragma unroll
      for (int ph = 0; ph < U; ++ph) sv[n][ph] = sl[((ql + 16 * n) * U + ph) * s + mm];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float w = wn[(16 * m + 4 * (lane >> 4) + r) * kNoiseRow + mm];
#pragma unroll
        for (int n = 0; n < NF; ++n)
#pragma unroll
          for (int ph = 0; ph < U; ++ph) acc[m][ph][n][r] = fmaf(sv[n][ph], w, acc[m][ph][n][r]);
      }
  }

  // D: col = l & 15, row = 4 (l >> 4) + r.  The lane's U phases of a row are U consecutive samples.
  float* yb = a.y + b * CO * Tout;
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    const long q = q0 + ql + 16 * n;
    if (q >= Tin) continue;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* o = yb + (long)(16 * m + 4 * (lane >> 4) + r) * Tout + q * U;
        if (a.vec) {
          if (U == 2) {
            f32x2t w2 = {acc[m][0][n][r], acc[m][1][n][r]};
            *reinterpret_cast<f32x2t*>(o) = w2;
          } else {
#pragma unroll
            for (int h = 0; h < U / 4; ++h) {
              f32x4t w4 = {acc[m][(4 * h) % U][n][r], acc[m][(4 * h + 1) % U][n][r], acc[m][(4 * h + 2) % U][n][r],
                           acc[m][(4 * h + 3) % U][n][r]};
              *reinterpret_cast<f32x4t*>(o + 4 * h) = w4;
            }
          }
        } else {
#pragma unroll
          for (int ph = 0; ph < U; ++ph) o[ph] = acc[m][ph][n][r];
        }
      }
  }
}

template <int CO, int U>
inline size_t seam_lds_bytes(int s) {
  constexpr int CI = 2 * CO, TQ = 64 * seam_nf(CO, U), CK = CI < 64 ? CI : 64;
  return ((size_t)CK * (TQ + 16) + (size_t)CO * kNoiseRow + (size_t)TQ * U * s + noise_taps(s) - s) * sizeof(float);
}

template <int CO, int U>
inline void launch_seam_cu(SeamArgs a, int B, hipStream_t st) {
  constexpr int TQ = 64 * seam_nf(CO, U);
  const long tiles = (a.Tin + TQ - 1) / TQ;
  const size_t lds = seam_lds_bytes<CO, U>(a.s);       // at most 36.9 + 2.3 + 16.4 KB
  const long split = batch_split();
  for (long b0 = 0; b0 < B; b0 += split) {
    a.b0 = b0;
    const long nb = B - b0 < split ? B - b0 : split;
    hipLaunchKernelGGL((k_upsample_seam<CO, U>), dim3((unsigned)tiles, (unsigned)nb), dim3(kThreads), lds, st, a);
  }
}

template <int CO>
inline void launch_seam_c(const SeamArgs& a, int B, int u, hipStream_t st) {
  if (u == 2) launch_seam_cu<CO, 2>(a, B, st);
  else if (u == 4) launch_seam_cu<CO, 4>(a, B, st);
  else launch_seam_cu<CO, 8>(a, B, st);
}

struct HeadArgs {
  const float* x; float* y;                            // [B, C, T], [B, 1, T] contiguous
  const float* w; const float* bias;                   // [1, C, 7], [1]
  float slope;
  long T; long b0;
};

template <int C>
__global__ __launch_bounds__(kThreads) void k_output_head(HeadArgs a) {
  __shared__ __attribute__((aligned(16))) float rows[kHeadRows * kHeadRS];
  const int tid = threadIdx.x;
  const long b = a.b0 + blockIdx.y;
  const long t0 = (long)blockIdx.x * kHeadTile;
  const long T = a.T;
  const float* xb = a.x + b * C * T;
  const float slope = a.slope;
  const float bv = a.bias[0];
  float acc[4] = {bv, bv, bv, bv};
  for (int c0 = 0; c0 < C; c0 += kHeadRows) {
    if (c0) __syncthreads();
    for (int i = tid; i < kHeadRows * kHeadRS; i += kThreads) {
      const int row = i / kHeadRS, c = i - row * kHeadRS;
      const long t = t0 - 4 + c;
      float v = 0.f;
      if (t >= 0 && t < T) {
        v = xb[(c0 + row) * T + t];
        v = v > 0.f ? v : v * slope;
      }
      rows[i] = v;
    }
    __syncthreads();
#pragma unroll
    for (int row = 0; row < kHeadRows; ++row) {
      const f32x4t* p = reinterpret_cast<const f32x4t*>(rows + row * kHeadRS + 4 * tid);
      const f32x4t v0 = p[0], v1 = p[1], v2 = p[2];
      const float v[12] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3], v2[0], v2[1], v2[2], v2[3]};
      const float* w = a.w + (c0 + row) * kHeadTaps;   // uniform: scalar loads
#pragma unroll
      for (int j = 0; j < kHeadTaps; ++j) {
        const float wj = w[j];
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[o] = fmaf(v[1 + o + j], wj, acc[o]);   // sample t0 + 4 tid + o + j - 3 is column 4 tid + 1 + o + j
      }
    }
  }
  const long t = t0 + 4 * tid;
  float* o = a.y + b * T + t;
  float r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = tanhf(acc[i]);
  if (t + 3 < T && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
    f32x4t w4 = {r[0], r[1], r[2], r[3]};
    *reinterpret_cast<f32x4t*>(o) = w4;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (t + i < T) o[i] = r[i];
  }
}

template <int C>
inline void launch_head_c(HeadArgs a, int B, hipStream_t st) {
  const long tiles = (a.T + kHeadTile - 1) / kHeadTile;
  const long split = batch_split();
  for (long b0 = 0; b0 < B; b0 += split) {
    a.b0 = b0;
    const long nb = B - b0 < split ? B - b0 : split;
    hipLaunchKernelGGL((k_output_head<C>), dim3((unsigned)tiles, (unsigned)nb), dim3(kThreads), 0, st, a);
  }
}

}  // namespace gentail

// ---- host side ---------------------------------------------------------------------------------------------------------------

size_t upsample_stage_pack_bytes(int CO, int u, int s) {
  return gentail::seam_shape_ok(CO, u, s) ? gentail::seam_pack_floats(CO, u) * sizeof(float) : 0;
}

// wu: [2 CO][CO][2 u] (ConvTranspose1d: input channel first), bu: [CO], wn: [CO][1][2 s] ([CO][1][1] at s = 1), bn: [CO], all host
// memory; out: host memory.  Fragments [u][2][CO / 16][CO / 2][64]: element (r, tap, m, cs, l) is Wu[4 cs + (l >> 4)][16 m +
// (l & 15)][(r + u / 2) mod u + tap u]; then bu + bn; then the noise taps, 9 floats per channel, zeros behind the last tap.
void upsample_stage_pack(const float* wu, const float* bu, const float* wn, const float* bn, int CO, int u, int s, float* out) {
  const int CI = 2 * CO, MT = CO / 16, KS = CI / 4, k = 2 * u, ks = gentail::noise_taps(s);
  for (int r = 0; r < u; ++r)
    for (int tap = 0; tap < 2; ++tap)
      for (int m = 0; m < MT; ++m)
        for (int cs = 0; cs < KS; ++cs)
          for (int l = 0; l < 64; ++l) {
            const int co = 16 * m + (l & 15), ci = 4 * cs + (l >> 4), j = (r + u / 2) % u + tap * u;
            out[((((size_t)r * 2 + tap) * MT + m) * KS + cs) * 64 + l] = wu[((size_t)ci * CO + co) * k + j];
          }
  float* o = out + (size_t)CI * CO * k;
  for (int c = 0; c < CO; ++c) o[c] = bu[c] + bn[c];
  o += CO;
  for (int c = 0; c < CO; ++c)
    for (int m = 0; m < gentail::kNoiseRow; ++m) o[c * gentail::kNoiseRow + m] = m < ks ? wn[c * ks + m] : 0.f;
}

void launch_upsample_stage(const float* x, const float* src, float* y, const float* packed, int B, int CO, long Tin, int u, int s,
                           hipStream_t st) {
  gentail::SeamArgs a;
  a.x = x; a.src = src; a.y = y; a.packed = packed;
  a.Tin = Tin; a.b0 = 0; a.s = s;
  a.vec = (reinterpret_cast<uintptr_t>(y) & (u == 2 ? 7 : 15)) == 0;
  if (CO == 16) gentail::launch_seam_c<16>(a, B, u, st);
  else if (CO == 32) gentail::launch_seam_c<32>(a, B, u, st);
  else gentail::launch_seam_c<64>(a, B, u, st);
}

void launch_output_head(const float* x, const float* w, const float* bias, float slope, float* y, int B, int C, long T,
                        hipStream_t st) {
  gentail::HeadArgs a;
  a.x = x; a.y = y; a.w = w; a.bias = bias; a.slope = slope; a.T = T; a.b0 = 0;
  if (C == 16) gentail::launch_head_c<16>(a, B, st);
  else if (C == 32) gentail::launch_head_c<32>(a, B, st);
  else gentail::launch_head_c<64>(a, B, st);
}

}  // namespace ddsp
