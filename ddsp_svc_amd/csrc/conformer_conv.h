// The conformer conv module of Unit2Control's decoder (diffusion/model_conformer_naive.py:117-150, the same text in reflow/, the
// same mathematics in ddsp/pcmer.py:189-216) as ONE launch: both pointwise convolutions as f32 MFMA GEMMs, the 4 D and 2 D wide
// intermediates kept on the CU.  Included from api.hip only (one translation unit holds the kernels).
//
//     net(x) = W2 silu(dw31(glu(W1 ln(x) + b1)) + bd) + b2           x, y [B, L, D], a frame's D channels contiguous
// ln: optional LayerNorm over the D channels of a frame (biased variance); glu: rows [0, 2 D) times sigmoid of rows [2 D, 4 D);
// dw31: a 31-tap cross-correlation per channel (not flipped) that zero-pads ITS OWN input by 15: the GLU's output is 0 at frames
// outside [0, L), not glu(b1).  y = net(x), or x + net(x) with add_input (the un-normalised x).
//
// k_conformer_conv<D>: grid (ceil(L / 98), B), 8 waves, 98 output frames per workgroup.  Frames run along the MFMA's N (lanes).
//   1. the x rows of the 128 frames the tile reaches (98 + 15 each side), zeros outside [0, L) -> LDS xs [128][D + 2].  The row
//      stride is 2 mod 32: the 32 lanes of a half wave read 16 frames x 2 consecutive channels of a B fragment from 32 banks.
//   2. LayerNorm in place, a wave per frame, sums and the normalisation in double (a frame of mean 1e3 does not cancel).
//   3. GEMM 2's accumulators, D x 112 frames, start at b2 and stay in registers: wave v owns rows [32 v, 32 v + 32), 14 fragments.
//   4. per chunk of 32 inner channels (2 D / 32 chunks):
//        GEMM 1 on the 128 frames for the chunk's 32 "out" rows and its 32 "gate" rows: wave v takes frames [32 (v & 3), + 32) of
//        channels [16 (v >> 2), + 16), so the out and the gate value of an element meet in one lane; accumulators start at b1.
//        GLU in registers, zero outside [0, L) -> LDS gs [32][144];  barrier
//        stencil: thread (channel, run of 7 frames) reads its 37 values, 7 x 31 fma, + bd, SiLU;  barrier;  over gs;  barrier
//        GEMM 2 += W2[:, chunk] gs (8 k-steps x 14 fragments per wave);  barrier before the next chunk's GLU writes gs.
//   5. + x when asked (read again from memory: it is in cache), float4 stores of 4 consecutive channels per lane.
// Weights come from a table packed once on the host in fragment order (one coalesced 256-byte read per fragment, the same for
// the waves that share it and for all workgroups).
//
// LDS: 128 (D + 2) + 32 x 144 floats = 150 528 bytes at D = 256: above the 64 KB the other kernels keep to, within the CU's 160 KiB,
// so ONE workgroup (8 waves, 2 per SIMD) is resident per CU.  DESIGN.md 7.8 has the arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "tuning.h"

namespace ddsp {
namespace cconv {

typedef float f32x4c __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kTaps = 31;
constexpr int kHalo = 15;
constexpr int kNW = 128;                               // frames of GEMM 1 per workgroup: the tile and the stencil's halo
constexpr int kTT = kNW - 2 * kHalo;                   // output frames per workgroup
constexpr int kN2 = 7;                                 // 16-frame fragments of GEMM 2: 112 >= kTT
constexpr int kCH = 32;                                // inner channels per chunk
constexpr int kGS = 144;                               // row stride of a chunk: 16 mod 32, >= kNW
constexpr int kRun = 7;                                // frames per stencil thread: 16 runs per channel cover 112

inline bool shape_ok(int D) { return D == 256; }
// the table, in floats: A1 [4 D x D], A2 [D x 2 D], b1 [4 D], wd [2 D][31], bd [2 D], b2 [D], then gamma [D], beta [D] with norm
constexpr size_t off_a2(int D) { return (size_t)4 * D * D; }
constexpr size_t off_b1(int D) { return off_a2(D) + (size_t)2 * D * D; }
constexpr size_t off_wd(int D) { return off_b1(D) + 4 * D; }
constexpr size_t off_bd(int D) { return off_wd(D) + (size_t)2 * D * kTaps; }
constexpr size_t off_b2(int D) { return off_bd(D) + 2 * D; }
constexpr size_t off_gamma(int D) { return off_b2(D) + D; }
constexpr size_t table_floats(int D, int norm) { return off_gamma(D) + (norm ? 2 * D : 0); }

struct Args {
  const float* x; float* y;                            // [B, L, D] contiguous
  const float* tab;
  long L; long b0;
  float eps;
  int norm, add_input;
};

// sigmoid and layer_norm_row are shared with the channel-split form (conformer_split.h): both kernels compile one text
__device__ __forceinline__ float sigmoid(float v) { return 1.f / (1.f + expf(-v)); }   // expf(-v) = inf gives 0, never a NaN

// LayerNorm of one frame's D channels in place, by one wave: sums and the normalisation in double (a frame of mean 1e3 does not
// cancel), lane l adds channels l + 64 i in the order of i, then an xor-shuffle reduction
template <int D>
__device__ __forceinline__ void layer_norm_row(float* row, const float* gamma, const float* beta, float eps, int lane) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < D / 64; ++i) s += (double)row[lane + 64 * i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  const double mean = s / D;
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < D / 64; ++i) { const double e = (double)row[lane + 64 * i] - mean; q += e * e; }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) q += __shfl_xor(q, m);
  const double rstd = 1.0 / sqrt(q / D + (double)eps);
#pragma unroll
  for (int i = 0; i < D / 64; ++i) {
    const int k = lane + 64 * i;
    row[k] = (float)(((double)row[k] - mean) * rstd * (double)gamma[k] + (double)beta[k]);
  }
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_conformer_conv(Args a) {
  constexpr int XS = D + 2, I = 2 * D, NCH = I / kCH, KS1 = D / 4, KS2 = kCH / 4, MT2 = D / 16 / kWaves;
  static_assert(D % (16 * kWaves) == 0 && D % 64 == 0, "rows of GEMM 2 per wave, channels per lane of the LayerNorm");
  static_assert(kThreads == kCH * 16 && 16 * kRun >= 16 * kN2 && 13 * kRun + kRun - 1 + kTaps - 1 < kNW && 14 * kRun >= kTT,
                "stencil threads: 14 runs of 7 cover the tile and stay inside the 128 frames, 16 cover GEMM 2's 112");
  __shared__ float xs[kNW * XS];
  __shared__ float gs[kCH * kGS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const long b = a.b0 + blockIdx.y;
  const long t0 = (long)blockIdx.x * kTT;
  const long L = a.L;
  const float* xb = a.x + b * L * D;
  const float* tab = a.tab;

  for (int i = tid; i < kNW * (D / 4); i += kThreads) {
    const int c = i / (D / 4), k4 = i % (D / 4);
    const long p = t0 - kHalo + c;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p >= 0 && p < L) v = *reinterpret_cast<const float4*>(xb + p * D + 4 * k4);
    float* d = xs + c * XS + 4 * k4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();

  if (a.norm) {
    const float* gamma = tab + off_gamma(D);
    const float* beta = gamma + D;
    for (int c = wave; c < kNW; c += kWaves) layer_norm_row<D>(xs + c * XS, gamma, beta, a.eps, lane);
    __syncthreads();
  }

  const float* A1 = tab;
  const float* A2 = tab + off_a2(D);
  const float* b1 = tab + off_b1(D);
  const float* wd = tab + off_wd(D);
  const float* bd = tab + off_bd(D);
  const float* b2 = tab + off_b2(D);

  // D fragment: col = l & 15, row = 4 (l >> 4) + r
  f32x4c acc2[MT2][kN2];
#pragma unroll
  for (int m = 0; m < MT2; ++m)
#pragma unroll
    for (int n = 0; n < kN2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc2[m][n][r] = b2[16 * (MT2 * wave + m) + 4 * lq + r];

  const int cg = wave & 3, rg = wave >> 2;             // GEMM 1: frames [32 cg, + 32), channels [16 rg, + 16) of the chunk
  const int sc = tid >> 4, run = tid & 15;             // stencil: channel of the chunk, run of kRun frames
  const float* pb1 = xs + (32 * cg + lj) * XS + lq;

  for (int ch = 0; ch < NCH; ++ch) {
    f32x4c acc1[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc1[h][0][r] = acc1[h][1][r] = b1[h * I + ch * kCH + 16 * rg + 4 * lq + r];
    // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
    const float* pa = A1 + ((size_t)(ch * 2 + rg) * 2 * KS1) * 64 + lane;
#pragma unroll 16
    for (int s = 0; s < KS1; ++s) {
      const float v0 = pb1[4 * s], v1 = pb1[16 * XS + 4 * s];
      const float a0 = pa[s * 64], a1 = pa[(KS1 + s) * 64];
      acc1[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, v0, acc1[0][0], 0, 0, 0);
      acc1[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, v1, acc1[0][1], 0, 0, 0);
      acc1[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, v0, acc1[1][0], 0, 0, 0);
      acc1[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, v1, acc1[1][1], 0, 0, 0);
    }
    __syncthreads();                                   // every wave is done with the previous chunk in gs
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int col = 32 * cg + 16 * n + lj;
      const long p = t0 - kHalo + col;
      const bool in = p >= 0 && p < L;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        gs[(16 * rg + 4 * lq + r) * kGS + col] = in ? acc1[0][n][r] * sigmoid(acc1[1][n][r]) : 0.f;
    }
    __syncthreads();

    float o[kRun];
    if (run * kRun < kTT) {
      const int c = ch * kCH + sc;
      const float* g = gs + sc * kGS + run * kRun;
      float win[kRun + kTaps - 1];
#pragma unroll
      for (int i = 0; i < kRun + kTaps - 1; ++i) win[i] = g[i];
      const float bias = bd[c];
#pragma unroll
      for (int u = 0; u < kRun; ++u) o[u] = bias;
#pragma unroll
      for (int j = 0; j < kTaps; ++j) {
        const float w = wd[c * kTaps + j];
#pragma unroll
        for (int u = 0; u < kRun; ++u) o[u] = __fmaf_rn(w, win[u + j], o[u]);
      }
#pragma unroll
      for (int u = 0; u < kRun; ++u) o[u] = o[u] * sigmoid(o[u]);
    } else {
#pragma unroll
      for (int u = 0; u < kRun; ++u) o[u] = 0.f;       // frames [98, 112) of GEMM 2: computed and dropped
    }
    __syncthreads();                                   // every thread holds its window
#pragma unroll
    for (int u = 0; u < kRun; ++u) gs[sc * kGS + run * kRun + u] = o[u];
    __syncthreads();

    const float* pa2 = A2 + ((size_t)(ch * (D / 16) + MT2 * wave) * KS2) * 64 + lane;
    const float* pb2 = gs + lq * kGS + lj;
#pragma unroll 4
    for (int ks = 0; ks < KS2; ++ks) {
      float bv[kN2];
#pragma unroll
      for (int n = 0; n < kN2; ++n) bv[n] = pb2[4 * ks * kGS + 16 * n];
#pragma unroll
      for (int m = 0; m < MT2; ++m) {
        const float av = pa2[(m * KS2 + ks) * 64];
#pragma unroll
        for (int n = 0; n < kN2; ++n) acc2[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[n], acc2[m][n], 0, 0, 0);
      }
    }
  }

  float* yb = a.y + b * L * D;
#pragma unroll
  for (int m = 0; m < MT2; ++m)
#pragma unroll
    for (int n = 0; n < kN2; ++n) {
      const int q = 16 * n + lj;
      const long t = t0 + q;
      if (q >= kTT || t >= L) continue;
      const long e = t * D + 16 * (MT2 * wave + m) + 4 * lq;
      float4 v = make_float4(acc2[m][n][0], acc2[m][n][1], acc2[m][n][2], acc2[m][n][3]);
      if (a.add_input) {
        const float4 xv = *reinterpret_cast<const float4*>(xb + e);
        v.x = xv.x + v.x; v.y = xv.y + v.y; v.z = xv.z + v.z; v.w = xv.w + v.w;
      }
      *reinterpret_cast<float4*>(yb + e) = v;
    }
}

template <int D>
inline void launch_d(Args a, int B, hipStream_t st) {
  const long tiles = (a.L + kTT - 1) / kTT;
  const long split = batch_split();
  for (long b0 = 0; b0 < B; b0 += split) {
    a.b0 = b0;
    const long nb = B - b0 < split ? B - b0 : split;
    hipLaunchKernelGGL((k_conformer_conv<D>), dim3((unsigned)tiles, (unsigned)nb), dim3(kThreads), 0, st, a);
  }
}

}  // namespace cconv

// ---- host side ---------------------------------------------------------------------------------------------------------------

size_t conformer_conv_pack_bytes(int D, int norm) {
  if (!cconv::shape_ok(D)) return 0;
  return cconv::table_floats(D, norm ? 1 : 0) * sizeof(float);
}

// w1 [4 D][D], b1 [4 D], wd [2 D][31], bd [2 D], w2 [D][2 D], b2 [D], gamma / beta [D] or both null: host memory, as is out.
// A1: per chunk c, channel half g, GLU half h (0 out, 1 gate), k-step s, lane l: W1[2 D h + 32 c + 16 g + (l & 15)][4 s + (l >> 4)].
// A2: per chunk c, 16-row block m, k-step s, lane l: W2[16 m + (l & 15)][32 c + 4 s + (l >> 4)].
void conformer_conv_pack(const float* w1, const float* b1, const float* wd, const float* bd, const float* w2, const float* b2,
                         const float* gamma, const float* beta, int D, float* out) {
  using namespace cconv;
  const int I = 2 * D, NCH = I / kCH, KS1 = D / 4, KS2 = kCH / 4;
  float* A1 = out;
  for (int c = 0; c < NCH; ++c)
    for (int g = 0; g < 2; ++g)
      for (int h = 0; h < 2; ++h)
        for (int s = 0; s < KS1; ++s)
          for (int l = 0; l < 64; ++l)
            A1[((((size_t)c * 2 + g) * 2 + h) * KS1 + s) * 64 + l] =
                w1[(size_t)(I * h + kCH * c + 16 * g + (l & 15)) * D + 4 * s + (l >> 4)];
  float* A2 = out + off_a2(D);
  for (int c = 0; c < NCH; ++c)
    for (int m = 0; m < D / 16; ++m)
      for (int s = 0; s < KS2; ++s)
        for (int l = 0; l < 64; ++l)
          A2[(((size_t)c * (D / 16) + m) * KS2 + s) * 64 + l] = w2[(size_t)(16 * m + (l & 15)) * I + kCH * c + 4 * s + (l >> 4)];
  for (int i = 0; i < 4 * D; ++i) out[off_b1(D) + i] = b1[i];
  for (int i = 0; i < I * kTaps; ++i) out[off_wd(D) + i] = wd[i];
  for (int i = 0; i < I; ++i) out[off_bd(D) + i] = bd[i];
  for (int i = 0; i < D; ++i) out[off_b2(D) + i] = b2[i];
  if (gamma)
    for (int i = 0; i < D; ++i) { out[off_gamma(D) + i] = gamma[i]; out[off_gamma(D) + D + i] = beta[i]; }
}

// one launch per 65 535 utterances.  packed: conformer_conv_pack's floats on the device.
void launch_conformer_conv(const float* x, float* y, const float* packed, int B, long L, int D, int norm, float eps, int add_input,
                           hipStream_t st) {
  cconv::Args a;
  a.x = x; a.y = y; a.tab = packed; a.L = L; a.b0 = 0; a.eps = eps; a.norm = norm; a.add_input = add_input;
  cconv::launch_d<256>(a, B, st);
  (void)D;
}

}  // namespace ddsp
