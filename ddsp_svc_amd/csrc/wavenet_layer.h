// The residual layer of the diffusion denoiser's WaveNet (diffusion/wavenet.py:31-61, ResidualBlock with dilation 1) as ONE launch:
// the 3-tap convolution and the conditioner projection as one f32 MFMA GEMM over a concatenated K, the gate in registers, the
// output projection as a second GEMM out of LDS.  Included from api.hip only (one translation unit holds the kernels).
//
//     z     = dil3(x + d) + bdil + Wc cond + bc        x [B, C, T], d [B, C], cond [B, H, T], z [B, 2 C, T]
//     g     = sigmoid(z[:C]) * tanh(z[C:])             the gate is the FIRST half
//     o     = Wo g + bo                                [B, 2 C, T]
//     x_out = (x + o[:C]) / sqrt(2);  skip = o[C:]     the residual is the FIRST half
// dil3: a 3-tap cross-correlation (not flipped) that zero-pads ITS OWN input x + d by 1: outside [0, T) the value is 0, not d.
//
// k_wavenet_layer<C, H>: grid (ceil(T / 64), B), 8 waves, 64 frames (four 16-frame fragments) per workgroup, frames along the MFMA's N
// (lanes): [B, C, T] has the frames contiguous, no transpose exists anywhere.
//   GEMM 1, M = 2 C, K = 3 C + H: K runs through LDS in chunks of 32 channels x (tile + 2) frames -- first the C / 32 chunks of
//     x + d (zeros outside [0, T), d added while staging; each chunk is read at three frame offsets, one per tap), then the H / 32
//     chunks of cond (one offset).  The next chunk's global loads are in flight while the MFMAs of this one run.  Wave v owns
//     gate rows [v C / 8, + C / 8) AND filter rows C + the same, so both values of an element meet in one lane; the accumulators
//     (2 C / 8 x tile per wave: 128 registers at C = 512) start at bdil + bc.
//   gate in registers -> LDS gs [C][tile], column bit 4 flipped on odd channels (a half wave reads two channels x 16 frames of a
//     B fragment from 32 different banks at a row stride of 0 mod 32).
//   GEMM 2, M = 2 C, K = C out of gs; the same row ownership, accumulators start at bo.
//   rows < C: (x + o) * (1 / sqrt 2) -> x_out (x read again: it is in cache); rows >= C -> skip, stored or added to what is there.
// Loads and stores along T are scalar per lane (16 consecutive frames per quarter wave): a [C, T] row starts 16-byte aligned
// only by accident (T = 862).
// Weights come from a table packed once on the host in fragment order: per k-step, per wave, its 2 C / 64 fragments of 256
// bytes, consecutive; every workgroup walks the table front to back.
//
// LDS: C tile + 32 (tile + 16) floats = 141 312 bytes at C = 512, 108 544 at C = 384: above the 64 KB the other kernels keep to,
// within the CU's 160 KiB, so ONE workgroup (8 waves, 2 per SIMD) is resident per CU.  DESIGN.md 7.9 has the arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "tuning.h"

namespace ddsp {
namespace wnet {

typedef float f32x4w __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kNT = 4;                                 // 16-frame fragments per workgroup
constexpr int kTile = 16 * kNT;                        // output frames per workgroup
constexpr int kKC = 32;                                // channels per staged chunk
constexpr int kW = kTile + 2;                          // frames of a chunk: the tile and one frame each side for the taps
constexpr int kPF = 4;                                 // k-steps the weight fragments are loaded ahead
constexpr int kXS = kTile + 16;                        // row stride of a chunk: 16 mod 32, >= kW

inline bool shape_ok(int C, int H) { return (C == 384 || C == 512) && H == 256; }
// the table, in floats: A1 [2 C x (3 C + H)], A2 [2 C x C], b1 = bdil + bc [2 C], bo [2 C]
constexpr size_t off_a2(int C, int H) { return (size_t)2 * C * (3 * C + H); }
constexpr size_t off_b1(int C, int H) { return off_a2(C, H) + (size_t)2 * C * C; }
constexpr size_t off_bo(int C, int H) { return off_b1(C, H) + 2 * C; }
constexpr size_t table_floats(int C, int H) { return off_bo(C, H) + 2 * C; }

// row of the [2 C] outputs that fragment f (0 .. 2 C / 128: first the wave's first-half blocks, then the matching second-half
// ones) of wave v holds at row i of the fragment; the same for both GEMMs
constexpr int row_of(int C, int v, int f, int i) { return (f / (C / 128)) * C + v * (C / 8) + 16 * (f % (C / 128)) + i; }

struct Args {
  const float* x; const float* cond; const float* d;   // [B, C, T], [B, H, T], [B, C]
  float* x_out; float* skip;                           // [B, C, T] each
  const float* tab;
  long T; long b0;
  int skip_mode;                                       // 0: store the skip rows, 1: add them to what is there
};

__device__ __forceinline__ float sigmoid(float v) { return 1.f / (1.f + expf(-v)); }   // expf(-v) = inf gives 0, never a NaN

template <int C, int H>
__global__ __launch_bounds__(kThreads) void k_wavenet_layer(Args a) {
  constexpr int MT = C / 128, NF = 2 * MT;             // 16-row blocks per half and fragments per wave
  constexpr int KS = kKC / 4;                          // k-steps per chunk and tap
  constexpr int NXC = C / kKC, NCH = NXC + H / kKC;    // chunks of x + d, chunks in all
  constexpr int NLD = (kKC * kW + kThreads - 1) / kThreads;
  static_assert(C % 128 == 0 && C % kKC == 0 && H % kKC == 0 && KS % kPF == 0 && (C / 4) % kPF == 0,
                "16-row blocks per wave and half, whole chunks, k-steps in runs of kPF");
  static_assert(kXS % 32 == 16 && kXS >= kW && kTile % 32 == 0, "bank spread of the B fragments; the column flip stays in the tile");
  __shared__ float xs[kKC * kXS];
  __shared__ float gs[C * kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const long b = a.b0 + blockIdx.y;
  const long t0 = (long)blockIdx.x * kTile;
  const long T = a.T;
  const float* xb = a.x + b * C * T;
  const float* cb = a.cond + b * H * T;
  const float* db = a.d + b * C;
  const float* tab = a.tab;
  const float* b1 = tab + off_b1(C, H);
  const float* bo = tab + off_bo(C, H);

  // chunk ch, element i -> channel i / kW of the chunk at frame t0 - 1 + i % kW
  float stage[NLD];
  auto fetch = [&](int ch) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int i = tid + kThreads * u;
      const int cc = i / kW, col = i - cc * kW;
      const long p = t0 - 1 + col;
      float v = 0.f;
      if (i < kKC * kW && p >= 0 && p < T) {
        if (ch < NXC) { const int c = ch * kKC + cc; v = xb[c * T + p] + db[c]; }
        else v = cb[((ch - NXC) * kKC + cc) * T + p];
      }
      stage[u] = v;
    }
  };

  // D fragment: col = l & 15, row = 4 (l >> 4) + r
  f32x4w acc[NF][kNT];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int n = 0; n < kNT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[f][n][r] = b1[row_of(C, wave, f, 4 * lq + r)];

  // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15].  The A fragments of a k-step are loaded kPF
  // k-steps ahead into a ring of kPF register sets (every run of k-steps below is a multiple of kPF, so a step's set is its index
  // mod kPF): the table is larger than an XCD's L2 and a load's latency is longer than one k-step's MFMAs.
  constexpr int AST = kWaves * NF * 64;                // floats of the table per k-step
  const float* pa = tab + (size_t)wave * NF * 64 + lane;               // + k-step * AST + f * 64
  float ar[kPF][NF];
#pragma unroll
  for (int q = 0; q < kPF; ++q)
#pragma unroll
    for (int f = 0; f < NF; ++f) ar[q][f] = pa[q * AST + f * 64];
  const float* pb = xs + lq * kXS + lj;
  fetch(0);
  for (int ch = 0; ch < NCH; ++ch) {
    __syncthreads();                                   // every wave is done with the previous chunk
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int i = tid + kThreads * u;
      const int cc = i / kW, col = i - cc * kW;
      if (i < kKC * kW) xs[cc * kXS + col] = stage[u];
    }
    __syncthreads();
    if (ch + 1 < NCH) fetch(ch + 1);
    const int taps = ch < NXC ? 3 : 1;                 // cond sits at the middle tap's offset
    for (int j = 0; j < taps; ++j) {
      const int off = ch < NXC ? j : 1;
      for (int s = 0; s < KS; s += kPF) {
#pragma unroll
        for (int q = 0; q < kPF; ++q) {
          float bv[kNT], av[NF];
#pragma unroll
          for (int n = 0; n < kNT; ++n) bv[n] = pb[4 * (s + q) * kXS + 16 * n + off];
#pragma unroll
          for (int f = 0; f < NF; ++f) { av[f] = ar[q][f]; ar[q][f] = pa[kPF * AST + f * 64]; }   // GEMM 2's table follows
#pragma unroll
          for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int n = 0; n < kNT; ++n) acc[f][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[f], bv[n], acc[f][n], 0, 0, 0);
          pa += AST;
        }
      }
    }
  }

  // the gate: channel = the wave's block + row of the fragment, first half sigmoid, second half tanh
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < kNT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = wave * (C / 8) + 16 * m + 4 * lq + r;
        const int col = (16 * n + lj) ^ ((c & 1) << 4);
        gs[c * kTile + col] = sigmoid(acc[m][n][r]) * tanhf(acc[MT + m][n][r]);
      }
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int n = 0; n < kNT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[f][n][r] = bo[row_of(C, wave, f, 4 * lq + r)];
  __syncthreads();

  // pa stands at A2: the table continues there; its first kPF k-steps are in the ring
  const float* pg = gs + lq * kTile + lj;              // channel 4 s + lq: its parity is lq's
  const int flip = (lq & 1) << 4;
  for (int s = 0; s < C / 4; s += kPF) {
    const int ahead = s + kPF < C / 4 ? kPF * AST : 0; // the last kPF steps load again what they hold: nothing follows A2
#pragma unroll
    for (int q = 0; q < kPF; ++q) {
      float bv[kNT], av[NF];
#pragma unroll
      for (int n = 0; n < kNT; ++n) bv[n] = pg[4 * (s + q) * kTile + ((16 * n) ^ flip)];
#pragma unroll
      for (int f = 0; f < NF; ++f) { av[f] = ar[q][f]; ar[q][f] = pa[ahead + f * 64]; }
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int n = 0; n < kNT; ++n) acc[f][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[f], bv[n], acc[f][n], 0, 0, 0);
      pa += AST;
    }
  }

  const float rs2 = 0.70710678118654752440f;
  float* ob = a.x_out + b * C * T;
  float* sb = a.skip + b * C * T;
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int n = 0; n < kNT; ++n) {
      const long t = t0 + 16 * n + lj;
      if (t >= T) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = wave * (C / 8) + 16 * (f % MT) + 4 * lq + r;
        const long e = c * T + t;
        const float v = acc[f][n][r];
        if (f < MT) ob[e] = (xb[e] + v) * rs2;
        else sb[e] = a.skip_mode ? sb[e] + v : v;
      }
    }
}

template <int C, int H>
inline void launch_ch(Args a, int B, hipStream_t st) {
  const long tiles = (a.T + kTile - 1) / kTile;
  const long split = batch_split();
  for (long b0 = 0; b0 < B; b0 += split) {
    a.b0 = b0;
    const long nb = B - b0 < split ? B - b0 : split;
    hipLaunchKernelGGL((k_wavenet_layer<C, H>), dim3((unsigned)tiles, (unsigned)nb), dim3(kThreads), 0, st, a);
  }
}

}  // namespace wnet

// ---- host side ---------------------------------------------------------------------------------------------------------------

size_t wavenet_layer_pack_bytes(int C, int H) {
  if (!wnet::shape_ok(C, H)) return 0;
  return wnet::table_floats(C, H) * sizeof(float);
}

// wdil [2 C][C][3], bdil [2 C], wc [2 C][H], bc [2 C], wo [2 C][C], bo [2 C]: host memory, as is out.
// A1: per k-step s1 (x part: chunk, tap, k-step of the chunk; then cond), wave v, fragment f, lane l: the weight of row
//     row_of(v, f, l & 15) at channel 4 s + (l >> 4) of the chunk (and its tap).  A2: per k-step s, wave, fragment, lane:
//     Wo[row_of(v, f, l & 15)][4 s + (l >> 4)].
void wavenet_layer_pack(const float* wdil, const float* bdil, const float* wc, const float* bc, const float* wo, const float* bo,
                        int C, int H, float* out) {
  using namespace wnet;
  const int NF = C / 64, KS = kKC / 4;
  float* p = out;
  for (int ch = 0; ch < C / kKC; ++ch)
    for (int j = 0; j < 3; ++j)
      for (int s = 0; s < KS; ++s)
        for (int v = 0; v < kWaves; ++v)
          for (int f = 0; f < NF; ++f)
            for (int l = 0; l < 64; ++l)
              *p++ = wdil[((size_t)row_of(C, v, f, l & 15) * C + ch * kKC + 4 * s + (l >> 4)) * 3 + j];
  for (int s = 0; s < H / 4; ++s)
    for (int v = 0; v < kWaves; ++v)
      for (int f = 0; f < NF; ++f)
        for (int l = 0; l < 64; ++l) *p++ = wc[(size_t)row_of(C, v, f, l & 15) * H + 4 * s + (l >> 4)];
  for (int s = 0; s < C / 4; ++s)
    for (int v = 0; v < kWaves; ++v)
      for (int f = 0; f < NF; ++f)
        for (int l = 0; l < 64; ++l) *p++ = wo[(size_t)row_of(C, v, f, l & 15) * C + 4 * s + (l >> 4)];
  for (int i = 0; i < 2 * C; ++i) *p++ = bdil[i] + bc[i];
  for (int i = 0; i < 2 * C; ++i) *p++ = bo[i];
}

// one launch per 65 535 utterances.  packed: wavenet_layer_pack's floats on the device.
void launch_wavenet_layer(const float* x, const float* cond, const float* d, float* x_out, float* skip, const float* packed, int B,
                          long T, int C, int H, int skip_mode, hipStream_t st) {
  wnet::Args a;
  a.x = x; a.cond = cond; a.d = d; a.x_out = x_out; a.skip = skip; a.tab = packed; a.T = T; a.b0 = 0; a.skip_mode = skip_mode;
  if (C == 384) wnet::launch_ch<384, 256>(a, B, st);
  else wnet::launch_ch<512, 256>(a, B, st);
  (void)H;
}

}  // namespace ddsp
