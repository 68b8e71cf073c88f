// The channel-split form of conformer_conv.h's module, for calls of a few hundred frames: the same mathematics, [B, L, D] layout,
// packed table and SUMS (every accumulator starts at the same value and walks k in the same order, the LayerNorm and the sigmoid are
// the tiled kernel's own helpers, so the result is bit-identical to ddsp_hip_conformer_conv), tiled the other way round.  The
// frame tile is ONE 16-frame MFMA fragment and the channels are split over blockIdx.y and the waves of a workgroup, so that
// 1 x 100 frames are a hundred workgroups instead of two.  Every dependency between workgroups is a launch boundary: three plain
// launches on the caller's stream, no flags, no atomics.  Included from api.hip only, after conformer_conv.h.
//
//     g = glu(W1 ln(x) + b1)         k_ccs_glu      grid (1, 2 D / 32, B tiles), 2 waves: the tile's x -> LDS xs [16][D + 2] (zeros at
//                                      frames >= L), the optional LayerNorm in place, a wave per frame (cconv::layer_norm_row); a
//                                      wave owns 16 inner channels, an "out" and a "gate" fragment: two independent chains of
//                                      D / 4 MFMAs, the W1 fragments kPF k-steps ahead in a register ring that is filled BEFORE
//                                      the tile is staged;  GLU in registers -> g [B][2 D][L]
//     h = silu(dw31(g) + bd)         k_ccs_stencil  grid (ceil(L / 64), 2 D / 16, B), 256 threads: thread (channel, run of 4 frames)
//                                      reads its 34 values of g (zero outside [0, L)) from memory;  -> h [B][2 D][L]
//     y = W2 h + b2 (+ x)            k_ccs_out      grid (1, D / 32, B tiles), 2 waves: a wave owns one 16-row block x 16 frames, one
//                                      chain of 2 D / 4 MFMAs; the B fragment of a k-step is four rows of h, 16 consecutive
//                                      frames each, read from memory kPF k-steps ahead like the W2 fragments.
// Two waves per workgroup: D = 256 has 16 row blocks in the last launch, so four waves would leave 28 workgroups at 1 x 100 and two
// leave 56; and 8 divides the 8 and 16 channel groups (see launch_d).
// Frames >= L of a tile: their x is zeros in launch 1 (and not normalised), their h is read at frame L - 1 in launch 3 (a column
// of an MFMA never reaches another column); none of their results is stored, so nothing is read past a row.
// The workspace is g | h = (2 + 2) B L D floats.  tiles = ceil(L / 16); B tiles <= kMaxTiles, on the grid's z.
// LDS: 16 (D + 2) floats = 16 512 bytes in launch 1, none elsewhere.  DESIGN.md 7.8 has the arithmetic and the measurements.
#pragma once
#include "conformer_conv.h"

namespace ddsp {
namespace ccs {

using cconv::f32x4c;

constexpr int kWaves = 2;
constexpr int kThreads = 64 * kWaves;
constexpr int kT = 16;                                 // frames per workgroup: one MFMA fragment
constexpr int kPF = 32;                                // k-steps the operands of both GEMMs are loaded ahead: a wave is alone on its
                                                       // SIMD and a round of the ring has to outlast a trip to memory
constexpr int kPB = 16;                                // GEMM 1: k-steps whose B fragments are read from LDS at once
constexpr int kSThreads = 256;                         // stencil: threads per workgroup
constexpr int kRun = 4;                                // stencil: frames per thread
constexpr int kSC = 16;                                // stencil: channels per workgroup
constexpr int kST = kRun * (kSThreads / kSC);          // stencil: frames per workgroup
constexpr long kMaxTiles = 4096;                       // B ceil(L / 16): the form is for small calls

struct Args {
  const float* x; float* y;                            // [B, L, D]
  float* g; float* h;                                  // the workspace: [B, 2 D, L], [B, 2 D, L]
  const float* tab;
  long L; long tiles;                                  // tiles = ceil(L / kT)
  float eps;
  int norm, add_input;
};

template <int D>
__global__ __launch_bounds__(kThreads) void k_ccs_glu(Args a) {
  constexpr int XS = D + 2, I = 2 * D, KS1 = D / 4, NG = I / 16;
  static_assert(NG % kWaves == 0 && KS1 % kPF == 0 && kPF % kPB == 0 && (kT * D / 4) % kThreads == 0 && D % 64 == 0,
                "whole workgroups of channel groups, k-steps in runs of kPF, whole rounds of staging, channels per lane of the LayerNorm");
  static_assert(XS % 32 == 2, "bank spread of the B fragments");
  static_assert(cconv::kCH == 32, "the table's (chunk, half) order of conformer_conv_pack: a 16-channel group is (chunk, half)");
  __shared__ float xs[kT * XS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const long b = blockIdx.z / a.tiles, L = a.L;
  const long t0 = (blockIdx.z - b * a.tiles) * kT;
  const int grp = blockIdx.y * kWaves + wave;            // 16 inner channels: half grp & 1 of the tiled kernel's chunk grp >> 1
  const int c0 = 16 * grp;
  // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
  const float* pa = a.tab + (size_t)grp * 2 * KS1 * 64 + lane;                 // + (half * KS1 + k-step) * 64
  float ar[kPF][2];
#pragma unroll
  for (int q = 0; q < kPF; ++q) { ar[q][0] = pa[q * 64]; ar[q][1] = pa[(KS1 + q) * 64]; }

  const float* xb = a.x + b * L * D;
#pragma unroll
  for (int u = 0; u < kT * D / 4 / kThreads; ++u) {
    const int i = tid + kThreads * u;
    const int f = i / (D / 4), c = 4 * (i - f * (D / 4));
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t0 + f < L) w = *reinterpret_cast<const float4*>(xb + (t0 + f) * D + c);
    float* o = xs + f * XS + c;
    o[0] = w.x; o[1] = w.y; o[2] = w.z; o[3] = w.w;
  }
  const float* b1 = a.tab + cconv::off_b1(D);
  f32x4c acc[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[h][r] = b1[h * I + c0 + 4 * lq + r];
  __syncthreads();

  if (a.norm) {
    const float* gamma = a.tab + cconv::off_gamma(D);
    for (int f = wave; f < kT && t0 + f < L; f += kWaves) cconv::layer_norm_row<D>(xs + f * XS, gamma, gamma + D, a.eps, lane);
    __syncthreads();
  }

  const float* pb = xs + lj * XS + lq;
  for (int s = 0; s < KS1; s += kPF) {
    const int ahead = s + kPF < KS1 ? kPF * 64 : 0;    // the last kPF steps load again what they hold
#pragma unroll
    for (int q0 = 0; q0 < kPF; q0 += kPB) {
      float bv[kPB];
#pragma unroll
      for (int q = 0; q < kPB; ++q) bv[q] = pb[4 * (s + q0 + q)];
#pragma unroll
      for (int q = 0; q < kPB; ++q) {
        const float a0 = ar[q0 + q][0], a1 = ar[q0 + q][1];
        ar[q0 + q][0] = pa[ahead]; ar[q0 + q][1] = pa[ahead + KS1 * 64];
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv[q], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv[q], acc[1], 0, 0, 0);
        pa += 64;
      }
    }
  }
  // D fragment: col = l & 15, row = 4 (l >> 4) + r
  const long t = t0 + lj;
  if (t >= L) return;
  float* gb = a.g + b * I * L;
#pragma unroll
  for (int r = 0; r < 4; ++r) gb[(long)(c0 + 4 * lq + r) * L + t] = acc[0][r] * cconv::sigmoid(acc[1][r]);
}

template <int D>
__global__ __launch_bounds__(kSThreads) void k_ccs_stencil(Args a) {
  constexpr int I = 2 * D;
  static_assert(I % kSC == 0 && kSThreads % kSC == 0, "whole workgroups of channels");
  const int tid = threadIdx.x;
  const int c = blockIdx.y * kSC + tid / (kSThreads / kSC);
  const long b = blockIdx.z, L = a.L;
  const long t0 = (long)blockIdx.x * kST + kRun * (tid % (kSThreads / kSC));
  if (t0 >= L) return;
  const float* g = a.g + (b * I + c) * L;
  const float* wd = a.tab + cconv::off_wd(D) + c * cconv::kTaps;
  float win[kRun + cconv::kTaps - 1], o[kRun];
#pragma unroll
  for (int i = 0; i < kRun + cconv::kTaps - 1; ++i) {
    const long q = t0 - cconv::kHalo + i;
    win[i] = (q >= 0 && q < L) ? g[q] : 0.f;
  }
  const float bias = a.tab[cconv::off_bd(D) + c];
#pragma unroll
  for (int u = 0; u < kRun; ++u) o[u] = bias;
#pragma unroll
  for (int j = 0; j < cconv::kTaps; ++j) {
    const float w = wd[j];
#pragma unroll
    for (int u = 0; u < kRun; ++u) o[u] = __fmaf_rn(w, win[u + j], o[u]);
  }
  float* h = a.h + (b * I + c) * L;
#pragma unroll
  for (int u = 0; u < kRun; ++u)
    if (t0 + u < L) h[t0 + u] = o[u] * cconv::sigmoid(o[u]);
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_ccs_out(Args a) {
  constexpr int I = 2 * D, KS2 = I / 4, MF = D / 16, KC = cconv::kCH / 4;
  static_assert(MF % kWaves == 0 && KS2 % kPF == 0 && kPF % KC == 0, "whole workgroups of row blocks, k-steps in runs of kPF chunks");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const int mf = blockIdx.y * kWaves + wave;
  const long b = blockIdx.z / a.tiles, L = a.L;
  const long t = (blockIdx.z - b * a.tiles) * kT + lj;
  const bool in = t < L;
  // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
  // the fragment of global k-step q: chunk q / KC of the tiled kernel, its k-step q % KC
  const float* pa = a.tab + cconv::off_a2(D) + (size_t)mf * KC * 64 + lane;            // + ((q / KC) MF KC + q % KC) * 64
  const float* pb = a.h + (b * I + lq) * L + (in ? t : L - 1);                         // + k-step * 4 L
  float ar[kPF], br[kPF];
#pragma unroll
  for (int q = 0; q < kPF; ++q) { ar[q] = pa[((q / KC) * MF * KC + q % KC) * 64]; br[q] = pb[(long)q * 4 * L]; }
  const float* b2 = a.tab + cconv::off_b2(D);
  const int c = 16 * mf + 4 * lq;
  // D fragment: col = l & 15, row = 4 (l >> 4) + r
  f32x4c acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = b2[c + r];
  for (int s = 0; s < KS2; s += kPF) {
    const bool more = s + kPF < KS2;                   // the last kPF steps load again what they hold
    const size_t aa = more ? (size_t)(kPF / KC) * MF * KC * 64 : 0;
    const long ab = more ? (long)kPF * 4 * L : 0;
#pragma unroll
    for (int q = 0; q < kPF; ++q) {
      const float av = ar[q], bv = br[q];
      ar[q] = pa[aa + ((q / KC) * MF * KC + q % KC) * 64]; br[q] = pb[ab + (long)q * 4 * L];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
    pa += (size_t)(kPF / KC) * MF * KC * 64; pb += (long)kPF * 4 * L;
  }
  if (!in) return;
  const long e = (b * L + t) * D + c;
  float4 v = make_float4(acc[0], acc[1], acc[2], acc[3]);
  if (a.add_input) {
    const float4 xv = *reinterpret_cast<const float4*>(a.x + e);
    v.x = xv.x + v.x; v.y = xv.y + v.y; v.z = xv.z + v.z; v.w = xv.w + v.w;
  }
  *reinterpret_cast<float4*>(a.y + e) = v;
}

inline long tiles_of(long L) { return (L + kT - 1) / kT; }
inline bool in_range(long B, long L) { return B * tiles_of(L) <= kMaxTiles; }

template <int D>
inline void launch_d(Args a, int B, hipStream_t st) {
  // the GEMMs' grids are (1, channel groups, B tiles): workgroups go round the chip's eight dies in the order of their linear index,
  // and 8 divides the number of channel groups, so all tiles that read one slice of a weight matrix share one die's L2
  static_assert(D / 16 / kWaves % 8 == 0, "a channel group stays on its die");
  a.tiles = tiles_of(a.L);
  const unsigned nz = (unsigned)(B * a.tiles), nb = (unsigned)B;
  hipLaunchKernelGGL((k_ccs_glu<D>), dim3(1, 2 * D / 16 / kWaves, nz), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL((k_ccs_stencil<D>), dim3((unsigned)((a.L + kST - 1) / kST), 2 * D / kSC, nb), dim3(kSThreads), 0, st, a);
  hipLaunchKernelGGL((k_ccs_out<D>), dim3(1, D / 16 / kWaves, nz), dim3(kThreads), 0, st, a);
}

}  // namespace ccs

// ---- host side ---------------------------------------------------------------------------------------------------------------

size_t conformer_split_ws_bytes(long B, long L, int D) { return (size_t)B * (size_t)L * 4 * D * sizeof(float); }

// three launches.  packed: conformer_conv_pack's floats on the device; ws: conformer_split_ws_bytes; B ceil(L / 16) <= 4096.
void launch_conformer_split(const float* x, float* y, const float* packed, float* ws, int B, long L, int D, int norm, float eps,
                            int add_input, hipStream_t st) {
  ccs::Args a;
  const size_t n = (size_t)B * (size_t)L * 512;
  a.x = x; a.y = y; a.g = ws; a.h = ws + n; a.tab = packed; a.L = L; a.tiles = 0; a.eps = eps; a.norm = norm; a.add_input = add_input;
  ccs::launch_d<256>(a, B, st);
  (void)D;
}

}  // namespace ddsp
