// The channel-split form of naive_v2_layer.h's layer, for calls of a few hundred frames: the same mathematics, layouts, packed
// table and SUMS (every accumulator starts at the same value and walks k in the same order, so the result is bit-identical to
// ddsp_hip_naive_v2_layer), tiled the other way round.  The frame tile is ONE 16-frame MFMA fragment and the channels are split
// over blockIdx.y and the waves of a workgroup, so that 1 x 100 frames are a few hundred waves instead of three workgroups.
// Every dependency between workgroups is a launch boundary: four plain launches on the caller's stream, no flags, no atomics.
// Included from api.hip only, after naive_v2_layer.h.
//
//     x' = x + d + Wc cond + bc      k_nv2s_xprime  grid (1, D / 64, B tiles), 4 waves: a wave owns one 16-row block x 16 frames,
//                                      32 MFMAs, all 32 + 32 operands loaded before the first one;  -> xp [B][L][D]
//     g  = glu(W1 x' + b1)           k_nv2s_glu     grid (1, 2 D / 64, B tiles), 4 waves: the tile's x' -> LDS xs [16][D + 2] (zeros
//                                      at frames >= L); a wave owns 16 inner channels, an "out" and a "gate" fragment: two
//                                      independent chains of D / 4 MFMAs, the W1 fragments kPF k-steps ahead in a register ring
//                                      that is filled BEFORE the tile is staged;  GLU in registers -> g [B][2 D][L]
//     h  = silu(dw31(g) + bd)        k_nv2s_stencil grid (ceil(L / 64), 2 D / 16, B), 256 threads: thread (channel, run of 4
//                                      frames) reads its 34 values of g (zero outside [0, L)) from memory;  -> h [B][2 D][L]
//     y  = x + W2 h + b2             k_nv2s_out     grid (1, D / 64, B tiles), 4 waves: a wave owns one 16-row block x 16 frames,
//                                      one chain of 2 D / 4 MFMAs; the B fragment of a k-step is four rows of h, 16 consecutive
//                                      frames each, read from memory kPF k-steps ahead like the W2 fragments.
// Frames >= L of a tile: their x and cond are zeros in launch 1, their x' zeros in launch 2, their h is read at frame L - 1 in
// launch 4 (a column of an MFMA never reaches another column); none of their results is stored, so nothing is read past a row.
// The workspace is xp | g | h = (1 + 2 + 2) B L D floats.  tiles = ceil(L / 16); B tiles <= kMaxTiles, on the grid's z with the
// channel groups on y: see launch_d for why the tiles are not on x.
// LDS: 16 (D + 2) floats = 32 896 bytes in launch 2, none elsewhere.  DESIGN.md 7.11 has the arithmetic and the measurements.
#pragma once
#include "naive_v2_layer.h"

namespace ddsp {
namespace nv2s {

using nv2::f32x4n;

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kT = 16;                                 // frames per workgroup: one MFMA fragment
constexpr int kPF = 32;                                // k-steps the operands of GEMM 1 and GEMM 2 are loaded ahead: a wave is alone
                                                       // on its SIMD and a round of the ring has to outlast a trip to memory
constexpr int kPB = 16;                                // GEMM 1: k-steps whose B fragments are read from LDS at once
constexpr int kRun = 4;                                // stencil: frames per thread
constexpr int kSC = 16;                                // stencil: channels per workgroup
constexpr int kST = kRun * (kThreads / kSC);           // stencil: frames per workgroup
constexpr long kMaxTiles = 4096;                       // B ceil(L / 16): the form is for small calls

struct Args {
  const float* x; const float* cond; const float* d;   // [B, L, D], [B, L, Hc], [B, D]
  float* y;                                            // [B, L, D]
  float* xp; float* g; float* h;                       // the workspace: [B, L, D], [B, 2 D, L], [B, 2 D, L]
  const float* tab;
  long L; long tiles;                                  // tiles = ceil(L / kT)
};

template <int D, int Hc>
__global__ __launch_bounds__(kThreads) void k_nv2s_xprime(Args a) {
  constexpr int KS0 = Hc / 4, MF = D / 16;
  static_assert(MF % kWaves == 0 && Hc % 4 == 0, "whole workgroups of row blocks");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const int mf = blockIdx.y * kWaves + wave;
  const long b = blockIdx.z / a.tiles, L = a.L;
  const long t = (blockIdx.z - b * a.tiles) * kT + lj;
  const bool in = t < L;
  const int c = 16 * mf + 4 * lq;
  // D fragment: col = l & 15, row = 4 (l >> 4) + r
  const float4 dv = *reinterpret_cast<const float4*>(a.d + b * D + c);
  const float4 bv = *reinterpret_cast<const float4*>(a.tab + nv2::off_bc(D, Hc) + c);
  float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (in) xv = *reinterpret_cast<const float4*>(a.x + (b * L + t) * D + c);
  f32x4n acc;
  acc[0] = xv.x + dv.x + bv.x; acc[1] = xv.y + dv.y + bv.y; acc[2] = xv.z + dv.z + bv.z; acc[3] = xv.w + dv.w + bv.w;
  // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
  const float* pa = a.tab + (size_t)mf * 64 + lane;                      // + k-step * MF * 64
  const float* pc = a.cond + (b * L + (in ? t : 0)) * Hc + lq;           // + 4 * k-step
  float av[KS0], cv[KS0];
#pragma unroll
  for (int s = 0; s < KS0; ++s) {
    av[s] = pa[(size_t)s * MF * 64];
    cv[s] = in ? pc[4 * s] : 0.f;
  }
#pragma unroll
  for (int s = 0; s < KS0; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], cv[s], acc, 0, 0, 0);
  if (in) *reinterpret_cast<float4*>(a.xp + (b * L + t) * D + c) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

template <int D, int Hc>
__global__ __launch_bounds__(kThreads) void k_nv2s_glu(Args a) {
  constexpr int XS = D + 2, I = 2 * D, KS1 = D / 4, NG = I / 16;
  static_assert(NG % kWaves == 0 && KS1 % kPF == 0 && kPF % kPB == 0 && (kT * D / 4) % kThreads == 0,
                "whole workgroups of channel groups, k-steps in runs of kPF, whole rounds of staging");
  static_assert(XS % 32 == 2, "bank spread of the B fragments");
  static_assert(nv2::kWaves == 8 && I % 256 == 0, "the table's (wave, round) order of naive_v2_layer_pack");
  __shared__ float xs[kT * XS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const long b = blockIdx.z / a.tiles, L = a.L;
  const long t0 = (blockIdx.z - b * a.tiles) * kT;
  // the wave's 16 inner channels are pair p of the 32 that wave v of the tiled kernel owns in its round rd
  const int grp = blockIdx.y * kWaves + wave;
  const int p = grp & 1, v = (grp >> 1) & 7, rd = grp >> 4;
  const int c0 = 16 * grp;
  const float* pa = a.tab + nv2::off_a1(D, Hc) + ((size_t)(4 * v + rd) * KS1 * 4 + 2 * p) * 64 + lane;   // + k-step * 256 + half * 64
  float ar[kPF][2];
#pragma unroll
  for (int q = 0; q < kPF; ++q) { ar[q][0] = pa[q * 256]; ar[q][1] = pa[q * 256 + 64]; }

  const float* xpb = a.xp + b * L * D;
#pragma unroll
  for (int u = 0; u < kT * D / 4 / kThreads; ++u) {
    const int i = tid + kThreads * u;
    const int f = i / (D / 4), c = 4 * (i - f * (D / 4));
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t0 + f < L) w = *reinterpret_cast<const float4*>(xpb + (t0 + f) * D + c);
    float* o = xs + f * XS + c;
    o[0] = w.x; o[1] = w.y; o[2] = w.z; o[3] = w.w;
  }
  const float* b1 = a.tab + nv2::off_b1(D, Hc);
  f32x4n acc[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[h][r] = b1[h * I + c0 + 4 * lq + r];
  __syncthreads();

  const float* pb = xs + lj * XS + lq;
  for (int s = 0; s < KS1; s += kPF) {
    const int ahead = s + kPF < KS1 ? kPF * 256 : 0;   // the last kPF steps load again what they hold
#pragma unroll
    for (int q0 = 0; q0 < kPF; q0 += kPB) {
      float bv[kPB];
#pragma unroll
      for (int q = 0; q < kPB; ++q) bv[q] = pb[4 * (s + q0 + q)];
#pragma unroll
      for (int q = 0; q < kPB; ++q) {
        const float a0 = ar[q0 + q][0], a1 = ar[q0 + q][1];
        ar[q0 + q][0] = pa[ahead]; ar[q0 + q][1] = pa[ahead + 64];
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv[q], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv[q], acc[1], 0, 0, 0);
        pa += 256;
      }
    }
  }
  const long t = t0 + lj;
  if (t >= L) return;
  float* gb = a.g + b * I * L;
#pragma unroll
  for (int r = 0; r < 4; ++r) gb[(long)(c0 + 4 * lq + r) * L + t] = acc[0][r] * nv2::sigmoid(acc[1][r]);
}

template <int D, int Hc>
__global__ __launch_bounds__(kThreads) void k_nv2s_stencil(Args a) {
  constexpr int I = 2 * D;
  static_assert(I % kSC == 0 && kThreads % kSC == 0, "whole workgroups of channels");
  const int tid = threadIdx.x;
  const int c = blockIdx.y * kSC + tid / (kThreads / kSC);
  const long b = blockIdx.z, L = a.L;
  const long t0 = (long)blockIdx.x * kST + kRun * (tid % (kThreads / kSC));
  if (t0 >= L) return;
  const float* g = a.g + (b * I + c) * L;
  const float* wd = a.tab + nv2::off_wd(D, Hc) + c * nv2::kTaps;
  float win[kRun + nv2::kTaps - 1], o[kRun];
#pragma unroll
  for (int i = 0; i < kRun + nv2::kTaps - 1; ++i) {
    const long q = t0 - nv2::kHalo + i;
    win[i] = (q >= 0 && q < L) ? g[q] : 0.f;
  }
  const float bias = a.tab[nv2::off_bd(D, Hc) + c];
#pragma unroll
  for (int u = 0; u < kRun; ++u) o[u] = bias;
#pragma unroll
  for (int j = 0; j < nv2::kTaps; ++j) {
    const float w = wd[j];
#pragma unroll
    for (int u = 0; u < kRun; ++u) o[u] = __fmaf_rn(w, win[u + j], o[u]);
  }
  float* h = a.h + (b * I + c) * L;
#pragma unroll
  for (int u = 0; u < kRun; ++u)
    if (t0 + u < L) h[t0 + u] = o[u] * nv2::sigmoid(o[u]);
}

template <int D, int Hc>
__global__ __launch_bounds__(kThreads) void k_nv2s_out(Args a) {
  constexpr int I = 2 * D, KS2 = I / 4, MF = D / 16;
  static_assert(MF % kWaves == 0 && KS2 % kPF == 0, "whole workgroups of row blocks, k-steps in runs of kPF");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const int mf = blockIdx.y * kWaves + wave;
  const long b = blockIdx.z / a.tiles, L = a.L;
  const long t = (blockIdx.z - b * a.tiles) * kT + lj;
  const bool in = t < L;
  // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
  const float* pa = a.tab + nv2::off_a2(D, Hc) + (size_t)mf * 64 + lane;              // + k-step * MF * 64
  const float* pb = a.h + (b * I + lq) * L + (in ? t : L - 1);                        // + k-step * 4 L
  float ar[kPF], br[kPF];
#pragma unroll
  for (int q = 0; q < kPF; ++q) { ar[q] = pa[(size_t)q * MF * 64]; br[q] = pb[(long)q * 4 * L]; }
  const float* b2 = a.tab + nv2::off_b2(D, Hc);
  const int c = 16 * mf + 4 * lq;
  // D fragment: col = l & 15, row = 4 (l >> 4) + r
  f32x4n acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = b2[c + r];
  for (int s = 0; s < KS2; s += kPF) {
    const bool more = s + kPF < KS2;                   // the last kPF steps load again what they hold
    const size_t aa = more ? (size_t)kPF * MF * 64 : 0;
    const long ab = more ? (long)kPF * 4 * L : 0;
#pragma unroll
    for (int q = 0; q < kPF; ++q) {
      const float av = ar[q], bv = br[q];
      ar[q] = pa[aa]; br[q] = pb[ab];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      pa += MF * 64; pb += 4 * L;
    }
  }
  if (!in) return;
  const long e = (b * L + t) * D + c;
  const float4 xv = *reinterpret_cast<const float4*>(a.x + e);
  *reinterpret_cast<float4*>(a.y + e) = make_float4(xv.x + acc[0], xv.y + acc[1], xv.z + acc[2], xv.w + acc[3]);
}

inline long tiles_of(long L) { return (L + kT - 1) / kT; }
inline bool in_range(long B, long L) { return B * tiles_of(L) <= kMaxTiles; }

template <int D, int Hc>
inline void launch_d(Args a, int B, hipStream_t st) {
  // the GEMMs' grids are (1, channel groups, B tiles): workgroups go round the chip's eight dies in the order of their linear index,
  // and 8 divides the number of channel groups, so all tiles that read one slice of a weight matrix share one die's L2
  static_assert(D / 16 / kWaves % 8 == 0, "a channel group stays on its die");
  a.tiles = tiles_of(a.L);
  const unsigned nz = (unsigned)(B * a.tiles), nb = (unsigned)B;
  hipLaunchKernelGGL((k_nv2s_xprime<D, Hc>), dim3(1, D / 16 / kWaves, nz), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL((k_nv2s_glu<D, Hc>), dim3(1, 2 * D / 16 / kWaves, nz), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL((k_nv2s_stencil<D, Hc>), dim3((unsigned)((a.L + kST - 1) / kST), 2 * D / kSC, nb), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL((k_nv2s_out<D, Hc>), dim3(1, D / 16 / kWaves, nz), dim3(kThreads), 0, st, a);
}

}  // namespace nv2s

// ---- host side ---------------------------------------------------------------------------------------------------------------

size_t naive_v2_split_ws_bytes(long B, long L, int D) { return (size_t)B * (size_t)L * 5 * D * sizeof(float); }

// four launches.  packed: naive_v2_layer_pack's floats on the device; ws: naive_v2_split_ws_bytes; B ceil(L / 16) <= 4096.
void launch_naive_v2_split(const float* x, const float* cond, const float* d, float* y, const float* packed, float* ws, int B,
                           long L, int D, int Hc, hipStream_t st) {
  nv2s::Args a;
  const size_t n = (size_t)B * (size_t)L * 512;
  a.x = x; a.cond = cond; a.d = d; a.y = y; a.xp = ws; a.g = ws + n; a.h = ws + 3 * n; a.tab = packed; a.L = L; a.tiles = 0;
  nv2s::launch_d<512, 128>(a, B, st);
  (void)D; (void)Hc;
}

}  // namespace ddsp
