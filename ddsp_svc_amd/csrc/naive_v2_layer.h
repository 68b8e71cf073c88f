// The layer of the reflow / diffusion-fast denoiser (reflow/naive_v2_diff.py:81-98, NaiveV2DiffLayer with attn None, wavenet_like
// off and a conv module without LayerNorm; the same text in diffusion/) as TWO launches: the pointwise half up to the GLU, then
// the 31-tap stencil, the second pointwise convolution and the residual.  Included from api.hip only.
//
//     x' = x + d + Wc cond + bc                x, y [B, L, D], cond [B, L, Hc], d [B, D]: a frame's channels contiguous
//     g  = glu(W1 x' + b1)                     rows [0, 2 D) times sigmoid of rows [2 D, 4 D)
//     h  = silu(dw31(g) + bd)                  a 31-tap cross-correlation per channel (not flipped); g is ZERO outside [0, L)
//     y  = x + W2 h + b2                       the residual is the ORIGINAL x, not x'
// g goes from launch A to launch B through a workspace, channel-major: g [B][2 D][L], so that both sides touch runs of
// consecutive frames (A stores 16 per quarter wave, B loads a row of tile + 30) and the stencil's halo is a memory read, not
// GEMM work done twice.
//
// k_naive_v2_glu<D, Hc> (A): grid (ceil(L / 64), B), 8 waves, 64 frames per workgroup, frames along the MFMA's N (lanes).
//   GEMM 0, M = D, K = Hc: wave v owns rows [64 v, + 64) x 64 frames; the accumulators start at x + d + bc; the cond B fragments
//     are read straight from memory (the 32 KB tile is the same for all waves: supposed to stay in cache); zeros at frames >= L.
//     -> LDS xs [64][D + 2], the x' tile.  The row stride is 2 mod 32: a half wave reads 16 frames x 2 channels from 32 banks.
//   GEMM 1, M = 4 D, K = D, in 2 D / 256 rounds: per round wave v owns 32 inner channels, their 32 "out" rows AND their 32
//     "gate" rows, x all 64 frames (16 accumulator fragments, started at b1), so both values of an element meet in one lane.
//     The A fragments are loaded kPF k-steps ahead into a ring; the table is in each wave's walking order.
//   GLU in registers -> g; frames >= L are not stored.
// k_naive_v2_out<D, Hc> (B): grid (ceil(L / 112), B), 8 waves, 112 output frames per workgroup.
//   GEMM 2's accumulators, D x 112, start at b2 and stay in registers: wave v owns rows [64 v, + 64), 28 fragments.
//   per chunk of 32 inner channels (2 D / 32 chunks): the chunk's rows of g at frames [t0 - 15, t0 + 127), zeros outside [0, L),
//     -> LDS gs [32][144] (loaded into registers while the previous chunk computes);  barrier
//     stencil: thread (channel, run of 7 frames) reads its 37 values, 7 x 31 fma, + bd, SiLU -> LDS hs [32][144];  barrier
//     GEMM 2 += W2[:, chunk] hs (8 k-steps x 28 fragments per wave).  Two buffers, so two barriers per chunk.
//   + x (the original), float4 stores of 4 consecutive channels per lane; frames >= L are not stored.
// Weights come from one table packed once on the host in fragment order: Wc, bc, W1, b1, wd, bd, W2, b2.
//
// LDS: A 64 (D + 2) floats = 131 584 bytes at D = 512 (one workgroup per CU); B 2 x 32 x 144 floats = 36 864 bytes.
// DESIGN.md 7.11 has the arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "tuning.h"

namespace ddsp {
namespace nv2 {

typedef float f32x4n __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kTaps = 31;
constexpr int kHalo = 15;
constexpr int kNT = 4;                                 // A: 16-frame fragments per workgroup
constexpr int kTA = 16 * kNT;                          // A: frames per workgroup
constexpr int kPF = 4;                                 // A: k-steps the weight fragments of GEMM 1 are loaded ahead
constexpr int kN2 = 7;                                 // B: 16-frame fragments of GEMM 2
constexpr int kTB = 16 * kN2;                          // B: output frames per workgroup
constexpr int kCH = 32;                                // B: inner channels per chunk
constexpr int kWin = kTB + 2 * kHalo;                  // B: frames of g per chunk row
constexpr int kGS = 144;                               // B: row stride of a chunk: 16 mod 32, >= kWin
constexpr int kRun = 7;                                // B: frames per stencil thread: 16 runs per channel cover kTB

inline bool shape_ok(int D, int Hc) { return D == 512 && Hc == 128; }
// the table, in floats: A0 [D x Hc], bc [D], A1 [4 D x D], b1 [4 D], wd [2 D][31], bd [2 D], A2 [D x 2 D], b2 [D]
constexpr size_t off_bc(int D, int Hc) { return (size_t)D * Hc; }
constexpr size_t off_a1(int D, int Hc) { return off_bc(D, Hc) + D; }
constexpr size_t off_b1(int D, int Hc) { return off_a1(D, Hc) + (size_t)4 * D * D; }
constexpr size_t off_wd(int D, int Hc) { return off_b1(D, Hc) + 4 * D; }
constexpr size_t off_bd(int D, int Hc) { return off_wd(D, Hc) + (size_t)2 * D * kTaps; }
constexpr size_t off_a2(int D, int Hc) { return off_bd(D, Hc) + 2 * D; }
constexpr size_t off_b2(int D, int Hc) { return off_a2(D, Hc) + (size_t)2 * D * D; }
constexpr size_t table_floats(int D, int Hc) { return off_b2(D, Hc) + D; }

struct Args {
  const float* x; const float* cond; const float* d;   // [B, L, D], [B, L, Hc], [B, D]
  float* y;                                            // [B, L, D]
  float* g;                                            // the workspace: [B, 2 D, L]
  const float* tab;
  long L; long b0;
};

__device__ __forceinline__ float sigmoid(float v) { return 1.f / (1.f + expf(-v)); }   // expf(-v) = inf gives 0, never a NaN

template <int D, int Hc>
__global__ __launch_bounds__(kThreads) void k_naive_v2_glu(Args a) {
  constexpr int XS = D + 2, I = 2 * D, MT0 = D / 16 / kWaves, KS0 = Hc / 4, KS1 = D / 4, NR = I / (32 * kWaves);
  static_assert(D % (16 * kWaves) == 0 && Hc % 4 == 0 && I % (32 * kWaves) == 0 && KS1 % kPF == 0,
                "rows of GEMM 0 per wave, whole rounds of GEMM 1, k-steps in runs of kPF");
  static_assert(XS % 32 == 2, "bank spread of the B fragments");
  __shared__ float xs[kTA * XS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const long b = a.b0 + blockIdx.y;
  const long t0 = (long)blockIdx.x * kTA;
  const long L = a.L;
  const float* xb = a.x + b * L * D;
  const float* cb = a.cond + b * L * Hc;
  const float* db = a.d + b * D;
  const float* tab = a.tab;
  const float* bc = tab + off_bc(D, Hc);
  const float* b1 = tab + off_b1(D, Hc);

  {
    // D fragment: col = l & 15, row = 4 (l >> 4) + r
    f32x4n acc[MT0][kNT];
#pragma unroll
    for (int m = 0; m < MT0; ++m) {
      const int c = 16 * (MT0 * wave + m) + 4 * lq;
      const float4 dv = *reinterpret_cast<const float4*>(db + c);
      const float4 bv = *reinterpret_cast<const float4*>(bc + c);
#pragma unroll
      for (int n = 0; n < kNT; ++n) {
        const long t = t0 + 16 * n + lj;
        float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < L) xv = *reinterpret_cast<const float4*>(xb + t * D + c);
        acc[m][n][0] = xv.x + dv.x + bv.x; acc[m][n][1] = xv.y + dv.y + bv.y;
        acc[m][n][2] = xv.z + dv.z + bv.z; acc[m][n][3] = xv.w + dv.w + bv.w;
      }
    }
    // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
    const float* pa = tab + (size_t)wave * MT0 * 64 + lane;              // + k-step * kWaves * MT0 * 64 + m * 64
    bool in[kNT];
    const float* pc[kNT];
#pragma unroll
    for (int n = 0; n < kNT; ++n) {
      const long t = t0 + 16 * n + lj;
      in[n] = t < L;
      pc[n] = cb + (in[n] ? t : 0) * Hc + lq;
    }
#pragma unroll 4
    for (int s = 0; s < KS0; ++s) {
      float av[MT0], bv[kNT];
#pragma unroll
      for (int n = 0; n < kNT; ++n) bv[n] = in[n] ? pc[n][4 * s] : 0.f;
#pragma unroll
      for (int m = 0; m < MT0; ++m) av[m] = pa[(size_t)s * kWaves * MT0 * 64 + m * 64];
#pragma unroll
      for (int m = 0; m < MT0; ++m)
#pragma unroll
        for (int n = 0; n < kNT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[n], acc[m][n], 0, 0, 0);
    }
#pragma unroll
    for (int m = 0; m < MT0; ++m)
#pragma unroll
      for (int n = 0; n < kNT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) xs[(16 * n + lj) * XS + 16 * (MT0 * wave + m) + 4 * lq + r] = acc[m][n][r];
  }
  __syncthreads();

  // GEMM 1: the wave's table is one run of NR rounds x KS1 k-steps x 4 fragments (pair 0 out, pair 0 gate, pair 1 out, pair 1
  // gate); a ring of kPF register sets holds the k-steps ahead (KS1 is a multiple of kPF, so a step's set is its index mod kPF)
  const float* pa = tab + off_a1(D, Hc) + (size_t)wave * NR * KS1 * 256 + lane;
  const float* pb = xs + lj * XS + lq;
  float* gb = a.g + b * I * L;
  float ar[kPF][4];
#pragma unroll
  for (int q = 0; q < kPF; ++q)
#pragma unroll
    for (int f = 0; f < 4; ++f) ar[q][f] = pa[q * 256 + f * 64];
  for (int rd = 0; rd < NR; ++rd) {
    const int c0 = 32 * (rd * kWaves + wave);          // the wave's inner channels of this round
    f32x4n acc[4][kNT];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int n = 0; n < kNT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[f][n][r] = b1[(f & 1) * I + c0 + 16 * (f >> 1) + 4 * lq + r];
    for (int s = 0; s < KS1; s += kPF) {
      // the last kPF steps of the last round load again what they hold: nothing of this wave follows
      const int ahead = (rd + 1 < NR || s + kPF < KS1) ? kPF * 256 : 0;
#pragma unroll
      for (int q = 0; q < kPF; ++q) {
        float bv[kNT], av[4];
#pragma unroll
        for (int n = 0; n < kNT; ++n) bv[n] = pb[16 * n * XS + 4 * (s + q)];
#pragma unroll
        for (int f = 0; f < 4; ++f) { av[f] = ar[q][f]; ar[q][f] = pa[ahead + f * 64]; }
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
          for (int n = 0; n < kNT; ++n) acc[f][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[f], bv[n], acc[f][n], 0, 0, 0);
        pa += 256;
      }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int n = 0; n < kNT; ++n) {
        const long t = t0 + 16 * n + lj;
        if (t >= L) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          gb[(long)(c0 + 16 * p + 4 * lq + r) * L + t] = acc[2 * p][n][r] * sigmoid(acc[2 * p + 1][n][r]);
      }
  }
}

template <int D, int Hc>
__global__ __launch_bounds__(kThreads) void k_naive_v2_out(Args a) {
  constexpr int I = 2 * D, NCH = I / kCH, KS2 = kCH / 4, MT2 = D / 16 / kWaves;
  constexpr int NLD = (kCH * kWin + kThreads - 1) / kThreads;
  static_assert(D % (16 * kWaves) == 0 && I % kCH == 0, "rows of GEMM 2 per wave, whole chunks");
  static_assert(kThreads == kCH * 16 && 16 * kRun == kTB && 15 * kRun + kRun - 1 + kTaps - 1 < kWin,
                "stencil threads: 16 runs of 7 cover the tile and stay inside the window");
  static_assert(kGS % 32 == 16 && kGS >= kWin, "bank spread of the B fragments");
  __shared__ float gs[kCH * kGS];
  __shared__ float hs[kCH * kGS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const long b = a.b0 + blockIdx.y;
  const long t0 = (long)blockIdx.x * kTB;
  const long L = a.L;
  const float* gb = a.g + b * I * L;
  const float* wd = a.tab + off_wd(D, Hc);
  const float* bd = a.tab + off_bd(D, Hc);
  const float* A2 = a.tab + off_a2(D, Hc);
  const float* b2 = a.tab + off_b2(D, Hc);

  // chunk ch, element i -> channel i / kWin of the chunk at frame t0 - kHalo + i % kWin
  float stage[NLD];
  auto fetch = [&](int ch) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int i = tid + kThreads * u;
      const int cc = i / kWin, col = i - cc * kWin;
      const long p = t0 - kHalo + col;
      float v = 0.f;
      if (i < kCH * kWin && p >= 0 && p < L) v = gb[(long)(ch * kCH + cc) * L + p];
      stage[u] = v;
    }
  };

  // D fragment: col = l & 15, row = 4 (l >> 4) + r
  f32x4n acc[MT2][kN2];
#pragma unroll
  for (int m = 0; m < MT2; ++m)
#pragma unroll
    for (int n = 0; n < kN2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[m][n][r] = b2[16 * (MT2 * wave + m) + 4 * lq + r];

  const int sc = tid >> 4, run = tid & 15;             // stencil: channel of the chunk, run of kRun frames
  const float* pb = hs + lq * kGS + lj;
  fetch(0);
  for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {                    // every wave read its windows of the previous chunk before GEMM 2 began
      const int i = tid + kThreads * u;
      const int cc = i / kWin, col = i - cc * kWin;
      if (i < kCH * kWin) gs[cc * kGS + col] = stage[u];
    }
    __syncthreads();                                   // and every wave is done with the previous chunk's hs
    if (ch + 1 < NCH) fetch(ch + 1);

    {
      const int c = ch * kCH + sc;
      const float* g = gs + sc * kGS + run * kRun;
      float win[kRun + kTaps - 1], o[kRun];
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
      for (int u = 0; u < kRun; ++u) hs[sc * kGS + run * kRun + u] = o[u] * sigmoid(o[u]);
    }
    __syncthreads();

    // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
    const float* pa = A2 + ((size_t)(ch * KS2) * kWaves + wave) * MT2 * 64 + lane;
#pragma unroll 4
    for (int ks = 0; ks < KS2; ++ks) {
      float bv[kN2], av[MT2];
#pragma unroll
      for (int n = 0; n < kN2; ++n) bv[n] = pb[4 * ks * kGS + 16 * n];
#pragma unroll
      for (int m = 0; m < MT2; ++m) av[m] = pa[(size_t)ks * kWaves * MT2 * 64 + m * 64];
#pragma unroll
      for (int m = 0; m < MT2; ++m)
#pragma unroll
        for (int n = 0; n < kN2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[n], acc[m][n], 0, 0, 0);
    }
  }

  const float* xb = a.x + b * L * D;
  float* yb = a.y + b * L * D;
#pragma unroll
  for (int m = 0; m < MT2; ++m)
#pragma unroll
    for (int n = 0; n < kN2; ++n) {
      const long t = t0 + 16 * n + lj;
      if (t >= L) continue;
      const long e = t * D + 16 * (MT2 * wave + m) + 4 * lq;
      const float4 xv = *reinterpret_cast<const float4*>(xb + e);
      *reinterpret_cast<float4*>(yb + e) =
          make_float4(xv.x + acc[m][n][0], xv.y + acc[m][n][1], xv.z + acc[m][n][2], xv.w + acc[m][n][3]);
    }
}

template <int D, int Hc>
inline void launch_d(Args a, int B, hipStream_t st) {
  const long tiles_a = (a.L + kTA - 1) / kTA, tiles_b = (a.L + kTB - 1) / kTB;
  const long split = batch_split();
  for (long b0 = 0; b0 < B; b0 += split) {
    a.b0 = b0;
    const long nb = B - b0 < split ? B - b0 : split;
    hipLaunchKernelGGL((k_naive_v2_glu<D, Hc>), dim3((unsigned)tiles_a, (unsigned)nb), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL((k_naive_v2_out<D, Hc>), dim3((unsigned)tiles_b, (unsigned)nb), dim3(kThreads), 0, st, a);
  }
}

}  // namespace nv2

// ---- host side ---------------------------------------------------------------------------------------------------------------

size_t naive_v2_layer_pack_bytes(int D, int Hc) {
  if (!nv2::shape_ok(D, Hc)) return 0;
  return nv2::table_floats(D, Hc) * sizeof(float);
}

size_t naive_v2_layer_ws_bytes(long B, long L, int D) { return (size_t)B * (size_t)L * 2 * D * sizeof(float); }

// wc [D][Hc], bc [D], w1 [4 D][D], b1 [4 D], wd [2 D][31], bd [2 D], w2 [D][2 D], b2 [D]: host memory, as is out.
// A0: per k-step s, wave v, fragment m, lane l: Wc[16 (4 v + m) + (l & 15)][4 s + (l >> 4)].
// A1: per wave v, round rd, k-step s, pair p, GLU half h (0 out, 1 gate), lane l:
//     W1[2 D h + 32 (8 rd + v) + 16 p + (l & 15)][4 s + (l >> 4)].
// A2: per chunk c, k-step s, wave v, fragment m, lane l: W2[16 (4 v + m) + (l & 15)][32 c + 4 s + (l >> 4)].
void naive_v2_layer_pack(const float* wc, const float* bc, const float* w1, const float* b1, const float* wd, const float* bd,
                         const float* w2, const float* b2, int D, int Hc, float* out) {
  using namespace nv2;
  const int I = 2 * D, MT = D / 16 / kWaves, NR = I / (32 * kWaves);
  float* p = out;
  for (int s = 0; s < Hc / 4; ++s)
    for (int v = 0; v < kWaves; ++v)
      for (int m = 0; m < MT; ++m)
        for (int l = 0; l < 64; ++l) *p++ = wc[(size_t)(16 * (MT * v + m) + (l & 15)) * Hc + 4 * s + (l >> 4)];
  for (int i = 0; i < D; ++i) *p++ = bc[i];
  for (int v = 0; v < kWaves; ++v)
    for (int rd = 0; rd < NR; ++rd)
      for (int s = 0; s < D / 4; ++s)
        for (int pr = 0; pr < 2; ++pr)
          for (int h = 0; h < 2; ++h)
            for (int l = 0; l < 64; ++l)
              *p++ = w1[(size_t)(I * h + 32 * (kWaves * rd + v) + 16 * pr + (l & 15)) * D + 4 * s + (l >> 4)];
  for (int i = 0; i < 4 * D; ++i) *p++ = b1[i];
  for (int i = 0; i < I * kTaps; ++i) *p++ = wd[i];
  for (int i = 0; i < I; ++i) *p++ = bd[i];
  for (int c = 0; c < I / kCH; ++c)
    for (int s = 0; s < kCH / 4; ++s)
      for (int v = 0; v < kWaves; ++v)
        for (int m = 0; m < MT; ++m)
          for (int l = 0; l < 64; ++l) *p++ = w2[(size_t)(16 * (MT * v + m) + (l & 15)) * I + kCH * c + 4 * s + (l >> 4)];
  for (int i = 0; i < D; ++i) *p++ = b2[i];
}

// two launches per 65 535 utterances.  packed: naive_v2_layer_pack's floats on the device; ws: naive_v2_layer_ws_bytes.
void launch_naive_v2_layer(const float* x, const float* cond, const float* d, float* y, const float* packed, float* ws, int B,
                           long L, int D, int Hc, hipStream_t st) {
  nv2::Args a;
  a.x = x; a.cond = cond; a.d = d; a.y = y; a.g = ws; a.tab = packed; a.L = L; a.b0 = 0;
  nv2::launch_d<512, 128>(a, B, st);
  (void)D; (void)Hc;
}

}  // namespace ddsp
