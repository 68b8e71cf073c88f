// The channel-split form of wavenet_layer.h's layer, for calls of a few hundred frames: the same mathematics, layouts, packed table
// and SUMS (every accumulator starts at the same value and walks k in the same order, so the result is bit-identical to
// ddsp_hip_wavenet_layer), tiled the other way round.  The frame tile is ONE 16-frame MFMA fragment and the channels are split over
// blockIdx.y and the waves of a workgroup, so that 1 x 100 frames are a few hundred waves instead of two workgroups.  The one
// dependency between workgroups -- every output row needs all C gate channels -- is a launch boundary: two plain launches on the
// caller's stream, no flags, no atomics.  Included from api.hip only, after wavenet_layer.h.
//
//     g = sigmoid(z[:C]) * tanh(z[C:])     k_wns_gate  grid (1, C / 16 / G, B tiles), 2 G waves (G = 1 at C = 384, 2 at C = 512):
//       z = dil3(x + d) + Wc cond + b1       the tile's x + d -> LDS xs [16 + 2][C + 2] (frames t0 - 1 .. t0 + 16, zeros outside
//                                            [0, T)) and its cond -> cs [16][H + 2] (zeros at frames >= T), a frame's channels
//                                            consecutive: lanes (k = l >> 4, frame = l & 15) of a half wave read 32 different banks
//                                            at a row stride of 2 mod 32.  A wave PAIR owns 16 channels: the even wave their gate
//                                            fragment (f = m of the tiled kernel's wave v), the odd wave their filter fragment
//                                            (f = C / 128 + m), ONE chain of (3 C + H) / 4 MFMAs each in the tiled kernel's order
//                                            (chunk of 32 channels, tap, k-step of the chunk; then cond), the weight fragments kPF
//                                            k-steps ahead in a register ring that is filled BEFORE the tile is staged.  The odd
//                                            wave hands tanh of its 16 x 16 values over in LDS, the even wave stores g [B][C][T].
//     o = Wo g + bo                        k_wns_out   grid (1, 2 C / 16 / W, B tiles), W waves (3 at C = 384, 4 at C = 512): a
//                                            wave owns one 16-row block x 16 frames, one chain of C / 4 MFMAs; the B fragment of a
//                                            k-step is four rows of g, 16 consecutive frames each; both operands of the first kPF
//                                            k-steps (all of them at C = 384) are loaded before the first MFMA.  The epilogue is the tiled kernel's.
// Staged in LDS and not read from memory ahead of use in launch 1: every value of x + d is a B operand three times (once per
// tap, at three frame offsets), and the zero outside [0, T) is one select while staging instead of three per k-step.
// Frames >= T of the last tile: their x + d and cond are zeros in launch 1, their g is read at frame T - 1 in launch 2 (a column
// of an MFMA never reaches another column); none of their results is stored, so nothing is read past a row.
// The workspace is g: B T C floats.  tiles = ceil(T / 16); B tiles <= kMaxTiles, on the grid's z with the channel groups on y.
// LDS: 18 (C + 2) + 16 (H + 2) + 256 G floats = 55 568 bytes at C = 512, 45 328 at C = 384 in launch 1, none in launch 2.
// DESIGN.md 7.9 has the arithmetic and the measurements.
#pragma once
#include "wavenet_layer.h"

namespace ddsp {
namespace wns {

using wnet::f32x4w;

constexpr int kT = 16;                                 // frames per workgroup: one MFMA fragment
constexpr int kW = kT + 2;                             // staged frames of x + d: the tile and one each side for the taps
constexpr int kCS = 24;                                // launch 1: k-steps of a chunk: 8 at each of the three taps
constexpr int kPC = 4;                                 // launch 1: chunks the weight fragments are loaded ahead
constexpr int kPF = kPC * kCS;                         // ... in k-steps: a wave is alone on its SIMD, and a round of the ring has to
                                                       // outlast a trip to memory; launch 2: k-steps whose operands are loaded at once
constexpr long kMaxTiles = 4096;                       // B ceil(T / 16): the form is for small calls

// channel groups (wave pairs) per workgroup of launch 1 and waves (row blocks) per workgroup of launch 2: a wave is alone on its
// SIMD at the real-time sizes, and the number of workgroups per tile is a multiple of 8 (launch_c)
constexpr int gate_groups(int C) { return C == 512 ? 2 : 1; }
constexpr int out_waves(int C) { return C == 512 ? 4 : 3; }

struct Args {
  const float* x; const float* cond; const float* d;   // [B, C, T], [B, H, T], [B, C]
  float* x_out; float* skip;                           // [B, C, T] each
  float* g;                                            // the workspace: [B, C, T]
  const float* tab;
  long T; long tiles;                                  // tiles = ceil(T / kT)
  int skip_mode;                                       // 0: store the skip rows, 1: add them to what is there
};

template <int C, int H, int G>
__global__ __launch_bounds__(128 * G) void k_wns_gate(Args a) {
  constexpr int NW = 2 * G, MT = C / 128, NF = 2 * MT;
  constexpr int XS = C + 2, CS = H + 2;
  constexpr int NXC = C / wnet::kKC, KSC = H / 4;      // chunks of x + d, k-steps of cond
  constexpr int AST = wnet::kWaves * NF * 64;          // floats of the table per k-step
  static_assert(wnet::kKC == 32 && kCS == 3 * wnet::kKC / 4 && NXC % kPC == 0, "a round of the ring is kPC chunks at their three taps");
  static_assert(C % 128 == 0 && C % wnet::kKC == 0 && H % 4 == 0 && KSC <= kPF && (C / 16) % G == 0, "whole chunks and workgroups");
  static_assert(XS % 32 == 2 && CS % 32 == 2, "bank spread of the B fragments");
  __shared__ float xs[kW * XS];
  __shared__ float cs[kT * CS];
  __shared__ float ex[G * 256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const long b = blockIdx.z / a.tiles, T = a.T;
  const long t0 = (blockIdx.z - b * a.tiles) * kT;
  // the pair's 16 channels are block m of the C / 8 that wave v of the tiled kernel owns
  const int grp = blockIdx.y * G + (wave >> 1), half = wave & 1;
  const int v = grp / MT, m = grp - v * MT, f = half * MT + m;
  const int c0 = 16 * grp;
  // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
  const float* pa = a.tab + ((size_t)v * NF + f) * 64 + lane;          // + k-step * AST
  float ar[kPF];
#pragma unroll
  for (int q = 0; q < kPF; ++q) ar[q] = pa[(size_t)q * AST];

  // x + d: a wave takes three channels x 18 frames a round (54 of its lanes), a lane keeps its frame; cond: four channels x 16
  const float* xb = a.x + b * C * T;
  const float* cb = a.cond + b * H * T;
  const float* db = a.d + b * C;
  // Every load is unconditional at a clamped address and the zero is a select afterwards: a load under a branch cannot be
  // issued before the branch before it is decided, and the staging would be one trip to memory per round instead of one per batch.
  {
    constexpr int NXI = (C + 3 * NW - 1) / (3 * NW), SB = (NXI + 1) / 2, NCI = H / (4 * NW);
    static_assert(H % (4 * NW) == 0, "whole rounds of cond");
    const int cl = lane / kW, col = lane - cl * kW;
    const long p = t0 - 1 + col;
    const bool ok = cl < 3 && p >= 0 && p < T;
    const long pc = p < 0 ? 0 : (p < T ? p : T - 1);
    for (int i0 = 0; i0 < NXI; i0 += SB) {
      float sx[SB], sd[SB];
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const int c = min(3 * wave + cl + 3 * NW * (i0 + u), C - 1);
        sx[u] = xb[c * T + pc]; sd[u] = db[c];
      }
#pragma unroll
      for (int u = 0; u < SB; ++u) {
        const int c = 3 * wave + cl + 3 * NW * (i0 + u);
        if (cl < 3 && c < C) xs[col * XS + c] = ok ? sx[u] + sd[u] : 0.f;
      }
    }
    const bool in = t0 + lj < T;
    const long tc = in ? t0 + lj : T - 1;
    float sc[NCI];
#pragma unroll
    for (int u = 0; u < NCI; ++u) sc[u] = cb[(4 * wave + lq + 4 * NW * u) * T + tc];
#pragma unroll
    for (int u = 0; u < NCI; ++u) cs[lj * CS + 4 * wave + lq + 4 * NW * u] = in ? sc[u] : 0.f;
  }
  // D fragment: col = l & 15, row = 4 (l >> 4) + r
  const float* b1 = a.tab + wnet::off_b1(C, H);
  f32x4w acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = b1[half * C + c0 + 4 * lq + r];
  __syncthreads();

  const float* px = xs + lj * XS + lq;                 // + tap * XS + channel of the k-step's first row
  for (int ch = 0; ch < NXC; ch += kPC) {
    const bool more = ch + kPC < NXC;                  // the last round loads cond's KSC k-steps: the table continues there
#pragma unroll
    for (int u = 0; u < kPC; ++u) {
      float bv[kCS];
#pragma unroll
      for (int q = 0; q < kCS; ++q) bv[q] = px[(q / 8) * XS + (ch + u) * wnet::kKC + 4 * (q % 8)];
#pragma unroll
      for (int q = 0; q < kCS; ++q) {
        const float av = ar[u * kCS + q];
        if (more || u * kCS + q < KSC) ar[u * kCS + q] = pa[(size_t)kPF * AST];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[q], acc, 0, 0, 0);
        pa += AST;
      }
    }
  }
  const float* pc = cs + lj * CS + lq;
#pragma unroll
  for (int s = 0; s < KSC; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[s], pc[4 * s], acc, 0, 0, 0);

  // the gate: the filter wave hands tanh over, the gate wave multiplies and stores
  float* e = ex + (wave >> 1) * 256 + 4 * lane;
  if (half) {
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = tanhf(acc[r]);
  }
  __syncthreads();
  const long t = t0 + lj;
  if (half || t >= T) return;
  float* gb = a.g + b * C * T;
#pragma unroll
  for (int r = 0; r < 4; ++r) gb[(long)(c0 + 4 * lq + r) * T + t] = wnet::sigmoid(acc[r]) * e[r];
}

template <int C, int H, int W>
__global__ __launch_bounds__(64 * W) void k_wns_out(Args a) {
  constexpr int MT = C / 128, NF = 2 * MT, KS2 = C / 4, NB = C / 16;
  constexpr int AST = wnet::kWaves * NF * 64;
  static_assert((2 * NB) % W == 0 && KS2 >= kPF, "whole workgroups of row blocks");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  // row block rb of the [2 C] outputs: half rb / NB (residual, skip), channels 16 (rb % NB) ..: block m of the tiled kernel's wave v
  const int rb = blockIdx.y * W + wave;
  const int half = rb / NB, cg = rb - half * NB;
  const int v = cg / MT, m = cg - v * MT, f = half * MT + m;
  const long b = blockIdx.z / a.tiles, T = a.T;
  const long t = (blockIdx.z - b * a.tiles) * kT + lj;
  const bool in = t < T;
  // 16x16x4: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
  const float* pa = a.tab + wnet::off_a2(C, H) + ((size_t)v * NF + f) * 64 + lane;    // + k-step * AST
  const float* pb = a.g + (b * C + lq) * T + (in ? t : T - 1);                        // + k-step * 4 T
  float ar[kPF], br[kPF];                              // both operands of the first kPF k-steps (all of them at C = 384) at once
#pragma unroll
  for (int q = 0; q < kPF; ++q) { ar[q] = pa[(size_t)q * AST]; br[q] = pb[(long)q * 4 * T]; }
  __builtin_amdgcn_sched_barrier(0);                   // or the scheduler sinks the loads to their MFMAs to save registers
  const float* bo = a.tab + wnet::off_bo(C, H);
  const int c = 16 * cg + 4 * lq;
  // D fragment: col = l & 15, row = 4 (l >> 4) + r
  f32x4w acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = bo[half * C + c + r];
#pragma unroll
  for (int q = 0; q < KS2; ++q) {
    const float av = ar[q % kPF], bv = br[q % kPF];
    if (q + kPF < KS2) { ar[q % kPF] = pa[(size_t)(q + kPF) * AST]; br[q % kPF] = pb[(long)(q + kPF) * 4 * T]; }
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
  }
  if (!in) return;
  const float rs2 = 0.70710678118654752440f;
  const float* xb = a.x + b * C * T;
  float* ob = a.x_out + b * C * T;
  float* sb = a.skip + b * C * T;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long e = (long)(c + r) * T + t;
    const float o = acc[r];
    if (half == 0) ob[e] = (xb[e] + o) * rs2;
    else sb[e] = a.skip_mode ? sb[e] + o : o;
  }
}

inline long tiles_of(long T) { return (T + kT - 1) / kT; }
inline bool in_range(long B, long T) { return B <= kMaxTiles && tiles_of(T) <= kMaxTiles && B * tiles_of(T) <= kMaxTiles; }

template <int C, int H>
inline void launch_c(Args a, int B, hipStream_t st) {
  // the grids are (1, channel groups, B tiles): workgroups go round the chip's eight dies in the order of their linear index, and
  // 8 divides the number of channel groups, so all tiles that read one slice of a weight matrix share one die's L2
  constexpr int G = gate_groups(C), W = out_waves(C);
  static_assert(C / 16 / G % 8 == 0 && 2 * C / 16 / W % 8 == 0, "a channel group stays on its die");
  a.tiles = tiles_of(a.T);
  const unsigned nz = (unsigned)(B * a.tiles);
  hipLaunchKernelGGL((k_wns_gate<C, H, G>), dim3(1, C / 16 / G, nz), dim3(128 * G), 0, st, a);
  hipLaunchKernelGGL((k_wns_out<C, H, W>), dim3(1, 2 * C / 16 / W, nz), dim3(64 * W), 0, st, a);
}

}  // namespace wns

// ---- host side ---------------------------------------------------------------------------------------------------------------

size_t wavenet_split_ws_bytes(long B, long T, int C) { return (size_t)B * (size_t)T * C * sizeof(float); }

// two launches.  packed: wavenet_layer_pack's floats on the device; ws: wavenet_split_ws_bytes; B ceil(T / 16) <= 4096.
void launch_wavenet_split(const float* x, const float* cond, const float* d, float* x_out, float* skip, const float* packed,
                          float* ws, int B, long T, int C, int H, int skip_mode, hipStream_t st) {
  wns::Args a;
  a.x = x; a.cond = cond; a.d = d; a.x_out = x_out; a.skip = skip; a.g = ws; a.tab = packed; a.T = T; a.tiles = 0;
  a.skip_mode = skip_mode;
  if (C == 384) wns::launch_c<384, 256>(a, B, st);
  else wns::launch_c<512, 256>(a, B, st);
  (void)H;
}

}  // namespace ddsp
