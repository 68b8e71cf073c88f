// The performer attention of PCmer (ddsp/pcmer.py: softmax_kernel :14-47, linear_attention :218-232, FastAttention.forward
// :297-325) as TWO launches, the [N, 266] feature maps of the queries and the keys kept on the CU.  Included from api.hip only.
//
// Per batch item b and head h, with q, k, v [N, 64], P [266, 64], dn = 64^-0.25, ratio = 266^-0.5:
//     (normalize only)  q = q / (|q| + 1e-8),  k = k / (|k| + 1e-8)
//     dq = (dn q) P^T,  dk = (dn k) P^T;   gq = |q|^2 / 2 * dn^2,  gk = |k|^2 / 2 * dn^2
//     q' = ratio (exp(dq - gq - rowmax(dq)) + 1e-4);   k' = ratio exp(dk - gk + 1e-4)
//     ksum = sum_n k',  ctx = k'^T v;   out = (q' ctx) / (q' . ksum + 1e-8)
// computed as written: the row maximum and the two small constants are not simplified away.
//
// Both kernels: 4 waves, tiles of 64 frames, f32 MFMA 16x16x4, the 266 features padded to 17 fragments of 16.  The table is
// dn P in fragment order (lane l of fragment (m, s) holds dn P[16 m + (l & 15)][4 s + (l >> 4)], rows past 266 zero): the same
// lane map serves as GEMM 1's B operand on the key side and as its A operand on the query side.
//
// k_performer_key: grid B H chunks (flat in x: no 65 535 limit).  A workgroup walks the tiles of its chunk:
//   1. k and v rows -> LDS [64][68] (row stride 4 mod 32: both fragment reads below are bank-conflict free within a half wave),
//      the optional normalisation and gk per row by 16 lanes and four xor-shuffles.
//   2. wave w owns the feature fragments m = w, w + 4, ... (5, 4, 4, 4).  Per fragment it loads the 16 table fragments once, then
//      per block of 16 frames: GEMM 1 with the FRAMES on M, so that lane (lj, lq) ends with k' of feature 16 m + lj at frames
//      4 lq + r -- which is exactly GEMM 2's B operand (k = frame) for the k-step "frames {4 lq + r}": k' never leaves registers.
//      GEMM 2: ctx^T [e][feature] += v^T k', A from the v rows in LDS.  The column sums add up per lane.
//   3. one partial per workgroup -> workspace: ctx [272][64], then ksum [272].  No atomics: the query pass adds the partials of a
//      (b, h) in chunk order.
//   A padded feature (>= 266) and a frame past N give k' = 0 by a select, so neither a zero key row (exp(1e-4) != 0) nor whatever
//   the table's padding holds reaches ctx or ksum.
// k_performer_query: grid B H ceil(N / 64).  The chunk partials are summed into LDS (272 x 68 + 272 floats), the q rows staged as
//   above; then wave w owns frames [16 w, 16 w + 16) alone: GEMM 1 with the FEATURES on M (17 accumulators, lane (lj, lq) holds
//   features 16 m + 4 lq + r of frame lj), the row maximum over the real features inside the wave (registers and two shuffles),
//   exp, and GEMM 2 out^T [e][frame] with q' as the B operand straight from those registers (k-step "(m, r)" = features
//   {16 m + 4 lq + r}), A from ctx in LDS; the denominator q' . ksum per lane and two shuffles; float4 stores of 4 consecutive e.
// LDS: key 35 KB; query 92.7 KB (one workgroup per CU).  DESIGN.md 7.10 has the arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace ddsp {
namespace perf {

typedef float f32x4a __attribute__((ext_vector_type(4)));

constexpr int kD = 64;                                 // head width
constexpr int kM = 266;                                // features: int(64 ln 64)
constexpr int kMF = 17;                                // 16-feature fragments
constexpr int kMP = 16 * kMF;                          // 272
constexpr int kS1 = kD / 4;                            // k-steps of GEMM 1
constexpr int kTile = 64;                              // frames per tile
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRS = 68;                                // row stride of a staged q / k / v tile and of ctx: 4 mod 32
constexpr int kNM = (kMF + kWaves - 1) / kWaves;       // feature fragments per wave of the key pass, at most
constexpr int kPart = kMP * kD + kMP;                  // floats of one partial: ctx [272][64], ksum [272]
constexpr int kCUs = 256;                              // the chunk rule fills this many
constexpr float kEps = 1e-4f;

inline bool shape_ok(int d, int m) { return d == kD && m == kM; }
constexpr size_t table_floats() { return (size_t)kMF * kS1 * 64; }
inline long tiles_of(long N) { return (N + kTile - 1) / kTile; }
inline long clamp_chunks(long chunks, long N) { const long t = tiles_of(N); return chunks > t ? t : chunks; }

struct Args {
  const float* q; const float* k; const float* v; float* out;
  const float* tab; float* ws;
  long sq[3], sk[3], sv[3], so[3];                     // (batch, head, frame) strides in floats; the 64 are contiguous
  long N;
  int H, chunks, tiles, normalize;
};

// rows [n0, n0 + 64) of x -> dst [64][kRS], zeros past N; with g: the optional row normalisation and |row|^2 / 2 * dn^2 (dn^2 = 1/8)
__device__ __forceinline__ void stage_rows(const float* x, long stride, long n0, long N, float* dst, float* g, int normalize,
                                           int tid) {
#pragma unroll
  for (int it = 0; it < kTile * (kD / 4) / kThreads; ++it) {
    const int i = tid + kThreads * it, fr = i >> 4, c4 = i & 15;
    const long n = n0 + fr;
    float4 x4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < N) x4 = *reinterpret_cast<const float4*>(x + n * stride + 4 * c4);
    if (g) {
      float ss = x4.x * x4.x + x4.y * x4.y + x4.z * x4.z + x4.w * x4.w;
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) ss += __shfl_xor(ss, m);
      if (normalize) {
        const float den = sqrtf(ss) + 1e-8f;
        x4.x /= den; x4.y /= den; x4.z /= den; x4.w /= den;
        ss = x4.x * x4.x + x4.y * x4.y + x4.z * x4.z + x4.w * x4.w;
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) ss += __shfl_xor(ss, m);
      }
      if (c4 == 0) g[fr] = ss * 0.0625f;
    }
    float* d = dst + fr * kRS + 4 * c4;
    d[0] = x4.x; d[1] = x4.y; d[2] = x4.z; d[3] = x4.w;
  }
}

__global__ __launch_bounds__(kThreads) void k_performer_key(Args a) {
  __shared__ float ks[kTile * kRS];
  __shared__ float vs[kTile * kRS];
  __shared__ float gk[kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const long wg = blockIdx.x;
  const int c = (int)(wg % a.chunks);
  const long bh = wg / a.chunks;
  const int h = (int)(bh % a.H);
  const long b = bh / a.H;
  const float* kb = a.k + b * a.sk[0] + h * a.sk[1];
  const float* vb = a.v + b * a.sv[0] + h * a.sv[1];
  const long t_begin = (long)c * a.tiles / a.chunks, t_end = (long)(c + 1) * a.tiles / a.chunks;
  const float ratio = 1.f / sqrtf((float)kM);
  const int nm = (kMF - wave + kWaves - 1) / kWaves;   // this wave's fragments: m = wave + kWaves i

  // D fragment of GEMM 2: col = l & 15 = feature, row = 4 (l >> 4) + r = e
  f32x4a acc[kNM][kD / 16];
  float ksum[kNM];
#pragma unroll
  for (int i = 0; i < kNM; ++i) {
    ksum[i] = 0.f;
#pragma unroll
    for (int e = 0; e < kD / 16; ++e)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][e][r] = 0.f;
  }

  for (long t = t_begin; t < t_end; ++t) {
    const long n0 = t * kTile;
    __syncthreads();                                   // every wave is done with the previous tile
    stage_rows(kb, a.sk[2], n0, a.N, ks, gk, a.normalize, tid);
    stage_rows(vb, a.sv[2], n0, a.N, vs, nullptr, 0, tid);
    __syncthreads();
    const long left = a.N - n0;
    const int nfb = left >= kTile ? kTile / 16 : (int)((left + 15) / 16);
#pragma unroll
    for (int i = 0; i < kNM; ++i) {
      if (i >= nm) continue;                           // wave-uniform
      const int m = wave + kWaves * i;
      const bool live = 16 * m + lj < kM;
      float bt[kS1];
#pragma unroll
      for (int s = 0; s < kS1; ++s) bt[s] = a.tab[(size_t)(m * kS1 + s) * 64 + lane];
      for (int fb = 0; fb < nfb; ++fb) {
        // GEMM 1, frames on M: A[i = frame lj][k = lq] from ks, B[k = lq][j = feature lj] from the table
        f32x4a d;
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = 0.f;
        const float* pa = ks + (16 * fb + lj) * kRS + lq;
#pragma unroll
        for (int s = 0; s < kS1; ++s) d = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[4 * s], bt[s], d, 0, 0, 0);
        // d[r]: frame 16 fb + 4 lq + r, feature 16 m + lj
        float kp[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int fr = 16 * fb + 4 * lq + r;
          const bool in = live && n0 + fr < a.N;
          kp[r] = in ? ratio * expf(d[r] - gk[fr] + kEps) : 0.f;
          ksum[i] += kp[r];
        }
        // GEMM 2, k-step r = frames {16 fb + 4 lq + r}: A[i = e lj][k = lq] = v[frame][e], B[k = lq][j = feature lj] = kp[r]
        const float* pv = vs + (16 * fb + 4 * lq) * kRS + lj;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int e = 0; e < kD / 16; ++e)
            acc[i][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[r * kRS + 16 * e], kp[r], acc[i][e], 0, 0, 0);
      }
    }
  }

  float* part = a.ws + (size_t)wg * kPart;
#pragma unroll
  for (int i = 0; i < kNM; ++i) {
    if (i >= nm) continue;
    const int f = 16 * (wave + kWaves * i) + lj;
#pragma unroll
    for (int e = 0; e < kD / 16; ++e)
      *reinterpret_cast<float4*>(part + f * kD + 16 * e + 4 * lq) = make_float4(acc[i][e][0], acc[i][e][1], acc[i][e][2], acc[i][e][3]);
    float s = ksum[i];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (lq == 0) part[kMP * kD + f] = s;
  }
}

__global__ __launch_bounds__(kThreads) void k_performer_query(Args a) {
  __shared__ float ctx[kMP * kRS];
  __shared__ float ksum[kMP];
  __shared__ float qs[kTile * kRS];
  __shared__ float gq[kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane >> 4, lj = lane & 15;
  const long wg = blockIdx.x;
  const long t = wg % a.tiles;
  const long bh = wg / a.tiles;
  const int h = (int)(bh % a.H);
  const long b = bh / a.H;
  const long n0 = t * kTile;
  const float ratio = 1.f / sqrtf((float)kM);

  stage_rows(a.q + b * a.sq[0] + h * a.sq[1], a.sq[2], n0, a.N, qs, gq, a.normalize, tid);
  const float* part = a.ws + (size_t)bh * a.chunks * kPart;
  for (int i = tid; i < kMP * (kD / 4); i += kThreads) {
    const int f = i >> 4, c4 = i & 15;
    float4 s = *reinterpret_cast<const float4*>(part + f * kD + 4 * c4);
    for (int c = 1; c < a.chunks; ++c) {               // in chunk order: a call is reproducible
      const float4 p = *reinterpret_cast<const float4*>(part + (size_t)c * kPart + f * kD + 4 * c4);
      s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
    }
    float* d = ctx + f * kRS + 4 * c4;
    d[0] = s.x; d[1] = s.y; d[2] = s.z; d[3] = s.w;
  }
  for (int f = tid; f < kMP; f += kThreads) {
    float s = part[kMP * kD + f];
    for (int c = 1; c < a.chunks; ++c) s += part[(size_t)c * kPart + kMP * kD + f];
    ksum[f] = s;
  }
  __syncthreads();
  if (n0 + 16 * wave >= a.N) return;                   // no frame of this wave exists; no barrier follows

  // GEMM 1, features on M: A[i = feature lj][k = lq] from the table, B[k = lq][j = frame lj] from qs
  f32x4a d[kMF];
#pragma unroll
  for (int m = 0; m < kMF; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) d[m][r] = 0.f;
  const float* pb = qs + (16 * wave + lj) * kRS + lq;
  const float* pt = a.tab + lane;
#pragma unroll 2
  for (int s = 0; s < kS1; ++s) {
    const float bq = pb[4 * s];
#pragma unroll
    for (int m = 0; m < kMF; ++m) d[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(pt[(size_t)(m * kS1 + s) * 64], bq, d[m], 0, 0, 0);
  }
  // d[m][r]: feature 16 m + 4 lq + r of frame 16 wave + lj; the row maximum over the 266 real ones
  float mx = -INFINITY;
#pragma unroll
  for (int m = 0; m < kMF; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * m + 4 * lq + r < kM) mx = fmaxf(mx, d[m][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float g = gq[16 * wave + lj];
  float den = 0.f;
#pragma unroll
  for (int m = 0; m < kMF; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 16 * m + 4 * lq + r;
      const float qp = f < kM ? ratio * (expf(d[m][r] - g - mx) + kEps) : 0.f;
      d[m][r] = qp;
      den = __fmaf_rn(qp, ksum[f], den);
    }
  den += __shfl_xor(den, 16);
  den += __shfl_xor(den, 32);

  // GEMM 2, k-step (m, r) = features {16 m + 4 lq + r}: A[i = e lj][k = lq] = ctx[feature][e], B[k = lq][j = frame lj] = d[m][r]
  f32x4a o[kD / 16];
#pragma unroll
  for (int e = 0; e < kD / 16; ++e)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[e][r] = 0.f;
  const float* pc = ctx + 4 * lq * kRS + lj;
#pragma unroll
  for (int m = 0; m < kMF; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int e = 0; e < kD / 16; ++e)
        o[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(pc[(16 * m + r) * kRS + 16 * e], d[m][r], o[e], 0, 0, 0);

  const long n = n0 + 16 * wave + lj;
  if (n >= a.N) return;
  const float inv = 1.f / (den + 1e-8f);
  float* ob = a.out + b * a.so[0] + h * a.so[1] + n * a.so[2];
#pragma unroll
  for (int e = 0; e < kD / 16; ++e)                    // o[e][r]: e index 16 e + 4 lq + r
    *reinterpret_cast<float4*>(ob + 16 * e + 4 * lq) = make_float4(o[e][0] * inv, o[e][1] * inv, o[e][2] * inv, o[e][3] * inv);
}

}  // namespace perf

// ---- host side ---------------------------------------------------------------------------------------------------------------

size_t performer_pack_bytes(int d, int m) { return perf::shape_ok(d, m) ? perf::table_floats() * sizeof(float) : 0; }

// proj [266][64] and out in host memory; rows past 266 are zero
void performer_pack(const float* proj, float* out) {
  using namespace perf;
  const float dn = 1.f / sqrtf(sqrtf((float)kD));
  for (int m = 0; m < kMF; ++m)
    for (int s = 0; s < kS1; ++s)
      for (int l = 0; l < 64; ++l) {
        const int f = 16 * m + (l & 15);
        out[((size_t)m * kS1 + s) * 64 + l] = f < kM ? dn * proj[(size_t)f * kD + 4 * s + (l >> 4)] : 0.f;
      }
}

// the default chunk count: B H chunks workgroups fill the CUs, and a chunk holds at least one tile
int performer_chunks(long B, long H, long N) {
  const long bh = B * H > 0 ? B * H : 1;
  long c = (perf::kCUs + bh - 1) / bh;
  c = perf::clamp_chunks(c, N);
  return (int)(c < 1 ? 1 : c);
}

size_t performer_ws_bytes(long B, long H, long N, long chunks) {
  return (size_t)B * H * perf::clamp_chunks(chunks, N) * perf::kPart * sizeof(float);
}

// strides: (batch, head, frame) of q, k, v, out in floats.  Two launches on st.
void launch_performer_attention(const float* q, const float* k, const float* v, float* out, const long* strides, const float* tab,
                                float* ws, long B, int H, long N, int normalize, long chunks, hipStream_t st) {
  perf::Args a;
  a.q = q; a.k = k; a.v = v; a.out = out; a.tab = tab; a.ws = ws;
  for (int i = 0; i < 3; ++i) { a.sq[i] = strides[i]; a.sk[i] = strides[3 + i]; a.sv[i] = strides[6 + i]; a.so[i] = strides[9 + i]; }
  a.N = N; a.H = H; a.tiles = (int)perf::tiles_of(N); a.chunks = (int)perf::clamp_chunks(chunks, N); a.normalize = normalize;
  hipLaunchKernelGGL(perf::k_performer_key, dim3((unsigned)(B * H * a.chunks)), dim3(perf::kThreads), 0, st, a);
  hipLaunchKernelGGL(perf::k_performer_query, dim3((unsigned)(B * H * a.tiles)), dim3(perf::kThreads), 0, st, a);
}

}  // namespace ddsp
