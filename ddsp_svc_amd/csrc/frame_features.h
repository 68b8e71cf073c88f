// The frame features of the real-time path and the gate between them: the volume envelope (ddsp/vocoder.py:147-157), the silence
// gate (gui.py:114-118 and :134), the salience decode behind RMVPE / FCPE (encoder/rmvpe/utils.py:106-121), the F0 track's fill /
// retime / unvoiced handling (ddsp/vocoder.py:104-105, :110-118, :139-143) and the two pools of ddsp/core.py:8-45.  Included from
// api.hip only (one translation unit holds the kernels).
//
//   k_volume      sqrt(mean(x^2)) over the reflect-padded hops, one wave per frame, float64 sums            grid (ceil(F/4), B)
//   k_gate        signal * upsample(dilate(volume > thr)); the frame masks of a span in LDS, no mask tensor    grid (ceil(n/4096), B)
//   k_salience    first argmax, the 9-bin weighted mean of cents, 10 * 2^(cents/1200); one wave per frame      grid (ceil(rows/4))
//   k_f0_track    fill, retime, unvoiced flag, second fill and floor: one workgroup per row, five passes       grid (B)
//   k_pool1d      masked average / median over k <= 16 reflect-padded samples, one thread per output           grid (ceil(N/256), B)
//
// Where float64 is used: every sum that decides a rounding of the result (the squares of float32 samples are exact in float64; the
// 9-bin cents mean spans 9000 cents, so float32 would cost 3e-7 in f0) and all of the track's time arithmetic, which np.interp
// does in float64: the source times are the products period * i as the reference forms them, and the bracketing index is an
// estimate corrected against those products.  Comparisons that decide a result are made in the reference's own type: the volume and
// the row maximum in float32 against the float32 threshold, the retimed unvoiced flag in float64 against 0.5.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace ddsp {
namespace features {

constexpr int kThreads = 256;
constexpr int kGateSpan = 4096;                        // gate: samples per workgroup
constexpr int kGateVecs = kGateSpan / (4 * kThreads);  // ... 16-byte loads per thread, all issued before the masks are made
constexpr int kMaxDilate = 64;
constexpr int kBins = 360;                             // salience classes (encoder/rmvpe/constants.py)
constexpr double kCentsBase = 1997.3794084376191;
constexpr int kTrackThreads = 1024;                    // track: one workgroup of 16 waves per row
constexpr int kTrackWaves = kTrackThreads / 64;
constexpr int kMaxPool = 16;

template <class T> __device__ inline T lesser(T a, T b) { return a < b ? a : b; }
template <class T> __device__ inline T greater(T a, T b) { return a > b ? a : b; }

__device__ inline double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// numpy's reflect (the edge sample is not repeated) of index s into [0, n); one reflection, the callers bound the pad by n - 1
__device__ inline long reflect(long s, long n) { return s < 0 ? -s : (s >= n ? 2 * (n - 1) - s : s); }

// ---- volume ----------------------------------------------------------------------------------------------------------------
// frame f: the padded samples [f hop, (f + 1) hop), padded index p = source index p - hop / 2 reflected.  A lane takes groups of
// four consecutive samples (one 16-byte load where the frame lies inside the row and is aligned, four reflected loads otherwise)
// and adds their squares in that order either way, so the sum does not depend on the alignment of the caller's buffer.
__global__ __launch_bounds__(kThreads) void k_volume(const float* audio, long ld, long T, int hop, long F, float* vol) {
  const int lane = threadIdx.x & 63;
  const long f = (long)blockIdx.x * (kThreads / 64) + (long)(threadIdx.x >> 6);
  if (f >= F) return;                                  // wave-uniform
  const float* x = audio + (long)blockIdx.y * ld;
  const long s0 = f * hop - hop / 2;
  const bool inside = s0 >= 0 && s0 + hop <= T;
  const bool vec = inside && (hop & 3) == 0 && (reinterpret_cast<uintptr_t>(x + s0) & 15) == 0;
  double acc = 0.0;
  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(x + s0);
#pragma unroll 4
    for (int j = lane; j < hop / 4; j += 64) {
      const float4 v = x4[j];
      acc = fma((double)v.x, (double)v.x, acc);
      acc = fma((double)v.y, (double)v.y, acc);
      acc = fma((double)v.z, (double)v.z, acc);
      acc = fma((double)v.w, (double)v.w, acc);
    }
  } else {
    for (int j = 4 * lane; j < hop; j += 256) {
      for (int e = 0; e < 4 && j + e < hop; ++e) {
        const double v = (double)x[inside ? s0 + j + e : reflect(s0 + j + e, T)];
        acc = fma(v, v, acc);
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) vol[(long)blockIdx.y * F + f] = (float)sqrt(acc / (double)hop);
}

// ---- gate ------------------------------------------------------------------------------------------------------------------
// sample i of frame f = i / block, r = i mod block: m = mask[f] + (mask[f + 1] - mask[f]) r / block with mask[F] = mask[F - 1]
// (ddsp/core.py upsample), mask[f] = any(volume[g] > thr, |g - f| <= dilate, g clipped) (edge-replicated padding adds nothing to a
// maximum that already holds the edge frame).  Equal neighbours give the float product with 0 or 1, exact.
__device__ inline float gate_one(float x, const unsigned char* sm, long f_rel, int r, double inv_block) {
  const int m0 = sm[f_rel], m1 = sm[f_rel + 1];
  if (m0 == m1) return __fmul_rn(x, (float)m0);
  return (float)((double)x * ((double)m0 + (double)(m1 - m0) * ((double)r * inv_block)));
}

__global__ __launch_bounds__(kThreads) void k_gate(const float* sig, long ld_s, float* out, long ld_o, const float* vol, long F,
                                                   int block, int dilate, float thr, double inv_block, int vec) {
  __shared__ unsigned char sm[kGateSpan + 2];
  const long n = F * block;
  const long i0 = (long)blockIdx.x * kGateSpan;
  const long i1 = lesser(i0 + (long)kGateSpan, n);
  const long f0 = i0 / block;
  const int count = (int)((i1 - 1) / block - f0) + 2;  // masks f0 .. f(i1 - 1) + 1: at most kGateSpan / block + 2
  const float* s = sig + (long)blockIdx.y * ld_s;
  float* o = out + (long)blockIdx.y * ld_o;
  float4 x[kGateVecs];                                 // the signal is on its way while the frame masks are made
  if (vec) {
#pragma unroll
    for (int u = 0; u < kGateVecs; ++u) {
      const long i = i0 + 4 * ((long)threadIdx.x + (long)u * kThreads);
      x[u] = i + 4 <= i1 ? *reinterpret_cast<const float4*>(s + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const float* v = vol + (long)blockIdx.y * F;
  for (int t = threadIdx.x; t < count; t += kThreads) {
    const long f = lesser(f0 + t, F - 1);                 // the held last frame
    const long lo = greater(f - dilate, 0L), hi = lesser(f + dilate, F - 1);
    int m = 0;
    for (long g = lo; g <= hi; ++g) m |= v[g] > thr ? 1 : 0;
    sm[t] = (unsigned char)m;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kGateVecs; ++u) {
    const long i = i0 + 4 * ((long)threadIdx.x + (long)u * kThreads);
    if (i >= i1) continue;
    long f = i / block;
    int r = (int)(i - f * block);
    f -= f0;
    if (vec && i + 4 <= i1) {
      float4 y;
      y.x = gate_one(x[u].x, sm, f, r, inv_block); if (++r == block) { r = 0; ++f; }
      y.y = gate_one(x[u].y, sm, f, r, inv_block); if (++r == block) { r = 0; ++f; }
      y.z = gate_one(x[u].z, sm, f, r, inv_block); if (++r == block) { r = 0; ++f; }
      y.w = gate_one(x[u].w, sm, f, r, inv_block);
      *reinterpret_cast<float4*>(o + i) = y;
    } else {
      for (int e = 0; e < 4 && i + e < i1; ++e) {
        o[i + e] = gate_one(s[i + e], sm, f, r, inv_block);
        if (++r == block) { r = 0; ++f; }
      }
    }
  }
}

// ---- salience decode -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_salience(const float* hidden, long rows, const long long* center, float thred,
                                                       float* f0) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * (kThreads / 64) + (long)(threadIdx.x >> 6);
  if (row >= rows) return;                             // wave-uniform
  const float* h = hidden + row * kBins;
  float bv = 0.f;
  int bi = -1;
  for (int i = lane; i < kBins; i += 64) {             // ascending: a strict > keeps the first of equal values
    const float v = h[i];
    if (bi < 0 || v > bv) { bv = v; bi = i; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  long c = center ? (long)center[row] : (long)bi;
  c = lesser(greater(c, -16L), (long)kBins + 16);             // any window past the range is empty either way
  const long i = c - 4 + lane;                         // [c - 4, c + 5) clipped to the range
  const bool in = lane < 9 && i >= 0 && i < kBins;
  const double w = in ? (double)h[in ? i : 0] : 0.0;
  const double ps = wave_sum(w * (20.0 * (double)i + kCentsBase));
  const double ws = wave_sum(w);
  if (lane == 0) {
    const double cents = ps / (ws + (ws == 0.0 ? 1.0 : 0.0));
    f0[row] = bv < thred ? 0.f : (float)(10.0 * exp2(cents / 1200.0));
  }
}

// ---- F0 track --------------------------------------------------------------------------------------------------------------
struct Track {
  const float* src; long ld; int N;                    // [B, N] on a grid of `period` seconds
  double period, hop, sr, step;                        // step = hop / sr
  int n_frames, start;
  int nearest, uv_interp;
  double f0_min;
  float* out;                                          // [B, n_frames]
  int* prev; float* filled; double* tgt;               // workspace rows: max(N, n_frames) ints, N floats, n_frames doubles
  long prev_ld, filled_ld, tgt_ld;
};

// prev[i] = the largest voiced index <= i (-1: none), a forward max-scan: wave scans with an LDS carry, chunk after chunk
template <class T>
__device__ inline void scan_prev(const T* f, int n, int* prev, int* sw) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = -1;
  for (int c0 = 0; c0 < n; c0 += kTrackThreads) {
    const int i = c0 + (int)threadIdx.x;
    int v = (i < n && f[i] != (T)0) ? i : -1;
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o);
      if (lane >= o) v = greater(v, t);
    }
    if (lane == 63) sw[wave] = v;
    __syncthreads();
    int pre = carry, tot = carry;
    for (int w = 0; w < kTrackWaves; ++w) {
      if (w < wave) pre = greater(pre, sw[w]);
      tot = greater(tot, sw[w]);
    }
    if (i < n) prev[i] = greater(v, pre);
    carry = tot;
    __syncthreads();                                   // sw is rewritten by the next chunk
  }
}

// the fill of np.interp(where(uv), where(~uv), f[~uv]) at every index, given prev: next[i] (the smallest voiced index >= i, n: none)
// is a backward min-scan made here, chunk after chunk from the end.  put(i, value, voiced_anywhere)
template <class T, class Put>
__device__ inline void fill_row(const T* f, int n, const int* prev, int* sw, Put put) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = n;
  for (int c0 = (n - 1) / kTrackThreads * kTrackThreads; c0 >= 0; c0 -= kTrackThreads) {
    const int i = c0 + (int)threadIdx.x;
    int v = (i < n && f[i] != (T)0) ? i : n;
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_down(v, o);
      if (lane + o < 64) v = lesser(v, t);
    }
    if (lane == 0) sw[wave] = v;
    __syncthreads();
    int post = carry, tot = carry;
    for (int w = 0; w < kTrackWaves; ++w) {
      if (w > wave) post = lesser(post, sw[w]);
      tot = lesser(tot, sw[w]);
    }
    const int q = lesser(v, post);
    if (i < n) {
      const int p = prev[i];
      double r;
      if (p == i || (p < 0 && q >= n)) r = (double)f[i];             // voiced, or no voiced frame in the row: unchanged
      else if (p < 0) r = (double)f[q];
      else if (q >= n) r = (double)f[p];
      else {
        const double slope = ((double)f[q] - (double)f[p]) / ((double)q - (double)p);
        r = slope * ((double)i - (double)p) + (double)f[p];
      }
      put(i, r);
    }
    carry = tot;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kTrackThreads) void k_f0_track(Track g) {
  __shared__ int sw[kTrackWaves];
  const int b = blockIdx.x;
  const float* src = g.src + (long)b * g.ld;
  int* prev = g.prev + (long)b * g.prev_ld;
  float* filled = g.filled + (long)b * g.filled_ld;
  double* tgt = g.tgt + (long)b * g.tgt_ld;
  float* out = g.out + (long)b * g.n_frames;
  const int N = g.N;
  if (!g.nearest) {                                    // vocoder.py:110-112; the reference stores the fill into its float32 array
    scan_prev(src, N, prev, sw);
    fill_row(src, N, prev, sw, [=](int i, double r) { filled[i] = (float)r; });
    __syncthreads();
  }
  for (int k = threadIdx.x; k < g.n_frames; k += kTrackThreads) {
    double r = 0.0;
    if (k >= g.start) {
      const double kk = (double)(k - g.start);
      if (g.nearest) {                                 // vocoder.py:104: round half to even, then the last index held
        const double e = rint(((kk * g.hop) / g.sr) / g.period);
        r = (double)src[e >= (double)(N - 1) ? N - 1 : (int)e];
      } else {                                         // vocoder.py:113-117: np.interp of the filled track and of the unvoiced flag
        const double x = g.step * kk;
        const double e = x / g.period;
        int j = e >= (double)(N - 1) ? N - 1 : (int)e;
        while (j > 0 && g.period * (double)j > x) --j;
        while (j + 1 < N && g.period * (double)(j + 1) <= x) ++j;
        const double xj = g.period * (double)j;
        double u;
        if (j >= N - 1 || xj == x) {
          r = (double)filled[j];
          u = src[j] == 0.f ? 1.0 : 0.0;
        } else {
          const double dx = g.period * (double)(j + 1) - xj, xm = x - xj;
          const double fj = (double)filled[j], uj = src[j] == 0.f ? 1.0 : 0.0, uj1 = src[j + 1] == 0.f ? 1.0 : 0.0;
          r = ((double)filled[j + 1] - fj) / dx * xm + fj;
          u = (uj1 - uj) / dx * xm + uj;
        }
        if (u > 0.5) r = 0.0;
      }
    }
    if (g.uv_interp) tgt[k] = r;
    else out[k] = (float)r;
  }
  if (!g.uv_interp) return;
  __syncthreads();                                     // vocoder.py:139-143 on the target grid, in float64 as there
  scan_prev(tgt, g.n_frames, prev, sw);
  const double f0_min = g.f0_min;
  fill_row(tgt, g.n_frames, prev, sw, [=](int i, double r) { out[i] = (float)(r < f0_min ? f0_min : r); });
}

// ---- pools -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_pool1d(const float* x, long N, int k, int median, float* y) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const float* row = x + (long)blockIdx.y * N;
  const long s0 = i - (k - 1) / 2;
  float v[kMaxPool];
#pragma unroll
  for (int j = 0; j < kMaxPool; ++j) v[j] = j < k ? row[reflect(s0 + j, N)] : 0.f;
  float res;
  if (!median) {
    double sum = 0.0;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < kMaxPool; ++j)
      if (j < k && v[j] == v[j]) { sum += (double)v[j]; ++cnt; }
    res = (float)(sum / (double)greater(cnt, 1));
  } else {                                             // rank selection: element (k - 1) / 2 of the sorted window, NaN last as torch.sort
    const int want = (k - 1) / 2;
    res = v[0];
#pragma unroll
    for (int a = 0; a < kMaxPool; ++a) {
      if (a >= k) continue;
      int below = 0;
#pragma unroll
      for (int c = 0; c < kMaxPool; ++c) {
        if (c >= k) continue;
        const bool an = v[a] != v[a], cn = v[c] != v[c];
        const bool lt = cn ? false : (an ? true : v[c] < v[a]);       // v[c] sorts before v[a]
        const bool eq = (an && cn) || v[c] == v[a];
        below += (lt || (eq && c < a)) ? 1 : 0;
      }
      if (below == want) res = v[a];
    }
  }
  y[(long)blockIdx.y * N + i] = res;
}

}  // namespace features

static inline size_t features_align(size_t v) { return (v + 15) / 16 * 16; }

size_t f0_track_ws_bytes(int B, long N, long n_frames) {
  const size_t ints = features_align(sizeof(int) * (size_t)(N > n_frames ? N : n_frames));
  return (size_t)B * (ints + features_align(sizeof(float) * (size_t)N) + features_align(sizeof(double) * (size_t)n_frames));
}

void launch_volume(const float* audio, long ld, int B, long T, int hop, float* vol, hipStream_t st) {
  using namespace features;
  const long F = T / hop + 1;
  hipLaunchKernelGGL(k_volume, dim3((unsigned)((F + kThreads / 64 - 1) / (kThreads / 64)), (unsigned)B), dim3(kThreads), 0, st,
                     audio, ld, T, hop, F, vol);
}

void launch_gate(const float* sig, long ld_s, const float* vol, int B, long F, int block, float thr, int dilate, float* out,
                 long ld_o, hipStream_t st) {
  using namespace features;
  const long n = F * block;
  const int vec = ((reinterpret_cast<uintptr_t>(sig) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 &&
                  (B == 1 || ((ld_s | ld_o) & 3) == 0);
  hipLaunchKernelGGL(k_gate, dim3((unsigned)((n + kGateSpan - 1) / kGateSpan), (unsigned)B), dim3(kThreads), 0, st, sig, ld_s, out,
                     ld_o, vol, F, block, dilate, thr, 1.0 / (double)block, vec);
}

void launch_salience(const float* hidden, long rows, const long long* center, float thred, float* f0, hipStream_t st) {
  using namespace features;
  hipLaunchKernelGGL(k_salience, dim3((unsigned)((rows + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, hidden, rows,
                     center, thred, f0);
}

void launch_f0_track(const float* src, long ld, int B, long N, double period, double hop, double sr, long n_frames, long start,
                     int nearest, int uv_interp, double f0_min, float* out, void* ws, hipStream_t st) {
  using namespace features;
  Track g;
  g.src = src; g.ld = ld; g.N = (int)N;
  g.period = period; g.hop = hop; g.sr = sr; g.step = hop / sr;
  g.n_frames = (int)n_frames; g.start = (int)start;
  g.nearest = nearest; g.uv_interp = uv_interp; g.f0_min = f0_min;
  g.out = out;
  const size_t ints = features_align(sizeof(int) * (size_t)(N > n_frames ? N : n_frames));
  const size_t floats = features_align(sizeof(float) * (size_t)N), doubles = features_align(sizeof(double) * (size_t)n_frames);
  char* p = static_cast<char*>(ws);
  g.prev = reinterpret_cast<int*>(p); g.prev_ld = (long)(ints / sizeof(int));
  p += (size_t)B * ints;
  g.filled = reinterpret_cast<float*>(p); g.filled_ld = (long)(floats / sizeof(float));
  p += (size_t)B * floats;
  g.tgt = reinterpret_cast<double*>(p); g.tgt_ld = (long)(doubles / sizeof(double));
  hipLaunchKernelGGL(k_f0_track, dim3((unsigned)B), dim3(kTrackThreads), 0, st, g);
}

void launch_pool1d(const float* x, int B, long N, int k, int median, float* y, hipStream_t st) {
  using namespace features;
  hipLaunchKernelGGL(k_pool1d, dim3((unsigned)((N + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0, st, x, N, k, median, y);
}

}  // namespace ddsp
