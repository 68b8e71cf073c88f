// The real-time caller's splice of consecutive blocks (gui.py:431-456): the SOLA offset search, the crossfade with the previous
// call's tail, and the phase-vocoder crossfade (gui.py:15-32).  Included from api.hip only (one translation unit holds the kernels).
//
//   k_splice_search        nom[s] / sqrt(energy[s] + 1e-8) for every candidate offset s = 0 .. S, in float64   grid (ceil((S+1)/64), B)
//   k_splice_spectra       (vocoder) argmax -> shift, the two windowed forward DFTs -> per-bin amplitude and phases, and the
//                          copy of tmp past the crossfade                                                        grid (ceil(K/64), B)
//   k_splice_finish<PV>    (plain) argmax -> shift; every output sample: crossfade or vocoder synthesis, then out / new buffer
//                                                  grid (ceil((Bf+C)/256), B); with the vocoder the crossfade only, (ceil(C/64), B)
// Plain splice = search + finish (2 launches); with the vocoder search + spectra + finish (3).  The shift never leaves the device:
// each workgroup that needs it takes the argmax of the S + 1 ratios itself (first index on ties, as torch.argmax), which costs
// less than a launch.  buf_in is only read and buf_out only written, so no workgroup can overwrite the tail another still reads.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

namespace ddsp {
namespace splice {

constexpr int kThreads = 256;
constexpr int kCandPerWave = 16;                       // search: candidate offsets one wave accumulates at once
constexpr int kCandPerBlock = 4 * kCandPerWave;
constexpr int kRatioStride = 4104;                     // doubles per utterance in the workspace: >= 4097 = S_max + 1, 64-byte rows
constexpr int kDftChunk = 1024;                        // spectra: windowed samples per LDS stage
constexpr int kPvSplit = 16;                           // vocoder kernels: waves per workgroup, each a share of the inner sum
constexpr int kPvThreads = 64 * kPvSplit;
constexpr int kPvItems = 64;                           // vocoder kernels: bins / output samples per workgroup (one per lane)

// one frequency bin of the vocoder, as the synthesis consumes it: cos(pi (2 (k n mod C) / C + n rk + pk))
struct Bin { double amp, rk, pk, pad; };               // amp = |A| + |B| (inner bins doubled), rk = dphi / (pi C), pk = phi_a / pi

struct Geometry {
  const float* audio; long ld; long off;               // seg of utterance b: audio + b ld + off, Bf + C + S samples
  const float* buf_in;                                 // [B, C] the previous tail (read only)
  const float* fade_in; const float* fade_out;         // [C]
  int C, S, Bf;
  double* ratio;                                       // [B, kRatioStride]; null: no search, shift 0 (the standalone vocoder)
  long long* shift;                                    // [B]; written by the workgroup x = 0 that takes the argmax
  Bin* bins;                                           // [B, C / 2 + 1]
  float* out;                                          // [B, Bf]
  float* buf_out;                                      // [B, C] the new tail
};

// first index of the largest of r[0 .. n) (n >= 1), the whole workgroup of NT threads; sv / si: NT entries of LDS
template <int NT>
__device__ inline int block_argmax(const double* r, int n, double* sv, int* si) {
  double bv = 0.0;
  int bi = -1;
  for (int s = threadIdx.x; s < n; s += NT) {          // ascending: a strict > keeps the first of equal values
    const double v = r[s];
    if (bi < 0 || v > bv) { bv = v; bi = s; }
  }
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      const double ov = sv[threadIdx.x + h];
      const int oi = si[threadIdx.x + h];
      const double v = sv[threadIdx.x];
      const int i = si[threadIdx.x];
      if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  const int r0 = si[0];
  __syncthreads();                                     // sv / si may be reused behind the call
  return r0 < 0 ? 0 : r0;
}

__global__ __launch_bounds__(kThreads) void k_splice_search(Geometry g) {
  const int b = blockIdx.y;
  const float* seg = g.audio + (long)b * g.ld + g.off;
  const float* buf = g.buf_in + (long)b * g.C;
  const int lane = threadIdx.x & 63;
  const int s0 = blockIdx.x * kCandPerBlock + (int)(threadIdx.x >> 6) * kCandPerWave;
  if (s0 > g.S) return;                                // wave-uniform; no barrier follows
  double nom[kCandPerWave], en[kCandPerWave];
  int si[kCandPerWave];
#pragma unroll
  for (int i = 0; i < kCandPerWave; ++i) { nom[i] = 0.0; en[i] = 0.0; si[i] = min(s0 + i, g.S); }   // past S: a valid repeat, not stored
  // float products are exact in float64: the sums are float64 sums of the exact terms
  for (int j = lane; j < g.C; j += 64) {
    const double w = (double)buf[j];
#pragma unroll
    for (int i = 0; i < kCandPerWave; ++i) {
      const double x = (double)seg[si[i] + j];
      nom[i] = fma(x, w, nom[i]);
      en[i] = fma(x, x, en[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < kCandPerWave; ++i) {
    for (int o = 32; o > 0; o >>= 1) {
      nom[i] += __shfl_xor(nom[i], o);
      en[i] += __shfl_xor(en[i], o);
    }
  }
  if (lane == 0) {
    double* r = g.ratio + (long)b * kRatioStride;
#pragma unroll
    for (int i = 0; i < kCandPerWave; ++i)
      if (s0 + i <= g.S) r[s0 + i] = nom[i] / sqrt(en[i] + 1e-8);
  }
}

// the vocoder's analysis: A = rfft(a w), B = rfft(x w) with w = sqrt(fade_out fade_in), direct sums in float64.  A workgroup takes
// kPvItems bins (one per lane) and its kPvSplit waves split the samples j (wave v: j = v mod kPvSplit), summed in LDS in wave order.
// The twiddle of (k, j) is exp(-i pi 2 m / C) from float32 sincospif, m = k j mod C kept exactly in integers and folded to
// |2 m / C| <= 1 before the one rounding to float32 (<= 2^-25 half-turns, ~1e-7 rad, plus sincospif's own ulp) at every C.
__global__ __launch_bounds__(kPvThreads) void k_splice_spectra(Geometry g) {
  __shared__ double sv[kPvThreads];
  __shared__ int sidx[kPvThreads];
  __shared__ float2 sab[kDftChunk];
  __shared__ double part[kPvSplit - 1][4][kPvItems];
  const int b = blockIdx.y;
  const int C = g.C, K = C / 2 + 1;
  int shift = 0;
  if (g.ratio) {
    shift = block_argmax<kPvThreads>(g.ratio + (long)b * kRatioStride, g.S + 1, sv, sidx);
    if (blockIdx.x == 0 && threadIdx.x == 0) g.shift[b] = shift;
  }
  const float* a = g.buf_in + (long)b * C;
  const float* x = g.audio + (long)b * g.ld + g.off + shift;
  // tmp[C : C + Bf] does not depend on the vocoder: this launch's workgroups copy it (grid-stride), so the synthesis grid
  // covers the crossfade alone
  for (int i = C + blockIdx.x * kPvThreads + threadIdx.x; i < g.Bf + C; i += gridDim.x * kPvThreads) {
    const float v = x[i];
    if (i < g.Bf) g.out[(long)b * g.Bf + i] = v;
    else g.buf_out[(long)b * C + (i - g.Bf)] = v;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = blockIdx.x * kPvItems + lane;
  const int kstep = (int)(((long long)k * kPvSplit) % C);
  const double two_over_c = 2.0 / C;
  double ra = 0.0, ia = 0.0, rb = 0.0, ib = 0.0;
  for (int j0 = 0; j0 < C; j0 += kDftChunk) {
    const int jn = min(kDftChunk, C - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < jn; j += kPvThreads) {
      const double w = sqrt((double)g.fade_out[j0 + j] * (double)g.fade_in[j0 + j]);
      sab[j] = make_float2((float)((double)a[j0 + j] * w), (float)((double)x[j0 + j] * w));
    }
    __syncthreads();
    if (k < K) {
      int m = (int)(((long long)k * (j0 + wave)) % C);
      for (int j = wave; j < jn; j += kPvSplit) {
        const int mr = 2 * m > C ? m - C : m;
        float sn, cs;
        sincospif((float)(mr * two_over_c), &sn, &cs);
        const float2 v = sab[j];
        ra = fma((double)v.x, (double)cs, ra);
        ia = fma(-(double)v.x, (double)sn, ia);
        rb = fma((double)v.y, (double)cs, rb);
        ib = fma(-(double)v.y, (double)sn, ib);
        m += kstep;
        if (m >= C) m -= C;
      }
    }
  }
  if (wave > 0) {
    part[wave - 1][0][lane] = ra; part[wave - 1][1][lane] = ia;
    part[wave - 1][2][lane] = rb; part[wave - 1][3][lane] = ib;
  }
  __syncthreads();
  if (wave == 0 && k < K) {
    for (int v = 0; v < kPvSplit - 1; ++v) {
      ra += part[v][0][lane]; ia += part[v][1][lane];
      rb += part[v][2][lane]; ib += part[v][3][lane];
    }
    ia += 0.0;                                         // -0 -> +0: the angle of an exactly real bin, as torch.angle gives it
    ib += 0.0;
    double amp = sqrt(ra * ra + ia * ia) + sqrt(rb * rb + ib * ib);
    if (k >= 1 && 2 * k != C) amp *= 2.0;              // absab[1:-1] (C even) / absab[1:] (C odd)
    const double pa = atan2(ia, ra);
    double d = atan2(ib, rb) - pa;
    d -= 2.0 * M_PI * floor(d / 2.0 / M_PI + 0.5);
    Bin q;
    q.amp = amp;
    q.rk = d / (M_PI * C);
    q.pk = pa / M_PI;
    q.pad = 0.0;
    g.bins[(long)b * K + k] = q;
  }
}

// The crossfaded head of tmp = seg[shift : shift + Bf + C] and, for the plain splice, the rest: sample i goes to out[b, i] (i < Bf)
// or buf_out[b, i - Bf].
// PV (i < C only; k_splice_spectra copies the rest): a fo^2 + x fi^2 + w / C sum_k amp_k cos(pi (2 (k i mod C) / C + i rk + pk)),
// float64 sums of float32 cospif of the argument reduced to [-1, 1] half-turns in float64; kPvItems samples per workgroup (one
// per lane), its kPvSplit waves split the bins.
// Plain: (x * fi) + (a * fo), two float32 roundings in the torch chain's order; kThreads samples per workgroup.
template <bool PV>
__global__ __launch_bounds__(PV ? kPvThreads : kThreads) void k_splice_finish(Geometry g) {
  const int b = blockIdx.y;
  const int C = g.C;
  int shift;
  if (PV) {
    shift = g.shift ? (int)g.shift[b] : 0;
  } else {
    __shared__ double sv[kThreads];
    __shared__ int sidx[kThreads];
    shift = block_argmax<kThreads>(g.ratio + (long)b * kRatioStride, g.S + 1, sv, sidx);
    if (blockIdx.x == 0 && threadIdx.x == 0) g.shift[b] = shift;
  }
  const int n_all = g.Bf + C;
  const float* x = g.audio + (long)b * g.ld + g.off + shift;
  const float* a = g.buf_in + (long)b * C;
  int i;
  float v;
  if (PV) {                                            // the grid covers [0, C): every workgroup has samples to synthesise
    __shared__ Bin sb[kPvThreads];
    __shared__ double part[kPvSplit - 1][kPvItems];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i = blockIdx.x * kPvItems + lane;
    const int K = C / 2 + 1;
    const Bin* bins = g.bins + (long)b * K;
    const double two_over_c = 2.0 / C;
    const double di = (double)i;
    const int istep = (int)(((long long)i * kPvSplit) % C);
    double acc = 0.0;
    for (int k0 = 0; k0 < K; k0 += kPvThreads) {
      const int kn = min(kPvThreads, K - k0);
      __syncthreads();
      if ((int)threadIdx.x < kn) sb[threadIdx.x] = bins[k0 + threadIdx.x];
      __syncthreads();
      if (i < C) {
        int m = (int)(((long long)(k0 + wave) * i) % C);
        for (int kk = wave; kk < kn; kk += kPvSplit) {
          const Bin q = sb[kk];
          const int mr = 2 * m > C ? m - C : m;
          double t = fma(di, q.rk, fma((double)mr, two_over_c, q.pk));
          t -= 2.0 * rint(0.5 * t);
          acc = fma(q.amp, (double)cospif((float)t), acc);
          m += istep;
          if (m >= C) m -= C;
        }
      }
    }
    if (wave > 0) part[wave - 1][lane] = acc;
    __syncthreads();
    if (wave > 0 || i >= C) return;                    // no barrier below
    for (int w = 0; w < kPvSplit - 1; ++w) acc += part[w][lane];
    const double fo = g.fade_out[i], fi = g.fade_in[i];
    v = (float)((double)a[i] * (fo * fo) + (double)x[i] * (fi * fi) + acc * sqrt(fo * fi) / C);
  } else {
    i = blockIdx.x * kThreads + threadIdx.x;
    v = i < n_all ? x[i] : 0.f;
    if (i < C) v = __fadd_rn(__fmul_rn(v, g.fade_in[i]), __fmul_rn(a[i], g.fade_out[i]));
  }
  if (i < g.Bf) g.out[(long)b * g.Bf + i] = v;
  else if (i < n_all) g.buf_out[(long)b * C + (i - g.Bf)] = v;
}

}  // namespace splice

size_t splice_ws_bytes(int B, int C, int use_pv) {
  const size_t ratio = (size_t)B * splice::kRatioStride * sizeof(double);
  return ratio + (use_pv ? (size_t)B * (C / 2 + 1) * sizeof(splice::Bin) : 0);
}

static void launch_splice(const splice::Geometry& g, int B, int use_pv, hipStream_t st) {
  using namespace splice;
  if (g.ratio)
    hipLaunchKernelGGL(k_splice_search, dim3((unsigned)(g.S / kCandPerBlock + 1), (unsigned)B), dim3(kThreads), 0, st, g);
  if (use_pv) {
    hipLaunchKernelGGL(k_splice_spectra, dim3((unsigned)((g.C / 2 + kPvItems) / kPvItems), (unsigned)B), dim3(kPvThreads), 0, st, g);
    hipLaunchKernelGGL((k_splice_finish<true>), dim3((unsigned)((g.C + kPvItems - 1) / kPvItems), (unsigned)B), dim3(kPvThreads),
                       0, st, g);
  } else {
    hipLaunchKernelGGL((k_splice_finish<false>), dim3((unsigned)((g.Bf + g.C + kThreads - 1) / kThreads), (unsigned)B),
                       dim3(kThreads), 0, st, g);
  }
}

void launch_sola_splice(const float* audio, long ld, int B, long off, int Bf, int C, int S, const float* buf_in, float* buf_out,
                        const float* fade_in, const float* fade_out, int use_pv, float* out, long long* shift, void* ws,
                        hipStream_t st) {
  splice::Geometry g;
  g.audio = audio; g.ld = ld; g.off = off;
  g.buf_in = buf_in; g.fade_in = fade_in; g.fade_out = fade_out;
  g.C = C; g.S = S; g.Bf = Bf;
  g.ratio = static_cast<double*>(ws);
  g.shift = shift;
  g.bins = reinterpret_cast<splice::Bin*>(static_cast<char*>(ws) + (size_t)B * splice::kRatioStride * sizeof(double));
  g.out = out; g.buf_out = buf_out;
  launch_splice(g, B, use_pv, st);
}

// gui.py:15-32 on its own: the spectra and synthesis kernels with no search (shift 0) and Bf = 0, so that all n samples land in
// the "new tail" and that is out.  ws: splice_ws_bytes(1, n, 1) bytes
void launch_phase_vocoder(const float* a, const float* b, const float* fade_out, const float* fade_in, int n, float* out, void* ws,
                          hipStream_t st) {
  splice::Geometry g;
  g.audio = b; g.ld = n; g.off = 0;
  g.buf_in = a; g.fade_in = fade_in; g.fade_out = fade_out;
  g.C = n; g.S = 0; g.Bf = 0;
  g.ratio = nullptr;
  g.shift = nullptr;
  g.bins = reinterpret_cast<splice::Bin*>(static_cast<char*>(ws) + splice::kRatioStride * sizeof(double));
  g.out = nullptr; g.buf_out = out;
  launch_splice(g, 1, 1, st);
}

}  // namespace ddsp
