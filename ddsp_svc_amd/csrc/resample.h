// Band-limited resampling, torchaudio's sinc_interp_hann / sinc_interp_kaiser (F.pad + a strided conv1d with an [n, 1, K]
// filter bank), as an f32 MFMA GEMM per utterance.  Included from api.hip only (one translation unit holds the kernels).
//
// With o = orig / gcd, n = new / gcd, K = 2w + o and xpad[p] = x[p - w] (0 outside [0, L)):
//     y[q n + j] = sum_k xpad[q o + k] h[j, k],   q = 0 .. M - 1, j = 0 .. n - 1, and only t = q n + j < T = ceil(n L / o) kept.
// That is Y = X H^T with X[q, k] = xpad[q o + k] (rows overlap when K > o) and the bank as B operand.
//
// Virtual phases.  For n < 32 the bank is expanded into G = 32 / n copies, h'[g n + j, k'] = h[j, k' - g o] with o' = G o,
// n' = G n: output row q' of the expanded bank holds rows q' G .. q' G + G - 1 of the plain one, every output takes the same
// products of the same taps, and N becomes 17 .. 32 instead of 1 .. 31.  t = q' n' + j' holds for both.
//
// Table (built on the host from the float32 bank, resample_table_*, then copied to the device once):
//   Hdr, then a TileHdr per tile of kTN virtual phases, then the taps of each tile as [kt][kTN] floats (16-byte aligned).
//   A tile's K range [klo, klo + kt) is the union of its phases' live bands (the taps that are not exactly 0.0f), kt rounded
//   up to kKC with zero taps (the kernel reads no sample against those: TileHdr::kl is the length before rounding).
//   For finite input the trimming changes only the summation order: the taps outside the range are exactly zero.  For a
//   sample that is inf or NaN it changes which outputs are non-finite, in both directions.  A zero tap that was dropped
//   no longer turns the output into NaN (0 * inf), while a tile's band is the union over its 32 virtual phases, so a zero
//   tap inside it that torchaudio's conv1d never multiplies (the shifted copies of the virtual phases add such taps,
//   h'[g n + j, k'] outside k' - g o in [0, K)) now does.  What holds: an output with a non-zero tap on the sample is
//   non-finite; no output outside the virtual rows q' whose window [q' G o, q' G o + (G - 1) o + K) of the padded input
//   covers the sample is; and every finite output has the bits it has with that sample set to zero.
//
// k_resample: grid (ceil(M' / kTM), tiles, B), 4 waves.  One workgroup: kTM output rows x one tile of kTN phases.  Stage s
// holds kKG = 4 kKC taps: the A rows (kTM x kKG, read with bounds checks in place of the zero padding) and the tile's taps
// (kKG x kTN) in LDS; wave v takes taps [v kKC, (v + 1) kKC) of the stage on v_mfma_f32_32x32x2_f32, so each wave keeps its
// own accumulator chain over a quarter of the band, summed in wave order at the end.  The next stage's global loads are in
// registers while the current one's MFMAs run.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "tuning.h"

namespace ddsp {
namespace resample {

typedef float f32x16r __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kTM = 32;                                // output rows (blocks of n' samples) per workgroup
constexpr int kTN = 32;                                // virtual phases per tile
constexpr int kKC = 32;                                // taps per wave per stage
constexpr int kKG = 4 * kKC;                           // taps per stage
constexpr int kAStride = kKG + 2;                      // A rows in LDS: lane halves land on even / odd banks
constexpr int kALoads = kTM * kKG / kThreads;          // 16 A floats per thread per stage
constexpr int kBLoads = kKG * kTN / 4 / kThreads;      // 4 float4 of taps per thread per stage
constexpr int kMaxRate = 4096;                         // reduced orig / new
constexpr int kMaxBand = 65536;                        // taps per tile
constexpr int kMagic = 0x52534d50;
constexpr size_t kTapAlign = 256;

struct Hdr { int magic, o, n, K, G, tiles, pad0, pad1; };   // the kernel checks magic, o, n, K and tiles against its call
struct TileHdr { int klo, kt, off, kl; };              // off: floats from the start of the tap section; kl: the band before rounding

inline int virt_group(int n) { return n < kTN ? kTN / n : 1; }
inline int tiles_of(int n) { return (n * virt_group(n) + kTN - 1) / kTN; }
inline size_t tap_section(int tiles) {
  const size_t h = sizeof(Hdr) + (size_t)tiles * sizeof(TileHdr);
  return (h + kTapAlign - 1) / kTapAlign * kTapAlign;
}

struct Args {
  const float* x; long ldx, sx, L;                     // x[b ldx + p sx], p < L
  float* y; long ldy, T, M;                            // y[b ldy + t], t < T; M = ceil(T / n') rows
  const Hdr* hdr; const TileHdr* tiles; const float* taps;
  int o, n, K;                                         // the rates and bank length the table must have been built for
  int op, np, w;                                       // o' = G o, n' = G n, pad width
  long b0;                                             // first utterance of this launch
};

__global__ __launch_bounds__(kThreads) void k_resample(Args a) {
  __shared__ float sA[kTM * kAStride];
  __shared__ float4 sB[kKG * kTN / 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long q0 = (long)blockIdx.x * kTM;
  const int tile = blockIdx.y;
  const long b = a.b0 + blockIdx.z;
  const Hdr hd = *a.hdr;
  if (hd.magic != kMagic || hd.o != a.o || hd.n != a.n || hd.K != a.K || hd.tiles != (int)gridDim.y) {
    // a table built for other rates: its tile and tap offsets mean nothing here.  Read none of them, write NaN to this
    // workgroup's outputs so that the mistake shows (uniform over the workgroup, before any barrier)
    for (int e = tid; e < kTM * kTN; e += kThreads) {
      const long q = q0 + e / kTN;
      const int j = tile * kTN + e % kTN;
      const long t = q * a.np + j;
      if (j < a.np && q < a.M && t < a.T) a.y[b * a.ldy + t] = __builtin_nanf("");
    }
    return;
  }
  const TileHdr th = a.tiles[tile];
  const float* xb = a.x + b * a.ldx;
  const float4* tb = reinterpret_cast<const float4*>(a.taps + th.off);
  const long p0 = q0 * a.op + th.klo - a.w;            // x position of row 0, first tap of the tile's band
  float ra[kALoads];
  float4 rb[kBLoads];
  f32x16r acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const int stages = (th.kt + kKG - 1) / kKG;
  for (int s = 0; s <= stages; ++s) {
    if (s > 0) {                                       // stage s - 1: registers -> LDS
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kALoads; ++r) {
        const int e = tid + r * kThreads;
        sA[(e / kKG) * kAStride + (e % kKG)] = ra[r];
      }
#pragma unroll
      for (int r = 0; r < kBLoads; ++r) sB[tid + r * kThreads] = rb[r];
      __syncthreads();
    }
    if (s < stages) {                                  // stage s: global -> registers, in flight under stage s - 1's MFMAs
      const int k0 = s * kKG;
#pragma unroll
      for (int r = 0; r < kALoads; ++r) {
        const int e = tid + r * kThreads;
        const int i = e / kKG, k = e % kKG;
        const long p = p0 + (long)i * a.op + k0 + k;
        ra[r] = (k0 + k < th.kl && p >= 0 && p < a.L) ? xb[p * a.sx] : 0.f;   // kl, not kt: no sample meets a rounding tap
      }
#pragma unroll
      for (int r = 0; r < kBLoads; ++r) {
        const int e = tid + r * kThreads;
        const int k = k0 + e / (kTN / 4);
        rb[r] = k < th.kt ? tb[(long)k * (kTN / 4) + e % (kTN / 4)] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    if (s > 0 && (s - 1) * kKG + wave * kKC < th.kt) {  // wave-uniform; no barrier inside
      // 32x32x2: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
      const float* pa = sA + (lane & 31) * kAStride + wave * kKC + (lane >> 5);
      const float* pb = reinterpret_cast<const float*>(sB) + (wave * kKC + (lane >> 5)) * kTN + (lane & 31);
#pragma unroll
      for (int k = 0; k < kKC; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k], pb[k * kTN], acc, 0, 0, 0);
    }
  }

  // the four chains, summed in wave order by wave 0; D: col = l & 31, row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)
  float* red = sA;                                     // 3 x 16 x 64 floats <= kTM x kAStride
  __syncthreads();
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wave - 1) * 16 + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (wave > 0) return;                                // no barrier below
  const int j = tile * kTN + (lane & 31);
  if (j >= a.np) return;
  float* yb = a.y + b * a.ldy;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = acc[r] + red[r * 64 + lane];
    v += red[(16 + r) * 64 + lane];
    v += red[(32 + r) * 64 + lane];
    const long q = q0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const long t = q * a.np + j;
    if (q < a.M && t < a.T) yb[t] = v;
  }
}

}  // namespace resample

// ---- host side: the table ----------------------------------------------------------------------------------------------------

// live band [lo, hi) of bank row j (K taps): the first and one past the last tap that is not exactly 0.0f; lo = hi = 0 if none
static inline void resample_band(const float* bank, int K, int j, int* lo, int* hi) {
  const float* h = bank + (size_t)j * K;
  int a = 0, e = K;
  while (a < K && h[a] == 0.f) ++a;
  while (e > a && h[e - 1] == 0.f) --e;
  *lo = a == K ? 0 : a;
  *hi = a == K ? 0 : e;
}

// per tile: klo and kt (rounded up to kKC); returns the tap floats of all tiles, or -1 past kMaxBand
static inline long resample_layout(const float* bank, int o, int n, int K, resample::TileHdr* th) {
  using namespace resample;
  const int G = virt_group(n), np = G * n, tiles = tiles_of(n);
  long total = 0;
  for (int t = 0; t < tiles; ++t) {
    int lo = 0, hi = 0;
    bool any = false;
    for (int jv = t * kTN; jv < t * kTN + kTN && jv < np; ++jv) {
      int a, e;
      resample_band(bank, K, jv % n, &a, &e);
      if (e <= a) continue;
      a += (jv / n) * o;
      e += (jv / n) * o;
      if (!any || a < lo) lo = a;
      if (!any || e > hi) hi = e;
      any = true;
    }
    const long kt = any ? ((long)(hi - lo) + kKC - 1) / kKC * kKC : 0;
    if (kt > kMaxBand) return -1;
    if (th) { th[t].klo = lo; th[t].kt = (int)kt; th[t].off = (int)total; th[t].kl = any ? hi - lo : 0; }
    total += kt * kTN;
  }
  return total;
}

bool resample_rates_ok(int o, int n, int K) {
  return o >= 1 && n >= 1 && o <= resample::kMaxRate && n <= resample::kMaxRate && K > o && ((K - o) & 1) == 0;
}

size_t resample_table_bytes(const float* bank, int o, int n, int K) {
  if (!bank || !resample_rates_ok(o, n, K)) return 0;
  const long taps = resample_layout(bank, o, n, K, nullptr);
  if (taps < 0) return 0;
  return resample::tap_section(resample::tiles_of(n)) + (size_t)taps * sizeof(float);
}

// fills a host buffer of resample_table_bytes(...) bytes; false if the rates or the band are out of range
bool resample_table(const float* bank, int o, int n, int K, void* out, size_t bytes) {
  using namespace resample;
  const size_t need = resample_table_bytes(bank, o, n, K);
  if (need == 0 || bytes < need) return false;
  const int G = virt_group(n), np = G * n, tiles = tiles_of(n);
  char* base = static_cast<char*>(out);
  memset(base, 0, need);
  Hdr* h = reinterpret_cast<Hdr*>(base);
  h->magic = kMagic; h->o = o; h->n = n; h->K = K; h->G = G; h->tiles = tiles;
  TileHdr* th = reinterpret_cast<TileHdr*>(base + sizeof(Hdr));
  resample_layout(bank, o, n, K, th);
  float* taps = reinterpret_cast<float*>(base + tap_section(tiles));
  for (int t = 0; t < tiles; ++t) {
    float* tt = taps + th[t].off;
    for (int c = 0; c < kTN; ++c) {
      const int jv = t * kTN + c;
      if (jv >= np) break;
      const float* row = bank + (size_t)(jv % n) * K;
      const int shift = (jv / n) * o;                  // h'[jv, k'] = h[jv mod n, k' - (jv / n) o]
      for (int k = 0; k < th[t].kt; ++k) {
        const int kk = th[t].klo + k - shift;
        if (kk >= 0 && kk < K) tt[(size_t)k * kTN + c] = row[kk];
      }
    }
  }
  return true;
}

// y[b ldy + t] for b < B, t < ceil(n L / o); table: resample_table's bytes on the device (16-byte aligned)
void launch_resample(const float* x, long ldx, long sx, int B, long L, float* y, long ldy, const void* table, int o, int n,
                     int w, hipStream_t st) {
  using namespace resample;
  const int G = virt_group(n), np = G * n, tiles = tiles_of(n);
  Args a;
  a.x = x; a.ldx = ldx; a.sx = sx; a.L = L;
  a.y = y; a.ldy = ldy;
  a.T = ((long)n * L + o - 1) / o;
  a.M = (a.T + np - 1) / np;
  a.hdr = static_cast<const Hdr*>(table);
  a.tiles = reinterpret_cast<const TileHdr*>(static_cast<const char*>(table) + sizeof(Hdr));
  a.o = o; a.n = n; a.K = 2 * w + o;
  a.taps = reinterpret_cast<const float*>(static_cast<const char*>(table) + tap_section(tiles));
  a.op = G * o; a.np = np; a.w = w;
  if (a.T == 0) return;
  const long mt = (a.M + kTM - 1) / kTM;
  const long split = batch_split();
  for (long b0 = 0; b0 < B; b0 += split) {
    a.b0 = b0;
    const long nb = B - b0 < split ? B - b0 : split;
    hipLaunchKernelGGL(k_resample, dim3((unsigned)mt, (unsigned)tiles, (unsigned)nb), dim3(kThreads), 0, st, a);
  }
}

}  // namespace ddsp
