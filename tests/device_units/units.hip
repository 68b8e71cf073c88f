// Unit-test kernels for the building blocks one layer below the product's kernels: the in-register / LDS FFT plans of fft_r.h and
// fft_1024p.h, the packed complex helpers of fft2048.h, and the wave scans, buffer descriptors and hardware-math wrappers of
// ddsp_common.h.  ONE source, built twice by tests/device_units/build.py: as host C++ against the CPU emulator (the plain C++ twins)
// and with hipcc for gfx950 under the product's flags (the bodies that ship).  tests/test_fft_plans.py and tests/test_device_units.py
// run both.  Every entry point takes raw pointers (host memory under the emulator, device memory on the GPU) and a stream, and
// returns 0.  TEST INFRASTRUCTURE ONLY.
#include "fft_1024p.h"

namespace {
using ddsp::f32x2;
using ddsp::fft::Plan;

// mode 0: Plan<R>::forward                 natural order in  -> natural order out
// mode 1: Plan<2>::forward_s<false>        natural in        -> out[s_index(tid, slot)]  (so out is in natural bin order)
// mode 2: Plan<2>::forward_s<true>         (upper half of the input must be zero)
// mode 3: Plan<2>::transposed              in[k] is read into layout S, out natural = DFT of in
// mode 4: Plan<2>::forward_s2<true>        two inputs (in, in2) -> (out, out2), both as mode 2
// mode 5: Plan<2>::transposed_and_forward_s   in -> out as mode 3, in2 -> out2 as mode 2
// modes 10..12 (every R): the lockstep pair forward2 (full / zero-padded inputs) and the zero-padded forward
// modes 13, 14: Plan<2>::transposed_then_forward_s (the three-buffer, staggered form of mode 5), plain and in layout S-
// modes 15, 16: the padded-row plan of fft_1024p.h (k_fir_blk6): forward_s<true, true> as mode 6, transposed_then_forward_s<true> as
//                mode 14; mode 17: its mirror_base against parked(-k) for every slot but the two self-mirrored ones (out = count of mismatches)
// modes 6..9: modes 2..5 in the sign-carrying layout S- (FLIP = true): what odd threads hold is written out negated
//             again, so the expected values are those of modes 2..5
// blockIdx.x selects one of a batch of inputs (N complex words apart in all four arrays)
template <int R>
__global__ void k_plan(int mode, const f32x2* in, const f32x2* in2, f32x2* out, f32x2* out2) {
  using PL = Plan<R>;
  constexpr int N = PL::N, P = PL::P;
  __shared__ __attribute__((aligned(16))) f32x2 ex[4][N];
  const int tid = threadIdx.x;
  in += (size_t)blockIdx.x * N; in2 += (size_t)blockIdx.x * N; out += (size_t)blockIdx.x * N; out2 += (size_t)blockIdx.x * N;
  typename PL::Tw tw;
  tw.init(tid);
  f32x2 v[8], u[8];
  if (mode == 0) {
    for (int m = 0; m < 8; ++m) v[m] = in[P * m + tid];
    PL::forward(v, tw, ex[0], ex[1], tid);
    for (int m = 0; m < 8; ++m) out[P * m + tid] = v[m];
  }
  if (mode == 10 || mode == 11) {                            // 10: forward2, 11: forward2<true> (upper halves of the inputs zero)
    for (int m = 0; m < 8; ++m) { v[m] = in[P * m + tid]; u[m] = in2[P * m + tid]; }
    if (mode == 10) PL::forward2(v, u, tw, ex[0], ex[1], ex[2], ex[3], tid);
    else PL::template forward2<true>(v, u, tw, ex[0], ex[1], ex[2], ex[3], tid);
    for (int m = 0; m < 8; ++m) { out[P * m + tid] = v[m]; out2[P * m + tid] = u[m]; }
  }
  if (mode == 12) {                                          // forward<true>: the pruned first pass alone
    for (int m = 0; m < 4; ++m) v[m] = in[P * m + tid];
    PL::template forward<true>(v, tw, ex[0], ex[1], tid);
    for (int m = 0; m < 8; ++m) out[P * m + tid] = v[m];
  }
  if constexpr (R == 2) {
    if (mode == 1 || mode == 2) {
      for (int m = 0; m < 8; ++m) v[m] = in[P * m + tid];
      if (mode == 1) PL::template forward_s<false>(v, tw, ex[0], ex[1], tid);
      else PL::template forward_s<true>(v, tw, ex[0], ex[1], tid);
      for (int m = 0; m < 8; ++m) out[PL::s_index(tid, m)] = v[m];
    } else if (mode == 3) {
      for (int m = 0; m < 8; ++m) v[m] = in[PL::s_index(tid, m)];
      PL::transposed(v, tw, ex[0], ex[1], tid);
      for (int m = 0; m < 8; ++m) out[P * m + tid] = v[m];
    } else if (mode == 4) {
      for (int m = 0; m < 8; ++m) { v[m] = in[P * m + tid]; u[m] = in2[P * m + tid]; }
      PL::template forward_s2<true>(v, u, tw, ex[0], ex[1], ex[2], ex[3], tid);
      for (int m = 0; m < 8; ++m) { out[PL::s_index(tid, m)] = v[m]; out2[PL::s_index(tid, m)] = u[m]; }
    } else if (mode == 5) {
      for (int m = 0; m < 8; ++m) { v[m] = in[PL::s_index(tid, m)]; u[m] = in2[P * m + tid]; }
      PL::transposed_and_forward_s(v, u, tw, ex[0], ex[1], ex[2], ex[3], tid);
      for (int m = 0; m < 8; ++m) { out[P * m + tid] = v[m]; out2[PL::s_index(tid, m)] = u[m]; }
    }
    const float sg = (tid & 1) ? -1.0f : 1.0f;
    if (mode == 13 || mode == 14) {
      for (int m = 0; m < 8; ++m) { v[m] = in[PL::s_index(tid, m)]; u[m] = in2[P * m + tid]; }
      if (mode == 13) PL::transposed_then_forward_s(v, u, tw, ex[0], ex[1], ex[2], tid);
      else PL::template transposed_then_forward_s<true>(v, u, tw, ex[0], ex[1], ex[2], tid);
      const float s2 = mode == 14 ? sg : 1.0f;
      for (int m = 0; m < 8; ++m) { out[P * m + tid] = v[m] * s2; out2[PL::s_index(tid, m)] = u[m] * s2; }
    }
    if (mode >= 15 && mode <= 17) {
      using PP = ddsp::fft::Plan1024P;
      __shared__ __attribute__((aligned(16))) f32x2 exp_[3][PP::WORDS];
      typename PP::Tw twl;
      twl.init(tid);
      typename PP::Ix ix;
      ix.init(tid);
      if (mode == 15) {
        for (int m = 0; m < 8; ++m) v[m] = in[P * m + tid];
        PP::template forward_s<true, true>(v, twl, exp_[0], exp_[1], ix);
        for (int m = 0; m < 8; ++m) out[PL::s_index(tid, m)] = v[m] * sg;
      } else if (mode == 16) {
        for (int m = 0; m < 8; ++m) { v[m] = in[PL::s_index(tid, m)]; u[m] = in2[P * m + tid]; }
        PP::template transposed_then_forward_s<true>(v, u, twl, exp_[0], exp_[1], exp_[2], ix);
        for (int m = 0; m < 8; ++m) { out[P * m + tid] = v[m] * sg; out2[PL::s_index(tid, m)] = u[m] * sg; }
      } else {
        int bad = 0;
        const int mb = PP::mirror_base(tid);
        for (int m = 0; m < 8; ++m) {
          const int want = PP::parked((1024 - PL::s_index(tid, m)) & 1023);
          const bool self = tid < 2 && m == 0;
          if (!self && mb - 64 * m != want) ++bad;
          if (mb - 64 * m < 0 || mb - 64 * m >= PP::WORDS) ++bad;
        }
        out[tid] = f32x2{(float)bad, 0.f};
      }
    }
    if (mode == 6) {
      for (int m = 0; m < 8; ++m) v[m] = in[P * m + tid];
      PL::template forward_s<true, true>(v, tw, ex[0], ex[1], tid);
      for (int m = 0; m < 8; ++m) out[PL::s_index(tid, m)] = v[m] * sg;
    } else if (mode == 7) {
      for (int m = 0; m < 8; ++m) v[m] = in[PL::s_index(tid, m)];
      PL::template transposed<true>(v, tw, ex[0], ex[1], tid);
      for (int m = 0; m < 8; ++m) out[P * m + tid] = v[m] * sg;
    } else if (mode == 8) {
      for (int m = 0; m < 8; ++m) { v[m] = in[P * m + tid]; u[m] = in2[P * m + tid]; }
      PL::template forward_s2<true, true>(v, u, tw, ex[0], ex[1], ex[2], ex[3], tid);
      for (int m = 0; m < 8; ++m) { out[PL::s_index(tid, m)] = v[m] * sg; out2[PL::s_index(tid, m)] = u[m] * sg; }
    } else if (mode == 9) {
      for (int m = 0; m < 8; ++m) { v[m] = in[PL::s_index(tid, m)]; u[m] = in2[P * m + tid]; }
      PL::template transposed_and_forward_s<true>(v, u, tw, ex[0], ex[1], ex[2], ex[3], tid);
      for (int m = 0; m < 8; ++m) { out[P * m + tid] = v[m] * sg; out2[PL::s_index(tid, m)] = u[m] * sg; }
    }
  }
}

// ---- packed complex helpers of fft2048.h, elementwise: record i is 16 complex words in, 16 out (unused outputs stay 0) ----
__device__ __forceinline__ float uniform_f32(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

__global__ void k_helpers(int op, const f32x2* in, f32x2* out, int n) {
  using namespace ddsp::fft;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;                                        // n is a multiple of 64: whole waves leave
  f32x2 a[16], o[16];
  for (int k = 0; k < 16; ++k) { a[k] = in[(size_t)i * 16 + k]; o[k] = f32x2{0.f, 0.f}; }
  switch (op) {
    case 0: o[0] = cmul(a[0], a[1]); break;
    case 1: o[0] = cmul_uniform(a[0], f32x2{uniform_f32(a[1].x), uniform_f32(a[1].y)}); break;   // the factor of the wave's first lane
    case 2: o[0] = cmul_lo(a[0], a[1]); break;
    case 3: o[0] = cmul_hi(a[0], a[1], a[2]); break;
    case 4: o[0] = cmulc_hi(a[0], a[1], a[2]); break;
    case 5: o[0] = cmulc(a[0], a[1]); break;
    case 6: twiddle7(a, a + 8); for (int k = 0; k < 8; ++k) o[k] = a[k]; break;
    case 7: {                                                // u = a[0..7] by a[8..15]; v = a[15..8] by a[7..0]
      f32x2 u[8], wu[8], v[8], wv[8];
      for (int k = 0; k < 8; ++k) { u[k] = a[k]; wu[k] = a[8 + k]; v[k] = a[15 - k]; wv[k] = a[7 - k]; }
      twiddle7x2(u, wu, v, wv);
      for (int k = 0; k < 8; ++k) { o[k] = u[k]; o[8 + k] = v[k]; }
      break;
    }
    case 8: o[0] = add_mi(a[0], a[1]); break;
    case 9: o[0] = sub_mi(a[0], a[1]); break;
    case 10: o[0] = add_conj(a[0], a[1]); break;
    case 11: o[0] = sub_conj(a[0], a[1]); break;
    case 12: o[0] = swap_scale(a[0], a[1]); break;
    case 13: o[0] = swap_scale_add(a[0], a[1], a[2]); break;
    case 14: o[0] = conj_minus_i_conj(a[0], a[1]); break;
    case 15: dft4(a[0], a[1], a[2], a[3]); for (int k = 0; k < 4; ++k) o[k] = a[k]; break;
    case 16: dft4_rot2(a[0], a[1], a[2], a[3]); for (int k = 0; k < 4; ++k) o[k] = a[k]; break;
    case 17: dft8(a); for (int k = 0; k < 8; ++k) o[k] = a[k]; break;
    case 18: for (int k = 4; k < 8; ++k) a[k] = f32x2{0.f, 0.f}; dft8_lo4(a); for (int k = 0; k < 8; ++k) o[k] = a[k]; break;
    default: break;
  }
  for (int k = 0; k < 16; ++k) out[(size_t)i * 16 + k] = o[k];
}

// ---- wave scans and reductions of ddsp_common.h: one value per lane, every lane writes what it got ----
__global__ void k_wave_f64(const double* in, double* incl, double* excl, double* sum) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const double v = in[i];
  incl[i] = ddsp::wave_incl_scan(v);
  excl[i] = ddsp::wave_excl_scan(v, threadIdx.x & 63);
  sum[i] = ddsp::wave_sum(v);
}
__global__ void k_wave_f32(const float* in, float* sum) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  sum[i] = ddsp::wave_sum_dpp(in[i]);
}
__global__ void k_wave_u32(const unsigned* in, unsigned* mx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  mx[i] = ddsp::wave_max_dpp(in[i]);
}

// ---- hardware-math wrappers of ddsp_common.h, elementwise over a grid-stride loop ----
__global__ void k_math(int fn, const float* a, const float* b, float* out, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float r = 0.f;
    switch (fn) {
      case 0: r = ddsp::tanh_hw(a[i]); break;
      case 1: r = ddsp::exp_hw(a[i]); break;
      case 2: r = ddsp::sin_turns(a[i]); break;
      case 3: {                                              // sin_turns2 on (a[i], b[i]): the low half here, the high half in case 4
        r = ddsp::sin_turns2(f32x2{a[i], b[i]}).x; break;
      }
      case 4: r = ddsp::sin_turns2(f32x2{a[i], b[i]}).y; break;
      case 5: r = ddsp::sinc_f32(a[i]); break;
      case 6: r = ddsp::div_pos(a[i], b[i]); break;
      case 7: r = ddsp::cis_pi(a[i]).x; break;
      case 8: r = ddsp::cis_pi(a[i]).y; break;
      default: break;
    }
    out[i] = r;
  }
}
// PhaseCfg::term on the inference path: f0.double() / sr through the reciprocal and one residual correction
__global__ void k_phase_term(const float* f0, double* out, long n, double sr) {
  ddsp::PhaseCfg c;
  c.sr_d = sr; c.rsr_d = 1.0 / sr; c.sr_f = (float)sr; c.infer = 1; c.has_ip = 0;      // as phase.hip builds it
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = c.term(f0[i]);
}

// ---- BufF32: lane i accesses float offset off[i] of a descriptor over n_floats floats at base ----
// op 0 ld, 1 ld_nt (-> got[i]); 2 st, 3 st_nt (of val[i])
__global__ void k_buf(int op, float* base, int n_floats, const int* off, const float* val, float* got, int n) {
  const ddsp::BufF32 buf = ddsp::BufF32::make(base, n_floats);
  const int i = threadIdx.x;
  if (i >= n) return;
  const int byte_off = off[i] * 4;
  if (op == 0) got[i] = buf.ld(byte_off);
  else if (op == 1) got[i] = buf.ld_nt(byte_off);
  else if (op == 2) buf.st(val[i], byte_off);
  else if (op == 3) buf.st_nt(val[i], byte_off);
}
}  // namespace

static int launched() { return (int)hipGetLastError(); }
static hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }

// complex arrays as interleaved float pairs, `batch` inputs of 512 R words each
extern "C" int du_fft_plan(int R, int mode, int batch, const float* in, const float* in2, float* out, float* out2, void* stream) {
  const f32x2* a = reinterpret_cast<const f32x2*>(in);
  const f32x2* b = reinterpret_cast<const f32x2*>(in2);
  f32x2* c = reinterpret_cast<f32x2*>(out);
  f32x2* d = reinterpret_cast<f32x2*>(out2);
  if (batch < 1) return -1;
  if (R == 1) hipLaunchKernelGGL(k_plan<1>, dim3(batch), dim3(64), 0, as_stream(stream), mode, a, b, c, d);
  else if (R == 2) hipLaunchKernelGGL(k_plan<2>, dim3(batch), dim3(128), 0, as_stream(stream), mode, a, b, c, d);
  else if (R == 4) hipLaunchKernelGGL(k_plan<4>, dim3(batch), dim3(256), 0, as_stream(stream), mode, a, b, c, d);
  else if (R == 8) hipLaunchKernelGGL(k_plan<8>, dim3(batch), dim3(512), 0, as_stream(stream), mode, a, b, c, d);
  else return -1;
  return launched();
}
// n records (a multiple of 64) of 16 complex words in and out
extern "C" int du_helpers(int op, const float* in, float* out, int n, void* stream) {
  if (n < 64 || n % 64) return -1;
  hipLaunchKernelGGL(k_helpers, dim3(n / 64), dim3(64), 0, as_stream(stream), op, reinterpret_cast<const f32x2*>(in),
                     reinterpret_cast<f32x2*>(out), n);
  return launched();
}
// `waves` waves of 64 values, waves_per_block of them to a workgroup
extern "C" int du_wave_f64(const double* in, double* incl, double* excl, double* sum, int waves, int waves_per_block, void* stream) {
  if (waves < 1 || waves_per_block < 1 || waves % waves_per_block) return -1;
  hipLaunchKernelGGL(k_wave_f64, dim3(waves / waves_per_block), dim3(64 * waves_per_block), 0, as_stream(stream), in, incl, excl, sum);
  return launched();
}
extern "C" int du_wave_f32(const float* in, float* sum, int waves, int waves_per_block, void* stream) {
  if (waves < 1 || waves_per_block < 1 || waves % waves_per_block) return -1;
  hipLaunchKernelGGL(k_wave_f32, dim3(waves / waves_per_block), dim3(64 * waves_per_block), 0, as_stream(stream), in, sum);
  return launched();
}
extern "C" int du_wave_u32(const unsigned* in, unsigned* mx, int waves, int waves_per_block, void* stream) {
  if (waves < 1 || waves_per_block < 1 || waves % waves_per_block) return -1;
  hipLaunchKernelGGL(k_wave_u32, dim3(waves / waves_per_block), dim3(64 * waves_per_block), 0, as_stream(stream), in, mx);
  return launched();
}
extern "C" int du_math(int fn, const float* a, const float* b, float* out, long n, void* stream) {
  hipLaunchKernelGGL(k_math, dim3(256), dim3(256), 0, as_stream(stream), fn, a, b, out, n);
  return launched();
}
extern "C" int du_phase_term(const float* f0, double* out, long n, double sr, void* stream) {
  hipLaunchKernelGGL(k_phase_term, dim3(256), dim3(256), 0, as_stream(stream), f0, out, n, sr);
  return launched();
}
extern "C" int du_buf(int op, float* base, int n_floats, const int* off, const float* val, float* got, int n, void* stream) {
  if (n < 0 || n > 128) return -1;
  hipLaunchKernelGGL(k_buf, dim3(1), dim3(128), 0, as_stream(stream), op, base, n_floats, off, val, got, n);
  return launched();
}
