/* ddsp_hip.h -- C ABI of libddsp_hip.so, the MI355X (gfx950) implementation of the DDSP-SVC
 * harmonic-plus-noise synthesis hot path.
 *
 * The reference (yxlllc/DDSP-SVC) is pure Python: the seam for this path is its Python API
 * (ddsp/core.py functions, ddsp/vocoder.py Sins/CombSub forward).  These entry points are what a
 * ctypes binding on the reference side calls; each one names the reference
 * code it replaces.  Conventions:
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     (torch tensors' data_ptr()), including workspaces -- the library never allocates or frees;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*), nothing synchronises;
 *   - return 0 on success, a negative DDSP_HIP_E* code for argument errors, or a positive
 *     hipError_t if a launch failed; ddsp_hip_error_string() decodes both;
 *   - tensors are float32 row-major; B = utterances, F = frames, hop = samples per frame,
 *     T = F*hop; control tensors take a row stride `ld` (floats between consecutive frames) so
 *     the torch.split views of Unit2Control's output can be passed without a copy;
 *   - more than 65 535 utterances in one call (a grid's limit in y and z): ddsp_hip_resblock1(_wide), ddsp_hip_upsample_stage,
 *     ddsp_hip_output_head, ddsp_hip_conformer_conv, ddsp_hip_wavenet_layer, ddsp_hip_naive_v2_layer, ddsp_hip_resample and ddsp_hip_mel_shifted_spectrogram split the batch into launches of 65 535; ddsp_hip_fast_source and
 *     ddsp_hip_combsubsuperfast_synth run their exciter on a flat grid then; ddsp_hip_sine_source(_drawn),
 *     ddsp_hip_spectral_loss(_backward), ddsp_hip_stft_loss(_backward), ddsp_hip_mel_spectrogram_backward,
 *     ddsp_hip_sola_splice, ddsp_hip_volume, ddsp_hip_gate, ddsp_hip_pool1d, ddsp_hip_fft_convolve with
 *     DDSP_HIP_FIR_SIMPLE and ddsp_hip_fft_convolve_backward at shapes only its direct form takes (hop != 512 or
 *     N > 1022) return DDSP_HIP_ESHAPE before any launch; the other entries index utterances
 *     on a flat grid.
 */
#ifndef DDSP_HIP_H
#define DDSP_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDSP_HIP_VERSION 165          /* 0.1.6.5: + ddsp_hip_allpass_taps_backward; ddsp_hip_combsub_tail_backward is three launches (the all-pass activation's adjoint in the tap adjoint's last stage), knob AP_BWD_SPLIT; 0.1.6.4: the fused layouts keep the noise filter's (even) tap rows as their first half, knob TAPS_FULL; 0.1.6.3: + ddsp_hip_mel_shifted_* (get_mel with keyshift / speed / center, any transform length); 0.1.6.2: + ddsp_hip_tail_layout, ddsp_hip_combsub_tail_backward; the fused one-stream layout of the tails at every shape (knob STREAM_LAYOUT 1 / 4: the two-stream ones); knob BWD_WPS */

#define DDSP_HIP_EINVAL   (-1)        /* bad size / null pointer */
#define DDSP_HIP_EHOP     (-2)        /* hop > 2048: wave-per-frame phase scan does not cover it */
#define DDSP_HIP_ESHAPE   (-3)        /* shape outside what the selected kernel supports */
#define DDSP_HIP_EWS      (-4)        /* workspace too small */

/* window handling of frequency_impulse_response (ddsp/core.py:254-270) */
#define DDSP_HIP_MODE_ROLL    0       /* hann_window=False                     core.py:269 */
#define DDSP_HIP_MODE_HANN    1       /* hann_window=True, half_width=None     core.py:263-264 */
#define DDSP_HIP_MODE_DYNAMIC 2       /* hann_window=True, half_width given    core.py:265-266 */

/* what the response pointers hold */
#define DDSP_HIP_ACT_NONE 0           /* the (real, imaginary) response itself, as ddsp.core takes it */
#define DDSP_HIP_ACT_EXP  1           /* raw control c: response = scale * exp(c)   vocoder.py:580,582,835,836 */

/* FIR implementation selector (0 lets the library choose) */
#define DDSP_HIP_FIR_AUTO   0
#define DDSP_HIP_FIR_SIMPLE 1
#define DDSP_HIP_FIR_MFMA   2       /* 4 waves = 1024 outputs per workgroup */
#define DDSP_HIP_FIR_MFMA8  3       /* 8 waves = 2048 outputs per workgroup */
#define DDSP_HIP_FIR_FFT    4       /* frequency-domain block convolution per frame (2048-point), hop 512, N <= 512 */
#define DDSP_HIP_FIR_BLK    5       /* frequency-domain convolution per hop block (1024-point), hop 512, N <= 512 */

int ddsp_hip_version(void);
const char* ddsp_hip_error_string(int code);

/* Tuning / test knobs of the launchers (workgroup run lengths, which occupancy build of a kernel is launched, ...):
 * names as in DESIGN.md section 7 without the DDSP_HIP_ prefix ("BLK_RUN", "STFT_WPS", ...).  Each knob takes its
 * initial value from the environment variable DDSP_HIP_<NAME> ONCE, at first use; after that only set_tuning changes
 * it (0 = built-in default).  No reference counterpart: measurement tools and the run-split tests use them.
 * Knobs that choose between forms of one operation: TAPS_GEMM (tap synthesis and its adjoint: 0 = by bin count -- prime
 * factors at 256, chirp-z from 112 to 1025, the dense contraction elsewhere; 1 = the dense contraction everywhere;
 * 2 = chirp-z wherever its plans reach), SINS_V1 (1 = the generic sinusoid bank at every hop; 2 is retired and refused), STFT_WPS (waves per SIMD of the short-time
 * spectral filter's variants), CZT_ROUNDS (rounds of resident workgroups of the loss kernels), CZT_TURNS (priority turns of a SIMD's waves in the loss's
 * backward kernel: 0 = on, 2 = off), BLK_WPS and BLK_PADLDS (retired with round 3's two-wave hop-block filter: any non-zero
 * value is refused, -1 from set_tuning and a warning from the environment), SINS_NOSKIP (1 = the sinusoid bank also sums the harmonics that are masked
 * to 1e-7 in both frames of a hop), SMALL_PATH (1 = never take the fused launches of the streaming shapes, B F < 4096: the
 * batch layout at every size; the results are the same bits either way), TAPS_FULL (1 = the fused layouts keep the noise
 * filter's tap rows whole, [B,F,N], instead of their first N/2 + 1 taps -- an even response; same bits either way),
 * AP_BWD_SPLIT (1 = ddsp_hip_combsub_tail_backward runs the all-pass activation's adjoint as a launch of its own instead of
 * in the last stage of the tap adjoint), SINS_SEQ (1 = the Sins tail's two filters as two launches instead of one whose workgroups
 * run the noise filter and then the all-pass filter over the same samples; same bits), BATCH_SPLIT (test knob: 1 .. 65535 =
 * the utterances per launch of the three entries that split a batch past the grid's 65 535, so that a handful of utterances
 * reach a second launch; 0 or anything else = 65 535; same bits); the rest are run lengths. */
int ddsp_hip_set_tuning(const char* name, long value);
long ddsp_hip_get_tuning(const char* name);

/* ddsp/core.py:66-70  upsample(signal[B,F,C], factor=hop) -> out[B,F*hop,C] */
int ddsp_hip_upsample(const float* sig, int B, int F, int C, int hop, float* out, void* stream);

/* ddsp/core.py:73-77  remove_above_fmax(amplitudes[rows,H], pitch[rows], fmax, level_start) */
int ddsp_hip_remove_above_fmax(const float* amps, const float* pitch, long rows, int H, float fmax,
                               int level_start, float* out, void* stream);

/* ddsp/vocoder.py:564-575 (Sins) == :819-829 (CombSub): upsample f0, cumulative sum of f0/sr
 * (float64 if infer, float32 outputs of a float64 running sum otherwise), optional initial phase,
 * wrap to [-0.5,0.5].
 *   f0_frames[B,F]; initial_phase[B] radians or NULL;
 *   frame_sums[B,F] (double, scratch); phase0[B,F] (double): unwrapped running sum before each
 *   frame -- the state the synth entry points consume; phase_frames[B,F] = 2*pi*x[:, ::hop]
 *   (what Unit2Control receives); x_or_null[B,T]: the full wrapped phase if the caller wants it. */
int ddsp_hip_phase(const float* f0_frames, const float* initial_phase, int B, int F, int hop, double sr,
                   int infer, double* frame_sums, double* phase0, float* phase_frames, float* x_or_null,
                   void* stream);

/* basis table for n_mag bins (cosine | sine | periodic Hann); build once per n_mag and keep it */
size_t ddsp_hip_ir_table_bytes(int n_mag);
int ddsp_hip_ir_table(int n_mag, float* table, void* stream);

/* ddsp/vocoder.py:581,599 / :834,845  exp(1j*cumsum(pi*tanh(c), -1)) -> re, im [rows,n_mag] */
int ddsp_hip_allpass_response(const float* c, long ld, long rows, int n_mag, float* re, float* im,
                              void* stream);

/* ddsp/core.py:254-270  frequency_impulse_response: one-sided response [rows,n_mag] (+ imaginary
 * part or NULL) -> causal-form taps [rows, N=2*(n_mag-1)]; `act`/`scale` fuse the control
 * activation, `half_width[rows]` is required for MODE_DYNAMIC. */
int ddsp_hip_impulse_response(const float* resp_re, long ld_re, const float* resp_im, long ld_im, int act,
                              float scale, int mode, const float* half_width, long rows, int n_mag,
                              const float* table, float* taps, void* stream);

/* The two calls above in one, from the raw group-delay control c[rows,n_mag] (row stride ld) to the all-pass taps
 * [rows, 2*(n_mag-1)] (vocoder.py:581,599 / :834,845 + core.py:254-270, hann_window=False).  For n_mag = 256 the response
 * never reaches memory (prime-factor kernel); other sizes stage it in `scratch` (allpass_taps_scratch_bytes). */
size_t ddsp_hip_allpass_taps_scratch_bytes(long rows, int n_mag);
int ddsp_hip_allpass_taps(const float* c, long ld, long rows, int n_mag, const float* table, float* taps, void* scratch,
                          size_t scratch_bytes, void* stream);

/* Adjoints of the two calls above (what autograd returns for the response / the raw control):
 *   impulse_response_backward: d_taps[rows,N] -> d_re[rows,n_mag] (+ d_im[rows,n_mag] when d_im is not NULL:
 *   the complex case, act NONE only; every window mode -- the reference builds its real responses as
 *   torch.complex(param, 0), vocoder.py:606,849,857, so a windowed complex response under autograd is the normal case).  With act EXP the result is the gradient of the raw control
 *   itself (d_re = dL/dc = dL/dresp * scale * exp(c), ctrl/ld_ctrl = the forward's resp_re/ld_re); the window
 *   (mode, half_width) is a constant factor.
 *   allpass_backward: (d_re, d_im)[rows,n_mag] of exp(1j*cumsum(pi*tanh(c))) -> d_c[rows,n_mag]. */
int ddsp_hip_impulse_response_backward(const float* d_taps, const float* ctrl, long ld_ctrl, int act, float scale,
                                       int mode, const float* half_width, long rows, int n_mag, const float* table,
                                       float* d_re, float* d_im, void* stream);
/* ddsp/core.py:185-237 apply_window_to_impulse_response (window_size = 0, causal = False) and :240-251
 * apply_dynamic_window_to_impulse_response on taps that are already in the time domain: zero-phase taps ir[rows,N] ->
 * windowed causal taps out[rows,N] (out != ir), out[j] = ir[(j - N/2) mod N] * w(j); MODE_ROLL = the bare roll of
 * core.py:269.  N may be odd in MODE_DYNAMIC (the reference allows 2*n_mag-1 there). */
int ddsp_hip_window_impulse_response(const float* ir, int mode, const float* half_width, long rows, int N, float* out,
                                     void* stream);
int ddsp_hip_allpass_backward(const float* c, long ld, long rows, int n_mag, const float* d_re, const float* d_im,
                              float* d_c, void* stream);
/* The two adjoints above back to back for the all-pass taps of vocoder.py:597-600 / :843-846 (what autograd returns for the raw
 * group-delay control c [rows, ld] given d taps [rows, 2 (n_mag - 1)]): d_c [rows, n_mag].  ONE launch at 256 bins (d_c 16-byte
 * aligned); elsewhere two launches through the scratch d_re_ws / d_im_ws ([rows, n_mag] each) -- DDSP_HIP_EWS when they are needed
 * and NULL. */
int ddsp_hip_allpass_taps_backward(const float* d_taps, const float* c, long ld, long rows, int n_mag, const float* table,
                                   float* d_c, float* d_re_ws, float* d_im_ws, void* stream);

/* ddsp/core.py:120-182  fft_convolve(audio[B,T], taps[B,F,N]) -> out[B,T]  (T = F*hop).
 * x_is_u01: the input is a raw U[0,1) draw and 2*u-1 is applied on load (vocoder.py:603,854);
 * addend[B,T] or NULL is added to the result (vocoder.py:609,860); out_plain[B,T] or NULL also
 * receives the un-added result. */
int ddsp_hip_fft_convolve(const float* audio, int x_is_u01, const float* taps, const float* addend,
                          float* out, float* out_plain, int B, int F, int hop, int N, int impl, void* stream);

/* ddsp/core.py:273-280  frequency_filter(audio[B,T], magnitudes[B,F,n_mag] (complex: resp_re + i resp_im, resp_im
 * may be NULL), hann_window, half_width_frames) = fft_convolve(audio, frequency_impulse_response(...)) in one call.
 * mode / half_width[B*F] as ddsp_hip_impulse_response; ws holds the taps
 * (ddsp_hip_frequency_filter_workspace_bytes(B, F, n_mag) bytes); out[B,T]. */
size_t ddsp_hip_frequency_filter_workspace_bytes(int B, int F, int n_mag);
int ddsp_hip_frequency_filter(const float* audio, const float* resp_re, long ld_re, const float* resp_im, long ld_im,
                              int mode, const float* half_width, int B, int F, int hop, int n_mag,
                              const float* table, float* out, void* ws, size_t ws_bytes, void* stream);

/* What autograd returns for ddsp_hip_fft_convolve given grad_out[B,T] = dL/dout: d_taps[B,F,N] and, if
 * d_audio is not NULL, d_audio[B,T] (the adjoints of core.py:120-182; training back-propagates through them,
 * solver.py:93-103).  hop 512, N <= 512: the hop-block FFT form; every other hop / even N: direct correlations
 * (csrc/fir_bwd_direct.hip; ~1 ms per launch at B = 32 x 10 s, N = 1022). */
int ddsp_hip_fft_convolve_backward(const float* audio, int x_is_u01, const float* taps, const float* grad_out,
                                   float* d_audio, float* d_taps, int B, int F, int hop, int N, void* stream);

/* The uniform draw of the noise branch (vocoder.py:603, :854 rand_like) as a counter-based stream, for callers that do
 * not want to materialise torch.rand: u[B,T] in [0,1) from Philox4x32-10 keyed by `seed`, counter = (128 * (t / 512) +
 * t % 128, utterance, offset lo, offset hi), output word (t % 512) / 128 -- reproducible from (seed, offset), independent
 * of launch geometry.  It is NOT torch's stream: the same seed gives different numbers than torch.rand (torch's mapping
 * of elements to counters depends on its launch geometry; reproducing it inside the filter would cost four generator
 * calls per block and thread instead of one).  The synthesiser tails below draw exactly these numbers inside their noise
 * filter when `noise` is NULL (hop 512, n_nz <= 257); this entry point writes them out. */
int ddsp_hip_uniform_noise(unsigned long long seed, unsigned long long offset, int B, long T, float* out, void* stream);

/* DSP tail of Sins.forward (ddsp/vocoder.py:580-611) from raw controls and the phase state.
 * noise[B,T]: uniform draw (noise_is_u01 ? U[0,1) : already 2u-1), or NULL: drawn inside the noise filter from
 * (noise_seed, noise_offset) as ddsp_hip_uniform_noise defines it (opt-in: 4 B / sample less HBM traffic and no separate
 * generator kernel, for ~20 % more arithmetic in that one filter launch); tables for n_ap / n_nz bins.
 * signal[B,T]; harmonic_or_null / noise_out_or_null [B,T] only if the caller wants the tuple. */
int ddsp_hip_sins_synth(const float* f0_frames, const float* initial_phase, const double* phase0,
                        const float* c_amp, long ld_amp, const float* c_gd, long ld_gd,
                        const float* c_nz, long ld_nz, const float* noise, int noise_is_u01,
                        int B, int F, int hop, double sr, int infer, int H, int n_ap, int n_nz,
                        const float* table_ap, const float* table_nz,
                        float* signal, float* harmonic_or_null, float* noise_out_or_null,
                        void* ws, size_t ws_bytes, int fir_impl, void* stream, void* aux_stream,
                        unsigned long long noise_seed, unsigned long long noise_offset);

/* DSP tail of CombSub.forward (ddsp/vocoder.py:834-862). */
int ddsp_hip_combsub_synth(const float* f0_frames, const float* initial_phase, const double* phase0,
                           const float* c_gd, long ld_gd, const float* c_harm, long ld_harm,
                           const float* c_nz, long ld_nz, const float* noise, int noise_is_u01,
                           int B, int F, int hop, double sr, int infer, int n_ap, int n_harm, int n_nz,
                           const float* table_ap, const float* table_harm, const float* table_nz,
                           float* signal, float* harmonic_or_null, float* noise_out_or_null,
                           void* ws, size_t ws_bytes, int fir_impl, void* stream, void* aux_stream,
                           unsigned long long noise_seed, unsigned long long noise_offset);

/* Launch layout (round 6).  With every filter at 256 bins and hop 512 -- the shipped configurations -- a call is issued on `stream`
 * ALONE: CombSub as three launches (exciter + the three tap syntheses as jobs of one launch | all-pass filter + noise filter as two
 * jobs of one launch | harmonic filter + noise), Sins as four; `aux_stream` is not used (independent kernels as jobs of ONE launch save
 * a ramp and a drain each, where two streams paid three cross-stream hand-overs for an overlap that is worth less: 0.319 -> 0.302 ms
 * at B = 32 x 10 s).  Tuning knob STREAM_LAYOUT = 1 / 4 restores the two-stream layouts at batch shapes.  Other bin counts / hops:
 *
 * aux_stream (both calls above): NULL, or a second stream of the same device, which must be the calling thread's
 * current device (hipSetDevice) -- the fork / join events are taken from a per-device pool there.  The noise branch (its taps and its
 * filter: independent of the harmonic chain until the final sum) is then enqueued there -- forked after everything
 * already on `stream`, joined back before the last kernel on `stream`, so for the caller the call still behaves as
 * one operation on `stream` -- and fills the machine where the chain's kernels leave it idle (tails, store phases).
 * Results are bit-identical to the one-stream order.  The events this needs come from a process-wide pool per device, checked
 * out per call (the only objects the library creates, beside the second lane's streams of knob LANE_ROWS). */

/* workspace the two synth entry points need (bytes); n_max = largest n_mag among the filters.  `ws` must be 16-byte
 * aligned (the tap arrays carved out of it are written 16 bytes at a time); an unaligned pointer is DDSP_HIP_EINVAL.
 * 256-bin models at hop 512 (and every model below 4096 frames): the workspace holds one tap buffer more (the fused layout
 * above: all tap syntheses of a step are one launch). */
size_t ddsp_hip_synth_workspace_bytes(int B, int F, int hop, int n_max);

/* Where a ddsp_hip_combsub_synth (combsub != 0; n0, n1, n2 = n_ap, n_harm, n_nz) / ddsp_hip_sins_synth (n0 = H, n1 = n_ap,
 * n2 = n_nz) call of this shape LEAVES ITS INTERMEDIATES in the workspace -- what a training caller keeps for the backward pass
 * (solver.py:93-103: the same forward with gradients) instead of recomputing or re-running the tail as separate operators:
 * byte offsets into `ws` of [0] the exciter [B,T], [1] the all-pass filter's output [B,T] (CombSub), [2] the all-pass taps
 * [B,F,N], [3] the harmonic taps (CombSub), [4] the noise taps -- [B,F,N/2+1]: the first N/2 + 1 taps of an even response (tap
 * N - j is tap j) unless knob TAPS_FULL --, [5] the filtered noise (when no noise output was passed); -1 = not kept.  Returns 1 when the call takes the fused layout and the offsets are valid until the workspace is written again, 0
 * when it does not (other bin counts / hops, in-kernel noise, sub-batch lanes: nothing is promised), < 0 on bad arguments. */
int ddsp_hip_tail_layout(int combsub, int B, int F, int hop, int n0, int n1, int n2, int fir_impl, int in_kernel_noise,
                         long long offsets[6]);

/* The backward pass of a fused ddsp_hip_combsub_synth call (256 / 256 / 256 bins, hop 512: where ddsp_hip_tail_layout returns 1) as
 * THREE launches on `stream`: what autograd returns for the three raw controls of vocoder.py:834-862 given the cotangents that
 * reach the harmonic branch (g_harm [B,T]: d signal + d harmonic) and the noise branch (g_noise [B,T]: d signal + d noise); either
 * may be NULL (that branch's gradients are not written).  fwd_ws is the forward call's workspace, untouched since; f0 / controls /
 * noise are that call's; table = the 256-bin basis table.  d_gd, d_harm, d_nz: [B,F,256] contiguous.  ws (16-byte aligned):
 * ddsp_hip_combsub_tail_backward_ws_bytes(B, F, hop, 256) bytes.  DDSP_HIP_ESHAPE for any other shape (use the per-operator
 * adjoints: ddsp_hip_fft_convolve_backward, ddsp_hip_impulse_response_backward, ddsp_hip_allpass_backward). */
size_t ddsp_hip_combsub_tail_backward_ws_bytes(int B, int F, int hop, int n_mag);
int ddsp_hip_combsub_tail_backward(const float* f0_frames, const float* c_gd, long ld_gd, const float* c_harm, long ld_harm,
                                   const float* c_nz, long ld_nz, const float* noise, int noise_is_u01, const void* fwd_ws,
                                   const float* g_harm, const float* g_noise, int B, int F, int hop, double sr, int n_mag,
                                   const float* table, float* d_gd, float* d_harm, float* d_nz, void* ws, size_t ws_bytes,
                                   void* stream);

/* exciters on their own (used by tests and by callers that want the intermediate):
 * combtooth (vocoder.py:839-840) and the sinusoid bank (vocoder.py:585-594), out[B,T] */
int ddsp_hip_combtooth(const float* f0_frames, const float* initial_phase, const double* phase0, int B, int F,
                       int hop, double sr, int infer, float* out, void* stream);
int ddsp_hip_sinusoid_bank(const float* f0_frames, const float* initial_phase, const double* phase0,
                           const float* c_amp, long ld_amp, int B, int F, int hop, int H, double sr, int infer,
                           float* out, void* stream);

/* Adjoint of ddsp_hip_sinusoid_bank w.r.t. the raw amplitude control: grad_out[B,T] -> d_c_amp[B,F,H]
 * (contiguous).  scratch: ddsp_hip_sinusoid_bank_backward_scratch_bytes(B, F, H) bytes.  Every hop <= 2048 (hop 512: the
 * matrix-pipe form; other hops: one wave per frame, direct sines, as the forward bank there). */
size_t ddsp_hip_sinusoid_bank_backward_scratch_bytes(int B, int F, int H);
int ddsp_hip_sinusoid_bank_backward(const float* f0_frames, const float* initial_phase, const double* phase0,
                                    const float* c_amp, long ld_amp, const float* grad_out, int B, int F, int hop,
                                    int H, double sr, int infer, void* scratch, float* d_c_amp, void* stream);

/* ---- CombSubFast / CombSubSuperFast (ddsp/vocoder.py:613-786): short-time spectral filtering ---- */

/* ddsp/vocoder.py:639-651  CombSubSuperFast.fast_source_gen(f0_frames[B,F]): closed-form per-frame
 * phase with a float32 frame-rate accumulator.
 *   rad_acc[B,F]: fmod(cumsum(rad2), 1) (:646), the state the exciter restarts from;
 *   phase_frames[B,F] or NULL = 2*pi*rad[:, :, 0] (:650, what Unit2Control receives);
 *   combtooth[B,T] or NULL = sinc(rad / (s0 + 1e-5)) (:649). */
int ddsp_hip_fast_source(const float* f0_frames, int B, int F, int hop, double sr, float* rad_acc,
                         float* phase_frames, float* combtooth, void* stream);

/* The shared tail of both models: frames of `win` samples every `hop` (win/2 padding each side:
 * reflect as torch.stft does (:667-684) or zeros (:766)), times window[win], rfft, times the
 * per-frame filters exp(c_hmag + i*pi*c_hphase) (exciter) and noise_scale*exp(c_nmag +
 * i*pi*c_nphase) (noise; c_nphase NULL = zero phase, :760), last filter frame repeated (:662,:759),
 * irfft, times window, overlap-add, crop win/2 (:783-784); normalize != 0 divides by the
 * overlap-added squared window as torch.istft does (:702-708).
 *   exciter, noise, signal [B,T]; controls [B,F,win/2+1] with row strides ld_*; window[win].
 * Supported: hop 512 with win 1024 (CombSubFast) or 2048 (CombSubSuperFast). */
int ddsp_hip_stft_filter(const float* exciter, const float* noise, int noise_is_u01,
                         const float* c_hmag, long ld_hmag, const float* c_hphase, long ld_hphase,
                         const float* c_nmag, long ld_nmag, const float* c_nphase, long ld_nphase,
                         float noise_scale, const float* window, int win, int pad_reflect, int normalize,
                         int B, int F, int hop, float* signal, void* stream);

/* What autograd returns for the four control streams of ddsp_hip_stft_filter given grad_signal[B,T] =
 * dL/dsignal (training: solver.py:93-103 back-propagates through CombSubFast / CombSubSuperFast.forward):
 * d_hmag, d_hphase, d_nmag [B,F,win/2+1] contiguous, d_nphase likewise or NULL when c_nphase is NULL.
 * Same arguments and supported shapes as the forward entry point. */
int ddsp_hip_stft_filter_backward(const float* exciter, const float* noise, int noise_is_u01,
                                  const float* c_hmag, long ld_hmag, const float* c_hphase, long ld_hphase,
                                  const float* c_nmag, long ld_nmag, const float* c_nphase, long ld_nphase,
                                  float noise_scale, const float* window, int win, int pad_reflect, int normalize,
                                  const float* grad_signal, int B, int F, int hop,
                                  float* d_hmag, float* d_hphase, float* d_nmag, float* d_nphase, void* stream);

/* DSP tail of CombSubFast.forward (ddsp/vocoder.py:758-784) from raw controls and the phase state of
 * ddsp_hip_phase: combtooth (:764) -> sqrt-Hann frames of 2*hop -> filters -> overlap-add.
 * noise[B,T]: uniform draw (noise_is_u01 ? U[0,1) : already 2u-1, :771); window[2*hop] is the
 * module's buffer (:726); ws: B*T floats (ddsp_hip_stft_workspace_bytes). */
int ddsp_hip_combsubfast_synth(const float* f0_frames, const float* initial_phase, const double* phase0,
                               const float* c_hmag, long ld_hmag, const float* c_hphase, long ld_hphase,
                               const float* c_nmag, long ld_nmag, const float* noise, int noise_is_u01,
                               const float* window, int B, int F, int hop, double sr, int infer,
                               float* signal, void* ws, size_t ws_bytes, void* stream);

/* DSP tail of CombSubSuperFast.forward (ddsp/vocoder.py:661-708) from raw controls and rad_acc of
 * ddsp_hip_fast_source.  noise[B,T] is the standard-normal draw (:687); window[win] the module's
 * Hann buffer (:629). */
int ddsp_hip_combsubsuperfast_synth(const float* f0_frames, const float* rad_acc,
                                    const float* c_hmag, long ld_hmag, const float* c_hphase, long ld_hphase,
                                    const float* c_nmag, long ld_nmag, const float* c_nphase, long ld_nphase,
                                    const float* noise, const float* window, int win, int B, int F, int hop,
                                    double sr, float* signal, void* ws, size_t ws_bytes, void* stream);

size_t ddsp_hip_stft_workspace_bytes(int B, int F, int hop);

/* ---- log-mel front-end of the cascade (nsf_hifigan/nvSTFT.py:73-117) ---- */

/* STFT.get_mel(y, keyshift=0, speed=1, center=False): pad (win-hop)/2 both sides (reflect, or zeros when
 * the right pad is not shorter than the signal, :97-103), frames of n_fft every hop, window[n_fft] (periodic
 * Hann, :93-94), rfft, sqrt(re^2+im^2+1e-9) (:108), mel_basis[n_mels, n_fft/2+1] @ spec (:115),
 * log(clamp(., clip_val)) (:116).
 *   audio[B,T]; band[n_mels][4] (int32) = {first, one-past-last non-zero bin of the mel_basis row, offset of
 *   the row's band weights in band_weights, 0}: the projection only visits that band; band_weights (or NULL)
 *   holds every row's band back to back (n_band_weights floats, staged on chip when <= 4096, else the dense
 *   basis is read); out element (b, mel, frame) is written at
 *   out[b*stride_b + mel*stride_mel + frame*stride_frame], frames = ddsp_hip_mel_frames(T, n_fft, hop).
 * Supported: n_fft == win == 2048, hop == 512 (the 44.1 kHz NSF-HiFiGAN configuration). */
int ddsp_hip_mel_frames(int T, int n_fft, int hop);
int ddsp_hip_mel_spectrogram(const float* audio, int B, int T, const float* window, int n_fft, int hop,
                             const float* mel_basis, const int* band, const float* band_weights,
                             int n_band_weights, int n_mels, float clip_val,
                             float* out, long stride_b, long stride_mel, long stride_frame, void* stream);

/* Adjoint of ddsp_hip_mel_spectrogram w.r.t. the waveform (the cascades' DDSP loss, F.mse_loss(get_mel(ddsp_wav), gt)):
 * grad_audio[B,T] (contiguous, overwritten) = d <grad_out, log-mel> / d audio, for the cotangent element (b, mel, frame) read
 * at grad_out[b*stride_b + mel*stride_mel + frame*stride_frame] (any strides, 0 included).  The forward's arguments
 * otherwise; bin_filters (int32) = n_fft/2+2 offsets, then filter ids: bin k lies in the band of the filters
 * bin_filters[n_fft/2+2 + e], e in [bin_filters[k], bin_filters[k+1]) (every row whose band holds k, ascending).
 * ws: ddsp_hip_mel_backward_workspace_bytes(B, T, n_fft, hop) bytes (each frame's gradient; 0 for an unsupported
 * configuration).  No atomics: the same bits on every call.  Supported: n_fft == 2048, hop == 512, n_mels <= 1016,
 * B <= 65535 (DDSP_HIP_ESHAPE otherwise); DDSP_HIP_EWS for a short or NULL workspace. */
size_t ddsp_hip_mel_backward_workspace_bytes(int B, int T, int n_fft, int hop);
int ddsp_hip_mel_spectrogram_backward(const float* audio, int B, int T, const float* window, int n_fft, int hop,
                                      const float* mel_basis, const int* band, const float* band_weights,
                                      int n_band_weights, const int* bin_filters, int n_mels, float clip_val,
                                      const float* grad_out, long stride_b, long stride_mel, long stride_frame,
                                      float* grad_audio, void* ws, size_t ws_bytes, void* stream);

/* STFT.get_mel(y, keyshift, speed, center) in full (nvSTFT.py:73-117; the cascade's formant shift, main_diff.py:359; the
 * pitch augmentation of preprocess.py:88-92), and any (n_fft, win, hop) configuration:
 *   n_fft_new = round(n_fft 2^(keyshift/12)), win_new = round(win 2^(keyshift/12)), hop_new = round(hop speed) (:83-85);
 *   manual padding from (win_new, hop_new) (:97-103); center != 0: torch.stft's reflect padding of n_fft_new/2 on top;
 *   frames of n_fft_new every hop_new, periodic Hann of win_new centred in them; the first min(n_bins, n_fft_new/2 + 1)
 *   bins of the n_fft_new-point DFT -- ANY integer length, a chirp-z transform -- sqrt(re^2+im^2+1e-9) (:108), the bins
 *   above them zero, all times mag_scale (the caller passes win / win_new when keyshift != 0, else 1, :109-114);
 *   mel basis [n_mels, n_bins] as band / band_weights (see above; always read from band_weights); log(clamp(., clip_val)).
 * tables: ddsp_hip_mel_shifted_table_bytes(n_fft_new, n_bins) bytes filled once per (n_fft_new, win_new, n_bins) by
 * ddsp_hip_mel_shifted_tables (the caller caches them per keyshift, as the reference caches its windows, :92-94).
 * Supported: n_bins <= 1025 (n_fft <= 2048); n_fft_new <= 8192 (<= 4096 when min(n_bins, n_fft_new/2 + 1) <= 513: the
 * 2048-point convolution plan); win_new <= n_fft_new, hop_new <= win_new: _table_bytes returns 0 outside.
 * One convolution of 4096 (2048) points per frame up to n_fft_new = 4096 (2048), two beyond.  _frames: the frame count, or
 * DDSP_HIP_EINVAL where torch.stft / F.pad raise (transform longer than the padded signal, center's reflection not
 * shorter than it). */
size_t ddsp_hip_mel_shifted_table_bytes(int n_fft_new, int n_bins);
int ddsp_hip_mel_shifted_tables(int n_fft_new, int win_new, int n_bins, float* tables, void* stream);
int ddsp_hip_mel_shifted_frames(int T, int n_fft_new, int win_new, int hop_new, int center);
int ddsp_hip_mel_shifted_spectrogram(const float* audio, int B, int T, const float* tables, int n_fft_new, int win_new,
                                     int hop_new, int center, int n_bins, float mag_scale, const int* band,
                                     const float* band_weights, int n_mels, float clip_val,
                                     float* out, long stride_b, long stride_mel, long stride_frame, void* stream);

/* ---- harmonic source of NSF-HiFiGAN (nsf_hifigan/models.py:101-204) ---- */

/* SourceModuleHnNSF.forward(f0, upp) = tanh(Linear(SineGen(f0, upp))) with SineGen's two random draws supplied:
 * rand_ini[dim] (initial phase per harmonic, entry 0 must be 0, models.py:150-152) and noise[B, L*upp, dim]
 * (standard normal, models.py:168).  f0[B,L] (0 = unvoiced); weight[dim], bias[1] of the 9 -> 1 linear layer;
 * rad_acc[B,L] scratch; out[B, L*upp].  dim = harmonic_num + 1; supported: 9 (the shipped vocoders) and 1. */
int ddsp_hip_sine_source(const float* f0, int B, int L, int upp, double sr, const float* rand_ini,
                         const float* noise, const float* weight, const float* bias, int dim, float sine_amp,
                         float noise_std, float voiced_threshold, float* rad_acc, float* out, void* stream);

/* The same with the standard-normal noise of models.py:168 (torch.randn_like(sine_waves): [B, L*upp, dim] values, 0.5 GB at
 * B = 32 x 10 s, 1.0 GB at B = 64) DRAWN INSIDE the kernel instead of read: opt-in, a Philox4x32-10 / Box-Muller stream of its
 * own keyed by (noise_seed, noise_offset) -- reproducible, independent of launch geometry, not torch.randn's numbers for a
 * seed.  noise_offset < 2^62, L*upp < 2^32.  ddsp_hip_normal_noise writes the same numbers out as z[B, T, dim]. */
int ddsp_hip_sine_source_drawn(const float* f0, int B, int L, int upp, double sr, const float* rand_ini,
                               unsigned long long noise_seed, unsigned long long noise_offset, const float* weight,
                               const float* bias, int dim, float sine_amp, float noise_std, float voiced_threshold,
                               float* rad_acc, float* out, void* stream);
int ddsp_hip_normal_noise(unsigned long long seed, unsigned long long offset, int B, long T, int dim, float* out,
                          void* stream);

/* ---- spectral loss of the training loop (ddsp/loss.py:9-54) ---- */

/* SSSLoss.forward behind the STFT (loss.py:22-31).  spec_true / spec_pred: the complex STFTs of the two signals
 * (interleaved re, im; any dense layout with the utterance outermost, the SAME layout for both),
 * bins_per_utterance complex values each; S = |X| inv_window_norm + eps (Spectrogram(power=1, normalized=True),
 * loss.py:20); loss[0] = mean_b ||St - Sp||_F / ||St + Sp||_F + alpha mean |log St - log Sp|.  norms[B][2]
 * receives the two Frobenius norms per utterance (input of the backward call); scratch of
 * ddsp_hip_spectral_loss_scratch_bytes(B, bins_per_utterance) bytes.  RSSLoss (loss.py:34-54) calls this once per
 * randomly drawn transform size. */
size_t ddsp_hip_spectral_loss_scratch_bytes(int B, long bins_per_utterance);
int ddsp_hip_spectral_loss(const float* spec_true, const float* spec_pred, int B, long bins_per_utterance,
                           float inv_window_norm, float eps, float alpha, void* scratch, size_t scratch_bytes,
                           float* norms, float* loss, void* stream);
/* d loss / d spec (complex: dRe + i dIm, interleaved, same layout) of the predicted (wrt_true = 0) or the true
 * (1) spectrum, times the upstream gradient grad_out[0] (device scalar). */
int ddsp_hip_spectral_loss_backward(const float* spec_true, const float* spec_pred, int B, long bins_per_utterance,
                                    const float* norms, float inv_window_norm, float eps, float alpha,
                                    const float* grad_out, int wrt_true, float* d_spec, void* stream);

/* The same loss straight from the waveforms, the STFT of Spectrogram(n_fft, hop_length = hop, power = 1,
 * normalized = True, center = False) (loss.py:20) inside the kernel: a chirp-z transform of ANY size
 * 2 <= n_fft <= 2048 (RSSLoss draws them at random, loss.py:47; most have large prime factors), both signals in one
 * complex transform.  tables: ddsp_hip_stft_loss_table_bytes(n_fft) bytes (0: size not supported), filled once per
 * size and device by ddsp_hip_stft_loss_tables.  x_true / x_pred: [B, T] float32 with row stride ld; frames =
 * ddsp_hip_stft_loss_frames(T, n_fft, hop) = 1 + (T - n_fft) / hop (0: signal shorter than one frame).  spec_true /
 * spec_pred receive the complex spectra as [B, frames, n_fft / 2 + 1] (interleaved; the backward call reads them),
 * norms[B][2] and loss[0] as ddsp_hip_spectral_loss.  inv_window_norm = 1 / ||hann(n_fft)||_2. */
size_t ddsp_hip_stft_loss_table_bytes(int n_fft);
int ddsp_hip_stft_loss_tables(int n_fft, float* tables, void* stream);
int ddsp_hip_stft_loss_frames(int T, int n_fft, int hop);
size_t ddsp_hip_stft_loss_scratch_bytes(int B, int T, int n_fft, int hop);
int ddsp_hip_stft_loss(const float* x_true, const float* x_pred, int B, int T, long ld, int n_fft, int hop,
                       const float* tables, float inv_window_norm, float eps, float alpha, void* scratch,
                       size_t scratch_bytes, float* spec_true, float* spec_pred, float* norms, float* loss, void* stream);
/* d loss / d x_pred (wrt_true = 0) or d x_true (1), times grad_out[0]: d_x[B, T] with row stride ld_dx, every sample written
 * (those no frame reaches with 0); accumulate != 0: added to what d_x holds instead (the scales of RSSLoss summed without
 * a temporary each).  hop == n_fft (overlap = 0, the configuration of RSSLoss, loss.py:40): no workspace.  hop < n_fft
 * (overlapping frames): ws of ddsp_hip_stft_loss_backward_ws_bytes(B, T, n_fft, hop) bytes, 16-byte aligned, receives the
 * frames' gradients, which a second kernel gathers per sample in ascending frame order (reproducible). */
size_t ddsp_hip_stft_loss_backward_ws_bytes(int B, int T, int n_fft, int hop);
int ddsp_hip_stft_loss_backward(const float* spec_true, const float* spec_pred, int B, int T, int n_fft, int hop,
                                const float* tables, const float* norms, float inv_window_norm, float eps, float alpha,
                                const float* grad_out, int wrt_true, float* d_x, long ld_dx, int accumulate, void* ws,
                                size_t ws_bytes, void* stream);

/* The real-time caller's splice of consecutive output blocks (gui.py:431-456).  These three entry points came after version 165
 * without a version step: a caller that must run against older builds looks them up by name (dlsym) before use.
 * Per utterance b of B:
 * seg = audio[b, L - (Bf + C + S + D) : L - D]; shift = the first argmax over s = 0 .. S of
 * sum_j seg[s + j] buf_in[b, j] / sqrt(sum_j seg[s + j]^2 + 1e-8) (j < C, float64 sums); tmp = seg[shift : shift + Bf + C];
 * tmp[:C] = tmp[:C] * fade_in + buf_in[b] * fade_out (two float32 roundings, the torch chain's), or with use_pv
 * phase_vocoder(buf_in[b], tmp[:C], fade_out, fade_in) (gui.py:15-32: float64 sums of float32 twiddles and cosines, the phase
 * arguments reduced exactly in integers);
 * out[b] = tmp[:Bf], buf_out[b] = tmp[Bf:] (after the crossfade: with Bf < C it holds crossfaded samples), shift[b] (int64).
 * audio row stride ld >= L >= Bf + C + S + D; Bf >= 1, D >= 1 (DDSP_HIP_EINVAL); 1 <= C <= 16384, 0 <= S <= 4096
 * (DDSP_HIP_ESHAPE otherwise).  buf_in and buf_out are distinct [B, C] buffers: a session ping-pongs them.  2 launches, 3 with
 * use_pv; no synchronisation (the shift never reaches the host).  ws: ddsp_hip_splice_workspace_bytes(B, C, use_pv) bytes,
 * 16-byte aligned. */
size_t ddsp_hip_splice_workspace_bytes(int B, int C, int use_pv);
int ddsp_hip_sola_splice(const float* audio, long ld, int B, long L, int Bf, int C, int S, int D, const float* buf_in,
                         float* buf_out, const float* fade_in, const float* fade_out, int use_pv, float* out, long long* shift,
                         void* ws, size_t ws_bytes, void* stream);
/* gui.py:15-32 on its own: out[n] = phase_vocoder(a, b, fade_out, fade_in), 1 <= n <= 16384 (2 launches; out may be b).
 * ws: ddsp_hip_splice_workspace_bytes(1, n, 1) bytes, 16-byte aligned. */
int ddsp_hip_phase_vocoder(const float* a, const float* b, const float* fade_out, const float* fade_in, int n, float* out,
                           void* ws, size_t ws_bytes, void* stream);

/* Band-limited resampling, torchaudio's sinc resample (torchaudio.functional.resample / transforms.Resample: F.pad(x, (w, w + o))
 * then conv1d with the [n, 1, K] bank at stride o, the blocks interleaved and cut to T = ceil(n L / o)).  These three entry points
 * came after version 165 without a version step: a caller that must run against older builds looks them up by name (dlsym)
 * before use.  orig / new_ are the REDUCED rates o = orig_freq / gcd, n = new_freq / gcd (1 .. 4096), K = 2 width + o.
 * ddsp_hip_resample_table_bytes: host bank [n, K] float32 (host memory) -> the bytes of its table; 0 when the rates are out of
 * range or a tile of 32 phases has a live band (taps that are not exactly 0.0f) wider than 65 536 taps.
 * ddsp_hip_resample_table: writes that table into HOST memory (the caller copies it to the device once and keeps it);
 * DDSP_HIP_ESHAPE out of range, DDSP_HIP_EWS short.  Only the band of live taps is kept: the result differs from the full
 * convolution by the order of the sums alone (for finite input).
 * ddsp_hip_resample: y[b ldy + t] = sum_k xpad_b[q o + k] bank[j, k], t = q n + j < T, xpad_b[p] = x[b ldx + (p - width) sx]
 * inside [0, L) and 0 outside, for b < B.  B >= 1, L >= 0 (T = 0: nothing is launched), sx >= 0 and ldx >= 0 (0: an expanded
 * input, every element read from the same address), ldy >= T when B > 1
 * (DDSP_HIP_EINVAL otherwise); table: the device copy, 16-byte aligned.  f32 MFMA, one launch per 65 535 utterances; no
 * allocation, no synchronisation.  table must be the device copy of what ddsp_hip_resample_table wrote for the same orig,
 * new_ and K = 2 width + orig, whole (table_bytes as ddsp_hip_resample_table_bytes gave it): the host cannot read the device
 * copy, so only its header size is checked here.  The kernel compares the table's header with (orig, new_, K) and, when they
 * differ, reads no tap and writes NaN to every output instead. */
size_t ddsp_hip_resample_table_bytes(const float* bank, int orig, int new_, int K);
int ddsp_hip_resample_table(const float* bank, int orig, int new_, int K, void* table, size_t table_bytes);
int ddsp_hip_resample(const float* x, long ldx, long sx, int B, long L, float* y, long ldy, const void* table,
                      size_t table_bytes, int orig, int new_, int width, void* stream);

/* The frame features of the real-time path and the silence gate between them (ddsp/vocoder.py:104-157, gui.py:114-118 and :134,
 * encoder/rmvpe/utils.py:106-121, ddsp/core.py:8-45).  These entry points came after version 165 without a version step: a caller
 * that must run against older builds looks them up by name (dlsym) before use.  One launch each on the caller's stream, no
 * allocation, no synchronisation.  Rows of a [B, n] argument are `ld` floats apart (ld >= n when B > 1); outputs without a stride
 * are contiguous.  B = 0 is a no-op.
 *
 * ddsp_hip_volume: volume[b, f] = sqrt(mean(pad(audio[b]^2)[f hop : (f + 1) hop])), f < F = T / hop + 1, the pad numpy's `reflect`
 * by (hop / 2, (hop + 1) / 2); float64 sums of the exact squares, one rounding to float32.  T <= (hop + 1) / 2: DDSP_HIP_ESHAPE.
 *
 * ddsp_hip_gate: out[b, i] = signal[b, i] * m, i < F block, m = mask[f] + (mask[f + 1] - mask[f]) r / block (f = i / block,
 * r = i mod block, mask[F] = mask[F - 1]: ddsp/core.py upsample), mask[f] = max over |g - f| <= dilate (edge frames repeated) of
 * volume[b, g] > threshold.  threshold is LINEAR and already float32 -- (float)10^(dB / 20) -- and the comparison is a float32
 * one.  Where mask[f] = mask[f + 1] the product is exact; on a ramp it is rounded once from float64.  out may be signal.
 * 0 <= dilate <= 64 (DDSP_HIP_ESHAPE).
 *
 * ddsp_hip_decode_salience: hidden [rows, 360] -> f0 [rows] (to_local_average_f0): c = the first argmax of the row, or center[row]
 * (int64) when center is not null; the mean of 20 i + 1997.3794084376191 cents over i in [c - 4, c + 5) clipped to [0, 360),
 * weighted by hidden (float64 sums; 0 cents when the weights sum to 0); f0 = 10 * 2^(cents / 1200), 0 where the row maximum
 * is < thred (a float32 comparison).
 *
 * ddsp_hip_f0_track: f0_src [B, N] on a grid of src_period seconds -> out [B, n_frames] on a grid of hop / sample_rate seconds
 * behind start_frame zeros (F0_Extractor.extract).  Zeros are unvoiced.  DDSP_HIP_TRACK_LINEAR: unvoiced frames of a row that has
 * a voiced one are filled by linear interpolation between the nearest voiced neighbours (edges held) and stored as float32; the
 * fill and the unvoiced flag are retimed with np.interp's arithmetic in float64 (source times src_period * i, target times
 * (hop / sample_rate) * k, slope * (x - xp[j]) + fp[j]; the last value held past the end) and the track is 0 where the retimed
 * flag is > 0.5.  DDSP_HIP_TRACK_NEAREST: out = f0_src[min(rint(k hop / sample_rate / src_period), N - 1)], no fill.  With
 * uv_interp the zeros of the result (the prefix included) are filled the same way in float64 and everything below f0_min is
 * raised to it (an all-unvoiced row becomes f0_min).  One workgroup per row; N, n_frames <= 2^30.
 * ws: ddsp_hip_f0_track_workspace_bytes(B, N, n_frames) bytes, 16-byte aligned (DDSP_HIP_EWS when short).
 *
 * ddsp_hip_pool1d: MaskedAvgPool1d (median = 0: the mean of the values that are not NaN, 0 when there is none; float64 sum) or
 * MedianPool1d (median = 1: element (k - 1) / 2 of the sorted window, NaN last) of x [B, N] over k samples, reflect-padded by
 * ((k - 1) / 2, k / 2).  1 <= k <= 16 and N > k / 2 (DDSP_HIP_ESHAPE); y must not be x. */
#define DDSP_HIP_TRACK_LINEAR   0
#define DDSP_HIP_TRACK_NEAREST  1
int ddsp_hip_volume(const float* audio, long ld, int B, long T, int hop, float* volume, void* stream);
int ddsp_hip_gate(const float* signal, long ld_signal, const float* volume, int B, long F, int block, float threshold, int dilate,
                  float* out, long ld_out, void* stream);
int ddsp_hip_decode_salience(const float* hidden, long rows, const long long* center, float thred, float* f0, void* stream);
size_t ddsp_hip_f0_track_workspace_bytes(int B, long N, long n_frames);
int ddsp_hip_f0_track(const float* f0_src, long ld, int B, long N, double src_period, double hop, double sample_rate,
                      long n_frames, long start_frame, int mode, int uv_interp, double f0_min, float* out, void* ws,
                      size_t ws_bytes, void* stream);
int ddsp_hip_pool1d(const float* x, int B, long N, int k, int median, float* y, void* stream);

/* NSF-HiFiGAN's ResBlock1 (nsf_hifigan/models.py:37-68) and the sum over the blocks of a stage (models.py:253-259), csrc/resblock.h.
 * These entry points came after version 165 without a version step: a caller that must run against older builds looks them up
 * by name (dlsym) before use.  C in {16, 32, 64}, k in {3, 7, 11} (DDSP_HIP_ESHAPE otherwise), x and y [B, C, T] contiguous.
 *
 * ddsp_hip_resblock1_tile: output columns per workgroup, 128 - (k - 1); 0 for a (C, k) the kernel does not take.
 * ddsp_hip_resblock1_pack_bytes / _pack: HOST weights w [2 pairs][C][C][k] in the order convs1[0], convs2[0], convs1[1], ... and
 * biases b [2 pairs][C] -> the table the kernel reads, written to HOST memory (the caller copies it to the device once and
 * keeps it); 1 <= pairs <= 8.  0 bytes / DDSP_HIP_ESHAPE out of range, DDSP_HIP_EWS short.
 * ddsp_hip_resblock1: for p < pairs, x <- conv1d(lrelu(conv1d(lrelu(x), w1_p, b1_p, dilation d_p)), w2_p, b2_p) + x with slope
 * 0.1 and "same" zero padding of each conv's own input; then y = (acc_in + x) / scale: acc_in may be null (nothing added) or y
 * itself, scale = 0 means no division (otherwise an IEEE division, as the reference's xs / num_kernels).  dilations: host ints,
 * each >= 1 (DDSP_HIP_EINVAL) and small enough for the tile's input to fit in 64 KB of LDS: C (16 + 32 ceil((112 + (k - 1) d) / 32))
 * <= 16384, i.e. d <= 11 at C = 64, k = 11 and more everywhere else (DDSP_HIP_ESHAPE).  T >= 1 (DDSP_HIP_EINVAL); B = 0 is a
 * no-op.  One launch per pair (per 65 535 utterances), f32 MFMA, the intermediate of a pair stays in LDS; the pairs hand over
 * through ws: ddsp_hip_resblock1_workspace_bytes(B, C, T, pairs) bytes (0 for one pair; DDSP_HIP_EWS when short).  x must not be
 * y or acc_in.  No allocation, no synchronisation. */
int ddsp_hip_resblock1_tile(int C, int k);
size_t ddsp_hip_resblock1_pack_bytes(int C, int k, int pairs);
int ddsp_hip_resblock1_pack(const float* w, const float* b, int C, int k, int pairs, void* packed, size_t packed_bytes);
size_t ddsp_hip_resblock1_workspace_bytes(int B, int C, long T, int pairs);
int ddsp_hip_resblock1(const float* x, float* y, const void* packed, size_t packed_bytes, int B, int C, long T, int k,
                       const int* dilations, int pairs, const float* acc_in, float scale, void* ws, size_t ws_bytes,
                       void* stream);

/* The wide form of the above, csrc/resblock_wide.h: C in {128, 256}, k in {3, 7, 11} (DDSP_HIP_ESHAPE otherwise, C = 64 included:
 * the entries above keep what they take and refuse).  Looked up by name like them; ddsp_hip_version() stays 165.  Same
 * arguments, same result, same codes.  One convolution per launch, two launches per pair (per 65 535 utterances), f32 MFMA; the
 * input channels pass through LDS in chunks of 64, each chunk one summation chain, the chunks' partial sums added in order.
 *
 * ddsp_hip_resblock1_wide_tile: output columns per workgroup, 128 for every k; 0 for a (C, k) this form does not take.
 * ddsp_hip_resblock1_wide_pack_bytes / _pack: as ddsp_hip_resblock1_pack, same sizes (2 C C k + 2 C floats per pair), the
 * fragments ordered per (64-row output slice, 64-channel chunk).  A table of one form is not the other's.
 * ddsp_hip_resblock1_wide: dilations each >= 1 (DDSP_HIP_EINVAL) and small enough for a chunk's input to fit in 64 KB of LDS:
 * 64 (16 + 32 ceil((112 + (k - 1) d) / 32)) <= 16384, i.e. d <= 11 at k = 11, 18 at k = 7, 56 at k = 3 (DDSP_HIP_ESHAPE).
 * ws: ddsp_hip_resblock1_wide_workspace_bytes(B, C, T, pairs) bytes, never 0: the intermediate of a pair and the hand-over
 * between pairs, min(pairs, 3) activations [B, C, T] (DDSP_HIP_EWS when short or null).  x must not be y or acc_in; acc_in
 * may be y.  Row b of the result does not depend on B.  No allocation, no synchronisation. */
int ddsp_hip_resblock1_wide_tile(int C, int k);
size_t ddsp_hip_resblock1_wide_pack_bytes(int C, int k, int pairs);
int ddsp_hip_resblock1_wide_pack(const float* w, const float* b, int C, int k, int pairs, void* packed, size_t packed_bytes);
size_t ddsp_hip_resblock1_wide_workspace_bytes(int B, int C, long T, int pairs);
int ddsp_hip_resblock1_wide(const float* x, float* y, const void* packed, size_t packed_bytes, int B, int C, long T, int k,
                            const int* dilations, int pairs, const float* acc_in, float scale, void* ws, size_t ws_bytes,
                            void* stream);

/* The rest of the NSF-HiFiGAN generator between the 128-channel stage and the waveform (nsf_hifigan/models.py:249-252, :260-262),
 * csrc/generator_tail.h.  As above, these entry points came after version 165 without a version step.
 *
 * The upsampling seam of a stage:
 *   y[b, co, t] = bu[co] + sum over (ci, j) of lrelu_0.1(x)[b, ci, q] Wu[ci, co, j] over t = u q - u / 2 + j   (ConvTranspose1d(2 Cout,
 *                 Cout, 2 u, u, padding u / 2))  + bn[co] + sum over m of src[b, t s - s / 2 + m] Wn[co, 0, m]   (Conv1d(1, Cout, 2 s,
 *                 s, padding s / 2), or Conv1d(1, Cout, 1) at s = 1), zeros outside both inputs.
 * Cout in {16, 32, 64}, u in {2, 4, 8}, s in {1, 2, 4} (DDSP_HIP_ESHAPE otherwise); x [B, 2 Cout, Tin], src [B, s u Tin],
 * y [B, Cout, u Tin], all contiguous; 1 <= Tin <= 2^30.
 * ddsp_hip_upsample_stage_tile: input columns per workgroup (128, or 64 at Cout = 64, u = 8); 0 for a (Cout, u) outside the range.
 * ddsp_hip_upsample_stage_pack_bytes / _pack: HOST weights wu [2 Cout][Cout][2 u] (ConvTranspose1d's order: input channel
 * first), bu [Cout], wn [Cout][1][2 s] ([Cout][1][1] at s = 1), bn [Cout] -> the table the kernel reads, written to HOST memory
 * (the caller copies it to the device once and keeps it).  0 bytes / DDSP_HIP_ESHAPE out of range, DDSP_HIP_EWS short.
 * ddsp_hip_upsample_stage: one launch (per 65 535 utterances), the transposed convolution as u polyphase f32 MFMA GEMMs, the
 * noise convolution and the add in the same launch.  y must be neither x nor src.  B = 0 is a no-op.
 *
 * The output head: y[b, 0, t] = tanh(bias + sum over (ci, j < 7) of lrelu_slope(x)[b, ci, t + j - 3] w[0, ci, j]), zeros outside
 * [0, T); C in {16, 32, 64} (DDSP_HIP_ESHAPE otherwise), x [B, C, T], y [B, 1, T], w [1][C][7] and bias [1] DEVICE memory (the
 * Conv1d's own parameters), slope finite (the reference's F.leaky_relu default is 0.01).  ddsp_hip_output_head_tile: outputs
 * per workgroup (1024), 0 for another C.  One launch (per 65 535 utterances); x must not be y; B = 0 is a no-op.
 * Neither allocates nor synchronises. */
int ddsp_hip_upsample_stage_tile(int Cout, int u);
size_t ddsp_hip_upsample_stage_pack_bytes(int Cout, int u, int s);
int ddsp_hip_upsample_stage_pack(const float* wu, const float* bu, const float* wn, const float* bn, int Cout, int u, int s,
                                 void* packed, size_t packed_bytes);
int ddsp_hip_upsample_stage(const float* x, const float* src, float* y, const void* packed, size_t packed_bytes, int B, int Cout,
                            long Tin, int u, int s, void* stream);
int ddsp_hip_output_head_tile(int C);
int ddsp_hip_output_head(const float* x, const float* w, const float* bias, float slope, float* y, int B, int C, long T,
                         void* stream);

/* The conformer conv module of Unit2Control's decoder and of every PCmer layer (diffusion/model_conformer_naive.py:117-150, the
 * same text in reflow/, ddsp/pcmer.py:189-216), csrc/conformer_conv.h.  As above, these entry points came after version 165
 * without a version step.
 *   net(x) = Conv1d(2 D, D, 1)(silu(Conv1d(2 D, 2 D, 31, padding 15, groups 2 D)(glu(Conv1d(D, 4 D, 1)(ln(x))))))
 * over x [B, L, D] contiguous (the module's own layout: no transposed copy), ln an optional LayerNorm(D) with the given eps, glu
 * = rows [0, 2 D) times the sigmoid of rows [2 D, 4 D), the depthwise convolution a cross-correlation that zero-pads the GLU's
 * output.  D = 256 (DDSP_HIP_ESHAPE otherwise), float32, forward only.
 * ddsp_hip_conformer_conv_tile: output frames per workgroup (98); 0 for a D the kernel does not take.
 * ddsp_hip_conformer_conv_pack_bytes / _pack: HOST weights w1 [4 D][D], b1 [4 D], wd [2 D][31], bd [2 D], w2 [D][2 D], b2 [D] and
 * gamma, beta [D] (both null: no LayerNorm) -> the table the kernel reads, written to HOST memory (the caller copies it to the
 * device once and keeps it).  0 bytes / DDSP_HIP_ESHAPE out of range, DDSP_HIP_EWS short.
 * ddsp_hip_conformer_conv: y = net(x), or x + net(x) with add_input (the un-normalised x); norm != 0 needs a table packed with
 * gamma and beta (DDSP_HIP_EWS otherwise).  1 <= L <= 2^40 (DDSP_HIP_EINVAL / DDSP_HIP_ESHAPE); x and y 16-byte aligned; x must
 * not be y (a tile reads its neighbours' frames: DDSP_HIP_EINVAL); B = 0 is a no-op.  One launch (per 65 535 utterances), f32
 * MFMA, 150.5 KB of LDS per workgroup.  No workspace, no allocation, no synchronisation. */
int ddsp_hip_conformer_conv_tile(int D);
size_t ddsp_hip_conformer_conv_pack_bytes(int D, int norm);
int ddsp_hip_conformer_conv_pack(const float* w1, const float* b1, const float* wd, const float* bd, const float* w2, const float* b2,
                                 const float* gamma, const float* beta, int D, void* packed, size_t packed_bytes);
int ddsp_hip_conformer_conv(const float* x, float* y, const void* packed, size_t packed_bytes, int B, long L, int D, int norm,
                            float eps, int add_input, void* stream);

/* The same module in its channel-split form, csrc/conformer_split.h, for calls of a few hundred frames: a frame tile of 16, the
 * channels split over workgroups and waves, three plain launches on the stream (the LayerNorm, first GEMM and GLU; the stencil and
 * SiLU; the output GEMM and residual), every sum in the order of ddsp_hip_conformer_conv and the LayerNorm and sigmoid its own
 * code, so the two give the same bits.  It reads the table of ddsp_hip_conformer_conv_pack.  As above, these entry points came
 * after version 165 without a version step.
 * ddsp_hip_conformer_conv_split_tile: frames per workgroup (16); 0 for a D the kernels do not take.
 * ddsp_hip_conformer_conv_split_workspace_bytes: 4 B L D floats (g and h [B, 2 D, L]); 0 for arguments the call below refuses.
 * ddsp_hip_conformer_conv_split: the arguments, checks and error codes of ddsp_hip_conformer_conv, a workspace (null or
 * misaligned: DDSP_HIP_EINVAL, short: DDSP_HIP_EWS) and B ceil(L / 16) <= 4096 (DDSP_HIP_ESHAPE beyond: the tiled form is for the
 * rest).  16.5 KB of LDS in the first launch.  No allocation, no synchronisation. */
int ddsp_hip_conformer_conv_split_tile(int D);
size_t ddsp_hip_conformer_conv_split_workspace_bytes(long B, long L, int D);
int ddsp_hip_conformer_conv_split(const float* x, float* y, const void* packed, size_t packed_bytes, void* ws, size_t ws_bytes, int B,
                                  long L, int D, int norm, float eps, int add_input, void* stream);

/* The residual layer of the diffusion denoiser's WaveNet (diffusion/wavenet.py:31-61, ResidualBlock with dilation 1),
 * csrc/wavenet_layer.h.  As above, these entry points came after version 165 without a version step.
 *   z = Conv1d(C, 2 C, 3, padding 1)(x + d) + Conv1d(H, 2 C, 1)(cond);  g = sigmoid(z[:C]) tanh(z[C:]);  o = Conv1d(C, 2 C, 1)(g)
 *   x_out = (x + o[:C]) / sqrt(2);  skip = o[C:]
 * over x [B, C, T], cond [B, H, T], d [B, C] (the layer's projection of the step embedding), x_out and skip [B, C, T], all
 * contiguous float32 with no alignment beyond 4 bytes; the 3-tap convolution is a cross-correlation that zero-pads x + d.
 * (C, H) = (384, 256) or (512, 256) (DDSP_HIP_ESHAPE otherwise), forward only.
 * ddsp_hip_wavenet_layer_tile: frames per workgroup (64); 0 for a (C, H) the kernel does not take.
 * ddsp_hip_wavenet_layer_pack_bytes / _pack: HOST weights wdil [2 C][C][3], bdil [2 C], wc [2 C][H], bc [2 C], wo [2 C][C],
 * bo [2 C] -> the table the kernel reads, written to HOST memory (the caller copies it to the device once and keeps it).
 * 0 bytes / DDSP_HIP_ESHAPE out of range, DDSP_HIP_EWS short.
 * ddsp_hip_wavenet_layer: skip_mode 0 stores the skip rows, 1 adds them to what skip holds (the running sum over the layers
 * of a stack; a tile owns its frames: no atomics).  1 <= T <= 2^40 (DDSP_HIP_EINVAL / DDSP_HIP_ESHAPE); x_out must not be x
 * (a tile reads its neighbours' frames) and skip neither of them (DDSP_HIP_EINVAL); B = 0 is a no-op.  One launch (per 65 535
 * utterances), f32 MFMA, 138 KB of LDS per workgroup at C = 512.  No workspace, no allocation, no synchronisation. */
int ddsp_hip_wavenet_layer_tile(int C, int H);
size_t ddsp_hip_wavenet_layer_pack_bytes(int C, int H);
int ddsp_hip_wavenet_layer_pack(const float* wdil, const float* bdil, const float* wc, const float* bc, const float* wo,
                                const float* bo, int C, int H, void* packed, size_t packed_bytes);
int ddsp_hip_wavenet_layer(const float* x, const float* cond, const float* d, float* x_out, float* skip, const void* packed,
                           size_t packed_bytes, int B, long T, int C, int H, int skip_mode, void* stream);

/* The same layer in its channel-split form, csrc/wavenet_split.h, for calls of a few hundred frames: a frame tile of 16, the
 * channels split over workgroups and waves, two plain launches on the stream (the gate g = sigmoid(z[:C]) tanh(z[C:]) into the
 * workspace, then the output GEMM with the tiled kernel's epilogue), every sum in the order of ddsp_hip_wavenet_layer, so the two
 * give the same bits.  It reads the table of ddsp_hip_wavenet_layer_pack.  As above, these entry points came after version 165
 * without a version step.
 * ddsp_hip_wavenet_layer_split_tile: frames per workgroup (16); 0 for a (C, H) the kernels do not take.
 * ddsp_hip_wavenet_layer_split_workspace_bytes: B T C floats (g [B, C, T]); 0 for C outside the shapes, B < 1, T < 1 and sizes
 * past the cap below.
 * ddsp_hip_wavenet_layer_split: the arguments, checks and error codes of ddsp_hip_wavenet_layer in the same order, and
 * B ceil(T / 16) <= 4096 (DDSP_HIP_ESHAPE beyond, whatever the buffers are: the tiled form is for the rest), ws not null
 * (DDSP_HIP_EINVAL) and of at least the bytes above (DDSP_HIP_EWS); every refusal comes before any launch.  54 KB of LDS per
 * workgroup in the first launch at C = 512.  No allocation, no synchronisation. */
int ddsp_hip_wavenet_layer_split_tile(int C, int H);
size_t ddsp_hip_wavenet_layer_split_workspace_bytes(long B, long T, int C);
int ddsp_hip_wavenet_layer_split(const float* x, const float* cond, const float* d, float* x_out, float* skip, const void* packed,
                                 size_t packed_bytes, void* ws, size_t ws_bytes, int B, long T, int C, int H, int skip_mode,
                                 void* stream);

/* The performer (softmax-kernel linear) attention of PCmer (ddsp/pcmer.py:14-47, 218-232, 297-325), csrc/performer_attention.h.
 * As above, these entry points came after version 165 without a version step.  Per batch item and head, q, k, v [N, d], the
 * projection P [m, d], dn = d^-0.25, ratio = m^-0.5:
 *   (normalize)  q = q / (|q| + 1e-8), k = k / (|k| + 1e-8)
 *   q' = ratio (exp(dn q P^T - |q|^2 dn^2 / 2 - rowmax(dn q P^T)) + 1e-4);  k' = ratio exp(dn k P^T - |k|^2 dn^2 / 2 + 1e-4)
 *   out = (q' (k'^T v)) / (q' . sum_n k' + 1e-8)
 * (d, m) = (64, 266) (DDSP_HIP_ESHAPE otherwise), float32, forward only, no mask.
 * ddsp_hip_performer_tile: frames per workgroup (64); 0 for anything but (64, 266).
 * ddsp_hip_performer_pack_bytes / _pack: the HOST projection [m][d] -> the table the kernels read, written to HOST memory (the
 * caller copies it to the device once and keeps it).  0 bytes / DDSP_HIP_ESHAPE out of range, DDSP_HIP_EWS short.
 * ddsp_hip_performer_chunks: the default number of key chunks: B H chunks workgroups fill 256 CUs, at most ceil(N / tile).
 * ddsp_hip_performer_workspace_bytes: B H min(chunks, ceil(N / tile)) partial blocks of (272 x 64 + 272) floats; 0 for
 * arguments the call below refuses.
 * ddsp_hip_performer_attention: strides is a HOST array of 12 longs, the (batch, head, frame) strides in floats of q, k, v
 * and out, whose d elements are contiguous; strides are non-negative multiples of 4 and the four pointers and ws 16-byte
 * aligned (DDSP_HIP_EINVAL); out must be none of q, k, v.  The three slices of one [B, N, 3 H d] projection result and a
 * [B, N, H d] result can be passed as they are.  1 <= N <= 2^30 and B H ceil(N / tile) < 2^31 (DDSP_HIP_ESHAPE); chunks >= 1, a
 * count above ceil(N / tile) is clamped; B = 0 is a no-op.  Two launches on the stream (keys, then queries), both grids flat
 * in x: no 65 535 limit.  The key partials are added in chunk order: a call is reproducible.  No allocation, no
 * synchronisation. */
int ddsp_hip_performer_tile(int d, int m);
size_t ddsp_hip_performer_pack_bytes(int d, int m);
int ddsp_hip_performer_pack(const float* proj, int d, int m, void* table, size_t table_bytes);
int ddsp_hip_performer_chunks(long B, int H, long N);
size_t ddsp_hip_performer_workspace_bytes(long B, int H, long N, int chunks);
int ddsp_hip_performer_attention(const float* q, const float* k, const float* v, float* out, const long* strides,
                                 const void* table, size_t table_bytes, void* ws, size_t ws_bytes, long B, int H, long N, int d,
                                 int m, int normalize, int chunks, void* stream);

/* The layer of the reflow / diffusion-fast denoiser (reflow/naive_v2_diff.py:81-98, NaiveV2DiffLayer in its default form: no
 * attention, not wavenet_like, a conv module without LayerNorm), csrc/naive_v2_layer.h.  As above, these entry points came after
 * version 165 without a version step.
 *   x' = x + d + Conv1d(Hc, D, 1)(cond);  g = glu(Conv1d(D, 4 D, 1)(x'));  h = silu(Conv1d(2 D, 2 D, 31, padding 15, groups 2 D)(g))
 *   y  = x + Conv1d(2 D, D, 1)(h)
 * over x, y [B, L, D], cond [B, L, Hc] (a frame's channels contiguous) and d [B, D] (the layer's projection of the step
 * embedding), contiguous float32; glu = rows [0, 2 D) times the sigmoid of rows [2 D, 4 D); the depthwise convolution is a
 * cross-correlation that zero-pads g; the residual is the x that came in.  (D, Hc) = (512, 128) (DDSP_HIP_ESHAPE otherwise),
 * forward only.
 * ddsp_hip_naive_v2_layer_tile: frames per workgroup of the first launch (which = 0: 64) or the second (1: 112); 0 for a shape
 * the kernels do not take or another which.
 * ddsp_hip_naive_v2_layer_pack_bytes / _pack: HOST weights wc [D][Hc], bc [D], w1 [4 D][D], b1 [4 D], wd [2 D][31], bd [2 D],
 * w2 [D][2 D], b2 [D] -> the table the kernels read, written to HOST memory (the caller copies it to the device once and keeps
 * it).  0 bytes / DDSP_HIP_ESHAPE out of range, DDSP_HIP_EWS short.
 * ddsp_hip_naive_v2_layer_workspace_bytes: B x 2 D x L floats, where the first launch leaves g for the second; 0 for arguments
 * the call below refuses.
 * ddsp_hip_naive_v2_layer: 1 <= L <= 2^30 (DDSP_HIP_EINVAL / DDSP_HIP_ESHAPE); x, d, y and packed 16-byte aligned; y must be
 * neither x nor cond (DDSP_HIP_EINVAL); a short table or workspace is DDSP_HIP_EWS; B = 0 is a no-op.  Two launches on the
 * stream (per 65 535 utterances), f32 MFMA, 128.5 KB and 36 KB of LDS per workgroup.  No allocation, no synchronisation. */
int ddsp_hip_naive_v2_layer_tile(int D, int Hc, int which);
size_t ddsp_hip_naive_v2_layer_pack_bytes(int D, int Hc);
int ddsp_hip_naive_v2_layer_pack(const float* wc, const float* bc, const float* w1, const float* b1, const float* wd,
                                 const float* bd, const float* w2, const float* b2, int D, int Hc, void* packed,
                                 size_t packed_bytes);
size_t ddsp_hip_naive_v2_layer_workspace_bytes(long B, long L, int D);
int ddsp_hip_naive_v2_layer(const float* x, const float* cond, const float* d, float* y, const void* packed, size_t packed_bytes,
                            void* ws, size_t ws_bytes, int B, long L, int D, int Hc, void* stream);

/* The same layer in its channel-split form, csrc/naive_v2_split.h, for calls of a few hundred frames: a frame tile of 16, the
 * channels split over workgroups and waves, four plain launches on the stream (x', the GLU, the stencil, the output GEMM), every
 * sum in the order of ddsp_hip_naive_v2_layer, so the two give the same bits.  It reads the table of ddsp_hip_naive_v2_layer_pack.
 * As above, these entry points came after version 165 without a version step.
 * ddsp_hip_naive_v2_layer_split_tile: frames per workgroup (16); 0 for a shape the kernels do not take.
 * ddsp_hip_naive_v2_layer_split_workspace_bytes: 5 B L D floats (x' [B, L, D], g and h [B, 2 D, L]); 0 for arguments the call
 * below refuses.
 * ddsp_hip_naive_v2_layer_split: the arguments, checks and error codes of ddsp_hip_naive_v2_layer, and B ceil(L / 16) <= 4096
 * (DDSP_HIP_ESHAPE beyond: the tiled form is for the rest); ws 16-byte aligned.  33 KB of LDS in the second launch.  No
 * allocation, no synchronisation. */
int ddsp_hip_naive_v2_layer_split_tile(int D, int Hc);
size_t ddsp_hip_naive_v2_layer_split_workspace_bytes(long B, long L, int D);
int ddsp_hip_naive_v2_layer_split(const float* x, const float* cond, const float* d, float* y, const void* packed,
                                  size_t packed_bytes, void* ws, size_t ws_bytes, int B, long L, int D, int Hc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDSP_HIP_H */
