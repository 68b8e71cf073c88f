"""ddsp_svc_amd -- MI355X-native DDSP harmonic-plus-noise synthesiser (drop-in for the
Sins/CombSub forward pass of yxlllc/DDSP-SVC).

  core      -- ddsp/core.py functions (upsample, frequency_filter, ...) on HIP kernels
  synth     -- phase state, exciters, fused Sins / CombSub DSP tails
  vocoder   -- nn.Module drop-ins + patch_reference()
  mel       -- nsf_hifigan.nvSTFT.STFT.get_mel (the cascade's waveform -> log-mel front-end)
  nsf_source -- nsf_hifigan.models.SourceModuleHnNSF (SineGen + merge), the vocoder's harmonic source
  nsf_generator -- nsf_hifigan.models.ResBlock1 and the per-stage block sum of Generator.forward: fused f32 MFMA conv pairs
  conformer -- the control network's ConformerConvModule / conv-only CFNEncoderLayer: one fused f32 MFMA launch per module, three in its channel-split form for real-time sizes (the conv-only ConformerNaiveEncoder)
  attention -- PCmer's performer attention (FastAttention / SelfAttention): two fused f32 MFMA launches per call
  wavenet   -- the diffusion denoiser's WaveNet ResidualBlock: one fused f32 MFMA launch per layer, the skip sum in place; two launches in its channel-split form for real-time sizes
  naive_v2  -- the reflow / diffusion-fast denoiser's NaiveV2DiffLayer: two fused f32 MFMA launches per layer, four in its channel-split form for real-time sizes
  loss      -- ddsp/loss.py SSSLoss / RSSLoss (the STFT of any size below 2049 as an in-kernel chirp-z transform, the loss and
               its gradient in the same kernels; torch.stft only above that)
  resample  -- torchaudio's sinc resampling (functional.resample / transforms.Resample) as an f32 MFMA GEMM
  splice    -- the real-time caller's block splice (gui.py:431-456): SOLA search, crossfade, phase vocoder
  features  -- the frame features of the real-time path: volume, silence mask / gate, salience decode, F0 track
  sharding  -- utterance sharding across the GPUs of a node (+ optional RCCL gather)
"""
from . import _ffi, attention, build, conformer, core, features, loss, mel, naive_v2, nsf_generator, nsf_source, resample, splice, synth, wavenet  # noqa: F401

__version__ = "0.1.0"
