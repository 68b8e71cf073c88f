"""The launchers that put the utterance index on the grid's y axis and do NOT split refuse more than 65 535 utterances
(DESIGN.md section 7.6).  Here: every such C entry returns its documented error code for B = 65 536 before any launch (the
pointers are never dereferenced, a sentinel stays as it was), and every Python entry in front of one raises an error that
names the limit instead of handing back a buffer nobody wrote."""
import types

import pytest
import torch

from tests.backends import dev  # noqa: F401

EINVAL, ESHAPE, EWS = -1, -3, -4
BIG = 65536
P = 4096                                                             # never dereferenced: every call below fails its checks first
HUGE = 1 << 40


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_c_abi_refuses_a_batch_past_the_grid_limit(dev):
    from ddsp_svc_amd import _ffi
    lib = _ffi.lib()
    sentinel = torch.full((64,), 7.0)
    out = sentinel.data_ptr()
    assert lib.ddsp_hip_stft_loss_table_bytes(397) > 0               # a transform size the loss kernels' plans cover
    calls = {
        # csrc/sinegen.hip
        "sine_source": lambda B: lib.ddsp_hip_sine_source(P, B, 4, 2, 44100.0, P, P, P, P, 9, 0.1, 0.003, 0.0, P, out, None),
        "sine_source_drawn": lambda B: lib.ddsp_hip_sine_source_drawn(P, B, 4, 2, 44100.0, P, 1, 0, P, P, 9, 0.1, 0.003, 0.0, P,
                                                                      out, None),
        # csrc/loss.hip
        "spectral_loss": lambda B: lib.ddsp_hip_spectral_loss(P, P, B, 40, 1.0, 1e-7, 1.0, P, HUGE, P, out, None),
        "spectral_loss_backward": lambda B: lib.ddsp_hip_spectral_loss_backward(P, P, B, 40, P, 1.0, 1e-7, 1.0, P, 0, out, None),
        # csrc/loss_czt.hip
        "stft_loss": lambda B: lib.ddsp_hip_stft_loss(P, P, B, 800, 800, 397, 397, P, 1.0, 1e-7, 1.0, P, HUGE, P, P, P, out, None),
        "stft_loss_backward": lambda B: lib.ddsp_hip_stft_loss_backward(P, P, B, 800, 397, 100, P, P, 1.0, 1e-7, 1.0, P, 0, out, 800,
                                                                        0, P, HUGE, None),
        # csrc/fir.hip (the simple form) and csrc/fir_bwd_direct.hip (a hop the FFT forms decline)
        "fft_convolve": lambda B: lib.ddsp_hip_fft_convolve(P, 0, P, None, out, None, B, 3, 100, 64, _ffi.FIR_SIMPLE, None),
        "fft_convolve_backward": lambda B: lib.ddsp_hip_fft_convolve_backward(P, 0, P, P, out, P, B, 3, 100, 64, None),
        # csrc/mel.hip
        "mel_spectrogram_backward": lambda B: lib.ddsp_hip_mel_spectrogram_backward(P, B, 512, P, 2048, 512, P, P, P, 100, P, 128,
                                                                                    1e-5, P, 128, 1, 128, out, P, HUGE, None),
        # csrc/splice.h, csrc/frame_features.h
        "sola_splice": lambda B: lib.ddsp_hip_sola_splice(P, 1000, B, 1000, 300, 128, 40, 20, P, 2 * P, P, P, 0, out, P, P, HUGE,
                                                          None),
        "volume": lambda B: lib.ddsp_hip_volume(P, 1000, B, 1000, 512, out, None),
        "gate": lambda B: lib.ddsp_hip_gate(P, 1024, P, B, 2, 512, 0.001, 4, out, 1024, None),
        "pool1d": lambda B: lib.ddsp_hip_pool1d(P, B, 100, 3, 1, out, None),
    }
    for name, call in calls.items():
        assert call(BIG) == ESHAPE, name
        assert call(BIG + 1) == ESHAPE, name
        assert (sentinel == 7.0).all(), name
    # the same arguments with no utterance are the documented no-op (or, for a mean over nothing, an argument error): the
    # refusal above is the batch's, not another argument's
    for name, call in calls.items():
        want = EINVAL if name.startswith(("spectral_loss", "stft_loss")) else 0
        assert call(0) == want, name
    assert (sentinel == 7.0).all()


def _fake_mel_ctx(B):
    from ddsp_svc_amd import mel as M
    stft = M.STFT(44100, 128, 2048, 2048, 512, 40, 16000)
    basis, (band, packed), window = stft._tables(torch.device("cpu"))
    ctx = types.SimpleNamespace(hop=512, clip=1e-5, dtype=torch.float32, needs_input_grad=(True,) + (False,) * 7)
    ctx.saved_tensors = (torch.empty(B, 512), window, basis, band, packed, M._bin_filters(basis))
    return ctx


def _entries():
    from ddsp_svc_amd import _ffi, core, features, loss, mel, nsf_source, splice, synth
    z = torch.zeros
    one = lambda n: z(n) + 1.0
    return {
        "features.volume": lambda B: features.volume(z(B, 8), 4),
        "features.gate": lambda B: features.gate(z(B, 8), z(B, 2), -60.0, 4),
        "core.MedianPool1d": lambda B: core.MedianPool1d(z(B, 8), 3),
        "core.MaskedAvgPool1d": lambda B: core.MaskedAvgPool1d(z(B, 8), 3),
        "nsf_source.sine_source": lambda B: nsf_source.sine_source(one(B * 2).view(B, 2) * 220.0, 2, 44100, one(1), z(1), z(1),
                                                                   z(B, 4, 1)),
        "nsf_source.sine_source drawn": lambda B: nsf_source.sine_source(one(B * 2).view(B, 2) * 220.0, 2, 44100, one(1), z(1), z(1),
                                                                         None, noise_seed=1),
        "splice.sola_splice": lambda B: splice.sola_splice(z(B, 30), z(B, 8), one(8), z(8), 16, 8, 4, 2),
        "loss.SSSLoss": lambda B: loss.SSSLoss(8)(one(B * 16).view(B, 16), z(B, 16)),
        "loss.SSSLoss overlapping": lambda B: loss.SSSLoss(8, overlap=0.5)(one(B * 16).view(B, 16), z(B, 16)),
        "core.fft_convolve simple": lambda B: core.fft_convolve(z(B, 8), z(B, 2, 4), impl=_ffi.FIR_SIMPLE),
        "core.fft_convolve_backward": lambda B: core.fft_convolve_backward(z(B, 8), z(B, 8), z(B, 2, 4)),
        "synth._fir_bwd": lambda B: synth._fir_bwd(z(B, 8), 0, z(B, 2, 4), z(B, 8), True),
        "mel get_mel backward": lambda B: mel._MelSpectrogram.backward(_fake_mel_ctx(B), torch.empty(B, 128, 1)),
    }


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
@pytest.mark.parametrize("entry", ["features.volume", "features.gate", "core.MedianPool1d", "core.MaskedAvgPool1d",
                                   "nsf_source.sine_source", "nsf_source.sine_source drawn", "splice.sola_splice", "loss.SSSLoss",
                                   "loss.SSSLoss overlapping", "core.fft_convolve simple", "core.fft_convolve_backward",
                                   "synth._fir_bwd", "mel get_mel backward"])
def test_python_entry_names_the_limit(dev, entry):
    """65 536 utterances of a handful of samples: the entry raises before anything is launched and says what the limit is"""
    with pytest.raises(ValueError, match="at most 65535 utterances"):
        _entries()[entry](BIG)


@pytest.mark.parametrize("dev", ["emu"], indirect=True)
def test_other_shape_errors_keep_their_message(dev):
    """the limit is named only when the batch is over it"""
    from ddsp_svc_amd import _ffi, core
    with pytest.raises(RuntimeError, match="shape") as e:
        _ffi.check(ESHAPE, batch=3)
    assert "65535" not in str(e.value)
    with pytest.raises(RuntimeError):
        _ffi.check(ESHAPE)
    _ffi.check(0, batch=BIG)
    assert core.MedianPool1d(torch.arange(12, dtype=torch.float32).view(2, 6), 3).shape == (2, 6)
