"""Stand-ins with the module trees of the reference's ``naive_v2_diff`` ``NaiveV2DiffLayer`` and ``NaiveV2Diff``.  Their
``forward`` is the package's dispatcher, as the reference's classes have it after ``patch_reference_naive_v2()``;
``reference_forward`` is the reference's own op chain, restated.  The conv module inside is a plain chain (it never dispatches
for itself: this file is about the layer)."""
import math

import torch
import torch.nn.functional as F
from torch import nn

from ddsp_svc_amd import naive_v2 as NV


class Transpose(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.dims = dims

    def forward(self, x):
        return x.transpose(*self.dims)


class ConvModule(nn.Module):
    def __init__(self, dim, dropout=0.0, use_norm=False, taps=31):
        super().__init__()
        inner = 2 * dim
        self.net = nn.Sequential(nn.LayerNorm(dim) if use_norm else nn.Identity(), Transpose((1, 2)),
                                 nn.Conv1d(dim, 2 * inner, 1), nn.GLU(dim=1),
                                 nn.Conv1d(inner, inner, taps, padding=taps // 2, groups=inner), nn.SiLU(),
                                 nn.Conv1d(inner, dim, 1), Transpose((1, 2)), nn.Dropout(dropout))

    def forward(self, x):
        return self.net(x)


class ScaleAttn(nn.Module):
    """any function of x stands in for the attention half"""

    def forward(self, x):
        return 0.5 * x


class DiffLayer(nn.Module):
    def __init__(self, dim_model, dim_cond, attn=None, wavenet_like=False, **conv):
        super().__init__()
        self.conformer = ConvModule(dim_model, **conv)
        self.norm = nn.LayerNorm(dim_model)
        self.dropout = nn.Dropout(0.1)                 # the reference keeps one it never calls
        self.wavenet_like_proj = nn.Conv1d(dim_model, 2 * dim_model, 1) if wavenet_like else None
        self.diffusion_step_projection = nn.Conv1d(dim_model, dim_model, 1)
        self.condition_projection = nn.Conv1d(dim_cond, dim_model, 1)
        self.attn = attn

    def reference_forward(self, x, condition=None, diffusion_step=None):
        """the layer's mathematics on [B, D, L]: bias x by the two projections, run the conv module on the frame-major view,
        add the x that came in"""
        bias = self.diffusion_step_projection(diffusion_step) + self.condition_projection(condition)
        h = (x + bias).transpose(1, 2)
        if self.attn is not None:
            h = self.attn(self.norm(h))
        h = self.conformer(h).transpose(1, 2)
        if self.wavenet_like_proj is None:
            return h + x
        h = F.glu(self.wavenet_like_proj(h), dim=1)
        return (h + x) / math.sqrt(2.0), x

    def forward(self, x, condition=None, diffusion_step=None):
        return NV.layer_forward(self, x, condition, diffusion_step)


class StepEmbedding(nn.Module):
    """any function of the step [B] -> [B, dim] stands in for the sinusoidal embedding and its mlp"""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, t):
        k = torch.arange(self.dim, dtype=torch.float32, device=t.device)
        return torch.cos(t[:, None] * (0.05 + 0.01 * k)[None, :])


class Diff(nn.Module):
    def __init__(self, mel_channels=8, dim=512, condition_dim=128, num_layers=3, layers=None):
        super().__init__()
        self.wavenet_like = False
        self.mask_cond_ratio = None
        self.input_projection = nn.Conv1d(mel_channels, dim, 1)
        self.diffusion_embedding = StepEmbedding(dim)
        self.conditioner_projection = nn.Identity()
        self.residual_layers = nn.ModuleList(layers if layers is not None
                                             else [DiffLayer(dim, condition_dim) for _ in range(num_layers)])
        self.output_projection = nn.Conv1d(dim, mel_channels, 1)

    def _around(self, spec, diffusion_step, cond, run):
        mel = spec.select(1, 0) if spec.dim() == 4 else spec
        x = F.gelu(self.input_projection(mel))
        step = self.diffusion_embedding(diffusion_step).unsqueeze(-1)
        condition = self.conditioner_projection(cond)
        for layer in self.residual_layers:
            x = run(layer)(x, condition, step)
        out = self.output_projection(x)
        return out.unsqueeze(1) if spec.dim() == 4 else out

    def reference_forward(self, spec, diffusion_step, cond):
        """what the reference's class does when it is not routed to the stack: every layer through its own ``forward``"""
        return self._around(spec, diffusion_step, cond, lambda layer: layer)

    def plain_forward(self, spec, diffusion_step, cond):
        """the same with every layer's ``reference_forward``: no dispatcher anywhere"""
        return self._around(spec, diffusion_step, cond, lambda layer: layer.reference_forward)

    def forward(self, spec, diffusion_step, cond):
        return NV.net_forward(self, spec, diffusion_step, cond)
