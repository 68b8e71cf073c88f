"""Stand-ins with the module trees of the reference's ``diffusion.wavenet`` ``ResidualBlock`` and ``WaveNet``.  Their ``forward``
is the package's dispatcher, as the reference's classes have it after ``patch_reference_wavenet()``; ``reference_forward`` is the
reference's own op chain, restated."""
import math

import torch
import torch.nn.functional as F
from torch import nn

from ddsp_svc_amd import wavenet as WN


class ResidualBlock(nn.Module):
    def __init__(self, encoder_hidden, residual_channels, dilation=1, kernel=3):
        super().__init__()
        self.residual_channels = residual_channels
        self.dilated_conv = nn.Conv1d(residual_channels, 2 * residual_channels, kernel_size=kernel,
                                      padding=dilation * (kernel // 2), dilation=dilation)
        self.diffusion_projection = nn.Linear(residual_channels, residual_channels)
        self.conditioner_projection = nn.Conv1d(encoder_hidden, 2 * residual_channels, 1)
        self.output_projection = nn.Conv1d(residual_channels, 2 * residual_channels, 1)

    def reference_forward(self, x, conditioner, diffusion_step):
        C = self.residual_channels
        diffusion_step = self.diffusion_projection(diffusion_step).unsqueeze(-1)
        y = self.dilated_conv(x + diffusion_step) + self.conditioner_projection(conditioner)
        gate, filt = torch.split(y, [C, C], dim=1)
        y = self.output_projection(torch.sigmoid(gate) * torch.tanh(filt))
        residual, skip = torch.split(y, [C, C], dim=1)
        return (x + residual) / math.sqrt(2.0), skip

    def forward(self, x, conditioner, diffusion_step):
        return WN.layer_forward(self, x, conditioner, diffusion_step)


class StepEmbedding(nn.Module):
    """any function of the step [B] -> [B, dim] stands in for the sinusoidal embedding"""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, t):
        k = torch.arange(self.dim, dtype=torch.float32, device=t.device)
        return torch.sin(t[:, None] * (0.1 + 0.01 * k)[None, :])


class WaveNet(nn.Module):
    def __init__(self, in_dims=8, n_layers=3, n_chans=384, n_hidden=256, blocks=None):
        super().__init__()
        self.input_projection = nn.Conv1d(in_dims, n_chans, 1)
        self.diffusion_embedding = StepEmbedding(n_chans)
        self.mlp = nn.Sequential(nn.Linear(n_chans, n_chans * 4), nn.Mish(), nn.Linear(n_chans * 4, n_chans))
        self.residual_layers = nn.ModuleList(blocks if blocks is not None
                                             else [ResidualBlock(n_hidden, n_chans) for _ in range(n_layers)])
        self.skip_projection = nn.Conv1d(n_chans, n_chans, 1)
        self.output_projection = nn.Conv1d(n_chans, in_dims, 1)

    def reference_forward(self, spec, diffusion_step, cond):
        x = F.relu(self.input_projection(spec.squeeze(1)))
        s = self.mlp(self.diffusion_embedding(diffusion_step))
        skip = []
        for layer in self.residual_layers:
            x, sk = layer.reference_forward(x, cond, s)
            skip.append(sk)
        x = torch.sum(torch.stack(skip), dim=0) / math.sqrt(len(self.residual_layers))
        x = F.relu(self.skip_projection(x))
        return self.output_projection(x)[:, None, :, :]

    def forward(self, spec, diffusion_step, cond):
        return WN.net_forward(self, spec, diffusion_step, cond)


def load(block, weights, proj=None):
    """copy oracle weights (numpy) into a ResidualBlock (a stand-in or the reference's)"""
    with torch.no_grad():
        for p, a in zip((block.dilated_conv.weight, block.dilated_conv.bias, block.conditioner_projection.weight,
                         block.conditioner_projection.bias, block.output_projection.weight, block.output_projection.bias), weights):
            p.copy_(torch.as_tensor(a))
        if proj is not None:
            block.diffusion_projection.weight.copy_(torch.as_tensor(proj[0]))
            block.diffusion_projection.bias.copy_(torch.as_tensor(proj[1]))
    return block
