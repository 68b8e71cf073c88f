"""Stand-ins with the module trees of the reference's conformer conv module, in both spellings: the naive one
(``nn.GLU``, ``nn.SiLU``, a padded depthwise ``nn.Conv1d``, ``nn.Identity`` or ``nn.LayerNorm`` in front) and pcmer's (its own
``GLU`` and ``Swish``, a pad-then-conv wrapper, always a LayerNorm).  Their ``forward`` is the package's dispatcher, as the
reference's classes have it after ``patch_reference_conformer()``."""
import torch
import torch.nn.functional as F
from torch import nn

from ddsp_svc_amd import conformer as CF


class Transpose(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.dims = dims

    def forward(self, x):
        return x.transpose(*self.dims)


class Swish(nn.Module):
    def forward(self, x):
        return x * x.sigmoid()


class GLU(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        out, gate = x.chunk(2, dim=self.dim)
        return out * gate.sigmoid()


class DepthWiseConv1d(nn.Module):
    def __init__(self, chan_in, chan_out, kernel_size, padding):
        super().__init__()
        self.padding = padding
        self.conv = nn.Conv1d(chan_in, chan_out, kernel_size, groups=chan_in)

    def forward(self, x):
        return self.conv(F.pad(x, self.padding))


class ConvModule(nn.Module):
    def __init__(self, dim, expansion=2, taps=31, dropout=0.0, use_norm=False, pcmer=False):
        super().__init__()
        inner = dim * expansion
        pad = taps // 2
        if pcmer:
            mid = [GLU(dim=1), DepthWiseConv1d(inner, inner, taps, (pad, pad)), Swish()]
        else:
            mid = [nn.GLU(dim=1), nn.Conv1d(inner, inner, taps, padding=pad, groups=inner), nn.SiLU()]
        self.net = nn.Sequential(nn.LayerNorm(dim) if (use_norm or pcmer) else nn.Identity(), Transpose((1, 2)),
                                 nn.Conv1d(dim, inner * 2, 1), *mid, nn.Conv1d(inner, dim, 1), Transpose((1, 2)),
                                 nn.Dropout(dropout))

    def forward(self, x):
        return CF.conv_forward(self, x)


class EncoderLayer(nn.Module):
    """``CFNEncoderLayer``'s attributes; ``attn`` is any module taking ``(x, mask=None)`` or None"""

    def __init__(self, dim, attn=None, **kw):
        super().__init__()
        self.conformer = ConvModule(dim, **kw)
        self.norm = nn.LayerNorm(dim)
        self.attn = attn

    def forward(self, x, mask=None):
        return CF.layer_forward(self, x, mask)


class ScaleAttn(nn.Module):
    """a stand-in for the attention half: any function of (x, mask)"""

    def forward(self, x, mask=None):
        return 0.5 * x


def load(module, weights, norm=None):
    """copy oracle weights (numpy) into a ConvModule"""
    net = module.net
    dw = net[4] if isinstance(net[4], nn.Conv1d) else net[4].conv
    with torch.no_grad():
        for p, a in zip((net[2].weight, net[2].bias, dw.weight, dw.bias, net[6].weight, net[6].bias), weights):
            p.copy_(torch.as_tensor(a))
        if norm is not None:
            net[0].weight.copy_(torch.as_tensor(norm[0]))
            net[0].bias.copy_(torch.as_tensor(norm[1]))
    return module
