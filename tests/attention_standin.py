"""Stand-ins carrying the attributes that ``ddsp_svc_amd.attention``'s eligibility checks read of the reference's
``FastAttention`` and ``SelfAttention`` (``ddsp.pcmer`` does not import without ``local_attention``).  ``_reference_forward`` is
the float32 torch op chain of the same mathematics (tests/attention_oracle.py has it in float64) -- what ``park`` leaves on the
reference's classes -- and ``forward`` is the package's dispatcher, as after ``patch_reference_attention()``.
``FLAG_PCMER_NORM`` is this module's global, as it is ``ddsp.pcmer``'s."""
import math

import torch
from torch import nn

from ddsp_svc_amd import attention as AT

FLAG_PCMER_NORM = False


def feature_map(x, proj, is_query):
    d, m = x.shape[-1], proj.shape[0]
    dn, ratio = d ** -0.25, m ** -0.5
    dash = torch.matmul(dn * x, proj.to(x.dtype).t())
    g = (x * x).sum(-1, keepdim=True) / 2.0 * dn ** 2
    if is_query:
        return ratio * (torch.exp(dash - g - dash.max(-1, keepdim=True).values) + 1e-4)
    return ratio * torch.exp(dash - g + 1e-4)


def torch_chain(q, k, v, proj, normalize=False):
    """the op chain in q's dtype, on q's device"""
    if normalize:
        q = q / (q.norm(dim=-1, keepdim=True) + 1e-8)
        k = k / (k.norm(dim=-1, keepdim=True) + 1e-8)
    qp, kp = feature_map(q, proj, True), feature_map(k, proj, False)
    ksum = kp.sum(-2)
    dinv = 1.0 / (torch.einsum("...nd,...d->...n", qp, ksum) + 1e-8)
    ctx = torch.einsum("...nd,...ne->...de", kp, v)
    return torch.einsum("...de,...nd,...n->...ne", ctx, qp, dinv)


class FastAttention(nn.Module):
    def __init__(self, dim_heads=64, nb_features=None, causal=False, generalized_attention=False, no_projection=False, seed=0):
        super().__init__()
        self.dim_heads = dim_heads
        self.nb_features = int(dim_heads * math.log(dim_heads)) if nb_features is None else nb_features
        self.causal, self.generalized_attention, self.no_projection = causal, generalized_attention, no_projection
        proj = torch.randn(self.nb_features, dim_heads, generator=torch.Generator().manual_seed(seed))
        self.register_buffer("projection_matrix", proj)

    @torch.no_grad()
    def redraw_projection_matrix(self, seed=1):
        fresh = torch.randn(self.nb_features, self.dim_heads, generator=torch.Generator().manual_seed(seed))
        self.projection_matrix.copy_(fresh)

    def _reference_forward(self, q, k, v):
        return torch_chain(q, k, v, self.projection_matrix, FLAG_PCMER_NORM)

    def forward(self, q, k, v):
        return AT.fast_forward(self, q, k, v)


class LocalStub(nn.Module):
    """stands where ``LocalAttention`` would: only its presence is read"""

    def forward(self, q, k, v, input_mask=None):
        return v


class SelfAttention(nn.Module):
    def __init__(self, dim=256, heads=8, dim_head=64, local_heads=0, dropout=0.0, seed=0):
        super().__init__()
        inner = dim_head * heads
        self.fast_attention = FastAttention(dim_head, seed=seed)
        self.heads, self.global_heads = heads, heads - local_heads
        self.local_attn = LocalStub() if local_heads > 0 else None
        self.to_q, self.to_k, self.to_v = nn.Linear(dim, inner), nn.Linear(dim, inner), nn.Linear(dim, inner)
        self.to_out = nn.Linear(inner, dim)
        self.dropout = nn.Dropout(dropout)

    def _reference_forward(self, x, context=None, mask=None, context_mask=None, **kw):
        b, n, _ = x.shape
        h, gh = self.heads, self.global_heads
        src = x if context is None else context
        cmask = mask if context is None and context_mask is None else context_mask
        q, k, v = self.to_q(x), self.to_k(src), self.to_v(src)
        q, k, v = (t.reshape(b, t.shape[1], h, -1).permute(0, 2, 1, 3) for t in (q, k, v))
        outs = []
        if gh > 0:
            vg = v[:, :gh]
            if cmask is not None:
                vg = vg.masked_fill(~cmask[:, None, :, None], 0.0)
            outs.append(self.fast_attention(q[:, :gh], k[:, :gh], vg))
        if gh < h:
            outs.append(self.local_attn(q[:, gh:], k[:, gh:], v[:, gh:], input_mask=mask))
        out = torch.cat(outs, dim=1).permute(0, 2, 1, 3).reshape(b, n, -1)
        return self.dropout(self.to_out(out))

    def forward(self, x, context=None, mask=None, context_mask=None, **kw):
        return AT.self_forward(self, x, context, mask, context_mask, **kw)


def load(module, weights):
    """copy oracle weights (numpy: wq, bq, wk, bk, wv, bv, wo, bo) into a SelfAttention"""
    with torch.no_grad():
        for lin, (w, b) in zip((module.to_q, module.to_k, module.to_v, module.to_out), zip(weights[0::2], weights[1::2])):
            lin.weight.copy_(torch.as_tensor(w))
            lin.bias.copy_(torch.as_tensor(b))
    return module
