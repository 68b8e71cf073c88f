"""A stand-in for the NSF-HiFiGAN generator, for the chain tests (tests/test_generator_chain.py): a plain ``torch.nn.Module``
with the attribute names ``ddsp_svc_amd.nsf_generator.generator_forward`` reads, built from ``Conv1d`` / ``ConvTranspose1d``
by the formulas of tests/generator_tail_oracle.py and tests/resblock_oracle.py, without weight norm:

    conv_pre   Conv1d(mels, C0, 7, padding 3)
    stage i    ConvTranspose1d(C0 / 2^i, C0 / 2^(i+1), 2 u, u, padding u / 2) on lrelu_0.1(x), plus the noise conv of the source:
               Conv1d(1, C, 2 s, s, padding s // 2) with s the product of the later rates, Conv1d(1, C, 1) at s = 1;
               then the mean of three residual blocks, k = 3, 7, 11, dilations (1, 3, 5)
    conv_post  Conv1d(C, 1, 7, padding 3) on lrelu_0.01(x), then tanh

``Generator.forward`` is the torch chain (the yardstick e_torch and what a call that cannot run on HIP falls back to); a block's
``forward`` is ``nsf_generator.resblock_forward``, as the patch binds it on the reference's class, and its ``chain`` the torch
line.  ``m_source`` returns a stored ``[B, L upp, 1]`` tensor.  Every weight is seeded (``weights``), so none is committed.

Two topologies:  "a", the stock vocoder's tail: C0 = 256, rates [2, 2, 2, 2] -- stage 0 (256 -> 128) stays on torch, then the
seams (Cout, u, s) = (64, 2, 4), (32, 2, 2), (16, 2, 1) and a 16-channel head;  "b": C0 = 128, rates [8, 4] -- seams (64, 8, 4),
whose tile is 64 columns, and (32, 4, 1), a 32-channel head, nothing on torch.

``oracle_chain`` is the float64 chain: conv_pre, ``generator_tail_oracle.seam``, ``resblock_oracle.stage``, ``head``.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import generator_tail_oracle as TO
from tests import resblock_oracle as BO

from ddsp_svc_amd import nsf_generator as NG

MELS = 8
KERNELS = (3, 7, 11)
DILATIONS = (1, 3, 5)
TOPOLOGIES = {"a": dict(C0=256, rates=(2, 2, 2, 2), frames=24, seed=1000),
              "b": dict(C0=128, rates=(8, 4), frames=20, seed=2000)}
MEL_STD = 1.0
SOURCE_STD = 0.5


def stages(name):
    """per stage ``(Cout, u, s)``"""
    t = TOPOLOGIES[name]
    return [(t["C0"] >> (i + 1), u, int(np.prod(t["rates"][i + 1:]))) for i, u in enumerate(t["rates"])]


def upp(name):
    return int(np.prod(TOPOLOGIES[name]["rates"]))


def weights(name):
    """the seeded float32 weights: ``pre`` (w, b), per stage ``seams[i]`` (wu, bu, wn, bn) and ``blocks[i]`` a list of
    ``(pairs, dilations)`` as ``resblock_oracle.stage`` takes them, ``head`` (w, b)"""
    t = TOPOLOGIES[name]
    seed, C0 = t["seed"], t["C0"]
    rng = np.random.default_rng(seed)
    pre = ((rng.standard_normal((C0, MELS, 7)) / np.sqrt(7 * MELS)).astype(np.float32),
           (rng.standard_normal(C0) * 0.1).astype(np.float32))
    seams, blocks = [], []
    for i, (C, u, s) in enumerate(stages(name)):
        seams.append(TO.seeded_seam_weights(C, u, s, seed=seed + 10 * i + 1))
        blocks.append([(BO.seeded_weights(C, k, len(DILATIONS), seed=seed + 10 * i + 2 + j), DILATIONS)
                       for j, k in enumerate(KERNELS)])
    return dict(pre=pre, seams=seams, blocks=blocks, head=TO.seeded_head_weights(stages(name)[-1][0], seed=seed + 99))


def seeded_inputs(name, B, frames, seed=0):
    """float32 ``mel [B, MELS, frames]``, ``f0 [B, frames]`` and ``source [B, frames upp, 1]``; every utterance is different"""
    rng = np.random.default_rng(TOPOLOGIES[name]["seed"] + 500 + seed)
    mel = (MEL_STD * rng.standard_normal((B, MELS, frames))).astype(np.float32)
    f0 = np.full((B, frames), 220.0, np.float32)
    source = (SOURCE_STD * rng.standard_normal((B, frames * upp(name), 1))).astype(np.float32)
    return mel, f0, source


def oracle_chain(w, mel, source, rates):
    """float64: ``pre``, per stage ``seam_<i>`` (the blocks' input) and ``stage_<i>`` (the next seam's input, before its
    lrelu), and ``out``; with them ``noise_<i>``, the noise-conv term of seam i alone"""
    src = np.asarray(source, np.float64).reshape(source.shape[0], -1)
    rec = {"pre": BO.conv1d(mel, w["pre"][0], w["pre"][1], 1, 3)}
    x = rec["pre"]
    for i, u in enumerate(rates):
        wu, bu, wn, bn = w["seams"][i]
        s = int(np.prod(rates[i + 1:]))
        rec["noise_%d" % i] = TO.noise_conv(src, wn, bn, s)
        x = rec["seam_%d" % i] = TO.seam(x, wu, bu, u, src, wn, bn, s)
        x = rec["stage_%d" % i] = BO.stage(x, w["blocks"][i])
    rec["out"] = TO.head(x, *w["head"])
    return rec


class Block(torch.nn.Module):
    def __init__(self, C, k, dilations):
        super().__init__()
        self.convs1 = torch.nn.ModuleList([torch.nn.Conv1d(C, C, k, 1, dilation=d, padding=(k * d - d) // 2) for d in dilations])
        self.convs2 = torch.nn.ModuleList([torch.nn.Conv1d(C, C, k, 1, dilation=1, padding=(k - 1) // 2) for _ in dilations])

    def chain(self, x):
        for c1, c2 in zip(self.convs1, self.convs2):
            x = c2(F.leaky_relu(c1(F.leaky_relu(x, 0.1)), 0.1)) + x
        return x

    def forward(self, x):
        return NG.resblock_forward(self, x)


class StoredSource(torch.nn.Module):
    """the harmonic source as a stored tensor ``[B, L upp, 1]`` (the reference's draws noise on every call)"""

    def __init__(self):
        super().__init__()
        self.value = None

    def forward(self, f0, upp):
        assert tuple(self.value.shape) == (f0.shape[0], f0.shape[1] * upp, 1), (self.value.shape, f0.shape, upp)
        return self.value


class Generator(torch.nn.Module):
    def __init__(self, name):
        super().__init__()
        t = TOPOLOGIES[name]
        self.name, self.rates = name, tuple(t["rates"])
        self.num_kernels = len(KERNELS)
        self.upp = upp(name)
        self.m_source = StoredSource()
        self.conv_pre = torch.nn.Conv1d(MELS, t["C0"], 7, 1, padding=3)
        self.ups, self.noise_convs, self.resblocks = torch.nn.ModuleList(), torch.nn.ModuleList(), torch.nn.ModuleList()
        for C, u, s in stages(name):
            self.ups.append(torch.nn.ConvTranspose1d(2 * C, C, 2 * u, u, padding=u // 2))
            self.noise_convs.append(torch.nn.Conv1d(1, C, 2 * s, s, padding=s // 2) if s > 1 else torch.nn.Conv1d(1, C, 1))
            for k in KERNELS:
                self.resblocks.append(Block(C, k, DILATIONS))
        self.conv_post = torch.nn.Conv1d(stages(name)[-1][0], 1, 7, 1, padding=3)

    def stage_blocks(self, i):
        return self.resblocks[i * self.num_kernels:(i + 1) * self.num_kernels]

    def torch_seam(self, i, x, source):
        return self.ups[i](F.leaky_relu(x, 0.1)) + self.noise_convs[i](source)

    def torch_stage(self, i, x):
        xs = None
        for b in self.stage_blocks(i):
            xs = b.chain(x) if xs is None else xs + b.chain(x)
        return xs / self.num_kernels

    def torch_head(self, x):
        return torch.tanh(self.conv_post(F.leaky_relu(x)))

    def forward(self, x, f0):
        source = self.m_source(f0, self.upp).transpose(1, 2)
        x = self.conv_pre(x)
        for i in range(len(self.ups)):
            x = self.torch_stage(i, self.torch_seam(i, x, source))
        return self.torch_head(x)


class Tail(torch.nn.Module):
    """stages ``first`` ... of a stand-in as a generator of their own, sharing its modules: ``x`` is the boundary in front of
    stage ``first`` (``conv_pre`` is the identity) -- for "a" and ``first`` 1 the stages that run on HIP, behind the torch stage"""

    def __init__(self, gen, first):
        super().__init__()
        n = gen.num_kernels
        self.num_kernels, self.upp, self.m_source = n, gen.upp, gen.m_source
        self.conv_pre = torch.nn.Identity()
        self.ups, self.noise_convs = gen.ups[first:], gen.noise_convs[first:]
        self.resblocks, self.conv_post = gen.resblocks[first * n:], gen.conv_post

    def stage_blocks(self, i):
        return self.resblocks[i * self.num_kernels:(i + 1) * self.num_kernels]


def load_weights(gen, w):
    """copy ``weights(name)`` (or a fixture's) into a module with the generator's attribute names, in place"""
    def put(param, a):
        assert tuple(param.shape) == tuple(a.shape), (tuple(param.shape), a.shape)
        param.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    n = gen.num_kernels
    with torch.no_grad():
        put(gen.conv_pre.weight, w["pre"][0]), put(gen.conv_pre.bias, w["pre"][1])
        for i, (wu, bu, wn, bn) in enumerate(w["seams"]):
            put(gen.ups[i].weight, wu), put(gen.ups[i].bias, bu)
            put(gen.noise_convs[i].weight, wn), put(gen.noise_convs[i].bias, bn)
            for j, (pairs, _) in enumerate(w["blocks"][i]):
                blk = gen.resblocks[i * n + j]
                for p, (w1, b1, w2, b2) in enumerate(pairs):
                    put(blk.convs1[p].weight, w1), put(blk.convs1[p].bias, b1)
                    put(blk.convs2[p].weight, w2), put(blk.convs2[p].bias, b2)
        put(gen.conv_post.weight, w["head"][0]), put(gen.conv_post.bias, w["head"][1])
    return gen


def build(name, device="cpu"):
    """the stand-in of a topology with its seeded weights, in eval mode, parameters without ``requires_grad``"""
    gen = load_weights(Generator(name), weights(name)).eval().to(device)
    for p in gen.parameters():
        p.requires_grad_(False)
    return gen
