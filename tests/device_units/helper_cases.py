"""Inputs and float64 models for the packed complex helpers of ddsp_svc_amd/csrc/fft2048.h, shared by tests/test_device_units.py and
tests/golden/make_golden_device_units.py (TEST INFRASTRUCTURE ONLY).

A record is 16 complex words in and 16 out (k_helpers of units.hip).  The one-value helpers read slots 0, 1, 2 (a, b, and the
addend of the three-operand forms) and write slot 0; the eight-value ones read slots 0..7 (values) and 8..15 (factors).
"""
import itertools

import numpy as np

# name -> (op of k_helpers, input slots read, output slots written)
HELPERS = {
    "cmul": (0, 2, 1), "cmul_uniform": (1, 2, 1), "cmul_lo": (2, 2, 1), "cmul_hi": (3, 3, 1), "cmulc_hi": (4, 3, 1), "cmulc": (5, 2, 1),
    "twiddle7": (6, 16, 8), "twiddle7x2": (7, 16, 16),
    "add_mi": (8, 2, 1), "sub_mi": (9, 2, 1), "add_conj": (10, 2, 1), "sub_conj": (11, 2, 1), "swap_scale": (12, 2, 1),
    "swap_scale_add": (13, 3, 1), "conj_minus_i_conj": (14, 2, 1),
    "dft4": (15, 4, 4), "dft4_rot2": (16, 4, 4), "dft8": (17, 8, 8), "dft8_lo4": (18, 4, 8),
}
# one float32 rounding each, and no other arithmetic: these must BE the correctly rounded result
EXACT = ("add_mi", "sub_mi", "add_conj", "sub_conj", "conj_minus_i_conj", "swap_scale")
SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf], np.float32)
N_RANDOM = 4096          # calls of a one-value helper; the eight-value helpers get 512 calls = 4096 complex operands
H32 = float(np.float32(0.70710678118654752))                 # the W_8 constant as dft8 holds it


def _normals(rng, exps):
    """float32 of random sign and mantissa with the given binary exponents"""
    m = rng.integers(0, 1 << 23, exps.shape, dtype=np.uint32)
    s = rng.integers(0, 2, exps.shape, dtype=np.uint32)
    return ((s << 31) | ((exps + 127).astype(np.uint32) << 23) | m).view(np.float32)


def random_records(name):
    """Seeded normal float32 with exponents spread over 2^-60 .. 2^60: one exponent per record for the values, one for the factors,
    each slot within 2^+-2 of its record's (so that the terms of a sum meet at comparable sizes and the roundings matter), and the
    addend of the three-operand helpers at the size of the product where that stays inside the range."""
    op, n_in, _ = HELPERS[name]
    n = N_RANDOM if n_in <= 3 else N_RANDOM // 8
    rng = np.random.default_rng(1000 + op)
    ea, eb = rng.integers(-58, 59, (n, 1, 1)), rng.integers(-58, 59, (n, 1, 1))
    base = np.zeros((n, 16, 1), np.int64)
    if n_in <= 3:
        base[:, 0], base[:, 1], base[:, 2] = ea[:, 0], eb[:, 0], np.clip(ea + eb, -58, 58)[:, 0]
    else:
        base[:, :8], base[:, 8:] = ea, eb
    rec = _normals(rng, base + rng.integers(-2, 3, (n, 16, 2)))
    rec[:, n_in:] = 0
    return _uniform_factor(name, rec)


def special_records(name):
    """Every combination of +-0, +-1 and +-inf in the operand slots of the one-value helpers (6^4 or 6^6 records) and, for the two
    twiddle helpers, in each (value, factor) pair, a different combination per k.  The butterflies have 6^8 .. 6^16 combinations:
    they get 4096 seeded draws, in which every pair of slots meets each of its 36 combinations about a hundred times."""
    op, n_in, _ = HELPERS[name]
    if name == "cmul_uniform":                               # one wave per factor: its 36 values of a, padded to 64 lanes
        pairs = np.array(list(itertools.product(SPECIALS, repeat=2)), np.float32)
        rec = np.zeros((36, 64, 16, 2), np.float32)
        rec[:, :36, 0] = pairs[None, :]
        rec[:, :, 1] = pairs[:, None]
        return rec.reshape(-1, 16, 2)
    if n_in <= 3:
        combos = np.array(list(itertools.product(SPECIALS, repeat=2 * n_in)), np.float32)
        rec = np.zeros((-(-len(combos) // 64) * 64, 16, 2), np.float32)
        rec[:len(combos), :n_in] = combos.reshape(-1, n_in, 2)
        return rec
    if name.startswith("twiddle7"):
        combos = np.array(list(itertools.product(SPECIALS, repeat=4)), np.float32).reshape(-1, 2, 2)     # 1296 (value, factor) pairs
        rec = np.zeros((1344, 16, 2), np.float32)
        for k in range(8):
            pick = (np.arange(1344) + 185 * k) % 1296
            rec[:, k], rec[:, 8 + k] = combos[pick, 0], combos[pick, 1]
        return rec
    rng = np.random.default_rng(2000 + op)
    rec = np.zeros((4096, 16, 2), np.float32)
    rec[:, :n_in] = SPECIALS[rng.integers(0, 6, (4096, n_in, 2))]
    return rec


def _uniform_factor(name, rec):
    if name == "cmul_uniform":                               # the factor is wave-uniform: every lane gets that of its wave's first
        rec[:, 1] = np.repeat(rec[::64, 1], 64, axis=0)
    return rec


def run(units, name, rec):
    """the helper on every record: (n, 16, 2) float32 -> the output slots it writes, (n, n_out, 2) float32"""
    import torch
    op, _, n_out = HELPERS[name]
    out = units.zeros(rec.shape, torch.float32)
    units.call("du_helpers", op, units.to(rec), out, len(rec))
    return units.numpy(out)[:, :n_out]


class C:
    """a complex array in float64 with, per component, the sum of the absolute values of its exact terms"""
    def __init__(self, x, y, mx=None, my=None):
        self.x, self.y = x, y
        self.mx, self.my = (np.abs(x) if mx is None else mx), (np.abs(y) if my is None else my)

    def __add__(self, o): return C(self.x + o.x, self.y + o.y, self.mx + o.mx, self.my + o.my)
    def __sub__(self, o): return C(self.x - o.x, self.y - o.y, self.mx + o.mx, self.my + o.my)
    def __mul__(self, o): return C(self.x * o.x - self.y * o.y, self.x * o.y + self.y * o.x,
                                   self.mx * o.mx + self.my * o.my, self.mx * o.my + self.my * o.mx)
    def conj(self): return C(self.x, -self.y, self.mx, self.my)
    def mi(self): return C(self.y, -self.x, self.my, self.mx)                     # -i z
    def stack(self): return np.stack([self.x, self.y], -1), np.stack([self.mx, self.my], -1)


def _const(x, y, like):
    return C(np.full_like(like.x, x), np.full_like(like.x, y))


def _dft4(a0, a1, a2, a3):
    t0, t1, t2, d = a0 + a2, a0 - a2, a1 + a3, a1 - a3
    return t0 + t2, t1 + d.mi(), t0 - t2, t1 - d.mi()


def _dft8(v):
    e = [v[k] + v[k + 4] for k in range(4)]
    o = [v[k] - v[k + 4] for k in range(4)]
    o[1], o[3] = o[1] * _const(H32, -H32, o[1]), o[3] * _const(-H32, -H32, o[3])
    ev, od = _dft4(*e), _dft4(o[0], o[1], o[2].mi(), o[3])
    return [ev[0], od[0], ev[1], od[1], ev[2], od[2], ev[3], od[3]]


def model(name, rec):
    """float64 value of every output component and the sum of |exact terms| behind it: two (n, n_out, 2) arrays"""
    r = rec.astype(np.float64)
    s = [C(r[:, k, 0], r[:, k, 1]) for k in range(16)]
    a, b, t = s[0], s[1], s[2]
    zero = np.zeros_like(a.x)
    if name in ("cmul", "cmul_uniform"): out = [a * b]
    elif name == "cmul_lo": out = [C(a.x * b.x, a.x * b.y)]
    elif name == "cmul_hi": out = [t + C(-a.y * b.y, a.y * b.x)]
    elif name == "cmulc_hi": out = [t + C(a.y * b.y, -a.y * b.x)]
    elif name == "cmulc": out = [a.conj() * b]
    elif name == "twiddle7": out = [s[0]] + [s[k] * s[8 + k] for k in range(1, 8)]
    elif name == "twiddle7x2": out = [s[0]] + [s[k] * s[8 + k] for k in range(1, 8)] + [s[15]] + [s[15 - k] * s[7 - k] for k in range(1, 8)]
    elif name == "add_mi": out = [a + b.mi()]
    elif name == "sub_mi": out = [a - b.mi()]
    elif name == "add_conj": out = [a + b.conj()]
    elif name == "sub_conj": out = [a - b.conj()]
    elif name == "swap_scale": out = [C(a.y * b.x, a.x * b.y)]
    elif name == "swap_scale_add": out = [C(a.y * b.x, a.x * b.y) + t]
    elif name == "conj_minus_i_conj": out = [C(a.x - b.y, -a.y - b.x, a.mx + b.my, a.my + b.mx)]
    elif name == "dft4": out = list(_dft4(*s[:4]))
    elif name == "dft4_rot2": out = list(_dft4(s[0], s[1], s[2].mi(), s[3]))
    elif name == "dft8": out = _dft8(s[:8])
    elif name == "dft8_lo4": out = _dft8(s[:4] + [C(zero, zero)] * 4)
    else: raise KeyError(name)
    vals, mags = zip(*(c.stack() for c in out))
    return np.stack(vals, 1), np.stack(mags, 1)


def correctly_rounded(name, rec):
    """the helpers of EXACT in float32 arithmetic: one IEEE rounding per component"""
    a, b = rec[:, 0], rec[:, 1]
    ax, ay, bx, by = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    with np.errstate(all="ignore"):
        x, y = {"add_mi": (ax + by, ay - bx), "sub_mi": (ax - by, ay + bx), "add_conj": (ax + bx, ay - by),
                "sub_conj": (ax - bx, ay + by), "conj_minus_i_conj": (ax - by, -ay - bx), "swap_scale": (ay * bx, ax * by)}[name]
    return np.stack([x, y], -1)[:, None]


def _model_bits(name, rec):
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(model(name, rec)[0].astype(np.float32)).view(np.uint32)


def pack(name, rec, twin):
    """the twin's outputs on the random records as they are kept in tests/golden/device_units.npz: the distance of their bit patterns
    from the float32 rounding of the float64 model (a few units in the last place, so the array compresses to a fraction)"""
    return np.ascontiguousarray(twin, np.float32).view(np.uint32) - _model_bits(name, rec)


def unpack(name, rec, packed):
    return (_model_bits(name, rec) + packed).view(np.float32)
