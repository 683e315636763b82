"""numpy restatement of the low-bit optimizer contract (csrc/quant_math.h "low-bit optimizer states").  TEST INFRASTRUCTURE ONLY.
Pinned against tests/golden/optim.npz, which tests/golden/make_golden_optim.py records from the reference's EAGER CPU run of
torchao/optim/adam.py single_param_adam and its three state subclasses.  Every operation is one fp32 operation rounded once:

  quantize (table)  scale = max(amax|x|, 1e-12) per block of the flat tensor;  y = x / scale;  branch-free descent (8 or 4 compares of
                    y >= qmap[code + step]);  up iff y - qmap[c] >= (qmap[min(c + 1, last)] - qmap[c]) * 0.5;  4-bit: element 2i in the HIGH nibble
  quantize (fp8)    scale = max(amax|x|, 1e-12) / 448;  code = e4m3fn_rne(x / scale)
  dequantize        qmap[code] * scale;  fp8: f32(code) * scale
  plain             read: to fp32;  write: RNE to the parameter's dtype
  step              AdamW p = p - (lr wd) p | Adam g = g + wd p;  m = lerp(m, g, 1 - b1);  v = lerp(v, g g, 1 - b2);  [vmax = max(vmax, v)];
                    denom = sqrt(v or vmax) / sqrt(1 - b2^t) + eps;  p = p - (lr (m / (1 - b1^t))) / denom;  the states are quantized from the
                    fp32 m, v, vmax the update used
  lerp              ATen's: |w| < 0.5: fma(w, e - s, s);  else fma(w - 1, e - s, e) -- ONE fused operation each (fma32 below is exact)
  SR (bf16 p)       away from zero iff r16 < (bits & 0xFFFF);  Philox4x32-10, key = the halves of the int64 seed, counter = (g_lo, g_hi, step,
                    param_index), g the flat index of the group of 8 elements;  element j takes bits 16 (j & 1) .. + 15 of word j >> 1
The seven scalars (lr, lr wd, wd, 1 - b1, 1 - b2, 1 - b1^t, sqrt(1 - b2^t), eps) come from the caller: ao_amd.optim.adam.step_scalars
computes them with the torch CPU operations the reference runs on its 0-dim tensors.
"""
import numpy as np

from nvfp4_train_ref import philox4x32_10

F32 = np.float32
FORMATS = {"q8s": 0, "q8u": 1, "q4s": 2, "q4u": 3, "fp8": 4, "plain": 5}
SCALAR_NAMES = ("lr", "lr_wd", "wd", "omb1", "omb2", "bc1", "sqrt_bc2", "eps")


# ---- the fixture's storage of p after a step: XOR with the bits before it -----------------------------------------------------------------
def _as_bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def pack_steps(rec, steps):
    """{p0, p1, ...} -> {p0, dp1, ...}; every other entry passes through"""
    out = {k: v for k, v in rec.items() if not (k[0] == "p" and k[1:].isdigit() and k != "p0")}
    for t in range(1, steps + 1):
        out[f"dp{t}"] = _as_bits(rec[f"p{t}"]) ^ _as_bits(rec[f"p{t - 1}"])
    return out


def load_golden(path):
    """tests/golden/optim.npz as a dict, with <case>_p<t> rebuilt from the stored XOR deltas"""
    import json

    z = np.load(path)
    g = {k: z[k] for k in z.files}
    for c in json.loads(str(g["cases"])):
        name = c["name"]
        for t in range(1, c["steps"] + 1):
            prev = g[f"{name}_p{t - 1}"]
            bits = _as_bits(prev) ^ g.pop(f"{name}_dp{t}")
            g[f"{name}_p{t}"] = bits.view(np.float32) if prev.dtype == np.float32 else bits
    return g


# ---- number formats ---------------------------------------------------------------------------------------------------------------------------
def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(x):
    """RNE, as bits (NaN is outside the contract)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def _e4m3_values():
    c = np.arange(128)
    e, m = c >> 3, (c & 7).astype(np.float64)
    return np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * np.exp2(e - 7.0))[:127]  # 0x7F is NaN


E4M3_POS = _e4m3_values()


def e4m3_decode(codes):
    c = np.asarray(codes, dtype=np.uint8)
    v = E4M3_POS[np.minimum(c & 0x7F, 126)].astype(np.float32)
    return np.where(c & 0x80, -v, v).astype(np.float32)


def e4m3_encode(y):
    """RNE onto the e4m3fn grid; |y| stays below the 464 that would round past 448"""
    y = np.asarray(y, dtype=np.float32)
    a = np.abs(y).astype(np.float64)
    _, e = np.frexp(a)
    step = np.exp2(np.maximum(e - 1, -6) - 3.0)
    q = np.rint(a / step) * step  # a / step is exact; rint: ties to even
    assert q.size == 0 or q.max() <= 448.0
    code = np.searchsorted(E4M3_POS, q).astype(np.uint8)
    assert np.array_equal(E4M3_POS[code], q)
    return np.where(np.signbit(y), code | np.uint8(0x80), code).astype(np.uint8)


def fma32(a, b, c):
    """fp32(a b + c), one rounding: the float64 product of two fp32 is exact; the float64 sum is rounded to ODD (TwoSum gives its error),
    so the final rounding to fp32 is never a double rounding (53 >= 24 + 2)."""
    p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, odd, s).astype(np.float32)


def lerp(s, e, w):
    w = F32(w)
    d = (e - s).astype(np.float32)
    if abs(w) < F32(0.5):
        return fma32(w, d, s)
    return fma32(F32(w - F32(1.0)), d, e)


def lerp_unfused(s, e, w):
    """the same formula with the product and the sum rounded separately: what the maker tells apart from lerp()"""
    w = F32(w)
    d = (e - s).astype(np.float32)
    if abs(w) < F32(0.5):
        return ((w * d).astype(np.float32) + s).astype(np.float32)
    return ((F32(w - F32(1.0)) * d).astype(np.float32) + e).astype(np.float32)


# ---- the state formats --------------------------------------------------------------------------------------------------------------------------
def block_scale(x, block_size):
    xb = np.asarray(x, dtype=np.float32).reshape(-1, block_size)
    return xb, np.maximum(np.abs(xb).max(axis=1), F32(1e-12)).astype(np.float32)


def quantize_table(x, qmap, block_size):
    """flat fp32 -> (codes uint8 one per element, scale fp32 [n / block_size])"""
    qmap = np.asarray(qmap, dtype=np.float32)
    last = qmap.size - 1
    xb, scale = block_scale(x, block_size)
    y = (xb / scale[:, None]).astype(np.float32).reshape(-1)
    codes = np.zeros(y.shape, dtype=np.int64)
    step = qmap.size // 2
    while step >= 1:
        codes += np.where(y >= qmap[codes + step], step, 0)
        step //= 2
    up = np.minimum(codes + 1, last)
    down_v, up_v = qmap[codes], qmap[up]
    codes = np.where((y - down_v).astype(np.float32) >= ((up_v - down_v).astype(np.float32) * F32(0.5)).astype(np.float32), up, codes)
    return codes.astype(np.uint8), scale


def pack4(codes):
    return ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8)


def unpack4(packed):
    return np.stack([packed >> 4, packed & 15], axis=-1).reshape(-1).astype(np.uint8)


def quantize_fp8(x, block_size):
    xb, amax = block_scale(x, block_size)
    scale = (amax / F32(448.0)).astype(np.float32)
    return e4m3_encode((xb / scale[:, None]).astype(np.float32).reshape(-1)), scale


def quantize(kind, x, block_size, qmap=None):
    """-> (codes as stored: one byte an element, 4-bit packed two a byte; scale)"""
    if kind == "fp8":
        return quantize_fp8(x, block_size)
    codes, scale = quantize_table(x, qmap, block_size)
    return (pack4(codes) if kind in ("q4s", "q4u") else codes), scale


def dequantize(kind, codes, scale, block_size, qmap=None):
    """-> flat fp32"""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1)
    if kind == "fp8":
        v = e4m3_decode(codes)
    else:
        v = np.asarray(qmap, dtype=np.float32)[unpack4(codes) if kind in ("q4s", "q4u") else codes]
    return (v.reshape(-1, block_size) * np.asarray(scale, dtype=np.float32)[:, None]).astype(np.float32).reshape(-1)


class State:
    """One moment: kind in FORMATS; quantized kinds hold codes / scale / qmap, "plain" holds `data` in the parameter's dtype (bf16 as uint16 bits)."""

    def __init__(self, kind, n, block_size=None, qmap=None, bf16=True):
        self.kind, self.n, self.block_size, self.bf16 = kind, n, block_size, bf16
        self.qmap = None if qmap is None else np.asarray(qmap, dtype=np.float32)
        if kind == "plain":
            self.data = np.zeros(n, dtype=np.uint16 if bf16 else np.float32)
        else:
            self.codes = np.zeros(n // 2 if kind in ("q4s", "q4u") else n, dtype=np.uint8)
            self.scale = np.zeros(n // block_size, dtype=np.float32)

    def read(self):
        if self.kind == "plain":
            return bf16_to_f32(self.data) if self.bf16 else self.data.copy()
        return dequantize(self.kind, self.codes, self.scale, self.block_size, self.qmap)

    def write(self, x):
        if self.kind == "plain":
            self.data = f32_to_bf16(x) if self.bf16 else np.asarray(x, dtype=np.float32).copy()
        else:
            self.codes, self.scale = quantize(self.kind, x, self.block_size, self.qmap)

    def fields(self):
        return {"data": self.data} if self.kind == "plain" else {"codes": self.codes, "scale": self.scale}


def new_states(kind, n, block_size, qmaps, bf16, amsgrad):
    """exp_avg, exp_avg_sq[, max_exp_avg_sq] for a format family "q8" | "q4" | "fp8" | "plain"; qmaps: {"q8s": ..., "q8u": ..., "q4s": ..., "q4u": ...}"""
    def one(signed):
        if kind in ("q8", "q4"):
            k = kind + ("s" if signed else "u")
            return State(k, n, block_size, qmaps[k], bf16)
        return State(kind, n, block_size, None, bf16)
    return [one(True), one(False)] + ([one(False)] if amsgrad else [])


# ---- stochastic rounding ------------------------------------------------------------------------------------------------------------------------
def sr_random16(n, seed, step, param_index):
    """the 16 random bits of each of n flat elements"""
    seed = int(seed) & (2 ** 64 - 1)
    g = np.arange((n + 7) // 8, dtype=np.uint64)
    with np.errstate(over="ignore"):
        words = philox4x32_10(g, g >> np.uint64(32), np.full_like(g, int(step) & 0xFFFFFFFF), np.full_like(g, int(param_index) & 0xFFFFFFFF),
                              seed & 0xFFFFFFFF, seed >> 32)
    w = np.stack(words, axis=-1)
    r = np.stack([w & np.uint64(0xFFFF), (w >> np.uint64(16)) & np.uint64(0xFFFF)], axis=-1)  # [groups, 4, 2]: element j = 2 word + half
    return r.reshape(-1)[:n].astype(np.uint32)


def sr_bf16(x, r16):
    """fp32 -> bf16 bits: away from zero iff r16 < the low half"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    up = np.asarray(r16, dtype=np.uint32) < (u & np.uint32(0xFFFF))
    return (((u & np.uint32(0xFFFF0000)).astype(np.uint64) + np.where(up, 0x10000, 0).astype(np.uint64)) >> np.uint64(16)).astype(np.uint16)


# ---- the step -------------------------------------------------------------------------------------------------------------------------------------
def adam_step(p, grad, states, scalars, is_adamw, bf16, sr=None, lerp_fn=lerp):
    """p, grad: the parameter's stored form (uint16 bf16 bits, or fp32), flat.  states: [m, v] or [m, v, vmax], updated in place.  scalars:
    dict over SCALAR_NAMES (fp32).  sr: None or (seed, step, param_index).  Returns the new p in its stored form."""
    s = {k: F32(scalars[k]) for k in SCALAR_NAMES}
    pf = bf16_to_f32(p) if bf16 else np.asarray(p, dtype=np.float32)
    gf = bf16_to_f32(grad) if bf16 else np.asarray(grad, dtype=np.float32)
    with np.errstate(under="ignore"):
        if is_adamw:
            pf = (pf - (s["lr_wd"] * pf).astype(np.float32)).astype(np.float32)
        else:
            gf = (gf + (s["wd"] * pf).astype(np.float32)).astype(np.float32)
        m = lerp_fn(states[0].read(), gf, s["omb1"])
        v = lerp_fn(states[1].read(), (gf * gf).astype(np.float32), s["omb2"])
        states[0].write(m)
        states[1].write(v)
        den = v
        if len(states) > 2:
            den = np.maximum(states[2].read(), v)
            states[2].write(den)
        denom = ((np.sqrt(den).astype(np.float32) / s["sqrt_bc2"]).astype(np.float32) + s["eps"]).astype(np.float32)
        pf = (pf - ((s["lr"] * (m / s["bc1"]).astype(np.float32)).astype(np.float32) / denom).astype(np.float32)).astype(np.float32)
    if not bf16:
        return pf
    if sr is not None:
        return sr_bf16(pf, sr_random16(pf.size, *sr))
    return f32_to_bf16(pf)
