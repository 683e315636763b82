"""Elementwise parity of a GEMM output against a float64 reference (test infrastructure; torch tensors on any device).

Output buffers are guarded: `Guarded(M, N, dtype, device)` holds a flat buffer of 256 guard bytes, then M x N outputs, then 16 guard rows,
the output starting 16-byte aligned, all filled with a NaN sentinel (bf16 0x7FA5; 0x7FA5A5A5 for fp32 and int32, which no int32
accumulator of an 8-bit GEMM reaches).  `check` then asserts, in this order: the guards are untouched, no sentinel is left inside
M x N, and every element matches the reference:
  * exact: the same bits as `ref_bits` (int8 scaled / dynamic outputs on the oracle's epilogue, int_mm's int32);
  * otherwise |y - ref64| <= ulp(ref64) + 2 max(K, k_floor) 2^-24 S per element, S = |x| |w|^T with the scales applied (float64),
    ulp of bf16 or fp32 as the output, `k_floor` 0 by default; and, for bf16 outputs of at least 1024 elements, a fraction `equal` of
    them equal to the oracle's rounding of ref64 (fp32 -> bf16): 0.97 by default.  The fp8 MFMAs sum e4m3 products spanning 2^36 less
    exactly than a float64 sum rounded once -- by a share of S that one MFMA sets and a longer K does not grow, hence the floor on K
    -- and the fp8 x int4 kernel rounds once more per group: callers pass what those families reach within the bound above.
`written_rows` (the grouped GEMMs: offs[-1]) asks for rows [written_rows, M) to still hold the sentinel and compares only the rows
above.  A failure names the count of bad elements, the first bad (row, column) and its tile and K parts under the route.
"""
import torch

GUARD_BYTES = 256
GUARD_ROWS = 16
SENTINEL = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5, torch.int32: 0x7FA5A5A5}
SENTINEL2 = {torch.bfloat16: 0x7FC3, torch.float32: 0x7FC3C3C3, torch.int32: 0x7FC3C3C3}
_BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32}
EQUAL_FRACTION = 0.97
EQUAL_MIN_ELEMENTS = 1024


def _signed(v, bits):
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


class Guarded:
    """A poisoned output buffer: .out is the M x N view the kernel writes, .raw the whole buffer as integers."""

    def __init__(self, M, N, dtype, device, sentinel=None):
        self.M, self.N, self.dtype = M, N, dtype
        esize = torch.empty((), dtype=dtype).element_size()
        self.lead = GUARD_BYTES // esize
        total = self.lead + (M + GUARD_ROWS) * N
        itype = _BITS[dtype]
        self.raw = torch.empty(total + 16, dtype=itype, device=device)
        off = (-self.raw.data_ptr() // esize) % (16 // esize)  # the output (after 256 bytes) 16-byte aligned
        self.raw = self.raw[off:off + total]
        self.poison(sentinel)
        self.out = self.raw[self.lead:self.lead + M * N].view(dtype).view(M, N)
        assert self.out.data_ptr() % 16 == 0

    def poison(self, sentinel=None):
        s = (sentinel or SENTINEL)[self.dtype]
        self.sentinel = _signed(s, self.raw.element_size() * 8)
        self.raw.fill_(self.sentinel)

    def bits(self):
        return self.raw[self.lead:self.lead + self.M * self.N].view(self.M, self.N)

    def guard_problems(self):
        head = self.raw[:self.lead]
        tail = self.raw[self.lead + self.M * self.N:]
        msgs = []
        if bool((head != self.sentinel).any()):
            i = int(torch.nonzero(head != self.sentinel)[0])
            msgs.append("write into the %d guard bytes before the output (element %d)" % (GUARD_BYTES, i - self.lead))
        if bool((tail != self.sentinel).any()):
            i = int(torch.nonzero(tail != self.sentinel)[0])
            msgs.append("write into the guard rows after row M: row %d, column %d" % (self.M + i // self.N, i % self.N))
        return msgs


def ulp(ref, dtype):
    """The spacing of `dtype` (bf16 or fp32) at |ref| (float64), its subnormal spacing near 0."""
    mant, lo = (8, -133) if dtype == torch.bfloat16 else (24, -149)
    _, e = torch.frexp(ref.abs())
    return torch.exp2(torch.clamp(e - mant, min=lo).to(torch.float64))


def oracle_round(ref64, dtype):
    """The oracle's rounding of a float64 result: fp32, then (bf16 outputs) bf16 round-to-nearest-even."""
    r = ref64.to(torch.float32)
    return r.to(torch.bfloat16) if dtype == torch.bfloat16 else r


def locate(i, j, route):
    """Tile and K-part coordinates of an output element under a route (route_cases.route_of)."""
    if route is None:
        return ""
    return " (tile %d, %d of %d x %d; %d K parts)" % (i // route["rows"], j // route["cols"], route["rows"], route["cols"], route["parts"])


def bound(ref64, S, K, dtype, k_floor=0):
    return ulp(ref64, dtype) + 2.0 * max(K, k_floor) * 2.0 ** -24 * S


def k_needed(y, ref64, S, dtype):
    """The smallest max(K, k_floor) under which every element of y meets the bound."""
    over = ((y.to(torch.float64) - ref64).abs() - ulp(ref64, dtype)).clamp(min=0)
    return (over / (2.0 * 2.0 ** -24 * S)).nan_to_num(0.0).max().item() if y.numel() else 0.0


def problems(buf, *, ref64=None, S=None, K=None, ref_bits=None, route=None, equal=EQUAL_FRACTION, k_floor=0, written_rows=None):
    """Every way the guarded output misses the reference, as messages (empty: the output passes)."""
    msgs = buf.guard_problems()
    bits = buf.bits()
    rows = buf.M if written_rows is None else written_rows
    if rows < buf.M:
        written = bits[rows:] != buf.sentinel
        if bool(written.any()):
            i, j = (int(v) for v in torch.nonzero(written)[0])
            msgs.append("%d elements written in the rows past %d that must stay unwritten, first at row %d, column %d%s"
                        % (int(written.sum()), rows, rows + i, j, locate(rows + i, j, route)))
    bits = bits[:rows]
    unwritten = bits == buf.sentinel
    if bool(unwritten.any()):
        i, j = (int(v) for v in torch.nonzero(unwritten)[0])
        msgs.append("%d elements left unwritten (sentinel), first at row %d, column %d%s" % (int(unwritten.sum()), i, j, locate(i, j, route)))
    y = buf.out[:rows]
    if ref64 is not None:
        ref64, S = ref64[:rows], S[:rows]
    if ref_bits is not None:
        ref_bits = ref_bits[:rows]
        want = ref_bits.view(_BITS[buf.dtype]) if ref_bits.dtype != _BITS[buf.dtype] else ref_bits
        bad = bits != want
        if bool(bad.any()):
            i, j = (int(v) for v in torch.nonzero(bad)[0])
            msgs.append("%d elements differ from the exact result, first at row %d, column %d: %r vs %r%s"
                        % (int(bad.sum()), i, j, y[i, j].item(), ref_bits.view(buf.dtype)[i, j].item(), locate(i, j, route)))
        return msgs
    yd = y.to(torch.float64)
    b = bound(ref64, S, K, buf.dtype, k_floor)
    bad = ~((yd - ref64).abs() <= b)  # NaN fails
    if bool(bad.any()):
        i, j = (int(v) for v in torch.nonzero(bad)[0])
        msgs.append("%d elements outside |y - ref| <= ulp + 2 max(K, %d) 2^-24 S, first at row %d, column %d: %r vs %r (bound %.3g; the "
                    "worst element needs max(K, k_floor) >= %.0f)%s"
                    % (int(bad.sum()), k_floor, i, j, y[i, j].item(), ref64[i, j].item(), b[i, j].item(), k_needed(y, ref64, S, buf.dtype),
                       locate(i, j, route)))
    if buf.dtype == torch.bfloat16 and y.numel() >= EQUAL_MIN_ELEMENTS:
        eq = (y == oracle_round(ref64, buf.dtype)).double().mean().item()
        if eq < equal:
            msgs.append("only %.4f of the elements equal the oracle's rounding (>= %.2f required)" % (eq, equal))
    return msgs


def check(buf, **kw):
    msgs = problems(buf, **kw)
    assert not msgs, "; ".join(msgs)
