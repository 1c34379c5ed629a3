"""Guard bands around kernel operands: a window of the requested shape inside ONE flat buffer whose every other element
holds a sentinel bit pattern, so that a kernel that writes outside its extents is caught (`assert_intact`) and a kernel
whose result depends on what lies outside is caught too (`poison` the outside with zeros / NaNs / huge values, run three
times, `assert_same_bits`).  Plain torch, any device; every comparison is on the integer view of the bits (a NaN
sentinel never equals itself as a float, and a NaN with another payload must count as a change).

    g = Guarded((m, n), torch.bfloat16, "cuda", ld=n + 8)   # rows of n inside rows of n + 8, 256 guard rows on both ends
    g.load(x)                                               # fill the window
    kernel(g.view.data_ptr(), ld=g.ld, ...)
    g.assert_intact("kernel output")
"""
import torch

# quiet NaNs with a recognisable payload (floats); a fixed odd byte / word for the integer-like buffers
_SENTINEL = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01, torch.float32: 0x7FC00123, torch.uint8: 0xA5,
             torch.int32: 0x5A5A5A5B}
# the integer type of the same width (the float8 types travel as uint8)
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8,
         torch.int32: torch.int32}
# largest finite value, (+, -); uint8 = OCP e4m3 +-448, int32 = its own extremes
_HUGE = {torch.bfloat16: (0x7F7F, 0xFF7F), torch.float16: (0x7BFF, 0xFBFF), torch.float32: (0x7F7FFFFF, 0xFF7FFFFF),
         torch.uint8: (0x7E, 0xFE), torch.int32: (0x7FFFFFFF, 0x80000001)}
GUARD_ROWS = 256        # the largest tile a kernel owns: 256 rows (the persistent GEMM kernel), of `ld` elements each
KINDS = ("zero", "nan", "huge")


def _signed(value, bits_dtype):
    """The Python int that, stored in `bits_dtype`, has the bit pattern `value`."""
    width = {torch.int16: 16, torch.int32: 32, torch.uint8: 8}[bits_dtype]
    if bits_dtype is not torch.uint8 and value >= 1 << (width - 1):
        value -= 1 << width
    return value


def bits(t):
    """`t` viewed as integers of its element width (same memory)."""
    return t if t.dtype in (torch.uint8, torch.int32, torch.int16) else t.view(_BITS[t.dtype])


class Guarded:
    def __init__(self, shape, dtype, device, ld=None, lead=None, trail=None, base_offset_bytes=0, fill="nan"):
        if dtype not in _SENTINEL:
            raise TypeError(f"Guarded: no sentinel for {dtype} (float8 buffers travel as torch.uint8)")
        shape = tuple(int(s) for s in shape)
        if not shape or min(shape) < 1:
            raise ValueError(f"Guarded: empty shape {shape}")
        self.shape, self.dtype, self.device = shape, dtype, torch.device(device)
        self.n = shape[-1]
        self.ld = int(ld) if ld is not None else self.n
        if self.ld < self.n:
            raise ValueError(f"Guarded: ld={self.ld} is smaller than the row width {self.n}")
        self.rows = 1
        for s in shape[:-1]:
            self.rows *= s
        esize = torch.empty((), dtype=dtype).element_size()
        if base_offset_bytes % esize or base_offset_bytes < 0:
            raise ValueError("Guarded: base_offset_bytes must be a non-negative multiple of the element size")
        guard = GUARD_ROWS * self.ld
        lead = guard if lead is None else int(lead)
        trail = guard if trail is None else int(trail)
        if lead < 0 or trail < 0:
            raise ValueError("Guarded: negative guard")
        # the window's base is `base_offset_bytes` past a 256-byte boundary: it has no alignment beyond what is asked for
        lead = -(-lead * esize // 256) * 256 // esize
        self.base = lead + base_offset_bytes // esize
        span = (self.rows - 1) * self.ld + self.n                   # first to last element of the window
        self.lead, self.trail = self.base, trail
        self.buf = torch.empty(self.base + span + trail, dtype=dtype, device=self.device)
        self._bits = bits(self.buf)
        # strides: the last axis contiguous, the one before it `ld`, the leading axes packed on top of that
        strides, acc = [1], self.ld
        for s in reversed(shape[1:-1]):
            strides.append(acc)
            acc *= s
        if len(shape) > 1:
            strides.append(acc)
        strides = tuple(reversed(strides[:len(shape)]))
        self.view = self.buf.as_strided(shape, strides, self.base)
        self._rows_view = self.buf.as_strided((self.rows, self.n), (self.ld, 1), self.base)
        self.outside = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.device)
        self.outside.as_strided((self.rows, self.n), (self.ld, 1), self.base).fill_(False)
        self._pattern = torch.empty_like(self._bits)
        self.kind = None
        self._set_pattern(fill)
        self._bits.copy_(self._pattern)                             # the window holds the fill as well until `load`

    # ---- patterns
    def _set_pattern(self, kind):
        bd = self._bits.dtype
        if kind == "nan":
            self._pattern.fill_(_signed(_SENTINEL[self.dtype], bd))
        elif kind == "zero":
            self._pattern.zero_()
        elif kind == "huge":
            pos, neg = (_signed(v, bd) for v in _HUGE[self.dtype])
            self._pattern[0::2] = pos
            self._pattern[1::2] = neg
        else:
            raise ValueError(f"Guarded: unknown fill {kind!r} (one of {KINDS})")
        self.kind = kind

    def poison(self, kind):
        """Refill everything OUTSIDE the window with zeros, the sentinel NaN, or the largest finite value with alternating
        sign; the window keeps its contents.  `assert_intact` then checks against this pattern."""
        self._set_pattern(kind)
        torch.where(self.outside, self._pattern, self._bits, out=self._bits)
        return self

    def load(self, tensor):
        """Fill the window (shape of the window, or anything that broadcasts / reshapes to it)."""
        t = torch.as_tensor(tensor, device=self.device)
        if t.dtype != self.dtype:
            t = t.to(self.dtype)
        if tuple(t.shape) != self.shape and t.numel() == self.view.numel():
            t = t.reshape(self.shape)
        self.view.copy_(t)
        return self

    def blank(self):
        """Fill the window with the sentinel NaN: after a kernel that must write every element, none may be left."""
        self._rows_view.view(self._bits.dtype).fill_(_signed(_SENTINEL[self.dtype], self._bits.dtype))
        return self

    # ---- checks
    def changed(self):
        """Flat buffer indices of the outside elements that no longer hold the pattern."""
        return torch.nonzero((self._bits != self._pattern) & self.outside).flatten()

    def locate(self, flat_index):
        """(row, column) of a flat buffer index relative to the window: row = whole `ld` steps from the window's first
        element (negative in the lead guard), column in [0, ld) - columns >= the width are the row's guard columns."""
        off = int(flat_index) - self.base
        row = off // self.ld
        return row, off - row * self.ld

    def assert_intact(self, what):
        bad = self.changed()
        if bad.numel():
            first = int(bad[0])
            row, col = self.locate(first)
            got = int(self._bits[first]) & ((1 << (8 * self.buf.element_size())) - 1)
            raise AssertionError(f"{what}: {bad.numel()} element(s) outside the [{self.rows}, {self.n}] window (ld {self.ld}) "
                                 f"changed; first at (row {row}, column {col}) = 0x{got:X} (guard pattern '{self.kind}')")


def assert_same_bits(a, b, what):
    """Two tensors of one shape and type hold the same bits (NaNs compare by payload)."""
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    ai, bi = bits(a.contiguous()), bits(b.contiguous())
    diff = torch.nonzero(ai != bi)
    if diff.shape[0]:
        idx = tuple(int(v) for v in diff[0])
        raise AssertionError(f"{what}: {diff.shape[0]} of {ai.numel()} element(s) differ in their bits; first at {idx}: "
                             f"{a[idx].item()!r} vs {b[idx].item()!r}")
