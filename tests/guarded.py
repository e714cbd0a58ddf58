"""Guard-band buffers for tests that call the C ABI directly (tests/test_gpu_guard.py; tests/test_guarded_cpu.py proves on the
CPU that every check below has teeth).

include/mink_hip.h: the caller owns every buffer, every scratch buffer travels with its size, every feature matrix has a leading
dimension.  A `Guarded` is one such buffer laid out inside memory the test owns,

    [ front band | payload | back band ]

all of it pre-filled with a sentinel, so that after the call three things can be asked bit for bit: the bands are untouched (no
store outside the buffer), every element the header says the call writes no longer holds the sentinel (no skipped tail), and
every other payload element -- pad columns of a matrix with ld > C, rows an accumulate or scatter does not visit, statistics
rows past the count the call reported -- holds exactly what it held before.

The payload starts 256-byte aligned -- or, with `skew`, that many bytes behind a 256-byte boundary, for the branch of a host
lane decision that an unaligned pointer takes -- and the back band begins at the first byte after it (no rounding slack: slack
would hide an overrun of a few bytes).  Each band is one full output tile of the widest kernel, 128 rows x leading dimension x 4 bytes, and
never under 64 KiB.  Float sentinels are quiet NaNs with a marker payload, so a NaN a kernel computed is not mistaken for
"untouched" and an input wrapped by `Guarded.input` poisons every result that an out-of-extent or pad-column read gets into, even
multiplied by zero."""
import torch

ALIGN = 256
MIN_BAND = 64 << 10
TILE_ROWS = 128  # BM / WROWS: rows of the tallest output tile in csrc/

# little-endian byte images of one sentinel element
_F32 = (0x7FC0BEEF).to_bytes(4, "little")
_SENTINEL = {
    torch.float32: _F32,
    torch.float64: (0x7FF8BEEF7FC0BEEF).to_bytes(8, "little"),
    torch.bfloat16: (0x7FDE).to_bytes(2, "little"),
    torch.float16: (0x7EDE).to_bytes(2, "little"),
    torch.int32: (0x5A5A5A5A).to_bytes(4, "little"),
    torch.int64: (0x5A5A5A5A5A5A5A5A).to_bytes(8, "little"),
    torch.uint8: b"\x5a",
}


def _prod(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class GuardError(AssertionError):
    pass


class Guarded:
    """One guarded buffer.

    shape_or_bytes : the payload's shape in elements of `dtype` (a matrix with a leading dimension is (n, ld)), or an int = a
                     size in BYTES (a workspace: `*_workspace_bytes()` exactly; the payload is then flat)
    cols           : logical columns of a (n, ld) matrix, ld > cols leaves pad columns (default: all)
    written        : the elements the call must write -- True / None = every logical element, False = none (an input, or a
                     buffer the call must leave alone), a boolean tensor of the payload's or the logical shape, or "any" = a
                     workspace: the call may write any part of the payload or none, only the bands are checked
    init           : values the logical elements hold before the call (accumulate and scatter targets, inputs); anything else
                     holds the sentinel.  `pad` overrides the sentinel of the pad columns (a finite value for an entry point
                     whose contract asks for finite pads).
    skew           : bytes (a multiple of the element size, below 256) between a 256-byte boundary and the payload's first
                     element: skew=4 gives a float pointer that is not 16-byte aligned.  The bands still end and begin at the
                     payload's first and last byte, and the sentinel pattern stays element-aligned."""

    def __init__(self, shape_or_bytes, dtype=torch.float32, device="cpu", written=None, init=None, cols=None, pad=None, name="buffer",
                 skew=0):
        self.name, self.dtype, self.device = name, dtype, torch.device(device)
        self.item = torch.empty((), dtype=dtype).element_size()
        if isinstance(shape_or_bytes, int):
            self.nbytes = int(shape_or_bytes)
            self.shape = (self.nbytes // self.item,)
            self.typed = self.nbytes % self.item == 0
        else:
            self.shape = tuple(int(s) for s in shape_or_bytes)
            self.nbytes, self.typed = _prod(self.shape) * self.item, True
        ld = self.shape[-1] if len(self.shape) > 1 else 0
        self.cols = ld if cols is None else int(cols)
        assert len(self.shape) < 2 or 0 <= self.cols <= ld, (self.cols, ld)
        band = max(MIN_BAND, TILE_ROWS * max(ld, 1) * 4)
        self.band = -(-band // ALIGN) * ALIGN
        self.skew = int(skew)
        assert 0 <= self.skew < ALIGN and self.skew % self.item == 0, (self.skew, self.item)
        total = 2 * self.band + self.nbytes
        raw = torch.empty(total + 2 * ALIGN, dtype=torch.uint8, device=self.device)
        start = (-raw.data_ptr()) % ALIGN + self.skew
        self.buf = raw[start : start + total]
        assert (self.buf.data_ptr() + self.band) % ALIGN == self.skew
        pat = torch.tensor(list(_SENTINEL[dtype]), dtype=torch.uint8)
        self.buf.copy_(pat.repeat(-(-total // len(pat)))[:total].to(self.device))  # (the band is a multiple of every item size)
        self.sentinel = pat.to(self.device)
        if self.typed and self.nbytes:
            self.t = self.buf[self.band : self.band + self.nbytes].view(dtype).view(self.shape)
        else:
            self.t = self.buf[self.band : self.band + self.nbytes]
        if pad is not None and self.cols < ld:
            self.t[..., self.cols :] = pad
        if init is not None:
            init = torch.as_tensor(init)
            dst = self.t if tuple(init.shape) == self.shape else self.logical()
            dst.copy_(init.to(device=self.device, dtype=dtype))
        self.free = isinstance(written, str) and written == "any"
        self.written = None if self.free else self._mask(written)
        self.before = self.buf.clone()

    # ---------------------------------------------------------------------------------------------------------- construction
    @classmethod
    def input(cls, tensor, ld=None, pad=None, name="input", skew=0):
        """An operand the call only reads: `tensor` ([n, C] or any shape) inside NaN bands at row pitch `ld` >= C, its pad columns
        NaN too (`pad`: a finite value instead), and after the call not one byte of it may differ."""
        tensor = tensor.detach()
        if ld is None or tensor.dim() != 2:
            return cls(tuple(tensor.shape), tensor.dtype, tensor.device, written=False, init=tensor, name=name, skew=skew)
        n, c = tensor.shape
        assert ld >= c
        return cls((n, ld), tensor.dtype, tensor.device, written=False, init=tensor, cols=c, pad=pad, name=name, skew=skew)

    def _mask(self, written):
        n = _prod(self.shape)
        m = torch.zeros(self.shape, dtype=torch.bool, device=self.device)
        if written is None or written is True:
            if len(self.shape) > 1:
                m[..., : self.cols] = True
            else:
                m[:] = True
        elif written is not False:
            written = torch.as_tensor(written, dtype=torch.bool).to(self.device)
            if tuple(written.shape) == self.shape:
                m.copy_(written)
            else:
                m[..., : self.cols].copy_(written)
        assert m.numel() == n
        return m

    # --------------------------------------------------------------------------------------------------------------- access
    @property
    def ptr(self):
        return self.buf.data_ptr() + self.band

    def logical(self):
        """The payload without its pad columns (a view)."""
        return self.t[..., : self.cols] if len(self.shape) > 1 else self.t

    def whole(self):
        """(flat typed view of the whole allocation, element index of the payload's first element): what a deliberately wrong
        fake kernel of tests/test_guarded_cpu.py needs to write outside the payload."""
        assert self.typed
        return self.buf.view(self.dtype), self.band // self.item

    def set_written(self, written):
        """The mask, when it is only known after the call (statistics rows: the call reports how many it wrote)."""
        self.written = self._mask(written)

    # ---------------------------------------------------------------------------------------------------------------- check
    def _fail(self, what, diff, base):
        idx = torch.nonzero(diff.flatten())
        raise GuardError(f"{self.name}: {what}: first offending byte at offset {int(idx[0]) + base} from the payload start "
                         f"(payload {self.nbytes} bytes, shape {self.shape}, cols {self.cols}), {idx.numel()} byte(s) differ")

    def check(self):
        """After torch.cuda.synchronize(): bands bit-identical to the sentinel, no `written` element still the sentinel, every
        other payload element as it was before the call."""
        b, e = self.band, self.band + self.nbytes
        diff = self.buf != self.before
        if bool(diff[:b].any()):
            self._fail("front band overwritten", diff[:b], -b)
        if bool(diff[e:].any()):
            self._fail("back band overwritten", diff[e:], self.nbytes)
        if self.free or not self.typed or self.nbytes == 0:
            return self
        per = (self.buf[b:e].view(-1, self.item) == self.sentinel).all(1)  # element still holds the sentinel
        w = self.written.flatten()
        stale = per & w
        if bool(stale.any()):
            self._fail("an element the call must write still holds the sentinel (never stored, or computed from a sentinel it read)", stale[:, None].expand(-1, self.item), 0)
        touched = diff[b:e].view(-1, self.item) & ~w[:, None]
        if bool(touched.any()):
            self._fail("an element the call must not write has changed", touched, 0)
        return self


def check_all(*bufs):
    for g in bufs:
        if g is not None:
            g.check()


def assert_finite(t, name="result"):
    """Every element finite: a result computed from in-range inputs only (the bands and pad columns of a Guarded.input are NaN)."""
    bad = ~torch.isfinite(t)
    if bool(bad.any()):
        idx = torch.nonzero(bad.flatten())
        raise GuardError(f"{name}: {idx.numel()} non-finite element(s), first at flat index {int(idx[0])}: a pad-column or "
                         "out-of-extent read got into the result")
