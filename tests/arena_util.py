"""The poisoned arena of the learner-kernel bounds tests (tests/test_learner_kernel_bounds.py): a helper, no test in it.

One byte tensor per test case, carved by a bump allocator into

    [slack | band | operand | band | band | operand | band | ... | slack]

Every operand of a launch lives inside it, so an access past an operand's end lands in memory the test owns and looks at:
  * bands and slack carry a fill that must come back bit-identical (a stray STORE shows as a changed byte);
  * around f32 operands the fill is a quiet NaN (a stray LOAD that reaches the arithmetic shows as a NaN in an output, also when the
    kernel "masks" it by a multiplication with 0); around integer operands it is a caller-given value outside the operand's domain that
    is harmless as an index (the harness must never turn a kernel bug into a wild address);
  * outputs are pre-filled with a SECOND NaN pattern, so "never written" and "written with poison" can be told apart.
Band width: at least 16 rows of the operand it guards and at least 64 KiB; the outer slack is 1 MiB at both ends -- any overrun a
tile-granular kernel can plausibly make stays inside the arena.  The arena provokes nothing.

Pointers are raw (`Region.ptr`): the calls go through abi.load_library(), not through ops.py, whose th.empty outputs are what this
bypasses.  `Arena("cpu")` keeps the bytes on the host (self-test and reference experiments)."""
import numpy as np
import torch as th

POISON_F32 = 0x7FC0DEAD          # quiet NaN: surroundings of f32 operands, slack
PREFILL_F32 = 0x7FE0BEEF         # another quiet NaN: outputs before the launch
BAND_MIN = 64 * 1024
SLACK = 1 << 20
ARENA_MAX = 64 << 20
TILE_ROWS = 16


def _pattern(nbytes, word):
    """nbytes of the little-endian 32-bit pattern `word`, phase-locked to offset 0 of the region it fills"""
    return np.frombuffer(np.full((nbytes + 3) // 4, word, dtype="<u4").tobytes(), dtype=np.uint8)[:nbytes]


class Region:
    """One operand: [start, start + nbytes) of the arena with a band on either side."""

    def __init__(self, arena, name, start, shape, dtype, band, kind, written):
        self.arena, self.name, self.start, self.shape, self.dtype = arena, name, start, tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.band, self.kind, self.written = band, kind, written          # kind: "in", "out" or "inout"

    @property
    def ptr(self):
        """device address (the first use seals the arena and uploads it)"""
        return self.arena._base() + self.start

    def array(self):
        """the operand as it is in the arena now (after check(): as the launch left it)"""
        raw = self.arena._download()[self.start:self.start + self.nbytes]
        return np.frombuffer(raw.tobytes(), dtype=self.dtype).reshape(self.shape)


class ArenaError(AssertionError):
    pass


class Arena:
    def __init__(self, device="cuda"):
        self.device = th.device(device)
        self.parts = [_pattern(SLACK, POISON_F32)]           # host mirror, concatenated when sealed
        self.used = SLACK
        self.regions = []
        self.mirror = None
        self.buf = None
        self._got = None

    # ---- carving ---------------------------------------------------------------------------------------------------------------
    def _carve(self, name, shape, dtype, content, align, offset_in_16, fill, row_bytes, kind, written):
        assert self.buf is None, "the arena is sealed (a pointer was taken)"
        assert offset_in_16 in (0, 4, 8, 12) and align in (1, 4, 8, 16)
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if row_bytes is None:
            row_bytes = (int(shape[-1]) if len(shape) > 1 else 1) * dtype.itemsize       # (a 1-D operand has no rows: one element)
        band = max(BAND_MIN, TILE_ROWS * row_bytes)
        band = (band + 15) & ~15
        if fill is None:
            assert dtype == np.float32, "integer / byte operands name their own harmless fill"
            pre = _pattern(band + 64, POISON_F32)
        else:
            pre = np.frombuffer(np.full((band + 64) // dtype.itemsize, fill, dtype=dtype).tobytes(), dtype=np.uint8)
        # leading band, then the operand at (16-byte boundary + offset_in_16) or at `align`
        start = self.used + band
        if offset_in_16 or align == 16:
            start = ((start + 15) & ~15) + offset_in_16
        else:
            start = (start + align - 1) // align * align
        lead = start - self.used
        self.parts.append(pre[pre.size - lead:])             # whole elements of the fill end where the operand starts
        self.parts.append(content)
        self.parts.append(pre[:band])
        reg = Region(self, name, start, shape, dtype, band, kind, written)
        reg.lead = lead
        self.used = start + nbytes + band
        assert self.used + SLACK <= ARENA_MAX, "arena over %d MiB" % (ARENA_MAX >> 20)
        self.regions.append(reg)
        return reg

    def place(self, name, array, align=4, offset_in_16=0, fill=None, row_bytes=None, inout=False):
        """copy a host array in (an input; inout: the launch also writes it).  fill: the value of the array's dtype its bands carry
        (default: the f32 NaN poison)."""
        array = np.ascontiguousarray(array)
        content = np.frombuffer(array.tobytes(), dtype=np.uint8)
        return self._carve(name, array.shape, array.dtype, content, align, offset_in_16, fill, row_bytes, "inout" if inout else "in", None)

    def reserve(self, name, shape, dtype=np.float32, align=4, offset_in_16=0, fill=None, row_bytes=None, written=True):
        """room for an output, pre-filled with PREFILL_F32.  written: True (every element), False (none: must keep the pre-fill) or a
        bool array of `shape` saying which elements the contract writes; None: no such rule (byte outputs, whose values may equal the
        pre-fill: the caller compares them with their expected values)."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if fill is None and dtype != np.float32:
            fill = np.frombuffer(_pattern(8, POISON_F32).tobytes(), dtype=dtype)[0]   # (an output's surroundings are never read as indices)
        return self._carve(name, shape, dtype, _pattern(nbytes, PREFILL_F32), align, offset_in_16, fill, row_bytes, "out", written)

    # ---- device side -----------------------------------------------------------------------------------------------------------
    def _base(self):
        if self.buf is None:
            self.parts.append(_pattern(SLACK, POISON_F32))
            self.mirror = np.concatenate(self.parts)
            self.parts = None
            assert self.mirror.size == self.used + SLACK
            self.buf = th.from_numpy(self.mirror.copy()).to(self.device)
            if self.device.type == "cuda":
                th.cuda.synchronize()
        return self.buf.data_ptr()

    def raw(self):
        """the arena's bytes as a writable numpy view (CPU arenas: the self-test writes through it)"""
        assert self.device.type == "cpu"
        self._base()
        return self.buf.numpy()

    def _download(self):
        if self._got is None:
            self._base()
            if self.device.type == "cuda":
                th.cuda.synchronize()
            self._got = self.buf.cpu().numpy().copy()
        return self._got

    # ---- the verdict -----------------------------------------------------------------------------------------------------------
    def check(self, allow_nan=()):
        """after the launch: every byte outside the outputs is bit-identical to what was uploaded (bands, slack AND inputs); every
        output element differs from the pre-fill where the contract writes it and still IS the pre-fill where it does not; no NaN
        in any f32 / f64 output (allow_nan: names of outputs exempt from the NaN rule)."""
        self._got = None
        got, exp = self._download(), self.mirror
        pos = 0
        for reg in self.regions + [None]:
            end = self.used + SLACK if reg is None else reg.start
            bad = np.flatnonzero(got[pos:end] != exp[pos:end])
            if bad.size:
                raise ArenaError(self._where(pos + int(bad[0]), reg))
            if reg is None:
                break
            seg = slice(reg.start, reg.start + reg.nbytes)
            if reg.kind == "in":
                bad = np.flatnonzero(got[seg] != exp[seg])
                if bad.size:
                    raise ArenaError("input operand %s was written at byte offset %d" % (reg.name, int(bad[0])))
            else:
                val = np.frombuffer(got[seg].tobytes(), dtype=reg.dtype).reshape(reg.shape)
                if reg.kind == "out" and reg.written is not None:
                    pre = np.frombuffer(exp[seg].tobytes(), dtype=reg.dtype).reshape(reg.shape)
                    same = val.view(_bits(reg.dtype)) == pre.view(_bits(reg.dtype))
                    w = np.broadcast_to(np.asarray(reg.written, dtype=bool), reg.shape)
                    if (same & w).any():
                        raise ArenaError("output %s: element %s keeps the pre-fill (never written)" % (reg.name, _first(same & w)))
                    if (~same & ~w).any():
                        raise ArenaError("output %s: element %s is outside the written set and was written" % (reg.name, _first(~same & ~w)))
                    val = np.where(w, val, 0) if reg.dtype.kind == "f" else val
                if reg.dtype.kind == "f" and reg.name not in allow_nan and np.isnan(val).any():
                    raise ArenaError("output %s: NaN at element %s (poison reached the arithmetic)" % (reg.name, _first(np.isnan(val))))
            pos = reg.start + reg.nbytes

    def _where(self, off, nxt):
        """which band / slack holds arena byte `off` (nxt: the region that follows the scanned gap, None = the tail)"""
        for reg in self.regions:
            if reg.start - reg.lead <= off < reg.start:
                return "band BEFORE %s changed, %d bytes before its start" % (reg.name, reg.start - off)
            e = reg.start + reg.nbytes
            if e <= off < e + reg.band:
                return "band AFTER %s changed at byte offset %d past its end" % (reg.name, off - e)
        return "slack %s changed at arena offset %d" % ("before the first operand" if off < SLACK else "behind the last operand", off)


def _bits(dtype):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]


def _first(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def selftest_case():
    """A small CPU arena after a correct host-side "kernel" (y[:, :3] = 2 x): (arena, x, ids, y, raw bytes, y view, x view with one band
    element on either side)."""
    a = Arena("cpu")
    x = a.place("x", np.arange(8, dtype=np.float32), offset_in_16=4)
    ids = a.place("ids", np.arange(4, dtype=np.int64), align=8, fill=7)
    w = np.ones((2, 4), dtype=bool); w[:, 3] = False
    y = a.reserve("y", (2, 4), written=w)
    assert x.ptr % 16 == 4 and ids.ptr % 8 == 0 and y.ptr % 4 == 0
    raw = a.raw()
    yv = raw[y.start:y.start + y.nbytes].view(np.float32).reshape(2, 4)
    xv = raw[x.start - 4:x.start + x.nbytes + 4].view(np.float32)
    yv[:, :3] = xv[1:9].reshape(2, 4)[:, :3] * 2
    return a, x, ids, y, raw, yv, xv


def _past_end(a, x, ids, y, raw, yv, xv): raw[y.start + y.nbytes] ^= 1
def _before(a, x, ids, y, raw, yv, xv): raw[y.start - 1] ^= 1
def _read_through(a, x, ids, y, raw, yv, xv): yv[1, 2] = xv[8] * 0.0 + xv[9] * 0.0      # "masked" by a multiply: x[7] * 0 + band * 0
def _unwritten(a, x, ids, y, raw, yv, xv): yv[0, 1] = np.frombuffer(_pattern(4, PREFILL_F32).tobytes(), dtype=np.float32)[0]
def _outside(a, x, ids, y, raw, yv, xv): yv[0, 3] = 1.0
def _input_written(a, x, ids, y, raw, yv, xv): raw[ids.start + 3] = 9
def _slack(a, x, ids, y, raw, yv, xv): raw[-5] = 0


# every way a case can go wrong -> the text check() must report (tests/test_arena_util.py: each check must be able to fail)
SELFTEST_FAULTS = {
    "write one byte past a reserved output": (_past_end, "band AFTER y changed at byte offset 0"),
    "write one byte before an output": (_before, "band BEFORE y changed, 1 bytes before"),
    "read-through of one poisoned f32": (_read_through, "output y: NaN at element (1, 2)"),
    "output element never written": (_unwritten, "output y: element (0, 1) keeps the pre-fill"),
    "write outside the written set": (_outside, "output y: element (0, 3) is outside the written set"),
    "input operand written": (_input_written, "input operand ids was written at byte offset 3"),
    "slack written": (_slack, "slack behind the last operand"),
}
