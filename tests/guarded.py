"""Guard-banded buffers for the EM entry points.

Arena: ONE allocation filled with a poison word, from which every buffer a test hands to the library is carved -- exactly
prod(shape) * itemsize bytes, at an address = 16 (mod 256) (the alignment include/vaenmf.h promises and no better), with at
least max(64 KiB, 32 rows) of poison before and after it.  An overrun of up to 32 rows lands in memory the test inspects
and cannot fault.  check() compares every guard bitwise; snapshot() / unchanged() do the same for buffers a call may only
read.  Works on CPU tensors too (tests/test_guarded_cpu.py).

GuardedEngine: a BatchEngine whose buffers come from an arena and whose free padding -- what the header calls `ignored`:
bins F..Fs-1 of X2 and Vb, unused sample rows of Zs, columns L..Lp-1 of the replay draws -- is poison instead of the
zeros bind() leaves there."""
import numpy as np
import torch

from vaenmf._lib import check, lib
from vaenmf.engine import BatchEngine, _ptr, _stream

# a quiet NaN with a payload, and 1e30f (0x7149F2CA): v_max / fmaxf and comparisons swallow a NaN and would hide a padding
# value that is used; 1e30 is finite, survives them, and squares to +inf
POISON = {"nan": 0x7FC0A5A5, "1e30": 0x7149F2CA}
MIN_GUARD, GUARD_ROWS, ALIGN, RESIDUE = 64 * 1024, 32, 256, 16


def _i32(word):
    return int(np.array([word], np.uint32).view(np.int32)[0])


def bits(t):
    """Integer view of a float tensor (any strides): comparisons on it are bitwise, NaN included."""
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b).to(a.device)))


class GuardError(AssertionError):
    pass


class Arena:
    def __init__(self, nbytes, poison, device="cpu"):
        self.word = _i32(POISON[poison] if isinstance(poison, str) else poison)
        self.raw = torch.empty(int(nbytes) + ALIGN, dtype=torch.uint8, device=device)
        base = (-self.raw.data_ptr()) % ALIGN                        # offsets below count from a 256-byte boundary
        self.size = int(nbytes) // 4 * 4
        self.mem = self.raw[base:base + self.size]
        self.words = self.mem.view(torch.int32)
        self.words.fill_(self.word)
        self.is_guard = torch.ones(self.size // 4, dtype=torch.bool, device=device)
        self.bufs = {}                                               # name -> dict(off, nbytes, row, rows, guard, view)
        self.order = []
        self.cursor = 0
        self._snap = {}

    # ------------------------------------------------------------------ carving
    def carve(self, name, shape, dtype):
        assert name not in self.bufs, name
        shape = tuple(int(v) for v in shape)
        item = torch.empty(0, dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        assert nbytes > 0 and nbytes % 4 == 0, (name, shape)
        row = nbytes // shape[0]                                     # bytes of one row (one frame, one utterance, one step)
        guard = max(MIN_GUARD, GUARD_ROWS * row)
        off = self.cursor + guard
        off += (RESIDUE - off) % ALIGN                               # = 16 (mod 256): 16-byte aligned and not 32
        if off + nbytes + guard > self.size:
            raise MemoryError("arena of %d bytes is full at %r (%d bytes + 2 guards of %d)" % (self.size, name, nbytes, guard))
        view = self.mem[off:off + nbytes].view(dtype).view(shape)
        self.is_guard[off // 4:(off + nbytes) // 4] = False
        self.bufs[name] = dict(off=off, nbytes=nbytes, row=row, rows=shape[0], guard=guard, view=view)
        self.order.append(name)
        self.cursor = off + nbytes + guard                           # the arena ends with this guard
        return view

    def view(self, name):
        return self.bufs[name]["view"]

    def name_of(self, t):
        off = t.data_ptr() - self.mem.data_ptr()
        return next(n for n in self.order if self.bufs[n]["off"] == off)

    def poison(self, t):
        """Fill a view (any strides) of a carved float32 buffer with the poison word."""
        assert t.element_size() == 4
        bits(t).fill_(self.word)

    def is_poison(self, t):
        return bool((bits(t) == self.word).all())

    # ------------------------------------------------------------------ checks
    def _where(self, byte):
        """(buffer, side, offset, row) of a damaged guard byte: the nearest buffer whose guard holds it."""
        best = None
        for name in self.order:
            b = self.bufs[name]
            if b["off"] - b["guard"] <= byte < b["off"]:
                d = b["off"] - byte                                  # bytes before the buffer's first
                cand = (d, name, "before", -d, -((d + b["row"] - 1) // b["row"]))
            elif b["off"] + b["nbytes"] <= byte < b["off"] + b["nbytes"] + b["guard"]:
                d = byte - b["off"] - b["nbytes"]
                cand = (d, name, "after", d, b["rows"] + d // b["row"])
            else:
                continue
            if best is None or cand[0] < best[0]:
                best = cand
        return best[1:] if best else ("(no buffer)", "slack", byte, -1)

    def check(self, what=""):
        """Every guard still holds the poison word, bit for bit."""
        bad = (self.words != self.word) & self.is_guard
        if not bool(bad.any()):
            return
        first = int(bad.nonzero()[0]) * 4
        name, side, off, row = self._where(first)
        raise GuardError("%s: guard %s buffer %r damaged: first at byte %+d %s (row %d of its %d rows of %d bytes); %d words in all"
                         % (what, side, name, off, "from its start" if side == "before" else "past its end", row,
                            self.bufs[name]["rows"] if name in self.bufs else 0, self.bufs[name]["row"] if name in self.bufs else 0,
                            int(bad.sum())))

    def snapshot(self, names):
        self._snap = {n: self.mem[self.bufs[n]["off"]:self.bufs[n]["off"] + self.bufs[n]["nbytes"]].view(torch.int32).clone() for n in names}

    def unchanged(self, names=None, what=""):
        """The buffers of the last snapshot (or those of them in `names`) hold the bits they held then."""
        for n in (self._snap if names is None else names):
            b = self.bufs[n]
            bad = self.mem[b["off"]:b["off"] + b["nbytes"]].view(torch.int32) != self._snap[n]
            if bool(bad.any()):
                first = int(bad.nonzero()[0]) * 4
                raise GuardError("%s: read-only buffer %r changed: first at byte %d (row %d of its %d rows of %d bytes); %d words in all"
                                 % (what, n, first, first // b["row"], b["rows"], b["row"], int(bad.sum())))


class GuardedEngine(BatchEngine):
    """A BatchEngine whose every buffer is carved from `arena`; after bind() the padding the header leaves free is poison."""

    def __init__(self, arena, *args, **kw):
        self.arena, self._names, self.last = arena, {}, None
        super().__init__(*args, **kw)

    def _empty(self, shape, dtype, name=None):
        n = self._names[name] = self._names.get(name, 0) + 1
        self.last = name if n == 1 else "%s#%d" % (name, n)
        return self.arena.carve(self.last, shape, dtype)            # starts as poison, as every output does

    def bind(self, frame_counts, Rcap, seeds=None):
        super().bind(frame_counts, Rcap, seeds)
        self.poison_free_padding()
        return self

    def poison_free_padding(self, samples=0):
        """bind() zeroed X, X2, W, Ht, Z, Zs.  What the header leaves free goes back to poison: bins F..Fs-1 of X2, sample
        rows r >= samples of Zs.  What it requires to be zero stays zero (X: see poison_x_padding): the padding of W and Ht, columns L..Lp-1 of
        Z and of the sample rows in use."""
        if self.Fs > self.F:
            self.arena.poison(self.X2[:, self.F:])
            self.poison_x_padding()
        if self.Rcap > samples:
            self.arena.poison(self.Zs[:, samples:])

    def poison_x_padding(self):
        """X, bins F..Fs-1: `must be zero`, and the header adds that any finite value still gives S_hat / N_hat their zero
        padding: the finite poison word goes there, the NaN word does not."""
        if self.Fs > self.F and np.isfinite(np.array([self.arena.word], np.int32).view(np.float32)[0]):
            self.arena.poison(self.X[:, self.F:])

    def carve_like(self, name, host):
        """A host array as an arena buffer of exactly its size."""
        host = np.ascontiguousarray(host)
        t = self.arena.carve(name, host.shape, torch.from_numpy(host).dtype)
        t.copy_(torch.from_numpy(host))
        return t

    def load_spectrogram(self, X):
        """The copy of BatchEngine.set_spectrogram without its vaenmf_power_spec (X's padding: must be zero)."""
        Xc = np.zeros((self.NT, self.Fs), np.complex64)
        for u, x in enumerate(X):
            Xc[self.utt_slice(u), :self.F] = x
        self.X.copy_(torch.from_numpy(Xc.view(np.float32).reshape(self.NT, self.Fs, 2)))
        self.poison_x_padding()


def power_spec(eng):
    """The library call of BatchEngine.set_spectrogram alone."""
    check(lib().vaenmf_power_spec(_ptr(eng.X), _ptr(eng.X2), eng.NT * eng.Fs, _stream()))


def make_guarded_engine(arena, params, F, K, counts, Rcap, precision="bf16x3", seeds=None):
    """tests/em_support.make_engine on an arena: exact buffers (max_frames = NT, max_utts = U), poisoned free padding."""
    from em_support import dec_list
    eng = GuardedEngine(arena, F, K, dec_list(params), precision=precision, max_frames=sum(counts), max_utts=len(counts),
                        z_dim=int(params["encoder.sample.mu.weight"].shape[0]))
    return eng.bind(counts, Rcap=Rcap, seeds=seeds)
