"""One allocation, carved views, checked afterwards: the containment harness of tests/test_gpu_containment_*.py.

The parity tests compare VALUES; this module checks WHERE an entry point touches memory.  An Arena is one tensor filled with
a position-dependent 32-bit canary.  Inputs and outputs of the call under test are contiguous views carved out of it at a
chosen alignment, with guard bands on both sides of every view.  After the call one device-to-host copy of the whole arena
shows
  * a write outside the declared outputs (a guard word, the slack or an input no longer holds what was put there),
  * a declared output word that was never written (it still holds the canary of its position), and
  * through Arena.twin(), a READ outside the declared inputs: the call runs once per poison kind (canary, AIR_DIST, a distance
    deep inside the surface, NaN) over the same input bits, and a kernel that reads beyond an input sees other bits and so
    produces other outputs in the two runs.
Every access of a test, right or wrong by up to a band, stays inside the arena's own allocation.

The same class runs over CPU tensors (device="cpu"): tests/test_arena_cpu.py drives it with numpy "kernels" that overrun,
underrun, skip, clobber and peek on purpose, which is the only place a wrong kernel is simulated."""
import numpy as np
import torch

import oracle_binding

CANARY_TAG = 0xA5000000   # as float32: -5.55e-17 * (1 + index / 2^23) -- finite, negative, never AIR_DIST, never -7.0
CANARY_MASK = 0x00FFFFFF
MIN_BAND = 64 * 1024      # the largest store unit is a workgroup's 4 KiB; 64 KiB holds sixteen of them
BASE_ALIGN = 256          # the first byte of the arena is aligned to this, so that offsets decide alignments
POISON_KINDS = ("canary", "air", "hit", "nan")
AIR_BITS = int(np.float32(oracle_binding.AIR_DIST).view(np.uint32))
HIT_BITS = int(np.float32(-1.0).view(np.uint32))   # a distance far inside any surface: a march that reads it stops there
NAN_BITS = 0x7FC00000

_TORCH_DTYPES = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8,
                 np.dtype(np.uint32): torch.int32}


def canary_words(first_word, n):
    """The canary of words [first_word, first_word + n) of an arena, uint32."""
    return (np.arange(first_word, first_word + n, dtype=np.uint64) & CANARY_MASK).astype(np.uint32) | np.uint32(CANARY_TAG)


def band_for(*arrays):
    """max(64 KiB, two slices of the widest array): `arrays` are (shape, dtype) pairs or host arrays.  A slice is what one
    index of the leading axis spans in an array of three or more axes (a z slice of a texture or volume, one camera's image);
    point lists and other flat arrays have none.  The largest plausible index error, one row pair or one slice, then lands in a
    band, not in another view and not outside the arena."""
    band = MIN_BAND
    for a in arrays:
        shape, dtype = (a.shape, a.dtype) if hasattr(a, "shape") else a
        if len(shape) >= 3 and shape[0] > 0:
            band = max(band, 2 * int(np.prod(shape[1:])) * np.dtype(dtype).itemsize)
    return band + (-band) % BASE_ALIGN


def arena_bytes(band, *arrays):
    """Bytes an arena needs for these views (band_for()'s arguments) with `band` around each."""
    total = band + BASE_ALIGN
    for a in arrays:
        shape, dtype = (a.shape, a.dtype) if hasattr(a, "shape") else a
        total += int(np.prod(shape)) * np.dtype(dtype).itemsize + band + 2 * BASE_ALIGN
    return total


class Untouched:
    """expected[name] = Untouched(values, written[, nan_open][, undefined]): an expected array with masks, each a boolean array
    that broadcasts to `values`' shape.
      written    False where the contract leaves the words alone (unvisited voxels of a pass, rows outside [y0, y1), list
                 entries beyond the count): they must still hold what the view held before the call -- the canary for an
                 output(), the uploaded bits for an inout().
      nan_open   float32 words where a NaN that is expected AND a NaN that came out count as equal (a 0 / 0 whose sign and
                 payload the host's and the device's divide choose differently); a NaN on one side alone still differs.
      undefined  elements whose content the contract leaves open after the call (scratch memory, the order of a list that
                 atomics fill): they lie inside the view, so they may hold anything, and twin() does not compare them between
                 runs.  What surrounds them is held as ever."""

    def __init__(self, values, written=True, nan_open=False, undefined=False):
        self.values = np.ascontiguousarray(values)
        self.written = np.ascontiguousarray(np.broadcast_to(written, self.values.shape)).astype(bool)
        self.undefined = None if undefined is False else np.ascontiguousarray(np.broadcast_to(undefined, self.values.shape)).astype(bool)
        self.nan_open = None if nan_open is False else np.ascontiguousarray(np.broadcast_to(nan_open, self.values.shape)).astype(bool)


class Approx(Untouched):
    """expected[name] = Approx(values, atol[, written]): for the one kind of output whose reference is not bit-exact, the shaded
    colour planes of the march (the oracle's shading agrees to march_compare.RGBA_TOL, the 8-bit plane to one step).  Every
    written element must lie within atol of `values` AND no longer hold the canary; containment around the view, Untouched
    words and the bit-identity between twin() runs are checked as for every view."""

    def __init__(self, values, atol, written=True):
        super().__init__(values, written)
        self.atol = atol


class _View:
    def __init__(self, name, kind, offset, shape, dtype, initial):
        self.name, self.kind, self.offset, self.shape, self.dtype, self.initial = name, kind, offset, tuple(shape), np.dtype(dtype), initial
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.tensor = None

    @property
    def end(self):
        return self.offset + self.nbytes


class ArenaError(AssertionError):
    pass


class Arena:
    def __init__(self, nbytes, pattern="canary", band=MIN_BAND, device="cuda", poison_around="all"):
        """nbytes of `device` memory behind one allocation, every 32-bit word poisoned with `pattern` (POISON_KINDS).  `band`:
        bytes of guard below and above every view, band_for() of the arrays the test will carve -- check() verifies that.
        poison_around="inputs": repoison(kind) puts `kind` into the half bands next to input() views only and the canary
        everywhere else (the march: a distance deep inside the surface around the volumes, the canary around the images)."""
        assert poison_around in ("all", "inputs")
        self.poison_around = poison_around
        nbytes += (-nbytes) % 4
        assert pattern in POISON_KINDS and band >= MIN_BAND and band % BASE_ALIGN == 0
        assert nbytes // 4 <= CANARY_MASK + 1, "the canary's word index has 24 bits: an arena holds at most 64 MiB"
        self.nbytes, self.band, self.device, self.kind = int(nbytes), int(band), torch.device(device), pattern
        self._alloc = torch.empty(self.nbytes + BASE_ALIGN, dtype=torch.uint8, device=self.device)
        pad = (-self._alloc.data_ptr()) % BASE_ALIGN
        self.raw = self._alloc[pad:pad + self.nbytes]          # uint8, the arena
        self.words = self.raw.view(torch.int32)                # the same bytes as 32-bit words
        self.views = []
        self._cursor = 0
        self._covered = torch.zeros(self.nbytes, dtype=torch.bool, device=self.device)  # bytes inside a carved view
        self.repoison(pattern)

    # -- poison ---------------------------------------------------------------------------------------------------------------
    def _poison_host(self, kind):
        """The poison of every word of the arena, uint32 (what lies inside views is overwritten by their contents)."""
        n = self.nbytes // 4
        canary = canary_words(0, n)
        if kind == "canary":
            return canary
        w = np.full(n, {"air": AIR_BITS, "hit": HIT_BITS, "nan": NAN_BITS}[kind], np.uint32)
        if self.poison_around == "all":
            return w
        # each gap between two views is split in the middle; a half belongs to the view it touches
        near_input = np.zeros(n, bool)
        vs = sorted(self.views, key=lambda v: v.offset)
        for i, v in enumerate(vs):
            lo = 0 if i == 0 else (vs[i - 1].end + v.offset) // 2
            hi = self.nbytes if i == len(vs) - 1 else (v.end + vs[i + 1].offset) // 2
            if v.kind == "input":
                near_input[lo // 4:-(-hi // 4)] = True
        return np.where(near_input, w, canary)

    def _poison_device(self, kind):
        return torch.from_numpy(self._poison_host(kind).view(np.int32)).to(self.device)

    def repoison(self, kind):
        """Rewrite every byte that is not inside a carved view (guards and slack) with the poison `kind`."""
        assert kind in POISON_KINDS
        poison = self._poison_device(kind).view(torch.uint8)
        self.raw.copy_(torch.where(self._covered, self.raw, poison))
        self.kind = kind

    # -- carving --------------------------------------------------------------------------------------------------------------
    def _carve(self, name, kind, shape, dtype, align, misalign, initial):
        dtype = np.dtype(dtype)
        assert align in (1, 2, 4, 8, 16, 32, 64, 128) and 0 <= misalign and misalign % dtype.itemsize == 0
        assert name not in [v.name for v in self.views], f"view name {name!r} used twice"
        off = self._cursor + self.band
        off += (-off) % (2 * align)
        off += align            # a multiple of `align` that is no multiple of 2 * align: EXACTLY the requested alignment
        off += misalign
        v = _View(name, kind, off, shape, dtype, initial)
        if v.end + self.band > self.nbytes:
            raise ArenaError(f"arena of {self.nbytes} bytes is too small for view {name!r} ({v.nbytes} bytes at {off}) and its band")
        assert (self.raw.data_ptr() + off - misalign) % align == 0 and (misalign or (self.raw.data_ptr() + off) % (2 * align) != 0)
        self._cursor = v.end
        self._covered[v.offset:v.end] = True
        v.tensor = self.raw[v.offset:v.end].view(_TORCH_DTYPES[dtype]).view(v.shape)
        self.views.append(v)
        self._reset(v)
        return v.tensor

    def output(self, shape, dtype=np.float32, align=16, misalign=0, name=None):
        """A contiguous view the call under test writes.  It keeps the canary until then."""
        return self._carve(name or f"out{len(self.views)}", "output", shape, dtype, align, misalign, None)

    def input(self, host_array, align=16, misalign=0, name=None):
        """A contiguous view holding `host_array`'s bits, which the call under test must leave alone."""
        a = np.ascontiguousarray(host_array)
        return self._carve(name or f"in{len(self.views)}", "input", a.shape, a.dtype, align, misalign, a.copy())

    def inout(self, host_array, align=16, misalign=0, name=None):
        """A view the call under test updates in place (a texture during a pass, the vertices of mesh_postproc): uploaded like
        an input, checked like an output; Untouched words must hold the uploaded bits."""
        a = np.ascontiguousarray(host_array)
        return self._carve(name or f"io{len(self.views)}", "inout", a.shape, a.dtype, align, misalign, a.copy())

    def view(self, name):
        return next(v for v in self.views if v.name == name)

    def _initial_bytes(self, v):
        """What view v holds before the call, as host bytes."""
        if v.initial is not None:
            return v.initial.reshape(-1).view(np.uint8)
        w0, w1 = v.offset // 4, -(-v.end // 4)
        return canary_words(w0, w1 - w0).view(np.uint8)[v.offset - 4 * w0:v.offset - 4 * w0 + v.nbytes]

    def _reset(self, v):
        self.raw[v.offset:v.end].copy_(torch.from_numpy(self._initial_bytes(v).copy()))

    def reset(self, names=None):
        """Every view (or the named ones) back to its state before the call: inputs and inouts re-uploaded, outputs re-filled
        with the canary."""
        for v in self.views:
            if names is None or v.name in names:
                self._reset(v)

    # -- checking -------------------------------------------------------------------------------------------------------------
    def _blame(self, byte):
        """Where a byte outside every output lies, in words a person can act on."""
        inside = [v for v in self.views if v.offset <= byte < v.end]
        if inside:
            return f"in another view: {inside[0].kind} {inside[0].name!r} at byte {byte - inside[0].offset} of {inside[0].nbytes}"
        outs = [v for v in self.views if v.kind != "input"] or self.views
        if not outs:
            return f"arena byte {byte} (no view carved)"
        near = min(outs, key=lambda v: min(abs(byte - v.offset), abs(byte - (v.end - 1))))
        if byte < near.offset:
            return f"below view {near.name!r}: byte {byte - near.offset} relative to its start"
        return f"above view {near.name!r}: byte {byte - near.offset} relative to its start, {byte - near.end + 1} past its {near.nbytes} bytes"

    def poison_of(self, name, kind):
        """The poison `kind` of the bytes of view `name`, a uint8 tensor on the arena's device: what tests/stream_gate.py puts
        into an input before the real bits arrive late, and (kind "canary") into an output after an early store."""
        v = self.view(name)
        return torch.from_numpy(self._poison_host(kind).view(np.uint8)[v.offset:v.end].copy()).to(self.device)

    def bytes_of(self, name):
        """View `name` as the uint8 slice of the arena it is."""
        v = self.view(name)
        return self.raw[v.offset:v.end]

    def check(self, expected, raw=None):
        """One copy of the whole arena to the host, then: every byte outside the output views holds its poison (or, inside an
        input, the uploaded bits), and each output view equals expected[name] bit for bit (an ndarray, or Untouched).  Returns
        {name: the output's bytes} for comparisons between runs.  raw: a copy of self.raw taken earlier (on a stream, between
        other work) to be held to the same instead of the arena as it is now."""
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        got = (self.raw if raw is None else raw).cpu().numpy()
        assert got.shape == (self.nbytes,)
        need = band_for(*[(v.shape, v.dtype) for v in self.views])
        assert self.band >= need, f"arena band {self.band} is below the {need} bytes its widest view asks for"
        want = self._poison_host(self.kind).view(np.uint8).copy()
        is_output = np.zeros(self.nbytes, bool)
        for v in self.views:
            if v.kind == "input":
                want[v.offset:v.end] = self._initial_bytes(v)
            else:
                is_output[v.offset:v.end] = True
        bad = np.flatnonzero((got != want) & ~is_output)
        problems = []
        if bad.size:
            first = bad[:4]
            problems.append(f"{bad.size} byte(s) written outside the declared outputs (poison {self.kind!r}); first: " +
                            "; ".join(f"{self._blame(int(b))} (holds 0x{got[b]:02x}, expected 0x{want[b]:02x})" for b in first))
        missing = sorted(set(v.name for v in self.views if v.kind != "input") ^ set(expected))
        assert not missing, f"expected must name exactly the output views; differs in {missing}"
        results = {}
        for v in self.views:
            if v.kind == "input":
                continue
            e = expected[v.name]
            values, written = (e.values, e.written) if isinstance(e, Untouched) else (np.ascontiguousarray(e), None)
            assert values.shape == v.shape and values.dtype.itemsize == v.dtype.itemsize, \
                f"expected[{v.name!r}] is {values.dtype}{values.shape}, the view is {v.dtype}{v.shape}"
            want_v = values.reshape(-1).view(np.uint8).copy()
            before = self._initial_bytes(v)
            wmask = np.ones(v.nbytes, bool) if written is None else np.repeat(written.reshape(-1), v.dtype.itemsize)
            got_v = got[v.offset:v.end]
            if getattr(e, "undefined", None) is not None:
                open_bytes = np.repeat(e.undefined.reshape(-1), v.dtype.itemsize)
                want_v[open_bytes] = got_v[open_bytes]
                wmask = wmask | open_bytes          # (not "untouched" either)
                if v.kind == "output":              # ... nor held to differ from the canary
                    before = before.copy()
                    before[open_bytes] = ~got_v[open_bytes]
            if getattr(e, "nan_open", None) is not None:
                assert v.dtype.itemsize == 4
                both = e.nan_open.reshape(-1) & np.isnan(want_v.view(np.float32)) & np.isnan(got_v.copy().view(np.float32))
                want_v.view(np.uint32)[both] = got_v.copy().view(np.uint32)[both]
            if isinstance(e, Approx):
                # within atol where written, and no longer the canary (four bytes at a time: a float, a pixel of an 8-bit plane)
                assert values.dtype == v.dtype and v.nbytes % 4 == 0
                g = got_v.view(v.dtype).reshape(v.shape).astype(np.float64)
                far = e.written & ~(np.abs(g - values.astype(np.float64)) <= e.atol)  # (a NaN is far)
                if far.any():
                    first = [tuple(int(i) for i in ix) for ix in np.argwhere(far)[:4]]
                    problems.append(f"view {v.name!r}: {int(far.sum())} element(s) further than {e.atol} from the expected result; "
                                    f"first elements {first}: got {[float(g[i]) for i in first]}, expected {[float(values[i]) for i in first]}")
                stale4 = ((got_v == before) & wmask).reshape(-1, 4).all(axis=1)
                if v.kind == "output" and stale4.any():
                    problems.append(f"view {v.name!r}: {int(stale4.sum())} written word(s) still hold the canary: never written; first "
                                    f"byte offsets {[4 * int(k) for k in np.flatnonzero(stale4)[:4]]} of {v.nbytes}")
                want_v = got_v.copy()   # what is left to compare bit for bit: the untouched words, below
            if v.kind == "output" and not isinstance(e, Approx):
                # "written" and "stale" must not be confusable: no expected element may equal the canary of its position
                # (elements of four bytes; a single byte of an 8-bit image can always coincide)
                if v.dtype.itemsize == 4:
                    full = np.flatnonzero((wmask & (want_v == before)).reshape(-1, 4).all(axis=1))
                    assert not full.size, f"expected[{v.name!r}] equals the canary at element(s) {full[:4].tolist()}"
            want_v[~wmask] = before[~wmask]
            results[v.name] = got_v.copy()
            diff = np.flatnonzero(got_v != want_v)
            if diff.size:
                stale = int(np.count_nonzero((got_v[diff] == before[diff]) & wmask[diff]))
                touched = int(np.count_nonzero(~wmask[diff]))
                problems.append(f"view {v.name!r}: {diff.size} byte(s) differ from the expected result ({stale} still hold what the view "
                                f"held before the call: never written; {touched} lie where the contract leaves the view untouched); "
                                f"first byte offsets {[int(b) for b in diff[:4]]} of {v.nbytes} "
                                f"(elements {[tuple(int(i) for i in np.unravel_index(b // v.dtype.itemsize, v.shape)) for b in diff[:4]]})")
        if problems:
            raise ArenaError("\n".join(problems))
        return results

    def twin(self, run, expected, kinds=("canary", "nan")):
        """The read-set test: run() once per poison kind in a freshly re-poisoned arena over the same input bits, check() each
        time.  The outputs of all runs must be bit-identical to `expected` and so to each other: a kernel that reads past a
        declared input sees different bits in the runs."""
        assert len(kinds) >= 2 and all(k in POISON_KINDS for k in kinds)
        first = None
        for kind in kinds:
            self.reset()
            self.repoison(kind)
            run()
            try:
                got = self.check(expected)
            except ArenaError as e:
                raise ArenaError(f"with poison {kind!r} around the views:\n{e}") from None
            if first is None:
                first = got
            for name in got:   # implied by the two checks; kept so that a masked (Untouched) region is compared as well
                e = expected[name]
                same = first[name] == got[name]
                if getattr(e, "undefined", None) is not None:   # (what is undefined need not repeat between runs)
                    same = same | np.repeat(e.undefined.reshape(-1), self.view(name).dtype.itemsize)
                assert same.all(), f"view {name!r} differs between poison {kinds[0]!r} and {kind!r}"
        return first
