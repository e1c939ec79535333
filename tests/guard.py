"""Guarded device allocations: where do the kernels write?

The parity tests compare WHAT the kernels compute; `guarded_allocations` checks WHERE they write.  Inside the block every tensor the
factory functions hand out on `device` is a contiguous, 256-byte aligned view into a larger base with a band of BAND bytes in front
and one behind, both filled with a fixed non-zero byte pattern.  On exit (and on verify()) every band must still hold the pattern.

BAND is 16 KiB = 1024 threads x 16 B, the largest contiguous piece one workgroup of any kernel of the library stores: a kernel that
writes one row, one block or one chunk past its buffer lands in a band.  This is a condition, not a measurement: an overrun that
STRIDES beyond the band (a wild index, a whole-image offset) is out of reach, and so is every out-of-bounds READ -- a read leaves no
trace in memory.  What a read of uninitialised scratch does is probed from the other side: `poison` sets what the empty* allocations
start with, and the wrapped checks must still pass at their own bars.

    poison = "none"       the interior is left as allocated
             "float_nan"  floating tensors start as NaN (parity_cases.poisoned_empty)
             "bytes"      every dtype starts as the byte `byte` (0xFF, 0x5A) -- the host-emulated build ONLY: an uninitialised index read
                          from scratch has to show up as a CPU segfault, never as a wild access on a shared GPU (refused on a cuda device)
    zeros / ones / full and their _like / new_ forms keep their values in every mode.
Besides the factory functions the copies t.to(...), t.clone(), t.cuda() and t.contiguous() are served the same way when they make a new
tensor on the device outside an autograd graph: that is how the checks put the buffers a kernel updates in place on the device.

Pinned and other-device allocations pass through untouched.  The context keeps every base alive until it exits, so no guarded block
is recycled while a kernel of the block might still write through a stale pointer."""
import sys

import torch

BAND = 16384          # bytes per band: 1024 threads x 16 B
ALIGN = 256           # the hosts and the library refuse or clone misaligned tensors, and a clone would escape the guard

_MODULE_FACTORIES = ("empty", "empty_like", "zeros", "zeros_like", "ones", "full", "full_like")
_TENSOR_FACTORIES = ("new_empty", "new_zeros", "new_full")
#: copies: t.to(device), t.clone(), t.cuda(), t.contiguous() -- how the checks put their inputs and the buffers a kernel updates in place (the
#: parameters and moments of an optimiser step, the rows of an exchange) on the device.  Guarded when the call made a NEW tensor on the device
#: that is not part of an autograd graph
_TENSOR_COPIES = ("to", "clone", "cuda", "contiguous")
_UNINITIALISED = ("empty", "empty_like", "new_empty")


def _pattern(device):
    """The band contents: BAND bytes, none of them zero, no two neighbours equal."""
    i = torch.arange(BAND, dtype=torch.int64)
    return ((i * 37 + 11) % 255 + 1).to(torch.uint8).to(device)


class Allocation:
    """One guarded allocation: (call site, dtype, shape, nbytes, fill) + the base that holds it."""
    __slots__ = ("site", "dtype", "shape", "nbytes", "fill", "base", "offset", "tensor", "factory")

    def __init__(self, site, dtype, shape, nbytes, fill, base, offset, tensor, factory):
        self.site, self.dtype, self.shape, self.nbytes, self.fill = site, dtype, shape, nbytes, fill
        self.base, self.offset, self.tensor, self.factory = base, offset, tensor, factory

    def record(self):
        return (self.site, self.dtype, self.shape, self.nbytes, self.fill)

    def bytes(self):
        """The interior as uint8 [nbytes] (a view of the base)."""
        return self.base[self.offset:self.offset + self.nbytes]

    def __repr__(self):
        return f"{self.factory} {tuple(self.shape)} {self.dtype} ({self.nbytes} bytes, fill {self.fill}) at {self.site}"


def _call_site():
    f = sys._getframe(2)
    while f is not None and f.f_code.co_filename == __file__:
        f = f.f_back
    if f is None:
        return "?"
    name = f.f_code.co_filename
    for marker in ("activesplat_amd", "tests", "oracle"):
        k = name.rfind("/" + marker + "/")
        if k >= 0:
            name = name[k + 1:]
            break
    return f"{name}:{f.f_lineno} ({f.f_code.co_name})"


class guarded_allocations:
    def __init__(self, device, poison="none", byte=0xFF):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if poison not in ("none", "float_nan", "bytes"):
            raise ValueError(f"guarded_allocations: poison = {poison!r}")
        if poison == "bytes" and self.device.type != "cpu":
            raise ValueError("guarded_allocations: poison='bytes' is for the host-emulated build only (an uninitialised index must fault on a CPU, not on a GPU)")
        self.poison, self.byte = poison, int(byte) & 0xFF
        self.allocations = []
        self._saved = None
        self._pat = None

    # ---- the allocation itself --------------------------------------------------------------------------------------------------------
    def _same_device(self, dev):
        if dev.type != self.device.type:
            return False
        return dev.type == "cpu" or dev.index == self.device.index

    def _serve(self, factory, plain, requires_grad):
        """plain: what the real factory returned (requires_grad stripped) -> the guarded stand-in, or `plain` itself when it passes through."""
        if not self._same_device(plain.device) or plain.is_pinned() or plain.layout != torch.strided or plain.is_quantized:
            return plain.requires_grad_(True) if requires_grad else plain
        real_empty = self._saved["empty"]
        nbytes = plain.numel() * plain.element_size()
        base = real_empty(nbytes + 2 * BAND + ALIGN, dtype=torch.uint8, device=plain.device)
        offset = BAND + (-(base.data_ptr() + BAND)) % ALIGN
        base[offset - BAND:offset].copy_(self._pat)
        base[offset + nbytes:offset + nbytes + BAND].copy_(self._pat)
        inner = base[offset:offset + nbytes]
        view = inner.view(plain.dtype).view(plain.shape) if plain.dtype != torch.uint8 else inner.view(plain.shape)
        fill = None
        if factory in _UNINITIALISED:
            if self.poison == "bytes":
                inner.fill_(self.byte)
                fill = self.byte
            elif self.poison == "float_nan" and plain.is_floating_point():
                if nbytes:
                    view.fill_(float("nan"))
                fill = "nan"
        else:
            view.copy_(plain)
            fill = "value"
        assert view.data_ptr() % ALIGN == 0 and view.is_contiguous()
        self.allocations.append(Allocation(_call_site(), plain.dtype, tuple(plain.shape), nbytes, fill, base, offset, view, factory))
        return view.requires_grad_(True) if requires_grad else view

    def _wrap(self, factory, real):
        def guarded(*a, **k):
            requires_grad = bool(k.pop("requires_grad", False))
            if k.get("out") is not None:
                return real(*a, **k)
            return self._serve(factory, real(*a, **k), requires_grad)
        guarded.__name__ = factory
        return guarded

    def _wrap_copy(self, name, real):
        def guarded(t, *a, **k):
            r = real(t, *a, **k)
            if r is t or not torch.is_tensor(r) or r.requires_grad or r.grad_fn is not None or r.is_sparse or \
                    (r.numel() and r.device == t.device and r.data_ptr() == t.data_ptr()):
                return r
            return self._serve(name, r, False)
        guarded.__name__ = name
        return guarded

    def __enter__(self):
        assert self._saved is None, "guarded_allocations is not re-entrant"
        self._pat = _pattern(self.device)
        self._saved = {n: getattr(torch, n) for n in _MODULE_FACTORIES}
        self._own = {n: n in torch.Tensor.__dict__ for n in _TENSOR_FACTORIES + _TENSOR_COPIES}
        self._saved_t = {n: getattr(torch.Tensor, n) for n in _TENSOR_FACTORIES + _TENSOR_COPIES}
        for n in _MODULE_FACTORIES:
            setattr(torch, n, self._wrap(n, self._saved[n]))
        for n in _TENSOR_FACTORIES:
            setattr(torch.Tensor, n, self._wrap(n, self._saved_t[n]))
        for n in _TENSOR_COPIES:
            setattr(torch.Tensor, n, self._wrap_copy(n, self._saved_t[n]))
        return self

    def _restore(self):
        if self._saved is None:
            return
        for n, f in self._saved.items():
            setattr(torch, n, f)
        for n, f in self._saved_t.items():
            if self._own[n]:
                setattr(torch.Tensor, n, f)
            else:
                delattr(torch.Tensor, n)
        self._saved = None

    def __exit__(self, etype, exc, tb):
        self._restore()
        try:
            if etype is None:
                self.verify()
        finally:
            self.allocations = []          # the bases go with the context
        return False

    # ---- checks -----------------------------------------------------------------------------------------------------------------------
    def verify(self):
        """Every band of every allocation still holds the pattern: one device-side comparison per allocation, one host sync in total (the
        offsets of a dirty band are fetched only once something is known to be wrong)."""
        if not self.allocations:
            return
        pat2 = torch.cat([self._pat, self._pat])
        flags = []
        for al in self.allocations:
            o, n = al.offset, al.nbytes
            flags.append((torch.cat([al.base[o - BAND:o], al.base[o + n:o + n + BAND]]) != pat2).any())
        dirty = torch.stack(flags).cpu().nonzero().flatten().tolist()
        if not dirty:
            return
        lines = []
        for i in dirty:
            al = self.allocations[i]
            o, n = al.offset, al.nbytes
            for name, band, first_at in (("front", al.base[o - BAND:o], -BAND - n), ("back", al.base[o + n:o + n + BAND], 0)):
                bad = (band != self._pat).nonzero().flatten()
                if bad.numel():
                    lo, hi = int(bad[0]) + first_at, int(bad[-1]) + first_at
                    lines.append(f"{name} band of allocation #{i} dirty: {bad.numel()} byte(s), first at {lo:+d}, last at {hi:+d} relative to the "
                                 f"buffer's end (buffer = {n} bytes): {al!r}")
        raise AssertionError("a kernel wrote outside its buffer:\n  " + "\n  ".join(lines))

    def records(self):
        return [al.record() for al in self.allocations]

    def find(self, nbytes, dtype=None):
        """The recorded allocation(s) of that byte size (and dtype), in allocation order."""
        return [al for al in self.allocations if al.nbytes == int(nbytes) and (dtype is None or al.dtype == dtype)]

    def owner(self, tensor):
        """The allocation `tensor` (a view of a guarded tensor) starts in, or None."""
        p = tensor.data_ptr()
        for al in self.allocations:
            q = al.tensor.data_ptr()
            if q == p and al.nbytes >= tensor.numel() * tensor.element_size() and al.tensor.device == tensor.device:
                return al
        return None


def check_extents(total_bytes, regions, name="buffer"):
    """The layout alone, before anything is launched with it: the used extents [offset, offset + used_bytes) lie inside total_bytes and none
    runs into the region behind it."""
    total = int(total_bytes)
    ordered = sorted((int(o), int(u)) for o, u in regions if int(u) > 0)
    for (a, ua), (b, _ub) in zip(ordered, ordered[1:]):
        assert a + ua <= b, (f"{name}: the region at offset {a} is used up to {a + ua}, {a + ua - b} byte(s) into the region at offset {b} "
                             f"({b - total:+d} relative to the buffer's end, {total} bytes): the layout is too small for what it describes")
    for off, used in regions:
        off, used = int(off), int(used)
        assert 0 <= off and off + used <= total, f"{name}: region [{off}, {off + used}) does not fit the {total} bytes of the buffer"


def check_regions(buffer, fill, regions, name="buffer"):
    """buffer: a guarded allocation (or a uint8 tensor) that started as the byte `fill`; regions: (offset, used_bytes) pairs from a published
    layout struct.  Every byte outside all [offset, offset + used_bytes) must still equal `fill`: those bytes are the padding align_up adds
    between the regions and behind the last one."""
    if isinstance(buffer, Allocation):
        name = f"{name} ({buffer!r})"
        buffer = buffer.bytes()
    raw = buffer.detach().reshape(-1).view(torch.uint8)
    padding = torch.ones(raw.numel(), dtype=torch.bool, device=raw.device)
    check_extents(raw.numel(), regions, name)
    for off, used in regions:
        padding[int(off):int(off) + int(used)] = False
    bad = (padding & (raw != int(fill))).nonzero().flatten()
    if bad.numel():
        first, last = int(bad[0]), int(bad[-1])
        starts = sorted(int(o) for o, _ in regions)
        before = [o for o in starts if o <= first]
        raise AssertionError(f"{name}: {bad.numel()} padding byte(s) written, first at offset {first}, last at {last} "
                             f"({first - raw.numel():+d} / {last - raw.numel():+d} relative to the buffer's end, {raw.numel()} bytes); "
                             f"the region in front starts at {before[-1] if before else None}; regions (offset, used): {sorted((int(o), int(u)) for o, u in regions)}")
    return int(padding.sum())


class unchanged:
    """`with unchanged(tensors):` -- the `const` inputs of a call are byte for byte what they were (compared through uint8, so that NaN
    equals NaN).  tensors: a dict name -> tensor (None entries are skipped) or a list."""

    def __init__(self, tensors):
        items = tensors.items() if isinstance(tensors, dict) else enumerate(tensors)
        self.tensors = [(str(k), t) for k, t in items if t is not None]

    @staticmethod
    def _raw(t):
        t = t.detach()
        base = torch._C.TensorBase           # (the unpatched methods: the snapshots are the harness's own and need no bands)
        return base.contiguous(t).reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1)

    def __enter__(self):
        self.before = [torch._C.TensorBase.clone(self._raw(t)) for _, t in self.tensors]
        return self

    def __exit__(self, etype, exc, tb):
        if etype is None:
            for (name, t), b in zip(self.tensors, self.before):
                now = self._raw(t)
                assert now.shape == b.shape, f"const input {name}: size changed"
                if not torch.equal(now, b):
                    bad = (now != b).nonzero().flatten()
                    raise AssertionError(f"const input {name} was written: {bad.numel()} byte(s), first at byte {int(bad[0])}, last at byte {int(bad[-1])} of {b.numel()}")
        return False
