"""A poisoned, guarded torch.empty (test infrastructure).

The library allocates every output and scratch buffer with torch.empty / torch.empty_like / Tensor.new_empty and relies on one invariant:
every byte that is read, on the device or by the caller, was written by this call first.  `poisoned(word)` makes
that testable: for its duration those three names return memory filled with a chosen 32-bit word, with a 4096-byte guard of the same
word on either side, so that

  * a result that depends on what the memory held before differs between two words, and
  * a store just outside an allocation lands in a guard, which check_guards() reads back, and not in the allocator's neighbouring block.

Three words are needed, because comparisons hide some poisons: ZERO is what fresh device pages hold (the baseline), SENTINEL is a payload
NaN that poisons every float sum it enters, and ONE is 1.0f as a float and a large finite integer: a NaN compares false, so an
`if (g != g) g = 0` or an `alpha < 1/255` reject drops it, a 1.0 passes.
"""
import contextlib

import numpy as np
import torch

ZERO = 0x00000000
SENTINEL = 0x7FC12345   # the payload NaN of test_gpu_adam*.py
ONE = 0x3F800000
PATTERNS = (("ZERO", ZERO), ("SENTINEL", SENTINEL), ("ONE", ONE))   # ZERO first: the baseline runs before a dirty pattern does
GUARD = 4096            # bytes on either side; a multiple of the caching allocator's 512-byte alignment

_REAL = dict(empty=torch.empty, empty_like=torch.empty_like, new_empty=torch.Tensor.new_empty)


class Poison:
    """The allocations made under one `poisoned` block: (raw uint8 block, nbytes of the tensor handed out) each."""

    def __init__(self, word, device_type):
        self.word, self.device_type, self.allocations = int(word) & 0xFFFFFFFF, device_type, []

    def alloc(self, shape, dtype, device, requires_grad=False):
        shape = torch.Size(shape)
        nbytes = shape.numel() * _REAL["empty"]((), dtype=dtype).element_size()
        body = (nbytes + 3) // 4 * 4
        raw = _REAL["empty"](GUARD + body + GUARD, dtype=torch.uint8, device=device)
        raw.view(torch.int32).fill_(int(np.uint32(self.word).view(np.int32)))
        self.allocations.append((raw, nbytes))
        out = raw[GUARD:GUARD + nbytes].view(dtype).view(shape)
        return out.requires_grad_() if requires_grad else out

    def check_guards(self):
        """Every guard word of every allocation still holds the pattern.  The tail guard starts at the 4-byte boundary after the tensor:
        the up to 3 bytes of padding before it belong to nobody and are not checked."""
        want = int(np.uint32(self.word).view(np.int32))
        for k, (raw, nbytes) in enumerate(self.allocations):
            body = (nbytes + 3) // 4 * 4
            words = raw.view(torch.int32)
            for name, part in (("front", words[:GUARD // 4]), ("back", words[(GUARD + body) // 4:])):
                bad = (part != want).nonzero()
                assert bad.numel() == 0, (f"allocation #{k} of {len(self.allocations)} ({nbytes} bytes): {name} guard overwritten, first at "
                                          f"word {int(bad[0])}: {int(part[int(bad[0])]) & 0xFFFFFFFF:#010x} != {self.word:#010x}")


def _plain(p, dtype, device, kwargs):
    """(dtype, device) if the poisoned allocation applies: strided, contiguous, not pinned, no out=, on p.device_type."""
    if kwargs.get("out") is not None or kwargs.get("pin_memory") or kwargs.get("layout", torch.strided) is not torch.strided:
        return None
    if kwargs.get("memory_format", torch.contiguous_format) is not torch.contiguous_format:
        return None
    if kwargs.get("names") is not None:
        return None
    dtype = torch.get_default_dtype() if dtype is None else dtype
    device = torch.device(torch.get_default_device() if device is None else device)
    if device.type != p.device_type or dtype.is_complex or getattr(dtype, "is_quantized", False):
        return None
    return dtype, device


def _size(args, kwargs):
    if "size" in kwargs:
        return kwargs["size"]
    if len(args) == 1 and not isinstance(args[0], int):
        return args[0]
    return args


@contextlib.contextmanager
def poisoned(word, device_type="cuda"):
    """torch.empty, torch.empty_like and Tensor.new_empty hand out `word`-filled, guarded memory on `device_type`; yields the Poison, whose
    check_guards() also runs when the block ends without an exception."""
    p = Poison(word, device_type)

    def empty(*args, **kwargs):
        ok = _plain(p, kwargs.get("dtype"), kwargs.get("device"), kwargs)
        if ok is None:
            return _REAL["empty"](*args, **kwargs)
        return p.alloc(_size(args, kwargs), *ok, requires_grad=kwargs.get("requires_grad", False))

    def empty_like(t, **kwargs):
        fmt = kwargs.get("memory_format", torch.preserve_format)
        dense = t.layout is torch.strided and t.is_contiguous() and fmt in (torch.preserve_format, torch.contiguous_format)
        kw = {k: v for k, v in kwargs.items() if k != "memory_format"}
        kw.setdefault("layout", t.layout)
        ok = _plain(p, kwargs.get("dtype") or t.dtype, kwargs.get("device") or t.device, kw) if dense else None
        if ok is None:
            return _REAL["empty_like"](t, **kwargs)
        return p.alloc(t.shape, *ok, requires_grad=kwargs.get("requires_grad", False))

    def new_empty(t, *args, **kwargs):
        ok = _plain(p, kwargs.get("dtype") or t.dtype, kwargs.get("device") or t.device, kwargs)
        if ok is None:
            return _REAL["new_empty"](t, *args, **kwargs)
        return p.alloc(_size(args, kwargs), *ok, requires_grad=kwargs.get("requires_grad", False))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield p
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = _REAL["empty"], _REAL["empty_like"], _REAL["new_empty"]
    p.check_guards()


def run_all(fn):
    """fn() unpatched, then under ZERO, SENTINEL and ONE, guards checked after each: [(label, result)], the unpatched run first."""
    runs = [("unpatched", fn())]
    for name, word in PATTERNS:
        with poisoned(word) as p:
            out = fn()
            if p.device_type == "cuda":
                torch.cuda.synchronize()
            p.check_guards()
        runs.append((name, out))
    return runs


def flatten(x, prefix=""):
    """A result (tensor, array, scalar, None, or a dict / list / tuple of these) as {path: value}."""
    if isinstance(x, dict):
        return {k2: v for k, c in x.items() for k2, v in flatten(c, f"{prefix}.{k}" if prefix else str(k)).items()}
    if isinstance(x, (list, tuple)):
        return {k2: v for k, c in enumerate(x) for k2, v in flatten(c, f"{prefix}[{k}]").items()}
    return {prefix: x}


def raw_bytes(v):
    """Tensor or array -> its bytes as a uint8 numpy array: the comparison is of bits, so NaN == NaN and -0 != 0."""
    if torch.is_tensor(v):
        v = v.detach().contiguous().cpu().reshape(-1)          # (flat first: a 0-dim tensor cannot change its element size in a view)
        return v.view(torch.uint8).numpy() if v.numel() else np.zeros(0, np.uint8)
    return np.ascontiguousarray(v).reshape(-1).view(np.uint8)


def assert_identical(runs, what=""):
    """Every leaf of every run is bit-identical with the first (unpatched) run's, same paths, shapes and dtypes included."""
    base_name, base = runs[0][0], flatten(runs[0][1])
    assert any(torch.is_tensor(v) or isinstance(v, np.ndarray) for v in base.values()), f"{what}: nothing to compare"
    for name, out in runs[1:]:
        got = flatten(out)
        assert got.keys() == base.keys(), (what, name, sorted(got.keys() ^ base.keys()))
        for path, b in base.items():
            g = got[path]
            if torch.is_tensor(b) or isinstance(b, np.ndarray):
                assert type(g) is type(b) and g.shape == b.shape and g.dtype == b.dtype, (what, name, path)
                rb, rg = raw_bytes(b), raw_bytes(g)
                if not np.array_equal(rb, rg):
                    diff = np.flatnonzero(rb != rg)
                    item = b.element_size() if torch.is_tensor(b) else b.itemsize
                    raise AssertionError(f"{what}: {path} differs between {base_name} and {name}: {len(np.unique(diff // item))} of "
                                         f"{rb.size // item} elements, first at flat index {int(diff[0]) // item}")
            else:
                assert g == b, (what, name, path, b, g)
