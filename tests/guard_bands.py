"""Guard bands: every buffer a call is given sits between two bands of a known byte, and the bands are read back afterwards.

A plain helper module like tests/gpu_support.py (no test imports a test).  The caching allocator packs blocks next to each
other, so a kernel that stores one row past the end of its workspace, an output, `packed_grad`, the flat gradient buffer or
an input gradient lands in mapped memory that belongs to some other tensor: nothing faults and every parity test stays
green.  Under `guarded()` that memory is the test's own, and it is checked.

    with GB.guarded() as bands:
        rays = GB.guard(rays)                 # inputs the test itself made
        out = renderer.render_rnb(rays, ...)  # every torch.empty / zeros / full / ones ... of the package is re-homed
        loss.backward()
        torch.cuda.synchronize()
        GB.assert_intact("case")              # both bands of every allocation still hold the pattern
        assert GB.seen(nbytes=ws_bytes)       # positive control: the workspace did go through the bands

What is replaced, as the poison tests of tests/test_gpu_parity.py replace torch.empty: torch.empty, empty_like, zeros,
zeros_like, full, full_like, and the two other allocators the package calls on the device, torch.ones (mesh_clean.py,
fields.py) and torch.ones_like (camera_refine.py).  (torch.arange / tensor / as_tensor / linspace / rand* results in the
package are inputs of torch ops or read-only kernel inputs made from host data, never a kernel's output; Tensor.new_full
appears once, on the host-side box of mesh_simplify.py.)

Each device result of n bytes is re-homed in ONE uint8 allocation of G + n + pad + G bytes (pad < 512 rounds the total to
the allocator's 512-byte granule and counts as part of the trailing band: it is filled and checked like it), the body
returned as big[G:G+n].view(dtype).view(shape).  G is a multiple of 512, so the body keeps the allocator's 512-byte
alignment and the kernels' 16-byte accesses see nothing new.  zeros / full / ones contents are copied in.  CPU tensors,
zero-byte tensors, non-contiguous results and results that require grad pass through untouched.

Band width.  G = 1 MiB.  The widest thing a kernel can spill is one padded tile: kRowPad = 128 rows (rnb_internal.h) of the
widest per-point row the library writes into caller memory.  That row is 320 fp32 = 1280 bytes: a row of the albedo input
`cin` / its adjoint `cinb` in the workspace (layout.hip carve_points: Cinp = pad32(256 + 54) for the shipped shape; the
widest state row of an SDF network the suite builds is w288's, 288 fp32); the widest row of an OUTPUT is feat_out /
feat_bar, 256 fp32 = 1024 bytes (include/rnbneus.h rnb_sdf_forward_save, rnb_color_backward).  One tile of it is
128 x 1280 = 163,840 bytes, and 1 MiB is 6.4 x that.  A store further than G from the buffer it belongs to is OUTSIDE what
these tests promise; so is a read of a band whose value is masked before it reaches a result (the bands read as NaN in every
float type and -1 in every integer type, and a result only changes if the value read is used).

Bodies.  What torch.empty / empty_like hand out holds the pattern too (`poison_bodies`, on by default).  Without that the
body of a guarded buffer would hold whatever the caching allocator's last owner of the block left there - more often
than not the 0xFF of an earlier test's bands - and a kernel that reads a word of its workspace it never wrote would
change a result in one run of the suite and not in the next.  With it such a read always reads NaN: the guarded run
is at the same time the poison test of tests/test_gpu_parity.py test_uninitialised_workspace_is_never_read, on every shape.

`guarded(shortchange=(shape, nbytes))` is the detector's own positive control: the first allocator result (not a guard()ed
input) of that shape keeps its allocation and its view, but its body counts as `nbytes` shorter, so the kernel's last
store lands in the first bytes of what is now the trailing band - memory this module owns.
"""
from __future__ import annotations

import sys
from contextlib import contextmanager

import torch

G_BYTES = 1 << 20
GRANULE = 512
PATCHED = ("empty", "empty_like", "zeros", "zeros_like", "full", "full_like", "ones", "ones_like")
_KEEPS_CONTENT = {"zeros", "zeros_like", "full", "full_like", "ones", "ones_like"}

_active = None     # the session inside its `with`
_last = None       # the most recent session: damaged() / seen() stay answerable after the `with` ends


class Entry:
    __slots__ = ("big", "nbytes", "shape", "dtype", "site", "how")

    def __init__(self, big, nbytes, shape, dtype, site, how):
        self.big, self.nbytes, self.shape, self.dtype, self.site, self.how = big, nbytes, tuple(shape), dtype, site, how

    def describe(self):
        return f"{self.how} {list(self.shape)} {str(self.dtype).replace('torch.', '')} ({self.nbytes} B) in {self.site}"


def _is_cuda(t):
    return t.is_cuda


class Session:
    def __init__(self, pattern, is_device, shortchange, band, poison_bodies):
        assert 0 <= pattern <= 255
        assert band > 0 and band % GRANULE == 0, "the band is a multiple of the allocator's 512-byte granule"
        self.pattern, self.is_device, self.band, self.poison_bodies = pattern, is_device, band, poison_bodies
        self.shortchange = shortchange
        self.registry: list[Entry] = []
        self._orig = {}

    # ---- re-homing ----------------------------------------------------------------------------------------------------
    def _rehome(self, t, site, how, keep_content):
        if not isinstance(t, torch.Tensor) or not self.is_device(t):
            return t
        n = t.numel() * t.element_size()
        if n == 0 or not t.is_contiguous() or t.requires_grad:
            return t
        G = self.band
        total = (2 * G + n + GRANULE - 1) // GRANULE * GRANULE
        big = self._orig["empty"](total, dtype=torch.uint8, device=t.device)
        if self.poison_bodies:
            big.fill_(self.pattern)       # the body too: what torch.empty hands out reads as NaN / -1, not as what the
        else:                             # allocator's last owner left there
            big[:G].fill_(self.pattern)
            big[G + n:].fill_(self.pattern)
        body = big[G:G + n].view(t.dtype).view(t.shape)
        if keep_content:
            body.copy_(t)
        body_bytes = n
        if self.shortchange is not None and how != "guard" and tuple(t.shape) == tuple(self.shortchange[0]):
            body_bytes = n - int(self.shortchange[1])
            assert body_bytes > 0
            self.shortchange = None       # one buffer only
            big[G + body_bytes:G + n].fill_(self.pattern)
        self.registry.append(Entry(big, body_bytes, t.shape, t.dtype, site, how))
        return body

    def guard(self, t):
        """an existing tensor (an input the test made) between bands of its own, same bits"""
        if t is None:
            return None
        f = sys._getframe(1)
        if f.f_code.co_name == "guard" and f.f_back is not None:    # (the module-level guard())
            f = f.f_back
        if not t.requires_grad:
            return self._rehome(t, f.f_code.co_name, "guard", True)
        d = t.detach()
        body = self._rehome(d, f.f_code.co_name, "guard", True)     # a leaf that requires grad stays one
        return t if body is d else body.requires_grad_(True)

    def _wrap(self, name):
        orig = self._orig[name]
        keep = name in _KEEPS_CONTENT

        def alloc(*a, **k):
            t = orig(*a, **k)
            if k.get("out") is not None:
                return t
            f = sys._getframe(1)
            site = f"{f.f_code.co_name} ({f.f_code.co_filename.rsplit('/', 1)[-1]}:{f.f_lineno})"
            return self._rehome(t, site, "torch." + name, keep)

        alloc.__name__ = name
        return alloc

    def install(self):
        for name in PATCHED:
            self._orig[name] = getattr(torch, name)
        for name in PATCHED:
            setattr(torch, name, self._wrap(name))

    def restore(self):
        for name, f in self._orig.items():
            setattr(torch, name, f)

    # ---- reading the bands back -----------------------------------------------------------------------------------------
    def _bands(self, e):
        return (("leading", e.big[:self.band], -self.band), ("trailing", e.big[self.band + e.nbytes:], e.nbytes))

    def damaged(self):
        """[{band, first, last, shape, dtype, site, nbytes, how}]: `first` / `last` are the first and last changed byte
        relative to the body's first byte (leading band: negative; trailing band: >= the body's size, so first - nbytes is
        the distance past the end)."""
        if not self.registry:
            return []
        flags = []
        for e in self.registry:
            for _, band, _ in self._bands(e):
                flags.append(band.ne(self.pattern).any())
        by_dev = {}
        for i, f in enumerate(flags):
            by_dev.setdefault(f.device, []).append((i, f))
        hit = set()
        for dev, lst in by_dev.items():
            got = torch.stack([f for _, f in lst]).cpu().tolist()      # one synchronisation per device
            hit.update(i for (i, _), g in zip(lst, got) if g)
        out = []
        for j, e in enumerate(self.registry):
            for b, (name, band, base) in enumerate(self._bands(e)):
                if 2 * j + b in hit:
                    idx = band.ne(self.pattern).nonzero().flatten()
                    out.append(dict(band=name, first=base + int(idx[0]), last=base + int(idx[-1]), shape=e.shape,
                                    dtype=e.dtype, site=e.site, nbytes=e.nbytes, how=e.how))
        return out

    def assert_intact(self, tag):
        bad = self.damaged()
        if bad:
            lines = [f"  {d['band']} band of {d['how']} {list(d['shape'])} {d['dtype']} ({d['nbytes']} B) allocated in "
                     f"{d['site']}: bytes {d['first']} .. {d['last']} relative to the body" for d in bad]
            raise AssertionError(f"{tag}: {len(bad)} guard band(s) were written to "
                                 f"({len(self.registry)} guarded allocations):\n" + "\n".join(lines))

    def seen(self, shape=None, dtype=None, nbytes=None):
        """the registry entries of that shape / dtype / size in bytes (positive controls: a list, empty when none)"""
        out = []
        for e in self.registry:
            if shape is not None and tuple(shape) != e.shape:
                continue
            if dtype is not None and dtype != e.dtype:
                continue
            if nbytes is not None and int(nbytes) != e.nbytes:
                continue
            out.append(e)
        return out


@contextmanager
def guarded(pattern=0xFF, *, shortchange=None, is_device=_is_cuda, band=G_BYTES, poison_bodies=True):
    """Replace the allocators of PATCHED for the duration; yields the Session (registry, damaged, assert_intact, seen).
    `is_device`: which tensors are re-homed (the host test passes `lambda t: True` to run the helper on CPU tensors).
    `poison_bodies`: torch.empty / empty_like results hold the pattern as well (see the module docstring)."""
    global _active, _last
    if _active is not None:
        raise RuntimeError("guard_bands.guarded() is already active: nested use would re-home the bands themselves")
    s = Session(pattern, is_device, shortchange, band, poison_bodies)
    s.install()
    _active = _last = s
    try:
        yield s
    finally:
        s.restore()
        _active = None


def _session():
    s = _active or _last
    if s is None:
        raise RuntimeError("guard_bands: no guarded() session yet")
    return s


def guard(t):
    if _active is None:
        raise RuntimeError("guard_bands.guard() outside guarded()")
    return _active.guard(t)


def damaged():
    return _session().damaged()


def assert_intact(tag):
    _session().assert_intact(tag)


def seen(shape=None, dtype=None, nbytes=None):
    return _session().seen(shape, dtype, nbytes)


def flatten(x, prefix="result"):
    """{name: tensor} of every tensor (numpy arrays and numbers become tensors) in nested dicts / lists / tuples"""
    out = {}
    if x is None:
        return out
    if isinstance(x, torch.Tensor):
        out[prefix] = x.detach()
    elif isinstance(x, dict):
        for k, v in x.items():
            out.update(flatten(v, f"{prefix}.{k}"))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            out.update(flatten(v, f"{prefix}[{i}]"))
    elif isinstance(x, (bool, int, float)):
        out[prefix] = torch.tensor(x)
    elif hasattr(x, "__array__"):
        import numpy as np
        out[prefix] = torch.from_numpy(np.ascontiguousarray(x))
    elif isinstance(x, str):
        pass
    else:
        raise TypeError(f"{prefix}: {type(x).__name__} is not something flatten() compares")
    return out


def same_bits(a, b):
    """equal shapes, dtypes and BITS (NaN equals the same NaN: torch.equal would not say so)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    if a.numel() == 0:
        return True
    if a.dtype == torch.bool:
        return torch.equal(a, b)
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def assert_same(tag, clean, got, reproducible=True):
    """every tensor of `got` (the guarded run) against `clean` (the same call on ordinary allocations): bit for bit, or,
    for a call that is not reproducible between two runs of its own, finite exactly where the clean run is finite"""
    a, b = flatten(clean), flatten(got)
    assert sorted(a) == sorted(b), f"{tag}: the guarded run returned other things: {sorted(set(a) ^ set(b))}"
    for k in a:
        x, y = a[k].cpu(), b[k].cpu()
        assert x.shape == y.shape and x.dtype == y.dtype, f"{tag}: {k}: {tuple(y.shape)} {y.dtype}, was {tuple(x.shape)} {x.dtype}"
        if reproducible or not x.dtype.is_floating_point:
            if not same_bits(x, y):
                diff = (x != y) & ~((x != x) & (y != y)) if x.dtype.is_floating_point else (x != y)
                n = int(diff.sum())
                first = int(diff.reshape(-1).nonzero()[0]) if n else -1
                raise AssertionError(f"{tag}: {k} differs from the unguarded run in {n} of {x.numel()} elements (first at flat "
                                     f"index {first}; NaNs: {int((y != y).sum())} guarded, {int((x != x).sum())} unguarded)")
        else:
            assert torch.equal(torch.isfinite(x), torch.isfinite(y)), \
                f"{tag}: {k} is finite in other places than in the unguarded run ({int((~torch.isfinite(y)).sum())} " \
                f"non-finite guarded, {int((~torch.isfinite(x)).sum())} unguarded)"


def release():
    """drop the last session's allocations (a module-level registry would otherwise keep them to the next guarded())"""
    global _last
    if _last is not None and _last is not _active:
        _last.registry.clear()
        _last = None
